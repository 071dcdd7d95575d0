"""CPU tests of the data preparation (lft_amd.prepare, lft_amd.h5write): contribution tables, the numpy restatement against the
reference-port fixtures, .mat loading, the MATLAB-form writer and the scripts' directory walk / numbering."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from lft_amd import datasets, h5lite, h5write, prepare

from prepare_util import TREE, make_datasets_tree, prepare_np, ulp_diff, write_v73

H5PY = "/opt/conda/bin/python3.9"


@pytest.fixture(scope="module")
def g(golden_dir):
    return {k: np.load(os.path.join(golden_dir, f"prepare_{k}.npz")) for k in ("tables", "views", "grid")}


def test_contributions_bit_identical(g):
    t = g["tables"]
    keys = sorted(k[2:] for k in t.files if k.startswith("w_"))
    assert len(keys) >= 20
    for k in keys:
        L, s = (int(x) for x in k.split("_"))
        w, i = prepare.contributions(L, s)
        assert w.dtype == np.float64 and i.dtype == np.int32
        assert w.shape == t["w_" + k].shape and i.shape == t["i_" + k].shape, k
        assert np.array_equal(w.view(np.uint64), t["w_" + k].view(np.uint64)), k
        assert np.array_equal(i, t["i_" + k]), k
        assert i.min() >= 0 and i.max() < L


def test_contributions_of_axes_shorter_than_the_kernel(golden_dir):
    """Lengths 1, 2, 3 and 5, down and up by 2 and 4: the mirror period 2 * L is shorter than the tap count, so an index wraps more
    than once.  Against tables recorded when prepare.contributions and colour.up_contributions were two separate functions."""
    from lft_amd import colour
    t = np.load(os.path.join(golden_dir, "contributions_short.npz"))
    for L, s, way in ((L, s, way) for L in (1, 2, 3, 5) for s in (2, 4) for way in ("down", "up")):
        w, i = (prepare.contributions if way == "down" else colour.up_contributions)(L, s)
        rw, ri = t[f"{way}_w_{L}_{s}"], t[f"{way}_i_{L}_{s}"]
        assert w.dtype == np.float64 and i.dtype == np.int32 and w.shape == rw.shape and i.shape == ri.shape, (way, L, s)
        assert np.array_equal(w.view(np.uint64), rw.view(np.uint64)) and np.array_equal(i, ri), (way, L, s)
        assert w.shape[0] == (L * s if way == "up" else -(-L // s)) and i.min() >= 0 and i.max() < L


def test_restatement_matches_reference_views(g):
    v = g["views"]
    names = sorted({k[:-5] for k in v.files if k.endswith("_meta")})
    assert len(names) == 8
    same = total = 0
    for name in names:
        A, s = (int(x) for x in v[name + "_meta"])
        lf = v[name + "_lf"]
        hr, lr = prepare_np(lf, A, s, [(0, 0)], lf.shape[2], lf.shape[3])
        for got, ref in ((hr[0], v[name + "_hr"]), (lr[0], v[name + "_lr"])):
            assert got.shape == ref.shape, name
            d = ulp_diff(got, ref)
            assert d.max() <= 1, (name, int(d.max()))
            same += int((d == 0).sum())
            total += d.size
    print(f"restatement vs reference port: {same / total:.6f} of {total} values bit-identical")
    assert same / total > 0.99


def test_restatement_matches_reference_grid(g):
    gr = g["grid"]
    A, s = (int(x) for x in gr["meta"])
    lf = gr["lf"]
    crops = prepare.patch_grid(lf.shape[2], lf.shape[3], s)
    assert np.array_equal(np.array(crops), gr["origins"])
    hr, lr = prepare_np(lf, A, s, crops, 32 * s, 32 * s)
    assert ulp_diff(hr, gr["hr"]).max() <= 1 and ulp_diff(lr, gr["lr"]).max() <= 1


def test_load_lf_v5(tmp_path):
    scipy_io = pytest.importorskip("scipy.io")
    rng = np.random.default_rng(3)
    for cls in (np.uint8, np.float64):
        lf = rng.random((3, 5, 7, 6, 3))
        lf = np.round(lf * 255).astype(np.uint8) if cls == np.uint8 else lf
        p = str(tmp_path / f"lf_{np.dtype(cls).name}.mat")
        scipy_io.savemat(p, {"LF": lf})
        got = prepare.load_lf(p)
        assert got.dtype == cls and got.shape == (3, 5, 7, 6, 3)
        assert np.array_equal(got, lf)


def test_load_lf_v73(golden_dir, g, tmp_path):
    got = prepare.load_lf(os.path.join(golden_dir, "prepare_lf_v73.mat"))
    ref = g["views"]["v73_lf"]
    assert got.dtype == np.uint8 and got.shape == ref.shape == (5, 5, 9, 7, 3)
    assert np.array_equal(got, ref)
    lf = np.random.default_rng(4).random((5, 3, 4, 6, 3)).astype(np.float32)
    p = str(tmp_path / "f32.mat")
    write_v73(p, lf)
    got = prepare.load_lf(p)
    assert got.dtype == np.float32 and np.array_equal(got, lf)


def test_centre_views_refuse_odd():
    lf = np.zeros((6, 5, 2, 2, 3), np.uint8)
    with pytest.raises(prepare.LftError, match="even"):
        prepare.centre_views(lf, 3)
    assert prepare.centre_views(np.zeros((9, 7, 1, 1, 3)), 5) == (2, 1)


def _roundtrip(tmp, name, expected, hr_first):
    lr_s, hr_s = expected[name + ":Lr_SAI_y"], expected[name + ":Hr_SAI_y"]   # as stored (the MATLAB matrix transposed)
    p = os.path.join(tmp, name)
    h5write.write_sai_pair(p, lr_s.T, hr_s.T, hr_first=hr_first)
    lr, hr = datasets.read_pair(p)
    assert lr.dtype == hr.dtype == np.float32
    assert np.array_equal(lr, lr_s) and np.array_equal(hr, hr_s)
    return p


def test_writer_roundtrip(golden_dir, tmp_path):
    e = np.load(os.path.join(golden_dir, "h5", "expected.npz"))
    p = _roundtrip(str(tmp_path), "train_000001.h5", e, False)
    _roundtrip(str(tmp_path), "scene_rect.h5", e, True)
    raw = open(p, "rb").read()
    assert raw[:8] == h5lite.SIGNATURE and raw[8] == 0                          # superblock version 0
    with h5lite.File(p) as hf:
        assert sorted(hf.keys()) == ["Hr_SAI_y", "Lr_SAI_y"]
        for n in hf.keys():
            ds = hf.get(n)
            assert ds._layout["cls"] == 1, ds._layout                          # contiguous
            assert not ds._filters
    # the reference's loader classes over a tree of written files
    args = type("Args", (), dict(path_for_train=str(tmp_path) + "/", path_for_test=str(tmp_path) + "/", angRes=5, scale_factor=2,
                                 data_name="ALL"))
    tr = tmp_path / "SR_5x5_2x" / "D"
    tr.mkdir(parents=True)
    shutil.copy(p, tr / "000001.h5")
    src = datasets.H5PatchSource(str(tmp_path) + "/", 5, 2)
    lr, hr = src.get([0])
    assert np.array_equal(lr[0, 0].numpy(), e["train_000001.h5:Lr_SAI_y"])
    assert np.array_equal(hr[0, 0].numpy(), e["train_000001.h5:Hr_SAI_y"])
    shutil.copy(os.path.join(str(tmp_path), "scene_rect.h5"), tr / "000001.h5")
    lr, hr = datasets.TestSetDataLoader(args, "D")[0]
    assert np.array_equal(lr[0].numpy(), e["scene_rect.h5:Lr_SAI_y"].T)
    assert np.array_equal(hr[0].numpy(), e["scene_rect.h5:Hr_SAI_y"].T)


@pytest.mark.skipif(not os.path.exists(H5PY), reason="no interpreter with h5py on this machine")
def test_writer_read_by_h5py(golden_dir, tmp_path):
    e = np.load(os.path.join(golden_dir, "h5", "expected.npz"))
    p = _roundtrip(str(tmp_path), "scene_rect.h5", e, True)
    code = ("import sys, h5py, numpy as np\n"
            "f = h5py.File(sys.argv[1], 'r')\n"
            "np.savez(sys.argv[2], **{n: np.array(f[n]) for n in f})\n"
            "print(f.libver, [f[n].id.get_create_plist().get_layout() == h5py.h5d.CONTIGUOUS for n in f])\n")
    out = str(tmp_path / "h5py.npz")
    r = subprocess.run([H5PY, "-c", code, p, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "False" not in r.stdout
    got = np.load(out)
    assert np.array_equal(got["Lr_SAI_y"], e["scene_rect.h5:Lr_SAI_y"]) and np.array_equal(got["Hr_SAI_y"], e["scene_rect.h5:Hr_SAI_y"])


def test_patch_grid_worked_example():
    # Training.m:40-41 with patchsize 64, stride 32 (s = 2) over 100 x 130 views: h = 1, 33; w = 1, 33, 65 (1-based)
    assert prepare.patch_grid(100, 130, 2) == [(0, 0), (0, 32), (0, 64), (32, 0), (32, 32), (32, 64)]
    # s = 4: patchsize 128, stride 64 over 128 x 191: h = 1; w = 1, 65 (191 - 128 + 1 = 64 < 65: one column of patches less)
    assert prepare.patch_grid(128, 191, 4) == [(0, 0)]
    assert prepare.patch_grid(128, 192, 4) == [(0, 0), (0, 64)]
    assert prepare.patch_grid(63, 500, 2) == []


def test_directory_walk_and_numbering(tmp_path):
    make_datasets_tree(str(tmp_path))
    (tmp_path / ".hidden").mkdir()
    (tmp_path / "README.txt").write_text("not a dataset")
    (tmp_path / "EPFL" / "training" / "notes.txt").write_text("not a scene")
    assert prepare.list_datasets(str(tmp_path)) == ["EPFL", "HCI_new"]
    assert [n for n, _ in prepare.list_scenes(str(tmp_path), "EPFL", "training")] == ["Bikes", "Flowers"]
    assert [n for n, _ in prepare.list_scenes(str(tmp_path), "HCI_new", "test")] == ["herbs"]
    plan = prepare.training_plan(str(tmp_path), 5, 2)
    # worked out from TREE: Bikes 75 x 101 -> h 1; w 1, 33.  Flowers 97 x 70 -> h 1, 33; w 1.  bedroom 66 x 97 -> h 1; w 1, 33.
    # boxes 70 x 67 -> (1, 1).  dino 99 x 99 -> h 1, 33; w 1, 33.  Numbering restarts at 000001 per dataset.
    assert plan == [("EPFL", "000001.h5", "Bikes", 0, 0), ("EPFL", "000002.h5", "Bikes", 0, 32),
                    ("EPFL", "000003.h5", "Flowers", 0, 0), ("EPFL", "000004.h5", "Flowers", 32, 0),
                    ("HCI_new", "000001.h5", "bedroom", 0, 0), ("HCI_new", "000002.h5", "bedroom", 0, 32),
                    ("HCI_new", "000003.h5", "boxes", 0, 0),
                    ("HCI_new", "000004.h5", "dino", 0, 0), ("HCI_new", "000005.h5", "dino", 0, 32),
                    ("HCI_new", "000006.h5", "dino", 32, 0), ("HCI_new", "000007.h5", "dino", 32, 32)]
    assert len(TREE) == 8
