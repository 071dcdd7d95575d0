"""GPU tests of lft_lf_prepare and the data-preparation paths built on it (lft_amd.prepare, tools/prepare_data.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from lft_amd import _lib, datasets, evaluate, prepare, trainer
from lft_amd._lib import LftError

from prepare_util import make_datasets_tree, prepare_np, ulp_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def g(golden_dir):
    return {k: np.load(os.path.join(golden_dir, f"prepare_{k}.npz")) for k in ("views", "grid")}


def _run(lf, A, s, crops, ch, cw):
    hr, lr = prepare.lf_prepare(torch.from_numpy(np.array(lf, order="K")).to(DEV), A, s, crops, ch, cw)
    torch.cuda.synchronize()
    return hr.cpu().numpy(), lr.cpu().numpy()


def _close(got, ref, what, stats):
    assert got.shape == ref.shape, what
    d = ulp_diff(got, ref)
    assert d.max() <= 1, (what, int(d.max()), int((d > 1).sum()))
    stats[0] += int((d == 0).sum())
    stats[1] += d.size


def test_fixture_views_every_class(g):
    v = g["views"]
    names = sorted({k[:-5] for k in v.files if k.endswith("_meta")})
    stats = [0, 0]
    for name in names:
        A, s = (int(x) for x in v[name + "_meta"])
        base = v[name + "_lf"]
        for cls in (np.uint8, np.float32, np.float64):
            if base.dtype == np.float64 and cls == np.uint8:
                continue
            lf = base.astype(cls)
            ref_hr, ref_lr = (v[name + "_hr"], v[name + "_lr"]) if cls == base.dtype else prepare_np(lf, A, s, [(0, 0)], *lf.shape[2:4])
            ref_hr, ref_lr = np.asarray(ref_hr).reshape(1, *np.shape(ref_hr)[-2:]), np.asarray(ref_lr).reshape(1, *np.shape(ref_lr)[-2:])
            hr, lr = _run(lf, A, s, [(0, 0)], lf.shape[2], lf.shape[3])
            _close(hr, ref_hr, (name, cls), stats)
            _close(lr, ref_lr, (name, cls), stats)
            # the kernel against the restatement: the same sums in the same order
            nh, nl = prepare_np(lf, A, s, [(0, 0)], lf.shape[2], lf.shape[3])
            assert ulp_diff(hr, nh).max() <= 1 and ulp_diff(lr, nl).max() <= 1
    print(f"lft_lf_prepare vs fixtures: {stats[0] / stats[1]:.6f} of {stats[1]} values bit-identical")
    assert stats[0] / stats[1] > 0.99


def test_fixture_grid_and_v73_layout(g, golden_dir):
    gr = g["grid"]
    A, s = (int(x) for x in gr["meta"])
    hr, lr = _run(gr["lf"], A, s, gr["origins"], 32 * s, 32 * s)
    stats = [0, 0]
    _close(hr, gr["hr"], "grid hr", stats)
    _close(lr, gr["lr"], "grid lr", stats)
    # a v7.3 file's reversed array, read through its strides, gives what the C-order copy gives
    lf = prepare.load_lf(os.path.join(golden_dir, "prepare_lf_v73.mat"))
    assert not lf.flags.c_contiguous
    t = torch.from_numpy(lf.base if lf.base is not None else lf).to(DEV).permute(4, 3, 2, 1, 0)
    h1, l1 = prepare.lf_prepare(t, 3, 2, [(0, 0), (1, 2)], 8, 5)
    h2, l2 = _run(np.ascontiguousarray(lf), 3, 2, [(0, 0), (1, 2)], 8, 5)
    assert torch.equal(h1.cpu(), torch.from_numpy(h2)) and torch.equal(l1.cpu(), torch.from_numpy(l2))


def test_large_cases_match_restatement():
    rng = np.random.default_rng(9)
    lf = np.round(rng.random((9, 9, 203, 266, 3)) * 255).astype(np.uint8)
    A, s = 5, 4
    t = prepare.to_device(lf, A, DEV)
    lr, hr = prepare.test_pair(t, A, s)
    assert tuple(hr.shape) == (5 * 200, 5 * 264) and tuple(lr.shape) == (5 * 50, 5 * 66)
    nh, nl = prepare_np(lf, A, s, [(0, 0)], 200, 264)
    stats = [0, 0]
    _close(hr.cpu().numpy()[None], nh, "test hr", stats)
    _close(lr.cpu().numpy()[None], nl, "test lr", stats)
    lr2, hr2 = prepare.training_pairs(t, A, s)
    crops = prepare.patch_grid(203, 266, s)
    assert len(crops) == 6                                         # 2 x 3 patches of 128, stride 64
    nh, nl = prepare_np(lf, A, s, crops, 128, 128)
    _close(hr2.cpu().numpy(), nh, "grid hr", stats)
    _close(lr2.cpu().numpy(), nl, "grid lr", stats)
    print(f"large cases: {stats[0] / stats[1]:.6f} bit-identical to the restatement")
    # deterministic: a second launch gives the same bits
    lr3, hr3 = prepare.training_pairs(t, A, s)
    assert torch.equal(lr2, lr3) and torch.equal(hr2, hr3)
    lr4, hr4 = prepare.test_pair(t, A, s)
    assert torch.equal(lr4, lr) and torch.equal(hr4, hr)


def test_prepare_fallback_path_gives_the_same_bits():
    """The true tables never span more than the staged region (kPrepSpan = 56 rows / columns per 32 x 32 HR tile), so the
    fall-back is forced through the C ABI, as test_gpu_colour.py::test_merge_fallback_path_gives_the_same_bits does for the colour
    path: one more tap of weight 0 that points to the far end of the crop widens every tile's span past the region and adds
    0 * y = 0 to each sum (Y is at least 16/255, so no partial sum changes).  The far end is the end farther from the output's
    own taps: with 'the last column for taps that start below 56, else column 0' the middle tile of 80 columns at s = 4 would
    span 54 and stay staged.  A = 2 needs an even number of spare views, so the centre 2 x 2 of 4 x 4 views are taken."""
    SPAN, MAX_TAPS, TILE_HR = 56, 18, 32                                    # kPrepSpan, kPrepMaxTaps, kPrepTileHr of lft_prepare.cuh
    A, H, W = 2, 96, 80
    lf = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (4, 4, H, W, 3)).astype(np.uint8)).to(DEV)
    crop = np.zeros((1, 2), dtype=np.int32)

    def tables(L, s, far):
        w, i = prepare.contributions(L, s)                                  # all-zero columns already dropped
        if far:
            end = np.where(L - 1 - i.min(axis=1) >= i.max(axis=1), L - 1, 0).astype(np.int32)
            w = np.concatenate([w, np.zeros((w.shape[0], 1))], axis=1)
            i = np.concatenate([i, end[:, None]], axis=1)
            assert w.shape[1] <= MAX_TAPS
            TO = TILE_HR // s
            spans = [int(i[o:o + TO].max() - i[o:o + TO].min() + 1) for o in range(0, i.shape[0], TO)]
            assert min(spans) > SPAN, (L, s, spans)                         # every tile leaves the staged region
        return torch.from_numpy(np.ascontiguousarray(w)).to(DEV), torch.from_numpy(np.ascontiguousarray(i)).to(DEV)

    def run(s, far_h, far_w):
        (wh, ih), (ww, iw) = tables(H, s, far_h), tables(W, s, far_w)
        hr = torch.zeros(1, A * H, A * W, device=DEV)
        lr = torch.zeros(1, A * wh.shape[0], A * ww.shape[0], device=DEV)
        _lib.enqueue("lft_lf_prepare", DEV, *prepare.lf_args(lf), A, s, crop.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, H, W,
                     wh.data_ptr(), ih.data_ptr(), wh.shape[1], ww.data_ptr(), iw.data_ptr(), ww.shape[1], hr.data_ptr(), lr.data_ptr())
        torch.cuda.synchronize()
        return hr, lr

    for s in (2, 4):
        want_hr, want_lr = run(s, False, False)
        got = prepare.lf_prepare(lf, A, s, [(0, 0)], H, W)
        assert torch.equal(got[0], want_hr) and torch.equal(got[1], want_lr)
        assert float(want_hr.min()) >= 0.0627 and float(want_lr.std()) > 0.0    # Y >= 16/255; the call computed something
        for far_h, far_w in ((True, True), (True, False), (False, True)):      # neither stage fits | rows only | columns only
            hr, lr = run(s, far_h, far_w)
            assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr), (s, far_h, far_w)


def test_argument_errors_enqueue_nothing():
    lf = torch.zeros(5, 5, 8, 8, 3, dtype=torch.uint8, device=DEV)
    w, i = prepare._device_table(8, 2, DEV)
    hr = torch.full((1, 3 * 8, 3 * 8), -7.0, device=DEV)
    lr = torch.full((1, 3 * 4, 3 * 4), -7.0, device=DEV)
    st = _lib.strides_array(lf)

    def call(lfp=lf.data_ptr(), cls=_lib.LF_UINT8, U=5, V=5, A=3, s=2, crops=((0, 0),), ch=8, cw=8, hrp=hr.data_ptr(), strides=st):
        c = np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 2))
        _lib.enqueue("lft_lf_prepare", DEV, lfp, cls, U, V, 8, 8, 3, strides, A, s, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), c.shape[0], ch, cw,
                     w.data_ptr(), i.data_ptr(), w.shape[1], w.data_ptr(), i.data_ptr(), w.shape[1], hrp, lr.data_ptr())

    bad = [dict(U=6, A=3), dict(V=4, A=3), dict(A=7), dict(s=3), dict(s=1), dict(crops=((1, 0),)), dict(crops=((0, -1),)),
           dict(crops=((0, 0), (0, 4)), ch=8, cw=5), dict(cls=3), dict(cls=-1), dict(lfp=None), dict(hrp=None), dict(strides=None)]
    for kw in bad:
        with pytest.raises(LftError, match="lft_lf_prepare"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((hr == -7.0).all()) and bool((lr == -7.0).all())           # nothing ran
    with pytest.raises(LftError):
        prepare.lf_prepare(lf.to(torch.int16), 3, 2, [(0, 0)], 8, 8)
    with pytest.raises(LftError):
        prepare.lf_prepare(lf.cpu(), 3, 2, [(0, 0)], 8, 8)
    call()                                                                   # the good call runs
    torch.cuda.synchronize()
    assert bool((hr != -7.0).all())


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("prep")
    src = str(root / "datasets") + "/"
    lfs = make_datasets_tree(src)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prepare_data
    A, s = 5, 2
    wtr = prepare_data.run("train", A, s, src, str(root / "data_for_train") + "/", DEV, log=lambda *a: None)
    wte = prepare_data.run("test", A, s, src, str(root / "data_for_test") + "/", DEV, log=lambda *a: None)
    return dict(src=src, lfs=lfs, A=A, s=s, train=str(root / "data_for_train") + "/", test=str(root / "data_for_test") + "/",
                wtr=wtr, wte=wte)


def test_tool_trees_match_restatement(tree):
    A, s = tree["A"], tree["s"]
    plan = prepare.training_plan(tree["src"], A, s)
    assert tree["wtr"] == {"EPFL": 4, "HCI_new": 7} and tree["wte"] == {"EPFL": 2, "HCI_new": 1}
    src = datasets.H5PatchSource(tree["train"], A, s)
    assert src.file_list == [f"{d}/{f}" for d, f, _, _, _ in plan]
    stats = [0, 0]
    for k, (d, _, scene, y0, x0) in enumerate(plan):
        lf = tree["lfs"][(d, "training", scene)]
        nh, nl = prepare_np(lf, A, s, [(y0, x0)], 32 * s, 32 * s)
        lr, hr = src.get([k])
        _close(lr[0, 0].numpy().T[None], nl, ("train", k), stats)              # the training loader sees the transpose
        _close(hr[0, 0].numpy().T[None], nh, ("train", k), stats)
    args = type("Args", (), dict(path_for_test=tree["test"], angRes=A, scale_factor=s))
    names, loaders, n = datasets.MultiTestSetDataLoader(args)
    assert sorted(names) == ["EPFL", "HCI_new"] and n == 3
    for name, loader in zip(names, loaders):
        files = loader.dataset.file_list
        for f, (lr, hr) in zip(files, loader):
            scene = os.path.basename(f)[:-3]
            lf = tree["lfs"][(name, "test", scene)]
            H, W = lf.shape[2] // 4 * 4, lf.shape[3] // 4 * 4
            nh, nl = prepare_np(lf, A, s, [(0, 0)], H, W)
            _close(lr[0, 0].numpy()[None], nl, ("test", scene), stats)
            _close(hr[0, 0].numpy()[None], nh, ("test", scene), stats)
    print(f"written trees vs restatement: {stats[0] / stats[1]:.6f} bit-identical")


def test_raw_source_equals_tree(tree):
    A, s = tree["A"], tree["s"]
    raw = prepare.RawLFPatchSource(tree["src"], A, s, device=DEV)
    h5 = datasets.H5PatchSource(tree["train"], A, s, cache=True)
    assert len(raw) == len(h5) == 11
    for i in range(len(raw)):
        a, b = raw.get([i]), h5.get([i])
        assert torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1].cpu(), b[1]), i
    ix = [10, 0, 3, 3, 7, 5, 1]
    a, b = raw.get(ix), h5.get(ix)
    assert torch.equal(a[0].cpu(), b[0]) and torch.equal(a[1].cpu(), b[1])


def test_fit_same_losses_from_either_source(tree):
    from types import SimpleNamespace

    from lft_amd.params import deterministic_state
    from model import LFT
    A, s = tree["A"], tree["s"]
    losses = []
    for src in (prepare.RawLFPatchSource(tree["src"], A, s, device=DEV), datasets.H5PatchSource(tree["train"], A, s, cache=True)):
        net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=5).items()})
        net = net.to(DEV)
        losses.append(trainer.fit(net, src, epochs=1, batch_size=4, seed=3, log=lambda *a: None))
    assert losses[0] == losses[1], losses


def test_evaluate_raw_scenes_equals_tree(tree):
    from types import SimpleNamespace

    from lft_amd.params import deterministic_state
    from model import LFT
    A, s = tree["A"], tree["s"]
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=6).items()})
    net = net.to(DEV).eval()
    for ds in ("EPFL", "HCI_new"):
        d = os.path.join(tree["test"], f"SR_{A}x{A}_{s}x", ds)
        written = []
        for f in sorted(os.listdir(d)):                                       # the tree's scenes in the raw walk's (sorted) order
            lr, hr = datasets.read_pair(os.path.join(d, f))
            written.append((torch.from_numpy(lr.T.copy()), torch.from_numpy(hr.T.copy())))
        raw = list(prepare.raw_test_scenes(tree["src"], A, s, ds, device=DEV))
        assert len(raw) == len(written)
        for (a, b), (c, e) in zip(raw, written):
            assert torch.equal(a.cpu(), c) and torch.equal(b.cpu(), e)
        assert evaluate.test(net, raw) == evaluate.test(net, written)
