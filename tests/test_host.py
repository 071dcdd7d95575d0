"""CPU-side tests: plugin surface, state-dict compatibility, C-ABI exports, loud failure without a GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lft_amd import _lib
from lft_amd.params import deterministic_state, num_params, param_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_param_counts():
    assert num_params(64, 2) == 1114240 and num_params(64, 4) == 1163392
    assert len(param_table(64, 2)) == 78


def test_plugin_surface_and_state_dict_roundtrip():
    from model import LFT
    for s in (2, 4):
        net = LFT.get_model(SimpleNamespace(channels=64, angRes=5, scale_factor=s))
        sd = net.state_dict()
        assert list(sd.keys()) == [n for n, _, _ in param_table(64, s)]
        assert all(tuple(sd[n].shape) == sh for n, sh, _ in param_table(64, s))
        ref = {k: torch.from_numpy(v) for k, v in deterministic_state(64, s, seed=3).items()}
        net.load_state_dict(ref)                                   # bare keys (reference test.py:45-50)
        assert torch.equal(net.state_dict()["altblock.2.ang_trans.attention.in_proj_weight"],
                           ref["altblock.2.ang_trans.attention.in_proj_weight"])
        net.apply(LFT.weights_init)                                # reference train.py:37
    assert isinstance(LFT.get_loss(None), torch.nn.Module)


def test_default_init_ranges():
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=5, scale_factor=2))
    sd = net.state_dict()
    assert float(sd["conv_init0.0.weight"].abs().max()) <= 1 / 3 + 1e-6
    assert float(sd["altblock.0.spa_trans.attention.in_proj_weight"].abs().max()) <= 1 / 128 ** 0.5 + 1e-6
    assert torch.all(sd["altblock.1.ang_trans.norm.weight"] == 1) and torch.all(sd["altblock.1.ang_trans.norm.bias"] == 0)


def test_no_cpu_fallback():
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=5, scale_factor=2))
    with pytest.raises(_lib.LftError):
        net(torch.zeros(1, 1, 40, 40))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "lft_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(lft_\w+)\s*\(", hdr, flags=re.M))
    test_hdr = open(os.path.join(ROOT, "include", "lft_hip_test.h")).read()
    test_only = set(re.findall(r"^(?:int|const char\*)\s+(lft_\w+)\s*\(", test_hdr, flags=re.M))
    assert test_only == set(_lib.TEST_EXPORTS) and not (test_only & declared)       # debug aids live in the test-only header
    declared |= test_only
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert _lib.lib().lft_version() == _lib.ABI_VERSION == 5


def test_stale_library_and_changed_flags_are_noticed(monkeypatch):
    """A library that reports another ABI version is refused at load time (its entry points may take other arguments), and a
    change of the compiler flags -- which live in _lib.py, not in a source file -- makes needs_build() true."""
    _lib.build()
    assert not _lib.needs_build()
    monkeypatch.setattr(_lib, "COMMON_FLAGS", _lib.COMMON_FLAGS + ["-DSOMETHING_ELSE"])
    assert _lib.needs_build()
    monkeypatch.undo()
    assert not _lib.needs_build()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", 99)
    with pytest.raises(_lib.LftError, match="ABI version"):
        _lib.lib()
    monkeypatch.undo()
    L = _lib.lib()
    assert L.lft_status_read(None, 1, 5, 8, 8, 2, _lib.PREC_F16, None, None) == -1        # argument check before any device work
    assert L.lft_status_reset(None, 1, 5, 8, 8, 2, _lib.PREC_F16, None) == -1


def test_size_queries_and_argument_errors():
    assert _lib.packed_bytes(5, 32, 32, 4, _lib.PREC_BF16) > 2_000_000
    assert _lib.workspace_bytes(4, 5, 32, 32, 4, _lib.PREC_BF16) > _lib.workspace_bytes(1, 5, 32, 32, 4, _lib.PREC_BF16)
    with pytest.raises(_lib.LftError, match="scale factor"):
        _lib.packed_bytes(5, 32, 32, 3, _lib.PREC_BF16)
    with pytest.raises(_lib.LftError, match="prec"):
        _lib.packed_bytes(5, 32, 32, 2, 7)
    with pytest.raises(_lib.LftError, match="not implemented"):
        _lib.packed_bytes(12, 32, 32, 2, _lib.PREC_F32)
    assert _lib.packed_bytes(9, 32, 32, 4, _lib.PREC_BF16) > 2_000_000      # 9x9 = 81 views is supported


def test_training_and_metrics_size_queries_and_argument_errors():
    """The training / metrics entry points validate their arguments before touching the device (no GPU needed)."""
    from lft_amd import train as T
    from lft_amd.params import param_table
    assert T.grad_floats(2) == sum(int(np.prod(s)) for _, s, _ in param_table(64, 2)) == 1_114_240
    assert T.grad_floats(4) == 1_163_392
    assert T.tape_bytes(2, 5, 32, 32, 2) > 2 * T.tape_bytes(1, 5, 32, 32, 2) * 0.9
    # the backward pass's gradient tensors share an arena and the partial sums are reduced per layer (both sized by a dry run of
    # the pass): BASELINE configs[2] at 8 patches per step stays under 1 GiB per patch (round 2: 1.94)
    assert T.tape_bytes(8, 5, 32, 32, 2) <= 8 * 2**30
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.lft_train_grad_floats(3, ctypes.byref(n)) == -2                            # LFT_ERR_SHAPE
    assert L.lft_train_tape_bytes(1, 5, 32, 32, 3, ctypes.byref(n)) == -2
    assert L.lft_train_tape_offset(b"no.such.field", 1, 5, 8, 8, 2, ctypes.byref(n)) == -1
    assert b"unknown tape field" in L.lft_last_error()
    assert L.lft_train_tape_offset(b"spa3.hdn", 1, 5, 8, 8, 2, ctypes.byref(n)) == 0 and n.value > 0
    arr = (ctypes.c_void_p * 78)(*([1] * 78))                                            # never dereferenced: rejected first
    assert L.lft_train_forward(arr, 77, 1, 1, 1, 1, 5, 8, 8, 2, 0, None) == -1
    assert b"78" in L.lft_last_error()
    assert L.lft_train_forward(arr, 78, 1, 1, 1, 1, 5, 8, 8, 2, 9, None) == -1
    assert b"math" in L.lft_last_error()
    assert L.lft_train_backward(arr, 78, 1, 1, None, 1, 1, 5, 8, 8, 2, 0, None) == -1    # null dout
    assert L.lft_train_block_backward(arr, 78, 1, 1, 9, 0, 1, 1, 1, 1, 5, 8, 8, 2, 0, None) == -1    # unknown block
    assert L.lft_view_metrics_scratch_bytes(1, 5, 32, 32, ctypes.byref(n)) == 0 and n.value == 25 * 4 * 3 * 8
    assert L.lft_view_metrics(1, 1, 1, 5, 8, 8, 2.0, 1, 1, 1, None) == -2                 # views smaller than the SSIM window
    assert L.lft_adam_step(1, 1, 1, 1, 10, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, 0.0, None) == -1   # steps count from 1
    assert L.lft_adam_step(1, 1, 1, 1, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, -0.1, None) == -1  # weight decay >= 0


def test_gradient_buckets_tile_the_flat_buffer():
    """lft_train_grad_bucket (host-only): the three buckets the backward pass reports are disjoint, contiguous and cover
    the flat gradient buffer; bucket 0 (finished first) is the far end -- altblock.2, altblock.3, upsampling."""
    from lft_amd.params import param_table
    L = _lib.lib()
    for s in (2, 4):
        total = _lib.query("lft_train_grad_floats", s)
        spans = [_lib.query("lft_train_grad_bucket", s, b) for b in range(_lib.GRAD_BUCKETS)]
        assert spans[2][0] == 0 and spans[2][0] + spans[2][1] == spans[1][0] and spans[1][0] + spans[1][1] == spans[0][0]
        assert spans[0][0] + spans[0][1] == total
        off, starts = 0, {}
        for name, shape, _ in param_table(64, s):
            starts[name] = off
            off += int(np.prod(shape))
        assert spans[1][0] == starts["altblock.0.spa_trans.MLP.weight"]
        assert spans[0][0] == starts["altblock.2.spa_trans.MLP.weight"]
    first, count = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lft_train_grad_bucket(2, 3, ctypes.byref(first), ctypes.byref(count)) != 0


@pytest.fixture(scope="module")
def isa_env(tmp_path_factory):
    """The hazard tools' --build listings in a directory of this test run (LFT_ISA_DIR): never another tree's or user's listings."""
    return dict(os.environ, LFT_ISA_DIR=str(tmp_path_factory.mktemp("isa")))


def test_no_asm_loaded_register_is_read_before_its_wait(isa_env):
    """Every unit assembled with the product flags (no GPU needed): a register filled by an inline-asm global load must not be
    read -- hipcc copies such registers to set up tied asm operands -- before the counted s_waitcnt that guards it
    (tools/asm_load_hazards.py; the first k_linr did exactly that and passed every test in fp32)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "asm_load_hazards.py"), "--build"], capture_output=True, text=True,
                       env=isa_env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 suspicious read(s)" in r.stdout


def test_lds_dma_pipelines_are_covered_by_counted_waits_and_barriers(isa_env):
    """Static check of every LDS-DMA pipeline in the product listing (tools/lds_dma_hazards.py; the listings of the test above are
    re-used): each slot is read only after all pieces of its fill were retired by a counted vmcnt wait AND published by a barrier,
    and refilled only after its reads were waited for and a barrier passed.  The check must also bite: with every counted wait of
    k_spa_b weakened by one it has to report violations."""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "lds_dma_hazards.py")
    r = subprocess.run([sys.executable, tool, "--build"], capture_output=True, text=True, env=dict(isa_env, LFT_HAZARD_REUSE="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 LDS-DMA protocol violation(s)" in r.stdout
    isa = isa_env["LFT_ISA_DIR"]
    lines = open(os.path.join(isa, _lib.INFERENCE_UNIT + ".s")).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN12_GLOBAL__N_17k_spa_bIDF16bLb0ELb1ELb0E"))
    n = 0
    for i in range(start, len(lines)):
        if "s_endpgm" in lines[i]:
            break
        m = re.search(r"vmcnt\((\d+)\)", lines[i])
        if m and "s_waitcnt" in lines[i] and int(m.group(1)) > 0:
            lines[i] = lines[i].replace(m.group(0), "vmcnt(%d)" % (int(m.group(1)) + 1))
            n += 1
    assert n >= 10
    open(os.path.join(isa, "spa_b_mut.s"), "w").write("\n".join(lines))
    r = subprocess.run([sys.executable, tool, os.path.join(isa, "spa_b_mut.s"), "k_spa_bIDF16bLb0ELb1ELb0E"], capture_output=True, text=True)
    assert r.returncode == 1 and "USE of" in r.stdout, r.stdout[-2000:]


def test_every_kernel_is_emitted_by_one_unit_except_the_shared_ones(isa_env):
    """A unit emits the kernels of the headers it includes, so each unit of the library includes only what it launches from (the
    listings of the hazard tests above are re-used): the kernel symbols found in more than one unit's listing are exactly
    _lib.SHARED_KERNELS, the kernels two units really launch -- and those are few."""
    import re
    found = {}
    for unit, path in _lib.listings(isa_env["LFT_ISA_DIR"], reuse=True).items():
        for sym in re.findall(r"^\s*\.amdhsa_kernel (\w+)", open(path, errors="replace").read(), flags=re.M):
            found.setdefault(sym, []).append(unit)
    assert {tuple(units) for units in found.values()} >= {(u,) for u in _lib.UNITS} and len(found) > 200, "the listings were not read"
    twice = {sym: units for sym, units in found.items() if len(units) > 1}
    unnamed = {sym: units for sym, units in twice.items() if not any(frag in sym for frag in _lib.SHARED_KERNELS)}
    assert not unnamed, unnamed
    unseen = [frag for frag in _lib.SHARED_KERNELS if sum(frag in sym for sym in twice) != 1]
    assert not unseen, unseen
    assert len(twice) == len(_lib.SHARED_KERNELS) <= 6
