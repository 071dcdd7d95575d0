"""-m gpu: the attention maps exported from the fp32 training forward (lft_train_attn_maps, lft_amd/attention.py) against the real
reference (tests/golden/attention_*.npz) and against torch's functional multi-head attention on the oracle's taps.

Gate: G.rel_max <= 1e-4, the per-stage fp32 bound of tests/test_gpu_parity.py (torch's own fp32 maps differ from its fp64 ones by
<= 5e-6 relative on these inputs, so the gate leaves more than an order of magnitude and still catches any structural error).
The reference's NaN rows (queries with an empty window, h < w) are mapped to 0: this library writes exact zeros there.
Observed on an MI355X: <= 7.9e-7 against the reference fixtures, <= 1.3e-6 against the functional
computation over the six shapes, maps x V against the tape's attention output <= 5.3e-7; bf16x6 tapes <= 4.0e-7, bf16x3 <= 4.1e-6."""
from types import SimpleNamespace

import pytest
import torch

from lft_amd import _lib, attention as AT, train as T
from lft_amd.params import deterministic_state, param_table, synthetic_lr
from oracle import lft_oracle as O

import attention_util as U
import gpu_util as G

pytestmark = pytest.mark.gpu

TOL = U.FP32_STAGE_TOL
BLOCKS = [f"{k}{l}" for l in range(4) for k in ("ang", "spa")]


def make_net(sd, A, s):
    from model import LFT
    net = LFT.get_model(SimpleNamespace(channels=64, angRes=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(G.DEV).eval()


def device_params(sd, s):
    return [torch.from_numpy(sd[n]).to(G.DEV).contiguous() for n, _, _ in param_table(64, s)]


def check_against(got, ref, h, w, what):
    """got: device maps; ref: CPU maps with torch's NaN rows.  Returns the relative error."""
    got = got.cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not torch.isnan(got).any(), what
    nan = torch.isnan(ref)
    if what.startswith("spa"):
        empty = U.empty_window_queries(h, w)
        nan_rows = nan.reshape(-1, h, w, 25).any(-1)
        assert torch.equal(nan_rows, empty.expand_as(nan_rows)), what      # torch's NaN rows are the empty windows, nothing else
        rows = got.reshape(-1, h, w, 25)
        assert torch.all(rows[:, empty] == 0), what                       # empty-window rows are exactly 0
        sums = rows[:, ~empty].sum(-1)
    else:
        assert not nan.any()
        sums = got.sum(-1)
    assert float((sums - 1).abs().max()) <= 1e-4, (what, float((sums - 1).abs().max()))
    rel = G.rel_max(got, torch.nan_to_num(ref))
    return rel


@pytest.mark.parametrize("name", U.FIXTURES)
def test_maps_match_the_reference(name):
    z, sd, lr, (A, s, B, h, w) = U.load_fixture(name)
    net = make_net(sd, A, s)
    worst = 0.0
    for per_head, key in ((False, "mean"), (True, "heads")):
        got = net.attention_maps(lr.to(G.DEV), per_head=per_head)
        assert list(got) == BLOCKS
        for b in BLOCKS:
            if f"{b}_{key}" not in z.files:
                continue
            rel = check_against(got[b], torch.from_numpy(z[f"{b}_{key}"]), h, w, b)
            print(f"{name} {b} {key}: rel_max vs reference {rel:.3e}")
            worst = max(worst, rel)
            assert rel <= TOL, (b, key, rel)
        if name.endswith("6x12"):                                          # the zeros sit where the reference's window is closed
            c = got["spa0"].cpu().reshape(-1, h, w, 25)
            open_taps = AT.compact_from_dense((O.window_mask(h, w) == 0).float(), h, w).reshape(h, w, 25) != 0
            assert torch.all(c[:, ~open_taps] == 0) and torch.all(c[:, open_taps] > 0)
    print(f"{name}: worst rel_max {worst:.3e}")


SHAPES = [(5, 2, 2, 6, 6), (3, 2, 1, 9, 7), (9, 4, 1, 8, 8), (5, 2, 1, 32, 32), (2, 2, 1, 64, 64), (2, 2, 1, 6, 12),
          # every other view count class: V = 1, 16 (k_ang_attn<32>), 49, 64, 100, 121 (k_ang_attn<128>; k_ang_maps sizes its LDS from V)
          (1, 2, 2, 6, 7), (4, 2, 1, 5, 5), (7, 2, 1, 3, 5), (8, 2, 1, 5, 3), (10, 4, 1, 3, 5), (11, 2, 1, 4, 3)]


@pytest.mark.parametrize("A,s,B,h,w", SHAPES)
def test_shape_coverage_against_functional_attention(A, s, B, h, w):
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0))
    net = make_net(sd, A, s)
    x = lr.to(G.DEV)
    heads = net.attention_maps(x, per_head=True)
    mean = net.attention_maps(x, per_head=False)
    for per_head, got in ((True, heads), (False, mean)):
        ref = U.functional_maps(sd, lr, A, s, per_head)
        for b in BLOCKS:
            rel = check_against(got[b], ref[b], h, w, b)
            print(f"A{A} s{s} B{B} {h}x{w} {b} {'heads' if per_head else 'mean'}: rel_max vs functional {rel:.3e}")
            assert rel <= TOL, (b, per_head, rel)
        if not per_head:
            for math in ("bf16x6", "bf16x3"):                            # reported, not gated
                lo = net.attention_maps(x, per_head=False, math=math)
                print(f"A{A} s{s} B{B} {h}x{w} {math}: " +
                      " ".join(f"{b} {G.rel_max(lo[b].cpu(), torch.nan_to_num(ref[b])):.2e}" for b in BLOCKS))
    for b in BLOCKS:                                                       # HEADS averaged over H is MEAN: a sum of 8 fp32 terms
        hm = heads[b].mean(dim=3 if b.startswith("ang") else 2)
        rel = G.rel_max(hm.cpu(), mean[b].cpu())
        assert rel <= 1e-6, (b, rel)


@pytest.mark.parametrize("A,s,B,h,w", [(5, 2, 2, 6, 6), (2, 2, 1, 6, 12), (9, 4, 1, 8, 8), (11, 2, 1, 4, 3)])
def test_maps_are_the_weights_the_network_used(A, s, B, h, w):
    """Per-head maps times the tape's V give the tape's attention output o (angular layer 1, spatial layer 2)."""
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    ps = device_params(sd, s)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    _, tape = T.train_forward(ps, lr, A, s)
    V = A * A
    m = AT.maps_from_tape(tape, _lib.BLOCK_ANG, 1, True, B, A, h, w, s)                       # [B,h,w,8,V,V]
    v = T.tape_view(tape, "ang1.v", B, A, h, w, s, (B, V, h, w, 8, 8))
    o = T.tape_view(tape, "ang1.o", B, A, h, w, s, (B, V, h, w, 8, 8))
    got = torch.einsum("byxhij,bjyxhc->biyxhc", m.double(), v.double()).float()
    rel = G.rel_max(got.cpu(), o.cpu())
    print(f"A{A} {h}x{w} ang1: maps x V vs tape o rel_max {rel:.3e}")
    assert rel <= TOL
    m = AT.maps_from_tape(tape, _lib.BLOCK_SPA, 2, True, B, A, h, w, s).reshape(B * V, 8, h, w, 5, 5)
    v = T.tape_view(tape, "spa2.v", B, A, h, w, s, (B * V, h, w, 8, 16))
    o = T.tape_view(tape, "spa2.o", B, A, h, w, s, (B * V, h, w, 8, 16))
    vp = torch.nn.functional.pad(v.double(), (0, 0, 0, 0, 2, 2, 2, 2))                          # zero halo around every view
    got = torch.zeros_like(o, dtype=torch.float64)
    for dy in range(5):
        for dx in range(5):
            got += m[:, :, :, :, dy, dx].permute(0, 2, 3, 1).unsqueeze(-1).double() * vp[:, dy:dy + h, dx:dx + w]
    rel = G.rel_max(got.float().cpu(), o.cpu())
    print(f"A{A} {h}x{w} spa2: maps x V vs tape o rel_max {rel:.3e}")
    assert rel <= TOL


def test_the_tape_is_only_read():
    A, s, B, h, w = 5, 2, 2, 8, 8
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    ps = device_params(sd, s)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    dout = torch.randn((B, 1, A * h * s, A * w * s), generator=torch.Generator().manual_seed(3)).to(G.DEV)
    _, tape = T.train_forward(ps, lr, A, s)
    g0 = T.train_backward(ps, lr, tape, dout, A, s).clone()
    _, tape = T.train_forward(ps, lr, A, s, tape=tape)
    before = tape.clone()
    for per_head in (False, True):
        for l in range(4):
            for block in (_lib.BLOCK_ANG, _lib.BLOCK_SPA):
                AT.maps_from_tape(tape, block, l, per_head, B, A, h, w, s)
    torch.cuda.synchronize()
    assert torch.equal(tape, before)
    g1 = T.train_backward(ps, lr, tape, dout, A, s)
    assert torch.equal(g0, g1)                                            # bit-identical gradients


@pytest.mark.parametrize("A,s,B,h,w", [(5, 2, 2, 16, 16), (9, 2, 1, 8, 8)])
def test_maps_are_deterministic_capturable_and_allocate_nothing(A, s, B, h, w):
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    ps = device_params(sd, s)
    lr = torch.from_numpy(synthetic_lr(B, A, h, w, seed=0)).to(G.DEV)
    _, tape = T.train_forward(ps, lr, A, s)
    for block in (_lib.BLOCK_ANG, _lib.BLOCK_SPA):
        for per_head in (False, True):
            shape = AT.map_shape(block, per_head, B, A, h, w)
            a, b, c = (torch.full(shape, float("nan"), dtype=torch.float32, device=G.DEV) for _ in range(3))
            torch.cuda.synchronize()
            used = torch.cuda.memory_allocated()
            AT.maps_from_tape(tape, block, 3, per_head, B, A, h, w, s, out=a)
            AT.maps_from_tape(tape, block, 3, per_head, B, A, h, w, s, out=b)
            assert torch.cuda.memory_allocated() == used                  # output and tape are caller buffers
            torch.cuda.synchronize()
            assert not torch.isnan(a).any() and torch.equal(a, b)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                AT.maps_from_tape(tape, block, 3, per_head, B, A, h, w, s, out=c)     # eager warm-up on the capture stream
                side.synchronize()
                c.fill_(float("nan"))
                with torch.cuda.graph(graph, stream=side, capture_error_mode=T.CAPTURE_MODE):
                    AT.maps_from_tape(tape, block, 3, per_head, B, A, h, w, s, out=c)
                graph.replay()
            side.synchronize()
            torch.cuda.current_stream().wait_stream(side)
            assert torch.equal(a, c)


def test_scene_angular_attention_matches_cpu_assembly():
    A, s, h0, w0, patch, stride, layer = 5, 2, 48, 40, 32, 16, 1
    sd = deterministic_state(64, s, seed=1, flavor="stress")
    net = make_net(sd, A, s)
    scene = torch.rand((A * h0, A * w0), generator=torch.Generator().manual_seed(11))
    got = AT.scene_angular_attention(net, scene.to(G.DEV), layer, patch=patch, stride=stride).cpu()
    assert tuple(got.shape) == (A * h0, A * w0)
    # the same on the CPU side: reference tiling of the oracle, per-patch maps of the centre view, LFintegrate at scale 1
    sub = O.lf_divide(scene, A, patch, stride)
    nu, nv = sub.shape[:2]
    patches = sub.reshape(nu * nv, 1, A * patch, A * patch)
    maps = net.attention_maps(patches.to(G.DEV), blocks=[f"ang{layer}"], max_batch=3)[f"ang{layer}"].cpu()     # [n,p,p,V,V]
    row = maps[:, :, :, (A * A) // 2, :].reshape(nu * nv, patch, patch, A, A)
    mosaics = row.permute(0, 3, 1, 4, 2).reshape(nu, nv, A * patch, A * patch)
    ref = O.views_to_scene_mosaic(O.lf_integrate(mosaics, A, patch, stride, h0, w0))
    rel = G.rel_max(got, ref)
    print(f"scene {A}x{A} of {h0}x{w0}: {nu * nv} patches, rel_max vs CPU assembly {rel:.3e}")
    assert rel <= TOL
    per_pixel = got.reshape(A, h0, A, w0).sum(dim=(0, 2))                  # every pixel's 25 weights
    assert float((per_pixel - 1).abs().max()) <= 1e-4
    other = AT.scene_angular_attention(net, scene.to(G.DEV), layer, query_view=0, patch=patch, stride=stride).cpu()
    assert not torch.equal(other, got)
