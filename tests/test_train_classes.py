"""CPU check of tests/train_classes.py against figures worked out BY HAND from lft_amd/csrc/lft_train_host.cuh (no GPU, no library),
of the case list of tests/test_gpu_train_classes.py against the model, and of the chunked fp64 reference against the unchunked one.

run_lin.  tiles = ceil(N / 32).  nt starts at 4 and is halved while nOT % nt != 0 or tiles * (nOT / nt) < 2048:
  64 outputs (nOT 2)     nt 4 never (2 % 4); nt 2 needs tiles >= 2048: N >= 2047 * 32 + 1 = 65 505.
  128 outputs (nOT 4)    nt 2 needs tiles * 2 >= 2048, tiles >= 1024: N >= 32 737; nt 4 needs tiles >= 2048: N >= 65 505.
  256 outputs (nOT 8)    nt 2: tiles * 4 >= 2048, tiles >= 512: N >= 16 353; nt 4: tiles * 2 >= 2048: N >= 32 737.
  1024 outputs (nOT 32)  nt 2: tiles * 16 >= 2048, tiles >= 128: N >= 4 065; nt 4: tiles * 8 >= 2048, tiles >= 256: N >= 8 161.
  The ring (k_linr) needs N > 65 536, so a 128-output view runs nt 4 WITHOUT the ring only for N in (65 504, 65 536]; from 65 537 it
  is one packed group of four tiles (full4) and rides the ring.  64-output views are "the view's last group of two" (OT % 4 == 2).
  Above 65 536 tokens k_lin keeps (i) VW_UPM at 2x: (s + 2)^2 = 16 footprint rows are ONE 32-row tile, so nt = 1 and the block is
  neither a group of four nor a last group of two (k_lin<1, MM, false>: the tiled-input form ends at 65 536 too); at 4x 36 rows are
  two tiles, a last group of two, through k_linr<2>; (ii) the position-token embedding of SpaTrans, whose N is h w, not the batch's.
  3x3 views ride the ring because their tiles are all of the view's (conv: OT = nt = 2; MLP: 4; its transpose: 2) and
  9 KS is even; on 32-wide views they take the row forms KS 4 (64 inputs) and KS 8 (128 inputs; nt 2 only).

wgrad, fp32, 64 x 64 Linear at N = 40 000: gridy = 2 x 1 = 2, slots = 256 x 4 = 1 024, base = min(128, 40 000 / 512) = 78,
  rounds = ceil(156 / 1 024) = 1, nch = min(min(512, 1 024 / 2), max(78, 40 000 / 256 = 156)) = 156; len = ceil(40 000 / 156) = 257
  -> 320 (multiple of 64); 40 000 / 320 = 125 chunks hold tokens, 31 are EMPTY; shares of 80 divide 40 000: no partial wave.
  bf16x3, 128 x 64 there: gridy 4, base * gridy * 4 = 1 248 > 1 024 -> nch = base = 78; len = 513 -> 576; 69 full chunks + 256 tokens:
  70 chunks hold tokens, 8 are empty; the last chunk's waves (144 each) get 144, 112 (PARTIAL), 0, 0.
  3x3, 64 -> 64, fp32, N = 76 800 on 32-wide views: gridy 6, slots 512, base 128, rounds = ceil(768 / 512) = 2,
  nch = min(min(512, 1 024 / 6 = 170), max(128, 300)) = 170; len = 452 -> 512; 150 chunks hold tokens, 20 are empty; shares of 128
  start at multiples of 16: every wave takes fast3.
Caps.  k_ln_bwd: min(512, ceil(N / 16)) workgroups, capped from N = 8 193.  k_conv0_wgrad: ceil(N / 2048) tokens per wave.
k_ang_attn<32> up to 32 views (A <= 5), <128> above.
"""
import pytest
import torch

import train_classes as C
import train_ref as R

V2, V4 = C.views(2), C.views(4)


def first_n(view, nOT, nt):
    return next(N for N in range(1, 70000) if C.run_lin(view, 0, nOT, N, 10).nt == nt)


def test_nt_thresholds():
    assert first_n(V2["aout_f"], 0, 2) == 65505 and all(C.run_lin(V2["aout_f"], 0, 0, N, 10).nt < 4 for N in (65505, 65536, 10 ** 6))
    assert first_n(V2["sout_f"], 0, 2) == 32737 and first_n(V2["sout_f"], 0, 4) == 65505
    assert first_n(V2["sff1_f"], 0, 2) == 16353 and first_n(V2["sff1_f"], 0, 4) == 32737
    assert V4["up_f"].OT == 32 and first_n(V4["up_f"], 0, 2) == 4065 and first_n(V4["up_f"], 0, 4) == 8161
    # blocks of a view count by their own tiles: Q | K of the 384 x 128 in-projection is a 256-output GEMM, V a 128-output one
    assert first_n(V2["sin_f"], 8, 4) == 32737 and C.run_lin(V2["sin_f"], 8, 4, 32737, 10).nt == 2


def test_ring_and_tiled_thresholds():
    v = V2["sout_f"]
    noring4 = [N for N in range(65000, 66000) if C.run_lin(v, 0, 0, N, 10).kernel == ("k_lin", 4, True)]
    assert noring4 == list(range(65505, 65537))
    assert C.run_lin(v, 0, 0, 65537, 10).kernel == ("k_linr", 4, 0)
    assert C.run_lin(V2["ain_f"], 4, 2, 65537, 10).kernel == ("k_linr", 2, 0) and C.run_lin(V2["ain_f"], 0, 4, 65537, 10).kernel == ("k_linr", 4, 0)
    # the views that keep k_lin above the threshold
    for N in (65537, 76800, 10 ** 6):
        stay = {k for k, l in C.lin_table(2, N, 1024, 32).items() if not l.ring}
        assert stay == {("upm", 0, "N"), ("mlp_f", 0, "hw")}
        assert C.lin_table(2, N, 1024, 32)[("upm", 0, "N")].kernel == ("k_lin", 1, False)
        assert {k for k, l in C.lin_table(4, N, 1024, 32).items() if not l.ring} == {("mlp_f", 0, "hw")}
    assert V2["upm"] == C.View(1, 16, 1) and V4["upm"] == C.View(2, 64, 1) and V2["upm_b"] == C.View(8, 2, 1) and V4["upm_b"] == C.View(32, 4, 1)
    assert not C.run_lin(V2["upm_b"], 0, 0, 40000, 10).tiled and C.run_lin(V4["upm_b"], 0, 0, 40000, 10).tiled      # KS 2 / KS 4
    # 3x3 views: row forms on 32-wide views only, and only on the ring
    assert C.run_lin(V2["conv_f"], 0, 0, 76800, 32).kernel == ("k_linr", 2, 4) and C.run_lin(V2["conv_f"], 0, 0, 76800, 31).kernel == ("k_linr", 2, 0)
    assert C.run_lin(V2["mlp_f"], 0, 0, 76800, 32).kernel == ("k_linr", 4, 4) and C.run_lin(V2["mlp_b"], 0, 0, 76800, 32).kernel == ("k_linr", 2, 8)
    assert C.run_lin(V2["mlp_f"], 0, 0, 65536, 32).kernel == ("k_lin", 4, False) and C.run_lin(V2["conv_b"], 0, 0, 4096, 32).kernel == ("k_lin", 1, False)


def test_wgrad_rows():
    assert C.wgrad(64, 64, 1, "fp32", 40000, 10) == C.Wg((2, 1), 156, 320, 31, 0, 0, 0, "none")
    assert C.wgrad(64, 64, 1, "bf16x3", 40000, 10) == C.wgrad(64, 64, 1, "fp32", 40000, 10)          # 78 * 2 * 4 = 624 <= 1 024: not reduced
    assert C.wgrad(128, 64, 1, "bf16x3", 40000, 10) == C.Wg((2, 1), 78, 576, 8, 1, 112, 2, "none")
    assert C.wgrad(128, 64, 1, "bf16x6", 40000, 10) == C.wgrad(128, 64, 1, "fp32", 40000, 10)
    assert C.wgrad(64, 64, 9, "fp32", 76800, 32) == C.Wg((2, 3), 170, 512, 20, 0, 0, 0, "all")
    assert C.wgrad(64, 64, 9, "fp32", 76800, 31).fast3 == "none"
    assert C.wgrad(128, 64, 9, "fp32", 1024, 32) == C.Wg((2, 3), 4, 256, 0, 0, 0, 0, "all")          # the position tokens of a 32 x 32 view


def test_caps():
    assert C.ln_bwd_blocks(8192) == (512, False) and C.ln_bwd_blocks(8193) == (512, True) and C.ln_bwd_blocks(4096) == (256, False)
    assert C.conv0_wgrad_per_wave(76800) == (38, 2022) and C.conv0_wgrad_per_wave(2048) == (1, 2048) and C.conv0_wgrad_per_wave(100) == (1, 100)
    assert [C.ang_attn_vp(A) for A in (1, 5, 6, 11)] == [32, 32, 128, 128]


@pytest.mark.parametrize("shape", [c for c, _ in C.GPU_CASES], ids=lambda c: "A%d_s%d_B%d_%dx%d" % c)
def test_case_reaches_its_class(shape):
    C.check_case(shape)


def test_cases_cover_every_variant():
    """The union of the GPU cases (in the blocks each compares with the reference) reaches every variant the model can produce for
    A <= 11, s in {2, 4}: every (kernel, NT, TILED | KS) of the GEMMs, every k_wgrad<NI, MM, TX> with and without fast3, both
    k_ang_attn sizes, k_ln_bwd below and at its cap -- each in the three math modes, which every case runs.  Nothing is unreachable
    or uncovered; what the case list does NOT hold is every (view, variant) PAIR: a 256-output view at nt 2 (16 353 .. 32 736
    tokens) runs the kernel the 128-output views run in the 40 000-token case, with another tile count in LinP."""
    universe = C.all_lin_kernels(2) | C.all_lin_kernels(4)
    assert universe == {("k_lin", nt, t) for nt in (1, 2, 4) for t in (True, False)} | {
        ("k_linr", 2, 0), ("k_linr", 4, 0), ("k_linr", 2, 4), ("k_linr", 2, 8), ("k_linr", 4, 4)}
    got, wg, vp, ln = set(), set(), set(), set()
    for shape, blocks in C.GPU_CASES:
        c = C.case_classes(shape, blocks)
        got |= c["kernels"]
        wg |= c["wg_kernels"]
        if "ang" in blocks:
            vp.add(c["vp"])
        if "spa" in blocks or "ang" in blocks:
            ln.add(c["ln"][1])
    assert got == universe, universe - got
    assert wg == {(2, 3, "fast3"), (2, 3, "general"), (4, 1, "general"), (2, 1, "general")}
    assert vp == {32, 128} and ln == {False, True}
    # both scales above and below the ring threshold
    assert {(s, C.tokens(A, s, B, h, w) > C.RING_N) for (A, s, B, h, w), _ in C.GPU_CASES} == {(2, False), (2, True), (4, False), (4, True)}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_chunked_spa_reference_equals_unchunked(dtype):
    """The SpaTrans reference over chunks of view images (views do not interact) with the weight gradients summed over the chunks
    == the one-pass form: fp64 to rounding, 7 images in chunks of 1, 2 and 3 (a short last chunk), h != w, given branch masks."""
    from lft_amd.params import deterministic_state
    from oracle import lft_oracle as O
    A_B, V, h, w = 1, 7, 5, 6
    sd = O.state_from_numpy(deterministic_state(64, 2, seed=1, flavor="stress"))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(A_B, 64, V, h, w, generator=g)
    d_out = torch.randn(A_B, 64, V, h, w, generator=g)
    masks = {"spa1": torch.rand(h * w, A_B * V, 256, generator=g) > 0.5}
    one = R.block_reference("spa", sd, 1, x, None, d_out, 0, 2, masks, dtype=dtype, max_images=A_B * V)
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    for step in (1, 2, 3):
        ch = R.block_reference("spa", sd, 1, x, None, d_out, 0, 2, masks, dtype=dtype, max_images=step)
        assert ch["grads"].keys() == one["grads"].keys() and len(ch["grads"]) == 10
        for k in ("y", "d_in"):
            assert float((ch[k] - one[k]).abs().max()) <= tol * float(one[k].abs().max()), (k, step)
        for k, v in one["grads"].items():
            assert float((ch["grads"][k] - v).abs().max()) <= tol * float(v.abs().max()), (k, step)
    # and the one-pass form is the oracle's own block under plain autograd
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xx = x.double().requires_grad_(True)
    O.branch_masks = masks
    try:
        O.spa_block(leaves, 1, xx).backward(d_out.double())
    finally:
        O.branch_masks = None
    ref = R.block_reference("spa", sd, 1, x, None, d_out, 0, 2, masks, max_images=2)
    assert float((ref["d_in"] - xx.grad).abs().max()) <= 1e-12 * float(xx.grad.abs().max())
    for k, v in ref["grads"].items():
        assert float((v - leaves[k].grad).abs().max()) <= 1e-12 * float(v.abs().max()), k
