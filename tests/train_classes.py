"""Class model of the training step's shape-dependent dispatch (pure Python; no GPU, no library).

The training GEMMs, weight gradients and the capped launches are chosen by the token count N = B A^2 h w, the view width w and the
scale s.  This module re-derives those choices from lft_amd/csrc/lft_train_host.cuh (build_views, run_lin, wgrad, wg_chunks, ln_bwd,
conv0_wgrad, ang_attn) and lft_train.cuh (k_wgrad's fast3 test), so that every size-class case of tests/test_gpu_train_classes.py
can ASSERT the classes it was chosen for: a later change of a threshold then fails the case's table instead of silently moving
the case into a class another one already covers.  tests/test_train_classes.py pins the thresholds to figures worked out by hand.
"""
from collections import namedtuple

RING_N = 65536                  # run_lin: k_linr above this many tokens, the tiled-input form of k_lin up to it
MIN_WAVE_TILES = 2048           # run_lin: a launch should have at least this many (32-token tile x output block) waves
K_WG_CHUNKS, K_WG_CHUNKS_MAX = 128, 512      # kWgChunks, kWgChunksMax
K_LN_BLOCKS = 512               # kLnBlocks
K_TAIL_WAVES = 2048             # kTailWaves
CUS = 256

View = namedtuple("View", "OT KS taps")


def views(s):
    """The packed weight views of build_views (one layer's; the four layers are alike): name -> (output tiles of 32, k-steps of 16, taps).
    fwd(O, I) = (O / 32, I / 16); bwd(O, I), the transpose of an O x I matrix, = (I / 32, O / 16)."""
    ss, gp = s * s, (s + 2) * (s + 2)
    gt = (gp + 31) // 32
    return {
        "conv_f": View(2, 4, 9), "conv_b": View(2, 4, 9),
        "mlp_f": View(4, 4, 9), "mlp_b": View(2, 8, 9),
        "sin_f": View(12, 8, 1), "sqk_b": View(4, 16, 1), "sv_b": View(4, 8, 1),
        "sout_f": View(4, 8, 1), "sout_b": View(4, 8, 1),
        "sff1_f": View(8, 8, 1), "sff1_b": View(4, 16, 1), "sff2_f": View(4, 16, 1), "sff2_b": View(8, 8, 1),
        "slin_f": View(2, 8, 1), "slin_b": View(4, 4, 1),
        "ain_f": View(6, 4, 1), "aqk_b": View(2, 8, 1), "av_b": View(2, 4, 1),
        "aout_f": View(2, 4, 1), "aout_b": View(2, 4, 1),
        "aff1_f": View(4, 4, 1), "aff1_b": View(2, 8, 1), "aff2_f": View(2, 8, 1), "aff2_b": View(4, 4, 1),
        "up_f": View(2 * ss, 4, 1), "up_b": View(2, 4 * ss, 1),
        "upm": View(gt, 4 * ss, 1), "upm_b": View(2 * ss, 2 * gt, 1),
    }


# (view, ot0, nOT, tokens) of every run_lin request of train_forward and of the backward pass, by block; nOT 0 = the whole view,
# tokens "N" = all tokens, "hw" = the position tokens of one view image (SpaTrans embeds its position table with the same conv)
LIN_CALLS = {
    "init": [("conv_f", 0, 0, "N"), ("conv_b", 0, 0, "N")],
    "ang": [("ain_f", 0, 4, "N"), ("ain_f", 4, 2, "N"), ("aout_f", 0, 0, "N"), ("aff1_f", 0, 0, "N"), ("aff2_f", 0, 0, "N"),
            ("aff2_b", 0, 0, "N"), ("aff1_b", 0, 0, "N"), ("aout_b", 0, 0, "N"), ("av_b", 0, 0, "N"), ("aqk_b", 0, 0, "N")],
    "spa": [("mlp_f", 0, 0, "N"), ("mlp_f", 0, 0, "hw"), ("sin_f", 0, 8, "N"), ("sin_f", 8, 4, "N"), ("sout_f", 0, 0, "N"),
            ("sff1_f", 0, 0, "N"), ("sff2_f", 0, 0, "N"), ("slin_f", 0, 0, "N"),
            ("slin_b", 0, 0, "N"), ("sff2_b", 0, 0, "N"), ("sff1_b", 0, 0, "N"), ("sout_b", 0, 0, "N"), ("sv_b", 0, 0, "N"),
            ("sqk_b", 0, 0, "N"), ("mlp_b", 0, 0, "N")],
    "upsample": [("up_f", 0, 0, "N"), ("upm", 0, 0, "N"), ("upm_b", 0, 0, "N"), ("up_b", 0, 0, "N")],
}

Lin = namedtuple("Lin", "nt ring tiled ks3 kernel")


def run_lin(view, ot0, nOT, N, w):
    """run_lin's choices for tiles [ot0, ot0 + nOT) of `view` at N tokens of w-wide views.  kernel: ("k_lin", NT, TILED) or
    ("k_linr", NT, KS) -- the template arguments besides the math mode."""
    OT, KS, taps = view
    if nOT <= 0:
        nOT = OT
    tiles = (N + 31) // 32
    nt = 4
    while nt > 1 and (nOT % nt or tiles * (nOT // nt) < MIN_WAVE_TILES):
        nt >>= 1
    full4 = nt == 4 and ot0 % 4 == 0 and ot0 + nOT <= OT // 4 * 4
    last2 = nt == 2 and nOT == 2 and OT % 4 == 2 and ot0 == OT // 4 * 4
    ring = N > RING_N and (full4 or last2) and (taps == 1 or (nOT == OT and OT == nt)) and (taps * KS) % 2 == 0
    tiled = taps == 1 and KS % 4 == 0 and N <= RING_N
    ks3 = KS if (taps == 9 and w == 32 and KS in (4, 8)) else 0
    if ring:
        kernel = ("k_linr", nt, (4 if ks3 == 4 else 0) if nt == 4 else ks3)
    else:
        kernel = ("k_lin", nt, tiled)
    return Lin(nt, ring, tiled, ks3, kernel)


def lin_table(s, N, hw, w, blocks=("init", "ang", "spa", "upsample")):
    """{(view, ot0, tokens): Lin} of every run_lin request of the given blocks."""
    V = views(s)
    return {(name, ot0, tok): run_lin(V[name], ot0, nOT, N if tok == "N" else hw, w)
            for b in blocks for name, ot0, nOT, tok in LIN_CALLS[b]}


def lin_kernels(s, N, hw, w, blocks=("init", "ang", "spa", "upsample")):
    return {l.kernel for l in lin_table(s, N, hw, w, blocks).values()}


# (Co, Ci, taps, tokens) of every weight-gradient launch of the backward pass, by block
def wgrad_calls(s):
    ss, gt = s * s, ((s + 2) * (s + 2) + 31) // 32
    return {
        "init": [(64, 64, 9, "N")],
        "ang": [(64, 128, 1, "N"), (128, 64, 1, "N"), (64, 64, 1, "N"), (128, 64, 1, "N")],
        "spa": [(64, 128, 1, "N"), (128, 256, 1, "N"), (256, 128, 1, "N"), (128, 128, 1, "N"), (128, 64, 9, "N"), (128, 64, 9, "hw")],
        "upsample": [(32 * gt, 64 * ss, 1, "N"), (64 * ss, 64, 1, "N")],
    }


Wg = namedtuple("Wg", "kernel nch chunk_len empty partial last_share idle fast3")


def wgrad(Co, Ci, taps, math, N, w):
    """wgrad's launch: kernel = k_wgrad's (NI, TX); nch chunks of chunk_len tokens (four waves x chunk_len / 4); `empty` chunks start
    at or past N (their partial images must still be written as zeros for k_reduce_all); `partial` waves have a share that is
    neither whole nor empty (0 or 1: the wave that holds token N - 1) of `last_share` tokens; `idle` waves of a non-empty chunk have
    none; fast3 = how many of the non-idle waves take the one-image-row-per-step path of k_wgrad<2, MM, 3> ("all", "none" or a count)."""
    if taps == 9:
        gridy, slots, kernel = Co // 32 * 3, CUS * 2, (2, 3)
    elif Ci % 128 == 0:
        gridy, slots, kernel = Co // 32 * (Ci // 128), CUS * 3, (4, 1)
    else:
        gridy, slots, kernel = Co // 32 * (Ci // 64), CUS * 4, (2, 1)
    base = min(K_WG_CHUNKS, max(4, N // 512))
    rounds = max(1, (base * gridy + slots - 1) // slots)
    nch = min(min(K_WG_CHUNKS_MAX, rounds * slots // gridy), max(base, N // 256))
    if math == "bf16x3" and base * gridy * 4 > slots:
        nch = base
    nch = max(nch, 1)
    length = ((N + nch - 1) // nch + 63) & ~63
    sub = length // 4
    live = (N + length - 1) // length
    partial = idle = last_share = nfast = nwork = 0
    for c in range(live):
        for k in range(4):
            ta = c * length + k * sub
            nsub = max(0, min(ta + sub, N) - ta)
            if nsub == 0:
                idle += 1
                continue
            nwork += 1
            if nsub < sub:
                partial += 1
                last_share = nsub
            if taps == 9 and w == 32 and nsub % 16 == 0 and ta % 16 == 0:
                nfast += 1
    fast3 = "all" if nfast == nwork else "none" if nfast == 0 else nfast
    return Wg(kernel, nch, length, nch - live, partial, last_share, idle, fast3)


def wgrad_table(s, math, N, hw, w, blocks=("init", "ang", "spa", "upsample")):
    calls = wgrad_calls(s)
    return {(Co, Ci, taps, tok): wgrad(Co, Ci, taps, math, N if tok == "N" else hw, w) for b in blocks for Co, Ci, taps, tok in calls[b]}


def wgrad_kernels(s, math, N, hw, w, blocks=("init", "ang", "spa", "upsample")):
    """{(NI, TX, fast3 taken by some wave, general form taken by some wave)}"""
    out = set()
    for g in wgrad_table(s, math, N, hw, w, blocks).values():
        if g.fast3 != "none":
            out.add(g.kernel + ("fast3",))
        if g.fast3 != "all":
            out.add(g.kernel + ("general",))
    return out


def ln_bwd_blocks(N):
    """(workgroups of k_ln_bwd, capped): capped = the grid is kLnBlocks and a workgroup's 16 token slots loop over several tokens."""
    want = (N + 15) // 16
    return min(K_LN_BLOCKS, want), want > K_LN_BLOCKS


def conv0_wgrad_per_wave(N):
    """k_conv0_wgrad: tokens per wave of its fixed kTailWaves waves, and how many waves have any."""
    per = (N + K_TAIL_WAVES - 1) // K_TAIL_WAVES
    return per, (N + per - 1) // per


def ang_attn_vp(A):
    """k_ang_attn<VP>: 32 up to 32 views (A <= 5), 128 above."""
    return 32 if A * A <= 32 else 128


def tokens(A, s, B, h, w):
    return B * A * A * h * w


def all_lin_kernels(s):
    """Every GEMM variant the model can produce at scale s: N over every 32-token tile count up to the ring threshold, N = 65 536,
    two sizes above it; views 32 wide or not (N a multiple of 32 leaves w free: B A^2 h is any integer)."""
    out = set()
    for N in [32 * t for t in range(1, RING_N // 32 + 1)] + [RING_N + 32, 4 * RING_N]:
        for w in (32, 10):
            out |= lin_kernels(s, N, min(N, 1024), w)
    return out


# ---- the size-class cases of tests/test_gpu_train_classes.py: (A, s, B, h, w), the blocks compared with the fp64 reference ----
ALL_BLOCKS = ("upsample", "spa", "ang", "init")
GPU_CASES = [
    ((2, 2, 1, 32, 32), ALL_BLOCKS),        # 4 096: 32-wide views under k_lin<1>; fast3 on its own
    ((5, 2, 16, 10, 10), ALL_BLOCKS),       # 40 000: mixed k_lin<1|2|4>, wgrad chunking with empty chunks, LayerNorm backward at its cap
    ((8, 4, 16, 8, 8), ALL_BLOCKS),         # 65 536: the last size before the ring, 4x, 64 views
    ((11, 2, 6, 10, 10), ALL_BLOCKS),       # 72 600: generic ring, ragged last workgroup, 121 views
    ((5, 2, 3, 32, 32), ALL_BLOCKS),        # 76 800: the benchmark's training shape: k_linr<.., KS 4 / 8>, fast3 at size
    ((6, 4, 2, 31, 31), ("upsample", "init")),   # 69 192: 4x above the ring threshold; 961-token views
]
MATHS = ("fp32", "bf16x3", "bf16x6")
KL, KR = "k_lin", "k_linr"


def case_classes(shape, blocks=ALL_BLOCKS):
    """What the case reaches in the blocks it compares: GEMM variants, weight-gradient tables per math mode, the caps."""
    A, s, B, h, w = shape
    N = tokens(*shape)
    return dict(N=N, lin=lin_table(s, N, h * w, w, blocks), kernels=lin_kernels(s, N, h * w, w, blocks),
                wg={m: wgrad_table(s, m, N, h * w, w, blocks) for m in MATHS},
                wg_kernels=set().union(*(wgrad_kernels(s, m, N, h * w, w, blocks) for m in MATHS)),
                ln=ln_bwd_blocks(N), conv0=conv0_wgrad_per_wave(N), vp=ang_attn_vp(A))


def check_case(shape):
    """The classes each case was chosen for (the table of the issue that introduced them); raises AssertionError when a constant of
    the host code has moved the case elsewhere."""
    c = case_classes(shape, dict(GPU_CASES)[shape])
    A, s, B, h, w = shape
    N, lin, wg = c["N"], c["lin"], c["wg"]
    big = lambda m, f: max(getattr(g, f) for g in wg[m].values())     # noqa: E731
    if shape == (2, 2, 1, 32, 32):
        assert N == 4096 and c["kernels"] == {(KL, 1, True), (KL, 1, False)}
        for m in MATHS:
            assert all(g.nch == 16 and g.empty == 0 and g.partial == 0 for k, g in wg[m].items() if k[3] == "N")
            assert all(g.fast3 == "all" for k, g in wg[m].items() if k[2] == 9) and all(g.fast3 == "none" for k, g in wg[m].items() if k[2] == 1)
        assert c["ln"] == (256, False) and c["vp"] == 32
    elif shape == (5, 2, 16, 10, 10):
        assert N == 40000 and c["kernels"] == {(KL, nt, t) for nt in (1, 2, 4) for t in (True, False)}
        assert lin[("upm_b", 0, "N")].kernel == (KL, 4, False) and lin[("mlp_f", 0, "N")].kernel == (KL, 2, False)
        assert big("fp32", "nch") == 156 and big("fp32", "empty") == 31 and big("fp32", "partial") == 1 and big("bf16x3", "partial") == 1
        assert wg["fp32"][(64, 64, 1, "N")] == Wg((2, 1), 156, 320, 31, 0, 0, 0, "none")
        assert c["ln"] == (512, True) and c["vp"] == 32
    elif shape == (8, 4, 16, 8, 8):
        assert N == RING_N and not any(l.ring for l in lin.values())
        assert all(l.nt == (2 if nOT_of(s, k) == 2 else 4) for k, l in lin.items() if k[2] == "N")
        assert lin[("mlp_f", 0, "N")].kernel == (KL, 4, False) and lin[("conv_f", 0, "N")].kernel == (KL, 2, False)
        assert lin[("up_f", 0, "N")].kernel == (KL, 4, True) and views(s)["upm"].OT == 2 and lin[("upm", 0, "N")].kernel == (KL, 2, True)
        assert c["vp"] == 128 and A * A == 64 and c["ln"] == (512, True)
    elif shape == (11, 2, 6, 10, 10):
        assert N == 72600 and N % 128 == 24 and c["vp"] == 128
        assert c["kernels"] == {(KR, 2, 0), (KR, 4, 0), (KL, 1, False)}
        assert {k for k, l in lin.items() if not l.ring} == {("upm", 0, "N"), ("mlp_f", 0, "hw")}
        assert big("fp32", "empty") == 56 and big("fp32", "nch") == 283 and big("fp32", "partial") == 1
    elif shape == (5, 2, 3, 32, 32):
        assert N == 76800 and c["kernels"] == {(KR, 2, 0), (KR, 4, 0), (KR, 2, 4), (KR, 2, 8), (KR, 4, 4), (KL, 1, False)}
        assert lin[("conv_f", 0, "N")].kernel == lin[("conv_b", 0, "N")].kernel == (KR, 2, 4)
        assert lin[("mlp_f", 0, "N")].kernel == (KR, 4, 4) and lin[("mlp_b", 0, "N")].kernel == (KR, 2, 8)
        for m in MATHS:
            assert all(g.fast3 == "all" for k, g in wg[m].items() if k[2] == 9)
        assert big("fp32", "nch") == 300 and big("fp32", "empty") == 20
    elif shape == (6, 4, 2, 31, 31):
        assert N == 69192 and (h * w) % 32 != 0 and c["kernels"] == {(KR, 2, 0), (KR, 4, 0)}
        assert lin[("upm", 0, "N")] == Lin(2, True, False, 0, (KR, 2, 0)) and views(s)["upm"].OT == 2     # the "last group of two" form
        assert big("fp32", "empty") == 15 and big("fp32", "partial") == 1
    else:
        raise AssertionError(f"no class table for {shape}")
    return c


def nOT_of(s, key):
    """Output tiles of the request `key` = (view, ot0, tokens) of LIN_CALLS."""
    for calls in LIN_CALLS.values():
        for name, ot0, nOT, tok in calls:
            if (name, ot0, tok) == key:
                return nOT or views(s)[name].OT
    raise KeyError(key)
