"""Class model of the spatial path's shape-dependent dispatch (pure Python; no GPU, no library).

The front-end convolutions, k_spa1, k_spa_b / k_win_attn_lds + k_spa2 and k_up choose tiles, hand-off layouts and LDS ring chunks
from the view size (h, w) and the precision.  This module re-derives those choices from the constants of lft_amd/csrc
(lft_network.hip: tok_lane_major, launch_spa1, lds_conv64, lds_conv64_lr, lds_spa1; lft_host.cuh: allow_lds; lft_kernels_a.cuh: ConvIn, LrStage;
lft_common.cuh: WRing, TileIO), so that every view-size case of the parity tests can ASSERT the class it was chosen for: a later
change of a constant then fails the case's table instead of silently moving it into a class another case already covers.
tests/test_spa_classes.py pins the thresholds to values worked out by hand from the headers.
"""
from collections import namedtuple

K_MAX_LDS = 160 * 1024          # kMaxLds: a workgroup may use all the LDS of a CU
K_SPA_OCC = 2                   # kSpaOcc: k_spa1 workgroups per CU that launch_spa1 aims for
NW = 4                          # kNwConv = kNwSpa1: waves (x 32 tokens) per workgroup tile
TT = 32 * NW                    # tokens per workgroup tile of the convs and k_spa1
K_CONV64_CHUNK = 12             # kConv64Chunk
K_CONV_ZERO_ROW = 256           # kConvZeroRow
K_CONV0_W_BYTES = 9 * 64 * 4    # kConv0WBytes
K_LDS_PARAMS = 1024             # kLdsParams
ATT_TY, ATT_TX = 4, 32          # kAttTY, kAttTX: k_spa_b's query tile (rows x columns of one view image)
W_SEARCH = 4096                 # widths searched for the limits; far above every limit


def esz(prec):
    return 4 if prec == "fp32" else 2


def wring_bytes(prec, ch):
    """WRing<T, CH, NW>::LDS_BYTES: 3 slots of CH fragments of 1 KiB (16-bit) / 2 KiB (fp32)."""
    return 3 * ch * 1024 * (2 if prec == "fp32" else 1)


def conv_in_bytes(prec, w):
    """ConvIn<T, NW>::bytes(w): 32 NW + 2 + 2 w token rows of 64 channels, in whole 1 KiB LDS-DMA pieces."""
    per_piece = 1024 // (64 * esz(prec))
    return (TT + 2 + 2 * w + per_piece - 1) // per_piece * 1024


def tile_io_bytes(prec, nt):
    """TileIO<NT, T>::BYTES: 16 rows of NT * 32 elements, padded by 16 B."""
    return 16 * (nt * 32 * esz(prec) + 16)


def lr_stage_bytes(w):
    """LrStage<NW>::bytes(w)."""
    rows = (TT + 2 * w + 1) // w + 6
    return (rows * (w + 4) * 4 + 15) & ~15


def lds_conv64(prec, w):
    return wring_bytes(prec, K_CONV64_CHUNK) + conv_in_bytes(prec, w) + NW * tile_io_bytes(prec, 2) + K_CONV_ZERO_ROW


def lds_front_end(prec, w):
    """LDS of the front end's widest launch: fp32 k_conv64 (lds_conv64); 16-bit k_conv64_lr / k_conv64<T, 2> (lds_conv64_lr)."""
    if prec == "fp32":
        return lds_conv64(prec, w)
    return lds_conv64(prec, w) + max(lr_stage_bytes(w), K_CONV0_W_BYTES)


def lds_spa1(prec, w, ch):
    return wring_bytes(prec, ch) + max(conv_in_bytes(prec, w), NW * tile_io_bytes(prec, 4)) + K_LDS_PARAMS + K_CONV_ZERO_ROW


def spa1_chunk(prec, w):
    """(ring chunk, LDS bytes) of launch_spa1; chunk None where allow_lds refuses the width."""
    l16, l8 = lds_spa1(prec, w, 16), lds_spa1(prec, w, 8)
    share = K_MAX_LDS // K_SPA_OCC
    use8 = (l16 > share and l8 <= share) or l16 > K_MAX_LDS
    ch, lds = (8, l8) if use8 else (16, l16)
    return (ch if lds <= K_MAX_LDS else None), lds


def tok_lane_major(h, w, prec):
    return (h * w) % TT == 0 and (prec == "fp32" or w % 32 == 0)


def front_end_w_max(prec):
    return max(w for w in range(1, W_SEARCH) if lds_front_end(prec, w) <= K_MAX_LDS)


def spa1_w_max(prec):
    return max(w for w in range(1, W_SEARCH) if spa1_chunk(prec, w)[0] is not None)


SpaClass = namedtuple("SpaClass", "lane_major chunk lds_spa1 tiles last_tile tiles_x tiles_y last_cols last_rows straddle")


def classify(h, w, prec):
    """lane_major   the k_spa1 -> part B hand-off (and, inside lft_forward, last block -> k_up) is lane-major
    chunk        k_spa1's ring chunk (8 / 16);  lds_spa1  its LDS bytes
    tiles        128-token workgroup tiles per view image (convs, k_spa1);  last_tile  valid tokens of the last one
    tiles_x/_y   k_spa_b's 4 x 32 query tiles per image;  last_cols / last_rows  columns / rows of the last one
    straddle     h*w % 32 != 0: the flat 32-token tiles of k_spa2 / k_up straddle view images"""
    hw = h * w
    chunk, lds = spa1_chunk(prec, w)
    return SpaClass(lane_major=tok_lane_major(h, w, prec), chunk=chunk, lds_spa1=lds,
                    tiles=(hw + TT - 1) // TT, last_tile=hw - (hw - 1) // TT * TT,
                    tiles_x=(w + ATT_TX - 1) // ATT_TX, tiles_y=(h + ATT_TY - 1) // ATT_TY,
                    last_cols=w - (w - 1) // ATT_TX * ATT_TX, last_rows=h - (h - 1) // ATT_TY * ATT_TY,
                    straddle=hw % 32 != 0)


def wave_valid(h, w, tile):
    """Valid tokens of each of the 4 waves of 128-token tile `tile` of a view image (store_tile's nvalid)."""
    return tuple(max(0, min(32, h * w - (tile * TT + 32 * wv))) for wv in range(NW))
