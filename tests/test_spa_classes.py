"""CPU check of tests/spa_classes.py against figures worked out BY HAND from the constants of lft_amd/csrc (no GPU, no library).

Sizes in bytes.  pieces(n, per) = ceil(n / per) KiB-sized LDS-DMA pieces of the conv input tile, which holds 130 + 2 w token rows
(ConvIn::slots: the 128 tokens of the tile, one image row and one token on either side): 4 rows per piece in fp32, 8 in 16 bit.

k_spa1 (lds_spa1 = ring + max(input tile, 4 x TileIO<4>) + 1024 + 256; the ring is 3 chunks of CH fragments of 2 KiB fp32 / 1 KiB):
  fp32    CH 16: 98 304 + tile + 1 280 is above 80 KiB (two workgroups per CU) at every width, and so is CH 8 (49 152 + tile + 1 280
          with a tile of at least 33 KiB), so launch_spa1 keeps 16 until it no longer fits at all:
          tile <= 163 840 - 99 584 = 64 256 -> 62 pieces -> 130 + 2 w <= 248 -> w <= 59, where it holds 163 072 of 163 840 B.
          From w = 60: CH 8, 50 432 + tile <= 163 840 -> 110 pieces -> 130 + 2 w <= 440 -> w <= 155.
  16 bit  CH 16: 49 152 + tile + 1 280 <= 81 920 -> tile <= 31 488 -> 30 pieces -> 130 + 2 w <= 240 -> w <= 55 (81 152 B).
          From w = 56: CH 8, 24 576 + tile + 1 280 <= 81 920 -> 54 pieces -> 130 + 2 w <= 432 -> w <= 151.
          From w = 152 neither shares a CU and launch_spa1 returns to CH 16 while it fits: 110 pieces -> w <= 375; then CH 8 again
          up to 134 pieces -> 130 + 2 w <= 1 072 -> w <= 471.
Front end (lds_conv64 = 3 x 12 fragments + tile + 4 x TileIO<2> + 256):
  fp32    73 728 + tile + 17 408 + 256 <= 163 840 -> tile <= 72 448 -> 70 pieces -> 130 + 2 w <= 280 -> w <= 75 (163 072 B).
  16 bit  36 864 + tile + 9 216 + 256 + LrStage, LrStage = 8 rows x (w + 4) x 4 B for w >= 130.
          w = 347: 824 rows -> 103 pieces = 105 472; 151 808 + 11 232 = 163 040.   w = 348: 826 rows -> 104 pieces; 164 096 > 163 840.
"""
import pytest

import spa_classes as S


def test_spa1_chunk_switch():
    assert S.spa1_chunk("fp32", 59) == (16, 163072) and S.spa1_chunk("fp32", 60) == (8, 114944)
    assert S.spa1_chunk("bf16", 55) == (16, 81152) and S.spa1_chunk("bf16", 56) == (8, 57600)
    assert S.spa1_chunk("fp16", 55) == S.spa1_chunk("bf16", 55) and S.spa1_chunk("fp16", 56) == S.spa1_chunk("bf16", 56)
    assert all(S.spa1_chunk("fp32", w)[0] == 16 for w in range(1, 60)) and all(S.spa1_chunk("fp32", w)[0] == 8 for w in range(60, 156))
    assert all(S.spa1_chunk("bf16", w)[0] == 16 for w in range(1, 56)) and all(S.spa1_chunk("bf16", w)[0] == 8 for w in range(56, 152))
    # beyond two workgroups per CU the 16-bit launch returns to 16-fragment chunks while they fit
    assert S.spa1_chunk("bf16", 152)[0] == 16 and S.spa1_chunk("bf16", 375) == (16, 163072) and S.spa1_chunk("bf16", 376)[0] == 8
    assert max(S.spa1_chunk(p, w)[1] for p in ("fp32", "bf16") for w in range(1, 76) if S.spa1_chunk(p, w)[0]) == 163072
    assert S.spa1_chunk("fp32", 156)[0] is None and S.spa1_chunk("bf16", 472)[0] is None


def test_width_limits():
    assert S.front_end_w_max("fp32") == 75 and S.lds_front_end("fp32", 75) == 163072 and S.lds_front_end("fp32", 76) > S.K_MAX_LDS
    assert S.front_end_w_max("bf16") == S.front_end_w_max("fp16") == 347
    assert S.lds_front_end("bf16", 347) == 163040 and S.lds_front_end("bf16", 348) == 164096
    assert S.spa1_w_max("fp32") == 155 and S.spa1_w_max("bf16") == S.spa1_w_max("fp16") == 471
    for p in ("fp32", "bf16", "fp16"):       # the front end is the narrower of the two: weights still pack at its widest view
        assert S.front_end_w_max(p) < S.spa1_w_max(p)


@pytest.mark.parametrize("h,w,prec,lm", [(32, 32, "fp32", True), (32, 32, "bf16", True), (16, 24, "fp32", True), (16, 24, "fp16", False),
                                         (31, 32, "bf16", False), (31, 32, "fp32", False), (62, 64, "bf16", True), (8, 8, "fp32", False)])
def test_lane_major(h, w, prec, lm):
    assert S.tok_lane_major(h, w, prec) is lm


def test_tiles():
    c = S.classify(17, 19, "bf16")          # 323 tokens = 128 + 128 + 67; 17 rows = 4 x 4 + 1; 323 = 10 x 32 + 3
    assert (c.tiles, c.last_tile, c.tiles_x, c.tiles_y, c.last_cols, c.last_rows, c.straddle) == (3, 67, 1, 5, 19, 1, True)
    assert S.wave_valid(17, 19, 1) == (32, 32, 32, 32) and S.wave_valid(17, 19, 2) == (32, 32, 3, 0)
    c = S.classify(35, 37, "fp32")          # 1295 = 10 x 128 + 15; 37 = 32 + 5; 35 = 8 x 4 + 3
    assert (c.tiles, c.last_tile, c.tiles_x, c.tiles_y, c.last_cols, c.last_rows, c.straddle) == (11, 15, 2, 9, 5, 3, True)
    c = S.classify(62, 64, "fp16")          # 3968 = 31 x 128; 62 = 15 x 4 + 2
    assert (c.tiles, c.last_tile, c.tiles_x, c.tiles_y, c.last_cols, c.last_rows, c.straddle) == (31, 128, 2, 16, 32, 2, False)
    c = S.classify(6, 6, "fp32")            # one partial tile that starts at token 0
    assert (c.tiles, c.last_tile, c.tiles_x, c.tiles_y, c.last_cols, c.last_rows, c.straddle) == (1, 36, 1, 2, 6, 2, True)
    assert S.wave_valid(6, 6, 0) == (32, 4, 0, 0)
