"""The case tables of the F(m,7) and F(4x4,3x3) conv tests, each case with a TAG that says which launch it selects on the
256 CUs of an MI355X (tests/wino_reach.py: tag7 / tag4).  Plain tuples and strings: the CPU suite imports this module.

tests/test_wino_reach_cpu.py holds every tag to the restated launch decision and the tables together to the REQUIRED set
below; the GPU files run the geometries (the rows are the tuples those files have always run: a seed taken from a row's hash
stays what it was):

    WINO7_CASES, W7_*           tests/test_conv_gpu.py                 F(6,7) (wino_m = 0) and F(4,7)
    F87_GEOMETRIES, F87_*       tests/test_wino7_f8_gpu.py             F(8,7), launched without a scratch unless said
    NUMERICS7, CLAMP_CASES      tests/test_wino_numerics_gpu.py, test_wino7_f8_gpu.py: the element-wise bound and descriptor tests
    WINO4_CASES, W4_*, HALF4    tests/test_conv_gpu.py                 F(4x4,3x3)
    PLANE_CASES                 tests/test_conv_gpu.py                 ... reading / writing channel planes
    PRELU_CASES                 tests/test_openpose_gpu.py             the PReLU epilogue in every form (rows of other forms too)
    SLICES                      tests/conv_slices.py                   the Winograd rows of TINY_F32 / LARGE_F32
    REACH7, REACH4              tests/test_wino_reach_gpu.py           the cases that fill what the tables above leave out
"""
from collections import namedtuple

import conv_slices as cs
import wino_reach as wr

# k, wino_m (0 = the library's default F(6,7)), geometry, branches, input padding, epilogue, storage, scratch passed
Geo = namedtuple("Geo", "k m n h w cin cout groups pad_in pool prelu planes scratch", defaults=(1, None, 0, 0, 0, True))

S1I, S1F = "wino7s_f32<1> image plain", "wino7s_f32<1> flat plain"
S2I, S2F = "wino7s_f32<2> image plain", "wino7s_f32<2> flat plain"


def t7(ni, gxt, fm, strips, launch):
    return "wino7_f32<%d,%d,%d,%d> %s %s" % (ni, gxt, fm, 2 if (fm == 6 and ni == 1) else 1, strips, launch)


# ---- tests/test_conv_gpu.py: F(6,7) and F(4,7) -------------------------------------------------------------------------------
WINO7_CASES = [
    # tag; n, h, w, cin (packed), cout, relu, pad_in, pad_out      (k = 7; wino_m = 0: F(6,7), groups of 6 pixels)
    (S1I, (2, 46, 46, 128, 128, 1, 3, 3)),      # Mconv2_stageN's map, 8 position groups per row (W % 6 == 4), strips per image
    (S1I, (1, 46, 49, 192, 128, 1, 3, 3)),      # ski.jpg geometry (46x49), 185 -> 192 packed input, W % 6 == 1
    (S1F, (3, 23, 18, 64, 256, 0, 3, 0)),       # W % 6 == 0, two N tiles, no ReLU, strips crossing images
    (S1F, (5, 6, 7, 16, 128, 1, 3, 3)),         # tiny maps: a block spans several images (W % 6 == 1)
    (S1F, (2, 20, 27, 32, 128, 1, 3, 3)),       # W % 6 == 3
    (S1F, (1, 17, 35, 8, 128, 0, 3, 1)),        # W % 6 == 5, one chunk
    (S1F, (1, 30, 44, 24, 128, 1, 3, 0)),       # W % 6 == 2
    (S1I, (1, 70, 66, 128, 128, 1, 3, 0)),      # multi-scale map, wider rows
    (S1F, (1, 9, 80, 8, 128, 1, 4, 1)),         # one chunk; 14 groups per row; gap wider than the padding
]
W7_STAGE = (2, 46, 46, 128, 128)                # n, h, w, cin, cout: two branches in one grid
W7_PERSIST = (12, 46, 46, 128, 128)             # two branches: 288 tiles
W7_PERSIST_HEAD = 3                             # ... its first images alone
W7_F47_BIG = (14, 46, 46, 128, 128)             # F(4,7), two branches: 504 tiles

# ---- tests/test_wino7_f8_gpu.py: F(8,7) -------------------------------------------------------------------------------------
F87_GEOMETRIES = [
    # tag; n, h, w, cin, cout, relu      (no scratch; the last image runs alone as well: the same instance)
    (t7(1, 6, 8, "image", "plain"), (2, 46, 46, 128, 128, 1)),     # 6 position groups per row, strips per image
    (t7(1, 6, 8, "image", "plain"), (1, 45, 45, 32, 128, 1)),      # W % 8 == 5: the last group's segments are clamped
    (t7(1, 0, 8, "flat", "plain"), (2, 30, 45, 64, 128, 0)),       # < 256 positions per image: one flat strip space, no ReLU
    (t7(1, 0, 8, "flat", "plain"), (2, 40, 47, 32, 128, 1)),       # W % 8 == 7
    (t7(1, 0, 8, "flat", "plain"), (5, 6, 7, 16, 128, 1)),         # tiny maps, one group per row: a strip spans several images
    (t7(2, 0, 8, "image", "plain"), (2, 20, 100, 32, 128, 1)),     # 13 groups per row: two transform items per thread
    (t7(1, 0, 8, "flat", "plain"), (3, 1, 46, 24, 128, 0)),        # H = 1
    (t7(1, 0, 8, "flat", "plain"), (4, 5, 23, 40, 256, 1)),        # H = 5, two column tiles
]
F87_STAGE_IN = (2, 46, 46, 185, 128)            # n, h, w, cin (packed to 192), cout: two branches
F87_PERSIST = (15, 46, 46, 128, 128)            # two branches: 15 x 9 strips x 2 = 270 tiles
F87_PERSIST_PART = (6, 8)                       # ... images [6, 8) alone: 36 tiles

NUMERICS7 = (2, 46, 46, 128, 128)               # n, h, w, cin, cout of the element-wise bound tests, one branch

# tests/test_wino_numerics_gpu.py, test_reads_past_the_tensor_are_clamped_by_the_buffer_descriptor (rtpose_conv2d_winograd: no
# scratch).  tag (None: F(2x2,3x3)); k, form (3: F(2x2,3x3), 43: F(4x4,3x3), 4 / 6: F(m,7)), (n, cin, cout, h, w)
CLAMP_CASES = [
    (None, (3, 3, (1, 32, 128, 10, 13))),
    (S1F, (7, 6, (1, 32, 128, 10, 13))),
    ("wino7_f32<1,0,4,1> flat plain", (7, 4, (1, 32, 128, 10, 13))),
    ("small", (3, 43, (1, 32, 128, 10, 13))),
    ("plain<=CUs", (3, 43, (1, 32, 128, 200, 200))),          # 79 m tiles x 2 column tiles: one round of 32 x 64 tiles
    ("persistent+small", (3, 43, (2, 32, 128, 184, 184))),    # 133 x 2 = 266 tiles: one round of 128 m tiles + 5 in the small form
]

# ---- tests/test_conv_gpu.py: F(4x4,3x3) --------------------------------------------------------------------------------------
WINO4_CASES = [
    # tag; n, h, w, cin (packed), cout, relu, pool, pad_in, pad_out
    ("small", (2, 46, 46, 256, 512, 1, 0, 1, 1)),            # conv4_1: 8 column tiles, H, W % 4 == 2 (clamped patch rows / columns)
    ("small", (1, 46, 46, 128, 128, 1, 0, 3, 1)),            # stage-1 conv reading the P = 3 concat layout
    ("small pool", (3, 96, 80, 64, 64, 1, 1, 1, 1)),         # conv1_2 shape: fused pool, one column tile
    ("small", (1, 100, 92, 128, 256, 1, 0, 1, 1)),           # H, W % 4 == 0
    ("small", (2, 45, 47, 32, 64, 0, 0, 1, 0)),              # odd sizes (W % 4 == 3, H % 4 == 1), no ReLU, 4 chunks
    ("small", (5, 7, 9, 48, 24, 1, 0, 1, 3)),                # tiny maps: a block spans several images; ragged cout; 6 chunks
    ("small pool", (1, 30, 44, 80, 128, 1, 1, 2, 0)),        # pool with H % 4 == 2; gap wider than the padding
    ("persistent+half", (40, 46, 46, 64, 128, 1, 0, 1, 1)),  # 180 m tiles x 2 column tiles: one round + 52 m tiles as half tiles
]
# the fixed geometries of the batch-invariance, small-grid and half-tile tests: n, h, w, cin, cout
W4_STAGE = (2, 46, 46, 128, 128)                # two branches
W4_ODD = (3, 45, 47, 64, 64)
W4_CONV4_1 = (9, 46, 46, 256, 512)
W4_POOLED = (20, 96, 80, 64, 64)                # fused pool
W4_TWO_BRANCH = (40, 45, 47, 128, 128)          # two branches
W4_STAGE1_BENCH = (32, 46, 46, 128, 128)        # two branches
HALF4 = [
    # tag; n, h, w, cin, cout, groups
    ("persistent+half", (32, 92, 92, 32, 256, 1)),
    ("persistent+half", (32, 46, 46, 64, 512, 1)),
    ("persistent+half", (32, 45, 47, 64, 256, 2)),
]
PLANE_CASES = [
    # tag; n, h, w, cin, cout, relu, pool, pad_in, pad_out, groups
    ("small planes", (2, 46, 46, 64, 128, 1, 0, 1, 1, 1)),
    ("persistent+half planes", (40, 46, 46, 64, 128, 1, 0, 1, 1, 1)),
    ("small pool planes", (3, 96, 80, 64, 64, 1, 1, 1, 1, 1)),        # fused pool
    ("small planes", (5, 7, 9, 48, 24, 0, 0, 1, 3, 1)),               # tiny maps, ragged cout (24 = 3 planes), no ReLU
    ("persistent+half planes", (20, 45, 47, 128, 128, 1, 0, 3, 3, 2)),  # two branches in one grid, odd sizes, one round + 26 m tiles
    ("persistent+half planes", (32, 92, 92, 32, 256, 1, 0, 1, 1, 1)),   # 8.27 rounds: 8 whole rounds + 17 m tiles as half tiles
]

# ---- tests/test_openpose_gpu.py: the PReLU epilogue in every form -------------------------------------------------------------
PRELU_CASES = [
    # tag (None: not a form of this file); n, h, w, cin, cout, k, form (0 direct, 2 F(2x2,3x3), 4 F(4x4,3x3)), planes
    (None, (2, 23, 19, 64, 96, 3, 0, False)),      # direct 3x3 (conv_mfma_f32), padded columns
    (None, (1, 46, 46, 128, 128, 3, 0, False)),
    (None, (2, 21, 17, 384, 512, 1, 0, False)),    # direct 1x1 (Mconv6)
    (None, (2, 23, 19, 96, 96, 3, 2, False)),      # F(2x2,3x3), small grid: wino3s_f32
    (None, (4, 46, 46, 128, 128, 3, 2, False)),    # ... 67 m tiles: still wino3s_f32
    (None, (16, 46, 46, 128, 128, 3, 2, False)),   # F(2x2,3x3), 265 m tiles: persistent wino_f32<1, 4, 16>
    (None, (16, 46, 46, 96, 96, 3, 2, False)),     # ... 96 columns padded to 128
    ("small prelu", (1, 23, 19, 288, 96, 3, 4, False)),
    ("small prelu", (8, 46, 46, 128, 128, 3, 4, False)),              # 36 m tiles x 2 column tiles
    ("small prelu planes", (8, 46, 46, 128, 128, 3, 4, True)),
    ("plain<=CUs prelu", (16, 46, 46, 128, 128, 3, 4, False)),        # 72 x 2 tiles
    ("plain<=CUs prelu planes", (16, 46, 46, 128, 128, 3, 4, True)),
    ("persistent+half prelu", (37, 46, 46, 128, 128, 3, 4, False)),   # 167 x 2 tiles: one round + 39 m tiles
    ("persistent+small prelu planes", (33, 46, 46, 128, 128, 3, 4, True)),   # 149 x 2 tiles: one round + 21 m tiles
]

# ---- tests/conv_slices.py: the Winograd rows of TINY_F32 (k, m, n, h, w, cin, cout, ...) and LARGE_F32 --------------------------
SLICES = {
    (3, 4, 5, 7, 9, 48, 24, 1, 0, 0): ["small"],
    (7, 4, 5, 6, 7, 16, 128, 1, 0, 0): [t7(1, 0, 4, "flat", "plain")],
    (7, 6, 5, 6, 7, 16, 128, 1, 0, 0): [S1F],
    (7, 8, 5, 6, 7, 16, 128, 1, 0, 0): [t7(1, 0, 8, "flat", "plain")],
    (7, 4, 1, 17, 35, 8, 128, 0, 0, 0): [t7(1, 0, 4, "flat", "plain")],
    (7, 6, 1, 17, 35, 8, 128, 0, 0, 0): [S1F],
    (7, 8, 1, 17, 35, 8, 128, 0, 0, 0): [t7(1, 0, 8, "flat", "plain")],
    # LARGE_F32 (k, m, n, h, w, cin, cout, relu, pool, groups): F(m,7) with a scratch, then without
    (3, 4, 40, 46, 46, 64, 128, 1, 0, 1): ["persistent+half"],
    (7, 4, 12, 46, 46, 128, 128, 1, 0, 2): [t7(1, 12, 4, "image", "persistent"), t7(1, 12, 4, "image", "plain+remap")],
    (7, 6, 12, 46, 46, 128, 128, 1, 0, 2): [t7(1, 8, 6, "image", "persistent"), t7(1, 8, 6, "image", "plain+remap")],
    # F(8,7): 12 x 9 strips x 2 = 216 tiles < 256 CUs: one block per tile with or without a scratch
    (7, 8, 12, 46, 46, 128, 128, 1, 0, 2): [t7(1, 6, 8, "image", "plain+remap"), t7(1, 6, 8, "image", "plain+remap")],
}

# ---- tests/test_wino_reach_gpu.py ---------------------------------------------------------------------------------------------
# F(m,7): cin 16 (two chunks), two branches unless said, pad_in 3.  tag; m, n, h, w, cout, groups
REACH7 = [
    # F(6,7)
    (S2I, (6, 1, 20, 80, 256, 2)),                                     # 14 groups per row, 10 rows of a strip: two items per thread
    (S2F, (6, 2, 5, 80, 256, 2)),                                      # 14 groups per row, a strip reaches into the next image
    (t7(1, 8, 6, "image", "plain"), (6, 3, 46, 46, 256, 2)),           # 36 strips x 4: the 46-wide instance in plain block order
    (t7(1, 0, 6, "flat", "plain"), (6, 11, 20, 27, 256, 2)),
    (t7(1, 0, 6, "flat", "persistent"), (6, 21, 20, 27, 256, 2)),
    (t7(1, 0, 6, "flat", "plain+remap"), (6, 43, 12, 20, 128, 2)),
    (t7(1, 0, 6, "image", "plain"), (6, 3, 46, 49, 256, 2)),           # the ski.jpg map
    (t7(1, 0, 6, "image", "persistent"), (6, 5, 46, 49, 256, 2)),
    (t7(2, 0, 6, "image", "plain"), (6, 4, 20, 80, 256, 2)),
    (t7(2, 0, 6, "image", "persistent"), (6, 8, 20, 80, 256, 2)),
    (t7(2, 0, 6, "image", "plain+remap"), (6, 6, 23, 80, 128, 2)),
    (t7(2, 0, 6, "flat", "plain"), (6, 15, 5, 80, 256, 2)),
    (t7(2, 0, 6, "flat", "persistent"), (6, 30, 5, 80, 256, 2)),
    (t7(1, 0, 6, "flat", "plain+remap"), (6, 21, 20, 27, 100, 2)),     # ragged cout: 100 columns stored of 128
    # F(4,7)
    (t7(1, 0, 4, "flat", "persistent"), (4, 21, 20, 27, 256, 2)),
    (t7(1, 0, 4, "flat", "plain+remap"), (4, 45, 5, 33, 128, 2)),
    (t7(1, 0, 4, "image", "plain"), (4, 1, 30, 33, 128, 1)),
    (t7(1, 0, 4, "image", "persistent"), (4, 6, 46, 27, 256, 2)),
    (t7(2, 0, 4, "image", "plain"), (4, 3, 46, 49, 256, 2)),
    (t7(2, 0, 4, "image", "persistent"), (4, 5, 46, 49, 256, 2)),
    (t7(2, 0, 4, "image", "plain+remap"), (4, 5, 30, 49, 128, 2)),
    (t7(2, 0, 4, "flat", "plain"), (4, 2, 5, 80, 128, 1)),
    (t7(2, 0, 4, "flat", "persistent"), (4, 32, 5, 49, 256, 2)),
    # F(8,7)
    (t7(1, 0, 8, "flat", "persistent"), (8, 46, 9, 33, 256, 2)),
    (t7(1, 0, 8, "image", "plain"), (8, 3, 46, 49, 256, 2)),
    (t7(1, 0, 8, "image", "persistent"), (8, 6, 46, 49, 256, 2)),
    (t7(1, 0, 8, "image", "plain+remap"), (8, 6, 46, 49, 128, 2)),
    (t7(2, 0, 8, "image", "persistent"), (8, 5, 30, 100, 256, 2)),
    (t7(2, 0, 8, "image", "plain+remap"), (8, 5, 30, 100, 128, 2)),
    (t7(2, 0, 8, "flat", "plain"), (8, 4, 20, 80, 256, 2)),
    (t7(2, 0, 8, "flat", "persistent"), (8, 32, 5, 100, 256, 2)),
]
REACH7_CIN, REACH7_PAD = 16, 3

# F(4x4,3x3): cin 32 (four chunks, the fewest the form takes is two of 16), pad_in 1.  tag; n, h, w, cout, groups, pool, prelu
REACH4 = [
    ("plain<=CUs", (10, 46, 46, 192, 1, 0, 0)),           # 45 m tiles x 3 column tiles = 135 blocks
    ("plain>CUs", (20, 46, 46, 192, 1, 0, 0)),            # 90 x 3 = 270 tiles, 256 % (8 x 3) != 0: one block per tile, XCD order
    ("plain>CUs prelu", (20, 46, 46, 192, 1, 0, 1)),
    ("persistent", (23, 30, 44, 512, 1, 0, 0)),           # 64 m tiles x 8 column tiles: two whole rounds of 32 blocks per column tile
    ("persistent prelu", (23, 45, 47, 128, 2, 0, 1)),     # two branches, 104 m tiles x 4: a whole round + 40 of 64: too many for a rest
    ("persistent+half pool", (9, 46, 46, 512, 1, 1, 0)),  # 41 m tiles x 8: one round + 9 m tiles as half tiles, pooled
]
REACH4_CIN, REACH4_PAD = 32, 1


# ---- every tagged launch of the tables as (where, tag, Geo) -------------------------------------------------------------------
def all_cases():
    out = []
    for tag, (n, h, w, cin, cout, _relu, pin, _pout) in WINO7_CASES:
        out.append(("WINO7_CASES", tag, Geo(7, 0, n, h, w, cin, cout, pad_in=pin)))
    n, h, w, cin, cout = W7_STAGE
    out += [("W7_STAGE", S1I, Geo(7, 0, n, h, w, cin, cout, 2, 3)),
            ("W7_STAGE F(6,7)", S1I, Geo(7, 6, n, h, w, cin, cout, 2, 3)),
            ("W7_STAGE F(4,7)", t7(1, 12, 4, "image", "plain"), Geo(7, 4, n, h, w, cin, cout, 2, 3))]
    n, h, w, cin, cout = W7_PERSIST
    out += [("W7_PERSIST", t7(1, 8, 6, "image", "persistent"), Geo(7, 0, n, h, w, cin, cout, 2, 3)),
            ("W7_PERSIST no scratch", t7(1, 8, 6, "image", "plain+remap"), Geo(7, 0, n, h, w, cin, cout, 2, 3, scratch=False)),
            ("W7_PERSIST_HEAD", S1I, Geo(7, 0, W7_PERSIST_HEAD, h, w, cin, cout, 2, 3))]
    n, h, w, cin, cout = W7_F47_BIG
    out += [("W7_F47_BIG", t7(1, 12, 4, "image", "persistent"), Geo(7, 4, n, h, w, cin, cout, 2, 3)),
            ("W7_F47_BIG no scratch", t7(1, 12, 4, "image", "plain+remap"), Geo(7, 4, n, h, w, cin, cout, 2, 3, scratch=False))]
    for tag, (n, h, w, cin, cout, _relu) in F87_GEOMETRIES:
        out += [("F87_GEOMETRIES", tag, Geo(7, 8, n, h, w, cin, cout, 1, 3, scratch=False)),
                ("F87_GEOMETRIES last image", tag, Geo(7, 8, 1, h, w, cin, cout, 1, 3, scratch=False))]
    n, h, w, cin, cout = F87_STAGE_IN
    out.append(("F87_STAGE_IN", t7(1, 6, 8, "image", "plain"), Geo(7, 8, n, h, w, 192, cout, 2, 3, scratch=False)))
    n, h, w, cin, cout = F87_PERSIST
    out += [("F87_PERSIST", t7(1, 6, 8, "image", "persistent"), Geo(7, 8, n, h, w, cin, cout, 2, 3)),
            ("F87_PERSIST no scratch", t7(1, 6, 8, "image", "plain+remap"), Geo(7, 8, n, h, w, cin, cout, 2, 3, scratch=False)),
            ("F87_PERSIST_PART", t7(1, 6, 8, "image", "plain"),
             Geo(7, 8, F87_PERSIST_PART[1] - F87_PERSIST_PART[0], h, w, cin, cout, 2, 3))]
    n, h, w, cin, cout = NUMERICS7
    out += [("NUMERICS7 F(4,7)", t7(1, 12, 4, "image", "plain"), Geo(7, 4, n, h, w, cin, cout, 1, 3)),
            ("NUMERICS7 F(6,7)", S1I, Geo(7, 6, n, h, w, cin, cout, 1, 3)),
            ("NUMERICS7 F(8,7)", t7(1, 6, 8, "image", "plain"), Geo(7, 8, n, h, w, cin, cout, 1, 3, scratch=False))]
    for tag, (k, form, (n, cin, cout, h, w)) in CLAMP_CASES:
        if tag is not None:
            out.append(("CLAMP_CASES", tag, Geo(k, 4 if form == 43 else form, n, h, w, cin, cout, 1, k // 2, scratch=False)))
    for tag, (n, h, w, cin, cout, _relu, pool, pin, _pout) in WINO4_CASES:
        out.append(("WINO4_CASES", tag, Geo(3, 4, n, h, w, cin, cout, 1, pin, pool)))
    # (name, geometry, pool, branches, tag, images that also run alone beside the batch: the 16 x 16 form)
    for name, g, pool, groups, tag, alone in (
            ("W4_STAGE", W4_STAGE, 0, 2, "small", 0), ("W4_ODD", W4_ODD, 0, 1, "small", 1),
            ("W4_CONV4_1", W4_CONV4_1, 0, 1, "persistent+half", 1), ("W4_POOLED", W4_POOLED, 1, 1, "persistent+small pool", 1),
            ("W4_TWO_BRANCH", W4_TWO_BRANCH, 0, 2, "persistent", 2), ("W4_STAGE1_BENCH", W4_STAGE1_BENCH, 0, 2, "persistent+small", 2)):
        n, h, w, cin, cout = g
        out.append((name, tag, Geo(3, 4, n, h, w, cin, cout, groups, 1, pool)))
        if alone:
            out.append((name + " alone", "small" + (" pool" if pool else ""), Geo(3, 4, alone, h, w, cin, cout, groups, 1, pool)))
    for tag, (n, h, w, cin, cout, groups) in HALF4:
        out += [("HALF4", tag, Geo(3, 4, n, h, w, cin, cout, groups, 1)),
                ("HALF4 alone", "small", Geo(3, 4, 1, h, w, cin, cout, groups, 1))]
    for tag, (n, h, w, cin, cout, _relu, pool, pin, _pout, groups) in PLANE_CASES:
        out.append(("PLANE_CASES", tag, Geo(3, 4, n, h, w, cin, cout, groups, pin, pool, planes=1)))
    for tag, (n, h, w, cin, cout, k, form, planes) in PRELU_CASES:
        if tag is not None:
            out.append(("PRELU_CASES", tag, Geo(3, 4, n, h, w, cin, cout, 1, 1, prelu=1, planes=int(planes))))
    for row, tags in SLICES.items():
        k, m, n, h, w, cin, cout = row[:7]
        groups = row[9] if row in cs.LARGE_F32 else 1
        for tag, scratch in zip(tags, (True, False)):
            out.append(("SLICES", tag, Geo(k, m, n, h, w, cin, cout, groups, k // 2, scratch=scratch)))
    for tag, (m, n, h, w, cout, groups) in REACH7:
        out.append(("REACH7", tag, Geo(7, m, n, h, w, REACH7_CIN, cout, groups, REACH7_PAD)))
    for tag, (n, h, w, cout, groups, pool, prelu) in REACH4:
        out.append(("REACH4", tag, Geo(3, 4, n, h, w, REACH4_CIN, cout, groups, REACH4_PAD, pool, prelu)))
    return out


def tag_of(g, cus=wr.CUS):
    """the tag the restated launch decision gives a case at `cus` CUs"""
    if g.k == 7:
        return wr.tag7(wr.reach7(g.n, g.h, g.w, g.cin, g.cout, g.groups, g.h + g.pad_in, g.m or 6, cus, g.scratch))
    return wr.tag4(wr.reach4(g.n, g.h, g.w, g.cin, g.cout, g.groups, cus, g.prelu), g.prelu, g.pool, g.planes)


# ---- what the tables together have to reach, with no allowance -----------------------------------------------------------------
def required7():
    """Every instance conv2d_wino7_launch can return: in each strip mode it occurs in, one block per tile and persistent; and each
    main-kernel instance in both block orders of the one-block-per-tile grid (the persistent walk and the small-grid kernel
    order their blocks themselves).  The compile-time GX instances exist with strips per image only."""
    req = {S1I, S1F, S2I, S2F}
    either = set()
    for fm in (4, 6, 8):
        for ni, gxt, modes in ((1, wr.GXT[fm], ("image",)), (1, 0, ("flat", "image")), (2, 0, ("flat", "image"))):
            for strips in modes:
                req.add(t7(ni, gxt, fm, strips, "persistent"))
                either.add((t7(ni, gxt, fm, strips, "plain"), t7(ni, gxt, fm, strips, "plain+remap")))
            inst = t7(ni, gxt, fm, "", "").split()[0]
            for order in ("plain", "plain+remap"):
                either.add(tuple("%s %s %s" % (inst, strips, order) for strips in modes))
    return req, either


def required4():
    """The six launch shapes, each without and with PReLU; pool and planes each on the small form and on both kinds of rest.
    (shape, word): a case of that shape whose tag has the word; (shape, None): one without PReLU."""
    req = [(s, None) for s in wr.SHAPES4] + [(s, "prelu") for s in wr.SHAPES4]
    req += [(s, word) for word in ("pool", "planes") for s in ("small", "persistent+small", "persistent+half")]
    return req
