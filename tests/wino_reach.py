"""Which kernel a Winograd conv launch runs: the host decisions of csrc/conv_wino7.hip (F(4,7) / F(6,7) / F(8,7)) and
csrc/conv_wino4.hip (F(4x4,3x3)) restated in plain Python - integers only, no library call, no torch, no numpy.

These two forms are the ones tests/conv_forward_exact.py cannot pin with exact integers (wino_proof), so their cases are
tolerance tests on chosen geometries, and a geometry only tests the kernel template it selects.  The selection is made on the
host from (N, H, W, cin, cout, groups, the device's CU count, whether the caller passed a hand-over scratch); `reach7` and
`reach4` repeat it, tests/wino_cases.py tags every case with what it selects, tests/test_wino_reach_cpu.py holds the tags and
`fits7` to the library, and tests/test_wino_reach_gpu.py asks each of its cases for its reach on the device it runs on.

What is restated, and where it stands (the source wins: when one of these changes, this file changes with it):

    csrc/common.h            kConvBN, cout_pad                                        -> cout_pad
    csrc/conv_desc.h         grid_ids (xcd_remap, padded ids)                         -> grid_ids
    csrc/conv_wino7.hip      CK, CG, row_stride, strip_rows (lines 159-169)           -> CK, CG, row_stride, strip_rows
                             make_plan (lines 930-960)                                -> plan7
                             conv2d_wino7_fits (lines 1110-1116)                      -> fits7
                             conv2d_wino7_launch: persistent form (1163-1180), small-grid form (1182-1190), the instance
                             ladders of F(6,7) / F(8,7) / F(4,7) (1191-1211)          -> reach7
                             wino7_f32 / wino7s_f32: which fields a launch reads      -> Reach7.remap_used
    csrc/conv_wino.hip       rtpose_conv2d_winograd_fits: wino_m, PReLU (831-841)     -> fits
    csrc/conv_wino4.hip      NT, NC, NTS (lines 119-120, 587), conv2d_wino4_ok (932)  -> NT4, NC4, NTS4, fits4
                             conv2d_wino4_launch: TY, TX, T, mtiles, ncombo (1039-1051), wino4_run (939-998) -> reach4
"""
from collections import namedtuple

CUS = 256                     # the MI355X: the CU count the case tags are written for

# ---- csrc/common.h -----------------------------------------------------------------------------------------------------------
BN = 64                       # kConvBN


def ceil_div(a, b):
    return -(-a // b)


def cout_pad(cout):
    return ceil_div(cout, BN) * BN


# ---- csrc/conv_desc.h: grid_ids ----------------------------------------------------------------------------------------------
def grid_ids(mtiles, ncombo):
    """(xcd_remap, block ids of the 1-D grid): the XCD-aware order pads the m tiles to a multiple of 8."""
    remap = 1 if (ncombo > 1 and mtiles >= 64) else 0
    return remap, (8 * ncombo * ceil_div(mtiles, 8) if remap else mtiles * ncombo)


# ---- csrc/conv_wino7.hip -----------------------------------------------------------------------------------------------------
CK, CG = 8, 2                 # channels per chunk, 16-byte channel groups per chunk
LDS7 = 156 * 1024             # conv2d_wino7_fits: the transformed rows of a block (two V buffers)
GXT = {6: 8, 8: 6, 4: 12}     # position groups per row of the compile-time instance of each form (46-wide maps)


def row_stride(gx, nfq):
    rs = nfq * CG * gx
    while (rs & 15) != (gx & 15):
        rs += 1
    return rs


def strip_rows(gx):
    return (31 + gx - 1) // gx + 1 + 6


Plan7 = namedtuple("Plan7", "fm nfq gx rs nrows ni tpi mtiles T lds crossing")


def plan7(N, H, W, hs, fm):
    """make_plan.  hs: rows from one image to the next in the INPUT layout (H + its padding).  None where make_plan fails
    (more than 2^31 - 1 positions).  `crossing`: a flat strip holds positions of two images (not a field of the source's Plan:
    an edge of the geometry)."""
    nfq = fm + 6
    gx = ceil_div(W, fm)
    rs = row_stride(gx, nfq)
    T = N * H * gx
    if T > 0x7fffffff:
        return None
    pi = H * gx
    tpi = ceil_div(pi, 32) if pi >= 256 else 0
    crossing = False
    if tpi:
        nrows = min(strip_rows(gx), H + 6)
        mtiles = N * tpi
    else:
        nrows = 0
        for t0 in range(0, T, 32):
            t1 = min(t0 + 31, T - 1)
            n0, n1 = t0 // pi, t1 // pi
            y0, y1 = (t0 - n0 * pi) // gx, (t1 - n1 * pi) // gx
            nrows = max(nrows, (n1 * hs + y1) - (n0 * hs + y0) + 7)
            crossing = crossing or n1 != n0
        mtiles = (T + 31) // 32
    return Plan7(fm, nfq, gx, rs, nrows, ceil_div(nrows * gx * CG, 256), tpi, mtiles, T, 2 * nrows * rs * 16, crossing)


def fits7(cin, cout, N, H, W, hs, fm):
    """conv2d_wino7_fits (fm resolved: 4, 6 or 8)"""
    if fm not in (4, 6, 8) or cin <= 0 or cin % CK or cout_pad(cout) % 128 or N <= 0 or H <= 0 or W <= 0:
        return 0
    p = plan7(N, H, W, hs, fm)
    return int(p is not None and p.ni <= 2 and p.lds <= LDS7)


# kernel: 'wino7s_f32<NI>' | 'wino7_f32<NI,GXT,FM,FS>'; strips: 'flat' | 'image'; second: always 'none' (one launch)
Reach7 = namedtuple("Reach7", "kernel strips persistent xcd_remap remap_used second ni blocks plan")


def reach7(N, H, W, cin, cout, groups, hs, fm, cus=CUS, scratch=True):
    """conv2d_wino7_launch for a geometry that fits.  scratch: the caller passed a hand-over scratch of
    rtpose_conv2d_winograd_scratch_bytes().  xcd_remap is the field as the host sets it; remap_used says whether the kernel
    reads it (the small-grid kernel and the persistent walk order their blocks themselves)."""
    assert fits7(cin, cout, N, H, W, hs, fm), "no F(%d,7) instance" % fm
    p = plan7(N, H, W, hs, fm)
    ncombo = cout_pad(cout) // 128 * groups
    remap, ids = grid_ids(p.mtiles, ncombo)
    tiles = p.mtiles * ncombo
    persistent = bool(tiles >= cus and tiles % cus != 0 and scratch)
    if persistent:
        ids = cus
    strips = "image" if p.tpi else "flat"
    if fm == 6 and not persistent and tiles * 2 <= cus:
        return Reach7("wino7s_f32<%d>" % p.ni, strips, False, remap, False, "none", p.ni, p.mtiles * (cout_pad(cout) // 32 * groups), p)
    g = GXT[fm]
    if p.gx == g and p.tpi and p.ni == 1 and p.nrows == strip_rows(g):
        inst = (1, g)
    else:
        inst = (p.ni, 0)
    fs = 2 if (fm == 6 and p.ni == 1) else 1
    return Reach7("wino7_f32<%d,%d,%d,%d>" % (inst + (fm, fs)), strips, persistent, remap, bool(remap and not persistent),
                  "none", p.ni, ids, p)


def tag7(r):
    """the tag of a 7x7 case: kernel, strip mode, launch ('plain', 'plain+remap': the XCD-aware block order, 'persistent')"""
    return "%s %s %s" % (r.kernel, r.strips, "persistent" if r.persistent else "plain+remap" if r.remap_used else "plain")


def edges7(N, H, W, cin, cout, groups, pad_in, fm):
    """the edges a 7x7 geometry has, as a set of words.  ('H<strip rows' - make_plan's min(strip_rows, H + 6) - needs 256 positions
    in fewer than 3 rows: no such map fits the LDS, the word is here for the day the limits move.)"""
    p = plan7(N, H, W, H + pad_in, fm)
    e = {"W%%%d=%d" % (fm, W % fm), "one chunk" if cin == CK else "chunks"}
    if p.tpi and H + 6 < strip_rows(p.gx):
        e.add("H<strip rows")
    if p.crossing:
        e.add("strip crosses images")
    if p.tpi and (H * p.gx) % 32:
        e.add("ragged last strip")
    if pad_in > 3:
        e.add("gap>padding")
    if cout % 128:
        e.add("ragged cout")
    if groups > 1:
        e.add("two branches")
    return e


# ---- csrc/conv_wino4.hip -----------------------------------------------------------------------------------------------------
NT4, NC4, NTS4 = 32, 64, 16   # wtiles and output columns of a block of wino4_f32<2>; wtiles of a block of wino4s_f32

SHAPES4 = ("small", "plain<=CUs", "plain>CUs", "persistent", "persistent+small", "persistent+half")


def fits4(cin, cout):
    """conv2d_wino4_ok"""
    return int(cout > 0 and cin % 16 == 0 and cin >= 32)


# shape: one of SHAPES4; second: 'none' | 'small' (wino4s_f32) | 'half' (wino4_f32<1>); rest: m tiles of the second launch;
# whole: the persistent launch's m tiles are whole rounds of its blocks
Reach4 = namedtuple("Reach4", "shape kernel persistent xcd_remap second rest whole mtiles ncombo blocks")


def reach4(N, H, W, cin, cout, groups, cus=CUS, prelu=0):
    """conv2d_wino4_launch + wino4_run<PR>"""
    assert fits4(cin, cout)
    pr = "true" if prelu else "false"
    T = N * ceil_div(H, 4) * ceil_div(W, 4)
    mtiles = ceil_div(T, NT4)
    ncombo = cout_pad(cout) // NC4 * groups
    remap, ids = grid_ids(mtiles, ncombo)
    if mtiles * ncombo * 2 <= cus:
        nb = ceil_div(T, NTS4) * (cout_pad(cout) // 16 * groups)
        return Reach4("small", "wino4s_f32<%s>" % pr, False, remap, "none", 0, False, mtiles, ncombo, nb)
    rest, half, persistent, whole = 0, False, False, False
    if mtiles * ncombo > cus and cus % (8 * ncombo) == 0:
        pc = cus // ncombo
        r = mtiles % pc
        if r and r * ncombo * 4 <= cus:
            rest = r
        elif r and 2 * r * ncombo <= cus:
            rest, half = r, True
        persistent, ids = True, cus
        whole = r == 0 or rest > 0
    shape = ("persistent" + ("+half" if half else "+small" if rest else "")) if persistent else \
        ("plain>CUs" if mtiles * ncombo > cus else "plain<=CUs")
    return Reach4(shape, "wino4_f32<2,%s>" % pr, persistent, remap, "half" if half else "small" if rest else "none", rest,
                  whole, mtiles - rest, ncombo, ids)


def tag4(r, prelu=0, pool=0, planes=0):
    """the tag of an F(4x4,3x3) case: launch shape + what the epilogue / the addressing adds"""
    return r.shape + (" prelu" if prelu else "") + (" pool" if pool else "") + (" planes" if planes else "")


def edges4(N, H, W, cin, cout, groups, pad_in):
    e = {"H%%4=%d" % (H % 4), "W%%4=%d" % (W % 4)}
    per = ceil_div(H, 4) * ceil_div(W, 4)
    if N > 1 and per % NT4:
        e.add("tile crosses images")
    if pad_in > 1:
        e.add("gap>padding")
    if cout % NC4:
        e.add("ragged cout")
    if groups > 1:
        e.add("two branches")
    return e


# ---- csrc/conv_wino.hip: rtpose_conv2d_winograd_fits for the two forms of this file -------------------------------------------
def fits(k, wino_m, cin, cout, N, H, W, hs, pool=0, relu=0, prelu=0, default_fm=6):
    """rtpose_conv2d_winograd_fits of a descriptor without residual / pre-activation, for k = 7 and for k = 3 with wino_m = 4.
    default_fm: what wino_m = 0 resolves to (6 unless RTPOSE_WINOGRAD7_M=4 is in the environment)."""
    if k == 7:
        if wino_m not in (0, 4, 6, 8) or prelu:
            return 0
        return int(not pool and fits7(cin, cout, N, H, W, hs, wino_m or default_fm))
    assert k == 3 and wino_m == 4
    if prelu and (pool or relu):
        return 0
    return fits4(cin, cout)
