"""The exact cases of the forward conv launchers (include/rtpose_mi355x.h section 2 and its bf16 / bf16x3 / Winograd
siblings): operands that are small integers, the float64 reference compared with ==, and the conditions under which == is
legitimate.  torch CPU + numpy only: no GPU, no library call.  tests/test_conv_forward_exact_cpu.py asserts the conditions
of every case, tests/test_conv_forward_exact_gpu.py runs the cases.

Why == holds.  Every launcher multiplies exactly (fp32 x fp32 of small integers; bf16 x bf16 is exact in fp32 anyway) and
accumulates in fp32.  While S = sum |x| |w| + |bias| (+ |residual|) of an output stays below 2^24, every product and every
partial sum - in any order, split over any fragments, chunks, slabs or fma chains - is an integer fp32 holds exactly, so
the sum is THE integer and the float64 reference gives the same bits.  PReLU slopes are powers of two (the product is
exact), the pre-activation relu(scale * x + shift) has integer scale / shift (exact whether or not it is contracted into an
fma), a bf16 output is the exact sum rounded ONCE (round to nearest even, lr.bf16_rne), a max-pool rounds nothing.

What a differing bit then means: a term missing, doubled or taken from a neighbouring pixel / channel / tap, an operand
rounded on its way (`discriminates` shows on the CPU that such a change of the sampled terms moves at least one output), a
stale tile, or a store at the wrong place.

bf16x3 (header section "bf16x3 variant"): v travels as hi = bf16(v), lo = bf16(v - hi); the kernel adds
hi*hi + hi*lo + lo*hi and drops lo*lo.  Small integers have lo = 0 and test nothing of the split, so there are two more
operand families: 'xwide' - x an odd integer of 9 significant bits (lo != 0 everywhere), w of at most 2 bits
(lo = 0) - and 'wwide', the other way round.  Then hi + lo is the operand exactly, the dropped product lo*lo is identically
zero and the three kept products are exact integers: the launch must give the exact conv of the fp32 operands.  A split
output is the exact sum v as (hi, lo) = lr.split(v): 16 of its bits.
The fp32 launchers run the same two families beside the small integers: every value of {-2 .. 2} is a bf16 value, so an
fp32 operand that is rounded to bf16 on its way would pass the small cases; an odd integer above 256 does not survive it.

Winograd (oracle/winograd_tables.py, exact rationals): see wino_proof.  F(2x2,3x3) is admitted; F(4x4,3x3) and F(4,7) are
not (the least multiplier c that makes G g G^T dyadic is 3^10 resp. 315 and the channel sums then pass 2^24 quanta at the
smallest cin the forms take); F(6,7) and F(8,7) store B^T entries that are no dyadic rationals."""
from collections import namedtuple
from fractions import Fraction as Fr
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import layout_restate as lr
from oracle import winograd_tables as wt_oracle

LIMIT = 2 ** 24
CUS = 256                   # the CU count the walk cases are sized for on the CPU (the GPU file takes the device's)

# ---- tile constants, with the place they are stated at ----------------------------------------------------------------------
BM = 128                    # csrc/conv_mfma.hip, conv_mfma_bf16.hip: kBM, pixels of a strip tile (its tail runs as 64-pixel halves)
STRIP_MAXW = 128            # plan_conv, fp32 (strip_maxw) and bf16x3: the widest map that runs as strips; wider maps and fused
STRIP_MAXW_BF16 = 64        # pools: 2-D tiles.  conv_mfma_bf16.hip, plan_conv: 64 for unsplit bf16 operands
LDS_LIMIT = 80 * 1024       # plan_conv: the LDS budget of a strip's halo buffers (see `strips`)
BN = 64                     # csrc/common.h: kConvBN, the column tile (cout_pad = multiples of it)
# (chunk widths: `conv_ck`; the bf16 / bf16x3 launchers take cin in multiples of 16, the fp32 ones of 8)
PAIR_BM = 64                # csrc/conv_tail.hip, conv_tail_bf16.hip: BM, pixels of a block of the pointwise pair
FIRST_TILE = (8, 32)        # csrc/conv_first.hip: TH, TW; fp32: 3 persistent blocks per CU once tiles >= 3 CUs
STEM_TILE = (32, 16)        # csrc/hourglass_ops.hip: TH, TW of OUTPUT pixels; 2 persistent blocks per CU
C64_TILE = (16, 32)         # csrc/conv_c64_bf16.hip: TH, TW; 2 persistent blocks per CU
# csrc/conv_wino.hip: a block owns 32 (cout_pad % 128 == 0) or 64 2 x 2 output tiles (wino2_form)

Case = namedtuple("Case", "launcher tag n h w cin cout k groups relu pool prelu cmap pad_in pad_out kind m out_f32 entry "
                          "family x edges walk seed")


def _c(launcher, tag, n, h, w, cin, cout, k=1, groups=1, relu=0, pool=0, prelu=0, cmap=0, pad_in=None, pad_out=1, kind="f32",
       m=None, out_f32=False, entry=None, family="int", x=None, edges=(), walk=None, seed=0):
    return Case(launcher, tag, n, h, w, cin, cout, k, groups, relu, pool, prelu, cmap, k // 2 if pad_in is None else pad_in,
                pad_out, kind, m, out_f32, entry, family, x or {}, tuple(edges), walk, seed)


def cin_packed(c):
    unit = 8 if c.kind == "f32" else 16
    return (c.cin + unit - 1) // unit * unit


# ---- host restatement of the launch geometry (only what the edge tags need) ------------------------------------------------
def conv_ck(c):
    """channels of an LDS chunk.  fp32 (conv_mfma.hip, conv_ck): 16 when cin % 16 == 0, else 8.  bf16 (conv_mfma_bf16.hip,
    conv_ck): 16 for split operands and cin % 32 != 0; 64 for 3x3 with cin % 64 == 0 and cin >= 256 and for 1x1 with
    cin % 64 == 0; else 32."""
    cin = cin_packed(c)
    if c.kind == "f32":
        return 16 if cin % 16 == 0 else 8
    if c.kind == "x3" or cin % 32:
        return 16
    if c.k == 3 and cin % 64 == 0 and cin >= 256:
        return 64
    return 64 if (c.k == 1 and cin % 64 == 0) else 32


def strip_maxw(c):
    """plan_conv of the launcher: the widest map that runs as strips"""
    return STRIP_MAXW_BF16 if c.kind == "bf16" else STRIP_MAXW


def strips(c):
    """plan_conv restated (conv_mfma.hip and conv_mfma_bf16.hip; the input layout is lr.padded(., h, w, pad_in), as
    conv_driver.to_layout makes it): a map no wider than strip_maxw without fused pool runs as 128-pixel strips if the
    longest run of buffer pixels a strip's halo spans (lb, rounded up to qs = 2 mod 4) fits the staging schedule of a
    double-buffered k x k kernel (pieces of 256 threads: k^2 - 1 sets, bf16 k^2) and both buffers fit 80 KiB of LDS."""
    if c.w > strip_maxw(c) or c.pool:
        return False
    p, ws, hs = c.k // 2, c.w + c.pad_in, c.h + c.pad_in
    lb = (BM - 1) + ((BM - 1) // c.w + 1) * (ws - c.w) + ((BM - 1) // (c.h * c.w) + 1) * (hs - c.h) * ws + 2 * p * ws + 2 * p + 1
    qs = lb
    while qs & 3 != 2:
        qs += 1
    nbuf = 1 if c.k == 1 else 2
    if c.kind == "f32":
        cg, sets, tail = conv_ck(c) // 4, c.k * c.k - 1, 256 * 16
    else:
        cg, sets, tail = conv_ck(c) // 8 * (2 if c.kind == "x3" else 1), c.k * c.k, 256 * 16 if nbuf == 2 else 0
    if nbuf == 2 and -(-qs * cg // 256) > sets:
        return False
    return nbuf * cg * qs * 16 + tail <= LDS_LIMIT


def geometry(c, cus=CUS):
    """What the launcher of `c` makes of the shape: pixel count, tile mode, tile counts, the half-tile tail."""
    M = c.n * c.h * c.w
    g = SimpleNamespace(M=M, cin_p=cin_packed(c), ntiles=(c.cout + BN - 1) // BN)
    g.ck = conv_ck(c)
    g.chunks = g.cin_p // g.ck
    g.strip = strips(c)
    g.mtiles = (M + BM - 1) // BM if g.strip else None
    if c.launcher in ("conv2d", "conv2d_x") and g.strip:
        total = g.mtiles * g.ntiles * c.groups
        slots = cus * (4 if c.k == 1 else 2)
        rem = total % slots
        g.total, g.nbig = total, total
        if total > slots and rem > 0 and 2 * rem <= cus:
            g.nbig = total - rem
        if total <= cus:
            g.nbig = 0
    return g


EDGES = {
    # tag -> predicate(case, geometry): the shape reaches the edge its tag claims
    "one pixel": lambda c, g: g.M == 1,
    "H=1": lambda c, g: c.h == 1 and c.w > 1,
    "W=1": lambda c, g: c.w == 1 and c.h > 1,
    "BM-1": lambda c, g: g.M == BM - 1,
    "BM": lambda c, g: g.M == BM,
    "BM+1": lambda c, g: g.M == BM + 1,
    "BM+BM/2-1": lambda c, g: g.M == BM + BM // 2 - 1,
    "BM+BM/2": lambda c, g: g.M == BM + BM // 2,
    "BM+BM/2+1": lambda c, g: g.M == BM + BM // 2 + 1,
    "strip": lambda c, g: g.strip,
    "2-D tiles": lambda c, g: not g.strip,
    "W=STRIP_MAXW+1": lambda c, g: c.w == strip_maxw(c) + 1,          # the launcher's own strip width
    # (every launcher refuses a fused pool of an odd map - tests/test_conv_forward_exact_gpu.py asserts the refusal -, so the
    # pool cases are even maps that are no multiple of any 2-D tile: 128 pixels as 4 x 32 ... 64 x 2)
    "pool": lambda c, g: c.pool and c.h % 2 == 0 and c.w % 2 == 0 and c.h % 4 != 0 and c.w % 4 != 0,
    "ck8": lambda c, g: g.ck == 8,
    "ck16": lambda c, g: g.ck == 16,
    "ck64": lambda c, g: g.ck == 64,
    # conv2d_bf16_launch: `tr`, the transposed epilogue of the k x k kernels - vector stores (bf16 output, cout % 64 == 0,
    # an aligned layout: the second output policy of the GPU file), no pool
    "transposed epilogue": lambda c, g: c.kind == "bf16" and c.k != 1 and c.cout % BN == 0 and not c.pool and not c.out_f32,
    "one chunk": lambda c, g: g.chunks == 1,
    "odd chunks": lambda c, g: g.chunks % 2 == 1 and g.chunks > 1,
    "cin>=128": lambda c, g: g.cin_p >= 128,
    "cin padded": lambda c, g: g.cin_p > c.cin,
    "BN-1": lambda c, g: c.cout == BN - 1,
    "BN": lambda c, g: c.cout == BN,
    "BN+1": lambda c, g: c.cout == BN + 1,
    "128-column tile": lambda c, g: c.k != 1 and c.cout % 128 == 0,      # conv2d_bf16_launch: `wide`
    "head 38": lambda c, g: c.cout == 38,
    "head 19": lambda c, g: c.cout == 19,
    "two groups": lambda c, g: c.groups == 2,
    "images": lambda c, g: c.n > 1,
    "halves only": lambda c, g: g.nbig == 0,
    "full tiles + halves": lambda c, g: 0 < g.nbig < g.total,
    "PAIR_BM-1": lambda c, g: g.M == PAIR_BM - 1,
    "PAIR_BM": lambda c, g: g.M == PAIR_BM,
    "PAIR_BM+1": lambda c, g: g.M == PAIR_BM + 1,
    "mid 128": lambda c, g: c.x["mid"] == 128,
    "mid 512": lambda c, g: c.x["mid"] == 512,
    "tile ragged": lambda c, g: out_hw(c)[0] % c.x["tile"][0] != 0 and out_hw(c)[1] % c.x["tile"][1] != 0,
    "tiles>1": lambda c, g: out_hw(c)[0] > c.x["tile"][0] or out_hw(c)[1] > c.x["tile"][1],
    "row tiles>1": lambda c, g: out_hw(c)[0] > c.x["tile"][0],
    "walk": lambda c, g: (walk_items(c) >= 2.5 * walk_blocks(c) and walk_items(c) % walk_blocks(c) != 0
                          and (g.strip or c.launcher not in ("conv2d_bf16", "conv2d_bf16x3"))),
    "wo 31": lambda c, g: (c.w + 1) // 2 == 31, "wo 32": lambda c, g: (c.w + 1) // 2 == 32, "wo 33": lambda c, g: (c.w + 1) // 2 == 33,
    "ho 31": lambda c, g: (c.h + 1) // 2 == 31, "ho 32": lambda c, g: (c.h + 1) // 2 == 32, "ho 33": lambda c, g: (c.h + 1) // 2 == 33,
    "ho 15": lambda c, g: (c.h + 1) // 2 == 15, "ho 16": lambda c, g: (c.h + 1) // 2 == 16, "ho 17": lambda c, g: (c.h + 1) // 2 == 17,
    "odd H": lambda c, g: c.h % 2 == 1, "even H": lambda c, g: c.h % 2 == 0,
    "odd W": lambda c, g: c.w % 2 == 1, "even W": lambda c, g: c.w % 2 == 0,
    "m": lambda c, g: c.h == 2 and c.w == 2, "m-1": lambda c, g: c.h == 1 and c.w == 1,
    "m+1": lambda c, g: c.h == 3 and c.w == 3, "2m+1": lambda c, g: c.h == 5 and c.w == 5,
    "small grid": lambda c, g: wino2_form(c) == "small",
    "plain grid": lambda c, g: wino2_form(c) == "plain",
    "persistent": lambda c, g: wino2_form(c) == "persistent",
    "res own": lambda c, g: c.x.get("res") == "own", "res in place": lambda c, g: c.x.get("res") == "inplace",
    "preact": lambda c, g: bool(c.x.get("preact")),
    "wino ck16 64 columns": lambda c, g: (c.cout + BN - 1) // BN * BN % 128 == 64 and cin_packed(c) % 16 == 0,   # wino_f32<2, 2, 16>
    "gap pixels": lambda c, g: c.pad_in > 0,
}


def out_hw(c):
    """the map the tiles of a launcher cover: its output before any fused pool (the stem: stride 2)"""
    return ((c.h + 1) // 2, (c.w + 1) // 2) if c.launcher == "conv7x7_s2" else (c.h, c.w)


def wino2_form(c, cus=CUS):
    """conv2d_wino_launch / wino_run restated: which of the three F(2x2,3x3) kernels a shape reaches."""
    coutp = (c.cout + BN - 1) // BN * BN
    wm = 1 if coutp % 128 == 0 else 2
    ck = 8 if (coutp % 128 == 64 and cin_packed(c) % 16 != 0) else 16
    T = c.n * ((c.h + 1) // 2) * ((c.w + 1) // 2)
    mtiles = (T + 32 * wm - 1) // (32 * wm)
    ncombo = coutp // (32 * (4 // wm)) * c.groups
    if mtiles * ncombo > cus and cus % ncombo == 0:
        return "persistent"
    return "small" if ck == 16 and mtiles * ncombo * 2 <= cus else "plain"


def walk_blocks(c, cus=CUS):
    """blocks of the persistent grid of a walk case"""
    return {"conv_first": 3 * cus, "conv_first_planes": 3 * cus, "conv7x7_s2": 2 * cus, "c64": 2 * cus, "conv2d_bf16": 2 * cus // 8 * 8,
            "conv2d_bf16x3": 2 * cus // 8 * 8, "wino2": cus}[c.launcher]


def walk_items(c):
    if c.launcher in ("conv_first", "conv_first_planes", "conv7x7_s2", "c64"):
        th, tw = c.x["tile"]
        ho, wo = ((c.h + 1) // 2, (c.w + 1) // 2) if c.launcher == "conv7x7_s2" else (c.h, c.w)
        return c.n * ((ho + th - 1) // th) * ((wo + tw - 1) // tw) * (c.cout // 64)
    if c.launcher == "wino2":
        coutp = (c.cout + BN - 1) // BN * BN
        wm = 1 if coutp % 128 == 0 else 2
        T = c.n * ((c.h + 1) // 2) * ((c.w + 1) // 2)
        return (T + 32 * wm - 1) // (32 * wm) * (coutp // (32 * (4 // wm))) * c.groups
    return (c.n * c.h * c.w + BM - 1) // BM * ((c.cout + BN - 1) // BN) * c.groups     # full strip tiles (the tail aside)


def sized(c, cus):
    """A walk case with its batch taken from the CU count: c.walk = (items per CU-block wanted, items per image)."""
    if c.walk is None:
        return c
    if c.launcher == "conv2d":          # 4 x CUs + 4 tiles of a 1x1 conv: two column tiles x two branches per 128-pixel image
        return c._replace(n=cus + 1)
    per_block, per_image = c.walk
    blocks = walk_blocks(c, cus)
    n = int(-(-(per_block * blocks) // per_image)) + 1
    c = c._replace(n=n)
    while walk_items(c) % blocks == 0:
        c = c._replace(n=c.n + 1)
    return c


# ---- operands -----------------------------------------------------------------------------------------------------------------
X_MAX, W_MAX, B_MAX, R_MAX = 2, 2, 3, 4
BF16_MAX = 8                                    # |x|, |w| of the bf16 launchers but the pointwise pair
SLOPES = (0.5, 0.25, 2.0, -0.5, 0.125)          # powers of two, one of them negative
WIDE_LO, WIDE_HI = 257, 511                     # 'xwide' / 'wwide': odd integers of 9 significant bits


def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _wide(g, *shape):
    """odd integers in +-[WIDE_LO, WIDE_HI]: never representable in bf16 (an odd integer above 256 needs 9 bits)"""
    v = torch.randint((WIDE_LO - 1) // 2, (WIDE_HI - 1) // 2 + 1, shape, generator=g) * 2 + 1
    return (v * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def operands(c):
    """The operands of a case, float32 holding integers.
    x  [n, cin, h, w] in {-2 .. 2} (a fifth of them zero, both signs; the border ring of every channel never zero; the
       bf16 launchers draw x and w from {-8 .. 8}: sums of the small range rarely pass 256, where a bf16 store rounds);
    w  [cout, cin, k, k] in {-2 .. 2} per branch, output channel 0 never zero; bias in {-3 .. 3};
    PReLU slopes from SLOPES; residual in {-4 .. 4}; in_scale in {-2, -1, 1, 2} (both signs), in_shift in {-2 .. 2};
    the pointwise pairs: a second filter bank w2 in {-1, 0, 1}, bias b2.
    Families 'xwide' / 'wwide' (the fp32 launchers and bf16x3): x resp. w odd integers in +-[257, 511] - no bf16 value, so
    an operand that passes through bf16 anywhere changes."""
    g = torch.Generator().manual_seed(4000 + c.seed)
    o = SimpleNamespace()
    wide = c.kind == "bf16" and "mid" not in c.x        # bf16 stores: a range whose sums pass 256 and need the rounding
    xm, wm = (BF16_MAX, BF16_MAX) if wide else (X_MAX, W_MAX)
    x = _wide(g, c.n, c.cin, c.h, c.w) if c.family == "xwide" else _ri(g, -xm, xm, c.n, c.cin, c.h, c.w)
    ring = torch.zeros(c.h, c.w, dtype=torch.bool)
    ring[0, :] = ring[-1, :] = True
    ring[:, 0] = ring[:, -1] = True
    x = torch.where(ring & (x == 0), torch.ones(()), x)
    if c.cin >= 3 and c.family != "xwide":       # the first and last two channels differ at the corners of the first and last
        for img in {0, c.n - 1}:                 # image: a term moved to the neighbouring channel shows even on one pixel
            for yy in {0, c.h - 1}:
                for xx in {0, c.w - 1}:
                    if c.cin == 3:
                        x[img, :, yy, xx] = torch.tensor([1.0, -2.0, 2.0])
                    else:
                        x[img, [0, 1, -2, -1], yy, xx] = torch.tensor([1.0, -2.0, -1.0, 2.0])
    o.x = x
    o.wts, o.biases, o.slopes = [], [], []
    for _ in range(c.groups):
        wt = _wide(g, c.cout, c.cin, c.k, c.k) if c.family == "wwide" else _ri(g, -wm, wm, c.cout, c.cin, c.k, c.k)
        wt[0] = torch.where(wt[0] == 0, torch.ones(()), wt[0])
        o.wts.append(wt)
        o.biases.append(_ri(g, -B_MAX, B_MAX, c.cout))
        o.slopes.append(torch.tensor(SLOPES)[torch.randint(0, len(SLOPES), (c.cout,), generator=g)] if c.prelu else None)
    if c.cmap:
        o.cmap = torch.randperm(c.cout, generator=g).to(torch.int32)       # a permutation of the slice's channels
    if c.x.get("res"):
        o.res = _ri(g, -R_MAX, R_MAX, c.n, c.cout, c.h, c.w)
    if c.x.get("preact"):
        sign = {"neg": -1.0, "pos": 1.0}.get(c.x["preact"])
        mag = _ri(g, 1, 2, c.cin)
        o.in_scale = mag * sign if sign else mag * (2 * _ri(g, 0, 1, c.cin) - 1)
        if not sign:
            o.in_scale[0], o.in_scale[-1] = -1.0, 2.0
        o.in_shift = _ri(g, -2, 2, c.cin)
        o.in_shift[0], o.in_shift[-1] = 1.0, -1.0
        for ch in (0, c.cin - 1):                # the staged corner values of these channels are positive: |scale| * 2 + shift
            for yy in {0, c.h - 1}:
                for xx in {0, c.w - 1}:
                    o.x[:, ch, yy, xx] = 2.0 * torch.sign(o.in_scale[ch])
    if "mid" in c.x:
        o.w2, o.b2 = [], []
        for _ in range(c.groups):
            w2 = _ri(g, -1, 1, c.cout, c.x["mid"], 1, 1)
            w2[0] = torch.where(w2[0] == 0, torch.ones(()), w2[0])
            o.w2.append(w2)
            o.b2.append(_ri(g, -B_MAX, B_MAX, c.cout))
        for gi in range(c.groups):                   # the first conv of a pair: 128 -> mid
            o.wts[gi] = _wide(g, c.x["mid"], c.cin, 1, 1) if c.family == "wwide" else _ri(g, -W_MAX, W_MAX, c.x["mid"], c.cin, 1, 1)
            o.wts[gi][0] = torch.where(o.wts[gi][0] == 0, torch.ones(()), o.wts[gi][0])
            o.biases[gi] = _ri(g, -B_MAX, B_MAX, c.x["mid"])
            for ch in (0, c.x["mid"] - 1):       # the first and last intermediate channel are positive at the first pixel, so
                sg = torch.sign(o.x[0, :, 0, 0]).view(-1, 1, 1)      # that the second conv's terms there show on one pixel too
                o.wts[gi][ch] = torch.where(sg != 0, o.wts[gi][ch].abs() * sg, o.wts[gi][ch])
    return o


# ---- the float64 reference ------------------------------------------------------------------------------------------------------
def _stride(c):
    return 2 if c.launcher == "conv7x7_s2" else 1


def staged_input(c, o, x):
    """what the conv sums over: x, or relu(in_scale * x + in_shift) (header: rtpose_conv_desc.in_scale / in_shift)"""
    x = x.double()
    if c.x.get("preact"):
        x = F.relu(x * o.in_scale.double().view(1, -1, 1, 1) + o.in_shift.double().view(1, -1, 1, 1))
    return x


def pre_activation(c, o, gi, x=None, wt=None, w2=None):
    """(conv + bias (+ residual) in float64 BEFORE ReLU / PReLU / pool / rounding, S of the same terms)"""
    x = staged_input(c, o, o.x if x is None else x)
    wt = (o.wts[gi] if wt is None else wt).double()
    b = o.biases[gi].double()
    y = F.conv2d(x, wt, b, stride=_stride(c), padding=c.k // 2)
    s = F.conv2d(x.abs(), wt.abs(), b.abs(), stride=_stride(c), padding=c.k // 2)
    if "mid" in c.x:                                 # conv -> ReLU (-> bf16) -> conv
        t = F.relu(y)
        if c.kind == "bf16":
            t = round_bf16(t)
        w2, b2 = (o.w2[gi] if w2 is None else w2).double(), o.b2[gi].double()
        y = F.conv2d(t, w2, b2)
        s = torch.maximum(s.max(), F.conv2d(t.abs(), w2.abs(), b2.abs()).max()).expand(1)
    if c.x.get("res"):
        r = o.res[:x.shape[0]].double()
        y, s = y + r, s + r.abs()
    return y, s


def round_bf16(t):
    """float64 tensor of values fp32 holds exactly -> the same rounded once to bf16 (RNE), as float64"""
    f = t.to(torch.float32)
    assert torch.equal(f.double(), t), "not an fp32 value"
    return torch.from_numpy(lr.bf16_to_f32(lr.bf16_rne(f.numpy())).reshape(f.shape)).double()


def finish(c, o, gi, y):
    """ReLU / PReLU / 2x2 max-pool and the rounding of the output element type, on a float64 pre-activation"""
    if c.relu:
        y = F.relu(y)
    if o.slopes[gi] is not None:
        y = torch.where(y >= 0, y, o.slopes[gi].double().view(1, -1, 1, 1) * y)
    if c.pool:
        y = F.max_pool2d(y, 2, 2, 0)
    if c.kind == "bf16" and not c.out_f32:
        y = round_bf16(y)
    elif c.kind == "x3" and not c.out_f32:
        f = y.to(torch.float32)
        hi, lo = lr.split(f.numpy())
        y = torch.from_numpy((lr.bf16_to_f32(hi) + lr.bf16_to_f32(lo)).reshape(f.shape)).double()
    return y


def expected_pieces(c, o):
    """A split bf16x3 output, piece by piece: per branch (hi, lo) as float32 [n, cout, ho, wo], lr.split of the exact sum -
    the split the header defines.  hi + lo alone would also pass a truncated hi with a compensating lo."""
    out = []
    for gi in range(c.groups):
        y = finish(c._replace(out_f32=True), o, gi, pre_activation(c, o, gi)[0]).to(torch.float32)
        hi, lo = lr.split(y.numpy())
        out.append((lr.bf16_to_f32(hi).reshape(y.shape), lr.bf16_to_f32(lo).reshape(y.shape)))
    return out


def expected(c, o, images=None):
    """The outputs the launch must give, bit for bit: [n, cout, ho, wo] float32 per branch (images: only the first few)."""
    x = o.x if images is None else o.x[:images]
    outs = []
    for gi in range(c.groups):
        y = finish(c, o, gi, pre_activation(c, o, gi, x)[0])
        f = y.to(torch.float32)
        assert torch.equal(f.double(), y)
        outs.append(f)
    return outs


# ---- the conditions that make == legitimate ---------------------------------------------------------------------------------------
MIN_SHARE = 0.25            # of the final outputs of a case with >= 64 of them are nonzero (after ReLU: positive)


def conditions(c, o):
    """S, the shares and the counts tests/test_conv_forward_exact_cpu.py asserts, from the reference side only."""
    r = SimpleNamespace(S=0.0, share=1.0, clipped=0, negative=0, pool_off_corner=0, outputs=0, rounded=0)
    shares = []
    for gi in range(c.groups):
        y, s = pre_activation(c, o, gi)
        r.S = max(r.S, s.max().item())
        out = finish(c, o, gi, y)
        shares.append((out != 0).double().mean().item())
        r.outputs += out.numel()
        r.clipped += int((y < 0).sum()) if c.relu else 0
        r.negative += int((y < 0).sum())
        if c.pool:
            a = F.relu(y) if c.relu else y
            ho, wo = a.shape[2] // 2, a.shape[3] // 2
            corner = a[:, :, 0:2 * ho:2, 0:2 * wo:2]
            r.pool_off_corner += int((F.max_pool2d(a, 2, 2, 0) > corner).sum())
        if c.kind == "bf16" and not c.out_f32:
            z = F.relu(y) if c.relu else y
            r.rounded += int((round_bf16(z) != z).sum())
    r.share = min(shares)
    return r


def split_properties(c, o):
    """bf16x3: (hi + lo == operand for x and w, share of x with lo != 0, share of w with lo != 0, max |lo_x * lo_w|)"""
    xs = lr.split(o.x.numpy())
    xh, xl = lr.bf16_to_f32(xs[0]).astype(np.float64), lr.bf16_to_f32(xs[1]).astype(np.float64)
    exact = bool(np.all(xh + xl == o.x.numpy().astype(np.float64)))
    wl_share, dropped = 0.0, 0.0
    for wt in o.wts:
        ws = lr.split(wt.numpy())
        wh, wl = lr.bf16_to_f32(ws[0]).astype(np.float64), lr.bf16_to_f32(ws[1]).astype(np.float64)
        exact = exact and bool(np.all(wh + wl == wt.numpy().astype(np.float64)))
        wl_share = max(wl_share, float(np.mean(wl != 0)))
        dropped = max(dropped, float(np.abs(xl).max() * np.abs(wl).max()))
    return exact, float(np.mean(xl != 0)), wl_share, dropped


# ---- discrimination ----------------------------------------------------------------------------------------------------------------
def live_taps(c):
    """taps (ky, kx) that meet a pixel of the map for some output (a 1 x 1 map under a 3x3 filter: the centre only)"""
    p = c.k // 2
    return [(ky, kx) for ky in range(c.k) for kx in range(c.k) if abs(ky - p) < c.h and abs(kx - p) < c.w]


def sampled_terms(c):
    """The sample of terms `discriminates` changes: filter entries (all output channels) at the first and last live tap of
    the first and last input channel - these lie in the first and last channel chunk - and the input at the four corner
    pixels of the first and the last image, first and last channel."""
    taps = live_taps(c)
    chans = sorted({0, c.cin - 1})
    wterms = [("w", ch, t) for ch in chans for t in sorted({taps[0], taps[-1]})]
    # (a fused pool drops the odd last row / column: under a 1x1 filter the last pixel that reaches an output is one further in)
    hl, wl = (c.h - 1, c.w - 1) if not (c.pool and c.k == 1) else (c.h // 2 * 2 - 1, c.w // 2 * 2 - 1)
    corners = sorted({(0, 0), (0, wl), (hl, 0), (hl, wl)})
    xterms = [("x", img, ch, yx) for img in sorted({0, c.n - 1}) for ch in chans for yx in corners]
    # the second conv of a pointwise pair: its filter column at the first and last intermediate channel (first and last chunk)
    w2terms = [("w2", ch) for ch in sorted({0, c.x["mid"] - 1})] if "mid" in c.x else []
    return wterms + w2terms + xterms


def _changed(c, o, base, x=None, wts=None, w2s=None):
    for gi in range(c.groups):
        y = finish(c, o, gi, pre_activation(c, o, gi, x, None if wts is None else wts[gi], None if w2s is None else w2s[gi])[0])
        if not torch.equal(y, base[gi]):
            return True
    return False


def discriminates(c, o):
    """For every sampled term: removing it, doubling it, and moving it by one channel / one tap / one pixel each change at
    least one final output of the case (after ReLU, pool and output rounding).  Returns the list of (term, change) that
    did NOT - empty for a case that discriminates.  A move is tried only where a neighbour exists (cin > 1, two live taps,
    a map wider or higher than one pixel)."""
    base = [finish(c, o, gi, pre_activation(c, o, gi)[0]) for gi in range(c.groups)]
    failed = []
    taps = live_taps(c)
    for term in sampled_terms(c):
        if term[0] == "w":
            _, ch, (ky, kx) = term
            changes = [("removed", lambda w: w[:, ch, ky, kx].zero_()), ("doubled", lambda w: w[:, ch, ky, kx].mul_(2))]
            if c.cin > 1:
                other = ch + 1 if ch + 1 < c.cin else ch - 1

                def move_c(w):
                    w[:, [ch, other], ky, kx] = w[:, [other, ch], ky, kx]
                changes.append(("moved a channel", move_c))
            if len(taps) > 1:
                i = taps.index((ky, kx))
                ty, tx = taps[i + 1] if i + 1 < len(taps) else taps[i - 1]

                def move_t(w):
                    a, b = w[:, ch, ky, kx].clone(), w[:, ch, ty, tx].clone()
                    w[:, ch, ky, kx], w[:, ch, ty, tx] = b, a
                changes.append(("moved a tap", move_t))
            for name, fn in changes:
                wts = [w.clone() for w in o.wts]
                for w in wts:
                    fn(w)
                if all(torch.equal(a, b) for a, b in zip(wts, o.wts)):
                    continue                         # (the swap met two equal columns: nothing was changed)
                if not _changed(c, o, base, wts=wts):
                    failed.append((term, name))
        elif term[0] == "w2":
            ch = term[1]
            other = ch + 1 if ch + 1 < c.x["mid"] else ch - 1

            def move_m(w):
                w[:, [ch, other]] = w[:, [other, ch]]
            for name, fn in (("removed", lambda w: w[:, ch].zero_()), ("doubled", lambda w: w[:, ch].mul_(2)),
                             ("moved a channel", move_m)):
                w2s = [w.clone() for w in o.w2]
                for w in w2s:
                    fn(w)
                if all(torch.equal(a, b) for a, b in zip(w2s, o.w2)):
                    continue
                if not _changed(c, o, base, w2s=w2s):
                    failed.append((term, name))
        else:
            _, img, ch, (yy, xx) = term
            changes = [("removed", lambda x: x[img, ch, yy, xx].zero_()), ("doubled", lambda x: x[img, ch, yy, xx].mul_(2))]
            if c.w > 1 or c.h > 1:
                y2, x2 = (yy, xx + 1 if xx + 1 < c.w else xx - 1) if c.w > 1 else (yy + 1 if yy + 1 < c.h else yy - 1, xx)

                def move_p(x):
                    a, b = x[img, ch, yy, xx].clone(), x[img, ch, y2, x2].clone()
                    x[img, ch, yy, xx], x[img, ch, y2, x2] = b, a
                changes.append(("moved a pixel", move_p))
            for name, fn in changes:
                x = o.x.clone()
                fn(x)
                if torch.equal(x, o.x):
                    continue
                if not _changed(c, o, base, x=x):
                    failed.append((term, name))
    return failed


# ---- Winograd: which forms integer operands pin ---------------------------------------------------------------------------------
def _odd_part_lcm(fracs):
    c = 1
    for f in fracs:
        d = f.denominator
        while d % 2 == 0:
            d //= 2
        c = c * d // np.gcd(c, d)
    return int(c)


def _quantum(fracs):
    """the largest power of two every entry is a multiple of (entries dyadic), as a Fraction; 1 if all are zero"""
    q = None
    for f in fracs:
        if f == 0:
            continue
        assert f.denominator & (f.denominator - 1) == 0, "not dyadic"
        n, e = abs(f.numerator), Fr(1, f.denominator)
        while n % 2 == 0:
            n //= 2
            e *= 2
        q = e if q is None or e < q else q
    return q or Fr(1)


def wino_proof(m, r, points, two_d, cin, rows=1, x_max=X_MAX, t_max=1, b_max=B_MAX):
    """Exactness of F(m, r) (two_d: F(m x m, r x r); else 1-D along x with `rows` = r direct filter rows summed with the
    channels) on integer inputs |d| <= x_max and weights c * t, |t| <= t_max, from the exact tables of
    oracle/winograd_tables.py - never from the kernel's.  c is the least multiplier that makes every entry of G g (G^T)
    dyadic for every integer t: the odd part of the common denominator of G (squared in 2-D).  Stages, each with the
    worst-case sum of absolute terms and its quantum (the largest power of two all its terms are multiples of):
      1. V = B^T d (B): row abs sums of B^T times x_max;
      2. M = sum over cin (x rows) of V o U, U = G (c t) (G^T) bounded by the row abs sums of G;
      3. y = A^T M (A) + bias.
    A stage is exact in fp32, in any order, while bound < 2^24 * quantum.  Returns (c, [(name, bound, quantum, ok)], True
    iff B^T and A^T are dyadic), with bound / quantum as floats."""
    AT, G, BT = wt_oracle.toom_cook(m, r, points)
    flat = lambda M_: [e for row in M_ for e in row]     # noqa: E731
    dyadic = all(e.denominator & (e.denominator - 1) == 0 for e in flat(BT) + flat(AT))
    c1 = _odd_part_lcm(flat(G))
    c = c1 * c1 if two_d else c1
    if not dyadic:
        return c, [], False
    pw = 2 if two_d else 1
    rs = lambda M_: max(sum(abs(e) for e in row) for row in M_)     # noqa: E731
    qB, qA = _quantum(flat(BT)) ** pw, _quantum(flat(AT)) ** pw
    qU = _quantum([e * c1 for e in flat(G)]) ** pw
    v_bound, u_bound = rs(BT) ** pw * x_max, (rs(G) * c1) ** pw * t_max
    stages = [("input transform", v_bound, qB)]
    m_bound, qM = cin * rows * v_bound * u_bound, qB * qU
    stages.append(("channel sum", m_bound, qM))
    y_bound, qY = rs(AT) ** pw * m_bound + b_max, min(qM * qA, Fr(1))
    stages.append(("output transform", y_bound, qY))
    return c, [(name, float(b), float(q), bool(b < LIMIT * q)) for name, b, q in stages], True


WINO_FORMS = {
    # name: (m, r, points, two_d, smallest cin the form takes, direct rows)
    "F(2x2,3x3)": (2, 3, wt_oracle.POINTS_F2_3, True, 16, 1),
    "F(4x4,3x3)": (4, 3, wt_oracle.POINTS_F4_3, True, 32, 1),
    "F(4,7)": (4, 7, wt_oracle.POINTS_F4_7, False, 8, 7),
    "F(6,7)": (6, 7, wt_oracle.POINTS_F6_7, False, 8, 7),
}
WINO2_C = 1                # F(2x2,3x3): every entry of G is dyadic; the cases use the integer weights as they are


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _pixel_edges(launcher, k):
    """N H W around a strip tile and its half-tile tail, as maps of one column, of several rows and as several images.
    (127, 191 and 193 are primes.  As one row - 1 x 127 - or as one-pixel images a 3x3 or 7x7 strip's halo spans more buffer
    pixels than plan_conv admits, and the launch takes 2-D tiles: `strips`.  A one-column map keeps the halo short.)"""
    shapes = [("BM-1", 1, 127, 1), ("BM", 2, 8, 8), ("BM+1", 1, 3, 43), ("BM+BM/2-1", 1, 191, 1), ("BM+BM/2", 3, 8, 8),
              ("BM+BM/2+1", 1, 193, 1)]
    return [_c(launcher, "k%d-px%d" % (k, n * h * w), n, h, w, 16, 24, k=k, relu=1, edges=(e, "strip"), seed=n * h * w + k)
            for e, n, h, w in shapes]


def _direct_f32():
    L, cs = "conv2d", []
    for k in (1, 3, 7):
        cs.append(_c(L, "k%d-1x1" % k, 1, 1, 1, 8, 8, k=k, edges=("one pixel", "one chunk"), seed=k))
        cs.append(_c(L, "k%d-H1" % k, 2, 1, 9, 8, 24, k=k, relu=1, edges=("H=1", "images"), seed=10 + k))
        cs.append(_c(L, "k%d-W1" % k, 1, 9, 1, 16, 24, k=k, relu=1, edges=("W=1", "ck16"), seed=20 + k))
        cs += _pixel_edges(L, k)
        cs.append(_c(L, "k%d-W129" % k, 1, 3, 129, 8, 24, k=k, relu=1, edges=("W=STRIP_MAXW+1", "2-D tiles"), seed=30 + k))
    for k in (1, 3):
        cs.append(_c(L, "k%d-pool" % k, 2, 6, 10, 16, 24, k=k, relu=1, pool=1, edges=("pool", "2-D tiles", "images"),
                     seed={1: 48, 3: 43}[k]))      # (seeds at which every sampled term shows through the pool in all three families)
        cs.append(_c(L, "k%d-prelu" % k, 2, 5, 7, 24, 38, k=k, prelu=1, edges=("odd chunks", "ck8", "head 38"), seed=50 + k))
        cs.append(_c(L, "k%d-prelu-2d" % k, 1, 2, 130, 16, 19, k=k, prelu=1, groups=2, edges=("2-D tiles", "two groups"),
                     seed=55 + k))
    cs.append(_c(L, "k7-pool", 1, 6, 10, 16, 8, k=7, relu=1, pool=1, edges=("2-D tiles",), seed=47))
    for cin, e in ((8, ("ck8", "one chunk")), (16, ("ck16", "one chunk")), (24, ("ck8", "odd chunks")),
                   (40, ("ck8", "odd chunks")), (37, ("cin padded", "ck8")), (136, ("ck8", "cin>=128", "odd chunks"))):
        for k in (1, 3):
            cs.append(_c(L, "k%d-cin%d" % (k, cin), 1, 5, 6, cin, 24, k=k, relu=1, edges=e + ("strip",), seed=60 + cin + k))
    cs.append(_c(L, "k1-cin512", 1, 5, 6, 512, 19, k=1, edges=("cin>=128", "ck16", "head 19"), seed=70))
    cs.append(_c(L, "k7-cin128", 1, 4, 5, 128, 8, k=7, relu=1, edges=("cin>=128", "ck16"), seed=71))
    cs.append(_c(L, "k7-cin185", 1, 4, 5, 185, 8, k=7, relu=0, edges=("cin>=128", "cin padded"), seed=72))
    for cout, e in ((63, "BN-1"), (64, "BN"), (65, "BN+1"), (38, "head 38"), (19, "head 19")):
        for k in (1, 3):
            cs.append(_c(L, "k%d-cout%d" % (k, cout), 1, 5, 6, 16, cout, k=k, relu=1, edges=(e,), seed=80 + cout + k))
    for k in (1, 3, 7):
        cs.append(_c(L, "k%d-groups2" % k, 2, 6, 7, 16, 38 if k == 1 else 8, k=k, relu=1, groups=2, edges=("two groups", "images"),
                     seed=90 + k))
    for k in (1, 3):
        cs.append(_c(L, "k%d-cmap" % k, 2, 5, 7, 16, 24, k=k, relu=1, cmap=1, edges=("images",), seed=95 + k))
    cs.append(_c(L, "k1-halves-only", 3, 9, 11, 8, 65, k=1, relu=1, edges=("halves only",), seed=97))
    # more tiles than the 4 x CUs co-resident slots, the remainder of the last round as 64-pixel halves (conv2d_launch: nbig)
    cs.append(_c(L, "k1-full-tiles-and-halves", 0, 8, 16, 8, 128, k=1, relu=1, groups=2, pad_in=0, pad_out=0,
                 edges=("full tiles + halves", "two groups"), walk=(1, 1), seed=98))
    return cs


def _direct_x():
    L, cs = "conv2d_x", []
    for res in ("own", "inplace"):
        e = "res own" if res == "own" else "res in place"
        cs.append(_c(L, "res-%s-1x1" % res, 1, 1, 1, 8, 8, x={"res": res}, edges=(e, "one pixel"), seed=101))
        cs.append(_c(L, "res-%s-px129" % res, 1, 3, 43, 16, 38, x={"res": res}, edges=(e, "BM+1", "head 38"), seed=102))
        cs.append(_c(L, "res-%s-px191-cin40" % res, 1, 191, 1, 40, 65, x={"res": res}, edges=(e, "BM+BM/2-1", "ck8", "BN+1"),
                     seed=103))
        cs.append(_c(L, "res-%s-2d" % res, 2, 2, 129, 16, 19, x={"res": res}, edges=(e, "2-D tiles", "head 19"), seed=104))
        cs.append(_c(L, "res-%s-cin136" % res, 2, 5, 6, 136, 24, x={"res": res}, edges=(e, "cin>=128", "images"), seed=105))
    for pre in ("neg", "pos", "both"):
        cs.append(_c(L, "pre-%s-px128" % pre, 2, 8, 8, 16, 24, relu=1, x={"preact": pre}, edges=("preact", "BM"), seed=110))
        cs.append(_c(L, "pre-%s-gaps" % pre, 2, 5, 7, 24, 38, pad_in=1, x={"preact": pre}, edges=("preact", "gap pixels", "ck8"),
                     seed=111))
    cs.append(_c(L, "pre-both-1x1", 1, 1, 1, 8, 8, x={"preact": "both"}, edges=("preact", "one pixel"), seed=112))
    # preact_cin < cin.  The header: channels >= preact_cin are staged as 0 whatever the buffer and the vectors hold there.
    # The -nan cases (NaN in the buffer's padded channels) meet that wording but cannot tell whether the kernel looks at
    # preact_cin at all: the pre-activation's ReLU is fmaxf(., 0), which promises nothing about NaN and turns it into 0 (header
    # section 2, "Non-finite values"), and the padded filter taps are zero.
    # The -inf cases can: the padded channels hold 1.0 and in_shift is +inf there, so a kernel that pre-activated them would
    # stage +inf, and inf x the zero tap is NaN in every output.
    cs.append(_c(L, "pre-cin21of24-inf", 2, 5, 7, 21, 24, relu=1, pad_in=2, x={"preact": "both", "inf_pad": 1},
                 edges=("preact", "cin padded", "gap pixels", "ck8"), seed=117))
    cs.append(_c(L, "pre-cin41of48-inf-2d", 1, 2, 131, 41, 65, x={"preact": "both", "inf_pad": 1},
                 edges=("preact", "cin padded", "2-D tiles", "ck16"), seed=118))
    cs.append(_c(L, "pre-cin21of24-nan", 2, 5, 7, 21, 24, relu=1, pad_in=2, x={"preact": "both", "nan_pad": 1},
                 edges=("preact", "cin padded", "gap pixels", "ck8"), seed=113))
    cs.append(_c(L, "pre-cin37of40-nan-2d", 1, 2, 131, 37, 65, x={"preact": "both", "nan_pad": 1},
                 edges=("preact", "cin padded", "2-D tiles"), seed=114))
    cs.append(_c(L, "pre-res-own-cin133of136-nan", 2, 9, 11, 133, 38, pad_in=1, x={"preact": "both", "nan_pad": 1, "res": "own"},
                 edges=("preact", "res own", "cin>=128", "gap pixels"), seed=115))
    cs.append(_c(L, "pre-res-inplace-px193", 1, 193, 1, 16, 64, x={"preact": "both", "res": "inplace"},
                 edges=("preact", "res in place", "BM+BM/2+1", "BN"), seed=116))
    return cs


def _first():
    cs = []
    for L, kind in (("conv_first", "f32"), ("conv_first_planes", "f32"), ("conv_first_bf16", "bf16")):
        t = {"tile": FIRST_TILE}
        for src in ("nchw", "layout"):
            x = dict(t, src=src)
            cs.append(_c(L, "%s-1x1" % src, 1, 1, 1, 3, 64, k=3, relu=1, kind=kind, x=x, edges=("one pixel",), seed=120))
            cs.append(_c(L, "%s-3x8x8" % src, 3, 8, 8, 3, 64, k=3, relu=1, kind=kind, x=x, edges=("images",), seed=121))
            cs.append(_c(L, "%s-2x13x37" % src, 2, 13, 37, 3, 64, k=3, relu=0 if src == "layout" else 1, kind=kind, x=x,
                         edges=("tile ragged", "tiles>1"), seed=122))
    # fp32 only: 3 persistent blocks per CU walk the tiles (conv_first.hip: blocks)
    for L in ("conv_first", "conv_first_planes"):
        cs.append(_c(L, "walk", 0, 3, 5, 3, 64, k=3, relu=1, x={"tile": FIRST_TILE, "src": "nchw"}, edges=("walk",), walk=(2.5, 1),
                     seed=123))
    return cs


def _stem():
    L, cs = "conv7x7_s2", []
    # W (H) for an output 31 / 32 / 33 wide (15 / 16 / 17 high): odd and even inputs of both
    geo = [(29, 61, ("ho 15", "wo 31", "odd H", "odd W")), (30, 62, ("ho 15", "wo 31", "even H", "even W")),
           (31, 64, ("ho 16", "wo 32", "odd H", "even W")), (32, 63, ("ho 16", "wo 32", "even H", "odd W")),
           (33, 65, ("ho 17", "wo 33", "odd H", "odd W")), (34, 66, ("ho 17", "wo 33", "even H", "even W"))]
    for src in ("nchw", "layout"):
        x = {"tile": STEM_TILE, "src": src}
        for h, w, e in geo:
            cs.append(_c(L, "%s-%dx%d" % (src, h, w), 1, h, w, 3, 64, k=7, relu=1, x=x, edges=e, seed=130 + h))
        cs.append(_c(L, "%s-1x1" % src, 1, 1, 1, 3, 64, k=7, x=x, edges=("one pixel",), seed=131))
        cs.append(_c(L, "%s-2x70x9" % src, 2, 70, 9, 3, 64, k=7, relu=1, x=x, edges=("images", "row tiles>1"), seed=132))
    # outputs 31 / 32 / 33 rows high: around the 32-row tile (narrow maps: one column tile, ragged)
    for h, w, e in ((61, 9, ("ho 31", "odd H")), (64, 10, ("ho 32", "even H")), (65, 37, ("ho 33", "odd H", "row tiles>1", "tile ragged")),
                    (66, 12, ("ho 33", "even H", "row tiles>1"))):
        cs.append(_c(L, "nchw-%dx%d" % (h, w), 1, h, w, 3, 64, k=7, relu=1, x={"tile": STEM_TILE, "src": "nchw"}, edges=e,
                     seed=134 + h))
    cs.append(_c(L, "walk", 0, 5, 7, 3, 64, k=7, relu=1, x={"tile": STEM_TILE, "src": "nchw"}, edges=("walk",), walk=(2.5, 1),
                 seed=133))
    return cs


def _pairs():
    cs = []
    for L, kind in (("pair", "f32"), ("pair_bf16", "bf16")):
        for mid in (128, 512):
            e = ("mid %d" % mid,)
            shapes = [("PAIR_BM-1", 1, 7, 9), ("PAIR_BM", 2, 4, 8), ("PAIR_BM+1", 1, 5, 13), ("BM+1", 3, 1, 43)]
            for edge, n, h, w in shapes:
                for cout in ((38, 19) if edge in ("PAIR_BM+1", "BM+1") else (38,)):
                    outs = (False, True) if (kind == "bf16" and edge == "PAIR_BM+1") else (False,)
                    for of in outs:
                        cs.append(_c(L, "mid%d-px%d-cout%d%s" % (mid, n * h * w, cout, "-f32out" if of else ""), n, h, w, 128, cout,
                                     groups=2, pad_in=0, pad_out=3, kind=kind, out_f32=of, x={"mid": mid},
                                     edges=e + (edge, "head %d" % cout, "two groups"), seed=140 + mid + cout))
            cs.append(_c(L, "mid%d-1x1" % mid, 1, 1, 1, 128, 38, groups=1, pad_in=0, pad_out=0, kind=kind, x={"mid": mid},
                         edges=e + ("one pixel",), seed=141 + mid))
    return cs


def _bf16_like(L, kind, outs, families=("int",)):
    cs = []
    for fam in families:
        f = "" if fam == "int" else fam + "-"
        small = fam != "int"                      # wide operands: keep cin k^2 small (S)
        for of in outs:
            t = f + ("f32out-" if of else "")
            kw = dict(kind=kind, out_f32=of, family=fam)
            for k in (1, 3, 7):
                cs.append(_c(L, "%sk%d-1x1" % (t, k), 1, 1, 1, 16, 8, k=k, edges=("one pixel", "one chunk"), seed=150 + k, **kw))
                for e, n, h, w in (("BM-1", 1, 127, 1), ("BM", 2, 8, 8), ("BM+1", 1, 3, 43), ("BM+BM/2-1", 1, 191, 1),
                                   ("BM+BM/2", 3, 8, 8), ("BM+BM/2+1", 1, 193, 1)):
                    if small and (e in ("BM", "BM+BM/2") or (of and e == "BM+BM/2+1")):     # (the wide families: the ragged
                        continue                                                            # counts, 193 with the split output)
                    cs.append(_c(L, "%sk%d-px%d" % (t, k, n * h * w), n, h, w, 16, 24, k=k, relu=1, edges=(e, "strip"),
                                 seed=151 + k + n * h * w, **kw))
            for k in (1, 3):
                wide_w = (STRIP_MAXW_BF16 if kind == "bf16" else STRIP_MAXW) + 1          # the launcher's own strip width + 1
                cs.append(_c(L, "%sk%d-W%d" % (t, k, wide_w), 1, 3, wide_w, 16, 24, k=k, relu=1,
                             edges=("W=STRIP_MAXW+1", "2-D tiles"), seed=152 + k, **kw))
                cs.append(_c(L, "%sk%d-pool" % (t, k), 2, 6, 10, 16, 24, k=k, relu=1, pool=1, edges=("pool", "2-D tiles", "images"),
                             seed=153 + k, **kw))
                for cin in (21, 48) if small else (21, 48, 144):
                    cs.append(_c(L, "%sk%d-cin%d" % (t, k, cin), 1, 5, 6, cin, 24, k=k, relu=1,
                                 edges=(("cin padded",) if cin % 16 else ("odd chunks",)) + (("cin>=128",) if cin >= 128 else ()),
                                 seed=154 + cin + k, **kw))
                for cout, e in ((63, "BN-1"), (64, "BN"), (65, "BN+1"), (38, "head 38"), (19, "head 19")):
                    if small and cout in (63, 65):
                        continue
                    cs.append(_c(L, "%sk%d-cout%d" % (t, k, cout), 1, 5, 6, 16, cout, k=k, relu=0 if cout < 60 else 1, edges=(e,),
                                 seed=155 + cout + k, **kw))
            cs.append(_c(L, "%sk1-cin512" % t, 1, 5, 6, 512 if not small else 64, 19, k=1, edges=("head 19",), seed=156, **kw))
            cs.append(_c(L, "%sk7-cin128" % t, 1, 4, 5, 128 if not small else 32, 128, k=7, relu=1, edges=("128-column tile",), seed=157, **kw))
            for k in (1, 3, 7):
                cs.append(_c(L, "%sk%d-groups2" % (t, k), 2, 6, 7, 16, 38 if k == 1 else 64, k=k, relu=1, groups=2,
                             edges=("two groups", "images"), seed=158 + k, **kw))
    return cs


def _bf16():
    cs = _bf16_like("conv2d_bf16", "bf16", (False, True))
    # k x k strips: 2 persistent blocks per CU walk the full tiles once there are more than 2 x CUs of them (npersist)
    cs.append(_c("conv2d_bf16", "k3-walk", 0, 8, 16, 16, 8, k=3, relu=1, kind="bf16", edges=("walk",), walk=(2.5, 1), seed=159))
    cs.append(_c("conv2d_bf16", "k7-walk-f32out", 0, 8, 16, 16, 8, k=7, relu=1, kind="bf16", out_f32=True, edges=("walk",),
                 walk=(2.5, 1), seed=160))
    # the network's own configuration: cout % 64 == 0 into an aligned layout, the transposed epilogue (`tr`), walked
    cs.append(_c("conv2d_bf16", "k3-walk-cout64-tr", 0, 8, 16, 16, 64, k=3, relu=1, kind="bf16",
                 edges=("walk", "transposed epilogue"), walk=(2.5, 1), seed=161))
    # the deep 3x3 layers: 64-channel chunks (conv_ck), strips and 2-D tiles
    cs.append(_c("conv2d_bf16", "k3-cin256-ck64", 2, 5, 6, 256, 64, k=3, relu=1, kind="bf16",
                 edges=("ck64", "strip", "transposed epilogue", "images"), seed=162))
    cs.append(_c("conv2d_bf16", "k3-cin256-ck64-2d", 1, 3, 65, 256, 24, k=3, relu=1, kind="bf16", edges=("ck64", "2-D tiles"),
                 seed=163))
    return cs


def _c64():
    L, cs, t = "c64", [], {"tile": C64_TILE}
    kw = dict(k=3, kind="bf16", entry="c64", x=t)
    cs.append(_c(L, "1x1", 1, 1, 1, 64, 64, edges=("one pixel",), seed=170, **kw))
    cs.append(_c(L, "16x32", 2, 16, 32, 64, 64, relu=1, edges=("images",), seed=171, **kw))
    cs.append(_c(L, "17x33-cout128", 1, 17, 33, 64, 128, relu=1, edges=("tile ragged", "tiles>1"), seed=172, **kw))
    cs.append(_c(L, "pool-18x34", 2, 18, 34, 64, 64, relu=1, pool=1, edges=("tile ragged", "tiles>1", "images"), seed=173, **kw))
    cs.append(_c(L, "15x31-norelu", 1, 15, 31, 64, 64, pad_in=3, pad_out=3, edges=("tile ragged",), seed=174, **kw))
    cs.append(_c(L, "walk", 0, 3, 5, 64, 64, relu=1, edges=("walk",), walk=(2.5, 1), seed=175, **kw))
    cs.append(_c(L, "walk-pool-cout128", 0, 4, 6, 64, 128, relu=1, pool=1, edges=("walk",), walk=(2.5, 2), seed=176, **kw))
    return cs


def _x3():
    cs = _bf16_like("conv2d_bf16x3", "x3", (False, True), families=("int", "xwide", "wwide"))
    cs.append(_c("conv2d_bf16x3", "xwide-k3-walk", 0, 8, 16, 16, 8, k=3, relu=1, kind="x3", family="xwide", edges=("walk",),
                 walk=(2.5, 1), seed=180))
    return cs


def _wino2():
    L, cs = "wino2", []
    kw = dict(k=3, m=2)
    for tag, h, w, e in (("m", 2, 2, "m"), ("m-1", 1, 1, "m-1"), ("m+1", 3, 3, "m+1"), ("2m+1", 5, 5, "2m+1")):
        cs.append(_c(L, "%s-cin32" % tag, 2, h, w, 32, 24, relu=1, edges=(e, "small grid", "images"), seed=190 + h, **kw))
        cs.append(_c(L, "%s-cin24-ck8" % tag, 1, h, w, 24, 38, edges=(e, "plain grid"), seed=191 + h, **kw))
    cs.append(_c(L, "groups2", 2, 7, 9, 32, 128, relu=1, groups=2, edges=("two groups", "small grid"), seed=192, **kw))
    cs.append(_c(L, "prelu", 2, 6, 5, 48, 65, prelu=1, edges=("small grid",), seed=193, **kw))
    cs.append(_c(L, "pool", 2, 6, 10, 16 * 2, 64, relu=1, pool=1, edges=("small grid",), seed=194, **kw))
    cs.append(_c(L, "noex", 1, 9, 7, 32, 64, relu=1, entry="noex", edges=("small grid",), seed=195, **kw))
    # cin 24: 8-channel chunks, which have no small-grid form - the whole-tile kernel, one block per tile, at any grid
    cs.append(_c(L, "plain-grid", 1400, 4, 6, 24, 64, relu=1, edges=("plain grid",), seed=196, **kw))
    # more tiles than CUs: persistent blocks walk them (wino_f32), 2.5 rounds with a ragged last one
    cs.append(_c(L, "walk", 0, 1, 2, 32, 128, relu=1, edges=("walk", "persistent"), walk=(2.5, 1.0 / 32), seed=197, **kw))
    cs.append(_c(L, "walk-64", 0, 2, 1, 24, 64, relu=1, edges=("walk", "persistent"), walk=(2.5, 1.0 / 64), seed=198, **kw))
    # conv1_2's instance: the 64-column block with 16-channel chunks on a grid that is not small (wino_f32<2, 2, 16>)
    cs.append(_c(L, "walk-64-ck16", 0, 2, 1, 32, 64, relu=1, edges=("walk", "persistent", "wino ck16 64 columns"),
                 walk=(2.5, 1.0 / 64), seed=199, **kw))
    return cs


def _families(cases, limit=2500):
    """the fp32 cases again with 9-bit x ('xwide') and with 9-bit w ('wwide'), where cin k^2 keeps S far below 2^24"""
    more = [c._replace(tag="%s-%s" % (fam, c.tag), family=fam) for fam in ("xwide", "wwide") for c in cases
            if c.cin * c.k * c.k <= limit]
    return cases + more


EXACT_CASES = {
    "conv2d": _families(_direct_f32()),
    "conv2d_x": _families(_direct_x()),
    "conv_first": _families([c for c in _first() if c.launcher == "conv_first"]),
    "conv_first_planes": _families([c for c in _first() if c.launcher == "conv_first_planes"]),
    "conv_first_bf16": [c for c in _first() if c.launcher == "conv_first_bf16"],
    "conv7x7_s2": _families(_stem()),
    "pair": _families([c for c in _pairs() if c.launcher == "pair"]),
    "pair_bf16": [c for c in _pairs() if c.launcher == "pair_bf16"],
    "conv2d_bf16": _bf16(),
    "c64": _c64(),
    "conv2d_bf16x3": _x3(),
    "wino2": _families(_wino2()),
}


def all_cases():
    return [c for cs in EXACT_CASES.values() for c in cs]


def case_id(c):
    return c.tag
