"""Host restatement of the bf16 PReLU passes of a layout-resident training run (include/rtpose_mi355x.h section 2b continued,
csrc/prelu_backward.hip, train.dense_stage): rtpose_prelu_bf16 and rtpose_prelu_grad_bf16 as the restatements of
tests/prelu_restate.py - a select or one numpy-float32 multiply, on the one numpy-float32 sum ga + gb - followed by
layout_restate.bf16_rne, and the cases and operands tests/test_prelu_bf16_gpu.py runs.  torch CPU + numpy only: no GPU, no
library call.

A NaN has no bits to pin here: the header promises that a NaN stays a NaN, and a NaN of its sign where the value only
travels (z > 0 and a single consumer: out is ga rounded).  The restatements return 0x7FC0 | sign for every NaN and
``same_bf16`` compares two results as "equal bits, or NaN in both".

The exact operand sets: z in -3 .. 3, ga and gb in +-{1, 2, 3} (so |g| <= 6), slopes the quarters of prelu_restate.SLOPES:
y, out and every term of dslope are multiples of 1/4 of at most 8 significant bits - bf16 holds them - and sums of |z g| below
2^24, so the float64 reference is compared with ==."""
from collections import namedtuple

import numpy as np
import torch

import layout_restate as lr
import prelu_restate as pr

NAN16 = 0x7FC0


def is_nan32(bits):
    bits = np.asarray(bits, dtype=np.uint32)
    return (bits & 0x7FFFFFFF) > 0x7F800000


def is_nan16(h):
    h = np.asarray(h, dtype=np.uint16)
    return (h & 0x7FFF) > 0x7F80


def round_bits(f32_bits):
    """fp32 bit patterns -> bf16 bit patterns (uint16), round to nearest even; a NaN becomes NAN16 with its sign"""
    b = np.ascontiguousarray(f32_bits, dtype=np.uint32)
    nan = is_nan32(b)
    h = lr.bf16_rne(np.where(nan, np.uint32(0), b).view(np.float32))
    return np.where(nan, (NAN16 | ((b >> 16) & 0x8000)).astype(np.uint16), h).astype(np.uint16)


def same_bf16(got, want):
    """element-wise: the same 16 bits, or a NaN in both"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    return (got == want) | (is_nan16(got) & is_nan16(want))


def bf16_f64(h):
    return lr.bf16_to_f32(np.ascontiguousarray(h, dtype=np.uint16)).astype(np.float64)


def sum_bits(ga_bits, gb_bits):
    """g = gb is None ? ga : ga + gb, one float32 add, as bits"""
    ga_bits = np.asarray(ga_bits, dtype=np.uint32)
    if gb_bits is None:
        return ga_bits
    with np.errstate(invalid="ignore", over="ignore"):
        return (ga_bits.view(np.float32) + np.asarray(gb_bits, dtype=np.uint32).view(np.float32)).astype(np.float32).view(np.uint32)


def prelu_bf16_bits(z, slope):
    """y = bf16(z >= 0 ? z : slope * z) on float32 arrays [n, c, h, w] / [c], as uint16"""
    return round_bits(pr.prelu_bits(z, slope))


def prelu_grad_bf16_bits(z, ga_bits, gb_bits, slope):
    """out = bf16(z > 0 ? g : slope * g), g = ga + gb (gb_bits None: ga), as uint16"""
    return round_bits(pr.prelu_grad_bits(z, sum_bits(ga_bits, gb_bits), slope))


def grad64(z, ga, gb, slope):
    """(dz, dslope, S) in float64 from F.prelu's CPU autograd on the float32 sum g = ga + gb (torch tensors; gb may be None)"""
    g = ga if gb is None else ga + gb
    _, dz, da, s = pr.prelu64(z, g, slope)
    return dz, da, s


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# z / ga / gb: (cstride, choff) of the fp32 buffers, out: of the bf16 one; the gaps differ as well (layouts()).  "vector":
# every fp32 cstride and choff a multiple of 4 floats and the bf16 ones multiples of 4 elements - 16-byte loads and an 8-byte
# store; "scalar" otherwise.  The shapes are prelu_restate.CASES'.
Case = namedtuple("Case", "channels n h w z ga gb out tags")
CASES = [
    Case(1, 1, 1, 1, (1, 0), (2, 1), (3, 2), (5, 3), "scalar; P = 1; one element"),
    Case(3, 1, 2, 2, (5, 2), (8, 4), (4, 1), (7, 3), "scalar; four layouts, slices end at cstride"),
    Case(19, 2, 5, 3, (24, 4), (20, 0), (28, 8), (24, 4), "vector; a last unit of 3 channels"),
    Case(52, 1, 4, 4, (56, 0), (52, 0), (60, 8), (156, 52), "vector; 13 units; a slice of a concat buffer"),
    Case(96, 2, 9, 7, (96, 0), (288, 96), (96, 0), (288, 192), "vector; several slabs; ga a slice of a concat gradient"),
    Case(130, 1, 3, 11, (136, 4), (137, 5), (136, 4), (136, 4), "scalar; three channel tiles of 64 units"),
    Case(130, 1, 3, 11, (136, 4), (136, 0), (132, 0), (140, 8), "vector; 33 units: 7 rows, 25 idle threads, last unit of 2"),
    Case(8, 1, 1, 1537, (9, 1), (12, 4), (8, 0), (9, 1), "scalar; several slabs; P = 1537: one pixel in the last slab"),
    Case(8, 3, 19, 18, (12, 4), (12, 4), (16, 8), (20, 12), "vector; several slabs across image boundaries"),
    Case(512, 1, 4, 4, (520, 4), (520, 4), (512, 0), (516, 4), "vector; two channel tiles"),
    Case(128, 2, 46, 46, (128, 0), (384, 128), (128, 0), (384, 256), "vector; several slabs; the largest"),
    Case(8, 1, 1, 63, (8, 0), (8, 0), (8, 0), (8, 0), "vector; P = 63 = slab - 1"),
    Case(8, 1, 1, 64, (8, 0), (8, 0), (8, 0), (8, 0), "vector; P = 64 = slab"),
    Case(8, 1, 1, 65, (8, 0), (8, 0), (8, 0), (10, 2), "scalar (the bf16 slice alone); several slabs; P = 65 = slab + 1"),
    Case(8, 2, 8, 8, (8, 0), (8, 0), (8, 0), (8, 0), "vector; several slabs; P = 2 slabs, full"),
]


def case_id(c):
    return "c%d_%dx%dx%d_z%d.%d_a%d.%d_b%d.%d_o%d.%d" % ((c.channels, c.n, c.h, c.w) + c.z + c.ga + c.gb + c.out)


def layouts(c):
    """(lz, lga, lgb, lout): the four buffers have gaps of 1, 0, 2 and 1 pixels"""
    return (lr.padded(c.z[0], c.h, c.w, 1, c.z[1]), lr.padded(c.ga[0], c.h, c.w, 0, c.ga[1]),
            lr.padded(c.gb[0], c.h, c.w, 2, c.gb[1]), lr.padded(c.out[0], c.h, c.w, 1, c.out[1]))


def is_vector(c, two=True):
    """whether the launch takes the 4-channel units (`two`: with gb)"""
    return all(v % 4 == 0 for pair in (c.z, c.ga, c.out) + ((c.gb,) if two else ()) for v in pair)


def as_prelu_case(c):
    """the prelu_restate.Case of the same shape with gy in ga's place and a dense fp32 out: what rtpose_prelu_grad runs on
    the summed gradient"""
    cs = (c.channels + 3) // 4 * 4
    return pr.Case(c.channels, c.n, c.h, c.w, c.z, (cs, 0), (cs, 0), c.tags)


# ---- operands -----------------------------------------------------------------------------------------------------------------------
def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_mixed(c, seed=0):
    """(z, ga, gb, slope): z in {-3 .. 3} with zeros, ga and gb in +-{1, 2, 3}, slopes cycling through prelu_restate.SLOPES"""
    g = torch.Generator().manual_seed(6000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    z = _ri(g, -3, 3, *shape)
    ga = _ri(g, 1, 3, *shape) * (2 * _ri(g, 0, 1, *shape) - 1)
    gb = _ri(g, 1, 3, *shape) * (2 * _ri(g, 0, 1, *shape) - 1)
    return z, ga, gb, pr.slopes(c.channels)


def exact_negative(c, seed=0):
    """(z, ga, gb, slope): z in {-3, -2, -1}, ga and gb in {1, 2, 3}: every term of dslope is strictly negative, so one
    missing or doubled pixel changes the sum of every channel"""
    g = torch.Generator().manual_seed(7000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    return _ri(g, -3, -1, *shape), _ri(g, 1, 3, *shape), _ri(g, 1, 3, *shape), pr.slopes(c.channels)


EXACT_SETS = {"mixed": exact_mixed, "negative": exact_negative}


def exact_margin(z, ga, gb):
    """S = max over channels of sum |z| (|ga| + |gb|): below 2^24 fp32 sums of the terms z * g are exact in any order"""
    return (z.double().abs() * (ga.double().abs() + gb.double().abs())).sum((0, 2, 3)).max().item()


SPECIALS = (0x7FC00777, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000)


def random_operands(c, seed=0):
    """(z, ga_bits, gb_bits, slope): randn z with exact zeros of both signs; randn ga and gb; on pixels where z > 0 ga holds
    NaNs of both signs (a signalling one too), -0, both Infs and subnormals in turn, gb a -0 under ga's -0 and an Inf of the
    other sign under ga's +Inf (their sum is NaN); subnormals in gb wherever z <= 0 allows (every 13th).  Slopes
    randn * 0.25 with both signs present where there are two channels.  The terms of dslope (z <= 0) stay finite."""
    g = torch.Generator().manual_seed(8000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    z = torch.randn(*shape, generator=g)
    ga = torch.randn(*shape, generator=g)
    gb = torch.randn(*shape, generator=g)
    slope = torch.randn(c.channels, generator=g) * 0.25
    if c.channels >= 2:
        slope[0], slope[1] = -slope[0].abs() - 0.01, slope[1].abs() + 0.01
    zf = z.view(-1)
    if zf.numel() >= 8:
        zf[1::7] = 0.0
        zf[2::11] = -0.0
    ga_bits, gb_bits = ga.numpy().view(np.uint32).copy(), gb.numpy().view(np.uint32).copy()
    fa, fb = ga_bits.reshape(-1), gb_bits.reshape(-1)
    where = np.flatnonzero((z.numpy() > 0).reshape(-1))
    for i, s in enumerate(SPECIALS):
        fa[where[i::2 * len(SPECIALS)]] = s
    fb[where[3::2 * len(SPECIALS)]] = 0x80000000          # -0 + -0 = -0
    fb[where[4::2 * len(SPECIALS)]] = 0xFF800000          # +Inf + -Inf = NaN
    rest = np.flatnonzero((z.numpy() <= 0).reshape(-1))
    fb[rest[::13]] = 0x00000003
    return z, ga_bits, gb_bits, slope


def sweep_operands():
    """(z_bits [1, 4, 512, 512], slope [4]): every 16-bit upper half of z times the lower halves 0x0000, 0x7FFF, 0x8000 and
    0x8001 - ties, just below and just above them, under a round-to-even and a round-to-odd upper half -, in two channels with
    a positive and in two with a negative slope"""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    bits = np.concatenate([hi | lo for lo in (0x0000, 0x7FFF, 0x8000, 0x8001)]).astype(np.uint32)
    z = np.stack([bits] * 4).reshape(1, 4, 512, 512)
    return z, torch.tensor([0.3, -0.7, 2.0, -0.001])
