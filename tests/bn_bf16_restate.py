"""Host restatement of the bf16 BatchNorm passes of a layout-resident training run (include/rtpose_mi355x.h section 2b
continued, csrc/batchnorm.hip, train.preact_chain): rtpose_bn_apply_bf16 and the dx of rtpose_bn_grad_bf16 as the fp32
restatements of tests/bn_restate.py followed by the rounding of tests/prelu_bf16_restate.py (layout_restate.bf16_rne; a NaN
is a NaN of its sign), and the cases and operands tests/test_batchnorm_bf16_gpu.py runs.  torch CPU + numpy only: no GPU, no
library call.

The ReLU of the forward is restated here as the kernel documents it, y <= 0 ? +0 : y, so that a NaN y stays NaN
(bn_restate.apply_restate selects with y > 0, which its own tests never feed a NaN).

The exact (dyadic) sets.  The element-wise passes read per-channel vectors, so an exact set GIVES them: scale, shift, mean,
invstd and weight are small dyadic numbers, x and gy small integers, and P is a power of two where the gradient runs.  Then
every product and sum of y = scale x + shift, of G1, G2, dweight, A, B = A G1 / P, C = A invstd dweight / P and of
dx = (g A - B) - (x - mean) C is a dyadic number of few bits: fp64 and fp32 hold each one exactly (``exact_in_fp32`` is the
condition, asserted on the float64 values), and the kernel's bf16 result is the float64 value rounded once."""
from collections import namedtuple

import numpy as np
import torch

import bn_restate as br
import layout_restate as lr
from prelu_bf16_restate import NAN16, bf16_f64, is_nan16, is_nan32, round_bits, same_bf16  # noqa: F401  (the rounding, shared)


def _c(v):
    return np.asarray(v).reshape(1, -1, 1, 1)


def apply_f32_restate(x, save, relu):
    """rtpose_bn_apply's fp32 y: fl(fl(scale x) + shift), then y <= 0 ? +0 : y if relu (a NaN y stays NaN)"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = br.apply_restate(x, save, False)
        return np.where(y <= 0, np.float32(0), y).astype(np.float32) if relu else y


def apply_bf16_restate(x, save, relu):
    """y of rtpose_bn_apply_bf16 as uint16 [n, c, h, w]"""
    return round_bits(apply_f32_restate(x, save, relu).view(np.uint32))


def dx_bf16_restate(x, gy, save, coef, relu):
    """dx of rtpose_bn_grad_bf16 as uint16 [n, c, h, w]: bn_restate.dx_restate (the mask is scale x + shift > 0: a NaN passes
    nothing) rounded"""
    with np.errstate(invalid="ignore", over="ignore"):
        return round_bits(br.dx_restate(x, gy, save, coef, relu).view(np.uint32))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
# bn_restate.CASES' rows (channels, n, h, w and the fp32 layouts of x and gy) with a bf16 destination each: its (cstride,
# choff) in ELEMENTS, its gap in pixels (0, 1, 3) and `shift`, the elements its base is moved by (2 bytes each).  "vector":
# every fp32 cstride and choff a multiple of 4 floats AND the bf16 cstride and choff multiples of 4 elements on an 8-byte
# base; "scalar" otherwise - for either reason alone, or both.
Case = namedtuple("Case", "channels n h w x gy out gap shift tags")
_DEST = [((3, 2), 0, 0), ((8, 4), 1, 0), ((8, 4), 3, 0), ((8, 0), 1, 0), ((7, 1), 0, 0), ((64, 0), 1, 0), ((68, 4), 3, 0),
         ((67, 1), 0, 0), ((256, 0), 1, 0), ((258, 2), 0, 0), ((260, 0), 3, 0), ((264, 4), 1, 0), ((16, 8), 1, 0), ((32, 0), 3, 0),
         ((8, 0), 0, 1), ((8, 0), 0, 0)]
assert len(_DEST) == len(br.CASES)


def _tags(b, out, shift):
    fp32_vec = all(v % 4 == 0 for pair in (b.x, b.gy) for v in pair)
    dest_vec = out[0] % 4 == 0 and out[1] % 4 == 0 and shift % 4 == 0
    how = "vector" if fp32_vec and dest_vec else "scalar (%s)" % ("both" if not fp32_vec and not dest_vec else
                                                                    "the fp32 slices alone" if dest_vec else "the bf16 slice alone")
    return how + "; " + b.tags.split("; ", 1)[1]


CASES = [Case(b.channels, b.n, b.h, b.w, b.x, b.gy, out, gap, shift, _tags(b, out, shift))
         for b, (out, gap, shift) in zip(br.CASES, _DEST)]
BIG = CASES[15]                       # 6 channels at 129 x 511: one test only
SMALL = [c for c in CASES if c is not BIG]


def case_id(c):
    return "c%d_%dx%dx%d_x%d.%d_g%d.%d_o%d.%d_gap%d_s%d" % ((c.channels, c.n, c.h, c.w) + c.x + c.gy + c.out + (c.gap, c.shift))


def layouts(c):
    """(lx, lgy, lout): gaps of 1 and 2 pixels around the fp32 buffers (bn_restate.layouts), the case's own around the bf16 one"""
    return (lr.padded(c.x[0], c.h, c.w, 1, c.x[1]), lr.padded(c.gy[0], c.h, c.w, 2, c.gy[1]),
            lr.padded(c.out[0], c.h, c.w, c.gap, c.out[1]))


def is_vector(c):
    return all(v % 4 == 0 for pair in (c.x, c.gy, c.out) for v in pair) and c.shift % 4 == 0


def base_case(c):
    """the bn_restate.Case of the same shape and fp32 layouts (its fp32 `out` is dense, 4-aligned)"""
    cs = (c.channels + 3) // 4 * 4
    return br.Case(c.channels, c.n, c.h, c.w, c.x, c.gy, (cs, 0), c.tags)


# ---- exact (dyadic) operand sets -----------------------------------------------------------------------------------------------------
def is_pow2(p):
    return p & (p - 1) == 0


def exact_in_fp32(a64):
    a64 = np.asarray(a64, np.float64)
    return bool((a64.astype(np.float32).astype(np.float64) == a64).all())


def exact_set(c, seed=0):
    """(x, gy, save [6, ch], weight): x in -4 .. 4 around an integer per-channel mean, gy in -3 .. 3, invstd in {1/2, 1, 2},
    weight in {1/2, -1, 2, 1/4, 1}, bias in quarters; scale = weight invstd and shift = bias - mean scale, exact"""
    g = torch.Generator().manual_seed(4000 + seed)
    ch, shape = c.channels, (c.n, c.channels, c.h, c.w)
    mean = torch.randint(-8, 9, (ch,), generator=g).double()
    x = (torch.randint(-4, 5, shape, generator=g).double() + mean.view(1, -1, 1, 1)).float()
    gy = torch.randint(-3, 4, shape, generator=g).float()
    invstd = torch.tensor([(0.5, 1.0, 2.0)[i % 3] for i in range(ch)], dtype=torch.float64)
    weight = torch.tensor([(0.5, -1.0, 2.0, 0.25, 1.0)[i % 5] for i in range(ch)], dtype=torch.float64)
    bias = torch.tensor([(0.0, 1.0, -0.5, 3.0, 0.25)[i % 5] for i in range(ch)], dtype=torch.float64)
    scale = weight * invstd
    shift = bias - mean * scale
    var = 1.0 / (invstd * invstd)            # (never read by the two passes)
    save = torch.stack([mean, var, invstd, scale, shift, torch.zeros(ch, dtype=torch.float64)]).float().numpy()
    return x, gy, save, weight.float()


def exact64(x, gy, save, weight, relu):
    """float64 (y, dx, dbias, dweight, coef [3, ch]) by the header's expressions from the GIVEN per-channel vectors"""
    x64, g64 = x.double().numpy(), gy.double().numpy()
    s = save.astype(np.float64)
    p = float(x64.shape[0] * x64.shape[2] * x64.shape[3])
    pre = _c(s[3]) * x64 + _c(s[4])
    y = np.where(pre <= 0, 0.0, pre) if relu else pre
    g = np.where(pre > 0, g64, 0.0) if relu else g64
    k = x64[0, :, 0, 0]
    g1, g2 = g.sum((0, 2, 3)), (g * (x64 - _c(k))).sum((0, 2, 3))
    mean, invstd, w = s[0] + s[5], s[2], weight.double().numpy()
    dw = invstd * (g2 - (mean - k) * g1)
    a = w * invstd
    coef = np.stack([a, a * g1 / p, a * invstd * dw / p])
    dx = (g * _c(coef[0]) - _c(coef[1])) - (x64 - _c(s[0])) * _c(coef[2])
    return y, dx, g1, dw, coef


# ---- random operands ------------------------------------------------------------------------------------------------------------------
def random_operands(c, seed=0, big_mean=False):
    """(x, gy, weight, bias, running_mean, running_var): bn_restate's (mean = 1000 std with `big_mean`)"""
    x, gy = br.random_operands(base_case(c), seed=seed, big_mean=big_mean)
    return (x, gy) + br.affine(c.channels, False)


LOWER_HALVES = (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def sweep_bits():
    """every 16-bit upper half under the five lower halves - ties, just below and above them and the largest, under a
    round-to-even and a round-to-odd upper half: uint32 [5 * 65536]"""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    return np.concatenate([hi | lo for lo in LOWER_HALVES]).astype(np.uint32)
