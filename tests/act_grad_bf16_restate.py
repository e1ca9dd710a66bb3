"""Host restatement of rtpose_relu_grad_bf16 (include/rtpose_mi355x.h section 2b, csrc/act_grad_bf16.hip) on uint16 views,
and the grid the GPU test runs.  numpy only: no GPU, no library call.

    out = y > 0 ? gy : +0        on bf16 bit patterns: y is positive when 0x0001 <= y <= 0x7f80 (subnormals and +Inf
                                 included; +-0, NaN and every negative are not); where it is, out is gy's 16 bits untouched

tests/test_act_grad_bf16_cpu.py holds this against torch.where on bfloat16 tensors over all 65,536 patterns of y."""
from collections import namedtuple

import numpy as np

import layout_restate as lr

SENTINEL16 = 0x7FC1          # a quiet bf16 NaN with a payload no operand below holds


def relu_grad_bf16_bits(y_bits, gy_bits):
    """uint16 arrays of one shape -> uint16"""
    y = np.asarray(y_bits, dtype=np.uint16)
    g = np.asarray(gy_bits, dtype=np.uint16)
    return np.where((y >= 0x0001) & (y <= 0x7F80), g, np.uint16(0)).astype(np.uint16)


# +0, -0, NaNs of both signs (quiet, signalling), +-Inf, the smallest subnormals of both signs, the largest subnormal, the
# smallest and largest normals, -1, 1
Y_SPECIAL = np.array([0x0000, 0x8000, 0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F,
                      0xFF7F, 0xBF80, 0x3F80], dtype=np.uint16)
# NaNs with payloads, +-Inf, +-0, a subnormal: what must pass through untouched
GY_SPECIAL = np.array([0x7FC7, 0xFFD3, 0x7F85, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0003, 0x3F80, 0xC2F7], dtype=np.uint16)

N, H, W = 3, 5, 7
CSTRIDE = 64
CHANNELS = (1, 8, 19, 38, 48)
CHOFFS = (0, 8, 3)                        # 0 and 8: 16-byte pieces; 3: element by element
GAPS = ((0, 1, 3), (1, 3, 0), (3, 0, 1))  # (y, gy, out of place out)
SHIFTS = ((0, 0, 0), (1, 0, 0), (0, 4, 4))  # elements the bases of (y, gy, out) sit past a 16-byte boundary

Case = namedtuple("Case", "channels choff gaps shifts inplace")


def cases(channels, choff):
    return [Case(channels, choff, g, s, ip) for g in GAPS for s in SHIFTS for ip in (False, True)]


def is_vector(c):
    return c.choff % 8 == 0 and CSTRIDE % 8 == 0 and not any(c.shifts)


def layouts(c):
    """(ly, lgy, lout): lout is lgy in place"""
    ly, lgy, lout = (lr.padded(CSTRIDE, H, W, gap, c.choff) for gap in c.gaps)
    return ly, lgy, (lgy if c.inplace else lout)


def operands(c, seed=0):
    """(y bits, gy bits) [N, channels, H, W] uint16: random patterns of every class with the special ones written over the
    first elements - every special y meets a plain gy and some meet a special one"""
    g = np.random.default_rng(1000 * c.channels + 10 * c.choff + seed)
    shape = (N, c.channels, H, W)
    y = g.integers(0, 1 << 16, size=shape, dtype=np.uint32).astype(np.uint16)
    gy = g.integers(0, 1 << 16, size=shape, dtype=np.uint32).astype(np.uint16)
    # (a random gy must not look like the sentinel: the test tells writes from sentinels by value)
    gy[gy == SENTINEL16] = 0x3F80
    yf, gf = y.reshape(-1), gy.reshape(-1)
    yf[:Y_SPECIAL.size] = Y_SPECIAL
    gf[Y_SPECIAL.size // 2:Y_SPECIAL.size // 2 + GY_SPECIAL.size] = GY_SPECIAL
    for j, v in enumerate(GY_SPECIAL):          # and every special gy under a positive y
        yf[Y_SPECIAL.size + GY_SPECIAL.size + j] = 0x3F80
        gf[Y_SPECIAL.size + GY_SPECIAL.size + j] = v
    return y, gy
