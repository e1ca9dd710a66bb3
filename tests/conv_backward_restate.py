"""Host restatement of the backward pass of the stride-1 "same" convs (include/rtpose_mi355x.h section 2b,
csrc/conv_backward.hip, train.py): float64 gradients taken from F.conv2d's own autograd on the CPU - never from the code
under test - with the quantity S a rounding-error bound is taken of, the bound itself, the ReLU gradient bit for bit, and
the cases the GPU tests run.  torch CPU + numpy only: no GPU, no library call."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(m):
    """gamma_m = m u / (1 - m u): the bound factor of an fp32 sum of products of m - 1 terms in any order, one rounding per
    product and per add (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    return m * U / (1.0 - m * U)


def _wgrad(x, gy, k):
    w = torch.zeros(gy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, padding=k // 2)
    return torch.autograd.grad(y, w, gy)[0]


def wgrad64(x, gy, k):
    """(dW, S): the float64 weight gradient [cout, cin, k, k] of conv2d(x, w, padding = k // 2) for the output gradient gy,
    and S = sum |gy| |x| over the same terms."""
    x, gy = x.double(), gy.double()
    return _wgrad(x, gy, k), _wgrad(x.abs(), gy.abs(), k)


def dbias64(gy):
    gy = gy.double()
    return gy.sum((0, 2, 3)), gy.abs().sum((0, 2, 3))


def _dgrad(gy, w):
    k = w.shape[2]
    x = torch.zeros(gy.shape[0], w.shape[1], gy.shape[2], gy.shape[3], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, padding=k // 2)
    return torch.autograd.grad(y, x, gy)[0]


def dgrad64(gy, w):
    """(dx, S): the float64 input gradient of conv2d(x, w, padding = k // 2) and S = sum |gy| |w| over the same terms."""
    gy, w = gy.double(), w.double()
    return _dgrad(gy, w), _dgrad(gy.abs(), w.abs())


def relu_grad_bits(y, gy_bits):
    """out = y > 0 ? gy : 0 on bit patterns: y float32 array (NaN compares false), gy_bits uint32 array."""
    return np.where(np.asarray(y, dtype=np.float32) > 0, gy_bits, np.uint32(0)).astype(np.uint32)


# ---- the cases of tests/test_conv_backward_gpu.py ----------------------------------------------------------------------------
# x_cs / x_off: cstride and choff of the input buffer; the output-gradient buffer is always wider than its slice
Case = namedtuple("Case", "k cin cout n h w x_cs x_off note")
CASES = [
    Case(1, 8, 19, 1, 5, 3, 16, 4, "smallest"),
    Case(3, 3, 64, 1, 16, 16, 8, 0, "cstride 8; conv1_1"),
    Case(3, 24, 38, 2, 9, 7, 40, 8, "slice at choff 8 of cstride 40; a slab spans the image boundary"),
    Case(7, 185, 128, 2, 10, 13, 192, 0, "cstride 192"),
    Case(1, 8, 512, 1, 4, 4, 16, 4, "several M tiles"),
    Case(1, 512, 8, 1, 4, 4, 520, 4, "several N tiles"),
    Case(3, 16, 32, 3, 46, 46, 24, 4, "several slabs, a partial last one"),
]


def case_id(c):
    return "k%d_%dto%d_%dx%dx%d" % (c.k, c.cin, c.cout, c.n, c.h, c.w)


def case_tensors(c, seed=0):
    """x = relu(randn) [n, cin, h, w] (non-negative: nothing cancels), gy = randn [n, cout, h, w], w = He-scaled filters"""
    g = torch.Generator().manual_seed(1000 + seed)
    x = F.relu(torch.randn(c.n, c.cin, c.h, c.w, generator=g))
    gy = torch.randn(c.n, c.cout, c.h, c.w, generator=g)
    wt = torch.randn(c.cout, c.cin, c.k, c.k, generator=g) * (2.0 / (c.cin * c.k * c.k)) ** 0.5
    return x, gy, wt
