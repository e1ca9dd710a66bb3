"""Host restatement of mixed-precision training (header section 2b, continued; csrc/conv_backward.hip;
train.conv2d(compute_dtype='bf16')): where a bf16 step rounds, stated in float64 on the CPU, the slab rule of the bf16 weight
gradient, and the cases the GPU tests run.  torch CPU + numpy only: no GPU, no library call.  The float64 gradients, the
bound factor gamma and the integer operands are those of tests/conv_backward_restate.py.

The reference project has no reduced-precision training, so what is restated here is this project's own contract:
  forward   y  = relu(conv2d(rb(x), rb(w)) + b)                rb = round to nearest even to bf16; b stays fp32
  backward  g  = rb(gy * mask)                                 the ONE rounding of the output gradient
            dx = dgrad(g, rb(w)),  dw = wgrad(rb(x), g),  db = sum g
with every product exact and every sum in fp32 on the device (float64 here).

Exact cases: integers bf16 holds (|v| <= 256) as operands, so rb changes nothing, every product and - while the sum of
absolute terms S stays below 2^24 - every partial sum is an integer fp32 holds: any summation order gives the float64 value."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from conv_backward_restate import gamma, wgrad64, dbias64, dgrad64, exact_tensors  # noqa: F401  (re-exported)
from conv_backward_restate import (FAKE, FAULT_H, FAULT_N, FAULT_W, WGRAD_FAULTS, set_field, set_layout,  # noqa: F401
                                   wgrad_null_empty_and_launch_limits, wgrad_passes_the_host_checks, wgrad_refused)

U = 2.0 ** -24


def rb(t):
    return t.to(torch.bfloat16).float()


# ---- the slab rule of csrc/conv_backward.hip (wgrad_geometry), restated ------------------------------------------------------
CHUNK = 64            # pixels per LDS chunk: 4 MFMA steps of K = 16
MIN_SLAB = 512
TARGET_BLOCKS = 1024


def geometry(cin, cout, k, n, h, w):
    """(slab pixels, slabs, workspace floats): conv_backward.hip's rule with a chunk of 64 pixels"""
    tm, tn = (2 if cout > 64 else 1), (2 if cin > 64 else 1)
    per_slab = -(-cout // (64 * tm)) * -(-cin // (64 * tn)) * k * k
    p = n * h * w
    want = max(1, min(-(-TARGET_BLOCKS // per_slab), -(-p // MIN_SLAB)))
    slab = -(-(-(-p // want)) // CHUNK) * CHUNK
    slabs = -(-p // slab)
    floats = slabs * (k * k * cout * cin + cout)
    return slab, slabs, -(-floats // 4) * 4


# ---- exact integer operands ---------------------------------------------------------------------------------------------------
# x_cs / x_off: cstride and choff of the bf16 input buffer, multiples of 8 elements; the output-gradient buffer is always wider
# than its slice, at choff 8.  gap: pixels of gap of the x buffer on top of k // 2.  wide: operands drawn from 0 .. 255 and
# +-1 .. 255 instead of conv_backward_restate.exact_tensors' 0 .. 3.  tags, tied to the library's geometry by
# tests/test_conv_backward_bf16_cpu.py: "several slabs" (slabs >= 2), "partial last chunk" (N H W % 64 != 0), "full"
# (N H W % 64 == 0); the rest says what the case is there for.
ExactCase = namedtuple("ExactCase", "k cin cout n h w x_cs x_off gap wide tags")
EXACT_CASES = [
    ExactCase(1, 1, 1, 1, 1, 1, 8, 0, 0, 0, "partial last chunk; one pixel, one channel: 7 pad channels of NaN in the group"),
    ExactCase(3, 1, 1, 1, 1, 1, 16, 8, 0, 0, "partial last chunk; only the centre tap sees data"),
    ExactCase(7, 1, 1, 1, 1, 1, 8, 0, 2, 0, "partial last chunk; the same with 49 taps; wide gap"),
    ExactCase(7, 3, 5, 2, 1, 9, 8, 0, 0, 0, "partial last chunk; H = 1: rows of taps read only the gap"),
    ExactCase(7, 5, 3, 2, 9, 1, 16, 8, 0, 0, "partial last chunk; W = 1"),
    ExactCase(1, 64, 64, 1, 4, 8, 64, 0, 0, 0, "partial last chunk; half a chunk, a full <1,1> tile"),
    ExactCase(1, 64, 64, 1, 8, 8, 64, 0, 0, 0, "full; exactly one chunk, a full <1,1> tile"),
    ExactCase(1, 63, 65, 1, 3, 11, 72, 0, 0, 0, "partial last chunk; <2,1>, a second M tile with one live channel"),
    ExactCase(1, 63, 65, 1, 5, 13, 72, 0, 0, 0, "partial last chunk; P = 65: one pixel in chunk 2"),
    ExactCase(1, 65, 63, 1, 3, 11, 72, 0, 0, 0, "partial last chunk; <1,2>"),
    ExactCase(1, 129, 130, 1, 5, 7, 136, 0, 0, 0, "partial last chunk; <2,2>, second M and N tiles with 2 and 1 live channels"),
    ExactCase(1, 257, 129, 1, 3, 3, 264, 0, 0, 0, "partial last chunk; three N tiles"),
    ExactCase(3, 65, 129, 2, 5, 7, 80, 8, 0, 0, "partial last chunk; <2,2>, 3x3, a chunk across the image boundary"),
    ExactCase(1, 8, 8, 1, 31, 33, 8, 0, 0, 0, "several slabs; partial last chunk; P = 1023"),
    ExactCase(1, 8, 8, 1, 32, 32, 8, 0, 0, 0, "several slabs; full; P = 1024: two whole slabs of 512"),
    ExactCase(1, 8, 8, 1, 25, 41, 16, 8, 0, 0, "several slabs; partial last chunk; P = 1025: a third slab, one pixel in its last chunk"),
    ExactCase(1, 8, 8, 3, 19, 18, 16, 0, 0, 0, "several slabs; partial last chunk; P = 1026, slabs across image boundaries"),
    ExactCase(1, 8, 8, 1, 1, 1537, 8, 0, 0, 0, "several slabs; partial last chunk; a single row"),
    ExactCase(3, 8, 8, 5, 15, 14, 16, 8, 2, 0, "several slabs; partial last chunk; five images; wide gap"),
    ExactCase(3, 72, 8, 2, 23, 23, 72, 0, 0, 0, "several slabs; partial last chunk; <1,2>"),
    ExactCase(7, 8, 72, 1, 23, 45, 16, 8, 0, 0, "several slabs; partial last chunk; <2,1>, 7x7"),
    ExactCase(1, 40, 24, 7, 13, 17, 48, 8, 0, 0, "several slabs; partial last chunk; seven images; ends at cstride"),
    ExactCase(3, 4, 4, 1, 6, 6, 8, 0, 0, 1, "partial last chunk; every integer bf16 holds below 256"),
]


def case_id(c):
    return "k%d_%dto%d_%dx%dx%d%s" % (c.k, c.cin, c.cout, c.n, c.h, c.w, "_wide" if getattr(c, "wide", 0) else "")


def exact_operands(c, seed=0):
    """(x, gy, wt, bias) of an exact case: conv_backward_restate.exact_tensors, or for a `wide` case x in {0 .. 255} with
    channel 0 in {1 .. 255} everywhere and gy in {+-1 .. +-255}, never zero (wt and bias as there).  Every value is an
    integer bf16 holds."""
    if not c.wide:
        return exact_tensors(c, seed)
    g = torch.Generator().manual_seed(3000 + seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    x = ri(0, 255, c.n, c.cin, c.h, c.w)
    x[:, 0] = ri(1, 255, c.n, c.h, c.w)
    gy = ri(1, 255, c.n, c.cout, c.h, c.w) * (2 * ri(0, 1, c.n, c.cout, c.h, c.w) - 1)
    return x, gy, ri(-2, 2, c.cout, c.cin, c.k, c.k), ri(-3, 3, c.cout)


def exact_margin(c, seed=0):
    """The largest sum of absolute terms S over dW, dbias, dx and the forward y of the case's operands: S < 2^24 is the
    condition under which fp32 accumulation in any order gives the exact integer."""
    x, gy, wt, bias = exact_operands(c, seed)
    s_y = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), padding=c.k // 2)
    return max(wgrad64(x, gy, c.k)[1].max().item(), dbias64(gy)[1].max().item(), dgrad64(gy, wt)[1].max().item(),
               s_y.max().item())


# ---- rounded operands ---------------------------------------------------------------------------------------------------------
# (k, cin, cout, n, h, w) as the issue of the kernel lists them, with the bf16 input buffer's cstride / choff
Case = namedtuple("Case", "k cin cout n h w x_cs x_off note")
CASES = [
    Case(1, 8, 19, 1, 5, 3, 16, 8, "smallest"),
    Case(3, 3, 64, 1, 16, 16, 8, 0, "cstride 8; conv1_1"),
    Case(3, 24, 38, 2, 9, 7, 40, 8, "slice at choff 8 of cstride 40; a chunk spans the image boundary"),
    Case(7, 185, 128, 2, 10, 13, 192, 0, "cstride 192"),
    Case(1, 8, 512, 1, 4, 4, 16, 8, "several M tiles"),
    Case(1, 512, 8, 1, 4, 4, 520, 8, "several N tiles"),
    Case(3, 16, 32, 3, 46, 46, 24, 8, "several slabs, a partial last one"),
]


def case_tensors(c, seed=0):
    """x = rb(relu(randn)) [n, cin, h, w] (non-negative: nothing cancels), gy = rb(randn) [n, cout, h, w]: rounded on the host,
    so the kernel's operands and the reference's are the same numbers"""
    g = torch.Generator().manual_seed(4000 + seed)
    x = rb(F.relu(torch.randn(c.n, c.cin, c.h, c.w, generator=g)))
    gy = rb(torch.randn(c.n, c.cout, c.h, c.w, generator=g))
    return x, gy


# ---- one conv of a bf16 step, its rounding points in float64 ----------------------------------------------------------------------
class EmulConv(torch.autograd.Function):
    """y = relu(conv2d(r(x), r(w)) + b) with the gradients of the module docstring, in float64; r = rb, or the identity with
    rounding = False (then this is torch's own float64 autograd of conv2d + relu).  mask: the ReLU decisions to use in the
    backward instead of y > 0 (a bool tensor shaped like y), for a comparison that must not hinge on the sign of a y that
    rounds to either side of zero."""
    @staticmethod
    def forward(ctx, x, w, b, relu, rounding=True, mask=None):
        r = (lambda t: rb(t).double()) if rounding else (lambda t: t.double())
        xr, wr = r(x), r(w)
        k = w.shape[2]
        y = F.conv2d(xr, wr, None if b is None else b.double(), padding=k // 2)
        if relu:
            y = F.relu(y)
        ctx.save_for_backward(xr, wr, (y > 0) if mask is None else mask)
        ctx.relu, ctx.r, ctx.k, ctx.has_bias = bool(relu), r, k, b is not None
        ctx.dtypes = (x.dtype, w.dtype, None if b is None else b.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        xr, wr, mask = ctx.saved_tensors
        g = gy.double()
        if ctx.relu:
            g = g * mask.double()
        g = ctx.r(g)
        with torch.enable_grad():        # dgrad64 / wgrad64 take their gradients from F.conv2d's own autograd
            dx = dgrad64(g, wr)[0] if ctx.needs_input_grad[0] else None
            dw = wgrad64(xr, g, ctx.k)[0] if ctx.needs_input_grad[1] else None
        db = dbias64(g)[0] if ctx.has_bias and ctx.needs_input_grad[2] else None
        dtx, dtw, dtb = ctx.dtypes
        return (None if dx is None else dx.to(dtx), None if dw is None else dw.to(dtw), None if db is None else db.to(dtb),
                None, None, None)


def emul_conv(x, w, b=None, relu=False, rounding=True, mask=None):
    return EmulConv.apply(x, w, b, relu, rounding, mask)
