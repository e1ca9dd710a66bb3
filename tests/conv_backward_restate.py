"""Host restatement of the backward pass of the stride-1 "same" convs (include/rtpose_mi355x.h section 2b,
csrc/conv_backward.hip, train.py): float64 gradients taken from F.conv2d's own autograd on the CPU - never from the code
under test - with the quantity S a rounding-error bound is taken of, the bound itself, the ReLU gradient bit for bit, and
the cases the GPU tests run.  torch CPU + numpy only: no GPU, no library call.

The exact cases (EXACT_CASES, exact_tensors): operands that are small integers held in float32.  Every kernel of the backward
pass is fp32 in, fp32 accumulate, so while every sum of absolute terms S stays below 2^24 each product and each partial sum is
an integer fp32 holds exactly - whatever the summation order, slab split or fma chain - and the float64 reference is compared
with ==.  exact_margin(c) is that S; the largest over EXACT_CASES is 8 783 (k7_8to72_1x23x45), of 16 777 216."""
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


# ---- exact integer operands ---------------------------------------------------------------------------------------------------
# x_cs / x_off as above; gap: pixels of gap of the x buffer on top of k // 2.  tags, checked against the library's host-side
# geometry by tests/test_conv_backward_cpu.py: "several slabs" (slabs >= 2), "partial last chunk" (N H W % 32 != 0), "full"
# (N H W % 32 == 0); the rest of the string says what the case is there for.
ExactCase = namedtuple("ExactCase", "k cin cout n h w x_cs x_off gap tags")
EXACT_CASES = [
    ExactCase(1, 1, 1, 1, 1, 1, 1, 0, 0, "partial last chunk; one pixel, one channel"),
    ExactCase(3, 1, 1, 1, 1, 1, 3, 2, 0, "partial last chunk; only the centre tap sees data; slice ends at cstride"),
    ExactCase(7, 1, 1, 1, 1, 1, 4, 0, 2, "partial last chunk; the same with 49 taps; wide gap"),
    ExactCase(3, 2, 2, 1, 2, 2, 5, 3, 0, "partial last chunk; map smaller than a chunk; odd choff, odd cstride, ends at cstride"),
    ExactCase(7, 3, 5, 2, 1, 9, 8, 4, 2, "partial last chunk; H = 1: rows of taps read only the gap; wide gap"),
    ExactCase(7, 5, 3, 2, 9, 1, 11, 3, 0, "partial last chunk; W = 1; odd choff, odd cstride"),
    ExactCase(1, 64, 64, 1, 4, 8, 64, 0, 0, "full; exactly one chunk, a full <1,1> tile"),
    ExactCase(1, 63, 65, 1, 3, 11, 67, 4, 2, "partial last chunk; <2,1>, one pixel in chunk 2; ends at cstride; wide gap"),
    ExactCase(1, 65, 63, 1, 3, 11, 72, 3, 0, "partial last chunk; <1,2>; odd choff"),
    ExactCase(1, 129, 130, 1, 5, 7, 136, 4, 0, "partial last chunk; <2,2>, second M and N tiles with 2 and 1 live channels"),
    ExactCase(1, 257, 129, 1, 3, 3, 257, 0, 0, "partial last chunk; three N tiles"),
    ExactCase(3, 65, 129, 2, 5, 7, 77, 11, 2, "partial last chunk; <2,2>, 3x3, a chunk across the image boundary; odd choff, "
                                              "odd cstride; wide gap"),
    ExactCase(1, 8, 8, 1, 31, 33, 11, 3, 0, "several slabs; partial last chunk; P = 1023; odd choff, odd cstride"),
    ExactCase(1, 8, 8, 1, 32, 32, 8, 0, 0, "several slabs; full; P = 1024"),
    ExactCase(1, 8, 8, 1, 25, 41, 16, 8, 0, "several slabs; partial last chunk; P = 1025, one pixel in the last chunk"),
    ExactCase(1, 8, 8, 3, 19, 18, 12, 4, 0, "several slabs; partial last chunk; P = 1026, slabs across image boundaries; ends at "
                                            "cstride"),
    ExactCase(1, 8, 8, 1, 1, 1537, 9, 1, 0, "several slabs; partial last chunk; a single row; odd choff, odd cstride, ends at "
                                            "cstride"),
    ExactCase(3, 8, 8, 5, 15, 14, 16, 4, 2, "several slabs; partial last chunk; five images; wide gap"),
    ExactCase(3, 72, 8, 2, 23, 23, 72, 0, 0, "several slabs; partial last chunk; <1,2>"),
    ExactCase(7, 8, 72, 1, 23, 45, 13, 5, 0, "several slabs; partial last chunk; <2,1>, 7x7; odd choff, odd cstride, ends at "
                                             "cstride"),
    ExactCase(1, 40, 24, 7, 13, 17, 48, 8, 0, "several slabs; partial last chunk; seven images; ends at cstride"),
]


def exact_tensors(c, seed=0):
    """(x, gy, wt, bias) of a case (any tuple with k cin cout n h w), float32 holding integers: x in {0, 1, 2, 3} with zeros as
    a ReLU leaves them but channel 0 in {1, 2, 3} everywhere, gy in {+-1, +-2, +-3} and never zero, wt in {-2 .. 2}, bias in
    {-3 .. 3}.  With gy never zero and channel 0 of x positive, a single missing (pixel, tap) term changes dbias[o] and
    dW[o, 0, tap]."""
    g = torch.Generator().manual_seed(2000 + seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    x = ri(0, 3, c.n, c.cin, c.h, c.w)
    x[:, 0] = ri(1, 3, c.n, c.h, c.w)
    gy = ri(1, 3, c.n, c.cout, c.h, c.w) * (2 * ri(0, 1, c.n, c.cout, c.h, c.w) - 1)
    wt = ri(-2, 2, c.cout, c.cin, c.k, c.k)
    bias = ri(-3, 3, c.cout)
    return x, gy, wt, bias


def exact_margin(c, seed=0):
    """The largest sum of absolute terms S over dW, dbias, dx and the forward y of the case's exact tensors.  S < 2^24 is the
    condition under which fp32 arithmetic in any order gives the exact integer."""
    x, gy, wt, bias = exact_tensors(c, seed)
    s_y = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), padding=c.k // 2)
    return max(wgrad64(x, gy, c.k)[1].max().item(), dbias64(gy)[1].max().item(), dgrad64(gy, wt)[1].max().item(),
               s_y.max().item())


# ---- the host refusals rtpose_conv2d_wgrad and rtpose_conv2d_wgrad_bf16 share (csrc/conv_backward.hip: one host path) ----------
# Each test file brings its own base(capi, k, cin, cout) descriptor - fake pointers, lx = padded(40, H, W, k // 2, 8), lgy =
# padded(48, H, W, 0, choff) - and runs every row on its entry point.  (name, fault(d), text the message holds)
def set_field(field, value):
    def f(d):
        setattr(d, field, value)
    return f


def set_layout(which, field, value):
    def f(d):
        setattr(getattr(d, which), field, value)
    return f


def _small_ws(d):
    d.workspace_floats -= 1


def _gy_past_cstride(d):
    d.cout = d.lgy.cstride - d.lgy.choff + 1        # (45 on the fp32 base, 41 on the bf16 one)


FAULT_N, FAULT_H, FAULT_W = 2, 9, 7
FAKE = 1 << 20          # a 16-byte aligned "device pointer" no refused launch touches

WGRAD_FAULTS = [
    ("null x", set_field("x", None), "NULL x"),
    ("null gy", set_field("gy", None), "NULL gy"),
    ("null dw", set_field("dw", None), "NULL dw"),
    ("null workspace", set_field("workspace", None), "NULL workspace"),
    ("k = 5", set_field("k", 5), "k must be 1, 3 or 7"),
    ("k = 0", set_field("k", 0), "k must be 1, 3 or 7"),
    ("cin = 0", set_field("cin", 0), "cin and cout must be >= 1"),
    ("cout = 0", set_field("cout", 0), "cin and cout must be >= 1"),
    ("x slice past cstride", set_field("cin", 33), "input slice exceeds cstride"),
    ("gy slice past cstride", _gy_past_cstride, "output-gradient slice exceeds cstride"),
    ("row gap below k/2", set_layout("lx", "ws", FAULT_W), "gap smaller than the conv padding"),
    ("image gap below k/2", set_layout("lx", "hs", FAULT_H), "gap smaller than the conv padding"),
    ("lead below k/2", set_layout("lx", "lead", FAULT_W + 1), "gap smaller than the conv padding"),
    ("gy rows shorter than the map", set_layout("lgy", "ws", FAULT_W - 1), "output-gradient layout smaller than the map"),
    ("bad layout", set_layout("lgy", "cstride", 0), "bad layout"),
    ("workspace too small", _small_ws, "workspace of"),
    ("dw not 16-byte aligned", set_field("dw", FAKE + 4), "16-byte aligned"),
    ("workspace not 16-byte aligned", set_field("workspace", FAKE + 8), "16-byte aligned"),
]


def wgrad_refused(capi, entry, who, d, shape, text):
    """`entry` returns RTPOSE_E_INVAL with `text` in a message that names the entry point, before any pointer is looked at"""
    import ctypes as C
    rc = entry(C.byref(d) if d is not None else None, *shape, None)
    err = capi.last_error()
    assert rc == -1, (rc, err)                                # RTPOSE_E_INVAL, not a HIP error
    assert text in err and err.startswith(who + ":"), err
    assert "device memory" not in err                         # returned before the pointers were looked at


def wgrad_null_empty_and_launch_limits(capi, entry, slabs, who, base):
    """the NULL descriptor, each of the three empty shapes and the two shapes above the launch limit"""
    n, h, w = FAULT_N, FAULT_H, FAULT_W
    wgrad_refused(capi, entry, who, None, (n, h, w), "NULL descriptor")
    d = base(capi)
    for shape in ((0, h, w), (n, 0, w), (n, h, 0)):
        wgrad_refused(capi, entry, who, d, shape, "empty tensor")
    # a tensor whose pixels do not fit the kernels' int index: N * H * W >= 2^31 - 256
    d = base(capi, k=1, cin=8, cout=8)
    big = 1 << 16
    d.lx = capi.Layout.padded(40, big, big, 0, 8)
    d.lgy = capi.Layout.padded(48, big, big, 0, 8)
    wgrad_refused(capi, entry, who, d, (1, big, big), "above the launch limit")
    # a grid beyond the launch limits: the slab count is at most 1024 by the slab rule and taps at most 49, so the grid can only
    # outgrow its limits along x, M tiles * N tiles - which needs taps * cout * cin >= 2^31 - 256, refused under the same text
    c = 46344                                   # c * c > 2^31, a multiple of 8
    assert slabs(8, 8, 1, 1, 1 << 15, 1 << 15) <= 1024
    d = base(capi, k=1, cin=c, cout=c)
    d.lx = capi.Layout.padded(c, h, w, 0, 0)
    d.lgy = capi.Layout.padded(c, h, w, 0, 0)
    d.workspace_floats = 1 << 62
    wgrad_refused(capi, entry, who, d, (n, h, w), "above the launch limit")
    assert slabs(c, c, 1, n, h, w) == 0


def wgrad_passes_the_host_checks(capi, entry, base):
    """k = 7 with a gap of exactly 3, with and without dbias, passes every host check: the refusal is then the pointer's
    (fake: no device owns it)"""
    import ctypes as C
    for dbias in (FAKE, None):
        d = base(capi, k=7)
        d.dbias = dbias
        rc = entry(C.byref(d), FAULT_N, FAULT_H, FAULT_W, None)
        assert rc != 0 and "gap" not in capi.last_error() and "x" in capi.last_error()
