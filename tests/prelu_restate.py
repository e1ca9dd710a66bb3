"""Host restatement of the PReLU passes of training (include/rtpose_mi355x.h section 2b continued, csrc/prelu_backward.hip,
train.conv2d(prelu=)): the float64 truth taken from torch's own F.prelu autograd on the CPU - never from the code under
test -, the fp32 results bit for bit (a select, or one numpy-float32 multiply), the quantity S a rounding-error bound of the
slope gradient is taken of, and the cases and operands the GPU tests run.  torch CPU + numpy only: no GPU, no library call.

Forward and backward treat z == 0 differently on purpose.  The forward is the library's fused epilogue (prelu1 in
csrc/common.h): y = z >= 0 ? z : slope * z, which differs from F.prelu only in the sign of a zero under a negative slope.
The backward is torch's prelu_backward: z > 0 ? gy : slope * gy, and z > 0 ? 0 : z * gy summed per channel; z == 0 and a
NaN z take the slope path.

The exact operand sets: float32 holding integers (z, gy) and quarters (slopes).  Every product and every partial sum is then
a multiple of 1/4 that fp32 holds exactly while the sum of absolute terms S stays below 2^24 (2^22 would do for the quarters
of y and out, which are single products): whatever the order of the sum, the float64 reference is compared with ==."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_backward_restate as cb
import layout_restate as lr

SLOPES = (-2.0, -0.5, 0.0, 0.25, 1.0, 2.0)
SLAB_UNIT = 64          # header: slabs are equal multiples of 64 pixels but for the last one


# ---- truth and bits ---------------------------------------------------------------------------------------------------------------
def prelu64(z, gy, slope):
    """(y, dz, dslope, S) in float64 from F.prelu's CPU autograd: z, gy [n, c, h, w], slope [c].  S[c] = sum |z| |gy| over
    the terms of dslope[c] (those with z <= 0 or NaN)."""
    z64 = z.double().detach().requires_grad_(True)
    a64 = slope.double().detach().requires_grad_(True)
    y = F.prelu(z64, a64)
    dz, da = torch.autograd.grad(y, (z64, a64), gy.double())
    terms = torch.where(z.double() > 0, torch.zeros((), dtype=torch.float64), z.double().abs() * gy.double().abs())
    return y.detach(), dz, da, terms.sum((0, 2, 3))


def _s(slope):
    return np.asarray(slope, dtype=np.float32).reshape(1, -1, 1, 1)


def prelu_bits(z, slope):
    """y = z >= 0 ? z : slope * z (prelu1) on float32 arrays [n, c, h, w] / [c], as uint32: the sign of a zero is z's, a NaN z
    goes through the multiply."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(z >= 0, z, _s(slope) * z).astype(np.float32).view(np.uint32)


def prelu_grad_bits(z, gy_bits, slope):
    """out = z > 0 ? gy : slope * gy on bit patterns: where z > 0 gy's bits (a NaN's payload included), else the bits of
    one float32 multiply."""
    z = np.asarray(z, dtype=np.float32)
    gy_bits = np.asarray(gy_bits, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        prod = (_s(slope) * gy_bits.view(np.float32)).astype(np.float32).view(np.uint32)
        return np.where(z > 0, gy_bits, prod).astype(np.uint32)


# ---- the cases of tests/test_prelu_backward_gpu.py ----------------------------------------------------------------------------------
# z / gy / out: (cstride, choff) of each buffer; their gaps differ as well (layouts()).  tags, held to the library's own
# query by tests/test_prelu_backward_cpu.py: "several slabs" (slabs >= 2), "partial last slab" (N H W % 64 != 0); "vector" /
# "scalar": whether every cstride and choff is a multiple of 4 floats (the 16-byte path) - the rest says what the case is for.
Case = namedtuple("Case", "channels n h w z gy out tags")
CASES = [
    Case(1, 1, 1, 1, (1, 0), (1, 0), (1, 0), "scalar; partial last slab; one element"),
    Case(3, 1, 2, 2, (5, 2), (8, 4), (4, 1), "scalar; partial last slab; three layouts, the slices end at cstride"),
    Case(19, 2, 5, 3, (24, 4), (24, 4), (24, 4), "vector; partial last slab; a last unit of 3 channels"),
    Case(52, 1, 4, 4, (56, 0), (56, 0), (60, 8), "vector; partial last slab; 13 units"),
    Case(96, 2, 9, 7, (96, 0), (96, 0), (96, 0), "vector; several slabs; partial last slab; dense"),
    Case(130, 1, 3, 11, (136, 4), (137, 5), (136, 4), "scalar; partial last slab; three channel tiles of 64 units"),
    Case(130, 1, 3, 11, (136, 4), (136, 4), (136, 4), "vector; partial last slab; 33 units: 7 rows, 25 idle threads, last unit of 2"),
    Case(8, 1, 1, 1537, (9, 1), (12, 4), (9, 1), "scalar; several slabs; partial last slab; one pixel in the last slab"),
    Case(8, 3, 19, 18, (12, 4), (12, 4), (16, 8), "vector; several slabs; partial last slab; slabs across image boundaries"),
    Case(512, 1, 4, 4, (520, 4), (520, 4), (520, 4), "vector; partial last slab; two channel tiles"),
    Case(128, 2, 46, 46, (128, 0), (128, 0), (128, 0), "vector; several slabs; partial last slab; the largest"),
    Case(8, 1, 1, 63, (8, 0), (8, 0), (8, 0), "vector; partial last slab; P = slab - 1"),
    Case(8, 1, 1, 64, (8, 0), (8, 0), (8, 0), "vector; P = slab"),
    Case(8, 1, 1, 65, (8, 0), (11, 3), (8, 0), "scalar; several slabs; partial last slab; P = slab + 1"),
    Case(8, 2, 8, 8, (8, 0), (8, 0), (8, 0), "vector; several slabs; P = 2 slabs, full"),
]


def case_id(c):
    return "c%d_%dx%dx%d_z%d.%d_g%d.%d_o%d.%d" % ((c.channels, c.n, c.h, c.w) + c.z + c.gy + c.out)


def layouts(c):
    """(lz, lgy, lout): the three buffers have gaps of 1, 2 and 0 pixels"""
    return (lr.padded(c.z[0], c.h, c.w, 1, c.z[1]), lr.padded(c.gy[0], c.h, c.w, 2, c.gy[1]),
            lr.padded(c.out[0], c.h, c.w, 0, c.out[1]))


def is_vector(c):
    return all(v % 4 == 0 for pair in (c.z, c.gy, c.out) for v in pair)


def slopes(channels):
    return torch.tensor([SLOPES[i % len(SLOPES)] for i in range(channels)], dtype=torch.float32)


def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def exact_mixed(c, seed=0):
    """(z, gy, slope): z in {-3 .. 3} with zeros, gy in +-{1, 2, 3} and never 0, slopes cycling through SLOPES"""
    g = torch.Generator().manual_seed(3000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    z = _ri(g, -3, 3, *shape)
    gy = _ri(g, 1, 3, *shape) * (2 * _ri(g, 0, 1, *shape) - 1)
    return z, gy, slopes(c.channels)


def exact_negative(c, seed=0):
    """(z, gy, slope): z in {-3, -2, -1}, gy in {1, 2, 3}: every term of dslope is strictly negative, so one missing or
    doubled pixel changes the sum of every channel"""
    g = torch.Generator().manual_seed(4000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    return _ri(g, -3, -1, *shape), _ri(g, 1, 3, *shape), slopes(c.channels)


EXACT_SETS = {"mixed": exact_mixed, "negative": exact_negative}


def exact_margin(z, gy):
    """S = max over channels of sum |z| |gy|: below 2^24 fp32 sums of the terms z * gy are exact in any order"""
    return (z.double().abs() * gy.double().abs()).sum((0, 2, 3)).max().item()


def random_operands(c, seed=0):
    """(z, gy_bits, slope): randn z with exact zeros of both signs, randn gy with NaN payloads and -0 on pixels where z > 0,
    slopes randn * 0.25 with both signs present where there are two channels"""
    g = torch.Generator().manual_seed(5000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    z = torch.randn(*shape, generator=g)
    gy = torch.randn(*shape, generator=g)
    slope = torch.randn(c.channels, generator=g) * 0.25
    if c.channels >= 2:
        slope[0], slope[1] = -slope[0].abs() - 0.01, slope[1].abs() + 0.01
    zf = z.view(-1)
    if zf.numel() >= 8:
        zf[1::7] = 0.0
        zf[2::11] = -0.0
    gy_bits = gy.numpy().view(np.uint32).copy()
    pos = (z.numpy() > 0).reshape(-1)
    where = np.flatnonzero(pos)
    flat = gy_bits.reshape(-1)
    flat[where[::5]] = 0x7FC00777         # a NaN gradient where z > 0 travels as its bits
    flat[where[1::5]] = 0x80000000        # so does -0
    return z, gy_bits, slope


# ---- train.conv2d(prelu=) on exact operands: the specs of tests/test_train_openpose_gpu.py -----------------------------------------
Spec = namedtuple("Spec", "k cin cout n h w req variant")
SUBSETS = ("x", "w", "b", "a", "xw", "xb", "xa", "wb", "wa", "ba", "xwb", "xwa", "xba", "wba", "xwba")
VARIANTS = ("shared_slope", "backward_twice", "side_stream")


def _specs():
    grid = [(k, ci, co, shape) for k in (1, 3, 7) for ci, co in ((3, 5), (9, 8)) for shape in ((1, 1, 1), (2, 5, 3), (3, 19, 18))
            if not (k == 7 and shape == (3, 19, 18))]
    out = [Spec(k, ci, co, *shape, SUBSETS[i % len(SUBSETS)] if i < len(SUBSETS) else "xwba", None)
           for i, (k, ci, co, shape) in enumerate(grid)]
    out.append(Spec(3, 9, 8, 2, 5, 3, "xwba", "shared_slope"))
    out.append(Spec(1, 3, 5, 3, 19, 18, "xwba", "backward_twice"))
    out.append(Spec(7, 9, 8, 2, 5, 3, "xwba", "side_stream"))
    return out


SPECS = _specs()
assert {s.req for s in SPECS} == set(SUBSETS) and {s.variant for s in SPECS} == set(VARIANTS) | {None}
assert len(SPECS) == 19


def spec_id(s):
    return "k%d_%dto%d_%dx%dx%d_%s%s" % (s.k, s.cin, s.cout, s.n, s.h, s.w, s.req, "_" + s.variant if s.variant else "")


def spec_tensors(s):
    """(x, G, wt, bias, slope): conv_backward_restate.exact_tensors of the spec, and dyadic slopes from SLOPES"""
    x, G, wt, b = cb.exact_tensors(s, seed=s.k + s.cin + 1)
    return x, G, wt, b, slopes(s.cout)


def spec_margin(s):
    """The largest sum of absolute terms over y, dx, dw, db and dslope of prelu(conv2d(x, w, b)) with output gradient G, the
    slopes' magnitudes included (m = max(1, |slope|) per channel bounds both branches of the PReLU), from torch on the CPU.
    All of these are sums of multiples of 1/4: they are exact in fp32, in any order, while 4 * S < 2^24."""
    x, G, wt, b, a = (t.double() for t in spec_tensors(s))
    m = a.abs().clamp_min(1.0).view(1, -1, 1, 1)
    s_z = F.conv2d(x.abs(), wt.abs(), b.abs(), padding=s.k // 2)
    s_gz = m * G.abs()
    return max((m * s_z).max().item(), cb.dgrad64(s_gz, wt)[1].max().item(), cb.wgrad64(x, s_gz, s.k)[1].max().item(),
               cb.dbias64(s_gz)[1].max().item(), (s_z * G.abs()).sum((0, 2, 3)).max().item())


# ---- the host refusals the four PReLU entry points share (csrc/prelu_backward.hip) ----------------------------------------------
# rtpose_prelu, rtpose_prelu_grad, rtpose_prelu_bf16 and rtpose_prelu_grad_bf16 take the same kinds of argument at different
# positions.  A test file describes its entry point's argument list - each slice as (name, index of the buffer, index of the
# layout, index of the layout in `lays`, buffer may be NULL), the index of the slopes, of `channels` (N, H, W and the stream
# follow it) and, for a gradient, of the workspace (workspace_floats follows it) - and shared_faults gives the rows that entry
# point has: (name, fault(a, lays), text the message holds).
FAULT_N, FAULT_H, FAULT_W, FAULT_CH = 2, 9, 7, 19


def arg_fault(i, v):
    def f(a, lays):
        a[i] = v
    return f


def layout_fault(j, field, v):
    def f(a, lays):
        setattr(lays[j], field, v)
    return f


def _past_cstride(j):
    def f(a, lays):
        lays[j].choff = lays[j].cstride - FAULT_CH + 1
    return f


def above_launch_limit(a, lays):
    """a map above the launch limit, in layouts that hold it"""
    for lay in lays:
        lay.ws, lay.hs, lay.lead = 1 << 15, 1 << 16, 0
    a[-4:-1] = [1, 1 << 16, 1 << 15]


def shared_faults(slices, slope, channels, workspace=None):
    rows = []
    for name, ib, il, j, optional in slices:
        if not optional:
            rows.append(("null " + name, arg_fault(ib, None), "NULL buffer (%s)" % name))
        rows += [("null l" + name, arg_fault(il, None), "NULL layout (%s)" % name),
                 (name + " bad layout", layout_fault(j, "cstride", 0), "bad layout (%s)" % name),
                 (name + " slice past cstride", _past_cstride(j), "%s slice exceeds cstride" % name),
                 (name + " rows shorter than the map", layout_fault(j, "ws", FAULT_W - 1), "layout smaller than the map (%s)" % name)]
    rows += [("null slope", arg_fault(slope, None), "NULL buffer (slope)"),
             ("no channels", arg_fault(channels, 0), "empty tensor"),
             ("no images", arg_fault(channels + 1, 0), "empty tensor"),
             ("above the launch limit", above_launch_limit, "above the launch limit")]
    if workspace is not None:
        rows += [("dslope without a workspace", arg_fault(workspace, None), "NULL workspace"),
                 ("workspace too small", arg_fault(workspace + 1, 2 * FAULT_CH - 1), "workspace of")]
    return rows


def refused(capi, fn, who, a, text):
    rc = fn(*a)
    err = capi.last_error()
    assert rc == -1, (rc, err)                                   # RTPOSE_E_INVAL, not a HIP error
    assert text in err and err.startswith(who + ":"), err
    assert "device memory" not in err                            # returned before the pointers were looked at
