"""Host restatement of the activation layout (include/rtpose_mi355x.h §1), of the bf16 / split element
formats and of the arithmetic of the kernels in csrc/layout_ops.hip, shufflenet_ops.hip and image_ops.hip.  numpy
(+ torch CPU float64), no GPU, no library call: tests/test_layout_ops_gpu.py compares every entry point of those files with this, and
tests/test_layout_restate_cpu.py checks this file against torch on the CPU.

Tensors are NCHW unless a name says NHWC.  The arithmetic references return (value, S): the float64 result
and the float64 sum of the absolute values of the terms that were added - the quantity a rounding-error
bound of the form n * 2^-24 * S is taken of.  The max-pools return the value only (a maximum has no rounding).
"""
from collections import namedtuple

import numpy as np
import torch

from oracle.host_oracle import SWAP_HEAT, SWAP_PAF

Lay = namedtuple("Lay", "cstride choff ws hs lead")


def dense(c, h, w, choff=0):
    return Lay(c, choff, w, h, 0)


def padded(c, h, w, pad, choff=0):
    ws = w + pad
    return Lay(c, choff, ws, h + pad, pad * ws + pad)


def pixels(l, n):
    """rtpose_layout_pixels restated: lead + n images + the tail slack the conv tiles may read."""
    return l.lead + n * l.hs * l.ws + 40 * l.ws + 4352


def offsets(l, n, h, w):
    """Element offset of channel 0 of the slice for every pixel: int64 [n, h, w]."""
    nn = np.arange(n, dtype=np.int64)[:, None, None]
    yy = np.arange(h, dtype=np.int64)[None, :, None]
    xx = np.arange(w, dtype=np.int64)[None, None, :]
    return (l.lead + (nn * l.hs + yy) * l.ws + xx) * l.cstride + l.choff


def index(l, n, h, w, c):
    """Element offsets of channels [0, c) of the slice: int64 [n, h, w, c]."""
    return offsets(l, n, h, w)[..., None] + np.arange(c, dtype=np.int64)


def index_map(l, n, h, w, cmap):
    """Offsets of ABSOLUTE channels cmap[i] of the pixel (choff not applied): the *_cmap copies."""
    return (offsets(l, n, h, w) - l.choff)[..., None] + np.asarray(cmap, dtype=np.int64)


def scatter(buf, l, x):
    """buf (1-D, fp32 or uint16 bf16 bits) <- x [n, c, h, w] at the slice of layout l."""
    n, c, h, w = x.shape
    buf[index(l, n, h, w, c)] = np.transpose(x, (0, 2, 3, 1))
    return buf


def gather(buf, l, n, h, w, c):
    return np.ascontiguousarray(np.transpose(buf[index(l, n, h, w, c)], (0, 3, 1, 2)))


def split_index(l, n, h, w, c):
    """Split buffers: per 8 channels [hi x 8 | lo x 8], 2 elements per channel; l counts elements.  choff may
    sit inside an 8-channel group (choff / 2 = first channel, addressed absolutely).  Returns (hi, lo)
    offsets, int64 [n, h, w, c]."""
    base = offsets(l, n, h, w)[..., None] - l.choff
    ca = l.choff // 2 + np.arange(c, dtype=np.int64)
    hi = base + (ca >> 3) * 16 + (ca & 7)
    return hi, hi + 8


def scatter_split(buf, l, hi, lo):
    n, c, h, w = hi.shape
    ih, il = split_index(l, n, h, w, c)
    buf[ih] = np.transpose(hi, (0, 2, 3, 1))
    buf[il] = np.transpose(lo, (0, 2, 3, 1))
    return buf


def gather_split(buf, l, n, h, w, c):
    ih, il = split_index(l, n, h, w, c)
    t = lambda a: np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))
    return t(buf[ih]), t(buf[il])


def untouched(bits, written, sentinel):
    """True iff every word of `bits` (an unsigned integer view of a buffer) whose offset is not in `written`
    (any int64 array of offsets, or a list of them) still holds `sentinel`, bit for bit."""
    mask = np.ones(bits.shape[0], dtype=bool)
    for w in (written if isinstance(written, (list, tuple)) else [written]):
        mask[np.asarray(w, dtype=np.int64).ravel()] = False
    return bool(np.all(bits[mask] == bits.dtype.type(sentinel)))


# ---- element formats -----------------------------------------------------------------------------------
def bf16_rne(f):
    """float32 -> bfloat16 bits (uint16), round to nearest even, in integer arithmetic.  NaN excluded."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(h):
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split(f):
    """hi = bf16(f), lo = bf16(f - hi) with the difference taken in fp32 (it is exact for |f| < 1e30)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    hi = bf16_rne(f)
    lo = bf16_rne(f - bf16_to_f32(hi))
    return hi, lo


def bf16_key(h):
    """Order-preserving integer key of bf16 bit patterns (-0 < +0; NaN excluded)."""
    h = np.asarray(h, dtype=np.uint16).astype(np.int32)
    return np.where(h & 0x8000, -(h & 0x7FFF) - 1, h)


def f32_round_interval(v, e):
    """float32(v - e), float32(v + e) of float64 arrays."""
    return (v - e).astype(np.float32), (v + e).astype(np.float32)


# ---- arithmetic references (float64) -------------------------------------------------------------------
def _t64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def maxpool2x2(x):
    """MaxPool2d(2, 2, 0): floor semantics, the odd last row / column is dropped."""
    x = _t64(x)
    ho, wo = x.shape[2] // 2, x.shape[3] // 2
    v = x[:, :, :2 * ho, :2 * wo]
    return torch.maximum(torch.maximum(v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2]),
                         torch.maximum(v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2]))


def maxpool3x3s2_ceil(x):
    """MaxPool2d(3, 2, 0, ceil_mode=True): windows that hang over the edge are clipped to the input."""
    x = _t64(x)
    n, c, h, w = x.shape
    ho, wo = (h - 3 + 1) // 2 + 1, (w - 3 + 1) // 2 + 1
    xp = torch.full((n, c, 2 * ho + 1, 2 * wo + 1), -float("inf"), dtype=torch.float64)
    xp[:, :, :h, :w] = x
    r = torch.full((n, c, ho, wo), -float("inf"), dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            r = torch.maximum(r, xp[:, :, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2])
    return r


def dwconv3x3(x, w, b, stride):
    """depthwise 3x3, pad 1: x [n,c,h,w], w [c,3,3], b [c]."""
    x, w, b = _t64(x), _t64(w), _t64(b)
    n, c, h, wd = x.shape
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    xp = torch.zeros(n, c, h + 2, wd + 2, dtype=torch.float64)
    xp[:, :, 1:h + 1, 1:wd + 1] = x
    v = b.view(1, c, 1, 1).expand(n, c, ho, wo).clone()
    s = v.abs()
    for ky in range(3):
        for kx in range(3):
            t = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] * w[:, ky, kx].view(1, c, 1, 1)
            v = v + t
            s = s + t.abs()
    return v, s


def affine(x, scale, shift):
    x = _t64(x)
    c = x.shape[1]
    a, t = x * _t64(scale).view(1, c, 1, 1), _t64(shift).view(1, c, 1, 1)
    return a + t, a.abs() + t.abs()


def stem_conv3x3_s2(x, scale, shift, w, b, relu=True):
    """affine (scale / shift or None) -> zero padding -> conv 3x3 stride 2 pad 1 (+bias) -> ReLU.
    x [n,ci,h,w], w [co,ci,3,3]."""
    x, w, b = _t64(x), _t64(w), _t64(b)
    n, ci, h, wd = x.shape
    co = w.shape[0]
    if scale is None:
        xa, xs = x, x.abs()
    else:
        xa, xs = affine(x, scale, shift)
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    xp = torch.zeros(n, ci, h + 2, wd + 2, dtype=torch.float64)
    sp = torch.zeros_like(xp)
    xp[:, :, 1:h + 1, 1:wd + 1] = xa
    sp[:, :, 1:h + 1, 1:wd + 1] = xs
    v = b.view(1, co, 1, 1).expand(n, co, ho, wo).clone()
    s = v.abs()
    for ky in range(3):
        for kx in range(3):
            sl = (slice(None), slice(None), slice(ky, ky + 2 * (ho - 1) + 1, 2), slice(kx, kx + 2 * (wo - 1) + 1, 2))
            v = v + torch.einsum("nchw,oc->nohw", xp[sl], w[:, :, ky, kx])
            s = s + torch.einsum("nchw,oc->nohw", sp[sl], w[:, :, ky, kx].abs())
    return (torch.relu(v) if relu else v), s


def axpby(dst, src, alpha, beta):
    a, b = float(alpha) * _t64(dst), float(beta) * _t64(src)
    return a + b, a.abs() + b.abs()


def flip_merge(normal, flipped, swap, negate_even):
    """handle_paf_and_heat (evaluate/coco_eval.py:197-242) for one map, NHWC: the average of `normal` with
    the x-mirrored, channel-swapped `flipped`; PAF: the channels gathered from an even index change sign."""
    a, f = _t64(normal), _t64(flipped)
    swap = np.asarray(swap)
    g = torch.flip(f, dims=[2])[..., torch.as_tensor(swap)]
    if negate_even:
        g = g * torch.as_tensor(np.where(swap % 2 == 0, -1.0, 1.0))
    return (a + g) / 2, (a.abs() + g.abs()) / 2


def resize_coords(nd, ns, valid):
    """Half-pixel source coordinates of nd destination samples, in the kernels' fp32 arithmetic:
    f = max((d + 0.5) * (valid / nd) - 0.5, 0); i0 = min(int(f), ns - 1); i1 = min(i0 + 1, ns - 1);
    l = min(f - i0, 1).  Returns i0, i1 (int64) and l (float32)."""
    sc = np.float32(valid) / np.float32(nd)
    f = (np.arange(nd, dtype=np.float32) + np.float32(0.5)) * sc - np.float32(0.5)
    f = np.maximum(f, np.float32(0))
    i0 = np.minimum(f.astype(np.int64), ns - 1)
    i1 = np.minimum(i0 + 1, ns - 1)
    l = np.minimum(f - i0.astype(np.float32), np.float32(1))
    return i0, i1, l


def resize_coords_exact(nd, ns, valid):
    """True iff (d + 0.5) * (valid / nd) is exact in fp32 for every d (then a fused and an unfused
    multiply-subtract give the same coordinate and resize_coords is the kernel's value whatever the compiler
    contracted)."""
    sc = np.float32(valid) / np.float32(nd)
    if float(sc) * nd != float(valid):
        return False
    d = np.arange(nd, dtype=np.float64) + 0.5
    p = d * float(sc)
    return bool(np.all(p.astype(np.float32).astype(np.float64) == p))


def resize_bilinear(src_nhwc, hd, wd, h_valid, w_valid, w_clamp=None):
    """bilinear resize of the top-left h_valid x w_valid region of src [n,hs,ws,c] to hd x wd, taps clamped
    to hs rows and w_clamp (default ws) columns."""
    s = _t64(src_nhwc)
    hs, ws = s.shape[1], s.shape[2]
    y0, y1, ly = resize_coords(hd, hs, h_valid)
    x0, x1, lx = resize_coords(wd, ws if w_clamp is None else w_clamp, w_valid)
    ly = torch.as_tensor(ly.astype(np.float64)).view(1, hd, 1, 1)
    lx = torch.as_tensor(lx.astype(np.float64)).view(1, 1, wd, 1)
    a = s.abs()

    def interp(t):
        r0, r1 = t[:, y0], t[:, y1]
        top = r0[:, :, x0] * (1 - lx) + r0[:, :, x1] * lx
        bot = r1[:, :, x0] * (1 - lx) + r1[:, :, x1] * lx
        return top * (1 - ly) + bot * ly
    return interp(s), interp(a)


def accumulate(acc, v, s, alpha, beta):
    """acc <- beta * acc + alpha * v (beta == 0: acc is not read) with its sum of absolute terms."""
    o = float(alpha) * v
    so = abs(float(alpha)) * s
    if beta != 0:
        o = o + float(beta) * _t64(acc)
        so = so + (float(beta) * _t64(acc)).abs()
    return o, so
