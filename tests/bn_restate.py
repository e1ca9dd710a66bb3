"""Host restatement of the training-mode BatchNorm passes (include/rtpose_mi355x.h section 2b continued, csrc/batchnorm.hip,
train.batch_norm): the float64 truth from F.batch_norm(training=True)'s own CPU autograd - never from the code under test -,
the header's documented fp64 / fp32 expressions evaluated in numpy (the bits the kernels must give when every sum is exact),
the error bounds the header states and those that follow from them, and the cases and operands the GPU tests run.
torch CPU + numpy only: no GPU, no library call.

Exactness.  With float32 operands holding small integers every term x - K, (x - K)^2, g, g (x - K) is an integer, and every
partial sum is exact in fp64 in any order while the sum of absolute terms stays below 2^53 (exact_margin).  What follows
the sums is a fixed sequence of fp64 operations (IEEE division and square root are correctly rounded), each restated here
in the header's order, and one rounding to fp32: the kernel's vectors equal these bit for bit.

Bounds.  u32 = 2^-24 (one fp32 rounding), u = 2^-53.  A sum of P terms in any order is within (P - 1) u S of its value, S the
sum of absolute terms.  D1 = sum |x - K| / P, D2 = sum (x - K)^2 / P:
    mean:   u32 |m| + dm,  dm = (P + 8) u (D1 + |m|)
    var:    u32 v + dv,    dv = (3 P + 8) u D2       (S2 / P, md * md <= D2 and the subtraction, each with its sum's error)
    invstd = (v + eps)^-1/2:  u32 t + di,  di = t^3 dv / 2 + 8 u t, doubled for the second-order term
    scale = w t:   u32 |s| + ds,  ds = |w| di + 8 u |s|
    shift = b - m s:   u32 |shift| + |s| dm + |m| ds + 8 u (|b| + |m s|)
    running:  u32 |r'| + momentum * (dm, or dv P / (P - 1)) + 8 u (|r| + |v|)
    dbias = sum g:   u32 |.| + (P + 8) u sum |g|
    dweight = invstd32 (G2 - mdk G1):   2 u32 |dw| + |dw| di / t
              + t ((P + 8) u (sum |g| |x - K| + |m - K| sum |g|) + (dm + 2^-47 |m|) |sum g|)
      (invstd32 carries one fp32 rounding, the result another; mean + mean_lo misses m by the fp64 dust dm and mean_lo's own
       rounding, at most 2^-48 |m|)
    y = fl(fl(scale x) + shift):   |x| (u32 |s| + ds) + bound(shift) + u32 (|s x| + |y|), times (1 + 2^-20)
    dx = (g A - B) - (x - mean) C:  see dx_bound, every operation's rounding and every coefficient's error added up.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import layout_restate as lr

U32 = 2.0 ** -24
U = 2.0 ** -53
EPS = 1e-5
MOMENTUM = 0.1
SLAB_UNIT = 64
SAVE_ROWS = 6           # mean, var, invstd, scale, shift, mean_lo
SLACK = 1.0 + 2.0 ** -20


def slab_geometry(n, h, w):
    """(slab pixels, slabs) of csrc/batchnorm.hip's bn_geometry: equal multiples of 64 pixels, at most 1024 slabs"""
    p = n * h * w
    per = SLAB_UNIT * 1024
    slab = SLAB_UNIT * ((p + per - 1) // per)
    return slab, (p + slab - 1) // slab


def workspace_doubles(channels, n, h, w):
    return slab_geometry(n, h, w)[1] * 2 * channels + 2 * channels


# ---- truth ---------------------------------------------------------------------------------------------------------------------------
def bn64(x, gy, weight, bias, running_mean=None, running_var=None, relu=False, momentum=MOMENTUM, eps=EPS):
    """float64 F.batch_norm(training=True) (+ relu) and its autograd: a dict of y, dx, dweight, dbias, mean, var (biased),
    invstd, scale, shift, running_mean, running_var (the updated ones, or None)"""
    x64 = x.double().detach().requires_grad_(True)
    w64 = weight.double().detach().requires_grad_(True)
    b64 = bias.double().detach().requires_grad_(True)
    rm = running_mean.double().clone() if running_mean is not None else None
    rv = running_var.double().clone() if running_var is not None else None
    y = F.batch_norm(x64, rm, rv, w64, b64, True, momentum, eps)
    if relu:
        y = F.relu(y)
    dx, dw, db = torch.autograd.grad(y, (x64, w64, b64), gy.double())
    mean = x.double().mean((0, 2, 3))
    var = x.double().var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = weight.double() * invstd
    return dict(y=y.detach(), dx=dx, dweight=dw, dbias=db, mean=mean, var=var, invstd=invstd, scale=scale,
                shift=bias.double() - mean * scale, running_mean=rm, running_var=rv)


# ---- the header's expressions in numpy ----------------------------------------------------------------------------------------------
def _nchw(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _c(v):
    return v.reshape(1, -1, 1, 1)


def stats_restate(x, weight, bias, running_mean=None, running_var=None, momentum=MOMENTUM, eps=EPS):
    """(save float32 [6, c], running_mean', running_var') by the documented fp64 expressions, each rounded to fp32 once"""
    x = _nchw(x)
    p = float(x.shape[0] * x.shape[2] * x.shape[3])
    k = x[0, :, 0, 0].astype(np.float64)
    d = x.astype(np.float64) - _c(k)
    s1, s2 = d.sum((0, 2, 3)), (d * d).sum((0, 2, 3))
    md = s1 / p
    mean = k + md
    var = np.maximum(s2 / p - md * md, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = np.asarray(weight, np.float32).astype(np.float64) * invstd
    shift = np.asarray(bias, np.float32).astype(np.float64) - mean * scale
    meanf = mean.astype(np.float32)
    save = np.stack([meanf, var.astype(np.float32), invstd.astype(np.float32), scale.astype(np.float32),
                     shift.astype(np.float32), (mean - meanf.astype(np.float64)).astype(np.float32)])
    rm = rv = None
    if running_mean is not None:
        keep = 1.0 - momentum
        unbiased = var * p / (p - 1.0)
        rm = (keep * np.asarray(running_mean, np.float32).astype(np.float64) + momentum * mean).astype(np.float32)
        rv = (keep * np.asarray(running_var, np.float32).astype(np.float64) + momentum * unbiased).astype(np.float32)
    return save, rm, rv


def apply_restate(x, save, relu):
    """y = fl(fl(scale * x) + shift), max(y, 0) if relu: float32 [n, c, h, w]"""
    x = _nchw(x)
    y = (_c(save[3]) * x).astype(np.float32)
    y = (y + _c(save[4])).astype(np.float32)
    return np.where(y > 0, y, np.float32(0)).astype(np.float32) if relu else y


def masked(x, gy, save, relu):
    """g = relu ? (apply's y > 0 ? gy : 0) : gy, float32"""
    gy = _nchw(gy)
    if not relu:
        return gy
    return np.where(apply_restate(x, save, False) > 0, gy, np.float32(0)).astype(np.float32)


def grad_vectors_restate(x, gy, save, weight, relu):
    """(dbias, dweight, coef float32 [3, c] = A, B, C) by the documented fp64 expressions from the fp32 save rows"""
    x = _nchw(x)
    p = float(x.shape[0] * x.shape[2] * x.shape[3])
    g = masked(x, gy, save, relu).astype(np.float64)
    k = x[0, :, 0, 0].astype(np.float64)
    d = x.astype(np.float64) - _c(k)
    g1, g2 = g.sum((0, 2, 3)), (g * d).sum((0, 2, 3))
    mean = save[0].astype(np.float64) + save[5].astype(np.float64)
    mdk = mean - k
    invstd = save[2].astype(np.float64)
    dw = invstd * (g2 - mdk * g1)
    a = np.asarray(weight, np.float32).astype(np.float64) * invstd
    coef = np.stack([a.astype(np.float32), (a * g1 / p).astype(np.float32), (a * invstd * dw / p).astype(np.float32)])
    return g1.astype(np.float32), dw.astype(np.float32), coef


def dx_restate(x, gy, save, coef, relu):
    """dx = (g * A - B) - (x - mean) * C, every operation rounded to fp32 on its own"""
    x = _nchw(x)
    g = masked(x, gy, save, relu)
    xm = (x - _c(save[0])).astype(np.float32)
    t = (g * _c(coef[0])).astype(np.float32)
    t = (t - _c(coef[1])).astype(np.float32)
    return (t - (xm * _c(coef[2])).astype(np.float32)).astype(np.float32)


# ---- bounds (module docstring) -------------------------------------------------------------------------------------------------------
def bounds(x, gy, weight, bias, t64, running_mean=None, running_var=None, relu=False, momentum=MOMENTUM):
    """dict name -> float64 [c] bound of |kernel - float64| for the per-channel vectors, plus the pieces y_bound / dx_bound
    need.  t64: bn64's dict for the same operands (gy masked by ITS y when relu)."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    n, c, h, w = x64.shape
    p = float(n * h * w)
    k = x64[0, :, 0, 0]
    d = x64 - _c(k)
    d1, d2 = np.abs(d).sum((0, 2, 3)) / p, (d * d).sum((0, 2, 3)) / p
    m, v, t, s, sh = (t64[q].numpy() for q in ("mean", "var", "invstd", "scale", "shift"))
    wt, b = np.asarray(weight, np.float64), np.asarray(bias, np.float64)
    dm = (p + 8) * U * (d1 + np.abs(m))
    dv = (3 * p + 8) * U * d2
    di = 2 * (0.5 * t ** 3 * dv + 8 * U * t)
    ds = np.abs(wt) * di + 8 * U * np.abs(s)
    dsh = np.abs(s) * dm + np.abs(m) * ds + 8 * U * (np.abs(b) + np.abs(m * s))
    out = dict(dm=dm, dv=dv, di=di, ds=ds, dsh=dsh,
               mean=U32 * np.abs(m) + dm, var=U32 * v + dv, invstd=U32 * t + di, scale=U32 * np.abs(s) + ds,
               shift=U32 * np.abs(sh) + dsh)
    if running_mean is not None:
        rm, rv = t64["running_mean"].numpy(), t64["running_var"].numpy()
        r0m, r0v = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
        out["running_mean"] = U32 * np.abs(rm) + momentum * dm + 8 * U * (np.abs(r0m) + np.abs(m))
        out["running_var"] = U32 * np.abs(rv) + momentum * dv * p / (p - 1) + 8 * U * (np.abs(r0v) + 2 * v)
    if gy is not None:
        g = np.asarray(gy, np.float32).astype(np.float64)
        if relu:
            g = np.where(t64["y"].numpy() > 0, g, 0.0)
        sg, sgd = np.abs(g).sum((0, 2, 3)), (np.abs(g) * np.abs(d)).sum((0, 2, 3))
        dw, db = t64["dweight"].numpy(), t64["dbias"].numpy()
        dust_g1 = (p + 8) * U * sg
        dust_dw = np.abs(dw) * di / t + t * ((p + 8) * U * (sgd + np.abs(m - k) * sg) + (dm + 2.0 ** -47 * np.abs(m)) * np.abs(db))
        out.update(dbias=U32 * np.abs(db) + dust_g1, dweight=2 * U32 * np.abs(dw) + dust_dw, dust_g1=dust_g1, dust_dw=dust_dw)
    return out


def y_bound(x, t64, bd):
    """|y - y64| elementwise [n, c, h, w] (before the ReLU, which cannot grow it)"""
    x64 = np.abs(np.asarray(x, np.float32).astype(np.float64))
    s, sh = np.abs(t64["scale"].numpy()), t64["shift"].numpy()
    pre = _c(t64["scale"].numpy()) * np.asarray(x, np.float32).astype(np.float64) + _c(sh)
    return SLACK * (x64 * _c(bd["scale"]) + _c(bd["shift"]) + U32 * (x64 * _c(s) + np.abs(pre)))


def dx_bound(x, gy, weight, t64, bd, relu):
    """|dx - dx64| elementwise for dx = (g A - B) - (x - mean) C: A = w invstd32 (two fp32 roundings and invstd's dust),
    B = A G1 / P (A's error, G1's dust, one rounding), C = A invstd32 dweight / P (A's, invstd32's, dweight's dust, one
    rounding); x - mean carries one rounding and mean's error; each of the five fp32 operations one rounding."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    p = float(x64.shape[0] * x64.shape[2] * x64.shape[3])
    g = np.abs(np.asarray(gy, np.float32).astype(np.float64))
    if relu:
        g = np.where(t64["y"].numpy() > 0, g, 0.0)
    m, t, wt = t64["mean"].numpy(), t64["invstd"].numpy(), np.asarray(weight, np.float64)
    a = wt * t
    b = a * t64["dbias"].numpy() / p
    cc = a * t * t64["dweight"].numpy() / p
    da = 2 * U32 * np.abs(a) + np.abs(wt) * bd["di"]
    db = 3 * U32 * np.abs(b) + np.abs(a) * bd["dust_g1"] / p
    dc = 4 * U32 * np.abs(cc) + np.abs(a) * t * bd["dust_dw"] / p + np.abs(cc) * bd["di"] / t
    xm = np.abs(x64 - _c(m))
    dxm = U32 * xm + _c(bd["mean"])
    ga, xc = g * _c(np.abs(a)), xm * _c(np.abs(cc))
    return SLACK * (g * _c(da) + _c(db) + xm * _c(dc) + _c(np.abs(cc)) * dxm
                    + U32 * (ga + (ga + _c(np.abs(b))) + xc + np.abs(t64["dx"].numpy())))


# ---- cases of tests/test_batchnorm_gpu.py --------------------------------------------------------------------------------------------
# x / gy / out: (cstride, choff) of each buffer (out: y and dx); gaps of 1, 2 and 0 pixels.  "vector": every cstride and choff
# a multiple of 4 floats.  Channels on both sides of a workgroup's width (64 units: 64 scalar, 256 vector channels), P at 2,
# 63, 64, 65 and shapes with several slabs, a partial last one and slabs across image boundaries (held to the library's
# query by tests/test_batchnorm_cpu.py).
Case = namedtuple("Case", "channels n h w x gy out tags")
CASES = [
    Case(1, 2, 1, 1, (1, 0), (1, 0), (1, 0), "scalar; P = 2; one channel"),
    Case(3, 1, 1, 2, (5, 2), (8, 4), (4, 1), "scalar; P = 2; three layouts, the slices end at cstride"),
    Case(4, 1, 7, 9, (4, 0), (4, 0), (4, 0), "vector; P = 63; one unit"),
    Case(5, 1, 8, 8, (12, 4), (12, 4), (12, 4), "vector; P = 64 = one slab; a last unit of one channel"),
    Case(5, 1, 5, 13, (7, 1), (9, 3), (7, 1), "scalar; P = 65; several slabs; one pixel in the last slab"),
    Case(64, 2, 5, 3, (64, 0), (64, 0), (64, 0), "vector; 16 units"),
    Case(64, 1, 3, 11, (67, 3), (65, 1), (67, 3), "scalar; exactly one workgroup width of units"),
    Case(65, 1, 3, 11, (67, 1), (67, 1), (67, 1), "scalar; two channel tiles"),
    Case(255, 1, 4, 4, (256, 0), (256, 0), (260, 4), "vector; 64 units, the last of 3 channels"),
    Case(256, 2, 3, 3, (256, 0), (256, 0), (256, 0), "vector; exactly one workgroup width"),
    Case(257, 1, 2, 3, (264, 4), (264, 4), (264, 4), "vector; two channel tiles, the second of one channel"),
    Case(257, 1, 2, 3, (259, 1), (264, 4), (264, 4), "scalar; five channel tiles"),
    Case(8, 3, 19, 18, (12, 4), (12, 4), (16, 8), "vector; several slabs; partial last slab; slabs across image boundaries"),
    Case(19, 2, 9, 7, (24, 4), (21, 1), (24, 4), "scalar; several slabs; partial last slab; across an image boundary"),
    Case(8, 2, 8, 8, (8, 0), (8, 0), (8, 0), "vector; several slabs; P = 2 slabs, full"),
    Case(6, 1, 129, 511, (8, 0), (8, 0), (8, 0), "vector; several slabs; slabs of 128 pixels; partial last slab"),
]


def case_id(c):
    return "c%d_%dx%dx%d_x%d.%d_g%d.%d_o%d.%d" % ((c.channels, c.n, c.h, c.w) + c.x + c.gy + c.out)


def layouts(c):
    return (lr.padded(c.x[0], c.h, c.w, 1, c.x[1]), lr.padded(c.gy[0], c.h, c.w, 2, c.gy[1]),
            lr.padded(c.out[0], c.h, c.w, 0, c.out[1]))


def is_vector(c):
    return all(v % 4 == 0 for pair in (c.x, c.gy, c.out) for v in pair)


def affine(channels, exact):
    """(weight, bias, running_mean, running_var) float32: dyadic for the exact sets, random otherwise (both signs, a zero
    weight where there are three channels)"""
    g = torch.Generator().manual_seed(11 + channels)
    if exact:
        w = torch.tensor([(0.5, -1.0, 2.0, 0.25, 1.0)[i % 5] for i in range(channels)])
        b = torch.tensor([(0.0, 1.0, -0.5, 3.0)[i % 4] for i in range(channels)])
    else:
        w, b = torch.randn(channels, generator=g), torch.randn(channels, generator=g)
        if channels >= 3:
            w[2] = 0.0
    return w.float(), b.float(), torch.randn(channels, generator=g), torch.rand(channels, generator=g) + 0.5


def exact_operands(c, seed=0):
    """(x, gy) float32 integers: x in -4 .. 4 on top of a per-channel integer offset up to +-40, gy in -3 .. 3"""
    g = torch.Generator().manual_seed(7000 + seed)
    shape = (c.n, c.channels, c.h, c.w)
    off = torch.randint(-40, 41, (1, c.channels, 1, 1), generator=g)
    x = (torch.randint(-4, 5, shape, generator=g) + off).float()
    gy = torch.randint(-3, 4, shape, generator=g).float()
    return x, gy


def exact_margin(x, gy):
    """the largest sum of absolute terms of the four sums (and of their squares' sum): below 2^53 every fp64 sum is exact"""
    d = (x.double() - x.double()[0:1, :, 0:1, 0:1]).abs()
    return max(d.sum((0, 2, 3)).max().item(), (d * d).sum((0, 2, 3)).max().item(), gy.double().abs().sum((0, 2, 3)).max().item(),
               (gy.double().abs() * d).sum((0, 2, 3)).max().item())


def random_operands(c, seed=0, big_mean=False):
    """(x, gy) float32: per-channel std in [0.5, 2), mean N(0, 1) - or 1000 std with `big_mean` -, randn gy"""
    g = torch.Generator().manual_seed(9000 + seed + (500 if big_mean else 0))
    shape = (c.n, c.channels, c.h, c.w)
    std = (torch.rand(1, c.channels, 1, 1, generator=g) * 1.5 + 0.5)
    mean = 1000.0 * std if big_mean else torch.randn(1, c.channels, 1, 1, generator=g)
    x = (torch.randn(shape, generator=g) * std + mean).float()
    return x, torch.randn(shape, generator=g).float()


RELU_SEEDS = 16


def relu_operands(c):
    """(x, gy, weight, bias, running_mean, running_var, t64, bd, margin) of the first seed < RELU_SEEDS for which no float64
    pre-activation lies within y_bound of zero (margin = min (|y64| - bound) > 0), so that the fp32 mask is the float64
    one; None if there is none (the case then runs its random operands without a ReLU)."""
    w, b, rm, rv = affine(c.channels, False)
    for seed in range(RELU_SEEDS):
        x, gy = random_operands(c, seed=100 + seed)
        t64 = bn64(x, gy, w, b, rm, rv, relu=True)
        bd = bounds(x.numpy(), gy.numpy(), w.numpy(), b.numpy(), t64, rm.numpy(), rv.numpy(), relu=True)
        pre = t64["scale"].view(1, -1, 1, 1) * x.double() + t64["shift"].view(1, -1, 1, 1)
        margin = float((pre.abs().numpy() - y_bound(x.numpy(), t64, bd)).min())
        if margin > 0:
            return x, gy, w, b, rm, rv, t64, bd, margin
    return None
