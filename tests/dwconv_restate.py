"""Host restatement of the depthwise 3x3 backward passes (include/rtpose_mi355x.h section 2b continued,
csrc/dwconv_backward.hip, train.dwconv3x3 / train.conv3x3_s2) and of the ShuffleNetV2 training forward
(train.shufflenet_forward): the float64 truth from F.conv2d(groups=C)'s own CPU autograd - never from the code under
test -, the header's sums in numpy float64, the data gradient in fp32 in the header's order of operations (the bits the
kernel must give), the zero-stuffing identities the stem's backward rests on, the reference forward in training mode on a
dict of tensors, and the cases and operands the GPU tests run.  torch CPU + numpy only: no GPU, and no library call but
host_refusals', which lists the calls both launchers refuse on the host.

H, W are the conv's input size, stride 1 or 2, Ho = (H - 1) / stride + 1, Wo likewise.

Weight gradient.  dw[c][ky][kx] = sum gy[n, yo, xo, c] * x[n, stride yo + ky - 1, stride xo + kx - 1, c] over the valid
output pixels, dbias[c] = sum gy.  The kernel adds fp64 terms (the product of two fp32 values is exact in fp64) in a fixed
order and rounds once: against the float64 sum v, |result - v| <= 2^-24 |v| + (P_out + 8) 2^-53 sum |terms| (a sum of
P_out terms in any order is within (P_out - 1) u of its value times the sum of absolute terms; the rest is slack), and
with small-integer operands every partial sum is exact, so the result is fp32(v) bit for bit.

Data gradient.  dx[n, y, x, c] = sum over the taps (ky, kx) with (y + 1 - ky), (x + 1 - kx) divisible by stride of
w[ky * 3 + kx][c] * gy[n, (y + 1 - ky) / stride, (x + 1 - kx) / stride, c], in fp32: from +0, one rounding per product and
one per add, the taps in order of ascending gy row, then ascending gy column, i.e. ky = 2, 1, 0 and within a row
kx = 2, 1, 0.  A tap on yo = -1, yo = Ho, xo = -1 or xo = Wo reads a zero of gy's gap: its product is a zero of either
sign, which changes no sum that started from +0.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import layout_restate as lr

U32 = 2.0 ** -24
U = 2.0 ** -53
SLAB_UNIT = 64
TERMS = 10
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def out_size(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def slab_geometry(n, h, w, stride):
    """(slab pixels, slabs) over the N * Ho * Wo output pixels: equal multiples of 64 pixels, at most 1024 slabs"""
    ho, wo = out_size(h, w, stride)
    p = n * ho * wo
    per = SLAB_UNIT * 1024
    slab = SLAB_UNIT * ((p + per - 1) // per)
    return slab, (p + slab - 1) // slab


def workspace_doubles(c, n, h, w, stride):
    return slab_geometry(n, h, w, stride)[1] * TERMS * c


# ---- truth ---------------------------------------------------------------------------------------------------------------------------
def autograd64(x, weight, gy, stride):
    """float64 F.conv2d(x, weight [C, 1, 3, 3], None, stride, 1, groups=C) and its autograd: (y, dx, dw)"""
    x64 = torch.as_tensor(x).double().detach().requires_grad_(True)
    w64 = torch.as_tensor(weight).double().detach().requires_grad_(True)
    y = F.conv2d(x64, w64, None, stride, 1, 1, x64.shape[1])
    dx, dw = torch.autograd.grad(y, (x64, w64), torch.as_tensor(gy).double())
    return y.detach(), dx, dw


# ---- the header's expressions in numpy -------------------------------------------------------------------------------------------------
def _taps_x(x, stride, ho, wo):
    """x [n, c, h, w] float64 -> the nine shifted views [9][n, c, ho, wo]: x[n, c, stride yo + ky - 1, stride xo + kx - 1]"""
    n, c, h, w = x.shape
    xp = np.zeros((n, c, stride * (ho - 1) + 3, stride * (wo - 1) + 3), np.float64)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    return [xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]


def wgrad_restate(x, gy, stride):
    """(dw float64 [c, 1, 3, 3], dbias float64 [c], sum |terms| of each in the same shapes) by the header's sums"""
    x = np.asarray(x, np.float32).astype(np.float64)
    g = np.asarray(gy, np.float32).astype(np.float64)
    n, c, h, w = x.shape
    ho, wo = out_size(h, w, stride)
    assert g.shape == (n, c, ho, wo)
    taps = _taps_x(x, stride, ho, wo)
    # (+ 0.0: the kernel's sums start from +0, so a sum of nothing but -0 terms is +0 there; numpy's would be -0)
    dw = np.stack([(g * t).sum((0, 2, 3)) + 0.0 for t in taps], 1).reshape(c, 1, 3, 3)
    sw = np.stack([np.abs(g * t).sum((0, 2, 3)) for t in taps], 1).reshape(c, 1, 3, 3)
    return dw, g.sum((0, 2, 3)) + 0.0, sw, np.abs(g).sum((0, 2, 3))


def wgrad_bound(v, s, p_out):
    """the header's bound of |kernel - float64| for a sum v with sum of absolute terms s"""
    return U32 * np.abs(v) + (p_out + 8) * U * s


def tap_major(weight):
    """[c, 1, 3, 3] -> [9, c], the forward's packing: w9[ky * 3 + kx][c]"""
    w = np.asarray(weight)
    return np.ascontiguousarray(w.reshape(w.shape[0], 9).T)


def _tap_index(size, out, k, stride):
    """the positions y in [0, size) that tap k reaches, and the rows yo + 1 of the zero-ringed gy they read"""
    ys = np.array([y for y in range(size) if (y + 1 - k) % stride == 0], dtype=np.int64)
    yo = (ys + 1 - k) // stride
    assert ((yo >= -1) & (yo <= out)).all()
    return ys, yo + 1


def dgrad_restate(gy, weight, h, w, stride, dtype=np.float32):
    """dx [n, c, h, w] in `dtype` arithmetic, one rounding per product and per add, in the header's order"""
    g = np.asarray(gy, np.float32).astype(dtype)
    wt = np.asarray(weight, np.float32).astype(dtype)
    n, c, ho, wo = g.shape
    assert (ho, wo) == out_size(h, w, stride)
    gp = np.zeros((n, c, ho + 2, wo + 2), dtype)
    gp[:, :, 1:ho + 1, 1:wo + 1] = g
    acc = np.zeros((n, c, h, w), dtype)
    for ky in (2, 1, 0):
        ys, yr = _tap_index(h, ho, ky, stride)
        for kx in (2, 1, 0):
            xs, xr = _tap_index(w, wo, kx, stride)
            if ys.size == 0 or xs.size == 0:
                continue
            prod = (wt[:, 0, ky, kx].reshape(1, c, 1, 1) * gp[:, :, yr[:, None], xr[None, :]]).astype(dtype)
            acc[:, :, ys[:, None], xs[None, :]] = (acc[:, :, ys[:, None], xs[None, :]] + prod).astype(dtype)
    return acc


# ---- the stem's backward by zero stuffing (train.conv3x3_s2) -------------------------------------------------------------------------------
def zero_stuff(gy, h, w):
    """gyz [n, c, h, w]: gyz[:, :, 2 y, 2 x] = gy[:, :, y, x], zero elsewhere"""
    gyz = torch.zeros(gy.shape[0], gy.shape[1], h, w, dtype=gy.dtype)
    gyz[:, :, ::2, ::2] = gy
    return gyz


def stem_grads_by_stuffing(x, weight, gy):
    """(dW, dx) of conv2d(x, weight, stride=2, padding=1) from the stride-1 operations on the zero-stuffed gradient: the
    stride-1 weight gradient of (x, gyz) and the stride-1 'same' conv of gyz with the flipped, transposed filter"""
    n, _, h, w = x.shape
    gyz = zero_stuff(gy, h, w)
    k = weight.shape[2]
    w1 = weight.detach().clone().requires_grad_(True)
    y1 = F.conv2d(x, w1, None, 1, k // 2)
    (dw,) = torch.autograd.grad(y1, (w1,), gyz)
    dx = F.conv2d(gyz, weight.flip(2, 3).transpose(0, 1).contiguous(), None, 1, k // 2)
    return dw, dx


# ---- the reference forward in training mode, on a dict of tensors ----------------------------------------------------------------------------
def tensors_of(model, dtype=torch.float64):
    """{key: tensor} of the module's state_dict, detached copies in `dtype` (num_batches_tracked stays int64); the
    parameters require a gradient"""
    params = set(k for k, _ in model.named_parameters())
    out = {}
    for k, v in model.state_dict().items():
        t = v.detach().clone()
        if t.is_floating_point():
            t = t.to(dtype)
        out[k] = t.requires_grad_(True) if k in params else t
    return out


def _bn(sd, p, x, relu):
    sd[p + '.num_batches_tracked'] += 1
    y = F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], True, BN_MOMENTUM, BN_EPS)
    return F.relu(y) if relu else y


def _cbr(sd, p, x, relu, stride=1, padding=0, groups=1):
    return _bn(sd, p + '.1', F.conv2d(x, sd[p + '.0.weight'], None, stride, padding, 1, groups), relu)


def _shuffle(x, groups=2):
    n, c, h, w = x.shape
    return x.view(n, groups, c // groups, h, w).permute(0, 2, 1, 3, 4).reshape(n, c, h, w)


def ref_block(sd, p, x, stride, two_branch):
    """lib/network/rtpose_shufflenetV2.py:31-63, oracle/shufflenet_oracle.py's _block order, in training mode"""
    def conv(z):
        z = _cbr(sd, p + '.conv.0', z, True)
        z = _cbr(sd, p + '.conv.1', z, False, stride, 1, z.shape[1])
        return _cbr(sd, p + '.conv.2', z, True)
    if not two_branch:
        half = x.shape[1] // 2
        x = torch.cat((x[:, :half], conv(x[:, half:])), 1)
    else:
        z = _cbr(sd, p + '.conv0.0', x, False, stride, 1, x.shape[1])
        z = _cbr(sd, p + '.conv0.1', z, True)
        x = torch.cat((z, conv(x)), 1)
    return _shuffle(x)


def ref_forward(sd, x):
    """reference Network.forward :144-148 in training mode -> (PAF, HEAT); updates the running statistics of `sd` in place"""
    x = _bn(sd, 'network.0', x, False)
    x = _cbr(sd, 'network.1', x, True, 2, 1)
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    for si, (nblocks, stride) in enumerate(((4, 2), (8, 1), (4, 1))):
        for b in range(nblocks):
            x = ref_block(sd, 'network.%d.%d' % (3 + si, b), x, stride if b == 0 else 1, b == 0)
    x = _cbr(sd, 'network.6', x, True)
    return F.conv2d(x, sd['paf.weight'], sd['paf.bias']), F.conv2d(x, sd['heatmap.weight'], sd['heatmap.bias'])


def torch_ops(spy=None):
    """(conv, bn, dw, stem) of torch's functional forms, in the modules' dtype: what train.shufflenet_forward runs when the
    tests hand it torch instead of the library.  spy: a list that receives the pre-activation of every BatchNorm that is
    followed by a ReLU."""
    def conv(x, m):
        return F.conv2d(x, m.weight, m.bias, m.stride, m.padding, m.dilation, m.groups)

    def bn(x, m, relu):
        m.num_batches_tracked += 1
        z = F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps)
        if relu and spy is not None:
            spy.append(z.detach())
        return F.relu(z) if relu else z

    return conv, bn, conv, conv


def seed_module(mod, seed):
    """He-scaled filters, BatchNorm weights in [0.5, 1.5), small biases: activations of unit scale at every depth"""
    rng = np.random.Generator(np.random.PCG64(seed))
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.from_numpy(rng.standard_normal(tuple(m.weight.shape)) * np.sqrt(2.0 / fan_in)).float())
                if m.bias is not None:
                    m.bias.copy_(torch.from_numpy(rng.standard_normal(m.bias.shape[0]) * 0.05).float())
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.weight.shape[0])).float())
                m.bias.copy_(torch.from_numpy(rng.standard_normal(m.bias.shape[0]) * 0.1).float())
    return mod


# ---- cases of tests/test_dwconv_backward_gpu.py ----------------------------------------------------------------------------------------------
# x / gy / dx: (cstride, choff) of each buffer.  "vector": every cstride and choff a multiple of 4 floats.  The shapes the
# issue names, each at both strides; then channels on both sides of a workgroup's width (64 units: 64 scalar, 256 vector
# channels); then, per stride, a shape whose output pixels make at least 3 slabs with a ragged last one, one slab boundary
# inside an image and one at an image boundary (8 x 12 = 96 output pixels per image, 3 images: boundaries at 64, 128,
# 192 = 2 * 96, 256; 32 pixels in the last slab), in a scalar and in a vector layout.
Case = namedtuple("Case", "n c h w stride x gy dx tags")
_SHAPES = [
    (1, 4, 1, 1, (4, 0), (4, 0), (4, 0), "vector; one pixel"),
    (2, 3, 5, 7, (5, 1), (7, 2), (4, 1), "scalar; odd sizes"),
    (1, 58, 8, 6, (64, 4), (60, 0), (64, 4), "vector; even sizes: the far tap on yo = Ho; a last unit of 2 channels"),
    (2, 8, 9, 11, (12, 4), (12, 4), (16, 8), "vector; two whole units"),
    (1, 70, 3, 4, (71, 1), (70, 0), (73, 3), "scalar; two channel tiles"),
    (1, 260, 2, 3, (260, 0), (264, 4), (260, 0), "vector; two channel tiles, the second of one unit"),
]
CASES = [Case(n, c, h, w, s, x, gy, dx, tags) for (n, c, h, w, x, gy, dx, tags) in _SHAPES for s in (1, 2)]
SLAB_CASES = [
    Case(3, 6, 8, 12, 1, (7, 1), (6, 0), (9, 2), "scalar; 5 slabs"),
    Case(3, 6, 8, 12, 1, (8, 0), (8, 0), (12, 4), "vector; 5 slabs; a last unit of 2 channels"),
    Case(3, 6, 15, 24, 2, (7, 1), (6, 0), (9, 2), "scalar; 5 slabs"),
    Case(3, 6, 16, 23, 2, (8, 0), (8, 0), (12, 4), "vector; 5 slabs; a last unit of 2 channels"),
]
CASES += SLAB_CASES


def case_id(c):
    return "%dx%dx%dx%d_s%d_x%d.%d_g%d.%d_d%d.%d" % ((c.n, c.c, c.h, c.w, c.stride) + c.x + c.gy + c.dx)


def slab_facts(c, slab, slabs):
    """what SLAB_CASES promise, from a (slab, slabs) pair: at least 3 slabs, a ragged last one, one slab boundary inside an
    image and one at an image boundary"""
    ho, wo = out_size(c.h, c.w, c.stride)
    per, p = ho * wo, c.n * ho * wo
    cuts = [k * slab for k in range(1, slabs)]
    return dict(slabs=slabs, ragged=p % slab != 0, inside=any(q % per for q in cuts), at_image=any(q % per == 0 for q in cuts))


def layouts(c, gap_x=1, gap_gy=1, gap_dx=0):
    """(lx of the conv's input, lgy of its output gradient, ldx) with the gaps given"""
    ho, wo = out_size(c.h, c.w, c.stride)
    return (lr.padded(c.x[0], c.h, c.w, gap_x, c.x[1]), lr.padded(c.gy[0], ho, wo, gap_gy, c.gy[1]),
            lr.padded(c.dx[0], c.h, c.w, gap_dx, c.dx[1]))


def exact_operands(c, seed=0):
    """(x, gy, weight) float32 integers: |x| <= 4, |gy| <= 3, |w| <= 3: every sum far below 2^24, let alone 2^53"""
    g = torch.Generator().manual_seed(5000 + seed)
    ho, wo = out_size(c.h, c.w, c.stride)
    return (torch.randint(-4, 5, (c.n, c.c, c.h, c.w), generator=g).float(), torch.randint(-3, 4, (c.n, c.c, ho, wo), generator=g).float(),
            torch.randint(-3, 4, (c.c, 1, 3, 3), generator=g).float())


def random_operands(c, seed=0):
    g = torch.Generator().manual_seed(6000 + seed)
    ho, wo = out_size(c.h, c.w, c.stride)
    return (torch.randn(c.n, c.c, c.h, c.w, generator=g), torch.randn(c.n, c.c, ho, wo, generator=g),
            torch.randn(c.c, 1, 3, 3, generator=g))


def host_refusals(capi, c, x, gy, dw, db, ws, w9, dx):
    """(what, rc) of every call the launchers refuse before any HIP call; the pointers are never followed"""
    lib, L = capi.lib, lambda l: C.byref(capi.Layout(*l))          # noqa: E731
    lx, lgy, ldx = layouts(c)
    doubles = workspace_doubles(c.c, c.n, c.h, c.w, c.stride)
    s = None

    def wg(x=x, lx=lx, gy=gy, lgy=lgy, dw=dw, db=db, ws=ws, doubles=doubles, ch=c.c, n=c.n, h=c.h, w=c.w, stride=c.stride):
        return lib.rtpose_dwconv3x3_wgrad(x, L(lx) if lx else None, gy, L(lgy) if lgy else None, dw, db, ws, doubles, ch, n, h, w, stride, s)

    def dg(gy=gy, lgy=lgy, w9=w9, dx=dx, ldx=ldx, ch=c.c, n=c.n, h=c.h, w=c.w, stride=c.stride):
        return lib.rtpose_dwconv3x3_dgrad(gy, L(lgy) if lgy else None, w9, dx, L(ldx) if ldx else None, ch, n, h, w, stride, s)

    lx0, lgy0, _ = layouts(c, gap_x=0, gap_gy=0)
    out = [("wgrad stride 3", wg(stride=3)), ("wgrad stride 0", wg(stride=0)), ("wgrad x gap 0", wg(lx=lx0)),
           ("wgrad short workspace", wg(doubles=doubles - 1)), ("wgrad NULL workspace", wg(ws=None)), ("wgrad NULL x", wg(x=None)),
           ("wgrad NULL gy", wg(gy=None)), ("wgrad NULL dw", wg(dw=None)), ("wgrad NULL lx", wg(lx=None)), ("wgrad NULL lgy", wg(lgy=None)),
           ("wgrad C = 0", wg(ch=0)), ("wgrad C < 0", wg(ch=-4)), ("wgrad N = 0", wg(n=0)), ("wgrad H = 0", wg(h=0)),
           ("wgrad slice beyond cstride", wg(ch=c.x[0] - c.x[1] + 1)),
           ("dgrad stride 3", dg(stride=3)), ("dgrad gy gap 0", dg(lgy=lgy0)), ("dgrad NULL gy", dg(gy=None)), ("dgrad NULL w", dg(w9=None)),
           ("dgrad NULL dx", dg(dx=None)), ("dgrad NULL lgy", dg(lgy=None)), ("dgrad NULL ldx", dg(ldx=None)), ("dgrad C = 0", dg(ch=0)),
           ("dgrad W = 0", dg(w=0)), ("dgrad slice beyond cstride", dg(ch=c.dx[0] - c.dx[1] + 1))]
    return out
