"""NaN and Inf through the kernels a training step launches (include/rtpose_mi355x.h, section 2, "Non-finite values"): the
operands, the float64 references and the comparison.  torch CPU + numpy only: no GPU, no library call.
tests/test_nonfinite_cpu.py asserts the conditions of every case, tests/test_nonfinite_gpu.py runs the cases.

Finite part: x, gy and the filters are drawn from {-2, -1, 1, 2} - never zero, so Inf * 0 does not arise by accident -, the
bias from {-3 .. 3}: every finite output is an integer fp32 holds exactly, in any summation order, and is compared with ==
(a bf16 output after its one rounding, lr.bf16_rne).

Injected part: single elements at stated positions - one NaN (the bit patterns 0x7FC00000 and 0xFFC00001 in turn, never the
payload of conv_driver.SENTINEL: a NaN result stays distinguishable from a word nobody wrote), one +Inf, one -Inf.  With single
injected elements the class of an output - NaN, +Inf, -Inf or finite - does not depend on the summation order: Inf + finite,
Inf + NaN and +Inf + -Inf give the same class in any order, and the integers cannot overflow a partial sum.  So the float64
reference (torch on the CPU; conv_taps / wgrad_taps restate it tap by tap) decides the class without argument.

Where a reference would have to decide what Inf * (a zero of the padding) is, the inputs stay away from it: the Inf of an
output gradient lies at least k // 2 from every border (5 x 7 maps for k <= 3, 9 x 9 for k = 7), the zero-stuffed stride-2
stems get injections into gy and the filters only, an injected filter element sits at the centre tap.  NaN goes anywhere."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_driver as cd
import layout_restate as lr

NAN_BITS = (0x7FC00000, 0xFFC00001)
PINF, NINF = 0x7F800000, 0xFF800000
SENTINELS = (cd.SENTINEL, 0x7FC1 << 16)         # an unwritten fp32 word; an unwritten bf16 word (0x7FC1) widened to fp32
FINITE, NAN, POS, NEG = 0, 1, 2, 3
NAMES = {FINITE: "finite", NAN: "NaN", POS: "+Inf", NEG: "-Inf"}
VALUES = torch.tensor([-2.0, -1.0, 1.0, 2.0])


def f32_of(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def classes(a):
    """FINITE / NAN / POS / NEG per element"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), NAN, np.where(a == np.inf, POS, np.where(a == -np.inf, NEG, FINITE))).astype(np.uint8)


def differences(got, want):
    """What keeps `got` (float32 array: what a kernel stored) from being `want` (the reference, any float type), as a list of
    strings - empty if NaN sits exactly where want has NaN, the same signed Inf exactly where want has Inf and every other
    value is == (-0 and +0 compare equal: torch's relu(-0.) is -0., the kernels' is +0).  A word that still holds a
    sentinel pattern was never written and is no NaN result."""
    got = np.ascontiguousarray(np.atleast_1d(got), dtype=np.float32)
    want = np.atleast_1d(np.asarray(want))
    if got.shape != want.shape:
        return ["shape %s, expected %s" % (got.shape, want.shape)]
    out = []
    bits = got.view(np.uint32)
    unwritten = np.isin(bits, np.array(SENTINELS, dtype=np.uint32))
    if unwritten.any():
        out.append("%d words still hold the sentinel, first at %s" % (int(unwritten.sum()), tuple(np.argwhere(unwritten)[0])))
    cg, cw = classes(got), classes(want)
    bad = cg != cw
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        out.append("%d of %d elements in another class, first at %s: %s (%r) where %s is due"
                   % (int(bad.sum()), bad.size, at, NAMES[int(cg[at])], got[at], NAMES[int(cw[at])]))
    fin = (cg == FINITE) & (cw == FINITE)
    wrong = fin & (got.astype(np.float64) != np.where(fin, want, 0).astype(np.float64))
    if wrong.any():
        at = tuple(int(i) for i in np.argwhere(wrong)[0])
        out.append("%d finite elements differ, first at %s: %r != %r" % (int(wrong.sum()), at, got[at], want[at]))
    return out


def same_class_and_values(got, want, what=""):
    d = differences(got, want)
    assert not d, "%s: %s" % (what, "; ".join(d))


def holds_every_class(want, injected, finite=True):
    """the condition on a case's expected output: at least one element of each class in `injected` and one finite element"""
    have = set(np.unique(classes(want)).tolist())
    return set(injected) <= have and (not finite or FINITE in have)


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def draw(g, *shape):
    return VALUES[torch.randint(0, 4, shape, generator=g)].clone()


def inject(t, injections):
    """t (float32 tensor) with (index tuple, bit pattern) written in place, bit for bit"""
    a = t.numpy().view(np.uint32)
    for idx, bits in injections:
        a[idx] = bits
    return t


def round_bf16(a):
    """float32 array -> rounded once to bf16 (RNE; NaN stays NaN, Inf stays Inf), as float32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    r = lr.bf16_to_f32(lr.bf16_rne(a)).reshape(a.shape)
    return np.where(np.isnan(a), a, r)


# ---- the forward convs ---------------------------------------------------------------------------------------------------------------
# inj: ((n, c, y, x), bits) into x.  zero: (output channel, bias) of the one all-zero filter of the finite case.
Conv = namedtuple("Conv", "tag kind k n cin h w cout relu out_f32 inj aligned zero", defaults=(False, None))


def _three(nan, pinf, ninf, i):
    return ((nan, NAN_BITS[i % 2]), (pinf, PINF), (ninf, NINF))


# (n, h, w) -> positions of NaN, +Inf, -Inf, and of the -Inf whose footprint overlaps +Inf's also for k = 1
MAPS = {
    "strip": ((2, 9, 9), (0, 1, 1, 2), (1, 3, 1, 1), (1, 6, 7, 7), (1, 6, 1, 1)),
    "tiles2d": ((1, 2, 131), (0, 1, 0, 5), (0, 3, 1, 60), (0, 6, 0, 120), (0, 6, 1, 60)),
    "tail": ((2, 5, 7), (0, 1, 1, 2), (1, 3, 1, 1), (1, 6, 3, 5), (1, 6, 1, 1)),
}


def _conv_f32():
    cs, i = [], 0
    for k in (1, 3, 7):
        for relu in (0, 1):
            for name, ((n, h, w), a, b, c, _) in MAPS.items():
                cs.append(Conv("k%d-relu%d-%s" % (k, relu, name), "f32", k, n, 8, h, w, 8, relu, True, _three(a, b, c, i)))
                i += 1
    for k in (1, 3):            # +Inf and -Inf at one pixel in two channels: wherever the two filters agree in sign, NaN
        (n, h, w), a, b, _, c = MAPS["strip"]
        cs.append(Conv("k%d-relu0-overlap" % k, "f32", k, n, 8, h, w, 8, 0, True, _three(a, b, c, i)))
        i += 1
    return cs


def _conv_bf16():
    """one case per epilogue of conv_tile (conv_mfma_bf16.hip): the transposed one (`tr`: k x k, cout % 64 == 0, bf16 out, an
    aligned layout), the vec_store one (the same with k = 1), the element-wise one (anything else)"""
    cs, i = [], 0
    (n, h, w), a, b, c, ov = MAPS["strip"]
    a, b, c, ov = [(p[0], p[1] * 2, p[2], p[3]) for p in (a, b, c, ov)]       # 16 input channels
    for relu in (0, 1):
        cs.append(Conv("relu%d-transposed" % relu, "bf16", 3, n, 16, h, w, 64, relu, False, _three(a, b, c, i), True))
        cs.append(Conv("relu%d-vec_store" % relu, "bf16", 1, n, 16, h, w, 64, relu, False, _three(a, b, c, i + 1), True))
        for of in (False, True):
            t = "f32out" if of else "bf16out"
            cs.append(Conv("relu%d-elementwise-k3-%s" % (relu, t), "bf16", 3, n, 16, h, w, 8, relu, of, _three(a, b, c, i)))
            cs.append(Conv("relu%d-elementwise-k7-%s" % (relu, t), "bf16", 7, n, 16, h, w, 8, relu, of, _three(a, b, c, i + 1)))
        cs.append(Conv("relu%d-elementwise-k1-cout64-f32out" % relu, "bf16", 1, n, 16, h, w, 64, relu, True, _three(a, b, c, i), True))
        i += 1
    cs.append(Conv("relu0-overlap-transposed", "bf16", 3, n, 16, h, w, 64, 0, False, _three(a, b, ov, 0), True))
    # 64 input channels: rtpose_conv2d_bf16 hands these to the kernel of csrc/conv_c64_bf16.hip (rtpose_conv3x3_c64_bf16_fits) -
    # conv2_1 of an RtposeVGG, and its data gradient, in a layout-resident bf16 run
    for relu in (0, 1):
        for cout in (64, 128):
            cs.append(Conv("relu%d-c64-cout%d" % (relu, cout), "bf16", 3, n, 64, h, w, cout, relu, False, _three(a, b, c, relu), True))
    cs.append(Conv("relu0-c64-overlap", "bf16", 3, n, 64, h, w, 64, 0, False, _three(a, b, ov, 1), True))
    (n2, h2, w2), a2, b2, c2, _ = MAPS["tiles2d"]
    cs.append(Conv("relu0-2d-k3-f32out", "bf16", 3, n2, 16, h2, w2, 8, 0, True, _three(a2, b2, c2, 1)))
    # finite: a sum in (-3.4e38, -3.0e38) is no ReLU's business.  The only case with a zero filter (and no injection)
    cs.append(Conv("relu0-finite-3.3e38", "bf16", 3, n, 16, h, w, 8, 0, True, (), False, (5, -3.3e38)))
    return cs


CONV_F32, CONV_BF16 = _conv_f32(), _conv_bf16()


def conv_operands(c, seed=0):
    """(x [n, cin, h, w] with the injections, w [cout, cin, k, k], bias [cout]) float32"""
    g = torch.Generator().manual_seed(9000 + seed + 7 * c.k + c.cout + c.h)
    x, wt = draw(g, c.n, c.cin, c.h, c.w), draw(g, c.cout, c.cin, c.k, c.k)
    b = torch.randint(-3, 4, (c.cout,), generator=g).float()
    if c.zero is not None:
        wt[c.zero[0]] = 0.0
        b[c.zero[0]] = c.zero[1]
    return inject(x, c.inj), wt, b


def conv_reference(c, x, wt, b, relu=None):
    """float64 conv2d (+ torch's relu) of the operands; a bf16 output rounded once.  float64 [n, cout, h, w] (numpy)"""
    y = F.conv2d(x.double(), wt.double(), b.double(), padding=c.k // 2)
    if c.relu if relu is None else relu:
        y = F.relu(y)
    y = y.numpy()
    if c.kind == "bf16" and not c.out_f32:
        y = round_bf16(y.astype(np.float32)).astype(np.float64)
    return y


def conv_taps(x, wt, b):
    """the same sum tap by tap in numpy float64, over the pixels of the map only: no product with a padding zero is formed"""
    x, wt = x.numpy().astype(np.float64), wt.numpy().astype(np.float64)
    n, cin, h, w = x.shape
    cout, k = wt.shape[0], wt.shape[2]
    p = k // 2
    y = np.broadcast_to(b.numpy().astype(np.float64).reshape(1, cout, 1, 1), (n, cout, h, w)).copy()
    for ky in range(k):
        for kx in range(k):
            y0, y1 = max(0, p - ky), min(h, h + p - ky)
            x0, x1 = max(0, p - kx), min(w, w + p - kx)
            if y0 >= y1 or x0 >= x1:
                continue
            src = x[:, None, :, y0 + ky - p:y1 + ky - p, x0 + kx - p:x1 + kx - p]
            with np.errstate(invalid="ignore"):
                y[:, :, y0:y1, x0:x1] += (wt[None, :, :, ky, kx, None, None] * src).sum(2)
    return y


def conv_injected_classes(c):
    return () if not c.inj else ((NAN, POS) if c.relu else (NAN, POS, NEG))


# ---- the weight gradients ---------------------------------------------------------------------------------------------------------------
# into: 'gy' or 'x'.  n is chosen for more than 512 pixels: two slabs, so the slab-sum launch sees the values
Wgrad = namedtuple("Wgrad", "tag k n cin cout h w into inj")


def _wgrad():
    cs, i = [], 0
    for k, (n, h, w) in ((1, (15, 5, 7)), (3, (15, 5, 7)), (7, (7, 9, 9))):
        mid = (h // 2, w // 2)
        far = (h // 2, w // 2 + 1)
        cs.append(Wgrad("k%d-gy" % k, k, n, 8, 8, h, w, "gy", _three((0, 0, 0, 0), (1, 2) + mid, (n - 1, 5) + far, i)))
        # +Inf and -Inf in one output channel, in different slabs: its bias gradient is NaN
        cs.append(Wgrad("k%d-gy-overlap" % k, k, n, 8, 8, h, w, "gy", _three((0, 0, h - 1, w - 1), (1, 2) + mid, (n - 1, 2) + far, i + 1)))
        cs.append(Wgrad("k%d-x" % k, k, n, 8, 8, h, w, "x", _three((0, 0, 0, 0), (1, 2, 0, 1), (n - 1, 5, h - 1, w - 2), i)))
        i += 1
    return cs


WGRAD = _wgrad()


def wgrad_operands(c, seed=0):
    """(x [n, cin, h, w], gy [n, cout, h, w]) float32, every value a bf16 value"""
    g = torch.Generator().manual_seed(9100 + seed + c.k)
    x, gy = draw(g, c.n, c.cin, c.h, c.w), draw(g, c.n, c.cout, c.h, c.w)
    inject(gy if c.into == "gy" else x, c.inj)
    return x, gy


def wgrad_taps(x, gy, k):
    """(dW [cout, cin, k, k], dbias [cout]) float64, tap by tap on the zero-padded x: a NaN of gy next to a border meets
    padding zeros and gives NaN there, as in F.conv2d's autograd (and in a kernel that reads zero gaps); an Inf would give
    NaN too where a sum over the map alone gives none, which is why the Infs of gy stay k // 2 inside"""
    x, gy = x.numpy().astype(np.float64), gy.numpy().astype(np.float64)
    n, cin, h, w = x.shape
    cout, p = gy.shape[1], k // 2
    xp = np.zeros((n, cin, h + 2 * p, w + 2 * p))
    xp[:, :, p:p + h, p:p + w] = x
    dw = np.zeros((cout, cin, k, k))
    with np.errstate(invalid="ignore"):
        for ky in range(k):
            for kx in range(k):
                dw[:, :, ky, kx] = (gy[:, :, None] * xp[:, None, :, ky:ky + h, kx:kx + w]).sum((0, 3, 4))
        return dw, gy.sum((0, 2, 3))


def wgrad_torch(x, gy, k):
    """the same from F.conv2d's float64 autograd"""
    wt = torch.zeros(gy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(gy.shape[1], dtype=torch.float64, requires_grad=True)
    dw, db = torch.autograd.grad(F.conv2d(x.double(), wt, b, padding=k // 2), (wt, b), gy.double())
    return dw.numpy(), db.numpy()


# ---- the per-channel kernels: BatchNorm and the depthwise 3x3 ----------------------------------------------------------------------------
# channel: the injected one - first, last, and inside a 4-channel vector; what: the bit pattern, or two of them for neighbouring
# pixels of a row (+Inf beside -Inf: their footprints overlap); into: 'x' or 'gy'
Chan = namedtuple("Chan", "tag channels channel what into")


def _chan(kinds):
    cs = []
    for channels, mid in ((8, 5), (24, 13)):
        for pos, ch in (("first", 0), ("mid", mid), ("last", channels - 1)):
            for into, name, bits in kinds:
                cs.append(Chan("c%d-%s-%s-%s" % (channels, pos, into, name), channels, ch, bits, into))
    return cs


# BatchNorm.  An Inf of gy: dbias has its class in any order; dweight = invstd * (G2 - mdk * G1) is Inf - Inf wherever the
# shifted sums G2 and mdk * G1 agree in sign, and dx meets Inf - Inf in an order the two sides do not share - the header
# pins both next to rtpose_bn_grad, the test holds dbias to torch and dweight to "torch's class or NaN"
BN = _chan((("x", "nan", NAN_BITS[0]), ("x", "pinf", PINF), ("x", "ninf", NINF), ("x", "both", (PINF, NINF)),
            ("gy", "nan", NAN_BITS[1]), ("gy", "pinf", PINF)))
BN_SHAPE = (2, 5, 7)            # 70 pixels: two slabs of 64
BN_AT = (1, 2, 3)               # (n, y, x) of the injected element: not pixel (0, 0, 0), whose value is the shift K of the sums
DW = _chan((("x", "nan", NAN_BITS[1]), ("x", "pinf", PINF), ("x", "both", (PINF, NINF)), ("gy", "nan", NAN_BITS[0]),
            ("gy", "ninf", NINF), ("gy", "both", (NINF, PINF))))
DW_SHAPE = (2, 9, 11)           # 198 / 60 output pixels at stride 1 / 2: four slabs / one
DW_AT_X = (1, 4, 6)             # even coordinates: a stride-2 output's centre tap; interior at both strides
DW_AT_GY = (1, 2, 3)            # interior of the 9 x 11 and of the 5 x 6 gradient map


def chan_operands(c, shape, hw_gy=None, seed=0):
    """(x [n, channels, h, w], gy [n, channels, ho, wo]) without an injection: integers of {-2, -1, 1, 2}; chan_inject puts
    the case's element into one channel of a copy of x or of gy"""
    n, h, w = shape
    ho, wo = hw_gy or (h, w)
    g = torch.Generator().manual_seed(9200 + seed + c.channels)
    x, gy = draw(g, n, c.channels, h, w), draw(g, n, c.channels, ho, wo)
    return x, gy


def chan_inject(c, x, gy, at_x, at_gy):
    x, gy = x.clone(), gy.clone()
    n, yy, xx = at_x if c.into == "x" else at_gy
    what = c.what if isinstance(c.what, tuple) else (c.what,)
    inject(x if c.into == "x" else gy, [((n, c.channel, yy, xx + i), bits) for i, bits in enumerate(what)])
    return x, gy


def chan_classes(c):
    """the classes the injected patterns belong to (two Infs of opposite sign also meet as NaN)"""
    what = c.what if isinstance(c.what, tuple) else (c.what,)
    cls = {NAN if b in NAN_BITS else (POS if b == PINF else NEG) for b in what}
    return tuple(sorted(cls | ({NAN} if len(what) > 1 else set())))


def dw_weights(channels, seed=0):
    g = torch.Generator().manual_seed(9300 + seed + channels)
    return draw(g, channels, 1, 3, 3)


# ---- the two stride-2 stems ---------------------------------------------------------------------------------------------------------------
STEM_SHAPE = (2, 10, 14)        # the image [2, 3, 10, 14]; outputs 5 x 7
STEM_GY = ((0, 1, 0, 0), (1, 20, 2, 3), (1, 7, 3, 4))      # NaN anywhere; the Infs inside the 5 x 7 gradient map


def stem_operands(cout, k, seed=0):
    """(image [n, 3, h, w] of small non-zero integers, filters [cout, 3, k, k], gy [n, cout, h / 2, w / 2] with the three
    injections, bias gradient wanted)"""
    n, h, w = STEM_SHAPE
    g = torch.Generator().manual_seed(9400 + seed + k)
    x, wt, gy = draw(g, n, 3, h, w), draw(g, cout, 3, k, k), draw(g, n, cout, h // 2, w // 2)
    return x, wt, inject(gy, _three(*STEM_GY, seed))


def stem_reference(x, wt, gy, k, need_x):
    """float64 autograd of conv2d(x, wt, stride 2, padding k // 2): (dW, dbias, dx or None) as numpy"""
    x64 = x.double().requires_grad_(need_x)
    w64 = wt.double().requires_grad_(True)
    b64 = torch.zeros(wt.shape[0], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, w64, b64, stride=2, padding=k // 2)
    gs = torch.autograd.grad(y, (w64, b64) + ((x64,) if need_x else ()), gy.double())
    return gs[0].numpy(), gs[1].numpy(), gs[2].numpy() if need_x else None


# ---- fp32 -> bf16 conversions ---------------------------------------------------------------------------------------------------------------
# signalling NaNs, the all-ones mantissa (RNE by integer addition would carry it into the exponent and sign), a negative
# quiet NaN and the largest signalling payload: each must stay a NaN of its sign
NAN_INPUTS = (0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0x7FBFFFFF)


def is_bf16_nan_of_sign(h, f32_bits):
    h = np.asarray(h, dtype=np.uint16)
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0) & ((h >> 15) == (np.uint32(f32_bits) >> 31))


# ---- end to end: a three-conv ReLU chain ---------------------------------------------------------------------------------------------------
CHAIN = ((3, 8, 12), (7, 12, 10), (1, 10, 5))   # (k, cin, cout): the convs of test_train_gpu's small chain, in a row
CHAIN_SHAPE = (2, 6, 5)


def chain_operands(seed=0):
    """(x [2, 8, 6, 5], [(w, b)]): integers; fp32 sums stay below 2^24 (|y1| <= 291, |y2| <= 3.5e5, |y3| <= 7e6)"""
    g = torch.Generator().manual_seed(9500 + seed)
    n, h, w = CHAIN_SHAPE
    x = draw(g, n, CHAIN[0][1], h, w)
    layers = [(draw(g, co, ci, k, k), torch.randint(-3, 4, (co,), generator=g).float()) for k, ci, co in CHAIN]
    return x, layers


def chain_reference(x, layers):
    """the torch modules in float64: conv + ReLU, conv + ReLU, conv"""
    mods = []
    for i, (wt, b) in enumerate(layers):
        m = torch.nn.Conv2d(wt.shape[1], wt.shape[0], wt.shape[2], 1, wt.shape[2] // 2).double()
        with torch.no_grad():
            m.weight.copy_(wt.double())
            m.bias.copy_(b.double())
        mods += [m, torch.nn.ReLU()] if i + 1 < len(layers) else [m]
    with torch.no_grad():
        return torch.nn.Sequential(*mods)(x.double()).numpy()
