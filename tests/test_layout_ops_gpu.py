"""Every entry point of csrc/layout_ops.hip against the host restatement in tests/layout_restate.py.

Method, the same for every case: the source buffer is built on the host with the addressing formula of the
header (§1) and uploaded; the DESTINATION is filled with a sentinel bit pattern (a NaN no case produces), the
call is made, the raw buffer comes back with .cpu() and is indexed on the host.  The words the operation owns
are compared with the reference - bit for bit, or within a bound derived from the arithmetic (never measured) -
and every other word (lead, gaps, tail slack, the other channels of each pixel) must still be the sentinel.
No layout kernel is used to check another, except where the subject is the agreement of two entry points.

Stencil inputs are signed and every stencil case also runs an all-negative tensor: a window or tap that read
a gap (value 0) instead of being clipped would change the result.  The max-pool inputs hold no NaN and no
+0 / -0 pair: fmaxf and nn.MaxPool2d differ there and the network never produces either.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import layout_restate as lr

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC12345          # a quiet NaN with a payload: no kernel here produces it
SENT16 = 0x7FA5              # a bf16 NaN
U24 = 2.0 ** -24
INVAL = -1

# ---- geometry ------------------------------------------------------------------------------------------
GEOS = [(1, 1, 1), (1, 3, 3), (3, 7, 5), (2, 23, 30), (3, 46, 46), (1, 92, 92)]
CROSS = {(3, 7, 5), (2, 23, 30)}            # these meet every layout variant, the others take turns
# sp/so/se: pad, choff, channels behind the slice of the SOURCE; dp/do/de: of the DESTINATION (dp 0 = dense)
VARIANTS = {
    "tight": dict(sp=1, so=0, se=0, dp=0, do=0, de=0),
    "offset": dict(sp=3, so=8, se=8, dp=1, do=16, de=24),
    "mixed": dict(sp=1, so=16, se=0, dp=3, do=0, de=8),
}


def _cid(g, c, v):
    return "%dx%dx%dx%s-%s" % (g + ("of".join(str(k) for k in c) if isinstance(c, tuple) else c, v))


def cases(cs_small, cs_big, min_hw=1, extra=()):
    out, i = [], 0
    for c in cs_small:
        for g in GEOS + list(extra):
            if g[1] < min_hw or g[2] < min_hw:
                continue
            for v in (VARIANTS if g in CROSS else [list(VARIANTS)[i % 3]]):
                out.append(pytest.param(g, c, v, id=_cid(g, c, v)))
            i += 1
    for c in cs_big:
        for g in ((3, 7, 5), (1, 46, 46)):
            v = list(VARIANTS)[i % 3]
            out.append(pytest.param(g, c, v, id=_cid(g, c, v)))
            i += 1
    return out


def lay(c, h, w, pad, off, extra, mult=1):
    cs = (off + c + extra) * mult
    return lr.padded(cs, h, w, pad, off * mult) if pad else lr.dense(cs, h, w, off * mult)


def src_lay(v, c, h, w, mult=1):
    v = VARIANTS[v]
    return lay(c, h, w, v["sp"], v["so"], v["se"], mult)


def dst_lay(v, c, h, w, mult=1):
    v = VARIANTS[v]
    return lay(c, h, w, v["dp"], v["do"], v["de"], mult)


# ---- plumbing ------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, capi, dev):
        self.capi, self.lib, self.dev = capi, capi.lib, dev

    @property
    def s(self):
        return self.capi.current_stream()

    def L(self, l):
        return C.byref(self.capi.Layout(*l))

    def up(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        return torch.from_numpy(a).to(self.dev)

    def sent32(self, words):
        return torch.full((int(words),), SENT32, dtype=torch.int32, device=self.dev)

    def sent16(self, words):
        return torch.full((int(words),), SENT16, dtype=torch.int16, device=self.dev)

    def ok(self, rc, what=""):
        self.capi.check(rc, what)

    def inval(self, rc, what=""):
        assert rc == INVAL, "%s: rc %d, expected RTPOSE_E_INVAL" % (what, rc)
        assert self.capi.last_error() != "", what


@pytest.fixture
def K(capi, cuda):
    return Ctx(capi, cuda)


def words(l, n):
    return lr.pixels(l, n) * l.cstride


def down32(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def down16(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def nhwc(x):
    x = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32_src(K, l, n, x, noise_seed=None):
    """fp32 source buffer with x [n,c,h,w] in the slice of l; everything else zero (stencil sources: the gaps
    are the padding) or, with noise_seed, random finite values (a wrong read then shows)."""
    w = words(l, n)
    if noise_seed is None:
        buf = np.zeros(w, dtype=np.float32)
    else:
        buf = np.random.default_rng(noise_seed).standard_normal(w).astype(np.float32) * 3 + 11
    lr.scatter(buf, l, np.asarray(x, dtype=np.float32))
    return K.up(buf)


def b16_src(K, l, n, xbits, noise_seed=None):
    w = words(l, n)
    if noise_seed is None:
        buf = np.zeros(w, dtype=np.uint16)
    else:
        buf = np.random.default_rng(noise_seed).integers(0, 0x10000, size=w).astype(np.uint16)
    lr.scatter(buf, l, xbits)
    return K.up(buf)


def check_bits(got, idx, want, sent, what=""):
    """got: unsigned view of the whole buffer; idx: offsets of the owned words; want: their bits."""
    g = got[idx]
    want = np.asarray(want)
    assert g.shape == want.shape, (g.shape, want.shape)
    bad = np.flatnonzero(g.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d owned words differ; first at %s: got %#x, want %#x" % (
        what, bad.size, g.size, np.unravel_index(bad[0], g.shape), g.ravel()[bad[0]], want.ravel()[bad[0]])
    assert lr.untouched(got, idx, sent), "%s: a word outside the owned set was written" % what


def check_close(got, idx, ref, bound, what=""):
    """|got - ref| <= bound element-wise (float64 arrays in the order of idx), and nothing else written."""
    g = got[idx].view(np.float32).astype(np.float64)
    ref, bound = np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    err = np.abs(g - ref)
    assert np.all(np.isfinite(g)), what
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s: worst |got - ref| / bound = %.3f" % (what, worst))
    assert np.all(err <= bound), "%s: %d elements outside the bound, worst ratio %.3f" % (
        what, int(np.sum(err > bound)), worst)
    assert lr.untouched(got, idx, SENT32), "%s: a word outside the owned set was written" % what


def check_bracket(got, idx, ref, e, what=""):
    """bf16 output of an fp32 sum: bf16_rne(ref - E) <= got <= bf16_rne(ref + E) as ordered values (rounding is
    monotone, the fp32 sum lies in [ref - E, ref + E]).  Every element is tested."""
    g = got[idx]
    lo32, hi32 = lr.f32_round_interval(np.asarray(ref, dtype=np.float64), np.asarray(e, dtype=np.float64))
    lo, hi, k = lr.bf16_key(lr.bf16_rne(lo32)), lr.bf16_key(lr.bf16_rne(hi32)), lr.bf16_key(g)
    assert g.shape == lo.shape
    assert not np.any((g & 0x7FFF) > 0x7F80), "%s: NaN in the output" % what
    inside = (lo <= k) & (k <= hi)
    print("%s: %.2f %% of the brackets are a single value" % (what, 100.0 * float(np.mean(lo == hi))))
    assert np.all(inside), "%s: %d of %d elements outside their bracket" % (what, int(np.sum(~inside)), g.size)
    assert lr.untouched(got, idx, SENT16), "%s: a word outside the owned set was written" % what


def signed_and_negative(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    return [("signed", x), ("negative", -x.abs() - 0.25)]


def special_f32(shape, seed, finite_below=None):
    """Random values with the patterns a bf16 conversion goes wrong at sprinkled in: exact ties (odd and even
    upper halves), values that round up into the next binade, subnormals, +-0, the largest finite value, +-inf."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * np.exp(rng.uniform(-8, 8, size=shape))).astype(np.float32)
    u = x.view(np.uint32).reshape(-1)
    sp = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F7FFFFF, 0xBF7FFFFF, 0x3FFF8000, 0x3F7F8000,
                   0x3F7F7FFF, 0x3F808001, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                   0x00008000, 0x00018000, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7F7F8000,
                   0x42FE8000, 0x42FF8000], dtype=np.uint32)
    if finite_below is not None:
        f = sp.view(np.float32)
        sp = sp[np.isfinite(f) & (np.abs(f) < finite_below)]
    k = min(u.size, 4 * sp.size)
    pos = rng.choice(u.size, size=k, replace=False)
    u[pos] = sp[np.arange(k) % sp.size]
    tie = rng.choice(u.size, size=max(1, u.size // 7), replace=False)       # many more random exact ties
    u[tie] = (u[tie] & 0xFFFF0000) | 0x8000
    u[(u & 0x7FFFFFFF) > 0x7F800000] = 0x3F800000                           # no NaN
    x = u.view(np.float32).reshape(shape)
    if finite_below is not None:
        x = np.where(np.isfinite(x) & (np.abs(x) < finite_below), x, np.float32(1.5)).astype(np.float32)
    return x


def test_layout_pixels_is_the_restated_formula(K):
    for l, n in ((lr.padded(24, 23, 30, 1), 2), (lr.dense(8, 4, 4), 0), (lr.padded(64, 92, 92, 3, 8), 3)):
        assert K.lib.rtpose_layout_pixels(K.L(l), n, 5, 5) == lr.pixels(l, n)
    assert b"gfx950" in K.lib.rtpose_version() and isinstance(K.lib.rtpose_last_error(), bytes)


# ---- NCHW <-> layout, copies ---------------------------------------------------------------------------
@pytest.mark.parametrize("geo, cc, v", cases([(3, 8), (19, 19), (38, 40), (24, 24)], [(116, 116), (232, 232)]))
def test_nchw_to_layout(K, geo, cc, v):
    (n, h, w), (c, cpad) = geo, cc
    x = special_f32((n, c, h, w), 1)
    l = dst_lay(v, cpad, h, w)
    dst = K.sent32(words(l, n))
    xd = K.up(x)
    K.ok(K.lib.rtpose_nchw_to_layout(K.capi.ptr(xd), K.capi.ptr(dst), K.L(l), c, cpad, n, h, w, K.s))
    want = np.zeros((n, h, w, cpad), dtype=np.uint32)                      # channels [C, cpad) are written as +0.0
    want[..., :c] = bits32(nhwc(x))
    check_bits(down32(dst), lr.index(l, n, h, w, cpad), want, SENT32, "nchw_to_layout")


@pytest.mark.parametrize("geo, c, v", cases([3, 19, 38, 24], [57, 232]))
def test_layout_to_nchw(K, geo, c, v):
    n, h, w = geo
    x = special_f32((n, c, h, w), 2)
    l = src_lay(v, c, h, w)
    src = f32_src(K, l, n, x, noise_seed=5)
    dst = K.sent32(x.size + 64)
    K.ok(K.lib.rtpose_layout_to_nchw(K.capi.ptr(src), K.L(l), K.capi.ptr(dst), c, n, h, w, K.s))
    check_bits(down32(dst), np.arange(x.size).reshape(x.shape), bits32(x), SENT32, "layout_to_nchw")


def _copy_layouts(v, c, h, w):
    if v == "slice166":     # the 19 heat-map channels at channel 166 of the 185-channel concat pixel
        return lr.padded(185, h, w, 3, 166), lr.padded(64, h, w, 1, 41)
    return src_lay(v, c, h, w), dst_lay(v, c, h, w)


@pytest.mark.parametrize("geo, c, v", cases([4, 24, 19, 38, 57], [116, 232]) + [
    pytest.param((3, 7, 5), 19, "slice166", id="3x7x5x19-slice166"),
    pytest.param((2, 46, 46), 19, "slice166", id="2x46x46x19-slice166")])
def test_layout_copy(K, geo, c, v):
    """C % 4 == 0 with aligned slices takes the float4 kernel, everything else the scalar one."""
    n, h, w = geo
    x = special_f32((n, c, h, w), 3)
    ls, ld = _copy_layouts(v, c, h, w)
    src = f32_src(K, ls, n, x, noise_seed=6)
    dst = K.sent32(words(ld, n))
    K.ok(K.lib.rtpose_layout_copy(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, n, h, w, K.s))
    check_bits(down32(dst), lr.index(ld, n, h, w, c), bits32(nhwc(x)), SENT32, "layout_copy")


def _cmaps(c, base):
    half = c // 2
    shuffle = base + np.array([(i % half) * 2 + i // half if i < 2 * half else i for i in range(c)])   # channel_shuffle(2)
    two_runs = np.array([i if i < half else i + 5 for i in range(c)]) + base
    return {"shuffle": shuffle.astype(np.int32), "tworuns": two_runs.astype(np.int32)}


@pytest.mark.parametrize("geo", [(1, 1, 1), (3, 7, 5), (2, 23, 30), (1, 46, 46)])
@pytest.mark.parametrize("path", ["aligned58of64", "unaligned58", "aligned24"])
@pytest.mark.parametrize("mapname", ["shuffle", "tworuns"])
def test_layout_copy_cmap(K, geo, path, mapname):
    """Both kernels: the 16-byte one (source slice aligned, padding channels behind it readable) and the scalar one.
    cmap holds ABSOLUTE destination channels: a non-zero destination choff must not shift them."""
    n, h, w = geo
    c = 24 if path == "aligned24" else 58
    ls = {"aligned58of64": lr.padded(64, h, w, 1, 0), "unaligned58": lr.padded(61, h, w, 1, 3),
          "aligned24": lr.padded(40, h, w, 3, 8)}[path]
    ld = lr.padded(96, h, w, 1, 12)
    cmap = _cmaps(c, 20)[mapname]
    assert cmap.max() < ld.cstride and np.unique(cmap).size == c
    x = special_f32((n, c, h, w), 4)
    src = f32_src(K, ls, n, x, noise_seed=7)
    dst = K.sent32(words(ld, n))
    cm = K.up(cmap)
    K.ok(K.lib.rtpose_layout_copy_cmap(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, K.capi.ptr(cm), n, h, w, K.s))
    check_bits(down32(dst), lr.index_map(ld, n, h, w, cmap), bits32(nhwc(x)), SENT32, "layout_copy_cmap")


@pytest.mark.parametrize("geo", [(1, 1, 1), (3, 7, 5), (2, 23, 30), (1, 46, 46)])
@pytest.mark.parametrize("c, ls_args", [(58, (64, 0)), (20, (40, 8)), (120, (240, 120)), (7, (16, 8))])
@pytest.mark.parametrize("mapname", ["shuffle", "tworuns"])
def test_layout_copy_cmap_bf16(K, geo, c, ls_args, mapname):
    n, h, w = geo
    ls = lr.padded(ls_args[0], h, w, 1, ls_args[1])
    ld = lr.padded(256, h, w, 3, 24)
    cmap = _cmaps(c, 9)[mapname]
    assert cmap.max() < ld.cstride and np.unique(cmap).size == c
    xb = np.random.default_rng(5).integers(0, 0x10000, size=(n, c, h, w)).astype(np.uint16)
    src = b16_src(K, ls, n, xb, noise_seed=8)
    dst = K.sent16(words(ld, n))
    cm = K.up(cmap)
    K.ok(K.lib.rtpose_layout_copy_cmap_bf16(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, K.capi.ptr(cm), n, h, w, K.s))
    check_bits(down16(dst), lr.index_map(ld, n, h, w, cmap), nhwc(xb), SENT16, "layout_copy_cmap_bf16")


# ---- bf16 and split conversions ------------------------------------------------------------------------
@pytest.mark.parametrize("geo, c, v", cases([3, 19, 24], [57, 232]))
def test_layout_bf16_to_f32(K, geo, c, v):
    n, h, w = geo
    xb = np.random.default_rng(6).integers(0, 0x10000, size=(n, c, h, w)).astype(np.uint16)
    ls, ld = src_lay(v, c, h, w), dst_lay(v, c, h, w)
    src = b16_src(K, ls, n, xb, noise_seed=9)
    dst = K.sent32(words(ld, n))
    K.ok(K.lib.rtpose_layout_bf16_to_f32(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, n, h, w, K.s))
    check_bits(down32(dst), lr.index(ld, n, h, w, c), nhwc(xb).astype(np.uint32) << 16, SENT32, "layout_bf16_to_f32")


BF_C = [(3, 8), (8, 8), (19, 24), (24, 24)]
BF_C_BIG = [(120, 120), (232, 232)]


@pytest.mark.parametrize("geo, cc, v", cases(BF_C, BF_C_BIG))
@pytest.mark.parametrize("entry", ["nchw_to_layout_bf16", "layout_f32_to_bf16"])
def test_to_bf16_rounds_to_nearest_even(K, entry, geo, cc, v):
    (n, h, w), (c, cpad) = geo, cc
    x = special_f32((n, c, h, w), 7)
    ld = dst_lay(v, cpad, h, w)
    dst = K.sent16(words(ld, n))
    if entry == "nchw_to_layout_bf16":
        xd = K.up(x)
        K.ok(K.lib.rtpose_nchw_to_layout_bf16(K.capi.ptr(xd), K.capi.ptr(dst), K.L(ld), c, cpad, n, h, w, K.s))
    else:
        ls = src_lay(v, c, h, w)
        src = f32_src(K, ls, n, x, noise_seed=10)
        K.ok(K.lib.rtpose_layout_f32_to_bf16(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, cpad, n, h, w, K.s))
    want = np.zeros((n, h, w, cpad), dtype=np.uint16)
    want[..., :c] = lr.bf16_rne(nhwc(x))
    check_bits(down16(dst), lr.index(ld, n, h, w, cpad), want, SENT16, entry)


@pytest.mark.parametrize("geo, cc, v", cases(BF_C, BF_C_BIG))
@pytest.mark.parametrize("entry", ["nchw_to_layout_split", "layout_f32_to_split"])
def test_to_split(K, entry, geo, cc, v):
    (n, h, w), (c, cpad) = geo, cc
    x = special_f32((n, c, h, w), 8, finite_below=1e30)
    ld = dst_lay(v, cpad, h, w, mult=2)                                     # split layouts count elements: 2 per channel
    dst = K.sent16(words(ld, n))
    if entry == "nchw_to_layout_split":
        xd = K.up(x)
        K.ok(K.lib.rtpose_nchw_to_layout_split(K.capi.ptr(xd), K.capi.ptr(dst), K.L(ld), c, cpad, n, h, w, K.s))
    else:
        ls = src_lay(v, c, h, w)
        src = f32_src(K, ls, n, x, noise_seed=11)
        K.ok(K.lib.rtpose_layout_f32_to_split(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, cpad, n, h, w, K.s))
    hi, lo = lr.split(nhwc(x))
    wh, wl = (np.zeros((n, h, w, cpad), dtype=np.uint16) for _ in range(2))
    wh[..., :c], wl[..., :c] = hi, lo
    got = down16(dst)
    ih, il = lr.split_index(ld, n, h, w, cpad)
    check_bits(got, np.stack([ih, il]), np.stack([wh, wl]), SENT16, entry)


@pytest.mark.parametrize("geo", [(1, 1, 1), (3, 7, 5), (2, 23, 30), (2, 46, 46)])
@pytest.mark.parametrize("c, cpix, choff_ch", [(8, 8, 0), (19, 192, 166), (38, 192, 128), (24, 40, 8), (5, 16, 3), (232, 232, 0)])
def test_layout_split_to_f32(K, geo, c, cpix, choff_ch):
    """The read side takes a choff inside an 8-channel group (the 19 heat-map channels start at channel 166 of
    the concat buffer); the value is float32(hi) + float32(lo), one correctly rounded fp32 add."""
    n, h, w = geo
    x = special_f32((n, c, h, w), 9, finite_below=1e30)
    hi, lo = lr.split(x)
    ls = lr.Lay(2 * cpix, 2 * choff_ch, w + 1, h + 1, w + 2)
    ld = lr.padded(c + 11, h, w, 3, 7)
    sb = np.random.default_rng(12).integers(0, 0x10000, size=words(ls, n)).astype(np.uint16)
    lr.scatter_split(sb, ls, hi, lo)
    src, dst = K.up(sb), K.sent32(words(ld, n))
    K.ok(K.lib.rtpose_layout_split_to_f32(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, n, h, w, K.s))
    want = lr.bf16_to_f32(nhwc(hi)) + lr.bf16_to_f32(nhwc(lo))
    check_bits(down32(dst), lr.index(ld, n, h, w, c), bits32(want), SENT32, "layout_split_to_f32")


# ---- max-pools -----------------------------------------------------------------------------------------
POOL_EXTRA = ((2, 6, 8), (2, 9, 4), (1, 4, 7), (1, 2, 2))          # even / odd H and W in every combination


@pytest.mark.parametrize("geo, c, v", cases([4, 24], [116, 232], min_hw=2, extra=POOL_EXTRA)
                         + [pytest.param((2, 92, 92), 24, "offset", id="plan-2x92x92x24")])
def test_maxpool2x2(K, geo, c, v):
    n, h, w = geo
    ho, wo = h // 2, w // 2
    ls, ld = src_lay(v, c, h, w), dst_lay(v, c, max(ho, 1), max(wo, 1))
    for name, x in signed_and_negative((n, c, h, w), 11):
        src = f32_src(K, ls, n, x.numpy())
        dst = K.sent32(words(ld, n))
        K.ok(K.lib.rtpose_maxpool2x2(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, n, h, w, K.s))
        want = lr.maxpool2x2(x).to(torch.float32)
        check_bits(down32(dst), lr.index(ld, n, ho, wo, c), bits32(nhwc(want)), SENT32, "maxpool2x2 " + name)


@pytest.mark.parametrize("geo, c, v", cases([4, 24], [116, 232], min_hw=3, extra=((2, 6, 8), (2, 9, 4), (1, 4, 7)))
                         + [pytest.param((2, 92, 92), 24, "offset", id="plan-2x92x92x24")])
def test_maxpool3x3s2_ceil(K, geo, c, v):
    n, h, w = geo
    ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    ls, ld = src_lay(v, c, h, w), dst_lay(v, c, ho, wo)
    for name, x in signed_and_negative((n, c, h, w), 12):
        src = f32_src(K, ls, n, x.numpy())
        dst = K.sent32(words(ld, n))
        K.ok(K.lib.rtpose_maxpool3x3s2_ceil(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, n, h, w, K.s))
        want = lr.maxpool3x3s2_ceil(x)
        assert want.shape == (n, c, ho, wo)
        check_bits(down32(dst), lr.index(ld, n, ho, wo, c), bits32(nhwc(want.to(torch.float32))), SENT32,
                   "maxpool3x3s2_ceil " + name)


@pytest.mark.parametrize("geo, c, v", cases([8, 24], [120, 232], min_hw=3, extra=((2, 6, 8), (2, 9, 4), (1, 4, 7)))
                         + [pytest.param((2, 92, 92), 24, "offset", id="plan-2x92x92x24")])
def test_maxpool3x3s2_ceil_bf16(K, geo, c, v):
    n, h, w = geo
    ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    ls, ld = src_lay(v, c, h, w), dst_lay(v, c, ho, wo)
    for name, x in signed_and_negative((n, c, h, w), 13):
        xb = lr.bf16_rne(x.numpy())
        src = b16_src(K, ls, n, xb)
        dst = K.sent16(words(ld, n))
        K.ok(K.lib.rtpose_maxpool3x3s2_ceil_bf16(K.capi.ptr(src), K.L(ls), K.capi.ptr(dst), K.L(ld), c, n, h, w, K.s))
        want = lr.maxpool3x3s2_ceil(lr.bf16_to_f32(xb)).to(torch.float32).numpy()      # the bf16 store of a bf16 value is the identity
        check_bits(down16(dst), lr.index(ld, n, ho, wo, c), lr.bf16_rne(nhwc(want)), SENT16, "maxpool3x3s2_ceil_bf16 " + name)


# ---- depthwise 3x3 -------------------------------------------------------------------------------------
DW_EXTRA = ((2, 4, 8), (2, 4, 9), (1, 5, 10), (2, 3, 11), (1, 2, 4), (1, 1, 6))      # W % 4 = 0, 1, 2, 3 (4 pixels per thread)
DW_PLAN = [pytest.param((2, 46, 46), 232, "offset", 1, id="plan-2x46x46x232-s1"),
           pytest.param((2, 92, 92), "C116", "mixed", 2, id="plan-2x92x92x116-s2"),
           pytest.param((2, 23, 30), 24, "tight", 1, id="building-blocks-2x24x23x30-s1"),
           pytest.param((2, 23, 30), 24, "tight", 2, id="building-blocks-2x24x23x30-s2")]


def _dw_cases(cs_small, cs_big):
    out = []
    for p in cases(cs_small, cs_big, extra=DW_EXTRA):
        for stride in (1, 2):
            out.append(pytest.param(*p.values, stride, id="%s-s%d" % (p.id, stride)))
    return out + DW_PLAN


def _dw_weights(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(c, 3, 3, generator=g), torch.randn(c, generator=g)


@pytest.mark.parametrize("geo, c, v, stride", _dw_cases([4, 24], [116, 232]))
def test_dwconv3x3(K, geo, c, v, stride):
    """|got - ref64| <= 10 * 2^-24 * S: the bias and nine products, each product and each add rounded once."""
    n, h, w = geo
    c = 116 if c == "C116" else c
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ls, ld = src_lay(v, c, h, w), dst_lay(v, c, ho, wo)
    wt, b = _dw_weights(c, 14)
    wd, bd = K.up(wt.view(c, 9).t().contiguous().numpy()), K.up(b.numpy())             # [9][C], tap-major
    for name, x in signed_and_negative((n, c, h, w), 15):
        src = f32_src(K, ls, n, x.numpy())
        dst = K.sent32(words(ld, n))
        K.ok(K.lib.rtpose_dwconv3x3(K.capi.ptr(src), K.L(ls), K.capi.ptr(wd), K.capi.ptr(bd), K.capi.ptr(dst), K.L(ld),
                                    c, n, h, w, stride, K.s))
        ref, s = lr.dwconv3x3(x, wt, b, stride)
        check_close(down32(dst), lr.index(ld, n, ho, wo, c), nhwc(ref), 10 * U24 * nhwc(s), "dwconv3x3 s%d %s" % (stride, name))


@pytest.mark.parametrize("geo, c, v, stride", _dw_cases([8, 24], [120, 232]))
def test_dwconv3x3_bf16(K, geo, c, v, stride):
    """bf16 activations, fp32 taps and sums, bf16 store: the bracket of the fp32 bound, every element."""
    n, h, w = geo
    c = 120 if c == "C116" else c          # the bf16 form takes C % 8 == 0: the nearest size
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ls, ld = src_lay(v, c, h, w), dst_lay(v, c, ho, wo)
    wt, b = _dw_weights(c, 16)
    wd, bd = K.up(wt.view(c, 9).t().contiguous().numpy()), K.up(b.numpy())
    for name, x in signed_and_negative((n, c, h, w), 17):
        xb = lr.bf16_rne(x.numpy())
        src = b16_src(K, ls, n, xb)
        dst = K.sent16(words(ld, n))
        K.ok(K.lib.rtpose_dwconv3x3_bf16(K.capi.ptr(src), K.L(ls), K.capi.ptr(wd), K.capi.ptr(bd), K.capi.ptr(dst),
                                         K.L(ld), c, n, h, w, stride, K.s))
        ref, s = lr.dwconv3x3(lr.bf16_to_f32(xb), wt, b, stride)
        check_bracket(down16(dst), lr.index(ld, n, ho, wo, c), nhwc(ref), 10 * U24 * nhwc(s),
                      "dwconv3x3_bf16 s%d %s" % (stride, name))


# ---- affine, stem, axpby -------------------------------------------------------------------------------
@pytest.mark.parametrize("geo, cc, v", cases([(3, 8), (24, 24)], [(116, 116)]))
def test_nchw_to_layout_affine(K, geo, cc, v):
    """with scale: two roundings (or one, fused): |got - ref64| <= 2^-23 (|x s| + |t|); without: bit-identical."""
    (n, h, w), (c, cpad) = geo, cc
    g = torch.Generator().manual_seed(18)
    x = torch.randn(n, c, h, w, generator=g)
    sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 3
    l = dst_lay(v, cpad, h, w)
    xd, scd, shd = K.up(x.numpy()), K.up(sc.numpy()), K.up(sh.numpy())
    idx = lr.index(l, n, h, w, cpad)
    dst = K.sent32(words(l, n))
    K.ok(K.lib.rtpose_nchw_to_layout_affine(K.capi.ptr(xd), K.capi.ptr(dst), K.L(l), c, cpad, n, h, w, K.capi.ptr(scd),
                                            K.capi.ptr(shd), K.s))
    ref, s = lr.affine(x, sc, sh)
    r, bd = np.zeros((n, h, w, cpad)), np.zeros((n, h, w, cpad))
    r[..., :c], bd[..., :c] = nhwc(ref), 2 * U24 * nhwc(s)
    got = down32(dst)
    check_close(got, idx, r, bd, "nchw_to_layout_affine")
    assert np.all(got[idx][..., c:] == 0), "padding channels must be +0.0"
    dst = K.sent32(words(l, n))
    K.ok(K.lib.rtpose_nchw_to_layout_affine(K.capi.ptr(xd), K.capi.ptr(dst), K.L(l), c, cpad, n, h, w, None, None, K.s))
    want = np.zeros((n, h, w, cpad), dtype=np.uint32)
    want[..., :c] = bits32(nhwc(x))
    check_bits(down32(dst), idx, want, SENT32, "nchw_to_layout_affine without scale")


STEM_GEOS = [(1, 1, 1), (1, 3, 3), (3, 7, 5), (2, 23, 30), (3, 46, 46), (1, 92, 92), (2, 6, 8), (2, 368, 368)]


def _stem_params(seed, big_shift):
    g = torch.Generator().manual_seed(seed)
    sc = torch.rand(3, generator=g) + 0.5
    sh = torch.randn(3, generator=g) + (40.0 if big_shift else 0.0)      # large against the data: an affine applied to the padding shows
    w = torch.randn(24, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(24, generator=g)
    wp = torch.zeros(3, 3, 8, 24)
    wp[:, :, :3, :] = w.permute(2, 3, 1, 0)                                # packed [ky][kx][cin_pad 8][cout]
    return sc, sh, w, b, wp.contiguous()


@pytest.mark.parametrize("geo", STEM_GEOS[:-1])
@pytest.mark.parametrize("v", list(VARIANTS))
def test_stem_conv3x3_s2(K, geo, v):
    """Layout input (3 real of 8 channels; the affine ran before): n = 30 of the stem bound with S = |b| + sum |w||x|."""
    n, h, w = geo
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    _, _, wt, b, wp = _stem_params(19, False)
    ls, ld = src_lay(v, 8, h, w), dst_lay(v, 24, ho, wo)
    wd, bd = K.up(wp.numpy()), K.up(b.numpy())
    for relu in (1, 0):
        for name, x in signed_and_negative((n, 3, h, w), 20 + relu):
            x8 = torch.zeros(n, 8, h, w)
            x8[:, :3] = x
            src = f32_src(K, ls, n, x8.numpy())
            dst = K.sent32(words(ld, n))
            K.ok(K.lib.rtpose_stem_conv3x3_s2(K.capi.ptr(src), K.L(ls), K.capi.ptr(wd), K.capi.ptr(bd), K.capi.ptr(dst),
                                              K.L(ld), 8, 24, n, h, w, relu, K.s))
            ref, s = lr.stem_conv3x3_s2(x, None, None, wt, b, bool(relu))
            check_close(down32(dst), lr.index(ld, n, ho, wo, 24), nhwc(ref), 30 * U24 * nhwc(s),
                        "stem_conv3x3_s2 relu%d %s" % (relu, name))


@pytest.mark.parametrize("geo", STEM_GEOS)
@pytest.mark.parametrize("entry", ["nchw", "nchw_ex", "nchw_ex_bf16"])
@pytest.mark.parametrize("with_affine", [True, False])
def test_stem_conv3x3_s2_nchw(K, geo, entry, with_affine):
    """Image -> affine -> zero padding -> conv 3x3 s2 p1 -> ReLU: |got - ref64| <= 30 * 2^-24 * S with
    S = |b| + sum |w| (|x s| + |t|); out-of-image taps contribute exactly 0 AFTER the affine (shift = 40)."""
    n, h, w = geo
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    sc, sh, wt, b, wp = _stem_params(22, True)
    bf = entry.endswith("bf16")
    v = ["tight", "offset", "mixed"][(h + len(entry)) % 3]
    ld = dst_lay(v, 24, ho, wo)
    wd, bd, scd, shd = K.up(wp.numpy()), K.up(b.numpy()), K.up(sc.numpy()), K.up(sh.numpy())
    p = K.capi.ptr
    for relu in ((1,) if h >= 92 else (1, 0)):
        for name, x in signed_and_negative((n, 3, h, w), 23)[:1 if h >= 368 else 2]:
            xd = K.up(x.numpy())
            dst = K.sent16(words(ld, n)) if bf else K.sent32(words(ld, n))
            a = (p(scd), p(shd)) if with_affine else (None, None)
            if entry == "nchw":
                K.ok(K.lib.rtpose_stem_conv3x3_s2_nchw(p(xd), a[0], a[1], p(wd), p(bd), p(dst), K.L(ld), 24, n, h, w, relu, K.s))
            else:
                K.ok(K.lib.rtpose_stem_conv3x3_s2_nchw_ex(p(xd), a[0], a[1], p(wd), p(bd), p(dst), K.L(ld), 24, n, h, w, relu,
                                                          int(bf), K.s))
            ref, s = lr.stem_conv3x3_s2(x, sc if with_affine else None, sh if with_affine else None, wt, b, bool(relu))
            what = "stem_conv3x3_s2_%s affine%d relu%d %s" % (entry, with_affine, relu, name)
            idx = lr.index(ld, n, ho, wo, 24)
            if bf:
                check_bracket(down16(dst), idx, nhwc(ref), 30 * U24 * nhwc(s), what)
            else:
                check_close(down32(dst), idx, nhwc(ref), 30 * U24 * nhwc(s), what)


@pytest.mark.parametrize("geo, c, v", cases([4, 19, 57], [232]))
def test_layout_axpby(K, geo, c, v):
    """dst = alpha * dst + beta * src: two products and an add, |got - ref64| <= 3 * 2^-24 * S."""
    n, h, w = geo
    g = torch.Generator().manual_seed(24)
    d0, sr = torch.randn(n, c, h, w, generator=g), torch.randn(n, h, w, c, generator=g)
    l = dst_lay(v, c, h, w)
    buf = np.full(words(l, n), SENT32, dtype=np.uint32)
    idx = lr.index(l, n, h, w, c)
    buf[idx] = bits32(nhwc(d0))
    dst, src = K.up(buf), K.up(sr.numpy())
    alpha, beta = 0.75, -1.3
    K.ok(K.lib.rtpose_layout_axpby(K.capi.ptr(dst), K.L(l), K.capi.ptr(src), c, n, h, w, alpha, beta, K.s))
    a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
    ref, s = lr.axpby(torch.from_numpy(nhwc(d0)), sr, a32, b32)
    check_close(down32(dst), idx, ref.numpy(), 3 * U24 * s.numpy(), "layout_axpby")


# ---- uint8 resize-and-normalise ------------------------------------------------------------------------
def _cv_round(v):
    return int(np.rint(v))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h0, w0, scale", [(37, 53, 0.73), (29, 31, 1.37), (64, 48, 0.61)])
def test_preprocess_flip_is_the_mirror_of_the_valid_columns(K, mode, h0, w0, scale):
    """flip = 1 == the x-mirror inside the first wr columns of flip = 0, bit for bit; the padding stays on the right."""
    img = np.random.default_rng(h0).integers(0, 256, (h0, w0, 3), dtype=np.uint8)
    hr, wr = _cv_round(h0 * scale), _cv_round(w0 * scale)
    hn, wn = (hr + 7) // 8 * 8 + 8, (wr + 7) // 8 * 8 + 8
    l = lr.padded(16, hn, wn, 1, 4)
    imd = K.up(img)
    p = K.capi.ptr
    idx = lr.index(l, 3, hn, wn, 8)[1:2]                                  # image slot 1 of 3
    out = []
    for flip in (0, 1, None):
        dst = K.sent32(words(l, 3))
        if flip is None:
            K.ok(K.lib.rtpose_preprocess_u8(p(imd), h0, w0, scale, mode, p(dst), K.L(l), 1, hn, wn, hr, wr, K.s))
        else:
            K.ok(K.lib.rtpose_preprocess_u8_flip(p(imd), h0, w0, scale, mode, p(dst), K.L(l), 1, hn, wn, hr, wr, flip, K.s))
        got = down32(dst)
        assert lr.untouched(got, idx, SENT32)
        out.append(got[idx][0])                                           # [hn, wn, 8]
    plain, flipped, noflag = out
    assert np.array_equal(plain, noflag)
    assert np.array_equal(flipped[:, :wr], plain[:, :wr][:, ::-1])
    assert np.array_equal(flipped[:, wr:], plain[:, wr:])
    assert np.all(plain[..., 3:] == 0)                                    # channels 3..7 of NHWC8 are +0.0
    pad = plain[hr:, :, :3].view(np.float32)
    assert np.all(pad == pad[0, 0]) and np.unique(plain[:hr, :wr, 0]).size > 8


@pytest.mark.parametrize("mode", [0, 1])
def test_preprocess_batch_of_130_equals_single_calls(K, mode):
    """130 descriptors = three launches of 64: mixed source sizes, scales, flips and a shuffled n_index."""
    rng = np.random.default_rng(31 + mode)
    hn = wn = 40
    count = 130
    l = lr.padded(8, hn, wn, 1)
    sizes = [(23, 31), (40, 40), (57, 33), (18, 64), (35, 29), (49, 51)]
    imgs = [K.up(rng.integers(0, 256, (a, b, 3), dtype=np.uint8)) for a, b in sizes]
    slots = rng.permutation(count)
    descs = (K.capi.PrepImage * count)()
    single = K.sent32(words(l, count))
    p = K.capi.ptr
    for i in range(count):
        k = int(rng.integers(len(sizes)))
        h0, w0 = sizes[k]
        smax = min(hn / h0, wn / w0)
        sc = float(rng.uniform(0.45, 0.98)) * smax
        hr, wr = max(1, _cv_round(h0 * sc)), max(1, _cv_round(w0 * sc))
        assert hr <= hn and wr <= wn
        d = descs[i]
        d.img_bgr, d.im_scale, d.h0, d.w0, d.hr, d.wr = imgs[k].data_ptr(), sc, h0, w0, hr, wr
        d.flip, d.n_index = int(rng.integers(2)), int(slots[i])
        K.ok(K.lib.rtpose_preprocess_u8_flip(p(imgs[k]), h0, w0, sc, mode, p(single), K.L(l), d.n_index, hn, wn, hr, wr,
                                             d.flip, K.s))
    batch = K.sent32(words(l, count))
    K.ok(K.lib.rtpose_preprocess_u8_batch(descs, count, mode, p(batch), K.L(l), hn, wn, K.s))
    a, b = down32(single), down32(batch)
    idx = lr.index(l, count, hn, wn, 8)
    assert lr.untouched(b, idx, SENT32) and lr.untouched(a, idx, SENT32)
    assert not np.any(b[idx] == SENT32)
    assert np.array_equal(a, b)


# ---- flip merge, bilinear accumulate, fused TTA --------------------------------------------------------
def _tta_maps(B, hs, ws_stored, seed):
    """One buffer as the net writes it: PAF at channel 2, heat map at channel 41 of a 64-channel pixel, pad 3."""
    lp, lh = lr.padded(64, hs, ws_stored, 3, 2), lr.padded(64, hs, ws_stored, 3, 41)
    g = torch.Generator().manual_seed(seed)
    paf, heat = torch.randn(2 * B, 38, hs, ws_stored, generator=g), torch.rand(2 * B, 19, hs, ws_stored, generator=g) - 0.2
    buf = np.random.default_rng(seed).standard_normal(words(lp, 2 * B)).astype(np.float32)
    lr.scatter(buf, lp, paf.numpy())
    lr.scatter(buf, lh, heat.numpy())
    return buf, lp, lh, paf, heat


def _acc(K, B, hd, wd, c, beta, seed):
    n = B * hd * wd * c
    a0 = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    buf = np.full(n + 64, SENT32, dtype=np.uint32)
    if beta != 0:
        buf[:n] = a0.view(np.uint32)
    return K.up(buf), a0.reshape(B, hd, wd, c)


TTA_GEOS = [  # hs, stored width, w_valid, hd, wd, src_h_valid, src_w_valid
    (23, 26, 20, 46, 40, 23.0, 20.0),        # up x2, exact coordinates
    (24, 24, 18, 16, 12, 24.0, 18.0),        # down x1.5, exact coordinates
    (31, 33, 29, 46, 40, 30.3, 28.6),        # fractional valid region: only the agreement of the two paths is asserted
    (46, 46, 46, 46, 46, 46.0, 46.0),        # identity
]


@pytest.mark.parametrize("geo", TTA_GEOS)
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("beta", [0.0, 0.6])
def test_tta_accumulate_is_flip_merge_then_resize_exactly(K, geo, flip, beta):
    """The header's promise: rtpose_tta_accumulate accumulates exactly as rtpose_flip_merge followed by
    rtpose_resize_bilinear_accum would - bit for bit.  Where the resize coordinates are exact in fp32 both are also
    compared with the float64 reference: n = 12 roundings for the resize, 13 with the flip average in front."""
    hs, wst, wv, hd, wd, hv, wvv = geo
    B, alpha = 2, 0.25
    buf, lp, lh, paf, heat = _tta_maps(B, hs, wst, 40 + hs)
    src = K.up(buf)
    p = K.capi.ptr
    dense = {19: np.ascontiguousarray(nhwc(heat)[:, :, :wv]), 38: np.ascontiguousarray(nhwc(paf)[:, :, :wv])}
    # the fused launch
    fh, h0 = _acc(K, B, hd, wd, 19, beta, 1)
    fp, p0 = _acc(K, B, hd, wd, 38, beta, 2)
    K.ok(K.lib.rtpose_tta_accumulate(p(src), K.L(lh), p(src), K.L(lp), B, hs, wv, p(fh), p(fp), hd, wd, hv, wvv, alpha, beta,
                                     flip, K.s))
    # the two-launch form on dense copies of the valid columns
    if flip:
        dh, dhf, dp, dpf = K.up(dense[19][:B]), K.up(dense[19][B:]), K.up(dense[38][:B]), K.up(dense[38][B:])
        mh, mp = K.sent32(B * hs * wv * 19 + 64), K.sent32(B * hs * wv * 38 + 64)
        K.ok(K.lib.rtpose_flip_merge(p(dh), p(dhf), p(dp), p(dpf), B, hs, wv, p(mh), p(mp), K.s))
    else:
        mh, mp = K.up(dense[19][:B]), K.up(dense[38][:B])
    th, _ = _acc(K, B, hd, wd, 19, beta, 1)
    tp, _ = _acc(K, B, hd, wd, 38, beta, 2)
    K.ok(K.lib.rtpose_resize_bilinear_accum(p(mh), hs, wv, p(th), hd, wd, 19, B, hv, wvv, alpha, beta, K.s))
    K.ok(K.lib.rtpose_resize_bilinear_accum(p(mp), hs, wv, p(tp), hd, wd, 38, B, hv, wvv, alpha, beta, K.s))
    got = {}
    for c, fused, two, a0 in ((19, fh, th, h0), (38, fp, tp, p0)):
        a, b = down32(fused), down32(two)
        nacc = B * hd * wd * c
        assert np.all(a[nacc:] == SENT32) and np.all(b[nacc:] == SENT32), "written behind the accumulator"
        assert not np.any(a[:nacc] == SENT32)
        diff = np.flatnonzero(a != b)
        assert diff.size == 0, "C=%d: %d of %d words differ between the fused and the two-launch form" % (c, diff.size, nacc)
        got[c] = (a[:nacc].view(np.float32).astype(np.float64).reshape(B, hd, wd, c), a0)
    if not (lr.resize_coords_exact(hd, hs, hv) and lr.resize_coords_exact(wd, wv, wvv)):
        return
    a32 = float(np.float32(alpha))
    b32 = float(np.float32(beta))
    for c, swap, neg, m in ((19, lr.SWAP_HEAT, False, mh), (38, lr.SWAP_PAF, True, mp)):
        if flip:
            v, s = lr.flip_merge(dense[c][:B], dense[c][B:], swap, neg)
            mg = down32(m)
            nm = B * hs * wv * c
            assert np.all(mg[nm:] == SENT32)
            err = np.abs(mg[:nm].view(np.float32).astype(np.float64).reshape(B, hs, wv, c) - v.numpy())
            assert np.all(err <= U24 * s.numpy()), "flip_merge C=%d" % c      # one rounded add; the halving is exact
        else:
            v = torch.from_numpy(dense[c][:B]).to(torch.float64)
        rv, rs = lr.resize_bilinear(v, hd, wd, hv, wvv)
        g, a0 = got[c]
        ref, s = lr.accumulate(torch.from_numpy(a0), rv, rs, a32, b32)
        err = np.abs(g - ref.numpy())
        bound = (13 if flip else 12) * U24 * s.numpy()
        print("tta C=%d flip=%d: worst ratio %.3f" % (c, flip, float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound), "accumulate C=%d flip=%d" % (c, flip)


def test_resize_bilinear_accum_with_a_valid_region_narrower_than_the_source(K):
    """src_w_valid < stored width: the columns behind the valid region hold large values; only the edge clamp may see them."""
    hs, ws, hd, wd, c, n = 12, 16, 24, 24, 5, 2
    g = torch.Generator().manual_seed(50)
    src = torch.randn(n, hs, ws, c, generator=g)
    src[:, :, 12:] = 1e6
    srcd = K.up(src.numpy())
    dst, _ = _acc(K, n, hd, wd, c, 0.0, 3)
    K.ok(K.lib.rtpose_resize_bilinear_accum(K.capi.ptr(srcd), hs, ws, K.capi.ptr(dst), hd, wd, c, n, 12.0, 12.0, 1.0, 0.0, K.s))
    assert lr.resize_coords_exact(hd, hs, 12.0) and lr.resize_coords_exact(wd, ws, 12.0)
    v, s = lr.resize_bilinear(src, hd, wd, 12.0, 12.0)
    got = down32(dst)
    nacc = n * hd * wd * c
    assert np.all(got[nacc:] == SENT32)
    g_ = got[:nacc].view(np.float32).astype(np.float64).reshape(n, hd, wd, c)
    # the last destination column interpolates towards stored column 12 with weight 0.25 - that IS the kernel's
    # contract (edge clamp at the stored width) - every column before it sees the valid region only
    assert np.all(np.abs(g_ - v.numpy()) <= 12 * U24 * s.numpy())
    assert np.all(np.abs(g_[:, :, :wd - 1]) < 100)


# ---- the empty call and the refusals -------------------------------------------------------------------
def _scene(K):
    """Small valid arguments for every entry point; all destinations are sentinel buffers."""
    n, h, w, c = 2, 8, 8, 24
    sc = type("S", (), {})()
    sc.n, sc.h, sc.w, sc.c = n, h, w, c
    sc.ls, sc.ld = lr.padded(32, h, w, 1, 8), lr.padded(48, h, w, 1, 16)
    sc.ls16, sc.ld32 = lr.padded(64, h, w, 1, 16), lr.padded(96, h, w, 1, 32)
    wmax = words(sc.ld32, n)
    sc.src = K.up(np.zeros(wmax, dtype=np.float32))
    sc.d32, sc.d16 = K.sent32(wmax), K.sent16(wmax)
    sc.wt, sc.b = K.up(np.ones(9 * 32 * 8, dtype=np.float32)), K.up(np.ones(64, dtype=np.float32))
    sc.cmap = K.up(np.arange(c, dtype=np.int32))
    sc.img = K.up(np.zeros((8, 8, 3), dtype=np.uint8))
    return sc


def _clean(sc):
    return bool(np.all(down32(sc.d32) == SENT32)) and bool(np.all(down16(sc.d16) == SENT16))


def test_empty_calls_return_ok_and_write_nothing(K):
    sc = _scene(K)
    lib, p, L, s = K.lib, K.capi.ptr, K.L, K.s
    n, h, w, c = 0, sc.h, sc.w, sc.c
    src, d32, d16, wt, b, cm = p(sc.src), p(sc.d32), p(sc.d16), p(sc.wt), p(sc.b), p(sc.cmap)
    ls, ld = sc.ls, sc.ld
    calls = {
        "rtpose_nchw_to_layout": lambda n, c: lib.rtpose_nchw_to_layout(src, d32, L(ld), c, c, n, h, w, s),
        "rtpose_layout_to_nchw": lambda n, c: lib.rtpose_layout_to_nchw(src, L(ls), d32, c, n, h, w, s),
        "rtpose_layout_copy": lambda n, c: lib.rtpose_layout_copy(src, L(ls), d32, L(ld), c, n, h, w, s),
        "rtpose_maxpool2x2": lambda n, c: lib.rtpose_maxpool2x2(src, L(ls), d32, L(ld), c, n, h, w, s),
        "rtpose_maxpool3x3s2_ceil": lambda n, c: lib.rtpose_maxpool3x3s2_ceil(src, L(ls), d32, L(ld), c, n, h, w, s),
        "rtpose_maxpool3x3s2_ceil_bf16": lambda n, c: lib.rtpose_maxpool3x3s2_ceil_bf16(src, L(ls), d16, L(ld), c, n, h, w, s),
        "rtpose_nchw_to_layout_affine": lambda n, c: lib.rtpose_nchw_to_layout_affine(src, d32, L(ld), c, c, n, h, w, b, b, s),
        "rtpose_dwconv3x3": lambda n, c: lib.rtpose_dwconv3x3(src, L(ls), wt, b, d32, L(ld), c, n, h, w, 1, s),
        "rtpose_dwconv3x3 s2": lambda n, c: lib.rtpose_dwconv3x3(src, L(ls), wt, b, d32, L(ld), c, n, h, w, 2, s),
        "rtpose_dwconv3x3_bf16": lambda n, c: lib.rtpose_dwconv3x3_bf16(src, L(ls), wt, b, d16, L(ld), c, n, h, w, 1, s),
        "rtpose_layout_copy_cmap": lambda n, c: lib.rtpose_layout_copy_cmap(src, L(ls), d32, L(ld), c, cm, n, h, w, s),
        "rtpose_layout_copy_cmap_bf16": lambda n, c: lib.rtpose_layout_copy_cmap_bf16(src, L(ls), d16, L(ld), c, cm, n, h, w, s),
        "rtpose_layout_axpby": lambda n, c: lib.rtpose_layout_axpby(d32, L(ld), src, c, n, h, w, 0.5, 0.5, s),
        "rtpose_nchw_to_layout_bf16": lambda n, c: lib.rtpose_nchw_to_layout_bf16(src, d16, L(ld), c, c, n, h, w, s),
        "rtpose_layout_f32_to_bf16": lambda n, c: lib.rtpose_layout_f32_to_bf16(src, L(ls), d16, L(ld), c, c, n, h, w, s),
        "rtpose_layout_bf16_to_f32": lambda n, c: lib.rtpose_layout_bf16_to_f32(src, L(ls), d32, L(ld), c, n, h, w, s),
        "rtpose_nchw_to_layout_split": lambda n, c: lib.rtpose_nchw_to_layout_split(src, d16, L(sc.ld32), c, c, n, h, w, s),
        "rtpose_layout_f32_to_split": lambda n, c: lib.rtpose_layout_f32_to_split(src, L(ls), d16, L(sc.ld32), c, c, n, h, w, s),
        "rtpose_layout_split_to_f32": lambda n, c: lib.rtpose_layout_split_to_f32(src, L(sc.ls16), d32, L(ld), c, n, h, w, s),
    }
    for name, f in calls.items():
        K.ok(f(0, c), name + " N = 0")
        K.ok(f(2, 0), name + " C = 0")                        # every one of these accepts an empty channel slice too
        assert _clean(sc), name
    only_n = {
        "rtpose_stem_conv3x3_s2": lambda: lib.rtpose_stem_conv3x3_s2(src, L(ls), wt, b, d32, L(ld), 8, 24, 0, h, w, 1, s),
        "rtpose_stem_conv3x3_s2_nchw": lambda: lib.rtpose_stem_conv3x3_s2_nchw(src, None, None, wt, b, d32, L(ld), 24, 0, h, w, 1, s),
        "rtpose_stem_conv3x3_s2_nchw_ex": lambda: lib.rtpose_stem_conv3x3_s2_nchw_ex(src, None, None, wt, b, d16, L(ld), 24, 0, h, w, 1, 1, s),
        "rtpose_flip_merge": lambda: lib.rtpose_flip_merge(src, src, src, src, 0, h, w, d32, d32, s),
    }
    for name, f in only_n.items():
        K.ok(f(), name + " N = 0")
        assert _clean(sc), name
    # the launchers that state a refusal of the empty call
    l8 = lr.padded(8, 8, 8, 1)
    refused = {
        "rtpose_resize_bilinear_accum": lambda: lib.rtpose_resize_bilinear_accum(src, 8, 8, d32, 8, 8, 4, 0, 8.0, 8.0, 1.0, 0.0, s),
        "rtpose_tta_accumulate": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16), src, L(sc.ls16), 0, 8, 8, d32, d32, 8, 8, 8.0, 8.0,
                                                                   1.0, 0.0, 0, s),
        "rtpose_stem_pool_nchw": lambda: lib.rtpose_stem_pool_nchw(src, None, None, wt, b, d32, L(ld), 24, 0, 16, 16, 0, s),
        "rtpose_preprocess_u8_batch": lambda: lib.rtpose_preprocess_u8_batch((K.capi.PrepImage * 1)(), 0, 0, d32, L(l8), 8, 8, s),
    }
    for name, f in refused.items():
        K.inval(f(), name)
        assert _clean(sc), name


def test_argument_checks_refuse_and_write_nothing(K):
    sc = _scene(K)
    lib, p, L, s = K.lib, K.capi.ptr, K.L, K.s
    n, h, w, c = sc.n, sc.h, sc.w, sc.c
    src, d32, d16, wt, b, cm, img = p(sc.src), p(sc.d32), p(sc.d16), p(sc.wt), p(sc.b), p(sc.cmap), p(sc.img)
    ls, ld = sc.ls, sc.ld
    odd_off, odd_cs = ld._replace(choff=2), ld._replace(cstride=50)
    off4, cs12 = ld._replace(choff=4), ld._replace(cstride=44)       # 16-byte but not 32-byte / bf16 aligned
    nogap = lr.dense(32, h, w, 8)                                     # a stencil source needs a gap of >= 1
    l8 = lr.padded(8, 8, 8, 1)
    bad = {
        "nchw_to_layout cpad < C": lambda: lib.rtpose_nchw_to_layout(src, d32, L(ld), 8, 4, n, h, w, s),
        "nchw_to_layout slice past cstride": lambda: lib.rtpose_nchw_to_layout(src, d32, L(ld), 24, 40, n, h, w, s),
        "maxpool2x2 C % 4": lambda: lib.rtpose_maxpool2x2(src, L(ls), d32, L(ld), 6, n, h, w, s),
        "maxpool2x2 choff": lambda: lib.rtpose_maxpool2x2(src, L(ls), d32, L(odd_off), c, n, h, w, s),
        "maxpool2x2 cstride": lambda: lib.rtpose_maxpool2x2(src, L(ls), d32, L(odd_cs), c, n, h, w, s),
        "affine cpad < C": lambda: lib.rtpose_nchw_to_layout_affine(src, d32, L(ld), 8, 4, n, h, w, b, b, s),
        "affine scale without shift": lambda: lib.rtpose_nchw_to_layout_affine(src, d32, L(ld), 8, 8, n, h, w, b, None, s),
        "stem no gap": lambda: lib.rtpose_stem_conv3x3_s2(src, L(nogap), wt, b, d32, L(ld), 8, 24, n, h, w, 1, s),
        "stem cout": lambda: lib.rtpose_stem_conv3x3_s2(src, L(ls), wt, b, d32, L(ld), 8, 20, n, h, w, 1, s),
        "stem cin_pad": lambda: lib.rtpose_stem_conv3x3_s2(src, L(ls), wt, b, d32, L(ld), 4, 24, n, h, w, 1, s),
        "stem_nchw cout": lambda: lib.rtpose_stem_conv3x3_s2_nchw(src, None, None, wt, b, d32, L(ld), 16, n, h, w, 1, s),
        "stem_nchw choff": lambda: lib.rtpose_stem_conv3x3_s2_nchw(src, None, None, wt, b, d32, L(odd_off), 24, n, h, w, 1, s),
        "stem_nchw_ex bf16 choff % 8": lambda: lib.rtpose_stem_conv3x3_s2_nchw_ex(src, None, None, wt, b, d16, L(off4), 24, n, h, w, 1, 1, s),
        "stem_pool NULL": lambda: lib.rtpose_stem_pool_nchw(None, None, None, wt, b, d32, L(ld), 24, n, 16, 16, 0, s),
        "stem_pool H < 8": lambda: lib.rtpose_stem_pool_nchw(src, None, None, wt, b, d32, L(ld), 24, n, 4, 16, 0, s),
        "stem_pool cout": lambda: lib.rtpose_stem_pool_nchw(src, None, None, wt, b, d32, L(ld), 16, n, 16, 16, 0, s),
        "stem_pool slice past cstride": lambda: lib.rtpose_stem_pool_nchw(src, None, None, wt, b, d32, L(ld._replace(choff=32)), 24, n, 16, 16, 0, s),
        "maxpool3x3 H < 3": lambda: lib.rtpose_maxpool3x3s2_ceil(src, L(ls), d32, L(ld), c, n, 2, w, s),
        "maxpool3x3 W < 3": lambda: lib.rtpose_maxpool3x3s2_ceil(src, L(ls), d32, L(ld), c, n, h, 2, s),
        "maxpool3x3 choff": lambda: lib.rtpose_maxpool3x3s2_ceil(src, L(ls), d32, L(odd_off), c, n, h, w, s),
        "maxpool3x3_bf16 H < 3": lambda: lib.rtpose_maxpool3x3s2_ceil_bf16(src, L(ls), d16, L(ld), c, n, 2, w, s),
        "maxpool3x3_bf16 choff % 8": lambda: lib.rtpose_maxpool3x3s2_ceil_bf16(src, L(ls), d16, L(off4), c, n, h, w, s),
        "maxpool3x3_bf16 C % 8": lambda: lib.rtpose_maxpool3x3s2_ceil_bf16(src, L(ls), d16, L(ld), 12, n, h, w, s),
        "dwconv stride 3": lambda: lib.rtpose_dwconv3x3(src, L(ls), wt, b, d32, L(ld), c, n, h, w, 3, s),
        "dwconv no gap": lambda: lib.rtpose_dwconv3x3(src, L(nogap), wt, b, d32, L(ld), c, n, h, w, 1, s),
        "dwconv cstride": lambda: lib.rtpose_dwconv3x3(src, L(ls), wt, b, d32, L(odd_cs), c, n, h, w, 1, s),
        "dwconv_bf16 stride 3": lambda: lib.rtpose_dwconv3x3_bf16(src, L(ls), wt, b, d16, L(ld), c, n, h, w, 3, s),
        "dwconv_bf16 no gap": lambda: lib.rtpose_dwconv3x3_bf16(src, L(nogap), wt, b, d16, L(ld), c, n, h, w, 2, s),
        "dwconv_bf16 cstride % 8": lambda: lib.rtpose_dwconv3x3_bf16(src, L(ls), wt, b, d16, L(cs12), c, n, h, w, 1, s),
        "copy_cmap NULL": lambda: lib.rtpose_layout_copy_cmap(src, L(ls), d32, L(ld), c, None, n, h, w, s),
        "copy_cmap_bf16 NULL": lambda: lib.rtpose_layout_copy_cmap_bf16(src, L(ls), d16, L(ld), c, None, n, h, w, s),
        "copy_cmap_bf16 source choff": lambda: lib.rtpose_layout_copy_cmap_bf16(src, L(ls._replace(choff=4)), d16, L(ld), c, cm, n, h, w, s),
        "preprocess mode": lambda: lib.rtpose_preprocess_u8(img, 8, 8, 1.0, 2, d32, L(l8), 0, 8, 8, 8, 8, s),
        "preprocess cstride < 8": lambda: lib.rtpose_preprocess_u8(img, 8, 8, 1.0, 0, d32, L(lr.padded(4, 8, 8, 1)), 0, 8, 8, 8, 8, s),
        "preprocess hr > Hn": lambda: lib.rtpose_preprocess_u8_flip(img, 8, 8, 1.0, 0, d32, L(l8), 0, 8, 8, 9, 8, 1, s),
        "preprocess NULL image": lambda: lib.rtpose_preprocess_u8(None, 8, 8, 1.0, 0, d32, L(l8), 0, 8, 8, 8, 8, s),
        "resize hs 0": lambda: lib.rtpose_resize_bilinear_accum(src, 0, 8, d32, 8, 8, 4, 1, 8.0, 8.0, 1.0, 0.0, s),
        "resize valid 0": lambda: lib.rtpose_resize_bilinear_accum(src, 8, 8, d32, 8, 8, 4, 1, 0.0, 8.0, 1.0, 0.0, s),
        "tta NULL": lambda: lib.rtpose_tta_accumulate(None, L(sc.ls16), src, L(sc.ls16), 1, 8, 8, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "tta w_valid 0": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16), src, L(sc.ls16), 1, 8, 0, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        # the COCO-18 doors share the table-driven doors' argument check (csrc/tta.hip): each of these used to read or
        # write outside the caller's buffers, or dereference NULL
        "tta NULL layout": lambda: lib.rtpose_tta_accumulate(src, None, src, L(sc.ls16), 1, 8, 8, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "tta w_valid above ws": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16), src, L(sc.ls16), 1, 8, sc.ls16.ws + 1, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "tta hs above the view's": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16), src, L(sc.ls16), 1, sc.ls16.hs + 1, 8, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "tta heat view of 18 channels": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16._replace(choff=64 - 18)), src, L(sc.ls16), 1, 8, 8, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "tta paf view of 37 channels": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16), src, L(sc.ls16._replace(choff=64 - 37)), 1, 8, 8, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "tta B 65536": lambda: lib.rtpose_tta_accumulate(src, L(sc.ls16), src, L(sc.ls16), 65536, 8, 8, d32, d32, 8, 8, 8.0, 8.0, 1.0, 0.0, 0, s),
        "flip_merge NULL output": lambda: lib.rtpose_flip_merge(src, src, src, src, 1, h, w, None, d32, s),
        "flip_merge NULL map": lambda: lib.rtpose_flip_merge(src, None, src, src, 1, h, w, d32, d32, s),
        "to_bf16 cpad % 8": lambda: lib.rtpose_nchw_to_layout_bf16(src, d16, L(ld), 4, 4, n, h, w, s),
        "to_bf16 cpad < C": lambda: lib.rtpose_nchw_to_layout_bf16(src, d16, L(ld), 16, 8, n, h, w, s),
        "f32_to_bf16 choff % 8": lambda: lib.rtpose_layout_f32_to_bf16(src, L(ls), d16, L(off4), 8, 8, n, h, w, s),
        "f32_to_bf16 cstride % 8": lambda: lib.rtpose_layout_f32_to_bf16(src, L(ls), d16, L(cs12), 8, 8, n, h, w, s),
        "to_split cstride % 16": lambda: lib.rtpose_nchw_to_layout_split(src, d16, L(ld._replace(cstride=56)), 8, 8, n, h, w, s),
        "to_split choff % 16": lambda: lib.rtpose_layout_f32_to_split(src, L(ls), d16, L(sc.ld32._replace(choff=8)), 8, 8, n, h, w, s),
        "to_split cpad < C": lambda: lib.rtpose_layout_f32_to_split(src, L(ls), d16, L(sc.ld32), 16, 8, n, h, w, s),
        "split_to_f32 odd choff": lambda: lib.rtpose_layout_split_to_f32(src, L(sc.ls16._replace(choff=3)), d32, L(ld), 8, n, h, w, s),
    }
    for name, f in bad.items():
        K.inval(f(), name)
    assert _clean(sc)


# ---- offsets beyond 2^32 bytes -------------------------------------------------------------------------
FAR_LEAD = (1 << 24) + 4099          # x 64 channels x 4 bytes (or 2 x 64 x 2) puts image 0 more than 2^32 bytes in


def _far_check(K, buf, l, n, idx, view, sent, compare):
    """Only the window around the images comes to the host; everything in front of it is checked on the device."""
    start = int(idx.min()) - 4096
    assert start * buf.element_size() > 2 ** 32
    torch.cuda.synchronize()
    step = 1 << 28
    for a in range(0, start, step):
        assert not bool((buf[a:min(a + step, start)] != sent).any().item()), "a word in front of the images was written"
    win = view(buf[start:])
    compare(win, idx - start)


@pytest.mark.parametrize("op", ["layout_copy", "maxpool2x2", "dwconv3x3", "dwconv3x3_bf16"])
def test_far_offset(K, op):
    """A layout whose lead puts image 0 more than 2^32 bytes into BOTH buffers (about 4.3 GB each, filled on the device):
    a 32-bit offset anywhere in the addressing would land in front of the images."""
    n, h, w, c = 2, 9, 10, 64
    bf = op.endswith("bf16")
    mult = 2 if bf else 1
    ls = lr.Lay(64 * mult, 0, w + 1, h + 1, FAR_LEAD)
    stride = 2 if op == "maxpool2x2" else 1
    ho, wo = (h // 2, w // 2) if op == "maxpool2x2" else (h, w)
    ld = lr.Lay(64 * mult, 0, wo + 1, ho + 1, FAR_LEAD + 7)
    dt = torch.int16 if bf else torch.int32
    sent = SENT16 if bf else SENT32
    x = signed_and_negative((n, c, h, w), 60)[1][1]
    src = torch.zeros(words(ls, n), dtype=dt, device=K.dev)
    s0 = int(lr.offsets(ls, 1, 1, 1)[0, 0, 0]) - (w + 2) * ls.cstride       # the window that holds the images and their gaps
    tail = np.zeros(words(ls, n) - s0, dtype=np.uint16 if bf else np.uint32)      # bits: the upload must not convert values
    if bf:
        xb = lr.bf16_rne(x.numpy())
        tail[lr.index(ls, n, h, w, c) - s0] = nhwc(xb)
        xv = lr.bf16_to_f32(xb)
    else:
        tail[lr.index(ls, n, h, w, c) - s0] = bits32(nhwc(x))
        xv = x.numpy()
    up = K.up(tail)
    assert up.dtype == src.dtype
    src[s0:] = up
    dst = torch.full((words(ld, n),), sent, dtype=dt, device=K.dev)
    p = K.capi.ptr
    wt, b = _dw_weights(c, 61)
    wd, bd = K.up(wt.view(c, 9).t().contiguous().numpy()), K.up(b.numpy())
    if op == "layout_copy":
        K.ok(K.lib.rtpose_layout_copy(p(src), K.L(ls), p(dst), K.L(ld), c, n, h, w, K.s))
        cmpf = lambda win, idx: check_bits(win, idx, bits32(nhwc(xv)), SENT32, op)
    elif op == "maxpool2x2":
        K.ok(K.lib.rtpose_maxpool2x2(p(src), K.L(ls), p(dst), K.L(ld), c, n, h, w, K.s))
        cmpf = lambda win, idx: check_bits(win, idx, bits32(nhwc(lr.maxpool2x2(xv).to(torch.float32))), SENT32, op)
    elif op == "dwconv3x3":
        K.ok(K.lib.rtpose_dwconv3x3(p(src), K.L(ls), p(wd), p(bd), p(dst), K.L(ld), c, n, h, w, 1, K.s))
        ref, s = lr.dwconv3x3(xv, wt, b, 1)
        cmpf = lambda win, idx: check_close(win, idx, nhwc(ref), 10 * U24 * nhwc(s), op)
    else:
        K.ok(K.lib.rtpose_dwconv3x3_bf16(p(src), K.L(ls), p(wd), p(bd), p(dst), K.L(ld), c, n, h, w, 1, K.s))
        ref, s = lr.dwconv3x3(xv, wt, b, 1)
        cmpf = lambda win, idx: check_bracket(win, idx, nhwc(ref), 10 * U24 * nhwc(s), op)
    _far_check(K, dst, ld, n, lr.index(ld, n, ho, wo, c), down16 if bf else down32, sent, cmpf)
    del src, dst
    torch.cuda.empty_cache()
