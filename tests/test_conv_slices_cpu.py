"""CPU suite of the input-slice tests: the builder of tests/conv_slices.py is correct, the cases of
tests/test_conv_input_slices_gpu.py discriminate (a kernel that reads the slice one alignment unit off, or walks the wide
buffer with the compact pixel stride, is further from the float64 reference than 100 times the tolerance that test applies),
and the first-layer launchers refuse an image slice that does not fit its pixel before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_driver as cd
import conv_slices as cs
import layout_restate as lr


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- the builder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,unit", [(torch.float32, cs.UNIT_F32), (torch.bfloat16, cs.UNIT_BF16), (torch.bfloat16, cs.UNIT_X3)],
                         ids=("fp32", "bf16", "bf16x3"))
@pytest.mark.parametrize("geom", (0, 1, 2), ids=("mid", "end", "dense"))
@pytest.mark.parametrize("pad", (0, 1, 3))
def test_widen_copies_the_slice_and_surrounds_it_with_decoys(dtype, unit, geom, pad):
    n, h, w, c, cin_e = 3, 5, 7, 13, 16
    lay = lr.padded(cin_e, h, w, pad)
    npx = lr.pixels(lay, n)
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(pad)).to(dtype)
    compact = cs.scatter_nchw(x, lay, npx, dtype)
    assert torch.equal(_bits(cs.slice_of(compact, lay, n, h, w, c)), _bits(x))
    name, extra, choff = cs.geometries(cin_e, unit)[geom]
    wide, wl = cs.widen(compact, lay, n, h, w, extra, choff, seed=5)
    assert wide.dtype == dtype and wide.numel() == npx * (cin_e + extra)
    assert (wl.cstride, wl.choff, wl.ws, wl.hs, wl.lead) == (cin_e + extra, choff, lay.ws, lay.hs, lay.lead)
    assert wl.cstride % unit == 0 and wl.choff % unit == 0 and wl.choff > 0
    if name == "end":
        assert wl.choff + cin_e == wl.cstride
    if name == "dense":
        assert wl.cstride == 3 * cin_e and wl.choff == cin_e
    # the slice, read back through lr.index, is the compact data bit for bit - on every pixel of the buffer
    assert torch.equal(_bits(cs.slice_of(wide, wl, n, h, w, c)), _bits(x))
    pm = wide.view(npx, wl.cstride)
    assert torch.equal(_bits(pm[:, choff:choff + cin_e].contiguous()), _bits(compact.view(npx, cin_e)))
    # decoys everywhere else on the real pixels, zeros on every gap pixel (lead, gaps, tail slack) in all channels
    real = np.zeros(npx, dtype=bool)
    real[lr.offsets(lr.Lay(1, 0, lay.ws, lay.hs, lay.lead), n, h, w).ravel()] = True
    assert real.sum() == n * h * w
    other = np.ones(wl.cstride, dtype=bool)
    other[choff:choff + cin_e] = False
    dec = pm[torch.from_numpy(real)][:, torch.from_numpy(other)].float()
    assert dec.numel() == n * h * w * extra
    assert torch.isfinite(dec).all() and (dec.abs() >= 1024).all() and (dec.abs() < 2048).all()
    assert (dec > 0).any() and (dec < 0).any()
    assert torch.equal(dec, dec.to(torch.bfloat16).float())                 # exactly representable in bf16
    assert _bits(pm[torch.from_numpy(~real)]).eq(0).all()
    # the compact buffer was not changed, and another seed gives other decoys
    assert torch.equal(_bits(compact), _bits(cs.scatter_nchw(x, lay, npx, dtype)))
    assert not torch.equal(_bits(cs.widen(compact, lay, n, h, w, extra, choff, seed=6)[0]), _bits(wide))


def test_relead_moves_pixel_zero_and_keeps_the_slice():
    n, h, w, c = 2, 4, 6, 8
    lay = lr.padded(c, h, w, 1)
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(1))
    wide, wl = cs.widen(cs.scatter_nchw(x, lay, lr.pixels(lay, n)), lay, n, h, w, 8, 4)
    moved, ml = cs.relead(wide, wl, lay.ws + 3)
    assert ml.lead == wl.lead + lay.ws + 3 and moved.numel() == lr.pixels(ml, n) * ml.cstride
    assert torch.equal(cs.slice_of(moved, ml, n, h, w, c), x)
    assert moved[:(lay.ws + 3) * ml.cstride].abs().sum().item() == 0


# ---- the cases discriminate -----------------------------------------------------------------------------------------------
def _wrong_views(wl, cin_e, unit):
    """the slice one alignment unit off (towards the side that has room) and the wide buffer walked with the compact stride"""
    shifted = wl.choff + unit if wl.choff + unit + cin_e <= wl.cstride else wl.choff - unit
    return [lr.Lay(wl.cstride, shifted, wl.ws, wl.hs, wl.lead), lr.Lay(cin_e, 0, wl.ws, wl.hs, wl.lead)]


def _assert_discriminates(x, cin_e, pad, unit, geoms, conv, tol_of):
    """x [n, c, h, w]; conv(x) -> float64 reference; tol_of(ref) -> the GPU test's tolerance (a number or a tensor)"""
    n, c, h, w = x.shape
    lay = lr.padded(cin_e, h, w, pad)
    compact = cs.scatter_nchw(x, lay, lr.pixels(lay, n))
    ref = conv(x)
    tol = tol_of(ref)
    for name, extra, choff in geoms:
        wide, wl = cs.widen(compact, lay, n, h, w, extra, choff)
        assert torch.equal(conv(cs.slice_of(wide, wl, n, h, w, c)), ref)
        for wrong in _wrong_views(wl, cin_e, unit):
            ratio = ((conv(cs.slice_of(wide, wrong, n, h, w, c)) - ref).abs() / tol).max().item()
            assert ratio > 100.0, (name, wrong, ratio)


@pytest.mark.parametrize("case", cs.TINY_F32, ids=lambda c: "k%d-m%s-%dx%dx%dx%d-%d-%d%d%d" % c)
def test_tiny_fp32_cases_discriminate(case):
    k, m, n, h, w, cin, cout, relu, pool, prelu = case
    g = torch.Generator().manual_seed(k * 100 + cin + cout)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    sl = (torch.rand(cout, generator=g) * 0.5 - 0.1).double().view(1, -1, 1, 1) if prelu else None

    def conv(v):
        y = F.conv2d(v.double(), wt.double(), b.double(), padding=k // 2)
        y = F.relu(y) if relu else y
        y = torch.where(y >= 0, y, sl * y) if prelu else y
        return F.max_pool2d(y, 2, 2, 0) if pool else y

    def tol_of(ref):
        if k == 7 and m == 8:      # F(8,7): the element-wise bound gamma * 2^-24 * sum |x| |w|
            return cd.gamma_limit_f87(wt) * cd.U * cd.ref64(x, wt, b, 7, None)[1]
        return cd.TOL * max(1.0, ref.abs().max().item())

    cin_e = (cin + 7) // 8 * 8
    _assert_discriminates(x, cin_e, k // 2, cs.UNIT_F32, cs.geometries(cin_e, cs.UNIT_F32), conv, tol_of)


@pytest.mark.parametrize("shape", [(1, 9, 13, 128), (1, 11, 7, 512)])
def test_pointwise_pair_cases_discriminate(shape):
    n, h, w, mid = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, 128, h, w, generator=g)
    w1 = torch.randn(mid, 128, 1, 1, generator=g).double() * (2.0 / 128) ** 0.5
    w2 = torch.randn(38, mid, 1, 1, generator=g).double() * (2.0 / mid) ** 0.5
    conv = lambda v: F.conv2d(F.relu(F.conv2d(v.double(), w1)), w2)      # noqa: E731
    _assert_discriminates(x, 128, 0, cs.UNIT_F32, [("mid", 16, 8), ("end", 8, 8)], conv,
                          lambda ref: cd.TOL * max(1.0, ref.abs().max().item()))


@pytest.mark.parametrize("shape,k", [((3, 8, 8), 3), ((1, 37, 45), 3), ((1, 43, 33), 7)])
def test_first_layer_cases_discriminate(shape, k):
    """rtpose_conv_first (k = 3) and rtpose_conv7x7_s2 (k = 7, stride 2) on the three image slices; their loads are scalar,
    so 'one unit off' is one channel."""
    n, h, w = shape
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.rand(n, 3, h, w, generator=g) - 0.5
    wt = torch.randn(64, 3, k, k, generator=g).double() * (2.0 / (3 * k * k)) ** 0.5
    conv = lambda v: F.relu(F.conv2d(v.double(), wt, None, stride=1 if k == 3 else 2, padding=k // 2))      # noqa: E731
    tol = cd.TOL if k == 3 else cd.STEM7_TOL
    geoms = [("lx", cstride - 3, choff) for cstride, choff in ((4, 0), (8, 4), (16, 8))]
    _assert_discriminates(x, 3, 1, 1, geoms, conv, lambda ref: tol * max(1.0, ref.abs().max().item()))


# ---- the first-layer launchers refuse an image slice that leaves its pixel --------------------------------------------------
FAKE = 1 << 20          # a device pointer no refused launch touches
N, H, W = 1, 8, 8


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: runs where no GPU is visible")
@pytest.mark.parametrize("entry", ("rtpose_conv_first", "rtpose_conv_first_bf16", "rtpose_conv_first_planes", "rtpose_conv7x7_s2"))
@pytest.mark.parametrize("lx", [(4, 2), (8, 6), (3, 1)], ids=lambda v: "cstride%d-choff%d" % v)
def test_first_layer_launchers_refuse_an_image_slice_outside_its_pixel(capi, entry, lx):
    """x_nchw = NULL and lx.choff + 3 > lx.cstride: RTPOSE_E_INVAL before any HIP call, from every launcher that reads the
    image through `lx` (rtpose_conv7x7_s2 already did).  The same call with the slice inside its pixel gets past this check:
    where no GPU is visible it fails at its first HIP call instead, with another code."""
    lib, Layout = capi.lib, capi.Layout
    lout = Layout.padded(64, H, W, 1)
    planes = entry == "rtpose_conv_first_planes"
    q = lib.rtpose_layout_pixels(C.byref(lout), N, H, W)

    def call(layout):
        args = [None, FAKE, C.byref(layout), FAKE, FAKE, C.byref(lout)] + ([q] if planes else []) + [1, N, H, W, None]
        return getattr(lib, entry)(*args)

    rc = call(Layout.padded(lx[0], H, W, 1, choff=lx[1]))
    err = capi.last_error()
    assert rc == -1, (entry, rc, err)
    assert "input slice exceeds cstride" in err, (entry, err)
    rc = call(Layout.padded(lx[1] + 3, H, W, 1, choff=lx[1]))      # the slice at the end of its pixel
    assert not (rc == -1 and "input slice exceeds cstride" in capi.last_error()), entry
