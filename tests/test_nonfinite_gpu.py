"""NaN and Inf through every kernel a training step launches (include/rtpose_mi355x.h section 2, "Non-finite values"),
against the float64 references of tests/nonfinite_cases.py: NaN exactly where the reference has NaN, the same signed Inf
exactly where it has Inf, every other value ==.  tests/test_nonfinite_cpu.py holds the cases to their conditions.

The launches go through the drivers the finite suites use: conv_driver for the forward convs, the launch helpers of
test_conv_backward_gpu / test_batchnorm_gpu / test_dwconv_backward_gpu (sentinel-guarded outputs, every word outside a
slice untouched) for the backward and per-channel kernels, train.py for the stems and the end-to-end chain."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_restate as br
import conv_backward_restate as cb
import conv_driver as cd
import dwconv_restate as dr
import layout_restate as lr
import nonfinite_cases as nf
import test_batchnorm_gpu as bn_gpu
import test_conv_backward_bf16_gpu as wgb_gpu
import test_conv_backward_gpu as wg_gpu
import test_dwconv_backward_gpu as dw_gpu

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC1                  # the sentinel of a bf16 output buffer
NAN16_IN = 0x7FC0               # beside a bf16 input slice


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


def _ids(cases):
    return dict(argvalues=cases, ids=[c.tag for c in cases])


# ---- the forward convs ---------------------------------------------------------------------------------------------------------------
def _conv(capi, dev, c):
    x, wt, b = nf.conv_operands(c)
    want = nf.conv_reference(c, x, wt, b)
    P = cd.given(cd.Form(c.kind, c.k, None, c.out_f32), [x], [wt], [b], c.relu)
    if c.kind == "f32" or c.out_f32:
        policy = cd.Out(16, 8, cd.SENTINEL) if c.aligned else cd.sentinel(1, 3)
    else:
        policy = cd.Out(16, 8, NAN16) if c.aligned else cd.Out(3, 1, NAN16)
    buf, lay = cd.to_layout(capi, dev, P, x, c.k // 2)
    fits = []
    obuf, louts = cd.launch(capi, dev, P, [(buf, lay)], policy, 1,
                            hook=lambda gi, d, ob, lo: fits.append(capi.lib.rtpose_conv3x3_c64_bf16_fits(C.byref(d), 1, c.n, c.h, c.w)))
    assert c.kind != "bf16" or fits == [int("c64" in c.tag)], "the 64-channel kernel takes exactly the c64 cases"
    cd.outputs(P, obuf, louts, policy, values=False)                # every word outside the slice still holds the sentinel
    bits = cd.np_bits(obuf)[lr.index(louts[0], c.n, c.h, c.w, c.cout)]
    got = bits.view(np.float32) if bits.dtype == np.uint32 else lr.bf16_to_f32(bits)
    got = np.ascontiguousarray(np.transpose(got.reshape(c.n, c.h, c.w, c.cout), (0, 3, 1, 2)))
    print("%s: expected classes %s, stored %s" % (c.tag, np.bincount(nf.classes(want).ravel(), minlength=4).tolist(),
                                                  np.bincount(nf.classes(got).ravel(), minlength=4).tolist()))
    nf.same_class_and_values(got, want, c.tag)


@pytest.mark.parametrize("c", **_ids(nf.CONV_F32))
def test_conv2d(capi, cuda, c):
    _conv(capi, cuda, c)


@pytest.mark.parametrize("c", **_ids(nf.CONV_BF16))
def test_conv2d_bf16(capi, cuda, c):
    _conv(capi, cuda, c)


# ---- the weight gradients ---------------------------------------------------------------------------------------------------------------
def _bf16_buffer(capi, lay, n, h, w, t, zero_channels, gaps_zero):
    """a bf16 layout buffer (uint16): NaN everywhere, zero in the slice's channels of every pixel if gaps_zero, the upper 16
    bits of t [n, c, h, w] - integers bf16 holds, and the injected patterns - at the valid pixels"""
    a = np.full((cd.npx(capi, lay, n, h, w), lay.cstride), NAN16_IN, dtype=np.uint16)
    if gaps_zero:
        a[:, lay.choff:lay.choff + zero_channels] = 0
    u = t.numpy().view(np.uint32)
    assert (np.isnan(t.numpy()) | ((u & 0xFFFF) == 0)).all()
    return lr.scatter(a.reshape(-1), lay, (u >> 16).astype(np.uint16))


def _check_wgrad(c, dw_bits, db_bits, x, gy):
    dw, db = nf.wgrad_torch(x, gy, c.k)
    got_w, got_b = dw_bits.view(np.float32).reshape(dw.shape), db_bits.view(np.float32)
    print("%s: dw classes %s, dbias %s" % (c.tag, np.bincount(nf.classes(got_w).ravel(), minlength=4).tolist(), got_b.tolist()))
    nf.same_class_and_values(got_w, dw, c.tag + " dw")
    nf.same_class_and_values(got_b, db, c.tag + " dbias")


@pytest.mark.parametrize("c", **_ids(nf.WGRAD))
def test_conv2d_wgrad(capi, cuda, c):
    x, gy = nf.wgrad_operands(c)
    assert capi.lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w) > 1
    lx, lgy = lr.padded(c.cin + 4, c.h, c.w, c.k // 2, 4), lr.padded(c.cout + 8, c.h, c.w, c.k // 2, 4)
    p = dict(lx=lx, lgy=lgy)
    p["xbuf"] = torch.from_numpy(wg_gpu.host_buffer(capi, lx, c.n, c.h, c.w, x, c.cin)).to(cuda)
    p["gbuf"] = torch.from_numpy(wg_gpu.host_buffer(capi, lgy, c.n, c.h, c.w, gy, 0)).to(cuda)
    _check_wgrad(c, *wg_gpu.wgrad(capi, cuda, c, p), x, gy)


@pytest.mark.parametrize("c", **_ids(nf.WGRAD))
def test_conv2d_wgrad_bf16(capi, cuda, c):
    x, gy = nf.wgrad_operands(c)
    assert capi.lib.rtpose_conv2d_wgrad_bf16_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w) > 1
    lx, lgy = lr.padded(c.cin + 8, c.h, c.w, c.k // 2, 8), lr.padded(c.cout + 16, c.h, c.w, c.k // 2, 8)
    p = dict(lx=lx, lgy=lgy)
    p["xbuf"] = wgb_gpu.to_device(_bf16_buffer(capi, lx, c.n, c.h, c.w, x, c.cin, True), cuda)
    p["gbuf"] = wgb_gpu.to_device(_bf16_buffer(capi, lgy, c.n, c.h, c.w, gy, c.cout, False), cuda)
    _check_wgrad(c, *wgb_gpu.wgrad(capi, cuda, c, p), x, gy)


# ---- the ReLU gradient ---------------------------------------------------------------------------------------------------------------
def test_relu_grad_pins_its_mask(capi, cuda):
    """out = y > 0 ? gy : +0 on the bits: a NaN y (either pattern) and -Inf give +0, +Inf passes gy; where y > 0, gy's bits
    pass untouched - NaN payloads and both Infs included."""
    n, ch, h, w = 2, 8, 5, 7
    g = torch.Generator().manual_seed(3)
    y, gy = nf.draw(g, n, ch, h, w), nf.draw(g, n, ch, h, w)
    nf.inject(y, [((0, 1, 1, 2), nf.NAN_BITS[0]), ((0, 2, 1, 2), nf.NAN_BITS[1]), ((1, 3, 2, 2), nf.PINF), ((1, 4, 2, 2), nf.NINF)])
    y[0, 5], y[1, 6] = 1.0, -1.0
    gy_bits = gy.numpy().view(np.uint32)
    for i, bits in enumerate(nf.NAN_BITS + (nf.PINF, nf.NINF)):
        gy_bits[0, 5, 0, i] = gy_bits[1, 6, 0, i] = gy_bits[0, 1 + i % 2, 1, 2] = bits      # under y > 0, y < 0 and a NaN y
    gy_bits[1, 3, 2, 2] = nf.NAN_BITS[1]                                                    # under y = +Inf
    ly, lg, lo = lr.padded(ch + 5, h, w, 1, 3), lr.padded(ch + 8, h, w, 3, 4), lr.padded(ch + 2, h, w, 2, 1)

    def buffer(lay, vals):
        a = np.full(cd.npx(capi, lay, n, h, w) * lay.cstride, np.nan, dtype=np.float32)
        return torch.from_numpy(lr.scatter(a, lay, vals)).to(cuda)
    ybuf, gbuf = buffer(ly, y.numpy()), buffer(lg, gy.numpy())
    obuf = torch.full((cd.npx(capi, lo, n, h, w) * lo.cstride,), cd.SENTINEL, dtype=torch.int32, device=cuda).view(torch.float32)
    capi.check(capi.lib.rtpose_relu_grad(capi.ptr(ybuf), C.byref(cd.L(capi, ly)), capi.ptr(gbuf), C.byref(cd.L(capi, lg)),
                                         capi.ptr(obuf), C.byref(cd.L(capi, lo)), ch, n, h, w, capi.current_stream()))
    torch.cuda.synchronize()
    bits, io = cd.np_bits(obuf), lr.index(lo, n, h, w, ch)
    got = np.transpose(bits[io], (0, 3, 1, 2))
    want = cb.relu_grad_bits(y.numpy(), gy_bits)
    assert want[0, 1, 1, 2] == 0 and want[0, 2, 1, 2] == 0 and want[1, 4, 2, 2] == 0 and want[1, 3, 2, 2] == nf.NAN_BITS[1]
    assert tuple(want[0, 5, 0, :4]) == nf.NAN_BITS + (nf.PINF, nf.NINF) and not want[1, 6].any()
    assert np.array_equal(got, want)
    assert lr.untouched(bits, io, cd.SENTINEL)


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------------
def _own_and_others(c, a):
    others = [i for i in range(c.channels) if i != c.channel]
    a = np.asarray(a)
    if a.ndim == 4:
        return a[:, c.channel], a[:, others]
    return (a[c.channel], a[others]) if a.ndim == 1 else (a[:, c.channel], a[:, others])


@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("c", **_ids(nf.BN))
def test_batchnorm(capi, cuda, c, relu, layout):
    n, h, w = nf.BN_SHAPE
    pair = (c.channels + 4, 4) if layout == "vector" else (c.channels + 3, 1)
    case = br.Case(c.channels, n, h, w, pair, pair, pair, "")
    assert br.is_vector(case) == (layout == "vector") and capi.lib.rtpose_bn_slabs(c.channels, n, h, w) > 1
    x0, gy0 = nf.chan_operands(c, nf.BN_SHAPE)
    x, gy = nf.chan_inject(c, x0, gy0, nf.BN_AT, nf.BN_AT)
    wt, b, rm, rv = br.affine(c.channels, True)
    r0 = bn_gpu.run(capi, cuda, case, x0, gy0, wt, b, rm, rv, relu)
    r = bn_gpu.run(capi, cuda, case, x, gy, wt, b, rm, rv, relu)
    t = br.bn64(x, gy, wt, b, rm, rv, relu=relu)
    # every other channel: the bits of the launch without the injection
    for k in ("save", "rm", "rv", "y", "dx", "dw", "db"):
        assert bn_gpu.same_bits(_own_and_others(c, r[k])[1], _own_and_others(c, r0[k])[1]), "%s of another channel changed" % k
    own = {k: _own_and_others(c, r[k])[0] for k in ("rm", "rv", "y", "dx", "dw", "db")}
    ref = {k: _own_and_others(c, t[name].numpy())[0] for k, name in (("rm", "running_mean"), ("rv", "running_var"), ("y", "y"), ("dx", "dx"),
                                                                       ("dw", "dweight"), ("db", "dbias"))}
    print("%s relu %s: rm %r rv %r dw %r db %r (float64: %r %r %r %r)" % (c.tag, relu, own["rm"], own["rv"], own["dw"], own["db"],
                                                                           ref["rm"], ref["rv"], ref["dw"], ref["db"]))
    def same_class(k, got, want):
        d = [m for m in nf.differences(got, want) if "finite elements differ" not in m or k == "db"]
        assert not d, "%s: %s" % (k, "; ".join(d))

    rows = ("mean", "var", "invstd", "scale", "shift")
    save_own, save_clean = r["save"][:5, c.channel], r0["save"][:5, c.channel]
    if c.into == "gy":
        # the forward does not see a gradient
        for k in ("y", "rm", "rv"):
            assert bn_gpu.same_bits(own[k], _own_and_others(c, r0[k])[0]), "a gradient changed %s" % k
        assert bn_gpu.same_bits(save_own, save_clean), "a gradient changed the saved statistics"
        # the ReLU passes the injected gradient only where its y is positive - in torch's threshold_backward as here
        live = not relu or t["y"].numpy()[(nf.BN_AT[0], c.channel) + nf.BN_AT[1:]] > 0
        same_class("db", own["db"], ref["db"])
        assert np.isfinite(ref["db"]) == (not live)
        if nf.chan_classes(c) == (nf.NAN,) or not live:
            same_class("dw", own["dw"], ref["dw"])
            same_class("dx", own["dx"], ref["dx"])
            assert not live or not (np.isfinite(ref["dx"]).any() or np.isfinite(ref["dw"]))
        else:
            # an Inf: dweight = invstd * (G2 - mdk * G1) of the shifted sums is torch's Inf, or Inf - Inf (header, rtpose_bn_grad);
            # dx is not held to torch
            assert not np.isfinite(ref["dw"]) and nf.classes(own["dw"])[()] in (nf.classes(ref["dw"])[()], nf.NAN)
            assert not np.isfinite(own["dx"]).all()
    else:
        for k in ("rm", "rv", "y"):
            same_class(k, own[k], ref[k])
            assert not np.isfinite(ref[k]).any()
        want_rows = np.array([t[k].numpy()[c.channel] for k in rows])
        assert np.array_equal(nf.classes(save_own), nf.classes(want_rows)), "saved %s: %r, float64 %r" % (rows, save_own, want_rows)
        if relu:
            # the pinned mask (header, rtpose_bn_grad): y is NaN in the whole channel and passes no gradient - dbias is +0, where
            # torch's threshold_backward passes gy under a NaN y; dweight and dx carry the NaN of the statistics
            assert own["db"].view(np.uint32) == 0 and np.isnan(own["dw"]) and np.isnan(own["dx"]).all()
        else:
            for k in ("dx", "dw", "db"):
                same_class(k, own[k], ref[k])
            assert np.isfinite(ref["db"]) and not np.isfinite(ref["dx"]).any() and not np.isfinite(ref["dw"])


def test_batchnorm_inf_at_the_first_pixel_gives_a_nan_mean(capi, cuda):
    """The documented difference (header, rtpose_bn_stats): the sums are shifted by K = x at pixel (0, 0, 0), so an Inf THERE
    makes every x - K NaN or -Inf and the mean NaN, where torch's mean is Inf; the variance is NaN on both sides."""
    c = nf.BN[1]
    assert c.tag == "c8-first-x-pinf"
    n, h, w = nf.BN_SHAPE
    case = br.Case(c.channels, n, h, w, (12, 4), (12, 4), (12, 4), "")
    x0, gy0 = nf.chan_operands(c, nf.BN_SHAPE)
    x, gy = nf.chan_inject(c, x0, gy0, (0, 0, 0), (0, 0, 0))
    wt, b, rm, rv = br.affine(c.channels, True)
    r0 = bn_gpu.run(capi, cuda, case, x0, None, wt, b, rm, rv, False)
    r = bn_gpu.run(capi, cuda, case, x, None, wt, b, rm, rv, False)
    t = br.bn64(x, gy, wt, b, rm, rv)
    assert np.isposinf(t["mean"].numpy()[c.channel]) and np.isnan(t["var"].numpy()[c.channel])
    assert np.isnan(r["save"][:5, c.channel]).all() and np.isnan(r["rm"][c.channel]) and np.isnan(r["rv"][c.channel])
    assert np.isnan(r["y"][:, c.channel]).all()
    for k in ("save", "rm", "rv", "y"):
        assert bn_gpu.same_bits(_own_and_others(c, r[k])[1], _own_and_others(c, r0[k])[1]), "%s of another channel changed" % k


# ---- the depthwise 3x3 ----------------------------------------------------------------------------------------------------------------
def _dw_forward(capi, dev, case, x, wt):
    lib = capi.lib
    ho, wo = dr.out_size(case.h, case.w, case.stride)
    lx, ly, _ = dr.layouts(case)
    xbuf = dw_gpu.to_dev(dw_gpu.slice_buffer(capi, lx, case.n, case.h, case.w, case.c, x.numpy()), dev)
    ybuf = dw_gpu.to_dev(dw_gpu.slice_buffer(capi, ly, case.n, ho, wo, case.c, zero_gaps=False), dev)
    w9 = torch.from_numpy(dr.tap_major(wt.numpy())).contiguous().to(dev)
    zero = torch.zeros(case.c, device=dev)
    capi.check(lib.rtpose_dwconv3x3(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(w9), capi.ptr(zero), capi.ptr(ybuf),
                                    C.byref(cd.L(capi, ly)), case.c, case.n, case.h, case.w, case.stride, capi.current_stream()),
               "rtpose_dwconv3x3")
    torch.cuda.synchronize()
    bits, idx = cd.np_bits(ybuf), lr.index(ly, case.n, ho, wo, case.c)
    assert lr.untouched(bits, idx, cd.SENTINEL), "the forward wrote outside the valid pixels of the slice"
    return np.ascontiguousarray(np.transpose(bits[idx], (0, 3, 1, 2))).view(np.float32)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", **_ids(nf.DW))
def test_dwconv3x3(capi, cuda, c, stride):
    n, h, w = nf.DW_SHAPE
    pair = (c.channels + 4, 4)
    case = dr.Case(n, c.channels, h, w, stride, pair, pair, pair, "")
    ho, wo = dr.out_size(h, w, stride)
    x0, gy0 = nf.chan_operands(c, nf.DW_SHAPE, (ho, wo))
    x, gy = nf.chan_inject(c, x0, gy0, nf.DW_AT_X, nf.DW_AT_GY)
    wt = nf.dw_weights(c.channels)
    y64, dx64, dw64 = (t.numpy() for t in dr.autograd64(x, wt, gy, stride))
    with np.errstate(invalid="ignore"):
        db64 = gy.double().numpy().sum((0, 2, 3))
    others = [i for i in range(c.channels) if i != c.channel]
    got, clean = {}, {}
    for into, xs, gs in ((got, x, gy), (clean, x0, gy0)):
        into["y"] = _dw_forward(capi, cuda, case, xs, wt)
        into["dx"] = dw_gpu.run_dgrad(capi, cuda, case, gs, wt)
        into["dw"], into["db"] = dw_gpu.run_wgrad(capi, cuda, case, xs, gs)
    print("%s stride %d: dw %r (float64 %r), dbias %r" % (c.tag, stride, got["dw"][c.channel].ravel(), dw64[c.channel].ravel(),
                                                          got["db"][c.channel]))
    for k, ref in (("y", y64), ("dx", dx64)):
        assert dw_gpu.same_bits(got[k][:, others], clean[k][:, others]), "%s of another channel changed" % k
        nf.same_class_and_values(got[k][:, c.channel], ref[:, c.channel], "%s %s" % (c.tag, k))
    for k, ref in (("dw", dw64), ("db", db64)):
        assert dw_gpu.same_bits(got[k][others], clean[k][others]), "%s of another channel changed" % k
        nf.same_class_and_values(got[k][c.channel], ref[c.channel], "%s %s" % (c.tag, k))


# ---- the two stride-2 stems ---------------------------------------------------------------------------------------------------------------
def test_conv7x7_s2_forward_carries_a_nan_pixel(cuda, train):
    x, wt, _ = nf.stem_operands(64, 7)
    nf.inject(x, [((1, 1, 4, 5), nf.NAN_BITS[1])])
    b = torch.arange(64).float() - 32
    want = F.conv2d(x.double(), wt.double(), b.double(), stride=2, padding=3).numpy()
    assert nf.holds_every_class(want, (nf.NAN,)) and np.isfinite(want[0]).all()
    y = train.conv7x7_s2(x.to(cuda), wt.to(cuda), b.to(cuda))
    nf.same_class_and_values(y.cpu().numpy(), want, "rtpose_conv7x7_s2")


@pytest.mark.parametrize("cout,k", [(64, 7), (24, 3)])
def test_stem_backward(cuda, train, cout, k):
    x, wt, gy = nf.stem_operands(cout, k)
    dw64, db64, dx64 = nf.stem_reference(x, wt, gy, k, k == 3)
    xd = x.to(cuda).requires_grad_(k == 3)
    wd = wt.to(cuda).requires_grad_(True)
    if k == 7:
        bd = torch.zeros(cout, device=cuda, requires_grad=True)
        y = train.conv7x7_s2(xd, wd, bd)
    else:
        y = train.conv3x3_s2(xd, wd)
    y.backward(gy.to(cuda))
    nf.same_class_and_values(wd.grad.cpu().numpy(), dw64, "stem k%d dW" % k)
    if k == 7:
        nf.same_class_and_values(bd.grad.cpu().numpy(), db64, "stem k7 dbias")
    else:
        nf.same_class_and_values(xd.grad.cpu().numpy(), dx64, "stem k3 dx")


# ---- fp32 -> bf16 conversions ---------------------------------------------------------------------------------------------------------------
def _nan_operands():
    """x [2, 8, 3, 5]: integers, and every pattern of NAN_INPUTS and NAN_BITS once in each of the 8 channels"""
    g = torch.Generator().manual_seed(5)
    x = nf.draw(g, 2, 8, 3, 5)
    pats = nf.NAN_INPUTS + nf.NAN_BITS
    u = x.numpy().view(np.uint32)
    for ch in range(8):
        for i, bits in enumerate(pats):
            u[i % 2, ch, (i + ch) % 3, (i * 2 + ch) % 5] = bits
    return x


def _check_bf16_words(got, x, what):
    u = x.numpy().view(np.uint32)
    nan = np.isnan(x.numpy())
    assert nan.sum() == 8 * 6
    assert np.array_equal(got[~nan], lr.bf16_rne(x.numpy())[~nan]), what + ": a finite value"
    ok = nf.is_bf16_nan_of_sign(got, u)
    bad = nan & ~ok
    assert not bad.any(), "%s: fp32 NaN %s became bf16 %s" % (what, ["%08x" % v for v in u[bad][:6]], ["%04x" % v for v in got[bad][:6]])


def test_conversions_to_bf16_keep_nan_a_nan_of_its_sign(capi, cuda):
    lib, x = capi.lib, _nan_operands()
    n, ch, h, w = x.shape
    stream = capi.current_stream()
    ld = lr.padded(16, h, w, 1, 8)
    idx = lr.index(ld, n, h, w, ch)

    def fresh(lay):
        return torch.full((cd.npx(capi, lay, n, h, w) * lay.cstride,), NAN16, dtype=torch.int16, device=cuda)

    def words(buf, index):
        return np.ascontiguousarray(np.transpose(cd.np_bits(buf.view(torch.bfloat16))[index], (0, 3, 1, 2)))
    xd = x.contiguous().to(cuda)
    dst = fresh(ld)
    capi.check(lib.rtpose_nchw_to_layout_bf16(capi.ptr(xd), capi.ptr(dst), C.byref(cd.L(capi, ld)), ch, ch, n, h, w, stream))
    torch.cuda.synchronize()
    _check_bf16_words(words(dst, idx), x, "rtpose_nchw_to_layout_bf16")
    assert lr.untouched(cd.np_bits(dst.view(torch.bfloat16)), idx, NAN16)

    ls = lr.padded(12, h, w, 1, 4)
    src = np.full(cd.npx(capi, ls, n, h, w) * ls.cstride, np.nan, dtype=np.float32)
    sd = torch.from_numpy(lr.scatter(src, ls, x.numpy())).to(cuda)
    dst = fresh(ld)
    capi.check(lib.rtpose_layout_f32_to_bf16(capi.ptr(sd), C.byref(cd.L(capi, ls)), capi.ptr(dst), C.byref(cd.L(capi, ld)), ch, ch, n, h, w,
                                             stream))
    torch.cuda.synchronize()
    _check_bf16_words(words(dst, idx), x, "rtpose_layout_f32_to_bf16")
    assert lr.untouched(cd.np_bits(dst.view(torch.bfloat16)), idx, NAN16)

    # split: hi = bf16(v) is the conversion; lo = bf16(v - hi) is NaN - NaN, a NaN of whatever sign the subtraction gives
    lsp = lr.padded(32, h, w, 1, 16)
    ih, il = lr.split_index(lsp, n, h, w, ch)
    dst = fresh(lsp)
    capi.check(lib.rtpose_nchw_to_layout_split(capi.ptr(xd), capi.ptr(dst), C.byref(cd.L(capi, lsp)), ch, ch, n, h, w, stream))
    torch.cuda.synchronize()
    hi, lo = words(dst, ih), words(dst, il)
    _check_bf16_words(hi, x, "rtpose_nchw_to_layout_split, hi")
    nan = np.isnan(x.numpy())
    assert (((lo[nan] & 0x7F80) == 0x7F80) & ((lo[nan] & 0x7F) != 0)).all(), "split lo of a NaN is no NaN"
    assert not lo[~nan].any(), "split lo of an integer"
    assert lr.untouched(cd.np_bits(dst.view(torch.bfloat16)), [ih, il], NAN16)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["input pixel", "hidden filter"])
@pytest.mark.parametrize("dt,resident", [("fp32", False), ("bf16", False), ("fp32", True), ("bf16", True)])
def test_a_nan_reaches_the_output_of_a_relu_chain(cuda, train, dt, resident, where):
    """conv3 + ReLU, conv7 + ReLU, conv1 through train.run_sequential: the output is class-equal to the torch modules in
    float64 (fp32: value-equal too; bf16 rounds the activations above 256, which the float64 modules do not)."""
    x, layers = nf.chain_operands()
    if where == "input pixel":
        nf.inject(x, [((1, 3, 2, 2), nf.NAN_BITS[0])])
    else:
        nf.inject(layers[1][0], [((4, 6, 3, 3), nf.NAN_BITS[1])])       # the centre tap: it meets no padding
    want = nf.chain_reference(x, layers)
    assert np.isnan(want).any() and (where == "hidden filter" or np.isfinite(want).any())
    mods = []
    for i, (wt, b) in enumerate(layers):
        m = nn.Conv2d(wt.shape[1], wt.shape[0], wt.shape[2], 1, wt.shape[2] // 2).to(cuda)
        m.weight, m.bias = nn.Parameter(wt.to(cuda)), nn.Parameter(b.to(cuda))
        mods += [m, nn.ReLU()] if i + 1 < len(layers) else [m]
    train.reset_bf16_fallbacks()
    y = train.run_sequential(nn.Sequential(*mods), x.to(cuda), compute_dtype=dt, resident=resident)
    got = y.detach().float().cpu().numpy()
    print("%s %s resident %s: %d NaN outputs of %d (float64: %d)" % (where, dt, resident, int(np.isnan(got).sum()), got.size,
                                                                     int(np.isnan(want).sum())))
    d = nf.differences(got, want)
    if dt == "bf16":
        d = [s for s in d if "finite elements differ" not in s]
    assert not d, "; ".join(d)
    assert train.bf16_fallbacks == {'fwd': 0, 'dgrad': 0}
