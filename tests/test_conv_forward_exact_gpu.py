"""The forward conv launchers against tests/conv_forward_exact.py, BIT FOR BIT: integer operands make every fp32 sum exact
in any order and every bf16 store the one rounding of an exact value (tests/test_conv_forward_exact_cpu.py asserts the
conditions), so the float64 reference is compared with == and one differing output is a wrong term, a dropped or doubled
pixel, a rounded operand, a stale tile or a wrong channel.

Per case: one launch into a sentinel-filled output at an odd stride and offset (where the launcher takes one: the bf16
vector stores, the channel planes and the stem want whole 16-byte pieces - there two different aligned places), one into
the network's aligned layout; every word outside the slices untouched, every word inside finite and == the reference; a
second launch into the same buffer gives the same bits; image 0 launched alone gives the bits it has in the batch.
The walk cases are sized from the device's CU count (fx.sized): 2.5 items per persistent block, a ragged last round.

The launchers with a cd.Form go through conv_driver (given, pack_all, to_layout, launch, outputs); rtpose_conv_first*,
rtpose_conv7x7_s2 and the pointwise pairs have none and are called bare."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import conv_driver as cd
import conv_forward_exact as fx
import layout_restate as lr

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC1                  # the sentinel of a bf16 buffer: a quiet NaN
TIMES = {}


@pytest.fixture(scope="module", autouse=True)
def _times_for_profiles():
    """the wall time of every case of this file, CPU reference included (written by conv_driver.note, for profiles/)"""
    yield
    slow = sorted(TIMES.items(), key=lambda kv: -kv[1])[:12]
    cd.note("conv_forward_exact_times.json", {"cases": len(TIMES), "total_s": round(sum(TIMES.values()), 2), "slowest": slow})


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _prepare(dev, c):
    """the case at this device's size with its operands and references; a walk case's conditions are asserted here"""
    c = fx.sized(c, _cus(dev))
    o = fx.operands(c)
    if c.walk is not None:
        r = fx.conditions(c, o)
        assert r.S < fx.LIMIT and r.share >= fx.MIN_SHARE and (not c.relu or r.clipped > 0)
        if "walk" in c.edges:
            blocks = fx.walk_blocks(c, _cus(dev))
            assert fx.walk_items(c) >= 2.5 * blocks and fx.walk_items(c) % blocks != 0
        else:
            g = fx.geometry(c, _cus(dev))
            assert 0 < g.nbig < g.total
    return c, o, fx.expected(c, o)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = got != want               # (NaN - an unwritten word - differs from everything)
    assert not bad.any(), "%s: %d of %d outputs differ from the exact reference, first at (n, c, y, x) %s: %r != %r" % (
        what, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def _timed(c, t0):
    TIMES["%s-%s" % (c.launcher, c.tag)] = round(time.time() - t0, 3)


# ---- launchers with a Form --------------------------------------------------------------------------------------------------------
def _policies(c):
    split = c.kind == "x3" and not c.out_f32
    if split:                                               # whole 8-channel [hi | lo] pieces
        return [cd.Out(8, 8, NAN16, 8), cd.Out(24, 16, NAN16, 8)]
    if c.kind == "f32" or c.out_f32:
        return [cd.sentinel(1, 3), cd.Out(16, 8, cd.SENTINEL)]
    if c.entry == "c64":                                    # 16-byte aligned slices only
        return [cd.Out(8, 8, NAN16), cd.Out(16, 16, NAN16)]
    return [cd.Out(3, 1, NAN16), cd.Out(16, 8, NAN16)]


def _hooks(capi, dev, c, o, P, policy, images):
    """(hook for cd.launch, cmaps for cd.outputs, tensors to keep alive) of a case's out_cmap / residual / pre-activation"""
    keep, cmaps = [], None
    if c.cmap:
        cmap = (policy.choff + o.cmap).to(torch.int32)              # absolute channels of the pixel
        keep.append(cmap.to(dev))
        cmaps = [cmap.numpy()]
    if c.x.get("preact"):
        cp = P.cin_p                                                # the padded channels: must be staged as 0 whatever these hold
        sc, sh = torch.full((cp,), -2.0), torch.full((cp,), 5.0)    # (inf_pad: 1 x 1.0 + inf = +inf, and inf x the zero tap
        if c.x.get("inf_pad"):                                      # is NaN, if a kernel pre-activated them)
            sc[c.cin:], sh[c.cin:] = 1.0, float("inf")
        sc[:c.cin], sh[:c.cin] = o.in_scale, o.in_shift
        keep += [sc.to(dev), sh.to(dev)]
    res = c.x.get("res")
    if res == "own":                                                # a layout of its own, NaN around the slice
        lres = lr.padded(c.cout + 5, c.h, c.w, 1, 3)
        host = np.full(cd.npx(capi, lres, images, c.h, c.w) * lres.cstride, np.nan, dtype=np.float32)
        lr.scatter(host, lres, o.res[:images].numpy())
        keep.append(torch.from_numpy(host).to(dev))
    n_keep = len(keep)

    def hook(gi, d, obuf, lout):
        i = 0
        if c.cmap:
            d.out_cmap = keep[i].data_ptr()
            i += 1
        if c.x.get("preact"):
            d.in_scale, d.in_shift = keep[i].data_ptr(), keep[i + 1].data_ptr()
            d.preact_cin = c.cin if P.cin_p != c.cin else 0
            i += 2
        if res == "own":
            d.residual, d.lres = keep[i].data_ptr(), cd.L(capi, lres)
        elif res == "inplace":                                      # the conv adds into the buffer it writes
            idx = torch.from_numpy(lr.index(lout, images, c.h, c.w, c.cout)).to(dev)
            obuf[idx] = o.res[:images].permute(0, 2, 3, 1).contiguous().to(dev)
            d.residual, d.lres = obuf.data_ptr(), cd.L(capi, lout)
        assert i <= n_keep
    need = c.cmap or c.x.get("preact") or res
    return (hook if need else None), cmaps, keep


def _form_case(capi, dev, case):
    t0 = time.time()
    c, o, want = _prepare(dev, case)
    form = cd.Form(c.kind, c.k, c.m, c.out_f32, c.entry)
    P = cd.pack_all(capi, dev, cd.given(form, [o.x], o.wts, o.biases, c.relu, c.pool, o.slopes))
    one = cd.given(form, [o.x[:1]], o.wts, o.biases, c.relu, c.pool, o.slopes)
    one.wp, one.bp, one.sl = P.wp, P.bp, P.sl

    def inputs(Q, x):
        buf, lay = cd.to_layout(capi, dev, Q, x, c.pad_in)
        if c.x.get("nan_pad"):                                      # NaN in the padded channels of every pixel, gaps included
            buf.view(-1, lay.cstride)[:, c.cin:] = float("nan")
        if c.x.get("inf_pad"):                                      # finite there, with in_shift = +inf (_hooks)
            buf.view(-1, lay.cstride)[:, c.cin:] = 1.0
        return [(buf, lay)] * c.groups
    inp = inputs(P, o.x)
    if c.entry == "c64":
        assert c.pad_in >= 1
    first = None
    for policy in _policies(c):
        hook, cmaps, keep = _hooks(capi, dev, c, o, P, policy, c.n)
        obuf, louts = cd.launch(capi, dev, P, inp, policy, c.pad_out, hook=hook)
        bits = cd.np_bits(obuf).copy()
        pieces = []
        outs = cd.outputs(P, obuf, louts, policy, cmaps=cmaps, pieces=pieces)
        for gi in range(c.groups):
            _same(outs[gi].numpy(), want[gi].numpy(), "%s branch %d" % (c.tag, gi))
        if pieces:                                                  # a split output: hi and lo each, not only their sum
            for gi, (hi, lo) in enumerate(fx.expected_pieces(c, o)):
                _same(pieces[gi][0], hi, "%s branch %d, hi words" % (c.tag, gi))
                _same(pieces[gi][1], lo, "%s branch %d, lo words" % (c.tag, gi))
        obuf2, _ = cd.launch(capi, dev, P, inp, policy, c.pad_out, hook=hook, into=obuf)
        assert np.array_equal(cd.np_bits(obuf2), bits), "a second launch into the same buffer gave other bits"
        first = first or (policy, outs)
    if c.n > 1:
        policy, outs = first
        hook, cmaps, keep = _hooks(capi, dev, c, o, one, policy, 1)
        obuf, louts = cd.launch(capi, dev, one, inputs(one, o.x[:1]), policy, c.pad_out, hook=hook)
        alone = cd.outputs(one, obuf, louts, policy, cmaps=cmaps)
        for gi in range(c.groups):
            assert torch.equal(alone[gi], outs[gi][:1]), "image 0 alone differs from image 0 of the batch"
    _timed(c, t0)


def _ids(name):
    return dict(argvalues=fx.EXACT_CASES[name], ids=[c.tag for c in fx.EXACT_CASES[name]])


@pytest.mark.parametrize("case", **_ids("conv2d"))
def test_conv2d_exact(capi, cuda, case):
    _form_case(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("conv2d_x"))
def test_conv2d_residual_and_preactivation_exact(capi, cuda, case):
    _form_case(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("conv2d_bf16"))
def test_conv2d_bf16_exact(capi, cuda, case):
    _form_case(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("c64"))
def test_conv3x3_c64_bf16_exact(capi, cuda, case):
    _form_case(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("conv2d_bf16x3"))
def test_conv2d_bf16x3_exact(capi, cuda, case):
    _form_case(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("wino2"))
def test_winograd_f2x2_3x3_exact(capi, cuda, case):
    if case.tag == "plain-grid":                 # (sized for 256 CUs or fewer: more 64-tile blocks than half the CUs, not more than CUs)
        assert fx.wino2_form(case, _cus(cuda)) == "plain"
    _form_case(capi, cuda, case)


@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
def test_a_fused_pool_of_an_odd_map_is_refused(capi, cuda, kind):
    """MaxPool2d(2, 2) drops the odd last row / column; the launchers have no such form and say so before any launch"""
    c = fx._c("conv2d", "pool-odd", 2, 7, 9, 16, 24, k=3, relu=1, pool=1, kind=kind, out_f32=kind != "f32")
    o = fx.operands(c)
    P = cd.pack_all(capi, cuda, cd.given(cd.Form(kind, 3, None, kind != "f32"), [o.x], o.wts, o.biases, 1, 1, o.slopes))
    buf, lay = cd.to_layout(capi, cuda, P, o.x, 1)
    with pytest.raises(capi.RtposeError, match="even H and W"):
        cd.launch(capi, cuda, P, [(buf, lay)], cd.sentinel(1, 3), 1)


# ---- bare launchers ---------------------------------------------------------------------------------------------------------------
def _fresh(dev, elems, bf16):
    if bf16:
        return torch.full((elems,), NAN16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return torch.full((elems,), cd.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _read(obuf, written, want):
    """[(offsets [n, h, w, c], reference [n, c, h, w])]: every written word == the reference, every other word untouched"""
    bits = cd.np_bits(obuf)
    bf16 = bits.dtype == np.uint16
    assert lr.untouched(bits, [idx for idx, _ in written], NAN16 if bf16 else cd.SENTINEL), "wrote outside its slice / into the gaps"
    for gi, (idx, _) in enumerate(written):
        v = lr.bf16_to_f32(bits[idx]) if bf16 else bits[idx].view(np.float32)
        _same(np.transpose(v, (0, 3, 1, 2)), want[gi].numpy()[:v.shape[0]], "branch %d" % gi)
    return bits.copy()


def _bare_case(capi, dev, case, run):
    """run(c, o, images, variant) -> (obuf, written, relaunch): the shared sequence of the bare launchers"""
    t0 = time.time()
    c, o, want = _prepare(dev, case)
    first = None
    for variant in (0, 1):
        obuf, written, again = run(c, o, c.n, variant)
        bits = _read(obuf, written, want)
        again()
        assert np.array_equal(cd.np_bits(obuf), bits), "a second launch into the same buffer gave other bits"
        first = first or [bits[idx] for idx, _ in written]
    if c.n > 1:
        obuf, written, _ = run(c, o, 1, 0)
        bits = _read(obuf, written, want)
        for (idx, _), batch in zip(written, first):
            assert np.array_equal(bits[idx], batch[:1]), "image 0 alone differs from image 0 of the batch"
    _timed(c, t0)


def _image_source(capi, dev, c, x, n):
    """(x_nchw, x_layout, lx) arguments of the first-layer launchers, and the tensors behind them"""
    lib = capi.lib
    xd = x[:n].contiguous().to(dev)
    if c.x["src"] == "nchw":
        return (capi.ptr(xd), None, None), [xd]
    lx = capi.Layout.padded(8, c.h, c.w, 1)
    xin = torch.zeros(lib.rtpose_layout_pixels(C.byref(lx), n, c.h, c.w) * 8, device=dev)
    capi.check(lib.rtpose_nchw_to_layout(capi.ptr(xd), capi.ptr(xin), C.byref(lx), 3, 8, n, c.h, c.w, capi.current_stream()))
    torch.cuda.synchronize()
    return (None, capi.ptr(xin), C.byref(lx)), [xin, lx]


def _first_layer(capi, dev, case):
    lib = capi.lib
    bf16, planes = case.launcher == "conv_first_bf16", case.launcher == "conv_first_planes"
    packed = {}

    def run(c, o, n, variant):
        if not packed:
            wd, bd = o.wts[0].to(dev), o.biases[0].to(dev)
            wp = torch.zeros(lib.rtpose_conv_first_packed_floats(), device=dev)
            pack = lib.rtpose_pack_conv_first_bf16 if bf16 else lib.rtpose_pack_conv_first
            capi.check(pack(capi.ptr(wd), capi.ptr(bd), capi.ptr(wp), capi.current_stream()))
            torch.cuda.synchronize()
            packed["w"] = wp
        src, keep = _image_source(capi, dev, c, o.x, n)
        # fp32 pixel-major: odd stride and offset, then the aligned layout; bf16 and planes: 8-channel pieces, two places
        cs, off = ((67, 1), (80, 8))[variant] if not (bf16 or planes) else ((80, 8), (72, 0))[variant]
        lo = lr.padded(cs, c.h, c.w, 1, off)
        q = cd.npx(capi, lo, n, c.h, c.w)
        qs = q + (7 if variant == 0 else 0)                       # slots per plane: more than the layout has pixels, then exactly
        obuf = _fresh(dev, (qs if planes else q) * cs, bf16)
        if planes:
            pix = lr.offsets(lr.Lay(1, 0, lo.ws, lo.hs, lo.lead), n, c.h, c.w)[..., None]
            ch = off + np.arange(64, dtype=np.int64)
            idx = ((ch >> 3) * qs + pix) * 8 + (ch & 7)
        else:
            idx = lr.index(lo, n, c.h, c.w, 64)

        def launch():
            args = src + (capi.ptr(packed["w"]), capi.ptr(obuf), C.byref(cd.L(capi, lo)))
            if planes:
                rc = lib.rtpose_conv_first_planes(*args, qs, c.relu, n, c.h, c.w, capi.current_stream())
            else:
                fn = lib.rtpose_conv_first_bf16 if bf16 else lib.rtpose_conv_first
                rc = fn(*args, c.relu, n, c.h, c.w, capi.current_stream())
            capi.check(rc, c.launcher)
            torch.cuda.synchronize()
        launch()
        return obuf, [(idx, keep)], launch
    _bare_case(capi, dev, case, run)


@pytest.mark.parametrize("case", **_ids("conv_first"))
def test_conv_first_exact(capi, cuda, case):
    _first_layer(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("conv_first_planes"))
def test_conv_first_planes_exact(capi, cuda, case):
    _first_layer(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("conv_first_bf16"))
def test_conv_first_bf16_exact(capi, cuda, case):
    _first_layer(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("conv7x7_s2"))
def test_conv7x7_s2_exact(capi, cuda, case):
    lib = capi.lib
    packed = {}

    def run(c, o, n, variant):
        if not packed:
            wd, bd = o.wts[0].to(cuda), o.biases[0].to(cuda)
            wp = torch.zeros(lib.rtpose_conv7x7_s2_packed_floats(), device=cuda)
            capi.check(lib.rtpose_pack_conv7x7_s2(capi.ptr(wd), capi.ptr(bd), capi.ptr(wp), capi.current_stream()))
            torch.cuda.synchronize()
            packed["w"] = wp
        src, keep = _image_source(capi, cuda, c, o.x, n)
        ho, wo = (c.h + 1) // 2, (c.w + 1) // 2
        cs, off = ((68, 4), (76, 8))[variant]                      # (cstride and choff multiples of 4: 16-byte pieces)
        lo = lr.padded(cs, ho, wo, 1, off)
        obuf = _fresh(cuda, cd.npx(capi, lo, n, ho, wo) * cs, False)

        def launch():
            capi.check(lib.rtpose_conv7x7_s2(*src, capi.ptr(packed["w"]), capi.ptr(obuf), C.byref(cd.L(capi, lo)), c.relu, n,
                                             c.h, c.w, capi.current_stream()), "rtpose_conv7x7_s2")
            torch.cuda.synchronize()
        launch()
        return obuf, [(lr.index(lo, n, ho, wo, 64), keep)], launch
    _bare_case(capi, cuda, case, run)


def _pair(capi, dev, case):
    lib = capi.lib
    bf16 = case.launcher == "pair_bf16"
    packed = {}

    def run(c, o, n, variant):
        mid = c.x["mid"]
        form = cd.Form("bf16" if bf16 else "f32", 1)
        if not packed:
            packed["p"] = [(cd.pack(capi, dev, form, o.wts[gi], o.biases[gi], 128), cd.pack(capi, dev, form, o.w2[gi], o.b2[gi], mid))
                           for gi in range(c.groups)]
        P = cd.given(form, [o.x[:n]], o.wts, o.biases, cin_pad=128)
        xin, lin = cd.to_layout(capi, dev, P, o.x[:n], c.pad_in)
        lmid = lr.padded(mid, c.h, c.w, 0)
        mids = _fresh(dev, cd.npx(capi, lmid, n, c.h, c.w) * mid, bf16)      # d1.out is ignored: stays untouched
        # the concat buffer's 38 | 19 split at odd offsets, then the stage's 192-channel layout
        cs, offs = ((2 * c.cout + 7, (3, 3 + c.cout)), (208, (128, 128 + c.cout)))[variant]
        out_bf16 = bf16 and not c.out_f32
        louts = [lr.padded(cs, c.h, c.w, c.pad_out, offs[gi]) for gi in range(c.groups)]
        obuf = _fresh(dev, cd.npx(capi, louts[0], n, c.h, c.w) * cs, out_bf16)
        d1, d2 = (capi.ConvDesc * c.groups)(), (capi.ConvDesc * c.groups)()
        for gi in range(c.groups):
            (w1, b1), (w2, b2) = packed["p"][gi]
            a, b = d1[gi], d2[gi]
            a.inp, a.w_packed, a.bias_packed, a.out = xin.data_ptr(), w1.data_ptr(), b1.data_ptr(), mids.data_ptr()
            a.lin, a.lout = cd.L(capi, lin), cd.L(capi, lmid)
            a.cin, a.cout, a.k, a.relu = 128, mid, 1, 1
            b.inp, b.w_packed, b.bias_packed, b.out = mids.data_ptr(), w2.data_ptr(), b2.data_ptr(), obuf.data_ptr()
            b.lin, b.lout = cd.L(capi, lmid), cd.L(capi, louts[gi])
            b.cin, b.cout, b.k = mid, c.cout, 1
        fits = lib.rtpose_conv1x1_pair_bf16_fits if bf16 else lib.rtpose_conv1x1_pair_fits
        assert fits(d1, d2, c.groups) == 1

        def launch():
            if bf16:
                rc = lib.rtpose_conv1x1_pair_bf16(d1, d2, c.groups, n, c.h, c.w, int(c.out_f32), capi.current_stream())
            else:
                rc = lib.rtpose_conv1x1_pair(d1, d2, c.groups, n, c.h, c.w, capi.current_stream())
            capi.check(rc, c.launcher)
            torch.cuda.synchronize()
            assert lr.untouched(cd.np_bits(mids), [], NAN16 if bf16 else cd.SENTINEL), "the ignored d1.out was written"
        launch()
        return obuf, [(lr.index(lo, n, c.h, c.w, c.cout), (xin, mids, d1, d2)) for lo in louts], launch
    _bare_case(capi, dev, case, run)


@pytest.mark.parametrize("case", **_ids("pair"))
def test_conv1x1_pair_exact(capi, cuda, case):
    _pair(capi, cuda, case)


@pytest.mark.parametrize("case", **_ids("pair_bf16"))
def test_conv1x1_pair_bf16_exact(capi, cuda, case):
    _pair(capi, cuda, case)
