"""GPU suite of the stacked hourglass (hourglass.HourglassNet, rtpose_hourglass_create): the native forward against the
reference's golden maps and the CPU restatement, and the kernels it added - residual epilogue and input pre-activation of
the 1x1 conv, the 7x7 stride-2 stem, upsample-add - through the C ABI against torch on the CPU."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_driver as cd  # noqa: E402
import hourglass_restate as R  # noqa: E402
import layout_restate as lr  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "hourglass_small.npz")
# (num_stacks, num_blocks, gain of the residual branches): the fixture's configurations
CONFIGS = ((8, 1, R.BRANCH_GAIN), (2, 1, R.BRANCH_GAIN), (2, 2, R.BRANCH_GAIN), (1, 1, R.STRONG_GAIN))


@pytest.fixture(scope="module")
def hgm(pkg):
    return importlib.import_module(pkg.__name__ + ".hourglass")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _model(hgm, stacks, blocks, seed, gain=R.BRANCH_GAIN, winograd3=None):
    m = hgm.hg(num_stacks=stacks, num_blocks=blocks, paf_classes=38, ht_classes=19)
    sd = R.seeded_state_dict(R.state_dict_spec(stacks, blocks, 38, 19), seed, gain)
    m.load_state_dict(sd)
    if winograd3 is not None:
        m.set_winograd(winograd3)
    return m.cuda().eval(), sd


def _check(outs, refs, what):
    for i, (a, b) in enumerate(zip(outs, refs)):
        b = torch.as_tensor(b)
        mx = b.abs().max().item()
        assert 0.1 <= mx <= 100.0, "%s: map %d max|value| %g (vanishing / exploding maps)" % (what, i, mx)
        err = (a.cpu() - b).abs().max().item()
        print("%s: map %d max abs err %.3g (ref max %.3g, bound %.3g)" % (what, i, err, mx, 1e-3 * max(1.0, mx)))
        assert err <= 1e-3 * max(1.0, mx), "%s: map %d max abs err %g (ref max %g)" % (what, i, err, mx)


@pytest.mark.parametrize("cfg", CONFIGS, ids=["s%d_b%d" % c[:2] for c in CONFIGS])
def test_forward_matches_the_reference_golden_maps(hgm, gold, cuda, cfg):
    stacks, blocks, gain = cfg
    tag = "s%d_b%d" % (stacks, blocks)
    assert float(gold[tag + "_gain"]) == gain
    m, _ = _model(hgm, stacks, blocks, int(gold["seed"]), gain)
    with torch.no_grad():
        (paf, heat), saved = m(torch.from_numpy(gold["x"]).to(cuda))
    assert saved[0] is paf and saved[1] is heat and paf.shape[1] == 38 and heat.shape[1] == 19
    _check([paf, heat], [gold[tag + "_paf"], gold[tag + "_heat"]], tag)


@pytest.mark.parametrize("shape", [(2, 3, 64, 128), (3, 3, 128, 192)], ids=["64x128", "128x192"])
@pytest.mark.parametrize("w3", [0, 1, 4, 'auto'])
def test_every_3x3_form_matches_the_restatement(hgm, cuda, w3, shape):
    m, sd = _model(hgm, 2, 1, 11, winograd3=w3)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(5)) - 0.5
    with torch.no_grad():
        (paf, heat), _ = m(x.to(cuda))
        ref = R.forward(sd, x, 2, 1)
    forms = {f for _, f, _ in m.conv_numerics(m.plan_for(x.to(cuda)))}
    want = {0: {0}, 1: {0, 3}, 4: {0, 43}, 'auto': {0, 43, 3}}[w3]
    assert forms <= want and (w3 == 0 or forms - {0}), (w3, forms)
    _check([paf, heat], ref, "winograd3=%s %s" % (w3, shape))


def test_every_stack_is_kept_under_keep_intermediates(hgm, cuda):
    """Three stacks with branches eight times the fixtures' gain: every stack's maps (read_output 2 + 2 s / 3 + 2 s) against the
    restatement, so that a wrong hand-over shows in the stack behind it."""
    m, sd = _model(hgm, 3, 1, 7, gain=0.05)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(6)) - 0.5
    with torch.no_grad():
        plan = m.forward_native(x.to(cuda), keep_intermediates=True)
        outs = [m.read_output(plan, i) for i in range(2 + 2 * 3)]
        ref = R.forward(sd, x, 3, 1, all_stacks=True)
    _check(outs[:2], ref[-1], "last stack")
    for s in range(3):
        _check(outs[2 + 2 * s:4 + 2 * s], ref[s], "stack %d" % s)


def test_a_16_image_384_batch_of_8_stacks_matches_the_restatement(hgm, cuda):
    m, sd = _model(hgm, 8, 1, 3)
    x = torch.rand(16, 3, 384, 384, generator=torch.Generator().manual_seed(8)) - 0.5
    with torch.no_grad():
        (paf, heat), _ = m(x.to(cuda))
        for i in (0, 15):
            ref = R.forward(sd, x[i:i + 1], 8, 1)
            _check([paf[i:i + 1], heat[i:i + 1]], ref, "image %d" % i)


def test_graph_replay_gives_the_bits_of_the_plain_forward(hgm, capi, cuda, monkeypatch):
    """RTPOSE_GRAPH=1: the first forward runs directly, the later ones replay the captured launch list (the stem then
    reads the plan's own input buffer; every buffer a launch adds into is rewritten earlier in the same list)."""
    lib = capi.lib
    x = (torch.rand(3, 3, 64, 128, generator=torch.Generator().manual_seed(21)) - 0.5).to(cuda)
    y = (torch.rand(3, 3, 64, 128, generator=torch.Generator().manual_seed(22)) - 0.5).to(cuda)
    ref = None
    for graph in ("0", "1"):
        monkeypatch.setenv("RTPOSE_GRAPH", graph)
        m, _ = _model(hgm, 2, 1, 11)
        with torch.no_grad():
            outs = [m(t)[0] for t in (x, y, x, y)]
        plan = m.plan_for(x)
        assert lib.rtpose_net_graph_active(plan.handle) == int(graph)
        assert m.device_status(plan) == 0
        assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[1][1], outs[3][1])
        assert not torch.equal(outs[0][0], outs[1][0])
        if ref is None:
            ref = outs
        else:
            for a, b in zip(outs, ref):
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("paf,heat", [(14, 9), (16, 8), (64, 64), (1, 1)])
def test_other_class_counts_match_the_restatement(hgm, cuda, paf, heat):
    """The score buffer is [PAF | pad to 8 | heat | pad to 8] and paf_score_ / ht_score_ read the pads as zero taps:
    counts with a pad, without one, the largest and the smallest, two stacks so that the hand-over reads them."""
    m = hgm.hg(num_stacks=2, num_blocks=1, paf_classes=paf, ht_classes=heat)
    sd = R.seeded_state_dict(R.state_dict_spec(2, 1, paf, heat), 13, gain=0.05)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(7)) - 0.5
    with torch.no_grad():
        plan = m.forward_native(x.to(cuda), keep_intermediates=True)
        outs = [m.read_output(plan, i) for i in range(6)]
        ref = R.forward(sd, x, 2, 1, all_stacks=True)
    assert outs[0].shape[1] == paf and outs[1].shape[1] == heat
    _check(outs[:2], ref[-1], "%d / %d last stack" % (paf, heat))
    for s in range(2):
        _check(outs[2 + 2 * s:4 + 2 * s], ref[s], "%d / %d stack %d" % (paf, heat, s))


def test_an_images_maps_are_the_same_bits_in_every_batch_size(hgm, cuda):
    m, _ = _model(hgm, 2, 1, 3)
    x = (torch.rand(12, 3, 128, 192, generator=torch.Generator().manual_seed(9)) - 0.5).to(cuda)
    with torch.no_grad():
        ref = {}
        for i in (0, 4, 11):
            (p, h), _ = m(x[i:i + 1])
            ref[i] = [p.clone(), h.clone()]
        for n in (5, 12):
            (p, h), _ = m(x[:n])
            for i, r in ref.items():
                if i < n:
                    assert torch.equal(p[i:i + 1], r[0]) and torch.equal(h[i:i + 1], r[1]), (n, i)


def test_a_forward_does_not_depend_on_what_an_earlier_one_left(hgm, capi, cuda):
    """The score maps live in one buffer whose pad channels paf_score_ / ht_score_ read as zero taps, and every stack
    adds into buffers the stack before wrote.  After a forward on a NaN input and with NaN written into both output
    slices, the next batch on the same plan gives the bits of a fresh plan."""
    lib = capi.lib
    x = (torch.rand(2, 3, 64, 128, generator=torch.Generator().manual_seed(4)) - 0.5).to(cuda)
    bad = x.clone()
    bad[0, :, 10:20, 10:20] = float('nan')
    bad[1] = float('nan')
    m1, _ = _model(hgm, 2, 1, 11)
    m2, _ = _model(hgm, 2, 1, 11)
    with torch.no_grad():
        m1(bad)
        plan = m1.plan_for(x)
        for which in (0, 1):
            base, lay, c, hh, ww = m1.output_view(plan, which)
            z = torch.zeros(x.shape[0], hh, ww, c, device=cuda)
            capi.check(lib.rtpose_layout_axpby(base, C.byref(lay), capi.ptr(z), c, x.shape[0], hh, ww, 0.0,
                                               float('nan'), None))
        assert torch.isnan(m1.read_output(plan, 0)).all() and torch.isnan(m1.read_output(plan, 1)).all()
        (p1, h1), _ = m1(x)
        (p2, h2), _ = m2(x)
    assert not torch.isnan(p1).any() and not torch.isnan(h1).any()
    assert torch.equal(p1, p2) and torch.equal(h1, h2)


# ---- kernels --------------------------------------------------------------------------------------------------------
def _sentinel(capi, cuda, lay, n, h, w):
    """a buffer of layout `lay` for n images of h x w, every word cd.SENTINEL (a NaN with a recognisable payload)"""
    words = capi.lib.rtpose_layout_pixels(C.byref(lay), n, h, w) * lay.cstride
    return torch.full((words,), cd.SENTINEL, dtype=torch.int32, device=cuda).view(torch.float32)


def _only_the_slice_was_written(buf, lay, c, n, h, w):
    """every word of `buf` outside the c channels of the n x h x w valid pixels of `lay` still holds cd.SENTINEL, bit for bit"""
    l = lr.Lay(lay.cstride, lay.choff, lay.ws, lay.hs, lay.lead)
    return lr.untouched(cd.np_bits(buf), lr.index(l, n, h, w, c), cd.SENTINEL)


def _to_layout(capi, cuda, x, lay, cpad=None, fill=0.0, sentinel=False):
    """NCHW CPU tensor -> device buffer of layout `lay` (slice at lay.choff); the rest of the buffer holds `fill`, or
    cd.SENTINEL."""
    lib = capi.lib
    n, c, h, w = x.shape
    if sentinel:
        buf = _sentinel(capi, cuda, lay, n, h, w)
    else:
        buf = torch.full((lib.rtpose_layout_pixels(C.byref(lay), n, h, w) * lay.cstride,), fill, device=cuda)
    xd = x.to(cuda).contiguous()
    capi.check(lib.rtpose_nchw_to_layout(capi.ptr(xd), capi.ptr(buf), C.byref(lay), c, cpad or c, n, h, w, None))
    torch.cuda.synchronize()
    return buf


def _from_layout(capi, cuda, buf, lay, c, n, h, w):
    out = torch.empty(n, c, h, w, device=cuda)
    capi.check(capi.lib.rtpose_layout_to_nchw(capi.ptr(buf), C.byref(lay), capi.ptr(out), c, n, h, w, None))
    torch.cuda.synchronize()
    return out.cpu()


def _packed(capi, cuda, wt, b, cin_packed):
    return cd.pack(capi, cuda, cd.Form("f32", 1), wt, b, cin_packed)


# the kernel a case reaches depends on the grid against the device's CUs; named here for the MI355X's 256
@pytest.mark.parametrize("n,h,w,cin,cout", [
    (2, 21, 17, 128, 256),     # strips, every tile split in halves
    (1, 6, 6, 128, 256),       # the smallest map of a 384 x 384 forward: one partial tile
    (16, 96, 96, 128, 256),    # 1152 m tiles x 4 column tiles: the XCD-aware order
    (3, 24, 24, 256, 38),      # padded columns (a score head's count)
    (2, 12, 20, 40, 256),      # cin not a multiple of 16: 8-channel chunks (paf_score_)
    (1, 10, 136, 64, 128),     # wider than a strip: 2-D tiles
])
def test_residual_epilogue_with_its_own_buffer_and_in_place(capi, cuda, n, h, w, cin, cout):
    lib, L = capi.lib, capi.Layout
    g = torch.Generator().manual_seed(n * 1000 + h)
    x = torch.rand(n, cin, h, w, generator=g) - 0.5
    r = torch.randn(n, cout, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x, wt, b) + r
    lin = L.padded(cin, h, w, 0)
    xin = _to_layout(capi, cuda, x, lin)
    wp, bp = _packed(capi, cuda, wt, b, cin)
    lres = L.padded(cout + 12, h, w, 1, choff=8)      # a layout of its own
    lout = L.padded(cout + 5, h, w, 0, choff=3)       # odd stride, offset slice

    def launch(out_buf, lo, res_buf, lr):
        d = capi.ConvDesc()
        d.inp, d.w_packed, d.bias_packed, d.out = xin.data_ptr(), wp.data_ptr(), bp.data_ptr(), out_buf.data_ptr()
        d.lin, d.lout, d.cin, d.cout, d.k = lin, lo, cin, cout, 1
        d.residual, d.lres = res_buf.data_ptr(), lr
        capi.check(lib.rtpose_conv2d(C.byref(d), 1, n, h, w, None), "rtpose_conv2d")
        torch.cuda.synchronize()
    res = _to_layout(capi, cuda, r, lres)
    before = res.clone()
    out = _sentinel(capi, cuda, lout, n, h, w)
    launch(out, lout, res, lres)
    got = _from_layout(capi, cuda, out, lout, cout, n, h, w)
    assert torch.equal(res, before), "the residual buffer was written"
    assert _only_the_slice_was_written(out, lout, cout, n, h, w), "wrote outside its slice"
    err = (got - ref).abs().max().item()
    assert err <= 2e-4 * max(1.0, ref.abs().max().item()), err
    # residual == out: the conv adds into the buffer; the same arithmetic, so the same bits
    acc = _to_layout(capi, cuda, r, lout, sentinel=True)
    launch(acc, lout, acc, lout)
    got2 = _from_layout(capi, cuda, acc, lout, cout, n, h, w)
    assert torch.equal(got2, got)
    assert _only_the_slice_was_written(acc, lout, cout, n, h, w), "wrote outside its slice"


@pytest.mark.parametrize("n,h,w,cin,cout,relu", [
    (2, 21, 17, 256, 128, 1),    # conv1 of a Bottleneck
    (1, 6, 6, 64, 64, 1),
    (4, 48, 48, 21, 64, 0),      # 21 real channels in a 24-channel slice: 8-channel chunks, 3 padded channels
    (2, 12, 20, 37, 128, 1),     # 37 in 40
    (1, 10, 136, 128, 128, 1),   # 2-D tiles
])
def test_pre_activated_1x1_conv(capi, cuda, n, h, w, cin, cout, relu):
    """relu(scale * x + shift) in front of the conv: negative scales, and - where the slice is padded - NaN in the
    padded channels of the input buffer with a negative scale and a positive shift there: they must stay zero taps."""
    lib, L = capi.lib, capi.Layout
    g = torch.Generator().manual_seed(n * 1000 + cin)
    cp = (cin + 7) // 8 * 8
    x = torch.rand(n, cin, h, w, generator=g) * 4 - 2
    sc = torch.rand(cin, generator=g) * 3 - 1.5
    sh = torch.randn(cin, generator=g) * 0.5
    assert (sc < 0).any() and (sc > 0).any()
    wt = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    ref = F.conv2d(a, wt, b)
    if relu:
        ref = F.relu(ref)
    assert (a == 0).any() and (a > 0).any()
    lin = L.padded(cp + 8, h, w, 0, choff=4)
    xin = _to_layout(capi, cuda, x, lin, fill=float('nan') if cp != cin else 0.0)   # NaN in the padded channels (and beyond)
    scp, shp = torch.full((cp,), -2.0), torch.full((cp,), 5.0)
    scp[:cin], shp[:cin] = sc, sh
    scd, shd = scp.to(cuda), shp.to(cuda)
    wp, bp = _packed(capi, cuda, wt, b, cp)
    lout = L.padded(cout + 5, h, w, 0, choff=3)
    out = _sentinel(capi, cuda, lout, n, h, w)
    d = capi.ConvDesc()
    d.inp, d.w_packed, d.bias_packed, d.out = xin.data_ptr(), wp.data_ptr(), bp.data_ptr(), out.data_ptr()
    d.lin, d.lout, d.cin, d.cout, d.k, d.relu = lin, lout, cp, cout, 1, relu
    d.in_scale, d.in_shift, d.preact_cin = scd.data_ptr(), shd.data_ptr(), cin if cp != cin else 0
    capi.check(lib.rtpose_conv2d(C.byref(d), 1, n, h, w, None), "rtpose_conv2d")
    torch.cuda.synchronize()
    got = _from_layout(capi, cuda, out, lout, cout, n, h, w)
    assert not torch.isnan(got).any(), "a padded input channel reached the sum"
    assert _only_the_slice_was_written(out, lout, cout, n, h, w), "wrote outside its slice"
    err = (got - ref).abs().max().item()
    assert err <= 2e-4 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("n,h,w", [(2, 44, 52), (1, 42, 70), (2, 150, 36), (1, 43, 33), (1, 128, 192)])
@pytest.mark.parametrize("src", ["nchw", "layout"])
def test_stem_7x7_stride_2(capi, cuda, n, h, w, src):
    """even and odd H / 2, tiles ragged in both directions (32 x 16 output pixels per tile), from the NCHW image and from
    an NHWC8 layout buffer"""
    lib, L = capi.lib, capi.Layout
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.rand(n, 3, h, w, generator=g) - 0.5
    wt = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    b = torch.randn(64, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, wt, b, stride=2, padding=3))
    ho, wo = ref.shape[2:]
    assert (ho, wo) == ((h + 1) // 2, (w + 1) // 2)
    wp = torch.zeros(lib.rtpose_conv7x7_s2_packed_floats(), device=cuda)
    wd, bd = wt.to(cuda), b.to(cuda)
    capi.check(lib.rtpose_pack_conv7x7_s2(capi.ptr(wd), capi.ptr(bd), capi.ptr(wp), None))
    lout = L.padded(64 + 12, ho, wo, 1, choff=8)
    out = _sentinel(capi, cuda, lout, n, ho, wo)
    if src == "nchw":
        xd = x.to(cuda)
        capi.check(lib.rtpose_conv7x7_s2(capi.ptr(xd), None, None, capi.ptr(wp), capi.ptr(out), C.byref(lout), 1, n, h, w,
                                         None))
    else:
        lx = L.padded(8, h, w, 1)
        xin = _to_layout(capi, cuda, x, lx, cpad=8)
        capi.check(lib.rtpose_conv7x7_s2(None, capi.ptr(xin), C.byref(lx), capi.ptr(wp), capi.ptr(out), C.byref(lout), 1,
                                         n, h, w, None))
    torch.cuda.synchronize()
    got = _from_layout(capi, cuda, out, lout, 64, n, ho, wo)
    assert _only_the_slice_was_written(out, lout, 64, n, ho, wo), "wrote outside its slice"
    assert (ref == 0).any() and (ref > 0).any()
    err = (got - ref).abs().max().item()
    assert err <= cd.STEM7_TOL * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("n,hl,wl,c", [(1, 3, 5, 256), (4, 24, 20, 256), (2, 48, 48, 64)])
def test_upsample_add_is_bit_exact_and_stays_in_its_slice(capi, cuda, n, hl, wl, c):
    lib, L = capi.lib, capi.Layout
    g = torch.Generator().manual_seed(hl)
    h, w = 2 * hl, 2 * wl
    up, low = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, hl, wl, generator=g)
    ref = up + F.interpolate(low, scale_factor=2, mode='nearest')
    lup, llow, lout = L.padded(c + 8, h, w, 1, choff=4), L.padded(c, hl, wl, 0), L.padded(c + 12, h, w, 0, choff=8)
    ub, lb = _to_layout(capi, cuda, up, lup, sentinel=True), _to_layout(capi, cuda, low, llow)
    out = _sentinel(capi, cuda, lout, n, h, w)
    capi.check(lib.rtpose_upsample2_add(capi.ptr(ub), C.byref(lup), capi.ptr(lb), C.byref(llow), capi.ptr(out),
                                        C.byref(lout), c, n, h, w, None))
    torch.cuda.synchronize()
    got = _from_layout(capi, cuda, out, lout, c, n, h, w)
    assert torch.equal(got, ref)
    assert _only_the_slice_was_written(out, lout, c, n, h, w), "wrote outside its slice"
    # in place on `up`, as the plan runs it
    capi.check(lib.rtpose_upsample2_add(capi.ptr(ub), C.byref(lup), capi.ptr(lb), C.byref(llow), capi.ptr(ub),
                                        C.byref(lup), c, n, h, w, None))
    torch.cuda.synchronize()
    got = _from_layout(capi, cuda, ub, lup, c, n, h, w)
    assert torch.equal(got, ref)
    assert _only_the_slice_was_written(ub, lup, c, n, h, w), "wrote outside its slice"


def test_launchers_without_the_new_fields_refuse_them(capi, cuda):
    lib = capi.lib
    v = torch.ones(512, device=cuda)
    buf = torch.zeros(1 << 20, device=cuda)

    def desc(k, cin, cout, pad, **kw):
        d = capi.ConvDesc()
        d.inp = d.w_packed = d.bias_packed = d.out = buf.data_ptr()
        d.lin = capi.Layout.padded(cin, 8, 8, pad)
        d.lout = capi.Layout.padded(cout, 8, 8, pad)
        d.cin, d.cout, d.k = cin, cout, k
        for key, val in kw.items():
            setattr(d, key, val)
        return d
    res = dict(residual=buf.data_ptr(), lres=capi.Layout.padded(128, 8, 8, 0))
    pre = dict(in_scale=v.data_ptr(), in_shift=v.data_ptr())

    def refused(rc, phrase, who):
        assert rc == -1 and phrase in capi.last_error(), (who, rc, capi.last_error())
    for kw, phrase in ((res, "residual"), (pre, "pre-activation")):
        d = desc(3, 128, 128, 3, **kw)
        refused(lib.rtpose_conv2d(C.byref(d), 1, 1, 8, 8, None), phrase, "direct 3x3")
        refused(lib.rtpose_conv2d_bf16(C.byref(d), 1, 1, 8, 8, 0, None), phrase, "bf16")
        refused(lib.rtpose_conv2d_bf16x3(C.byref(d), 1, 1, 8, 8, 0, None), phrase, "bf16x3")
        for m_ in (2, 4):
            d.wino_m = m_
            assert lib.rtpose_conv2d_winograd_fits(C.byref(d), 1, 8, 8) == 0
            refused(lib.rtpose_conv2d_winograd(C.byref(d), 1, 1, 8, 8, None), phrase, "F(%dx%d,3x3)" % (m_, m_))
        d7 = desc(7, 128, 128, 3, wino_m=6, **kw)
        refused(lib.rtpose_conv2d_winograd(C.byref(d7), 1, 1, 8, 8, None), phrase, "F(6,7)")
        d7.wino_m = 0
        refused(lib.rtpose_conv2d(C.byref(d7), 1, 1, 8, 8, None), phrase, "direct 7x7")
        d64 = desc(3, 64, 64, 1, **kw)
        assert lib.rtpose_conv3x3_c64_bf16_fits(C.byref(d64), 1, 1, 8, 8) == 0
        refused(lib.rtpose_conv3x3_c64_bf16(C.byref(d64), 1, 8, 8, None), phrase, "c64 bf16")
        d1, d2 = desc(1, 128, 128, 0, relu=1), desc(1, 128, 38, 0)
        assert lib.rtpose_conv1x1_pair_fits(C.byref(d1), C.byref(d2), 1) == 1
        d2 = desc(1, 128, 38, 0, **kw)
        assert lib.rtpose_conv1x1_pair_fits(C.byref(d1), C.byref(d2), 1) == 0
        refused(lib.rtpose_conv1x1_pair(C.byref(d1), C.byref(d2), 1, 1, 8, 8, None), phrase, "1x1 pair")
        assert lib.rtpose_conv1x1_pair_bf16_fits(C.byref(d1), C.byref(d2), 1) == 0
        refused(lib.rtpose_conv1x1_pair_bf16(C.byref(d1), C.byref(d2), 1, 1, 8, 8, 0, None), phrase, "1x1 pair bf16")
    # ... and the 1x1 kernel that has them refuses what it does not do with them
    refused(lib.rtpose_conv2d(C.byref(desc(1, 128, 128, 0, relu=1, **res)), 1, 1, 8, 8, None), "residual", "relu")
    refused(lib.rtpose_conv2d(C.byref(desc(1, 128, 128, 0, out_cmap=buf.data_ptr(), **res)), 1, 1, 8, 8, None),
            "residual", "out_cmap")
    refused(lib.rtpose_conv2d(C.byref(desc(1, 128, 128, 0, in_scale=v.data_ptr())), 1, 1, 8, 8, None), "pre-activation",
            "scale without shift")
    refused(lib.rtpose_conv2d(C.byref(desc(1, 128, 128, 0, preact_cin=200, **pre)), 1, 1, 8, 8, None), "preact_cin",
            "preact_cin")
    small = dict(residual=buf.data_ptr(), lres=capi.Layout.padded(100, 8, 8, 0))
    refused(lib.rtpose_conv2d(C.byref(desc(1, 128, 128, 0, **small)), 1, 1, 8, 8, None), "residual", "lres extent")
    lay = capi.Layout.padded(64, 8, 8, 0)
    assert lib.rtpose_upsample2_add(capi.ptr(buf), C.byref(lay), capi.ptr(buf), C.byref(lay), capi.ptr(buf), C.byref(lay),
                                    64, 1, 7, 8, None) == -1 and "even" in capi.last_error()
    assert lib.rtpose_upsample2_add(capi.ptr(buf), C.byref(lay), capi.ptr(buf), C.byref(lay), capi.ptr(buf), C.byref(lay),
                                    62, 1, 8, 8, None) == -1 and "16-byte" in capi.last_error()
    l60 = capi.Layout.padded(60, 8, 8, 0)
    assert lib.rtpose_conv7x7_s2(capi.ptr(buf), None, None, capi.ptr(buf), capi.ptr(buf), C.byref(l60), 1, 1, 16, 16,
                                 None) == -1 and "64-channel" in capi.last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


# ---- decoder path ---------------------------------------------------------------------------------------------------
def test_pose_estimator_records_match_the_oracle_and_the_pipelined_path(hgm, pkg, cuda):
    from oracle import post_oracle
    dec = importlib.import_module(pkg.__name__ + ".decode")
    synth = importlib.import_module(pkg.__name__ + ".synth")
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    m, _ = _model(hgm, 2, 1, 3)
    B, S = 4, 256
    cfg = dec.default_config()
    cfg.MODEL.DOWNSAMPLE = 4

    def batch(r):
        g = torch.Generator().manual_seed(500 + r)
        rng = np.random.default_rng(600 + r)
        hs, ps = [], []
        for _ in range(B):
            people = synth.random_people(rng, int(rng.integers(1, 5)), S, S)
            hm, pf = synth.render(people, S, S, stride=4, rng=rng)
            hs.append(hm)
            ps.append(pf)
        return (torch.rand(B, 3, S, S, generator=g) - 0.5).to(cuda), (torch.from_numpy(np.stack(hs)).to(cuda),
                                                                      torch.from_numpy(np.stack(ps)).to(cuda))

    def content(block, c):
        out = []
        for r in block:
            d = dec.parse_image(r, c)
            out.append((d["peaks"].view(np.uint32).tobytes(), d["parts"].tobytes(), d["score"].view(np.uint32).tobytes(),
                        d["flags"]))
        return out
    data = [batch(r) for r in range(2)]
    est = pipeline.PoseEstimator(m, cfg)
    want = []
    for x, scene in data:
        est(x, scene, scene_alpha=2e-3)                       # capacities settle
        bufs = est.enqueue(x, scene, scene_alpha=2e-3)
        recs = dec.fetch(bufs).copy()
        want.append(content(recs, bufs.cfg))
        assert bufs.map_hw == (S // 4, S // 4)
        # the maps the decoder read: the blended last-stack maps, where the plan keeps them
        paf = m.read_output(bufs.plan, 0).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        heat = m.read_output(bufs.plan, 1).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        humans = 0
        for i in range(B):
            d = dec.parse_image(recs[i], bufs.cfg)
            jl, ref = post_oracle.paf_to_pose(heat[i], paf[i], up=4)
            assert np.array_equal(d["peaks"][:, [0, 1, 3, 4]], jl[:, [0, 1, 3, 4]])
            assert np.array_equal(d["peaks"][:, 2].view(np.uint32), jl[:, 2].view(np.uint32))
            assert np.array_equal(d["parts"], ref["parts"])
            assert np.array_equal(d["score"].view(np.uint32), ref["score"].view(np.uint32))
            humans += len(d["parts"])
        assert humans >= B
    order = [0, 1, 1, 0]
    prev, got = None, []
    cfgc = bufs.cfg
    for r in order:
        t = est.submit(*data[r], scene_alpha=2e-3)
        if prev is not None:
            got.append(content(est.collect(prev)[1].reshape(B, -1), cfgc))
        prev = t
    got.append(content(est.collect(prev)[1].reshape(B, -1), cfgc))
    torch.cuda.synchronize()
    for k, r in enumerate(order):
        assert got[k] == want[r], "step %d: the pipelined records differ from the serial path's" % k
    hs = est.humans(data[0][0], scene=data[0][1], scene_alpha=2e-3)
    assert len(hs) == B and sum(len(h) for h in hs) >= B
