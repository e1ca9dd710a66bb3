"""The conv launchers on input slices of wider pixel buffers (rtpose_conv_desc.lin with choff != 0, cstride > cin, and - in a
grouped launch - a cstride / choff / lead / base per branch), through the C ABI.

One runner performs the same launch twice: on a COMPACT input (cstride == cin elements, choff == 0 - what every other
launcher test feeds) and on the same data as a slice of a wider pixel whose other channels hold finite decoys of magnitude
2^10 .. 2^11 (tests/conv_slices.py).  Problem, packing, launch and read-back are the shared driver's (tests/conv_driver.py);
weights, output layout (the driver's preset for the form), ws / hs / lead, stream and scratch are the same.  It asserts

  (a) the wide run's output buffer holds the bits of the compact run's: lin.cstride / lin.choff change addresses only,
  (b) on the tiny shapes, the wide run against a float64 conv2d of the slice data within the tolerance of the form
      (conv_driver.check: TOL, check_bf16, X3_TOL, the gamma bound of F(8,7); STEM7_TOL for the hourglass stem),
  (c) the wide input buffer is bit-identical after the launch,
  (d) every output word outside the written slices is untouched (layout_restate.untouched, in conv_driver.outputs),
  (e) the device error word of a Winograd launch with a scratch is 0 (conv_driver.call),
  (f) the compact fp32 / bf16 input, which the library's conversion kernel fills, is bit-equal to conv_slices.scatter_nchw:
      the input side of this file does not rest on the library.

No launcher was found to pick another ARITHMETIC from the input cstride / choff, so (a) holds everywhere.  One launcher reads
them for a scheduling choice: rtpose_conv2d_bf16 runs its persistent strips only when the branches of a grouped launch share
lin.cstride and lin.lead (csrc/conv_mfma_bf16.hip, `same_pitch` in conv_bf16_launch); the two-buffer test below differs in
lead in its compact run as well, so both runs take the same path, and the sums do not depend on it anyway.

The large shapes are the smallest of the existing case tables known to select a launcher's main / persistent form; they
run with bit identity only (the CPU reference is the slow part of a case)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_driver as cd
import conv_slices as cs
import layout_restate as lr
from conv_driver import STEM7_TOL, TOL, Form

pytestmark = pytest.mark.gpu


def _unit(form):
    return {"f32": cs.UNIT_F32, "bf16": cs.UNIT_BF16, "x3": cs.UNIT_X3}[form.kind]


def _out(form):
    """the output buffer of the form's own test file: 8-channel pieces for bf16x3, 16-byte aligned slices for the 64-channel
    kernel, odd stride + channel offsets for the rest"""
    return cd.PIECES if form.kind == "x3" else cd.ALIGNED if form.entry == "c64" else cd.ODD


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _compare(capi, dev, form, n, h, w, cin, cout, relu=1, pool=0, prelu=0, groups=1, pad_out=1, seed=0, ref=True,
             geoms=None, scratch=True):
    """The generic runner: one compact launch, then the same launch per input geometry; (a) - (f)."""
    P = cd.problem(form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, ref=torch.float64 if ref else None)
    out = _out(form)
    buf, lay = cd.to_layout(capi, dev, P, P.xs[0], form.k // 2)
    if form.kind != "x3":
        host = cs.scatter_nchw(P.xs[0], lay, cd.npx(capi, lay, n, h, w), buf.dtype)
        assert _same_bits(buf.cpu(), host), "the conversion kernel's buffer is not the host scatter's"     # (f)
    ob_c, louts = cd.launch(capi, dev, P, [(buf, lay)] * groups, out, pad_out, scratch)
    assert _bits(ob_c).ne(0).any()
    geoms = geoms or cs.geometries(lay.cstride, _unit(form))
    for name, extra, choff in geoms:
        wide, wlay = cs.widen(buf, lay, n, h, w, extra, choff, seed)
        before = wide.clone()
        ob_w, _ = cd.launch(capi, dev, P, [(wide, wlay)] * groups, out, pad_out, scratch)
        assert _same_bits(wide, before), (name, "the launch changed its input buffer")                        # (c)
        assert _same_bits(ob_w, ob_c), (name, "lin.cstride / lin.choff changed the result")                   # (a)
        outs = cd.outputs(P, ob_w, louts, out, ref)                                                             # (d)
        if ref:
            for gi in range(groups):
                cd.check(P, gi, outs[gi], P.xs[0])                                                            # (b)


def _mid(form, cin_e):
    return [cs.geometries(cin_e, _unit(form))[0]]


# ---- rtpose_conv2d and the Winograd forms, fp32 -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cs.TINY_F32, ids=lambda c: "k%d-m%s-%dx%dx%dx%d-%d-%d%d%d" % c)
def test_fp32_launchers_on_tiny_input_slices(capi, cuda, case):
    k, m, n, h, w, cin, cout, relu, pool, prelu = case
    _compare(capi, cuda, Form("f32", k, m), n, h, w, cin, cout, relu, pool, prelu, pad_out=3 if pool else 1,
             seed=k * 100 + cin + cout)


@pytest.mark.parametrize("case", cs.LARGE_F32, ids=lambda c: "k%d-m%s-%dx%dx%dx%d-%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6]))
def test_fp32_launchers_main_forms_on_input_slices(capi, cuda, case):
    """The large-form geometries: bit identity, input and output untouched, error word - the slice in the middle of a wider
    pixel; the F(m,7) launches with the caller's scratch (persistent blocks, split tiles) and without (one block per tile)."""
    k, m, n, h, w, cin, cout, relu, pool, groups = case
    form = Form("f32", k, m)
    for scratch in ((True, False) if (k == 7 and m) else (True,)):
        _compare(capi, cuda, form, n, h, w, cin, cout, relu, pool, 0, groups=groups, seed=7 + k, ref=False,
                 geoms=_mid(form, cin), scratch=scratch)


# ---- rtpose_conv2d_bf16, rtpose_conv2d_bf16x3, rtpose_conv3x3_c64_bf16 ----------------------------------------------------------
BF16_TINY = [(1, 16, 16, 96, 64, 1), (1, 12, 10, 16, 24, 3), (5, 6, 6, 32, 8, 7)]     # n, h, w, cin, cout, k


@pytest.mark.parametrize("out_f32", (False, True), ids=("bf16out", "f32out"))
@pytest.mark.parametrize("case", BF16_TINY, ids=lambda c: "k%d" % c[5])
def test_bf16_launcher_on_tiny_input_slices(capi, cuda, case, out_f32):
    n, h, w, cin, cout, k = case
    _compare(capi, cuda, Form("bf16", k, None, out_f32), n, h, w, cin, cout, 1, 0, pad_out=1, seed=300 + k)


@pytest.mark.parametrize("out_f32", (False, True), ids=("bf16out", "f32out"))
def test_bf16_launcher_7x7_strips_on_an_input_slice(capi, cuda, out_f32):
    form = Form("bf16", 7, None, out_f32)
    _compare(capi, cuda, form, 2, 46, 46, 128, 128, 1, 0, pad_out=3, seed=307, ref=False, geoms=_mid(form, 128))


@pytest.mark.parametrize("case", [(5, 6, 6, 32, 8, 7, 1), (3, 23, 17, 128, 38, 1, 0)], ids=("k7", "k1"))
def test_bf16x3_launcher_on_input_slices(capi, cuda, case):
    """The two smallest of tests/test_bf16x3_gpu.py's CASES; the input counts 2 elements per channel (hi / lo pieces of 8
    channels), so the alignment unit of lin is 16 elements."""
    n, h, w, cin, cout, k, relu = case
    _compare(capi, cuda, Form("x3", k), n, h, w, cin, cout, relu, 0, pad_out=3, seed=400 + k)


@pytest.mark.parametrize("case", [(1, 1, 1, 64, 1, 0), (2, 9, 13, 128, 1, 0), (1, 6, 10, 64, 1, 1), (1, 5, 37, 64, 0, 0)],
                         ids=("1x1", "oddW", "pool", "two-tiles"))
def test_c64_bf16_launcher_on_input_slices(capi, cuda, case):
    """rtpose_conv3x3_c64_bf16 (raw-buffer byte offsets from lin.cstride / lin.choff): the smallest geometry its `_fits`
    accepts (one pixel, one pass of 64 channels), an odd map with two passes, the fused pool, and an odd map wider than one
    32-column tile - only there do the last two halo columns, which the kernel fetches through a load path of their own
    (`issue_extra`), hold real pixels."""
    n, h, w, cout, relu, pool = case
    _compare(capi, cuda, Form("bf16", 3, None, False, "c64"), n, h, w, 64, cout, relu, pool, pad_out=1, seed=64 + w)


# ---- branches that read different buffers ---------------------------------------------------------------------------------------
TWO_BUFFER_FORMS = [Form("f32", 3), Form("f32", 7), Form("f32", 3, 2), Form("f32", 3, 4), Form("f32", 7, 6), Form("bf16", 7)]


def _side_by_side(bufs):
    """The buffers as views of ONE allocation with as much zero slack behind them as both hold: a kernel that walked one
    branch's buffer with the other's pixel stride or lead reads wrong data (and fails the test), not memory outside the
    allocation."""
    sizes = [(t.numel() + 63) // 64 * 64 for t in bufs]
    arena = torch.zeros(2 * sum(sizes), dtype=bufs[0].dtype, device=bufs[0].device)
    views, at = [], 0
    for t, sz in zip(bufs, sizes):
        views.append(arena[at:at + t.numel()])
        views[-1].copy_(t)
        at += sz
    return views


def _fits(capi, form, n, h, w, cin, cout):
    if form.m is None:
        return True
    d = (capi.ConvDesc * 1)()
    d[0].k, d[0].cin, d[0].cout, d[0].wino_m = form.k, cin, cout, form.m
    d[0].lin = cd.L(capi, lr.padded(cin, h, w, form.k // 2))
    return capi.lib.rtpose_conv2d_winograd_fits(d, n, h, w) == 1


@pytest.mark.parametrize("shape", [(2, 9, 11, 32, 16), (2, 46, 46, 128, 128)], ids=("tiny", "stage"))
@pytest.mark.parametrize("form", TWO_BUFFER_FORMS, ids=lambda f: "%s-k%d-m%s" % (f.kind, f.k, f.m))
def test_branches_that_read_different_buffers(capi, cuda, form, shape):
    """A two-group launch whose branches read different buffers, as the CPM branches do from their second conv on: group 0
    the middle slice of buffer A, group 1 the END slice of buffer B - another cstride, another choff, and a lead larger by
    one row plus 3 pixels (ws / hs equal: the launchers demand it).  Each branch has the bits of the same grouped launch on
    compact buffers (which differ in base and lead as well), and on the tiny shape is within tolerance of its own reference.
    F(6,7) takes whole 128-column tiles only (header: rtpose_conv2d_winograd_fits is 0 for cout = 16), so its tiny shape
    has cout = 128."""
    n, h, w, cin, cout = shape
    if not _fits(capi, form, n, h, w, cin, cout):
        assert form.k == 7 and form.m and cout == 16
        cout = 128
    ref = h < 20
    P = cd.problem(form, n, h, w, cin, cout, 1, 0, 0, groups=2, seed=500 + form.k, ninputs=2,
                   ref=torch.float64 if ref else None)
    pad, u = form.k // 2, _unit(form)
    a, lay = cd.to_layout(capi, cuda, P, P.xs[0], pad)
    b0, _ = cd.to_layout(capi, cuda, P, P.xs[1], pad)
    by = lay.ws + 3
    b, lay_b = cs.relead(b0, lay, by)
    a, b = _side_by_side([a, b])
    ob_c, louts = cd.launch(capi, cuda, P, [(a, lay), (b, lay_b)], _out(form), 3)
    wa, wlay_a = cs.widen(a, lay, n, h, w, 2 * u, u, 1)                 # middle: cstride cin + 2 u, choff u
    wb0, wl = cs.widen(b0, lay, n, h, w, 3 * u, 3 * u, 2)               # end: cstride cin + 3 u, choff 3 u
    wb, wlay_b = cs.relead(wb0, wl, by)
    wa, wb = _side_by_side([wa, wb])
    assert wlay_a.cstride != wlay_b.cstride and wlay_a.choff != wlay_b.choff and wlay_b.lead == wlay_a.lead + by
    keep = (wa.clone(), wb.clone())
    ob_w, _ = cd.launch(capi, cuda, P, [(wa, wlay_a), (wb, wlay_b)], _out(form), 3)
    assert _same_bits(wa, keep[0]) and _same_bits(wb, keep[1]), "the launch changed an input buffer"
    outs_c = cd.outputs(P, ob_c, louts, _out(form))
    outs_w = cd.outputs(P, ob_w, louts, _out(form))
    for gi in range(2):
        assert torch.equal(outs_w[gi], outs_c[gi]), "branch %d reads its buffer through the other's view" % gi
        assert outs_w[gi].abs().max().item() > 0
    assert _same_bits(ob_w, ob_c)
    assert not torch.equal(outs_w[0], outs_w[1])
    if ref:
        for gi in range(2):
            cd.check(P, gi, outs_w[gi], P.xs[gi])


# ---- read and write one buffer: the OpenPose dense block --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 9, 11, 16), (1, 46, 46, 128)], ids=("tiny", "stage"))
@pytest.mark.parametrize("form", [Form("f32", 3), Form("f32", 3, 2), Form("f32", 3, 4)], ids=("direct", "F2x2", "F4x4"))
def test_dense_block_reads_and_writes_one_buffer(capi, cuda, form, shape):
    """in == out, cstride = 3 c: the conv reads slice 0 and writes slice 1, then reads slice 1 and writes slice 2 (the 3x3
    convs of an OpenPose dense block, csrc/net.hip).  Slices 1 and 2 hold the bits of the same two convs on separate compact
    buffers, slice 0 and every other word of the buffer are untouched.  Both Winograd forms need at least 32 input
    channels (rtpose_conv2d_winograd_fits is 0 for c = 16): their tiny shape has c = 32."""
    n, h, w, c = shape
    if not _fits(capi, form, n, h, w, c, c):
        assert form.m and c == 16
        c = 32
    lib = capi.lib
    P = cd.pack_all(capi, cuda, cd.problem(form, n, h, w, c, c, 1, 0, 0, groups=2, seed=600 + c, ref=None))   # two filter banks: conv 1, conv 2
    x0, lay = cd.to_layout(capi, cuda, P, P.xs[0], 1)
    npx = cd.npx(capi, lay, n, h, w)

    def conv(gi, src, lsrc, dst, ldst):
        d = (capi.ConvDesc * 1)()
        d[0].inp, d[0].w_packed, d[0].bias_packed, d[0].out = src.data_ptr(), P.wp[gi].data_ptr(), P.bp[gi].data_ptr(), dst.data_ptr()
        d[0].lin, d[0].lout = cd.L(capi, lsrc), cd.L(capi, ldst)
        d[0].cin, d[0].cout, d[0].k, d[0].relu, d[0].wino_m = c, c, 3, 1, form.m or 0
        cd.call(capi, cuda, form, d, 1, n, h, w, True)

    # separate compact buffers
    t1, t2 = torch.zeros(npx * c, device=cuda), torch.zeros(npx * c, device=cuda)
    conv(0, x0, lay, t1, lay)
    conv(1, t1, lay, t2, lay)
    # one buffer of three slices
    views = [lr.Lay(3 * c, s * c, lay.ws, lay.hs, lay.lead) for s in range(3)]
    blk = torch.zeros(npx, 3 * c, device=cuda)
    blk[:, :c] = x0.view(npx, c)
    blk = blk.reshape(-1)
    conv(0, blk, views[0], blk, views[1])
    conv(1, blk, views[1], blk, views[2])
    got = blk.view(npx, 3 * c)
    assert _same_bits(got[:, :c].contiguous(), x0.view(npx, c)), "slice 0 was written"
    assert _same_bits(got[:, c:2 * c].contiguous(), t1.view(npx, c)), "slice 1 differs from the separate-buffer run"
    assert _same_bits(got[:, 2 * c:].contiguous(), t2.view(npx, c)), "slice 2 differs from the separate-buffer run"
    assert t1.abs().max().item() > 0 and t2.abs().max().item() > 0
    # (slice equality over EVERY pixel covers the gaps; stated once more in the suite's exact form for slices 1 and 2)
    written = [lr.index(v, n, h, w, c) for v in views]
    assert lr.untouched(cd.np_bits(blk), written, 0), "a conv wrote into the gaps of the shared buffer"


# ---- rtpose_conv1x1_pair (fp32) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 9, 13, 128), (1, 11, 7, 512)])
def test_pointwise_pair_on_input_slices(capi, cuda, shape):
    """Mconv6 + Mconv7 as one launch (csrc/conv_tail.hip), both branches, each reading its own buffer: compact, the slice
    at choff = 8 in the middle of a 144-channel pixel, and at the end of a 136-channel one."""
    lib, Layout = capi.lib, capi.Layout
    n, h, w, mid = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    stream = capi.current_stream()
    couts = (38, 19)
    xs = [torch.randn(n, 128, h, w, generator=g) for _ in range(2)]
    w1 = [torch.randn(mid, 128, 1, 1, generator=g) * (2.0 / 128) ** 0.5 for _ in range(2)]
    b1 = [torch.randn(mid, generator=g) * 0.1 for _ in range(2)]
    w2 = [torch.randn(c, mid, 1, 1, generator=g) * (2.0 / mid) ** 0.5 for c in couts]
    b2 = [torch.randn(c, generator=g) * 0.1 for c in couts]
    lay = lr.padded(128, h, w, 0)
    npx = cd.npx(capi, lay, n, h, w)
    keep = []

    def pack(wt, b, cout):
        packed = cd.pack(capi, cuda, cd.Form("f32", 1), wt, b, wt.shape[1])
        keep.extend(packed)
        return packed

    p1 = [pack(w1[gi], b1[gi], mid) for gi in range(2)]
    p2 = [pack(w2[gi], b2[gi], couts[gi]) for gi in range(2)]
    compact = [cs.scatter_nchw(xs[gi], lay, npx).to(cuda) for gi in range(2)]
    lcat = [lr.padded(192, h, w, 3, 128), lr.padded(192, h, w, 3, 166)]
    lmid = lr.padded(mid, h, w, 0)

    def run(inputs):
        cat = torch.zeros(cd.npx(capi, lcat[0], n, h, w) * 192, device=cuda)
        mids = [torch.zeros(cd.npx(capi, lmid, n, h, w) * mid, device=cuda) for _ in range(2)]
        d1, d2 = (capi.ConvDesc * 2)(), (capi.ConvDesc * 2)()
        for gi, (buf, l) in enumerate(inputs):
            d1[gi].inp, d1[gi].w_packed, d1[gi].bias_packed, d1[gi].out = (buf.data_ptr(), p1[gi][0].data_ptr(),
                                                                         p1[gi][1].data_ptr(), mids[gi].data_ptr())
            d1[gi].lin, d1[gi].lout = cd.L(capi, l), cd.L(capi, lmid)
            d1[gi].cin, d1[gi].cout, d1[gi].k, d1[gi].relu, d1[gi].pool = 128, mid, 1, 1, 0
            d2[gi].inp, d2[gi].w_packed, d2[gi].bias_packed, d2[gi].out = (mids[gi].data_ptr(), p2[gi][0].data_ptr(),
                                                                         p2[gi][1].data_ptr(), cat.data_ptr())
            d2[gi].lin, d2[gi].lout = cd.L(capi, lmid), cd.L(capi, lcat[gi])
            d2[gi].cin, d2[gi].cout, d2[gi].k, d2[gi].relu, d2[gi].pool = mid, couts[gi], 1, 0, 0
        assert lib.rtpose_conv1x1_pair_fits(d1, d2, 2) == 1
        capi.check(lib.rtpose_conv1x1_pair(d1, d2, 2, n, h, w, stream), "rtpose_conv1x1_pair")
        torch.cuda.synchronize()
        return cat

    cat_c = run([(compact[0], lay), (compact[1], lay)])
    refs = [F.conv2d(F.relu(F.conv2d(xs[gi].double(), w1[gi].double(), b1[gi].double())), w2[gi].double(), b2[gi].double())
            for gi in range(2)]
    for (e0, c0), (e1, c1) in (((16, 8), (8, 8)), ((8, 8), (16, 8))):
        wide = [cs.widen(compact[0], lay, n, h, w, e0, c0, 3), cs.widen(compact[1], lay, n, h, w, e1, c1, 4)]
        before = [t.clone() for t, _ in wide]
        cat_w = run(wide)
        assert all(_same_bits(t, b) for (t, _), b in zip(wide, before)), "the launch changed an input buffer"
        assert _same_bits(cat_w, cat_c), "lin.cstride / lin.choff changed the result"
        host = cat_w.cpu()
        assert lr.untouched(cd.np_bits(host), [lr.index(l, n, h, w, c) for l, c in zip(lcat, couts)], 0)
        for gi in range(2):
            o = cs.slice_of(host, lcat[gi], n, h, w, couts[gi]).double()
            assert (o - refs[gi]).abs().max().item() <= TOL * max(1.0, refs[gi].abs().max().item())


# ---- the first layers reading a layout buffer: rtpose_conv_first, rtpose_conv_first_bf16, rtpose_conv7x7_s2 --------------------------
LX = [(4, 0), (8, 4), (16, 8)]      # (cstride, choff) of the three image channels


def _image_views(capi, dev, x, n, h, w):
    """the image as a compact 3-channel layout buffer and as the three LX slices of wider pixels"""
    lay = lr.padded(3, h, w, 1)
    compact = cs.scatter_nchw(x, lay, cd.npx(capi, lay, n, h, w)).to(dev)
    return (compact, lay), [cs.widen(compact, lay, n, h, w, cstride - 3, choff, cstride) for cstride, choff in LX]


@pytest.mark.parametrize("bf16", (False, True), ids=("fp32", "bf16"))
@pytest.mark.parametrize("shape", [(3, 8, 8), (1, 37, 45)])
def test_first_layer_kernels_read_an_image_slice(capi, cuda, shape, bf16):
    lib = capi.lib
    n, h, w = shape
    g = torch.Generator().manual_seed(h * 1000 + w + int(bf16))
    x = torch.rand(n, 3, h, w, generator=g) - 0.5
    wt = torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    b = torch.randn(64, generator=g) * 0.1
    stream = capi.current_stream()
    wd, bd = wt.to(cuda), b.to(cuda)
    wp = torch.zeros(lib.rtpose_conv_first_packed_floats(), device=cuda)
    capi.check((lib.rtpose_pack_conv_first_bf16 if bf16 else lib.rtpose_pack_conv_first)(capi.ptr(wd), capi.ptr(bd), capi.ptr(wp),
                                                                                         stream))
    lo = lr.padded(64 + 16, h, w, 1, 8) if bf16 else lr.padded(64 + 5, h, w, 1, 3)
    entry = lib.rtpose_conv_first_bf16 if bf16 else lib.rtpose_conv_first

    def run(buf, lay):
        obuf = torch.zeros(cd.npx(capi, lo, n, h, w) * lo.cstride, device=cuda, dtype=torch.bfloat16 if bf16 else torch.float32)
        capi.check(entry(None, capi.ptr(buf), C.byref(cd.L(capi, lay)), capi.ptr(wp), capi.ptr(obuf), C.byref(cd.L(capi, lo)), 1,
                         n, h, w, stream), "rtpose_conv_first")
        torch.cuda.synchronize()
        return obuf

    (compact, lay), wides = _image_views(capi, cuda, x, n, h, w)
    ob_c = run(compact, lay)
    if bf16:
        ref = F.relu(F.conv2d(cd.rb(x).double(), cd.rb(wt).double(), b.double(), padding=1)).float()
    else:
        ref = F.relu(F.conv2d(x.double(), wt.double(), b.double(), padding=1))
    for wide, wlay in wides:
        before = wide.clone()
        ob_w = run(wide, wlay)
        assert _same_bits(wide, before) and _same_bits(ob_w, ob_c), (wlay.cstride, wlay.choff)
        host = ob_w.cpu()
        assert lr.untouched(cd.np_bits(host), lr.index(lo, n, h, w, 64), 0)
        out = cs.slice_of(host, lo, n, h, w, 64).float()
        if bf16:
            cd.check_bf16(out, ref, False)
        else:
            assert (out.double() - ref).abs().max().item() <= TOL * max(1.0, ref.abs().max().item())


def test_hourglass_stem_reads_an_image_slice(capi, cuda):
    lib = capi.lib
    n, h, w = 1, 43, 33
    g = torch.Generator().manual_seed(4333)
    x = torch.rand(n, 3, h, w, generator=g) - 0.5
    wt = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    b = torch.randn(64, generator=g) * 0.1
    ref = F.relu(F.conv2d(x.double(), wt.double(), b.double(), stride=2, padding=3))
    ho, wo = (h + 1) // 2, (w + 1) // 2
    wd, bd = wt.to(cuda), b.to(cuda)
    wp = torch.zeros(lib.rtpose_conv7x7_s2_packed_floats(), device=cuda)
    capi.check(lib.rtpose_pack_conv7x7_s2(capi.ptr(wd), capi.ptr(bd), capi.ptr(wp), capi.current_stream()))
    lo = lr.padded(64 + 12, ho, wo, 1, 8)

    def run(buf, lay):
        obuf = torch.zeros(cd.npx(capi, lo, n, ho, wo) * lo.cstride, device=cuda)
        capi.check(lib.rtpose_conv7x7_s2(None, capi.ptr(buf), C.byref(cd.L(capi, lay)), capi.ptr(wp), capi.ptr(obuf),
                                         C.byref(cd.L(capi, lo)), 1, n, h, w, capi.current_stream()), "rtpose_conv7x7_s2")
        torch.cuda.synchronize()
        return obuf

    (compact, lay), wides = _image_views(capi, cuda, x, n, h, w)
    ob_c = run(compact, lay)
    for wide, wlay in wides:
        before = wide.clone()
        ob_w = run(wide, wlay)
        assert _same_bits(wide, before) and _same_bits(ob_w, ob_c), (wlay.cstride, wlay.choff)
        host = ob_w.cpu()
        assert lr.untouched(cd.np_bits(host), lr.index(lo, n, ho, wo, 64), 0)
        out = cs.slice_of(host, lo, n, ho, wo, 64).double()
        assert (out - ref).abs().max().item() <= STEM7_TOL * max(1.0, ref.abs().max().item())
