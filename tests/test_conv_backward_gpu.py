"""GPU suite of the conv backward kernels (header section 2b, csrc/conv_backward.hip): rtpose_conv2d_wgrad, the data gradient
as rtpose_conv2d on the flipped, transposed filter, and rtpose_relu_grad, on slices of wider buffers.

Inputs: x = relu(randn) (non-negative: nothing cancels), gy = randn.  Every channel outside a slice holds NaN, the gaps of
the slices are zero.  References: tests/conv_backward_restate.py (float64, F.conv2d's autograd on the CPU).  Bound: an fp32
sum of n products in any order, one rounding per product and per add, is within gamma_(n+1) * S of the exact sum, S the
sum of the absolute terms and gamma_m = m u / (1 - m u), u = 2^-24; it covers the MFMA's fma chain plus the slab sums
(n = N H W) and the forward kernel's chain of the data gradient (n = cout k k).  The worst err / bound of every case goes
through conv_driver.note (profiles/r16_conv_backward.txt).

The *_exact tests need no bound: with the integer operands of conv_backward_restate.exact_tensors every product and partial
sum is an integer below 2^24 (tests/test_conv_backward_cpu.py holds the cases to that), fp32 arithmetic in any order is exact
and the float64 reference is compared with ==.  One dropped, doubled or misplaced term changes an integer.  The bounded tests
above stay for rounding, which integers cannot show."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_backward_restate as cb
import conv_driver as cd
import layout_restate as lr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel floats on either side of an output


def up8(c):
    return (c + 7) // 8 * 8


def host_buffer(capi, lay, n, h, w, t, zero_channels):
    """A layout buffer on the host: NaN everywhere, zero in `zero_channels` channels from lay.choff of every pixel (the
    slice and its gaps), the tensor t [n, c, h, w] at the valid pixels of the slice."""
    a = np.full((cd.npx(capi, lay, n, h, w), lay.cstride), np.nan, dtype=np.float32)
    a[:, lay.choff:lay.choff + zero_channels] = 0
    return lr.scatter(a.reshape(-1), lay, t.numpy())


def guarded(numel, dev):
    """(whole buffer of sentinel words, the 16-byte aligned view of `numel` floats inside it)"""
    whole = torch.full((numel + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + numel].view(torch.float32)


def guards_intact(whole, numel):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + numel:] == cd.SENTINEL).all())


_problems = {}


def problem(capi, dev, c):
    """The case's tensors, buffers and float64 references, made once and left unchanged."""
    key = cb.case_id(c)
    if key not in _problems:
        x, gy, wt = cb.case_tensors(c)
        lx = lr.padded(c.x_cs, c.h, c.w, c.k // 2, c.x_off)
        lgy = lr.padded(up8(c.cout) + 8, c.h, c.w, c.k // 2, 4)
        p = dict(x=x, gy=gy, wt=wt, lx=lx, lgy=lgy)
        p["xbuf"] = torch.from_numpy(host_buffer(capi, lx, c.n, c.h, c.w, x, c.cin)).to(dev)
        # the output gradient as the weight gradient sees it: exactly cout channels, NaN next to them ...
        p["gbuf"] = torch.from_numpy(host_buffer(capi, lgy, c.n, c.h, c.w, gy, c.cout)).to(dev)
        # ... and as the data-gradient conv reads it: the slice padded to 8 channels with zeros
        p["gbuf8"] = torch.from_numpy(host_buffer(capi, lgy, c.n, c.h, c.w, gy, up8(c.cout))).to(dev)
        p["dw64"], p["s_dw"] = cb.wgrad64(x, gy, c.k)
        p["db64"], p["s_db"] = cb.dbias64(gy)
        p["dx64"], p["s_dx"] = cb.dgrad64(gy, wt)
        _problems[key] = p
    return _problems[key]


def wgrad(capi, dev, c, p, want_bias=True):
    """One launch into fresh sentinel-guarded outputs: (dw bits, dbias bits or None), after the guard checks."""
    lib = capi.lib
    nw = c.cout * c.cin * c.k * c.k
    floats = lib.rtpose_conv2d_wgrad_workspace_floats(c.cin, c.cout, c.k, c.n, c.h, c.w)
    w_whole, dw = guarded(nw, dev)
    b_whole, db = guarded(c.cout, dev)
    s_whole, ws = guarded(floats, dev)
    d = capi.WgradDesc()
    d.x, d.gy, d.dw, d.workspace = p["xbuf"].data_ptr(), p["gbuf"].data_ptr(), dw.data_ptr(), ws.data_ptr()
    d.dbias = db.data_ptr() if want_bias else None
    d.workspace_floats = floats
    d.lx, d.lgy = cd.L(capi, p["lx"]), cd.L(capi, p["lgy"])
    d.cin, d.cout, d.k = c.cin, c.cout, c.k
    capi.check(lib.rtpose_conv2d_wgrad(C.byref(d), c.n, c.h, c.w, capi.current_stream()), "rtpose_conv2d_wgrad")
    torch.cuda.synchronize()
    assert guards_intact(w_whole, nw), "written outside dw"
    assert guards_intact(s_whole, floats), "written outside the workspace"
    assert guards_intact(b_whole, c.cout), "written outside dbias"
    if not want_bias:
        assert (cd.np_bits(db) == cd.SENTINEL).all(), "dbias = NULL but written"
    return cd.np_bits(dw), cd.np_bits(db) if want_bias else None


@pytest.mark.parametrize("c", cb.CASES, ids=cb.case_id)
def test_weight_and_bias_gradient(capi, cuda, c):
    p = problem(capi, cuda, c)
    n = c.n * c.h * c.w
    slabs = capi.lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
    if "several slabs" in c.note:
        # slabs are equal multiples of the 32-pixel chunk but for the last one (header section 2b)
        assert slabs >= 3 and n % 32 != 0
    dw_bits, db_bits = wgrad(capi, cuda, c, p)
    dw = torch.from_numpy(dw_bits.view(np.float32).copy()).view(c.cout, c.cin, c.k, c.k).double()
    db = torch.from_numpy(db_bits.view(np.float32).copy()).double()
    # nothing outside the slices reached a sum (every channel beside them is NaN), every element was written
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    g = cb.gamma(n + 1)
    err_w, bound_w = (dw - p["dw64"]).abs(), g * p["s_dw"]
    err_b, bound_b = (db - p["db64"]).abs(), g * p["s_db"]
    ratio_w = (err_w / bound_w.clamp_min(1e-300)).max().item()
    ratio_b = (err_b / bound_b.clamp_min(1e-300)).max().item()
    print("wgrad %s: slabs %d, worst err/bound dw %.4g, dbias %.4g" % (cb.case_id(c), slabs, ratio_w, ratio_b))
    cd.note("conv_backward_wgrad_%s.json" % cb.case_id(c), {"slabs": slabs, "n": n, "dw_err_over_bound": ratio_w,
                                                             "dbias_err_over_bound": ratio_b})
    assert (err_w <= bound_w).all(), "dw: worst err / bound %g" % ratio_w
    assert (err_b <= bound_b).all(), "dbias: worst err / bound %g" % ratio_b
    # the same inputs give the same bits; without dbias the same dw and an untouched dbias
    dw2, db2 = wgrad(capi, cuda, c, p)
    assert np.array_equal(dw_bits, dw2) and np.array_equal(db_bits, db2)
    dw3, _ = wgrad(capi, cuda, c, p, want_bias=False)
    assert np.array_equal(dw_bits, dw3)


@pytest.mark.parametrize("c", cb.CASES, ids=cb.case_id)
def test_data_gradient_is_the_conv_of_the_flipped_filter(capi, cuda, pkg, c):
    import importlib
    train = importlib.import_module(pkg.__name__ + ".train")
    p = problem(capi, cuda, c)
    form = cd.Form("f32", c.k)
    cin_p = up8(c.cout)                       # the conv's input is gy
    wp, bp = cd.pack(capi, cuda, form, train.dgrad_weights(p["wt"]), torch.zeros(c.cin), cin_p)
    lout = lr.dense(up8(c.cin) + 4, c.h, c.w, 4)
    obuf = torch.full((cd.npx(capi, lout, c.n, c.h, c.w) * lout.cstride,), cd.SENTINEL, dtype=torch.int32,
                      device=cuda).view(torch.float32)
    d = (capi.ConvDesc * 1)()
    d[0].inp, d[0].w_packed, d[0].bias_packed, d[0].out = p["gbuf8"].data_ptr(), wp.data_ptr(), bp.data_ptr(), obuf.data_ptr()
    d[0].lin, d[0].lout = cd.L(capi, p["lgy"]), cd.L(capi, lout)
    d[0].cin, d[0].cout, d[0].k, d[0].relu = cin_p, c.cin, c.k, 0
    cd.call(capi, cuda, form, d, 1, c.n, c.h, c.w)
    bits = cd.np_bits(obuf)
    idx = lr.index(lout, c.n, c.h, c.w, c.cin)
    assert lr.untouched(bits, idx, cd.SENTINEL), "the conv wrote outside its slice"
    dx = torch.from_numpy(np.ascontiguousarray(np.transpose(bits[idx].view(np.float32), (0, 3, 1, 2)))).double()
    assert torch.isfinite(dx).all()
    err, bound = (dx - p["dx64"]).abs(), cb.gamma(c.cout * c.k * c.k + 1) * p["s_dx"]
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print("dgrad %s: worst err/bound %.4g" % (cb.case_id(c), ratio))
    cd.note("conv_backward_dgrad_%s.json" % cb.case_id(c), {"n": c.cout * c.k * c.k, "dx_err_over_bound": ratio})
    assert (err <= bound).all(), "dx: worst err / bound %g" % ratio


# (1, 1, 1, 1): one element; (8, 1, 4, 8): 256 elements, exactly one block; (3, 2, 1, 43): H = 1 and one pixel's channels past a
# block; (5, 2, 43, 1): W = 1
@pytest.mark.parametrize("channels,n,h,w", [(19, 1, 5, 3), (38, 2, 9, 7), (128, 2, 10, 13), (32, 3, 46, 46),
                                            (1, 1, 1, 1), (8, 1, 4, 8), (3, 2, 1, 43), (5, 2, 43, 1)])
def test_relu_grad_bit_for_bit(capi, cuda, channels, n, h, w):
    """y and gy in different layouts whose gaps and outside channels are NaN: only the valid pixels of the slices are read,
    only those of `out` are written, and out = gy (aliased) gives the same bits."""
    lib = capi.lib
    g = torch.Generator().manual_seed(channels)
    y = torch.randn(n, channels, h, w, generator=g)
    y[:, :, ::2, 1::3] = 0.0                                 # exact zeros and negative zeros: no gradient
    if y.numel() > 1:
        y[:, 0, 0, 0] = -0.0
    gy = torch.randn(n, channels, h, w, generator=g)
    gy_bits = gy.numpy().view(np.uint32).copy()
    gy_bits[0, 1:2, 0, :] = 0x7FC00777                       # a NaN gradient travels as its bits
    gy_bits[0, 2:3, 0, :] = 0x80000000                       # so does -0
    ly = lr.padded(channels + 5, h, w, 1, 3)
    lg = lr.padded(up8(channels) + 8, h, w, 3, 4)
    lo = lr.padded(channels + 2, h, w, 2, 1)

    def nan_buffer(lay, vals):
        a = np.full(cd.npx(capi, lay, n, h, w) * lay.cstride, np.nan, dtype=np.float32)
        return lr.scatter(a, lay, vals)
    ybuf = torch.from_numpy(nan_buffer(ly, y.numpy())).to(cuda)
    g_host = nan_buffer(lg, gy_bits.view(np.float32))
    gbuf = torch.from_numpy(g_host.copy()).to(cuda)
    obuf = torch.full((cd.npx(capi, lo, n, h, w) * lo.cstride,), cd.SENTINEL, dtype=torch.int32, device=cuda).view(torch.float32)
    want = np.transpose(cb.relu_grad_bits(y.numpy(), gy_bits), (0, 2, 3, 1))     # NHWC, as index() orders it
    assert want.size == 1 or ((want == 0).any() and (want != 0).any())

    capi.check(lib.rtpose_relu_grad(capi.ptr(ybuf), C.byref(cd.L(capi, ly)), capi.ptr(gbuf), C.byref(cd.L(capi, lg)),
                                    capi.ptr(obuf), C.byref(cd.L(capi, lo)), channels, n, h, w, capi.current_stream()))
    torch.cuda.synchronize()
    bits, io = cd.np_bits(obuf), lr.index(lo, n, h, w, channels)
    assert np.array_equal(bits[io], want)
    assert lr.untouched(bits, io, cd.SENTINEL), "written outside the valid pixels of the slice"
    assert np.array_equal(cd.np_bits(gbuf), g_host.view(np.uint32)), "gy was modified"

    capi.check(lib.rtpose_relu_grad(capi.ptr(ybuf), C.byref(cd.L(capi, ly)), capi.ptr(gbuf), C.byref(cd.L(capi, lg)),
                                    capi.ptr(gbuf), C.byref(cd.L(capi, lg)), channels, n, h, w, capi.current_stream()))
    torch.cuda.synchronize()
    after, ig = cd.np_bits(gbuf), lr.index(lg, n, h, w, channels)
    assert np.array_equal(after[ig], want)
    expect = g_host.view(np.uint32).copy()
    expect[ig] = want
    assert np.array_equal(after, expect), "aliased: something besides the valid pixels of the slice changed"


# ---- bit for bit, with exact integer operands ---------------------------------------------------------------------------------
def exact_problem(capi, dev, c):
    """The exact case's tensors, buffers and float64 references, made once and left unchanged.

    x buffer: NaN in every channel outside the slice, the slice's gaps ZERO - all of them, also where the gap is wider than
    k / 2: the header asks for "zero gaps of at least k/2" and, unlike for gy, does not promise that gap pixels farther than
    k / 2 from a valid pixel are never read, so they hold what section 1 says gaps hold.  gy buffer of the weight gradient:
    NaN everywhere but at the valid pixels of the slice, its own gap pixels included ("read at the valid pixels only").  gy
    buffer of the data gradient: the slice padded to 8 channels with zero gaps, as rtpose_conv2d reads it."""
    key = "exact_" + cb.case_id(c)
    if key not in _problems:
        x, gy, wt, _ = cb.exact_tensors(c)
        lx = lr.padded(c.x_cs, c.h, c.w, c.k // 2 + c.gap, c.x_off)
        lgy = lr.padded(up8(c.cout) + 8, c.h, c.w, c.k // 2, 4)
        p = dict(x=x, gy=gy, wt=wt, lx=lx, lgy=lgy)
        p["xbuf"] = torch.from_numpy(host_buffer(capi, lx, c.n, c.h, c.w, x, c.cin)).to(dev)
        p["gbuf"] = torch.from_numpy(host_buffer(capi, lgy, c.n, c.h, c.w, gy, 0)).to(dev)
        p["gbuf8"] = torch.from_numpy(host_buffer(capi, lgy, c.n, c.h, c.w, gy, up8(c.cout))).to(dev)
        p["dw"] = cb.wgrad64(x, gy, c.k)[0].float().numpy().ravel()
        p["db"] = cb.dbias64(gy)[0].float().numpy()
        p["dx"] = cb.dgrad64(gy, wt)[0].float().numpy()
        assert cb.exact_margin(c) < 2 ** 24
        _problems[key] = p
    return _problems[key]


def mismatch(got, want):
    bad = np.flatnonzero(got.ravel() != want.ravel())
    return "%d of %d differ, first at %s: %r != %r" % (bad.size, want.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


@pytest.mark.parametrize("c", cb.EXACT_CASES, ids=cb.case_id)
def test_weight_and_bias_gradient_exact(capi, cuda, c):
    """dw and dbias equal the float64 sums of the integer operands, with and without dbias; the workspace held sentinel
    words, so the result does not depend on what it held."""
    p = exact_problem(capi, cuda, c)
    slabs = capi.lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
    assert ("several slabs" in c.tags) == (slabs >= 2)
    dw_bits, db_bits = wgrad(capi, cuda, c, p)
    dw, db = dw_bits.view(np.float32), db_bits.view(np.float32)
    print("wgrad exact %s: slabs %d, dw %d wrong of %d, dbias %d wrong of %d"
          % (cb.case_id(c), slabs, int((dw != p["dw"]).sum()), dw.size, int((db != p["db"]).sum()), db.size))
    assert np.array_equal(dw, p["dw"]), "dw: " + mismatch(dw, p["dw"])
    assert np.array_equal(db, p["db"]), "dbias: " + mismatch(db, p["db"])
    dw2, _ = wgrad(capi, cuda, c, p, want_bias=False)
    assert np.array_equal(dw2.view(np.float32), p["dw"]), "dw without dbias: " + mismatch(dw2.view(np.float32), p["dw"])


@pytest.mark.parametrize("c", cb.EXACT_CASES, ids=cb.case_id)
def test_data_gradient_exact(capi, cuda, pkg, c):
    """rtpose_conv2d of gy (slice padded to 8 channels) with the flipped, transposed integer filter, written to a slice of
    up8(cin) + 4 channels at choff 4, equals the float64 input gradient."""
    import importlib
    train = importlib.import_module(pkg.__name__ + ".train")
    p = exact_problem(capi, cuda, c)
    form = cd.Form("f32", c.k)
    cin_p = up8(c.cout)
    wp, bp = cd.pack(capi, cuda, form, train.dgrad_weights(p["wt"]), torch.zeros(c.cin), cin_p)
    lout = lr.dense(up8(c.cin) + 4, c.h, c.w, 4)
    obuf = torch.full((cd.npx(capi, lout, c.n, c.h, c.w) * lout.cstride,), cd.SENTINEL, dtype=torch.int32,
                      device=cuda).view(torch.float32)
    d = (capi.ConvDesc * 1)()
    d[0].inp, d[0].w_packed, d[0].bias_packed, d[0].out = p["gbuf8"].data_ptr(), wp.data_ptr(), bp.data_ptr(), obuf.data_ptr()
    d[0].lin, d[0].lout = cd.L(capi, p["lgy"]), cd.L(capi, lout)
    d[0].cin, d[0].cout, d[0].k, d[0].relu = cin_p, c.cin, c.k, 0
    cd.call(capi, cuda, form, d, 1, c.n, c.h, c.w)
    bits = cd.np_bits(obuf)
    idx = lr.index(lout, c.n, c.h, c.w, c.cin)
    assert lr.untouched(bits, idx, cd.SENTINEL), "the conv wrote outside its slice"
    dx = np.ascontiguousarray(np.transpose(bits[idx].view(np.float32), (0, 3, 1, 2)))
    print("dgrad exact %s: %d wrong of %d" % (cb.case_id(c), int((dx != p["dx"]).sum()), dx.size))
    assert np.array_equal(dx, p["dx"]), "dx: " + mismatch(dx, p["dx"])
