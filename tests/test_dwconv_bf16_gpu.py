"""GPU suite of the bf16 depthwise 3x3 kernels (header section 2b continued: rtpose_dwconv3x3_bf16_f32 in
csrc/shufflenet_ops.hip, rtpose_dwconv3x3_wgrad_bf16 / rtpose_dwconv3x3_dgrad_bf16 in csrc/dwconv_backward.hip) and of
train.dwconv3x3(compute_dtype='bf16').

Every buffer is filled with a NaN sentinel around the slices (bf16 buffers with a bf16 NaN, fp32 ones with
conv_driver.SENTINEL); x and gy keep the zero gaps the kernels may read in their own channels.  After every launch the
inputs are intact and no element outside the destination slice has changed, bit for bit.  Every output is held, bit for
bit, to the host restatement on the widened operands (tests/dwconv_bf16_restate.py; tests/test_dwconv_bf16_cpu.py shows that
the float64 sums of these operands are exact, so the weight gradient has one value whatever the order) AND to the existing
fp32 kernel run on the widened operands.  The cases are the shapes of dwconv_restate.CASES, slab cases included, plus
C = 6 in 8, each in three alignment classes (16-byte pieces, 8-byte pieces, element by element).  The forward has the doors of
rtpose_dwconv3x3_bf16 (C % 8, 16-byte aligned slices), so it runs each shape with the channels rounded up to 8 in the
16-byte layouts."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_driver as cd
import dwconv_bf16_restate as db
import dwconv_restate as dr
import layout_restate as lr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel words on either side of an output
SENT16 = 0x7FC1         # a quiet bf16 NaN with a recognisable payload


def L(capi, lay):
    return C.byref(capi.Layout(*lay))


def bf16_buffer(capi, lay, n, h, w, c, values=None, zero_gaps=True):
    """A bf16 layout buffer on the host, as uint16: SENT16 everywhere but in the slice's own channels, which are zero at every
    pixel if `zero_gaps` and hold the bf16 bits of `values` float32 [n, c, h, w] at the valid pixels"""
    a = np.full(cd.npx(capi, lay, n, h, w) * lay.cstride, SENT16, dtype=np.uint16)
    if zero_gaps:
        a.reshape(-1, lay.cstride)[:, lay.choff:lay.choff + c] = 0
    return a if values is None else lr.scatter(a, lay, db.bf16_bits(values))


def f32_buffer(capi, lay, n, h, w, c, values=None, zero_gaps=True):
    a = np.full(cd.npx(capi, lay, n, h, w) * lay.cstride, cd.SENTINEL, dtype=np.uint32)
    if zero_gaps:
        a.reshape(-1, lay.cstride)[:, lay.choff:lay.choff + c] = 0
    return a if values is None else lr.scatter(a, lay, np.ascontiguousarray(values, np.float32).view(np.uint32))


def dev16(a, dev):
    return torch.from_numpy(a.view(np.int16).copy()).to(dev)


def dev32(a, dev):
    return torch.from_numpy(a.view(np.int32).copy()).to(dev).view(torch.float32)


def bits16(t):
    return t.cpu().numpy().view(np.uint16)


def guarded(words, dev):
    whole = torch.full((words + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + words].view(torch.float32)


def guards_intact(whole, words):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + words:] == cd.SENTINEL).all())


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(u32(a), u32(b))


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return bool(((u32(a) == u32(b)) | both).all())


# ---- the three bf16 launches, on poisoned buffers ---------------------------------------------------------------------------------------
def run_wgrad16(capi, dev, c, x, gy, bias=True, gap_x=1):
    lib = capi.lib
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    lx, lgy, _ = dr.layouts(c, gap_x=gap_x, gap_gy=2)
    xh = bf16_buffer(capi, lx, c.n, c.h, c.w, c.c, x.numpy())
    gh = bf16_buffer(capi, lgy, c.n, ho, wo, c.c, gy.numpy(), zero_gaps=False)      # gy is read at its valid pixels only
    xbuf, gbuf = dev16(xh, dev), dev16(gh, dev)
    doubles = lib.rtpose_dwconv3x3_wgrad_workspace_doubles(c.c, c.n, c.h, c.w, c.stride)
    dw_whole, dw = guarded(c.c * 9, dev)
    db_whole, dbias = guarded(c.c, dev)
    ws_whole, ws = guarded(2 * doubles, dev)
    capi.check(lib.rtpose_dwconv3x3_wgrad_bf16(capi.ptr(xbuf), L(capi, lx), capi.ptr(gbuf), L(capi, lgy), capi.ptr(dw),
                                               capi.ptr(dbias) if bias else None, capi.ptr(ws), doubles, c.c, c.n, c.h, c.w, c.stride,
                                               capi.current_stream()), "rtpose_dwconv3x3_wgrad_bf16")
    torch.cuda.synchronize()
    assert np.array_equal(bits16(xbuf), xh) and np.array_equal(bits16(gbuf), gh), "wgrad modified an input"
    assert guards_intact(dw_whole, c.c * 9) and guards_intact(db_whole, c.c) and guards_intact(ws_whole, 2 * doubles)
    if not bias:
        assert (cd.np_bits(dbias) == cd.SENTINEL).all(), "dbias = NULL but written"
    return cd.np_bits(dw).view(np.float32).reshape(c.c, 1, 3, 3).copy(), cd.np_bits(dbias).view(np.float32).copy() if bias else None


def run_dgrad16(capi, dev, c, gy, wt, gap_gy=1):
    lib = capi.lib
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    _, lgy, ldx = dr.layouts(c, gap_gy=gap_gy, gap_dx=1)
    gh = bf16_buffer(capi, lgy, c.n, ho, wo, c.c, gy.numpy())
    gbuf = dev16(gh, dev)
    dbuf = dev32(f32_buffer(capi, ldx, c.n, c.h, c.w, c.c, zero_gaps=False), dev)
    w_whole, w9 = guarded(9 * c.c, dev)
    w9.copy_(torch.from_numpy(dr.tap_major(wt.numpy())).reshape(-1))
    w9h = cd.np_bits(w9)
    capi.check(lib.rtpose_dwconv3x3_dgrad_bf16(capi.ptr(gbuf), L(capi, lgy), capi.ptr(w9), capi.ptr(dbuf), L(capi, ldx), c.c, c.n, c.h,
                                               c.w, c.stride, capi.current_stream()), "rtpose_dwconv3x3_dgrad_bf16")
    torch.cuda.synchronize()
    assert np.array_equal(bits16(gbuf), gh) and np.array_equal(cd.np_bits(w9), w9h) and guards_intact(w_whole, 9 * c.c)
    bits, idx = cd.np_bits(dbuf), lr.index(ldx, c.n, c.h, c.w, c.c)
    assert lr.untouched(bits, idx, cd.SENTINEL), "dgrad wrote outside the valid pixels of the slice"
    return np.ascontiguousarray(np.transpose(bits[idx], (0, 3, 1, 2))).view(np.float32)


def forward_geometry(c):
    """the forward's case of a shape: (channels rounded up to 8, lin in bf16 elements, lout in floats), 16-byte aligned"""
    cf = -(-c.c // 8) * 8
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    return cf, lr.padded(cf + 8, c.h, c.w, 1, 8), lr.padded(cf + 8, ho, wo, 1, 4)


def pad_channels(t, cf, dim=1):
    """zeros appended along `dim` up to cf channels"""
    if cf == t.shape[dim]:
        return t
    shape = list(t.shape)
    shape[dim] = cf - t.shape[dim]
    return torch.cat([t, torch.zeros(shape)], dim)


def run_forward16(capi, dev, c, x, wt, bias):
    """y float32 [n, cf, ho, wo] of the shape's channels rounded up to 8 (the added ones: zero input, taps and bias)"""
    lib = capi.lib
    cf, lin, lout = forward_geometry(c)
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    xh = bf16_buffer(capi, lin, c.n, c.h, c.w, cf, pad_channels(x, cf).numpy())
    xbuf = dev16(xh, dev)
    obuf = dev32(f32_buffer(capi, lout, c.n, ho, wo, cf, zero_gaps=False), dev)
    w_whole, w9 = guarded(9 * cf, dev)
    w9.copy_(torch.from_numpy(dr.tap_major(pad_channels(wt, cf, 0).numpy())).reshape(-1))
    b_whole, bb = guarded(cf, dev)
    bb.copy_(pad_channels(bias.reshape(1, -1), cf).reshape(-1))
    capi.check(lib.rtpose_dwconv3x3_bf16_f32(capi.ptr(xbuf), L(capi, lin), capi.ptr(w9), capi.ptr(bb), capi.ptr(obuf), L(capi, lout),
                                             cf, c.n, c.h, c.w, c.stride, capi.current_stream()), "rtpose_dwconv3x3_bf16_f32")
    torch.cuda.synchronize()
    assert np.array_equal(bits16(xbuf), xh) and guards_intact(w_whole, 9 * cf) and guards_intact(b_whole, cf)
    bits, idx = cd.np_bits(obuf), lr.index(lout, c.n, ho, wo, cf)
    assert lr.untouched(bits, idx, cd.SENTINEL), "the forward wrote outside the valid pixels of the slice"
    return np.ascontiguousarray(np.transpose(bits[idx], (0, 3, 1, 2))).view(np.float32)


# ---- the existing fp32 kernels on the widened operands ----------------------------------------------------------------------------------------
def _plain32(capi, dev, lay, n, h, w, t):
    a = np.zeros(cd.npx(capi, lay, n, h, w) * lay.cstride, np.float32)
    return torch.from_numpy(lr.scatter(a, lay, t.numpy())).to(dev)


def fp32_wgrad(capi, dev, c, x, gy):
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    c4 = -(-c.c // 4) * 4
    lx, lgy = lr.padded(c4, c.h, c.w, 1), lr.dense(c4, ho, wo)
    xbuf, gbuf = _plain32(capi, dev, lx, c.n, c.h, c.w, x), _plain32(capi, dev, lgy, c.n, ho, wo, gy)
    doubles = capi.lib.rtpose_dwconv3x3_wgrad_workspace_doubles(c.c, c.n, c.h, c.w, c.stride)
    ws = torch.empty(doubles, dtype=torch.float64, device=dev)
    dw, dbias = torch.empty(c.c * 9, device=dev), torch.empty(c.c, device=dev)
    capi.check(capi.lib.rtpose_dwconv3x3_wgrad(capi.ptr(xbuf), L(capi, lx), capi.ptr(gbuf), L(capi, lgy), capi.ptr(dw), capi.ptr(dbias),
                                               capi.ptr(ws), doubles, c.c, c.n, c.h, c.w, c.stride, capi.current_stream()),
               "rtpose_dwconv3x3_wgrad")
    return dw.cpu().numpy().reshape(c.c, 1, 3, 3), dbias.cpu().numpy()


def fp32_dgrad(capi, dev, c, gy, wt):
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    c4 = -(-c.c // 4) * 4
    lgy, ldx = lr.padded(c4, ho, wo, 1), lr.dense(c4, c.h, c.w)
    gbuf = _plain32(capi, dev, lgy, c.n, ho, wo, gy)
    dbuf = torch.zeros(cd.npx(capi, ldx, c.n, c.h, c.w) * ldx.cstride, device=dev)
    w9 = torch.from_numpy(dr.tap_major(wt.numpy())).to(dev)
    capi.check(capi.lib.rtpose_dwconv3x3_dgrad(capi.ptr(gbuf), L(capi, lgy), capi.ptr(w9), capi.ptr(dbuf), L(capi, ldx), c.c, c.n, c.h,
                                               c.w, c.stride, capi.current_stream()), "rtpose_dwconv3x3_dgrad")
    return lr.gather(dbuf.cpu().numpy(), ldx, c.n, c.h, c.w, c.c)


def fp32_forward(capi, dev, c, x, wt, bias):
    cf = -(-c.c // 8) * 8
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    lin, lout = lr.padded(cf, c.h, c.w, 1), lr.dense(cf, ho, wo)
    xbuf = _plain32(capi, dev, lin, c.n, c.h, c.w, pad_channels(x, cf))
    obuf = torch.zeros(cd.npx(capi, lout, c.n, ho, wo) * lout.cstride, device=dev)
    w9 = torch.from_numpy(dr.tap_major(pad_channels(wt, cf, 0).numpy())).to(dev)
    bb = pad_channels(bias.reshape(1, -1), cf).reshape(-1).to(dev)
    capi.check(capi.lib.rtpose_dwconv3x3(capi.ptr(xbuf), L(capi, lin), capi.ptr(w9), capi.ptr(bb), capi.ptr(obuf), L(capi, lout), cf,
                                         c.n, c.h, c.w, c.stride, capi.current_stream()), "rtpose_dwconv3x3")
    return lr.gather(obuf.cpu().numpy(), lout, c.n, ho, wo, cf)


def _bias(c):
    return torch.randn(c.c, generator=torch.Generator().manual_seed(70 + c.c))


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("c", db.CASES, ids=db.case_id)
def test_backward_kernels_bit_for_bit(capi, cuda, c, kind):
    x, gy, wt = (db.exact_operands if kind == "exact" else db.random_operands)(c)
    dw64, db64, _, _ = dr.wgrad_restate(x.numpy(), gy.numpy(), c.stride)
    dw, dbias = run_wgrad16(capi, cuda, c, x, gy)
    assert same_bits(dw, dw64.astype(np.float32)), "dw against the restatement"
    assert same_bits(dbias, db64.astype(np.float32)), "dbias against the restatement"
    dw32, db32 = fp32_wgrad(capi, cuda, c, x, gy)
    assert same_bits(dw, dw32) and same_bits(dbias, db32), "against rtpose_dwconv3x3_wgrad on the widened operands"
    dw2, db2 = run_wgrad16(capi, cuda, c, x, gy, bias=False, gap_x=2)
    assert db2 is None and same_bits(dw2, dw), "a second run, without dbias, a wider gap"
    dx = run_dgrad16(capi, cuda, c, gy, wt)
    assert same_bits(dx, dr.dgrad_restate(gy.numpy(), wt.numpy(), c.h, c.w, c.stride)), "dx against the restatement"
    assert same_bits(dx, fp32_dgrad(capi, cuda, c, gy, wt)), "against rtpose_dwconv3x3_dgrad on the widened gy"
    assert same_bits(run_dgrad16(capi, cuda, c, gy, wt, gap_gy=2), dx), "a second run, a wider gap"
    if kind == "exact":
        _, dx64, dwa = dr.autograd64(x, wt, gy, c.stride)
        assert np.array_equal(dx.astype(np.float64), dx64.numpy()) and np.array_equal(dw.astype(np.float64), dwa.numpy())


_FORWARD_CASES = [c for c in db.CASES if c.tags == "x8"]


@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("c", _FORWARD_CASES, ids=db.case_id)
def test_forward_kernel_bit_for_bit(capi, cuda, c, kind):
    x, gy, wt = (db.exact_operands if kind == "exact" else db.random_operands)(c)
    bias = _bias(c).round() if kind == "exact" else _bias(c)
    y = run_forward16(capi, cuda, c, x, wt, bias)
    want = db.forward_restate(x.numpy(), wt.numpy(), c.stride, bias.numpy())
    assert same_bits(y[:, :c.c], want), "against the restatement"
    assert not y[:, c.c:].any(), "the channels added to reach a multiple of 8"
    assert same_bits(y, fp32_forward(capi, cuda, c, x, wt, bias)), "against rtpose_dwconv3x3 on the widened input"
    assert same_bits(run_forward16(capi, cuda, c, x, wt, bias), y), "a second run"
    if kind == "exact":
        y64 = dr.autograd64(x, wt, gy, c.stride)[0] + bias.double().reshape(1, -1, 1, 1)
        assert np.array_equal(y[:, :c.c].astype(np.float64), y64.numpy())


@pytest.mark.parametrize("c", [c for c in db.CASES if (c.n, c.c, c.h, c.w) == (2, 8, 9, 11)], ids=db.case_id)
def test_non_finite_values_come_out_where_the_fp32_kernels_put_them(capi, cuda, c):
    x, gy, wt = db.random_operands(c, seed=1)
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    x[0, 1, 2, 3], x[1, 5, c.h - 1, 0] = float("nan"), float("inf")
    gy[1, 2, 1, 1], gy[0, 6, ho - 1, wo - 1] = float("nan"), float("-inf")
    dw, dbias = run_wgrad16(capi, cuda, c, x, gy)
    dw32, db32 = fp32_wgrad(capi, cuda, c, x, gy)
    assert same_bits_or_nan(dw, dw32) and same_bits_or_nan(dbias, db32)
    assert np.isnan(dw[1]).any() and np.isnan(dw[2]).all() and np.isnan(dbias[2]) and np.isinf(dbias[6])
    assert not np.isfinite(dw[5]).all() and np.isfinite(dw[[0, 3, 4, 7]]).all() and np.isfinite(dbias[[0, 1, 3, 4, 5, 7]]).all()
    dx = run_dgrad16(capi, cuda, c, gy, wt)
    dx32 = fp32_dgrad(capi, cuda, c, gy, wt)
    assert same_bits_or_nan(dx, dx32) and np.isnan(dx[1, 2]).any() and np.isinf(dx[0, 6]).any()
    assert np.isfinite(np.delete(dx, (2, 6), 1)).all()
    if c.tags == "x8":
        bias = _bias(c)
        y = run_forward16(capi, cuda, c, x, wt, bias)
        y32 = fp32_forward(capi, cuda, c, x, wt, bias)
        assert same_bits_or_nan(y, y32) and np.isnan(y[0, 1]).any() and np.isinf(y[1, 5]).any()
        assert np.isfinite(np.delete(y, (1, 5), 1)).all()


def test_refusals(capi, cuda):
    """every host refusal of the three launchers, on live device buffers none of which is written; then memory that is not
    the device's"""
    bufs = [torch.zeros(1 << 16, dtype=torch.float64, device=cuda) for _ in range(9)]
    live = dict(zip((db.P_IN, db.P_W, db.P_B, db.P_OUT, db.P_GY, db.P_DW, db.P_DB, db.P_WS, db.P_DX), (b.data_ptr() for b in bufs)))

    def on_device(a):
        return [live[v] if isinstance(v, int) and v in live else v for v in a]

    for entry, (who, make, faults) in db.ENTRY_POINTS.items():
        fn = getattr(capi.lib, entry)
        for name, fault, text in faults:
            lays, a = make(capi)
            a = on_device(a)
            fault(a, lays)             # (a fault that moves a base sets the table's own misaligned address: never followed)
            db.refused(capi, fn, who, a, text)
        lays, a = make(capi)
        a = on_device(a)
        host = np.zeros(1 << 16, np.float64)
        for i in [i for i, v in enumerate(a) if isinstance(v, int) and v in live.values()]:
            b = list(a)
            b[i] = host.ctypes.data
            assert fn(*b) == -1 and "device memory" in capi.last_error(), (entry, i)
    torch.cuda.synchronize()
    assert all(not b.any() for b in bufs), "a refused call wrote"


# ---- train.dwconv3x3(compute_dtype='bf16') ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train(pkg):
    import importlib
    from conftest import PKG_NAME
    return importlib.import_module(PKG_NAME + ".train")


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("subset", ("x", "w", "xw"))
def test_train_dwconv3x3_bf16_equals_float64_autograd_on_integers(capi, cuda, train, stride, subset):
    c = dr.Case(2, 12, 9, 11, stride, None, None, None, "")
    x, gy, wt = db.exact_operands(c)
    y64, dx64, dw64 = dr.autograd64(x, wt, gy, stride)
    xd = x.to(cuda).requires_grad_("x" in subset)
    wd = wt.to(cuda).requires_grad_("w" in subset)
    y = train.dwconv3x3(xd, wd, stride, compute_dtype='bf16')
    assert y.dtype == torch.float32 and torch.equal(y.detach().cpu().double(), y64)
    y.backward(gy.to(cuda))
    assert (xd.grad is not None) == ("x" in subset) and (wd.grad is not None) == ("w" in subset)
    if "x" in subset:
        assert xd.grad.dtype == torch.float32 and torch.equal(xd.grad.cpu().double(), dx64)
    if "w" in subset:
        assert wd.grad.dtype == torch.float32 and torch.equal(wd.grad.cpu().double(), dw64)


@pytest.mark.parametrize("stride", (1, 2))
def test_train_dwconv3x3_bf16_is_the_emulation_and_fp32_is_the_call_without_the_keyword(capi, cuda, train, stride):
    c = dr.Case(2, 12, 9, 11, stride, None, None, None, "")
    x, gy, wt = dr.random_operands(c)            # fp32 operands: the node rounds x and gy itself
    want_y, want_dx, want_dw = db.emulate(x.numpy(), wt.numpy(), gy.numpy(), stride)
    outs = {}
    for key, kw in (("bf16", dict(compute_dtype='bf16')), ("fp32", dict(compute_dtype='fp32')), ("default", {})):
        xd, wd = x.to(cuda).requires_grad_(True), wt.to(cuda).requires_grad_(True)
        y = train.dwconv3x3(xd, wd, stride, **kw)
        y.backward(gy.to(cuda))
        outs[key] = (y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu())
    assert all(torch.equal(a, b) for a, b in zip(outs["fp32"], outs["default"]))
    y, dx, dw = (t.numpy() for t in outs["bf16"])
    assert same_bits(y, want_y) and same_bits(dx, want_dx) and same_bits(dw, want_dw.astype(np.float32))
    assert not torch.equal(outs["bf16"][0], outs["fp32"][0])
