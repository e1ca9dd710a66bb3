"""GPU suite of rtpose_conv2d_wgrad_bf16 (header section 2b, continued; csrc/conv_backward.hip): the weight and bias
gradient of a stride-1 "same" conv from bf16 slices of wider buffers.

Buffers: bf16 NaN (0x7FC0) in every channel beside a slice - the pad channels that share a 16-byte group with its last
channels included - and, for gy, at every pixel of its gaps; the gaps of the x slice are zero.  dw, dbias and the workspace
sit between sentinel words.

Exact cases (conv_backward_bf16_restate.EXACT_CASES): the operands are integers bf16 holds, every product and every partial
sum an integer below 2^24 (tests/test_conv_backward_bf16_cpu.py holds the cases to that), so fp32 accumulation in any order
is exact and the float64 reference is compared with ==.  One dropped, doubled or transposed (pixel, channel) term changes an
integer.

Bounded cases: x = rb(relu(randn)), gy = rb(randn), rounded on the host, against wgrad64 / dbias64 of those rounded tensors.
Required |err| <= 2 gamma_(n+1) S, n = N H W, u = 2^-24: products of bf16 values are exact in fp32, so only the adds round; the
adder inside one MFMA is not documented to round to nearest at each add, and a truncating adder has unit error 2 u - hence the
factor 2 over the fp32 kernel's bound.  The worst err / bound of every case goes through conv_driver.note
(profiles/r28_bf16_training.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_backward_bf16_restate as cb
import conv_driver as cd
import layout_restate as lr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel floats on either side of an output
NAN16 = 0x7FC0


def up8(c):
    return (c + 7) // 8 * 8


def host_buffer(capi, lay, n, h, w, t, zero_channels, gaps_zero):
    """A bf16 layout buffer on the host (uint16): NaN everywhere; with gaps_zero, zero in `zero_channels` channels from
    lay.choff of every pixel (the slice and its gaps); the tensor t [n, c, h, w] at the valid pixels of the slice."""
    a = np.full((cd.npx(capi, lay, n, h, w), lay.cstride), NAN16, dtype=np.uint16)
    if gaps_zero:
        a[:, lay.choff:lay.choff + zero_channels] = 0
    bits = lr.bf16_rne(t.numpy())
    assert np.array_equal(lr.bf16_to_f32(bits), t.numpy()), "the operands are bf16 values already"
    return lr.scatter(a.reshape(-1), lay, bits.reshape(t.shape))


def to_device(a, dev):
    return torch.from_numpy(a.view(np.int16)).to(dev)


def guarded(numel, dev):
    """(whole buffer of sentinel words, the 16-byte aligned view of `numel` floats inside it)"""
    whole = torch.full((numel + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + numel].view(torch.float32)


def guards_intact(whole, numel):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + numel:] == cd.SENTINEL).all())


_problems = {}


def problem(capi, dev, c, exact):
    """The case's tensors, buffers and float64 references, made once and left unchanged."""
    key = ("exact_" if exact else "") + cb.case_id(c)
    if key not in _problems:
        x, gy = cb.exact_operands(c)[:2] if exact else cb.case_tensors(c)
        lx = lr.padded(c.x_cs, c.h, c.w, c.k // 2 + (c.gap if exact else 0), c.x_off)
        lgy = lr.padded(up8(c.cout) + 16, c.h, c.w, c.k // 2, 8)
        p = dict(lx=lx, lgy=lgy)
        p["xbuf"] = to_device(host_buffer(capi, lx, c.n, c.h, c.w, x, c.cin, True), dev)
        p["gbuf"] = to_device(host_buffer(capi, lgy, c.n, c.h, c.w, gy, c.cout, False), dev)
        p["dw64"], p["s_dw"] = cb.wgrad64(x, gy, c.k)
        p["db64"], p["s_db"] = cb.dbias64(gy)
        if exact:
            assert cb.exact_margin(c) < 2 ** 24
        _problems[key] = p
    return _problems[key]


def wgrad(capi, dev, c, p, want_bias=True):
    """One launch into fresh sentinel-guarded outputs: (dw bits, dbias bits or None), after the guard checks."""
    lib = capi.lib
    nw = c.cout * c.cin * c.k * c.k
    floats = lib.rtpose_conv2d_wgrad_bf16_workspace_floats(c.cin, c.cout, c.k, c.n, c.h, c.w)
    w_whole, dw = guarded(nw, dev)
    b_whole, db = guarded(c.cout, dev)
    s_whole, ws = guarded(floats, dev)
    d = capi.WgradBf16Desc()
    d.x, d.gy, d.dw, d.workspace = p["xbuf"].data_ptr(), p["gbuf"].data_ptr(), dw.data_ptr(), ws.data_ptr()
    d.dbias = db.data_ptr() if want_bias else None
    d.workspace_floats = floats
    d.lx, d.lgy = cd.L(capi, p["lx"]), cd.L(capi, p["lgy"])
    d.cin, d.cout, d.k = c.cin, c.cout, c.k
    capi.check(lib.rtpose_conv2d_wgrad_bf16(C.byref(d), c.n, c.h, c.w, capi.current_stream()), "rtpose_conv2d_wgrad_bf16")
    torch.cuda.synchronize()
    assert guards_intact(w_whole, nw), "written outside dw"
    assert guards_intact(s_whole, floats), "written outside the workspace"
    assert guards_intact(b_whole, c.cout), "written outside dbias"
    if not want_bias:
        assert (cd.np_bits(db) == cd.SENTINEL).all(), "dbias = NULL but written"
    return cd.np_bits(dw), cd.np_bits(db) if want_bias else None


def mismatch(got, want):
    bad = np.flatnonzero(got.ravel() != want.ravel())
    return "%d of %d differ, first at %s: %r != %r" % (bad.size, want.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


@pytest.mark.parametrize("c", cb.EXACT_CASES, ids=cb.case_id)
def test_weight_and_bias_gradient_exact(capi, cuda, c):
    """dw and dbias equal the float64 sums of the integer operands, with and without dbias; the workspace held sentinel
    words, so the result does not depend on what it held."""
    p = problem(capi, cuda, c, True)
    slabs = capi.lib.rtpose_conv2d_wgrad_bf16_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
    assert ("several slabs" in c.tags) == (slabs >= 2)
    want_w, want_b = p["dw64"].float().numpy().ravel(), p["db64"].float().numpy()
    dw_bits, db_bits = wgrad(capi, cuda, c, p)
    dw, db = dw_bits.view(np.float32), db_bits.view(np.float32)
    print("wgrad bf16 exact %s: slabs %d, dw %d wrong of %d, dbias %d wrong of %d"
          % (cb.case_id(c), slabs, int((dw != want_w).sum()), dw.size, int((db != want_b).sum()), db.size))
    assert np.array_equal(dw, want_w), "dw: " + mismatch(dw, want_w)
    assert np.array_equal(db, want_b), "dbias: " + mismatch(db, want_b)
    dw2, _ = wgrad(capi, cuda, c, p, want_bias=False)
    assert np.array_equal(dw2.view(np.float32), want_w), "dw without dbias: " + mismatch(dw2.view(np.float32), want_w)


@pytest.mark.parametrize("c", cb.CASES, ids=cb.case_id)
def test_weight_and_bias_gradient(capi, cuda, c):
    p = problem(capi, cuda, c, False)
    n = c.n * c.h * c.w
    slabs = capi.lib.rtpose_conv2d_wgrad_bf16_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
    if "several slabs" in c.note:
        assert slabs >= 3 and n % cb.CHUNK != 0
    dw_bits, db_bits = wgrad(capi, cuda, c, p)
    dw = torch.from_numpy(dw_bits.view(np.float32).copy()).view(c.cout, c.cin, c.k, c.k).double()
    db = torch.from_numpy(db_bits.view(np.float32).copy()).double()
    # nothing outside the slices reached a sum (every channel beside them is NaN), every element was written
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    g = 2 * cb.gamma(n + 1)
    err_w, bound_w = (dw - p["dw64"]).abs(), g * p["s_dw"]
    err_b, bound_b = (db - p["db64"]).abs(), g * p["s_db"]
    ratio_w = (err_w / bound_w.clamp_min(1e-300)).max().item()
    ratio_b = (err_b / bound_b.clamp_min(1e-300)).max().item()
    print("wgrad bf16 %s: slabs %d, worst err/bound dw %.4g, dbias %.4g" % (cb.case_id(c), slabs, ratio_w, ratio_b))
    cd.note("conv_backward_bf16_wgrad_%s.json" % cb.case_id(c), {"slabs": slabs, "n": n, "dw_err_over_bound": ratio_w,
                                                                  "dbias_err_over_bound": ratio_b})
    assert (err_w <= bound_w).all(), "dw: worst err / bound %g" % ratio_w
    assert (err_b <= bound_b).all(), "dbias: worst err / bound %g" % ratio_b
    # the same inputs give the same bits; without dbias the same dw and an untouched dbias
    dw2, db2 = wgrad(capi, cuda, c, p)
    assert np.array_equal(dw_bits, dw2) and np.array_equal(db_bits, db2)
    dw3, _ = wgrad(capi, cuda, c, p, want_bias=False)
    assert np.array_equal(dw_bits, dw3)
