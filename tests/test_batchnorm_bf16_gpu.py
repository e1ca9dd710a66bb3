"""GPU suite of the bf16 BatchNorm passes (header section 2b continued, csrc/batchnorm.hip): rtpose_bn_apply_bf16 and
rtpose_bn_grad_bf16 on slices of wider buffers - the fp32 inputs hold conv_driver.SENTINEL NaNs in their other channels and
gaps, the bf16 destination the bf16 NaN SENT16 everywhere; after every launch everything outside the destination's valid
pixels and channels is intact, bit for bit, and so is every input.

Every case of tests/bn_bf16_restate.py: y and dx bit for bit the restatement's, from the per-channel vectors the launch read
(save) and wrote (A, B, C).  Exact dyadic sets: y, dx, dweight, dbias and A, B, C == the float64 values (rounded to bf16 where
the kernel rounds).  test_split_equals_fused is what lets train.preact_chain claim the per-conv path's bits: rtpose_bn_apply /
rtpose_bn_grad followed by rtpose_layout_f32_to_bf16 give the same 16 bits on the same inputs, and rtpose_bn_grad the same
dweight, dbias and A, B, C."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_bf16_restate as bb
import bn_restate as br
import conv_driver as cd
import layout_restate as lr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel floats on either side of dweight, dbias and the workspace
SENT16 = 0x7FC1         # a bf16 NaN no result here has: the restatement's NaNs are 0x7FC0 | sign, and no operand rounds to it


def sent32(capi, lay, c, bits):
    a = np.full(cd.npx(capi, lay, c.n, c.h, c.w) * lay.cstride, cd.SENTINEL, dtype=np.uint32)
    return lr.scatter(a, lay, np.ascontiguousarray(bits, dtype=np.uint32))


def dev32(a, dev):
    return torch.from_numpy(a.view(np.int32).copy()).to(dev).view(torch.float32)


def dev16(capi, lay, c, dev, shift):
    """the bf16 destination, SENT16 everywhere: (whole tensor, the view that starts `shift` elements in)"""
    numel = cd.npx(capi, lay, c.n, c.h, c.w) * lay.cstride
    whole = torch.full((numel + shift,), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return whole, whole[shift:]


def guarded(numel, dev):
    whole = torch.full((numel + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + numel].view(torch.float32)


def guards_intact(whole, numel):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + numel:] == cd.SENTINEL).all())


def nhwc(a):
    return np.transpose(a, (0, 2, 3, 1))


def bits32(t):
    return np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t, dtype=np.float32).view(np.uint32)


def host_save(x, w, b):
    """the six save rows by the header's fp64 expressions (bn_restate.stats_restate): what the two passes read"""
    return br.stats_restate(x.numpy(), w.numpy(), b.numpy())[0]


def apply16(capi, dev, c, x_bits, save, relu):
    """rtpose_bn_apply_bf16 of the case: y's bits, NHWC"""
    lx, _, ly = bb.layouts(c)
    xh = sent32(capi, lx, c, x_bits)
    xbuf, sv = dev32(xh, dev), torch.from_numpy(np.ascontiguousarray(save, np.float32).reshape(-1).copy()).to(dev)
    whole, ybuf = dev16(capi, ly, c, dev, c.shift)
    capi.check(capi.lib.rtpose_bn_apply_bf16(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(sv), capi.ptr(ybuf),
                                             C.byref(cd.L(capi, ly)), 1 if relu else 0, c.channels, c.n, c.h, c.w,
                                             capi.current_stream()), "rtpose_bn_apply_bf16")
    torch.cuda.synchronize()
    bits, iy = cd.np_bits(whole), lr.index(ly, c.n, c.h, c.w, c.channels) + c.shift
    assert lr.untouched(bits, iy, SENT16), "bn_apply_bf16 wrote outside the valid pixels and channels of the slice"
    assert np.array_equal(cd.np_bits(xbuf), xh), "x was modified"
    return bits[iy]


def grad(capi, dev, c, x_bits, gy_bits, save, weight, relu, want="xwb", bf16=True):
    """rtpose_bn_grad_bf16 of the case - or, bf16 False, rtpose_bn_grad into a dense fp32 buffer followed by
    rtpose_layout_f32_to_bf16: a dict of dx (uint16 NHWC or None), dw, db (uint32 bits or None), coef (uint32 [3, ch] or None)"""
    lib, ch = capi.lib, c.channels
    lx, lgy, lout = bb.layouts(c)
    stream = capi.current_stream()
    xh, gh = sent32(capi, lx, c, x_bits), sent32(capi, lgy, c, gy_bits)
    xbuf, gbuf = dev32(xh, dev), dev32(gh, dev)
    sv = torch.from_numpy(np.ascontiguousarray(save, np.float32).reshape(-1).copy()).to(dev)
    wd = weight.float().contiguous().to(dev)
    doubles, slabs = lib.rtpose_bn_workspace_doubles(ch, c.n, c.h, c.w), lib.rtpose_bn_slabs(ch, c.n, c.h, c.w)
    dw_whole, dw = guarded(ch, dev)
    db_whole, db = guarded(ch, dev)
    w_whole, ws = guarded(2 * doubles, dev)
    need_x, need_w, need_b = ("x" in want), ("w" in want), ("b" in want)
    cp = (ch + 7) // 8 * 8
    l32 = lr.dense(cp, c.h, c.w)
    if bf16:
        whole, dbuf = dev16(capi, lout, c, dev, c.shift)
        ld, fn, name = lout, lib.rtpose_bn_grad_bf16, "rtpose_bn_grad_bf16"
    else:
        whole = dbuf = torch.zeros(cd.npx(capi, l32, c.n, c.h, c.w) * cp, dtype=torch.float32, device=dev)
        ld, fn, name = l32, lib.rtpose_bn_grad, "rtpose_bn_grad"
    capi.check(fn(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(gbuf), C.byref(cd.L(capi, lgy)), capi.ptr(sv), capi.ptr(wd),
                  1 if relu else 0, capi.ptr(dbuf) if need_x else None, C.byref(cd.L(capi, ld)) if need_x else None,
                  capi.ptr(dw) if need_w else None, capi.ptr(db) if need_b else None, capi.ptr(ws), doubles, ch, c.n, c.h, c.w,
                  stream), name)
    out = dict(dx=None, coef=None)
    if bf16:
        torch.cuda.synchronize()
        bits, idx = cd.np_bits(whole), lr.index(lout, c.n, c.h, c.w, ch) + c.shift
        if need_x:
            assert lr.untouched(bits, idx, SENT16), "bn_grad_bf16 wrote outside the valid pixels and channels of the slice"
            out["dx"] = bits[idx]
        else:
            assert (bits == SENT16).all(), "dx = NULL but something was written"
    elif need_x:
        h = torch.zeros(cd.npx(capi, l32, c.n, c.h, c.w) * cp, dtype=torch.bfloat16, device=dev)
        capi.check(lib.rtpose_layout_f32_to_bf16(capi.ptr(dbuf), C.byref(cd.L(capi, l32)), capi.ptr(h), C.byref(cd.L(capi, l32)), ch,
                                                 cp, c.n, c.h, c.w, stream), "rtpose_layout_f32_to_bf16")
        torch.cuda.synchronize()
        out["dx"] = cd.np_bits(h)[lr.index(l32, c.n, c.h, c.w, ch)]
    torch.cuda.synchronize()
    assert np.array_equal(cd.np_bits(xbuf), xh) and np.array_equal(cd.np_bits(gbuf), gh), "x or gy was modified"
    assert guards_intact(dw_whole, ch) and guards_intact(db_whole, ch) and guards_intact(w_whole, 2 * doubles)
    if need_x:
        out["coef"] = cd.np_bits(ws)[4 * slabs * ch:][:3 * ch].reshape(3, ch).copy()
    out["dw"] = cd.np_bits(dw).copy() if need_w else None
    out["db"] = cd.np_bits(db).copy() if need_b else None
    if not need_w:
        assert (cd.np_bits(dw) == cd.SENTINEL).all(), "dweight = NULL but written"
    if not need_b:
        assert (cd.np_bits(db) == cd.SENTINEL).all(), "dbias = NULL but written"
    return out


def apply_split(capi, dev, c, x_bits, save, relu):
    """rtpose_bn_apply into a dense fp32 buffer followed by rtpose_layout_f32_to_bf16: y's bits, NHWC"""
    lib, ch = capi.lib, c.channels
    lx, _, _ = bb.layouts(c)
    cp = (ch + 7) // 8 * 8
    l32 = lr.dense(cp, c.h, c.w)
    xbuf = dev32(sent32(capi, lx, c, x_bits), dev)
    sv = torch.from_numpy(np.ascontiguousarray(save, np.float32).reshape(-1).copy()).to(dev)
    numel = cd.npx(capi, l32, c.n, c.h, c.w) * cp
    y32 = torch.zeros(numel, dtype=torch.float32, device=dev)
    h = torch.zeros(numel, dtype=torch.bfloat16, device=dev)
    capi.check(lib.rtpose_bn_apply(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(sv), capi.ptr(y32), C.byref(cd.L(capi, l32)),
                                   1 if relu else 0, ch, c.n, c.h, c.w, capi.current_stream()), "rtpose_bn_apply")
    capi.check(lib.rtpose_layout_f32_to_bf16(capi.ptr(y32), C.byref(cd.L(capi, l32)), capi.ptr(h), C.byref(cd.L(capi, l32)), ch, cp,
                                             c.n, c.h, c.w, capi.current_stream()), "rtpose_layout_f32_to_bf16")
    torch.cuda.synchronize()
    return cd.np_bits(h)[lr.index(l32, c.n, c.h, c.w, ch)]


def differing(got, want):
    same = bb.same_bf16(got, want)
    return "%d of %d elements differ" % (int((~same).sum()), same.size)


# ---- 1. every case against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", bb.CASES, ids=bb.case_id)
def test_cases_bit_for_bit(capi, cuda, c):
    x, gy, w, b, _, _ = bb.random_operands(c)
    save = host_save(x, w, b)
    xb, gb = bits32(x), bits32(gy)
    for relu in (False, True):
        y = apply16(capi, cuda, c, xb, save, relu)
        want = nhwc(bb.apply_bf16_restate(x.numpy(), save, relu))
        assert bb.same_bf16(y, want).all(), "y (relu %s): %s" % (relu, differing(y, want))
        r = grad(capi, cuda, c, xb, gb, save, w, relu)
        want = nhwc(bb.dx_bf16_restate(x.numpy(), gy.numpy(), save, r["coef"].view(np.float32), relu))
        assert bb.same_bf16(r["dx"], want).all(), "dx (relu %s): %s" % (relu, differing(r["dx"], want))
        if relu and y.size >= 64:
            assert (y == 0).any() and (y != 0).any()


# ---- 2. exact (dyadic) sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", bb.SMALL, ids=bb.case_id)
def test_exact_sets_equal_float64(capi, cuda, c):
    x, gy, save, weight = bb.exact_set(c)
    for relu in (False, True):
        y64, dx64, db64, dw64, coef64 = bb.exact64(x, gy, save, weight, relu)
        y = apply16(capi, cuda, c, bits32(x), save, relu)
        want = torch.from_numpy(nhwc(y64).copy()).to(torch.bfloat16).double().numpy()
        assert np.array_equal(bb.bf16_f64(y), want), "y (relu %s)" % relu
        if not bb.is_pow2(c.n * c.h * c.w):
            continue
        r = grad(capi, cuda, c, bits32(x), bits32(gy), save, weight, relu)
        f64 = lambda bits: bits.view(np.float32).astype(np.float64)                     # noqa: E731
        assert np.array_equal(f64(r["db"]), db64) and np.array_equal(f64(r["dw"]), dw64), "dbias / dweight (relu %s)" % relu
        assert np.array_equal(f64(r["coef"]), coef64), "A, B, C (relu %s)" % relu
        want = torch.from_numpy(nhwc(dx64).copy()).to(torch.bfloat16).double().numpy()
        assert np.array_equal(bb.bf16_f64(r["dx"]), want), "dx (relu %s)" % relu


# ---- 3. split equals fused ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unit", "mean1000std"])
@pytest.mark.parametrize("c", bb.SMALL, ids=bb.case_id)
def test_split_equals_fused(capi, cuda, c, kind):
    """y: rtpose_bn_apply -> rtpose_layout_f32_to_bf16 on the same inputs; dx: rtpose_bn_grad -> rtpose_layout_f32_to_bf16;
    dweight, dbias and A, B, C: rtpose_bn_grad's bits.  Then the same results with dweight, dbias or dx NULL."""
    x, gy, w, b, _, _ = bb.random_operands(c, seed=1, big_mean=kind == "mean1000std")
    save = host_save(x, w, b)
    xb, gb = bits32(x), bits32(gy)
    for relu in (False, True):
        y, y2 = apply16(capi, cuda, c, xb, save, relu), apply_split(capi, cuda, c, xb, save, relu)
        assert np.array_equal(y, y2), "y (relu %s): %s" % (relu, differing(y, y2))
        r, r2 = grad(capi, cuda, c, xb, gb, save, w, relu), grad(capi, cuda, c, xb, gb, save, w, relu, bf16=False)
        assert np.array_equal(r["dx"], r2["dx"]), "dx (relu %s): %s" % (relu, differing(r["dx"], r2["dx"]))
        for k in ("dw", "db", "coef"):
            assert np.array_equal(r[k], r2[k]), "%s (relu %s)" % (k, relu)
        rx = grad(capi, cuda, c, xb, gb, save, w, relu, want="x")
        assert rx["dw"] is None and rx["db"] is None and np.array_equal(rx["dx"], r["dx"]) and np.array_equal(rx["coef"], r["coef"])
        rp = grad(capi, cuda, c, xb, gb, save, w, relu, want="wb")
        assert rp["dx"] is None and np.array_equal(rp["dw"], r["dw"]) and np.array_equal(rp["db"], r["db"])
        rw = grad(capi, cuda, c, xb, gb, save, w, relu, want="xw")
        assert rw["db"] is None and np.array_equal(rw["dw"], r["dw"]) and np.array_equal(rw["dx"], r["dx"])
        again = grad(capi, cuda, c, xb, gb, save, w, relu)
        assert all(np.array_equal(again[k], r[k]) for k in ("dx", "dw", "db", "coef")), "two runs gave different bits"


# ---- 4. the apply over every upper half of x ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shift", [0, 1], ids=["units of 4", "element by element"])
def test_apply_over_every_upper_half(capi, cuda, shift, relu):
    """all 65,536 upper halves of x under the lower halves 0x0000, 0x7FFF, 0x8000, 0x8001 and 0xFFFF with scale 1 and shift 0:
    every rounding case, both zeros, subnormals, both Infs and every NaN class, through the 8-byte store and the 2-byte one"""
    bits = bb.sweep_bits()
    c = bb.Case(4, 1, 512, 640, (4, 0), (4, 0), (4, 0), 0, shift, "")
    x_bits = np.stack([bits] * 4).reshape(1, 4, 512, 640)
    save = np.zeros((6, 4), dtype=np.float32)
    save[3] = 1.0
    y = apply16(capi, cuda, c, x_bits, save, relu)
    want = nhwc(bb.apply_bf16_restate(x_bits.view(np.float32), save, relu))
    same = bb.same_bf16(y, want)
    assert same.all(), "%d of %d differ; first x bits %s" % (int((~same).sum()), same.size,
                                                              [hex(v) for v in nhwc(x_bits)[~same][:6].tolist()])
    nan = nhwc(bb.is_nan32(x_bits))
    assert bb.is_nan16(y[nan]).all() and not bb.is_nan16(y[~nan]).any()
    pinf = nhwc(x_bits == 0x7F800000)
    assert (y[pinf] == 0x7F80).all()
    assert (y[nhwc(x_bits == 0xFF800000)] == (0 if relu else 0xFF80)).all()


# ---- 5. NaN and Inf -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [bb.CASES[12], bb.CASES[13]], ids=bb.case_id)
def test_nan_and_inf_follow_the_fp32_pair(capi, cuda, c):
    """a NaN and an Inf in x and in gy, one channel each: every output has the class the fp32 pair gives it in that channel,
    then rounded; the other channels are untouched by them"""
    x0, gy0, w, b, _, _ = bb.random_operands(c, seed=2)
    assert w[1] != 0 and w[5] != 0                     # (bn_restate.affine zeroes weight 2: an Inf of x there would be 0 * Inf)
    save = host_save(x0, w, b)
    x, gy = x0.clone(), gy0.clone()
    x[0, 1, 2, 3], x[1, 5, 0, 1] = float("nan"), float("inf")
    gy[0, 3, 1, 1], gy[1, 4, 2, 2] = float("nan"), float("-inf")
    xb, gb = bits32(x), bits32(gy)
    quiet = [ch for ch in range(c.channels) if ch not in (1, 5, 3, 4)]
    for relu in (False, True):
        y, y2 = apply16(capi, cuda, c, xb, save, relu), apply_split(capi, cuda, c, xb, save, relu)
        assert bb.same_bf16(y, y2).all() and bb.is_nan16(y[0, 2, 3, 1]) and bb.is_nan16(y).sum() == 1
        assert (y[1, 0, 1, 5] & 0x7FFF) == 0x7F80 or (relu and y[1, 0, 1, 5] == 0)
        r, r2 = grad(capi, cuda, c, xb, gb, save, w, relu), grad(capi, cuda, c, xb, gb, save, w, relu, bf16=False)
        assert bb.same_bf16(r["dx"], r2["dx"]).all(), differing(r["dx"], r2["dx"])
        for k in ("dw", "db", "coef"):
            assert np.array_equal(r[k], r2[k]), k
        want = nhwc(bb.dx_bf16_restate(x.numpy(), gy.numpy(), save, r["coef"].view(np.float32), relu))
        assert bb.same_bf16(r["dx"], want).all()
        clean = grad(capi, cuda, c, bits32(x0), bits32(gy0), save, w, relu)
        assert np.array_equal(r["dx"][..., quiet], clean["dx"][..., quiet]), "a non-finite value left its channel"
        assert np.array_equal(r["dw"][quiet], clean["dw"][quiet]) and np.array_equal(r["db"][quiet], clean["db"][quiet])
        if not relu:
            assert np.isnan(r["db"].view(np.float32)[3]) and np.isinf(r["db"].view(np.float32)[4])
            assert bb.is_nan16(r["dx"][..., 1]).all() and bb.is_nan16(r["dx"][..., 3]).all()
