"""GPU suite of the bf16 PReLU passes (header section 2b continued, csrc/prelu_backward.hip): rtpose_prelu_bf16 and
rtpose_prelu_grad_bf16 on slices of wider buffers - four different layouts per case - whose other channels and gaps hold NaN
sentinels (conv_driver.SENTINEL in the fp32 inputs, SENT16 in the bf16 destination); after every launch everything outside
the destination's valid pixels is intact, bit for bit, and so is every input.

Exact sets (prelu_bf16_restate: integers, quarter slopes, |g| <= 6): y, out and dslope == float64 from F.prelu's CPU autograd.
Random operands with NaN payloads, -0, Inf and subnormals: y and out bit for bit the restatement's (a NaN for a NaN), dslope
within gamma(P + 1) * S of the float64 sum (conv_backward_restate.gamma); the worst err / bound goes through conv_driver.note.
test_split_equals_fused is what lets train.dense_stage claim the per-conv path's bits: rtpose_prelu_grad on torch's fp32
ga + gb followed by rtpose_layout_f32_to_bf16 gives the same 16 bits, and the same dslope where both take 4-channel units."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_backward_restate as cb
import conv_driver as cd
import layout_restate as lr
import prelu_bf16_restate as pb
import prelu_restate as pr
import test_prelu_bf16_cpu as host

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel floats on either side of dslope and the workspace
SENT16 = 0x7FC1         # a bf16 NaN no result here has: the restatement's NaNs are 0x7FC0 | sign, and no operand rounds to it


def sent32(capi, lay, c, bits=None):
    a = np.full(cd.npx(capi, lay, c.n, c.h, c.w) * lay.cstride, cd.SENTINEL, dtype=np.uint32)
    return a if bits is None else lr.scatter(a, lay, bits)


def dev32(a, dev):
    return torch.from_numpy(a.view(np.int32).copy()).to(dev).view(torch.float32)


def dev16(capi, lay, c, dev, shift=0):
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


def f64(bits):
    return bits.view(np.float32).astype(np.float64)


def forward(capi, dev, c, z_bits, slope, shift=0):
    """rtpose_prelu_bf16 of the case's z slice into the `out` layout: y's bits, NHWC.  shift: elements the bf16 base is moved
    by (2 bytes each: off the 8-byte alignment of the 4-channel units)"""
    lz, _, _, ly = pb.layouts(c)
    zh = sent32(capi, lz, c, z_bits)
    zbuf = dev32(zh, dev)
    whole, ybuf = dev16(capi, ly, c, dev, shift)
    sl = slope.to(dev)
    capi.check(capi.lib.rtpose_prelu_bf16(capi.ptr(zbuf), C.byref(cd.L(capi, lz)), capi.ptr(sl), capi.ptr(ybuf),
                                          C.byref(cd.L(capi, ly)), c.channels, c.n, c.h, c.w, capi.current_stream()),
               "rtpose_prelu_bf16")
    torch.cuda.synchronize()
    bits, iy = cd.np_bits(whole), lr.index(ly, c.n, c.h, c.w, c.channels) + shift
    assert lr.untouched(bits, iy, SENT16), "prelu_bf16 wrote outside the valid pixels of the slice"
    assert np.array_equal(cd.np_bits(zbuf), zh), "z was modified"
    return bits[iy]


def backward(capi, dev, c, z_bits, ga_bits, gb_bits, slope, want, shift=0):
    """rtpose_prelu_grad_bf16 of the case (gb_bits None: gb = NULL): (out's bits NHWC, dslope's bits or None).  want: with
    the slope gradient (else dslope and workspace are given as NULL, and sentinel-filled ones must stay as they are)"""
    lib = capi.lib
    lz, lga, lgb, lout = pb.layouts(c)
    zh, ah = sent32(capi, lz, c, z_bits), sent32(capi, lga, c, ga_bits)
    zbuf, abuf = dev32(zh, dev), dev32(ah, dev)
    bh = sent32(capi, lgb, c, gb_bits) if gb_bits is not None else None
    bbuf = dev32(bh, dev) if gb_bits is not None else None
    whole, obuf = dev16(capi, lout, c, dev, shift)
    sl = slope.to(dev)
    floats = lib.rtpose_prelu_grad_bf16_workspace_floats(c.channels, c.n, c.h, c.w)
    assert floats >= lib.rtpose_prelu_grad_bf16_slabs(c.channels, c.n, c.h, c.w) * c.channels > 0
    d_whole, ds = guarded(c.channels, dev)
    w_whole, ws = guarded(floats, dev)
    capi.check(lib.rtpose_prelu_grad_bf16(capi.ptr(zbuf), C.byref(cd.L(capi, lz)), capi.ptr(sl), capi.ptr(abuf),
                                          C.byref(cd.L(capi, lga)), capi.ptr(bbuf),
                                          C.byref(cd.L(capi, lgb)) if bbuf is not None else None, capi.ptr(obuf),
                                          C.byref(cd.L(capi, lout)), capi.ptr(ds) if want else None,
                                          capi.ptr(ws) if want else None, floats if want else 0, c.channels, c.n, c.h, c.w,
                                          capi.current_stream()), "rtpose_prelu_grad_bf16")
    torch.cuda.synchronize()
    bits, io = cd.np_bits(whole), lr.index(lout, c.n, c.h, c.w, c.channels) + shift
    assert lr.untouched(bits, io, SENT16), "written outside the valid pixels of the slice"
    assert np.array_equal(cd.np_bits(zbuf), zh) and np.array_equal(cd.np_bits(abuf), ah), "z or ga was modified"
    assert bbuf is None or np.array_equal(cd.np_bits(bbuf), bh), "gb was modified"
    assert guards_intact(d_whole, c.channels) and guards_intact(w_whole, floats), "written outside dslope / the workspace"
    if not want:
        assert (cd.np_bits(ds) == cd.SENTINEL).all() and (cd.np_bits(ws) == cd.SENTINEL).all(), "dslope = NULL but written"
    return bits[io], cd.np_bits(ds).copy() if want else None


# ---- 1. exact sets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pb.CASES, ids=pb.case_id)
def test_exact_sets_equal_float64(capi, cuda, c):
    """y, out and dslope equal the float64 reference with ==: two consumers and one, dslope given and NULL"""
    for kind, make in sorted(pb.EXACT_SETS.items()):
        z, ga, gb, slope = make(c)
        assert pb.exact_margin(z, ga, gb) < 2 ** 24
        zb, ab, bb = (t.numpy().view(np.uint32) for t in (z, ga, gb))
        y = forward(capi, cuda, c, zb, slope)
        assert np.array_equal(pb.bf16_f64(y), nhwc(pr.prelu64(z, ga, slope)[0].numpy())), (kind, "y")
        assert np.array_equal(y, nhwc(pb.prelu_bf16_bits(z.numpy(), slope.numpy()))), (kind, "y bits: the sign of a zero is z's")
        for two in (True, False):
            dz64, da64, _ = pb.grad64(z, ga, gb if two else None, slope)
            out, ds = backward(capi, cuda, c, zb, ab, bb if two else None, slope, want=True)
            wrong = int((pb.bf16_f64(out) != nhwc(dz64.numpy())).sum())
            assert wrong == 0, "%s out (gb %s): %d of %d elements differ" % (kind, two, wrong, out.size)
            bad = np.flatnonzero(f64(ds) != da64.numpy())
            assert bad.size == 0, "%s dslope (gb %s): channels %s differ" % (kind, two, bad[:8].tolist())
            out, ds = backward(capi, cuda, c, zb, ab, bb if two else None, slope, want=False)
            assert ds is None and np.array_equal(pb.bf16_f64(out), nhwc(dz64.numpy())), (kind, two, "out without dslope")


# ---- 2. random operands, repeatability, gb = NULL --------------------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize("c", pb.CASES, ids=pb.case_id)
def test_random_operands(capi, cuda, c):
    z, ga_bits, gb_bits, slope = pb.random_operands(c)
    zn, sn = z.numpy(), slope.numpy()
    zb = zn.view(np.uint32)
    y = forward(capi, cuda, c, zb, slope)
    assert pb.same_bf16(y, nhwc(pb.prelu_bf16_bits(zn, sn))).all(), "y"
    want2, want1 = nhwc(pb.prelu_grad_bf16_bits(zn, ga_bits, gb_bits, sn)), nhwc(pb.prelu_grad_bf16_bits(zn, ga_bits, None, sn))
    out, ds = backward(capi, cuda, c, zb, ga_bits, gb_bits, slope, want=True)
    assert pb.same_bf16(out, want2).all(), "out: %d elements differ" % int((~pb.same_bf16(out, want2)).sum())
    again, ds_again = backward(capi, cuda, c, zb, ga_bits, gb_bits, slope, want=True)
    assert np.array_equal(out, again) and np.array_equal(ds, ds_again), "two runs on the same inputs gave different bits"
    out3, _ = backward(capi, cuda, c, zb, ga_bits, gb_bits, slope, want=False)
    assert np.array_equal(out3, out), "out without dslope"
    # one consumer: where z > 0 out is ga rounded - a NaN of ga's sign, -0 as -0
    one, ds1 = backward(capi, cuda, c, zb, ga_bits, None, slope, want=True)
    assert pb.same_bf16(one, want1).all(), "out with gb = NULL"
    travels = nhwc((zn > 0) & pb.is_nan32(ga_bits))
    assert ((one[travels] >> 15) == (nhwc(ga_bits)[travels] >> 31)).all(), "a NaN that only travels keeps its sign"
    # gb = zeros is gb = NULL but for ga's -0 (ga + (+0) = +0) and the bits of a NaN
    zeros, _ = backward(capi, cuda, c, zb, ga_bits, np.zeros_like(ga_bits), slope, want=False)
    assert pb.same_bf16(zeros, nhwc(pb.prelu_grad_bf16_bits(zn, ga_bits, np.zeros_like(ga_bits), sn))).all()
    plain = ~nhwc((ga_bits == 0x80000000) | pb.is_nan32(ga_bits))
    assert np.array_equal(zeros[plain], one[plain])
    # the slope gradients against float64: the specials sit where z > 0 and enter no term
    p = c.n * c.h * c.w
    for name, got, gbb in (("two", ds, gb_bits), ("one", ds1, None)):
        g = torch.from_numpy(pb.sum_bits(ga_bits, gbb).view(np.float32).copy())
        g = torch.where(z > 0, torch.zeros(()), g)
        _, da64, s = pb.grad64(z, g, None, slope)
        err, bound = np.abs(f64(got) - da64.numpy()), cb.gamma(p + 1) * s.numpy()
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print("prelu_grad_bf16 %s (%s): worst dslope err / bound %.4g" % (pb.case_id(c), name, ratio))
        _worst["%s %s" % (pb.case_id(c), name)] = {"p": p, "dslope_err_over_bound": ratio}
        cd.note("prelu_grad_bf16_bounds.json", _worst)
        assert np.isfinite(f64(got)).all() and (err <= bound).all(), "dslope (%s): worst err / bound %g" % (name, ratio)


@pytest.mark.parametrize("c", [pb.CASES[i] for i in (2, 8, 12)], ids=pb.case_id)
def test_a_base_off_the_8_byte_alignment_takes_the_element_path_with_the_same_bits(capi, cuda, c):
    assert pb.is_vector(c)
    z, ga_bits, gb_bits, slope = pb.random_operands(c, seed=2)
    zb = z.numpy().view(np.uint32)
    assert np.array_equal(forward(capi, cuda, c, zb, slope), forward(capi, cuda, c, zb, slope, shift=1))
    out, _ = backward(capi, cuda, c, zb, ga_bits, gb_bits, slope, want=True)
    moved, _ = backward(capi, cuda, c, zb, ga_bits, gb_bits, slope, want=True, shift=1)
    assert np.array_equal(out, moved)


def test_nan_z_stores_nan_and_takes_the_slope_path(capi, cuda):
    c = pb.CASES[2]
    z, ga_bits, gb_bits, slope = pb.random_operands(c, seed=1)
    z[0, 3, 1, 1] = float("nan")
    z[1, 3, 0, 2] = float("nan")
    ga_bits[0, 3, 1, 1] = ga_bits[1, 3, 0, 2] = 0x3FC00000          # finite gradients there: slope * g, and NaN * g in the sum
    gb_bits[0, 3, 1, 1] = gb_bits[1, 3, 0, 2] = 0x3F000000
    zn = z.numpy()
    out, ds = backward(capi, cuda, c, zn.view(np.uint32), ga_bits, gb_bits, slope, want=True)
    want = nhwc(pb.prelu_grad_bf16_bits(zn, ga_bits, gb_bits, slope.numpy()))
    assert pb.same_bf16(out, want).all() and not pb.is_nan16(out[0, 1, 1, 3]) and not pb.is_nan16(out[1, 0, 2, 3])
    d = ds.view(np.float32)
    assert np.isnan(d[3]) and np.isfinite(np.delete(d, 3)).all()
    y = forward(capi, cuda, c, zn.view(np.uint32), slope)
    assert pb.is_nan16(y[0, 1, 1, 3]) and pb.is_nan16(y[1, 0, 2, 3]) and pb.is_nan16(y).sum() == 2


# ---- 3. the forward over every upper half of z ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["units of 4", "element by element"])
def test_forward_over_every_upper_half(capi, cuda, shift):
    """all 65,536 upper halves of z times the lower halves 0x0000, 0x7FFF, 0x8000 and 0x8001 under slopes of both signs: every
    rounding case, both zeros, subnormals, both Infs and every NaN class, through the 8-byte store and the 2-byte one"""
    z_bits, slope = pb.sweep_operands()
    c = pb.Case(4, 1, 512, 512, (4, 0), (4, 0), (4, 0), (4, 0), "")
    y = forward(capi, cuda, c, z_bits, slope, shift)
    want = nhwc(pb.prelu_bf16_bits(z_bits.view(np.float32), slope.numpy()))
    same = pb.same_bf16(y, want)
    assert same.all(), "%d of %d differ; first z bits %s" % (int((~same).sum()), same.size,
                                                              [hex(v) for v in nhwc(z_bits)[~same][:6].tolist()])
    nan = nhwc(pb.is_nan32(z_bits))
    assert pb.is_nan16(y[nan]).all() and not pb.is_nan16(y[~nan]).any()
    inf = nhwc((z_bits & 0x7FFFFFFF) == 0x7F800000)
    assert ((y[inf] & 0x7FFF) == 0x7F80).all()


# ---- 4. split equals fused -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [pb.CASES[i] for i in (1, 2, 4, 5, 6, 7, 8, 13)], ids=pb.case_id)
@pytest.mark.parametrize("operands", ["exact", "random"])
def test_split_equals_fused(capi, cuda, c, operands):
    """rtpose_prelu_grad_bf16 against rtpose_prelu_grad on torch's fp32 ga + gb followed by rtpose_layout_f32_to_bf16: out
    bit for bit, NaNs included; dslope bit for bit where both launches take the 4-channel units"""
    lib = capi.lib
    if operands == "exact":
        z, ga, gb, slope = pb.exact_mixed(c, seed=3)
        zb, ab, bb = (t.numpy().view(np.uint32) for t in (z, ga, gb))
    else:
        z, ab, bb, slope = pb.random_operands(c, seed=3)
        zb = z.numpy().view(np.uint32)
    out, ds = backward(capi, cuda, c, zb, ab, bb, slope, want=True)
    # the per-conv path: autograd's sum, the fp32 PReLU gradient in place, its one rounding
    pc = pb.as_prelu_case(c)
    lz, lg, _ = pr.layouts(pc)
    g = torch.from_numpy(ab.view(np.float32).copy()).to(cuda) + torch.from_numpy(bb.view(np.float32).copy()).to(cuda)
    zbuf = dev32(sent32(capi, lz, c, zb), cuda)
    gbuf = dev32(sent32(capi, lg, c, cd.np_bits(g)), cuda)
    sl = slope.to(cuda)
    floats = lib.rtpose_prelu_grad_workspace_floats(c.channels, c.n, c.h, c.w)
    ws, ds2 = torch.empty(floats, device=cuda), torch.empty(c.channels, device=cuda)
    capi.check(lib.rtpose_prelu_grad(capi.ptr(zbuf), C.byref(cd.L(capi, lz)), capi.ptr(sl), capi.ptr(gbuf), C.byref(cd.L(capi, lg)),
                                     capi.ptr(gbuf), C.byref(cd.L(capi, lg)), capi.ptr(ds2), capi.ptr(ws), floats, c.channels,
                                     c.n, c.h, c.w, capi.current_stream()), "rtpose_prelu_grad")
    cp = (c.channels + 7) // 8 * 8
    l16 = lr.dense(cp, c.h, c.w)
    h = torch.zeros(cd.npx(capi, l16, c.n, c.h, c.w) * cp, dtype=torch.bfloat16, device=cuda)
    capi.check(lib.rtpose_layout_f32_to_bf16(capi.ptr(gbuf), C.byref(cd.L(capi, lg)), capi.ptr(h), C.byref(cd.L(capi, l16)),
                                             c.channels, cp, c.n, c.h, c.w, capi.current_stream()), "rtpose_layout_f32_to_bf16")
    torch.cuda.synchronize()
    want = cd.np_bits(h)[lr.index(l16, c.n, c.h, c.w, c.channels)]
    differ = out != want
    assert not differ.any(), "%d of %d elements differ" % (int(differ.sum()), out.size)
    if operands == "random" and out.size >= 500:
        assert pb.is_nan16(out).any() and ((out & 0x7FFF) == 0x7F80).any() and (out == 0x8000).any()
    if pb.is_vector(c):
        assert c.z[0] % 4 == 0 and c.z[1] % 4 == 0          # the fused launch took the 4-channel units as well
        assert np.array_equal(ds, cd.np_bits(ds2)), "dslope"
    else:
        np.testing.assert_allclose(f64(ds), f64(cd.np_bits(ds2)), rtol=1e-4, atol=1e-5)


# ---- 5. refusals, with device memory behind every pointer -----------------------------------------------------------------------------
def _device_args(dev):
    """one device allocation per pointer of host.grad_args, each large enough for its slice"""
    bufs = [torch.zeros(1 << 14, dtype=torch.float32, device=dev) for _ in range(7)]
    bufs[4].view(torch.int32).fill_((SENT16 << 16) | SENT16)
    return bufs, tuple(b.data_ptr() for b in bufs)


@pytest.mark.parametrize("name,fault,text", host.GRAD_FAULTS, ids=[f[0] for f in host.GRAD_FAULTS])
def test_prelu_grad_bf16_refusals_launch_nothing(capi, cuda, name, fault, text):
    bufs, ptrs = _device_args(cuda)
    lays, a = host.grad_args(capi, ptrs)
    fault(a, lays)
    host.refused(capi, capi.lib.rtpose_prelu_grad_bf16, "prelu_grad_bf16", a, text)
    torch.cuda.synchronize()
    assert (cd.np_bits(bufs[4]) == ((SENT16 << 16) | SENT16)).all() and not bufs[5].any() and not bufs[6].any()


@pytest.mark.parametrize("name,fault,text", host.FWD_FAULTS, ids=[f[0] for f in host.FWD_FAULTS])
def test_prelu_bf16_refusals_launch_nothing(capi, cuda, name, fault, text):
    bufs, ptrs = _device_args(cuda)
    lays, a = host.fwd_args(capi, (ptrs[0], ptrs[1], ptrs[4]))
    fault(a, lays)
    host.refused(capi, capi.lib.rtpose_prelu_bf16, "prelu_bf16", a, text)
    torch.cuda.synchronize()
    assert (cd.np_bits(bufs[4]) == ((SENT16 << 16) | SENT16)).all()


def test_valid_arguments_of_the_refusal_tests_launch(capi, cuda):
    """the arguments every refusal above starts from are accepted: what was refused was the fault"""
    bufs, ptrs = _device_args(cuda)
    lays, a = host.grad_args(capi, ptrs)
    capi.check(capi.lib.rtpose_prelu_grad_bf16(*a), "rtpose_prelu_grad_bf16")
    lays, a = host.fwd_args(capi, (ptrs[0], ptrs[1], ptrs[4]))
    capi.check(capi.lib.rtpose_prelu_bf16(*a), "rtpose_prelu_bf16")
    torch.cuda.synchronize()
