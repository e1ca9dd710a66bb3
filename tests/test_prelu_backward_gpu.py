"""GPU suite of the PReLU passes of training (header section 2b continued, csrc/prelu_backward.hip): rtpose_prelu and
rtpose_prelu_grad on slices of wider buffers whose other channels and gaps hold conv_driver.SENTINEL NaNs - after every launch
they are intact, bit for bit - against tests/prelu_restate.py (float64 from F.prelu's CPU autograd; fp32 bits from a select or
one numpy multiply).

The exact tests need no bound: with the operand sets of prelu_restate (integers and quarter slopes, S < 2^24 - held to that by
tests/test_prelu_backward_cpu.py) fp32 arithmetic in any order is exact and the float64 reference is compared with ==.  On
random operands y and out are compared bit for bit, and the slope gradient, an fp32 sum of P = N H W products in an order
of the kernel's own, within gamma(P + 1) * S of the float64 sum, S the sum of |z gy| over its terms (conv_backward_restate.gamma).
The worst err / bound goes through conv_driver.note (profiles/r22_openpose_train.txt).

test_split_equals_fused is what lets the training forward claim the inference kernels' bits: rtpose_conv2d with the PReLU in
its epilogue against rtpose_conv2d without an activation followed by rtpose_prelu."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_backward_restate as cb
import conv_driver as cd
import layout_restate as lr
import prelu_restate as pr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel floats on either side of an output


def sent_buffer(capi, lay, c, bits=None):
    """A layout buffer on the host, as uint32: SENTINEL everywhere, `bits` [n, ch, h, w] at the valid pixels of the slice."""
    a = np.full(cd.npx(capi, lay, c.n, c.h, c.w) * lay.cstride, cd.SENTINEL, dtype=np.uint32)
    return a if bits is None else lr.scatter(a, lay, bits)


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32).copy()).to(dev).view(torch.float32)


def guarded(numel, dev):
    whole = torch.full((numel + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + numel].view(torch.float32)


def guards_intact(whole, numel):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + numel:] == cd.SENTINEL).all())


def nhwc(a):
    return np.transpose(a, (0, 2, 3, 1))


def forward(capi, dev, c, z_bits, slope, inplace):
    """rtpose_prelu of the case's z slice into the `out` layout (inplace: onto z itself): y's bits, NHWC"""
    lz, _, lout = pr.layouts(c)
    zh = sent_buffer(capi, lz, c, z_bits)
    zbuf = to_dev(zh, dev)
    ly = lz if inplace else lout
    ybuf = zbuf if inplace else to_dev(sent_buffer(capi, ly, c), dev)
    sl = slope.to(dev)
    capi.check(capi.lib.rtpose_prelu(capi.ptr(zbuf), C.byref(cd.L(capi, lz)), capi.ptr(sl), capi.ptr(ybuf), C.byref(cd.L(capi, ly)),
                                     c.channels, c.n, c.h, c.w, capi.current_stream()), "rtpose_prelu")
    torch.cuda.synchronize()
    bits, iy = cd.np_bits(ybuf), lr.index(ly, c.n, c.h, c.w, c.channels)
    assert lr.untouched(bits, iy, cd.SENTINEL), "prelu wrote outside the valid pixels of the slice"
    if not inplace:
        assert np.array_equal(cd.np_bits(zbuf), zh), "z was modified"
    return bits[iy]


def backward(capi, dev, c, z_bits, gy_bits, slope, alias, want):
    """rtpose_prelu_grad of the case: (out's bits NHWC, dslope's bits or None).  alias: out names gy's slice; want: with the
    slope gradient (else dslope and workspace are NULL)."""
    lib = capi.lib
    lz, lgy, lout = pr.layouts(c)
    if alias:
        lout = lgy
    zh, gh = sent_buffer(capi, lz, c, z_bits), sent_buffer(capi, lgy, c, gy_bits)
    zbuf, gbuf = to_dev(zh, dev), to_dev(gh, dev)
    obuf = gbuf if alias else to_dev(sent_buffer(capi, lout, c), dev)
    sl = slope.to(dev)
    floats = lib.rtpose_prelu_grad_workspace_floats(c.channels, c.n, c.h, c.w)
    assert floats >= lib.rtpose_prelu_grad_slabs(c.channels, c.n, c.h, c.w) * c.channels > 0
    d_whole, ds = guarded(c.channels, dev)
    w_whole, ws = guarded(floats, dev)
    capi.check(lib.rtpose_prelu_grad(capi.ptr(zbuf), C.byref(cd.L(capi, lz)), capi.ptr(sl), capi.ptr(gbuf), C.byref(cd.L(capi, lgy)),
                                     capi.ptr(obuf), C.byref(cd.L(capi, lout)), capi.ptr(ds) if want else None,
                                     capi.ptr(ws) if want else None, floats if want else 0, c.channels, c.n, c.h, c.w,
                                     capi.current_stream()), "rtpose_prelu_grad")
    torch.cuda.synchronize()
    bits, io = cd.np_bits(obuf), lr.index(lout, c.n, c.h, c.w, c.channels)
    assert np.array_equal(cd.np_bits(zbuf), zh), "z was modified"
    if alias:
        expect = gh.copy()
        expect[io] = bits[io]
        assert np.array_equal(bits, expect), "aliased: something besides the valid pixels of the slice changed"
    else:
        assert lr.untouched(bits, io, cd.SENTINEL), "written outside the valid pixels of the slice"
        assert np.array_equal(cd.np_bits(gbuf), gh), "gy was modified"
    assert guards_intact(d_whole, c.channels) and guards_intact(w_whole, floats), "written outside dslope / the workspace"
    if not want:
        assert (cd.np_bits(ds) == cd.SENTINEL).all() and (cd.np_bits(ws) == cd.SENTINEL).all(), "dslope = NULL but written"
    return bits[io], cd.np_bits(ds).copy() if want else None


def f64(bits):
    return bits.view(np.float32).astype(np.float64)


# ---- 1. exact sets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pr.CASES, ids=pr.case_id)
def test_exact_sets_bit_for_bit(capi, cuda, c):
    """y, out and dslope equal the float64 restatement with ==, out separate and aliased, dslope given and NULL"""
    slabs = capi.lib.rtpose_prelu_grad_slabs(c.channels, c.n, c.h, c.w)
    assert ("several slabs" in c.tags) == (slabs >= 2)
    for i, (kind, make) in enumerate(sorted(pr.EXACT_SETS.items())):
        z, gy, slope = make(c)
        assert pr.exact_margin(z, gy) < 2 ** 24
        y64, dz64, da64, _ = pr.prelu64(z, gy, slope)
        zb, gb = z.numpy().view(np.uint32), gy.numpy().view(np.uint32)
        y = forward(capi, cuda, c, zb, slope, inplace=bool(i))
        assert np.array_equal(f64(y), nhwc(y64.numpy())), (kind, "y")
        assert np.array_equal(y, nhwc(pr.prelu_bits(z.numpy(), slope.numpy()))), (kind, "y bits: the sign of a zero is z's")
        for alias in (False, True):
            out, ds = backward(capi, cuda, c, zb, gb, slope, alias, want=True)
            wrong = int((f64(out) != nhwc(dz64.numpy())).sum())
            assert wrong == 0, "%s out (aliased %s): %d of %d elements differ" % (kind, alias, wrong, out.size)
            bad = np.flatnonzero(f64(ds) != da64.numpy())
            assert bad.size == 0, "%s dslope (aliased %s): channels %s differ" % (kind, alias, bad[:8].tolist())
        out, ds = backward(capi, cuda, c, zb, gb, slope, alias=bool(i), want=False)
        assert ds is None and np.array_equal(f64(out), nhwc(dz64.numpy())), (kind, "out without dslope")


# ---- 2. + 3. random operands and repeatability ------------------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize("c", pr.CASES, ids=pr.case_id)
def test_random_operands(capi, cuda, c):
    z, gy_bits, slope = pr.random_operands(c)
    if c.channels >= 2:
        assert (slope < 0).any() and (slope > 0).any()
    zn = z.numpy()
    if zn.size >= 64:
        assert (zn == 0).any() and np.signbit(zn[zn == 0]).any() and (gy_bits == 0x7FC00777).any()
    zb = zn.view(np.uint32)
    for inplace in (False, True):
        y = forward(capi, cuda, c, zb, slope, inplace)
        assert np.array_equal(y, nhwc(pr.prelu_bits(zn, slope.numpy()))), "y (in place %s)" % inplace
    want_out = nhwc(pr.prelu_grad_bits(zn, gy_bits, slope.numpy()))
    out, ds = backward(capi, cuda, c, zb, gy_bits, slope, alias=False, want=True)
    assert np.array_equal(out, want_out), "out"
    out2, ds2 = backward(capi, cuda, c, zb, gy_bits, slope, alias=True, want=True)
    assert np.array_equal(out2, want_out), "out aliasing gy"
    assert np.array_equal(ds, ds2), "two runs on the same inputs gave different dslope bits"
    out3, _ = backward(capi, cuda, c, zb, gy_bits, slope, alias=False, want=False)
    assert np.array_equal(out3, want_out), "out without dslope"
    # the slope gradient against float64: the NaN and -0 gradients sit where z > 0 and enter no term
    gy = torch.from_numpy(gy_bits.view(np.float32).copy())
    gy = torch.where(z > 0, torch.zeros(()), gy)
    _, _, da64, s = pr.prelu64(z, gy, slope)
    p = c.n * c.h * c.w
    err, bound = np.abs(f64(ds) - da64.numpy()), cb.gamma(p + 1) * s.numpy()
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("prelu_grad %s: slabs %d, worst dslope err / bound %.4g" % (pr.case_id(c), capi.lib.rtpose_prelu_grad_slabs(
        c.channels, c.n, c.h, c.w), ratio))
    _worst[pr.case_id(c)] = {"p": p, "dslope_err_over_bound": ratio}
    cd.note("prelu_grad_bounds.json", _worst)
    assert np.isfinite(f64(ds)).all() and (err <= bound).all(), "dslope: worst err / bound %g" % ratio


def test_nan_z_takes_the_slope_path(capi, cuda):
    c = pr.CASES[2]
    z, gy_bits, slope = pr.random_operands(c, seed=1)
    z[0, 3, 1, 1] = float("nan")
    z[1, 3, 0, 2] = float("nan")
    gy_bits[0, 3, 1, 1] = gy_bits[1, 3, 0, 2] = 0x3FC00000          # finite gradients there: slope * 1.5, and NaN * 1.5 in the sum
    out, ds = backward(capi, cuda, c, z.numpy().view(np.uint32), gy_bits, slope, alias=False, want=True)
    assert np.array_equal(out, nhwc(pr.prelu_grad_bits(z.numpy(), gy_bits, slope.numpy())))
    d = ds.view(np.float32)
    assert np.isnan(d[3]) and np.isfinite(np.delete(d, 3)).all()
    y = forward(capi, cuda, c, z.numpy().view(np.uint32), slope, inplace=False)
    assert np.isnan(y.view(np.float32)[0, 1, 1, 3]) and np.isnan(y.view(np.float32)[1, 0, 2, 3])


# ---- 4. split equals fused -----------------------------------------------------------------------------------------------------------
Conv = cb.Case          # k cin cout n h w x_cs x_off note: only the shape fields are used here


@pytest.mark.parametrize("policy", [cd.sentinel(4, 8), cd.sentinel(1, 3)], ids=["aligned", "odd"])
@pytest.mark.parametrize("operands", ["exact", "random"])
@pytest.mark.parametrize("k,cin,cout,n,h,w", [(k,) + s for k in (1, 3) for s in ((9, 8, 2, 5, 3), (24, 96, 2, 9, 7))])
def test_split_equals_fused(capi, cuda, k, cin, cout, n, h, w, operands, policy):
    """rtpose_conv2d with d.prelu = slope against rtpose_conv2d (prelu = NULL, relu = 0) followed by rtpose_prelu on its
    output slice, in place: the same accumulation and a single-rounding epilogue, so the same values"""
    form = cd.Form("f32", k)
    if operands == "exact":
        x, _, wt, b = cb.exact_tensors(Conv(k, cin, cout, n, h, w, 0, 0, ""))
        fused = cd.given(form, [x], [wt], [b], slopes=[pr.slopes(cout)])
        fused.refs = [cd.reference(form, x, wt, b, 0, 0, pr.slopes(cout))]
    else:
        fused = cd.problem(form, n, h, w, cin, cout, relu=0, prelu=1, seed=7 * k + cout)
        assert (fused.slopes[0] < 0).any() and (fused.slopes[0] > 0).any()
    split = cd.given(form, fused.xs, fused.wts, fused.biases)
    buf, lay = cd.to_layout(capi, cuda, fused, fused.xs[0], k // 2)
    obuf, louts = cd.launch(capi, cuda, fused, [(buf, lay)], policy, 1)
    want = cd.outputs(fused, obuf, louts, policy)[0]
    zbuf, lz = cd.launch(capi, cuda, split, [(buf, lay)], policy, 1)
    z = cd.outputs(split, zbuf, lz, policy)[0]
    sl = fused.slopes[0].to(cuda)
    capi.check(capi.lib.rtpose_prelu(capi.ptr(zbuf), C.byref(cd.L(capi, lz[0])), capi.ptr(sl), capi.ptr(zbuf),
                                     C.byref(cd.L(capi, lz[0])), cout, n, h, w, capi.current_stream()), "rtpose_prelu")
    torch.cuda.synchronize()
    got = cd.outputs(split, zbuf, lz, policy)[0]
    assert (z < 0).any() and (z > 0).any() and not torch.equal(got, z)
    assert torch.equal(got, want), "%d of %d elements differ" % (int((got != want).sum()), want.numel())
    if operands == "exact":
        assert torch.equal(got.double(), fused.refs[0])
    else:
        cd.check(fused, 0, got, fused.xs[0])
