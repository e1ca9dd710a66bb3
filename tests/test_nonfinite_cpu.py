"""The conditions of tests/nonfinite_cases.py, on the CPU: every case's expected output holds each injected class and finite
elements (so neither the propagation nor the containment check of tests/test_nonfinite_gpu.py is vacuous), the comparison
rejects the wrong answers that matter, torch's float64 references agree with tap-by-tap numpy sums in class and value on
the families' operands, and the shapes reach the code paths their tags name."""
import numpy as np
import pytest
import torch

import bn_restate as br
import conv_backward_bf16_restate as cbb
import conv_driver as cd
import conv_forward_exact as fx
import dwconv_restate as dr
import nonfinite_cases as nf


def _ids(cases):
    return dict(argvalues=cases, ids=[c.tag for c in cases])


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def _want():
    c = nf.CONV_F32[0]._replace(k=3, relu=0)
    return nf.conv_reference(c, *nf.conv_operands(c))


def test_checker_accepts_the_reference_and_signed_zeros():
    want = _want()
    assert nf.holds_every_class(want, (nf.NAN, nf.POS, nf.NEG))
    assert nf.differences(want.astype(np.float32), want) == []
    assert nf.differences(np.zeros(4, np.float32), -np.zeros(4)) == []            # torch's relu(-0.) is -0., the kernels' +0
    assert nf.differences(np.float32(np.nan), np.float64(np.nan)) == [] and nf.differences(np.float32(3), np.float64(np.inf))


@pytest.mark.parametrize("mutant", ["nan->-3.0e38", "nan->0", "inf swapped", "inf->nan", "sentinel for nan", "bf16 sentinel for nan",
                                    "finite off by one", "finite->nan"])
def test_checker_rejects(mutant):
    want = _want()
    cls = nf.classes(want)
    got = want.astype(np.float32)
    if mutant == "nan->-3.0e38":
        got[cls == nf.NAN] = -3.0e38
    elif mutant == "nan->0":
        got[cls == nf.NAN] = 0.0
    elif mutant == "inf swapped":
        got[cls == nf.POS], got[cls == nf.NEG] = -np.inf, np.inf
    elif mutant == "inf->nan":
        got[cls == nf.POS] = np.nan
    elif mutant == "sentinel for nan":
        got.view(np.uint32)[tuple(np.argwhere(cls == nf.NAN)[0])] = cd.SENTINEL
    elif mutant == "bf16 sentinel for nan":
        got.view(np.uint32)[tuple(np.argwhere(cls == nf.NAN)[0])] = 0x7FC1 << 16
    elif mutant == "finite off by one":
        got[tuple(np.argwhere(cls == nf.FINITE)[-1])] += 1.0
    else:
        got[tuple(np.argwhere(cls == nf.FINITE)[0])] = np.nan
    assert nf.differences(got, want), mutant
    with pytest.raises(AssertionError):
        nf.same_class_and_values(got, want, mutant)


def test_injected_patterns_are_no_sentinels():
    for b in nf.NAN_BITS + nf.NAN_INPUTS:
        assert np.isnan(nf.f32_of(b)) and b not in nf.SENTINELS and (b >> 16) != 0x7FC1
    assert np.isposinf(nf.f32_of(nf.PINF)) and np.isneginf(nf.f32_of(nf.NINF))
    used = {bits for c in nf.CONV_F32 + nf.CONV_BF16 + nf.WGRAD for _, bits in c.inj}
    assert set(nf.NAN_BITS) <= used, "both NaN patterns are in use"


# ---- the forward convs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_ids(nf.CONV_F32 + nf.CONV_BF16))
def test_conv_case_holds_every_class_and_torch_equals_the_tap_sum(c):
    x, wt, b = nf.conv_operands(c)
    assert (x != 0).all() and (c.zero is not None or (wt != 0).all())
    assert len(c.inj) in (0, 3) and torch.isfinite(x).sum().item() == x.numel() - len(c.inj)
    pre = nf.conv_reference(c._replace(out_f32=True), x, wt, b, relu=False)
    taps = nf.conv_taps(x, wt, b)
    assert nf.differences(pre.astype(np.float32), taps) == [], "torch's float64 conv2d against the tap-by-tap sum"
    assert c.zero is not None or np.abs(taps[np.isfinite(taps)]).max() < 2 ** 24
    want = nf.conv_reference(c, x, wt, b)
    if c.inj:
        assert nf.holds_every_class(pre, (nf.NAN, nf.POS, nf.NEG)) and nf.holds_every_class(want, nf.conv_injected_classes(c))
        if c.relu:
            assert not (nf.classes(want) == nf.NEG).any() and (want[np.isfinite(want)] == 0).any()
    else:
        ch, bias = c.zero
        assert np.isfinite(want).all() and (want[:, ch] == np.float32(bias)).all() and -3.4e38 < np.float32(bias) < -3.0e38
    f = want.astype(np.float32)
    assert np.array_equal(f.astype(np.float64)[np.isfinite(want)], want[np.isfinite(want)]), "every finite output is an fp32 value"


def _fx(c):
    return fx._c("conv2d" if c.kind == "f32" else "conv2d_bf16", c.tag, c.n, c.h, c.w, c.cin, c.cout, k=c.k, relu=c.relu,
                 kind=c.kind, out_f32=c.out_f32)


@pytest.mark.parametrize("c", **_ids(nf.CONV_F32 + nf.CONV_BF16))
def test_conv_case_reaches_the_path_its_tag_names(c):
    e, g = _fx(c), fx.geometry(_fx(c))
    if "strip" in c.tag or "tail" in c.tag or c.kind == "bf16" and "2d" not in c.tag:
        assert g.strip
    if "tiles2d" in c.tag or "2d" in c.tag.split("-"):
        assert not g.strip
    if "tail" in c.tag or "strip" in c.tag:
        assert g.M % 64 != 0, "a half-tile tail"
    if c.kind == "bf16":
        tr = fx.EDGES["transposed epilogue"](e, g) and c.aligned
        vec = not c.out_f32 and c.cout % fx.BN == 0 and c.aligned
        assert ("transposed" in c.tag or "c64" in c.tag) == tr and ("vec_store" in c.tag) == (vec and not tr)
        assert ("elementwise" in c.tag or "2d" in c.tag or c.zero is not None) == (not vec)
        assert ("c64" in c.tag) == (c.cin == 64 and c.k == 3 and vec)       # (the library's own predicate: the GPU test)


# ---- the weight gradients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_ids(nf.WGRAD))
def test_wgrad_case_holds_every_class_and_torch_equals_the_tap_sum(c):
    x, gy = nf.wgrad_operands(c)
    dw, db = nf.wgrad_taps(x, gy, c.k)
    tw, tb = nf.wgrad_torch(x, gy, c.k)
    assert nf.differences(tw.astype(np.float32), dw) == [] and nf.differences(tb.astype(np.float32), db) == []
    assert nf.holds_every_class(dw, (nf.NAN, nf.POS, nf.NEG))
    if c.into == "gy":
        p = c.k // 2
        for (n, o, yy, xx), bits in c.inj:
            if bits in (nf.PINF, nf.NINF):
                assert p <= yy < c.h - p and p <= xx < c.w - p, "an Inf of gy within k // 2 of a border"
        assert nf.holds_every_class(db, (nf.NAN,) if "overlap" in c.tag else (nf.NAN, nf.POS, nf.NEG))
        if "overlap" in c.tag:
            assert np.isnan(db[2]) and np.isnan(db[0])
    else:
        assert np.isfinite(db).all()
    assert cbb.geometry(c.cin, c.cout, c.k, c.n, c.h, c.w)[1] > 1, "one slab: the slab sum adds nothing"


def test_wgrad_slab_counts_by_the_library(capi):
    for c in nf.WGRAD:
        assert capi.lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w) > 1
        assert capi.lib.rtpose_conv2d_wgrad_bf16_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w) > 1


# ---- the per-channel kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", **_ids(nf.BN))
def test_bn_case_fills_its_channel_and_no_other(c):
    x0, gy0 = nf.chan_operands(c, nf.BN_SHAPE)
    x, gy = nf.chan_inject(c, x0, gy0, nf.BN_AT, nf.BN_AT)
    w, b, rm, rv = br.affine(c.channels, True)
    t0, t = br.bn64(x0, gy0, w, b, rm, rv), br.bn64(x, gy, w, b, rm, rv)
    others = [i for i in range(c.channels) if i != c.channel]
    for k in ("y", "dx", "dweight", "dbias", "running_mean", "running_var"):
        a0, a = t0[k].numpy(), t[k].numpy()
        sel = (slice(None), others) if a.ndim == 4 else (others,)
        assert np.array_equal(a0[sel], a[sel]), "the reference leaks into other channels: %s" % k
    own = (slice(None), c.channel)
    assert not np.isfinite(t["dx"].numpy()[own]).any() and not np.isfinite(t["dweight"].numpy()[c.channel])
    if c.into == "x":
        assert not np.isfinite(t["y"].numpy()[own]).any() and np.isnan(t["running_var"].numpy()[c.channel])
        assert np.isfinite(t["dbias"].numpy()[c.channel])
    assert nf.BN_AT != (0, 0, 0) and br.slab_geometry(*((nf.BN_SHAPE[0],) + nf.BN_SHAPE[1:]))[1] > 1


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", **_ids(nf.DW))
def test_dw_case_holds_its_class_in_its_channel_only(c, stride):
    n, h, w = nf.DW_SHAPE
    ho, wo = dr.out_size(h, w, stride)
    x0, gy0 = nf.chan_operands(c, nf.DW_SHAPE, (ho, wo))
    x, gy = nf.chan_inject(c, x0, gy0, nf.DW_AT_X, nf.DW_AT_GY)
    wt = nf.dw_weights(c.channels)
    (y0, dx0, dw0), (y, dx, dw) = dr.autograd64(x0, wt, gy0, stride), dr.autograd64(x, wt, gy, stride)
    others = [i for i in range(c.channels) if i != c.channel]
    for a0, a in ((y0, y), (dx0, dx)):
        assert torch.equal(a0[:, others], a[:, others])
    assert torch.equal(dw0[others], dw[others])
    cls = (nf.NAN,) if nf.chan_classes(c) == (nf.NAN,) else (nf.NAN, nf.POS, nf.NEG)
    touched = y[:, c.channel] if c.into == "x" else dx[:, c.channel]
    assert np.isin(nf.classes(touched.numpy()), cls + (nf.FINITE,)).all()
    assert any((nf.classes(touched.numpy()) == k).any() for k in cls) and torch.isfinite(touched).any()
    assert not torch.isfinite(dw[c.channel]).all()
    # an Inf of gy meets no padding zero of x: every tap of its pixel lies inside the map
    yy, xx = nf.DW_AT_GY[1:]
    assert 1 <= stride * yy <= h - 2 and 1 <= stride * xx and stride * (xx + 1) <= w - 2
    if stride == 1:
        assert dr.slab_geometry(n, h, w, stride)[1] > 1


# ---- the stems and the chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,k", [(64, 7), (24, 3)])
def test_stem_case_holds_every_class(cout, k):
    x, wt, gy = nf.stem_operands(cout, k)
    dw, db, dx = nf.stem_reference(x, wt, gy, k, k == 3)
    assert torch.isfinite(x).all() and nf.holds_every_class(dw, (nf.NAN, nf.POS, nf.NEG)) and nf.holds_every_class(db, (nf.NAN, nf.POS, nf.NEG))
    if dx is not None:
        assert nf.holds_every_class(dx, (nf.NAN, nf.POS, nf.NEG))


def test_chain_reference_is_exact_and_carries_the_nan_to_the_output():
    x, layers = nf.chain_operands()
    y = nf.chain_reference(x, layers)
    assert np.isfinite(y).all() and np.abs(y).max() < 2 ** 24 and np.array_equal(y, np.round(y))
    xn = nf.inject(x.clone(), [((1, 3, 2, 2), nf.NAN_BITS[0])])
    yn = nf.chain_reference(xn, layers)
    assert nf.holds_every_class(yn, (nf.NAN,)) and np.array_equal(yn[0], y[0])
    w1 = nf.inject(layers[1][0].clone(), [((4, 6, 3, 3), nf.NAN_BITS[1])])
    yw = nf.chain_reference(x, [layers[0], (w1, layers[1][1]), layers[2]])
    assert np.isnan(yw).all(), "a NaN filter of a hidden layer reaches every output"
