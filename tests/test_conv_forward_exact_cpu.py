"""The conditions under which tests/test_conv_forward_exact_gpu.py may compare the forward conv launchers with a float64
reference by ==, asserted per case from the reference side only (tests/conv_forward_exact.py; no GPU, no library call):
the edge tags (the shape reaches the tile edge it claims, from the constants stated in that file), S < 2^24, the share of
nonzero outputs and the clipped ones, negative pre-activations under PReLU, pool windows whose maximum is not the top-left
element, discrimination, the bf16x3 operand families, and the per-stage Winograd bounds."""
import numpy as np
import pytest
import torch

import conv_forward_exact as fx
import layout_restate as lr

ALL = [fx.sized(c, fx.CUS) for c in fx.all_cases()]
IDS = ["%s-%s" % (c.launcher, c.tag) for c in ALL]


def test_case_ids_are_unique_and_every_launcher_has_cases():
    assert len(set(IDS)) == len(IDS)
    assert all(len(v) >= 6 for v in fx.EXACT_CASES.values())
    assert all(c.launcher == name for name, cs in fx.EXACT_CASES.items() for c in cs)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_edge_tags(c):
    g = fx.geometry(c)
    assert c.edges, "a case says what it is there for"
    for e in c.edges:
        assert fx.EDGES[e](c, g), "%s does not reach the edge %r" % (c.tag, e)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_conditions_of_equality(c):
    o = fx.operands(c)
    r = fx.conditions(c, o)
    assert r.S < fx.LIMIT, "S = %g" % r.S
    for t in [o.x] + o.wts + o.biases:
        assert torch.equal(t, t.round()) and (t.numel() < 16 or ((t > 0).any() and (t < 0).any()))
    assert (o.x != 0).float().mean() >= 0.75
    if c.kind == "bf16":                    # every operand is a bf16 value
        for t in [o.x] + o.wts + getattr(o, "w2", []):
            assert np.array_equal(lr.bf16_to_f32(lr.bf16_rne(t.numpy())).reshape(t.shape), t.numpy())
    if r.outputs >= 64:
        assert r.share >= fx.MIN_SHARE, "only %.2f of the outputs are nonzero" % r.share
    if c.relu:
        assert r.clipped > 0, "the ReLU clips nothing"
    if c.prelu:
        assert r.negative > 0, "no negative pre-activation meets a PReLU slope"
        for sl in o.slopes:
            m, _ = np.frexp(np.abs(sl.numpy()))
            assert np.all(m == 0.5), "a slope is no power of two"
    if c.pool:
        assert r.pool_off_corner > 0, "every pool window has its maximum in the top-left corner"
    if c.x.get("preact"):
        assert torch.equal(o.in_scale, o.in_scale.round()) and torch.equal(o.in_shift, o.in_shift.round())
        want = {"neg": (True, False), "pos": (False, True), "both": (True, True)}[c.x["preact"]]
        assert ((o.in_scale < 0).any().item(), (o.in_scale > 0).any().item()) == want
        a = fx.staged_input(c, o, o.x)
        assert (a == 0).any() and (a > 0).any()
    if c.x.get("res"):
        assert torch.equal(o.res, o.res.round()) and (o.res != 0).any()
    if c.cmap:
        assert sorted(o.cmap.tolist()) == list(range(c.cout)) and o.cmap.tolist() != list(range(c.cout))


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_every_case_discriminates(c):
    """(the walk cases: the same draw at three images - the property is one of the operands, not of the batch)"""
    if c.walk is not None:
        c = c._replace(n=3)
    failed = fx.discriminates(c, fx.operands(c))
    assert not failed, failed


def test_the_sample_of_terms_covers_chunks_taps_and_borders():
    for c in ALL:
        terms = fx.sampled_terms(c)
        taps = fx.live_taps(c)
        chans = {t[1] for t in terms if t[0] == "w"}
        if "mid" in c.x:
            assert {t[1] for t in terms if t[0] == "w2"} == {0, c.x["mid"] - 1}     # the second conv's first and last chunk
        assert 0 in chans and c.cin - 1 in chans                       # first and last channel chunk
        assert {t[2] for t in terms if t[0] == "w"} == {taps[0], taps[-1]}
        px = {t[3] for t in terms if t[0] == "x"}
        assert (0, 0) in px and ((c.h - 1, c.w - 1) in px or (c.pool and c.k == 1)) and {t[1] for t in terms if t[0] == "x"} == {0, c.n - 1}
        if c.k > 1 and c.h >= c.k and c.w >= c.k:
            assert taps[0] == (0, 0) and taps[-1] == (c.k - 1, c.k - 1)


def test_every_bf16_launcher_has_outputs_that_need_the_rounding():
    """a bf16 output is exact below 256; the cases of every launcher that stores bf16 reach sums that round"""
    for name in ("conv_first_bf16", "pair_bf16", "conv2d_bf16", "c64"):
        rounded = sum(fx.conditions(c, fx.operands(c)).rounded for c in ALL if c.launcher == name)
        print(name, "outputs that are not their own bf16 rounding:", rounded)
        assert rounded >= 100


X3 = [c for c in ALL if c.kind == "x3" or (c.kind == "f32" and c.family != "int")]


@pytest.mark.parametrize("c", X3, ids=["%s-%s" % (c.launcher, c.tag) for c in X3])
def test_operand_families(c):
    """bf16x3: hi + lo is the operand exactly; 'xwide': every x has a low piece, no w has one; 'wwide' the other way round;
    'int': single-piece operands.  The product the kernel drops (lo * lo) is then identically zero.
    fp32 launchers, 'xwide' / 'wwide': the same draw - (nearly) every x resp. w is no bf16 value (a pre-activated case pins
    a few corner values to +-2)."""
    exact, x_lo, w_lo, dropped = fx.split_properties(c, fx.operands(c))
    assert exact and dropped == 0.0
    if c.kind == "x3":
        assert (x_lo, w_lo) == {"int": (0.0, 0.0), "xwide": (1.0, 0.0), "wwide": (0.0, 1.0)}[c.family]
    else:
        assert (x_lo >= 0.7, w_lo) == (True, 0.0) if c.family == "xwide" else (x_lo, w_lo) == (0.0, 1.0)


def test_winograd_forms_admitted_by_the_exact_tables():
    """F(2x2,3x3) passes every stage at the widest cin of its cases; F(4x4,3x3) and F(4,7) fail the channel sum at the
    smallest cin they take with ternary t; F(6,7)'s B^T is not dyadic (F(8,7) adds the points +-5/4 to it)."""
    cin = max(c.cin for c in fx.EXACT_CASES["wino2"])
    for x_max, t_max in ((fx.X_MAX, fx.W_MAX), (fx.WIDE_HI, fx.W_MAX), (fx.X_MAX, fx.WIDE_HI)):      # the three families
        c2, stages, dyadic = fx.wino_proof(*fx.WINO_FORMS["F(2x2,3x3)"][:4], cin, x_max=x_max, t_max=t_max)
        assert c2 == fx.WINO2_C == 1 and dyadic and all(ok for *_, ok in stages), stages
        print("F(2x2,3x3) at cin %d, |d| <= %d, |t| <= %d: %s" % (cin, x_max, t_max, stages))
    for name, c_want in (("F(4x4,3x3)", 3 ** 10), ("F(4,7)", 315)):
        m, r, pts, two_d, cin_min, rows = fx.WINO_FORMS[name]
        c, stages, dyadic = fx.wino_proof(m, r, pts, two_d, cin_min, rows, x_max=1, t_max=1)
        print("%s at cin %d, |d| <= 1, |t| <= 1: c = %d, %s" % (name, cin_min, c, stages))
        assert c == c_want and dyadic and stages[0][3] and not stages[1][3]
    assert fx.wino_proof(*fx.WINO_FORMS["F(6,7)"][:4], 8)[2] is False


def test_case_counts_and_figures():
    worst, share = (0.0, None), (1.0, None)
    for c in ALL:
        r = fx.conditions(c, fx.operands(c))
        worst = max(worst, (r.S, c.launcher + "-" + c.tag))
        if r.outputs >= 64:
            share = min(share, (r.share, c.launcher + "-" + c.tag))
    print("cases per launcher %s; %d in all" % ({k: len(v) for k, v in fx.EXACT_CASES.items()}, len(ALL)))
    print("largest S %d (%s) of %d; smallest nonzero share %.2f (%s)" % (worst[0], worst[1], fx.LIMIT, share[0], share[1]))
    assert worst[0] < fx.LIMIT and share[0] >= fx.MIN_SHARE
