"""The kernel instances of csrc/conv_wino7.hip and csrc/conv_wino4.hip that no other conv test launches, on the GPU: the
smallest geometries that select them (tests/wino_cases.py: REACH7, REACH4; tests/test_wino_reach_cpu.py shows that with them
every instance the launchers can select is launched).  A case first asks tests/wino_reach.py for its launch on THIS device's
CU count and fails if that is not its tag - a geometry that slid onto another instance tests nothing new - then checks

  - every branch against a float64 direct conv within the form's existing tolerance (cd.check: cd.TOL, or gamma_limit_f87),
  - the first and the last image run alone (another strip composition; for F(6,7) and F(4x4,3x3) the small-grid form):
    the same bits,
  - a persistent launch against the same launch without a scratch (one block per tile): the same bits,
  - a second launch: the same bits (hand-over flags back at zero),
  - the device error word of every launch with a scratch is 0 (cd.call), and every word of the output buffer outside the
    branches' slices still holds the sentinel (cd.outputs).
"""
import pytest
import torch

import conv_driver as cd
import wino_cases as wc
import wino_reach as wr

pytestmark = pytest.mark.gpu

_WORST = {}


def _cus(cuda):
    n = torch.cuda.get_device_properties(cuda).multi_processor_count
    if n != wr.CUS:
        pytest.skip("the case tags are written for the %d CUs of an MI355X; this device reports %d" % (wr.CUS, n))
    return n


def _run(capi, cuda, form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, pad_in, scratch=True, ref=True, images=None):
    first, count = images or (0, None)
    P = cd.problem(form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, only_images=count, first_image=first,
                   ref=torch.float64 if ref else None)
    # 16-byte aligned slices (the layout the network uses) for even batches, odd stride and offsets (scalar stores) for odd ones
    out = cd.sentinel(8, 16) if n % 2 == 0 else cd.sentinel(1, 3)
    return P, cd.run(capi, cuda, P, out, pad_in, 1, scratch)


def _case(capi, cuda, name, form, n, h, w, cin, cout, relu, pool, prelu, groups, pad_in, persistent):
    seed = 7000 + 131 * n + 17 * h + w + cout
    P, outs = _run(capi, cuda, form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, pad_in)
    worst = 0.0
    for gi in range(groups):
        ref = P.refs[gi]
        worst = max(worst, (outs[gi].double() - ref).abs().max().item() / max(1.0, ref.abs().max().item()))
    _WORST[name] = float("%.3g" % worst)
    print("%s: worst |err| / max(1, max|ref|) = %.3g" % (name, worst))
    cd.note("wino_reach.json", {"unit": "max |err| / max(1, max|ref|) against float64, worst branch", "worst": _WORST})
    for gi in range(groups):
        cd.check(P, gi, outs[gi], P.xs[0])
    for first in sorted({0, n - 1}):
        _, one = _run(capi, cuda, form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, pad_in, ref=False, images=(first, 1))
        for a, b in zip(outs, one):
            assert torch.equal(a[first:first + 1], b), "image %d alone gives other bits" % first
    if persistent:
        _, plain = _run(capi, cuda, form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, pad_in, scratch=False, ref=False)
        for a, b in zip(outs, plain):
            assert torch.equal(a, b), "persistent blocks and one block per tile give different bits"
    _, again = _run(capi, cuda, form, n, h, w, cin, cout, relu, pool, prelu, groups, seed, pad_in, ref=False)
    for a, b in zip(outs, again):
        assert torch.equal(a, b), "a second launch gives other bits"


@pytest.mark.parametrize("tag,row", wc.REACH7, ids=["F%d-%dx%dx%d-%dx%d" % r for _, r in wc.REACH7])
def test_7x7_instance(capi, cuda, tag, row):
    m, n, h, w, cout, groups = row
    cus = _cus(cuda)
    cin, pad_in = wc.REACH7_CIN, wc.REACH7_PAD
    r = wr.reach7(n, h, w, cin, cout, groups, h + pad_in, m, cus, True)
    assert wr.tag7(r) == tag, "this geometry selects %s here" % wr.tag7(r)
    if n > 1 and not r.kernel.startswith("wino7s"):     # one image alone is another launch: the composition of its strips differs
        one = wr.reach7(1, h, w, cin, cout, groups, h + pad_in, m, cus, True)
        assert (one.kernel, one.plan.mtiles) != (r.kernel, r.plan.mtiles) and (m != 6 or one.kernel.startswith("wino7s"))
    _case(capi, cuda, "F(%d,7) %d x %d x %d -> %d x %d: %s" % (m, n, h, w, cout, groups, tag), cd.Form("f32", 7, m),
          n, h, w, cin, cout, 1, 0, 0, groups, pad_in, r.persistent)


@pytest.mark.parametrize("tag,row", wc.REACH4, ids=["%dx%dx%d-%dx%d-%d%d" % r for _, r in wc.REACH4])
def test_4x4_launch_shape(capi, cuda, tag, row):
    n, h, w, cout, groups, pool, prelu = row
    cus = _cus(cuda)
    cin, pad_in = wc.REACH4_CIN, wc.REACH4_PAD
    r = wr.reach4(n, h, w, cin, cout, groups, cus, prelu)
    assert wr.tag4(r, prelu, pool) == tag, "this geometry selects %s here" % wr.tag4(r, prelu, pool)
    assert wr.reach4(1, h, w, cin, cout, groups, cus, prelu).shape == "small"      # an image alone: the 16 x 16 form
    _case(capi, cuda, "F(4x4,3x3) %d x %d x %d -> %d x %d: %s" % (n, h, w, cout, groups, tag), cd.Form("f32", 3, 4),
          n, h, w, cin, cout, 0 if prelu else 1, pool, prelu, groups, pad_in, False)
