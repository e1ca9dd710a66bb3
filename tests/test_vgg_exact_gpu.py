"""The rtpose_vgg plans (csrc/net.hip: add_trunk, build_plan) pinned as a whole, through network.get_model('vgg19') -
load_state_dict of the tracer operands of tests/vgg_exact.py, set_winograd, set_compute_dtype:

a. the four exact plans - fp32 direct, fp32 F(2x2,3x3), bf16, bf16x3 - give all 12 stage outputs == the float64 restatement
   cast to fp32, at every shape the dtype admits, on a fresh plan and again after a forward of other data (conditions, edge
   tags and mutations: tests/test_vgg_exact_cpu.py);
b. outputs 10 and 11 without the stage records (keep_intermediates = False) are the same bits;
c. the forms that are not exact - F(4x4,3x3), F(4,7), F(6,7), F(8,7) forced, and the default plan - land within
   1e-3 * max(1, max |integers|) of the integers, which is below half a unit (vgg_exact.conditions), and the outputs whose
   whole chain ran in exact forms are still ==;
d. an image's 12 outputs are the same bits in a batch of one;      e. A, B, A: operands and dtypes change on one module;
f. a NaN pixel of one image stays in that image.

What ran where in c (rtpose_net_conv_numerics, recorded on the MI355X): the docstring of test_forms_that_are_not_exact, and
DESIGN.md 3.8c with the largest error of each form."""
import pytest
import torch

import vgg_exact as vx

pytestmark = pytest.mark.gpu

# name -> (compute dtype, winograd3, winograd7)
EXACT_PLANS = {"fp32-direct": ("fp32", 0, 0), "fp32-wino2": ("fp32", 1, 0), "bf16": ("bf16", 0, 0), "bf16x3": ("bf16x3", 0, 0)}
CASE_PLANS = [(c, p) for c in vx.CASES for p, (dtype, _, _) in EXACT_PLANS.items() if vx.admits(c, dtype)]
# name -> (winograd3, winograd7, the form code rtpose_net_conv_numerics reports for the forced form, the kernel size it is for)
OTHER_FORMS = {"F(4x4,3x3)": (4, 0, 43, 3), "F(4,7)": (0, 4, 4, 7), "F(6,7)": (0, 6, 6, 7), "F(8,7)": (0, 8, 8, 7),
               "default": (None, None, None, None)}
EXACT_FORMS = (0, 3)        # direct, F(2x2,3x3)


@pytest.fixture(scope="module")
def model(pkg, cuda):
    m = pkg.get_model('vgg19').cuda().eval()
    yield m
    m._plans.clear()


def _load(m, c, family=0):
    m.load_state_dict(vx.state_dict(vx.tracer(c, family).ops))


def _set(m, plan, fresh=True):
    dtype, w3, w7 = plan
    m.set_compute_dtype(dtype).set_winograd(winograd3=w3, winograd7=w7)
    if fresh:
        m._plans.clear()        # (the plan cache of _native_state.py: the next forward creates its plan and its workspace)


def _run(m, x, keep=True):
    m.keep_intermediates = keep
    try:
        with torch.no_grad():
            (paf, heat), saved = m(x)
    finally:
        m.keep_intermediates = True
    assert paf is saved[10] and heat is saved[11]
    return [None if s is None else s.cpu() for s in saved]


def _same(got, want, what):
    """== with a message that says where"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | (got.isnan() != want.isnan())
    first = bad.nonzero()[:6].tolist()
    raise AssertionError("%s: %d of %d elements differ (images %s, channels %s); first at %s: got %s, want %s" % (
        what, int(bad.sum()), bad.numel(), sorted(set(bad.nonzero()[:, 0].tolist())), sorted(set(bad.nonzero()[:, 1].tolist()))[:16],
        first, [got[tuple(i)].item() for i in first], [want[tuple(i)].item() for i in first]))


def _all_same(got, want, what):
    assert len(got) == len(want) == 12
    for name, g, w in zip(vx.output_names(), got, want):
        _same(g, w, "%s, %s" % (name, what))


def test_the_plan_reports_the_convs_the_restatement_names(model, cuda):
    _set(model, EXACT_PLANS["fp32-direct"])
    plan = model.plan_for(torch.zeros(1, 3, 8, 8, device=cuda))
    got = model.conv_numerics(plan)
    assert [name for name, _, _ in got] == [name for name, _, _, _ in vx.layer_table()]
    assert all(form == 0 for _, form, _ in got)


@pytest.mark.parametrize("c,plan", CASE_PLANS, ids=["%s-%s" % (vx.case_id(c), p) for c, p in CASE_PLANS])
def test_tracer_is_exact(model, cuda, c, plan):
    """a.  Every stored activation of the case is an integer every exact plan holds exactly: the 12 outputs are the
    restatement's bits - and the 12 of another image under the same operands too, and then the first ones again."""
    t = vx.tracer(c)
    want = vx.expected(c)
    _load(model, c)
    _set(model, EXACT_PLANS[plan])
    x = t.x.to(cuda)
    _all_same(_run(model, x), want, "fresh %s plan" % plan)
    x2 = vx.image(c, 2)
    _all_same(_run(model, x2.to(cuda)), vx.expected_of(c, x2), "%s plan, another image" % plan)
    _all_same(_run(model, x), want, "%s plan after other data" % plan)
    forms = {form for _, form, _ in model.conv_numerics(model.plan_for(x))}
    assert forms == ({0, 3} if plan == "fp32-wino2" else {0})


@pytest.mark.parametrize("plan", list(EXACT_PLANS))
@pytest.mark.parametrize("shape", [(5, 24, 24), (2, 64, 72)], ids=["5x24x24", "2x64x72"])
def test_last_outputs_without_the_stage_records(model, cuda, shape, plan):
    """b.  keep_intermediates = False: no OP_SAVE runs.  The bf16 plan's stage-6 heads write the fp32 record themselves, at
    offsets {0, 38}; the other plans' record of stage 6 is still made.  Outputs 10 and 11 are the integers either way, on
    a fresh plan that never ran an OP_SAVE and after a forward that did."""
    c = vx.by_shape(*shape)
    want = vx.expected(c)
    _load(model, c)
    _set(model, EXACT_PLANS[plan])
    x = vx.tracer(c).x.to(cuda)
    for what in ("fresh", "after a forward with the records"):
        got = _run(model, x, keep=False)
        assert got[:10] == [None] * 10
        _same(got[10], want[10], "PAF without the records, %s, %s" % (what, plan))
        _same(got[11], want[11], "heat-map without the records, %s, %s" % (what, plan))
        _all_same(_run(model, x), want, "%s with the records" % plan)


def _exact_outputs(forms):
    """indices of the 12 outputs whose whole chain - trunk, the stages before, the own branch; every stage reads both heads of
    the one before - ran in exact forms"""
    form = {name: f for name, f, _ in forms}
    nt = vx.net()
    ok = all(form[l.name] in EXACT_FORMS for l in nt.trunk)
    out = []
    for s in range(1, 7):
        br = [ok and all(form[l.name] in EXACT_FORMS for l in nt.stage[(s, b)]) for b in (1, 2)]
        out += [2 * (s - 1) + i for i in (0, 1) if br[i]]
        ok = all(br)
    return out


@pytest.mark.parametrize("name", list(OTHER_FORMS))
@pytest.mark.parametrize("shape", [(5, 24, 24), (2, 64, 72)], ids=["5x24x24", "2x64x72"])
def test_forms_that_are_not_exact(model, cuda, shape, name):
    """c.  |out - integers| <= 1e-3 * max(1, max |integers|) - below half a unit, so a wrong integer term fails it - for all
    12 outputs, in fp32 plans with one form forced and in the default plan; the forced form ran on at least one conv; outputs
    whose whole chain ran direct or F(2x2,3x3) are ==.  The largest error of each form is printed (pytest -s) and recorded in
    DESIGN.md 3.8c.
    What ran, at both shapes: winograd3 = 4 - F(4x4,3x3) on the 17 3x3 convs with >= 32 input channels (model0.2 .. model0.25,
    model1_{1,2}.0 .. .4), conv1_1 (3 input channels) direct, as every 7x7 and 1x1 conv; winograd7 = 4 / 6 / 8 - the forced
    form on all 50 7x7 convs (model{2..6}_{1,2}.0 .. .8), everything else direct.  No forced form fell back: at 3 x 3 and
    8 x 9 stage maps conv2d_winograd_fits admits every F(m,7).  The default plan chooses per conv from the amplification
    estimates of the loaded filters (amp_limit 256): F(4x4,3x3) on the 17, and for the 7x7 convs what DESIGN.md 3.8c records
    of each shape."""
    c = vx.by_shape(*shape)
    want = vx.expected(c)
    w3, w7, code, k = OTHER_FORMS[name]
    _load(model, c)
    _set(model, ("fp32", w3, w7))
    x = vx.tracer(c).x.to(cuda)
    got = _run(model, x)
    forms = model.conv_numerics(model.plan_for(x))
    ran = sorted({f for _, f, _ in forms})
    if code is not None:
        on = [n for n, f, _ in forms if f == code]
        assert on, "%s ran nowhere at %s: forms %s" % (name, vx.case_id(c), ran)
        assert all(vx.net().table[n].k == k for n in on)
        assert {f for n, f, _ in forms if vx.net().table[n].k not in (k, 1)} == {0}
    bound = vx.TOL * max(1.0, max(w.abs().max().item() for w in want))
    assert bound < 0.5
    err = [(g - w).abs().max().item() for g, w in zip(got, want)]
    exact = _exact_outputs(forms)
    print("\n%s at %s: forms %s (%s), max error %.3g of bound %.3g, outputs with an exact chain %s" % (
        name, vx.case_id(c), ran, ", ".join("%d x form %d" % (sum(1 for _, f, _ in forms if f == r), r) for r in ran), max(err),
        bound, exact))
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(g).all()
        assert err[i] <= bound, "%s, %s: max error %g above %g" % (vx.output_names()[i], name, err[i], bound)
        if i in exact:
            _same(g, w, "%s (exact chain under %s)" % (vx.output_names()[i], name))
    if w3 == 0 and w7 in (4, 6, 8):
        assert exact[:2] == [0, 1]          # the trunk and stage 1 hold no 7x7 conv


@pytest.mark.parametrize("plan", list(EXACT_PLANS))
def test_an_image_has_the_same_bits_in_a_batch_of_one(model, cuda, plan):
    """d.  5x24x24: 45 stage pixels, one strip tile and one block of the 1x1 pair hold all five images."""
    c = vx.by_shape(5, 24, 24)
    want = vx.expected(c)
    _load(model, c)
    _set(model, EXACT_PLANS[plan])
    x = vx.tracer(c).x.to(cuda)
    for i in (0, 2, 4):
        _all_same(_run(model, x[i:i + 1]), [w[i:i + 1] for w in want], "image %d alone, %s" % (i, plan))
    pair = _run(model, x[[3, 1]])
    _all_same(pair, [w[[3, 1]] for w in want], "images 3 and 1 as a batch of two, %s" % plan)


def test_operands_and_dtypes_change_on_one_module(model, cuda):
    """e.  Tracer A; tracer B (other seeds of filters and image) loaded into the same module at the same shape - the plans
    stay, the arenas are packed again -; A again gives the first bits.  All the while the module goes fp32 -> bf16 ->
    bf16x3 -> fp32 (the F(2x2,3x3) plan), and every plan stays exact."""
    c = vx.by_shape(5, 24, 24)
    order = ("fp32-direct", "bf16", "bf16x3", "fp32-wino2")
    model._plans.clear()
    first = {}
    for family in (0, 1, 0):
        _load(model, c, family)
        x = vx.tracer(c, family).x.to(cuda)
        want = vx.expected(c, family)
        for plan in order:
            _set(model, EXACT_PLANS[plan], fresh=False)
            got = _run(model, x)
            _all_same(got, want, "tracer %s, %s" % ("AB"[family], plan))
            if family == 0:
                for a, b in zip(first.setdefault(plan, got), got):
                    assert torch.equal(a, b)
    assert len(model._plans) == len(order)


@pytest.mark.parametrize("plan", list(EXACT_PLANS))
def test_a_nan_pixel_stays_in_its_image(model, cuda, plan):
    """f.  Image 2 of the five of 5x24x24 carries NaN pixels, in the corners, on an edge and inside; one strip tile and one
    block of the 1x1 pair hold pixels of all five images.  The other four images' 12 outputs are still the integers.  (Every
    filter row of the family has a non-zero tap: no output is the bias alone, which would be right whatever the kernel read.
    What image 2 itself gives is not asserted: include/rtpose_mi355x.h, "Non-finite values", promises nothing for the
    executors - their ReLU is max(v, 0), which stores a NaN sum as 0 -, and only the bf16x3 plan, whose conv1_1 is the
    generic kernel, was seen to carry the NaN to its outputs.)"""
    c = vx.by_shape(5, 24, 24)
    t = vx.tracer(c)
    assert all((w != 0).flatten(1).any(1).all() for w, _ in t.ops.values())
    want = vx.expected(c)
    _load(model, c)
    _set(model, EXACT_PLANS[plan])
    bad = t.x.clone()
    for ch, yy, xx in ((0, 0, 0), (1, 0, 23), (2, 23, 0), (0, 23, 23), (1, 11, 13), (2, 0, 7), (0, 16, 23)):
        bad[2, ch, yy, xx] = float("nan")
    clean = [0, 1, 3, 4]
    assert torch.equal(bad[clean], t.x[clean]) and bad[2].isnan().sum() == 7
    got = _run(model, bad.to(cuda))
    _all_same([g[clean] for g in got], [w[clean] for w in want], "the clean images, %s" % plan)
