"""Both ShuffleNetV2 plans (csrc/shufflenet.hip: the fp32 and the bf16 launch lists) pinned as a whole, through
shufflenet.Network:

a. the tracer cases of tests/shufflenet_exact.py - PAF and heat-map == the float64 restatement cast to fp32, on a fresh plan
   and again after a forward of other data (conditions, edge tags and mutations: tests/test_shufflenet_exact_cpu.py);
b. an image's maps are the same bits in every batch size;      c. a forward does not depend on what an earlier one left;
d. NaN / Inf pixels of one image stay in that image;           e. odd sizes against the oracles of oracle/shufflenet_oracle.py
                                                                  at the tolerances of tests/test_shufflenet_gpu.py.
b - d are invariance properties and compare runs of the library with each other, on the seeded random weights of
tests/test_shufflenet_gpu.py; a and e compare with a reference."""
import ctypes as C
import importlib

import pytest
import torch

import shufflenet_exact as sx
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DTYPES = ("fp32", "bf16")


def _run(m, x):
    with torch.no_grad():
        (paf, heat), _ = m(x)
    return paf.clone(), heat.clone()


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


@pytest.fixture(scope="module")
def net_sd(pkg, cuda):
    """the construction of tests/test_shufflenet_gpu.py's net_sd"""
    from oracle import shufflenet_oracle as so
    sn = importlib.import_module(PKG_NAME + ".shufflenet")
    m = sn.Network(1.0)
    sd = so.seeded_state_dict(m, seed=0)
    m.load_state_dict(sd)
    return m.cuda().eval(), sd


def _tracer_network(cuda, c, dtype):
    """A Network of the test's own (eps = 0 in every BatchNorm: the fold is then exact, tests/test_shufflenet_exact_cpu.py)
    that takes the case's operands through load_state_dict; all its plans are fresh."""
    sn = importlib.import_module(PKG_NAME + ".shufflenet")
    m = sn.Network(1.0)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps = 0.0
    m = m.cuda().eval()
    m.load_state_dict(sx.state_dict(sx.tracer(c).ops, m.state_dict()))
    return m.set_compute_dtype(dtype)


def test_the_plan_reports_the_layers_the_restatement_names(pkg, capi, cuda):
    m = _tracer_network(cuda, sx.CASES[0], "fp32")
    for dtype in DTYPES:
        plan = m.set_compute_dtype(dtype).plan_for(torch.zeros(1, 3, 32, 32, device=cuda))
        lib = capi.lib
        name = C.create_string_buffer(96)
        kind, co, ci = C.c_int(), C.c_int(), C.c_int()
        got = []
        for i in range(lib.rtpose_shufflenet_num_layers(plan.handle)):
            capi.check(lib.rtpose_shufflenet_layer_info(plan.handle, i, name, 96, C.byref(kind), C.byref(co), C.byref(ci)))
            got.append((name.value.decode(), kind.value, co.value, ci.value))
        assert got == sx.layer_table()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", sx.CASES, ids=[sx.case_id(c) for c in sx.CASES])
def test_tracer_is_exact(pkg, cuda, c, dtype):
    """a.  Every activation of the case is an integer both plans hold exactly: PAF and heat-map are the restatement's bits."""
    t = sx.tracer(c)
    want_paf, want_heat = sx.expected(c)
    m = _tracer_network(cuda, c, dtype)
    x = t.x.to(cuda)
    paf, heat = _run(m, x)
    _same(paf.cpu(), want_paf, "PAF, fresh %s plan" % dtype)
    _same(heat.cpu(), want_heat, "heat-map, fresh %s plan" % dtype)
    other = (torch.rand(x.shape, generator=torch.Generator().manual_seed(c.seed)) * 37.0 - 11.0).to(cuda)
    _run(m, other)
    paf, heat = _run(m, x)
    _same(paf.cpu(), want_paf, "PAF, %s plan after other data" % dtype)
    _same(heat.cpu(), want_heat, "heat-map, %s plan after other data" % dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(61, 75), (64, 96)], ids=["61x75", "64x96"])
def test_an_image_has_the_same_bits_in_every_batch_size(net_sd, cuda, hw, dtype):
    """b.  Images 0, 2 and 4 of a 5-image batch, in batches of 1, 2, 3 and 5 and at several positions."""
    m, _ = net_sd
    x = (torch.rand(5, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(31)) - 0.5).to(cuda)
    m.set_compute_dtype(dtype)
    try:
        alone = {i: _run(m, x[i:i + 1]) for i in (0, 2, 4)}
        assert not torch.equal(alone[0][0], alone[2][0])
        for batch in ([0], [0, 2], [4, 0], [4, 0, 2], [2, 1, 4], [0, 1, 2, 3, 4]):
            paf, heat = _run(m, x[batch])
            for pos, i in enumerate(batch):
                if i in alone:
                    _same(paf[pos:pos + 1], alone[i][0], "PAF of image %d at %d of %s (%s)" % (i, pos, batch, dtype))
                    _same(heat[pos:pos + 1], alone[i][1], "heat-map of image %d at %d of %s (%s)" % (i, pos, batch, dtype))
    finally:
        m.set_compute_dtype("fp32")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_forward_does_not_depend_on_an_earlier_one(net_sd, cuda, dtype):
    """c.  A, B, A on one plan at an odd size."""
    m, _ = net_sd
    g = torch.Generator().manual_seed(32)
    a = (torch.rand(2, 3, 45, 83, generator=g) - 0.5).to(cuda)
    b = (torch.rand(2, 3, 45, 83, generator=g) * 9.0 - 3.0).to(cuda)
    m.set_compute_dtype(dtype)
    try:
        plan = m.plan_for(a)
        first = _run(m, a)
        other = _run(m, b)
        again = _run(m, a)
        assert m.plan_for(a) is plan
    finally:
        m.set_compute_dtype("fp32")
    assert not torch.equal(first[0], other[0])
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_pixels_stay_in_their_image(net_sd, cuda, dtype):
    """d.  Image 1 of 3 holds NaN, +Inf and -Inf, border pixels included: images 0 and 2 are the bits of the clean batch.
    (3 x 8 x 10 stage pixels: every linear pixel tile of the pointwise kernels holds pixels of two images.)"""
    m, _ = net_sd
    g = torch.Generator().manual_seed(33)
    x = torch.rand(3, 3, 61, 75, generator=g) - 0.5
    bad = x.clone()
    r = torch.rand(3, 61, 75, generator=g)
    bad[1][r < 0.02] = float("nan")
    bad[1][(r >= 0.02) & (r < 0.04)] = float("inf")
    bad[1][(r >= 0.04) & (r < 0.06)] = float("-inf")
    for ch, (yy, xx), v in ((0, (0, 0), "nan"), (1, (0, 74), "inf"), (2, (60, 0), "-inf"), (0, (60, 74), "nan"),
                            (1, (0, 37), "-inf"), (2, (60, 38), "inf"), (0, (30, 0), "inf"), (1, (31, 74), "nan")):
        bad[1, ch, yy, xx] = float(v)
    assert torch.equal(bad[[0, 2]], x[[0, 2]])
    m.set_compute_dtype(dtype)
    try:
        clean = _run(m, x.to(cuda))
        dirty = _run(m, bad.to(cuda))
    finally:
        m.set_compute_dtype("fp32")
    assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[1]).all()
    assert not torch.equal(dirty[0][1], clean[0][1])
    for k, what in ((0, "PAF"), (1, "heat-map")):
        _same(dirty[k][[0, 2]], clean[k][[0, 2]], "%s of the clean images (%s)" % (what, dtype))


@pytest.mark.parametrize("shape", [(2, 3, 33, 47), (2, 3, 97, 131)], ids=["2x33x47", "2x97x131"])
def test_odd_sizes_match_the_oracles(net_sd, cuda, shape):
    """e.  fp32 against oracle forward (1e-3 of the map scale), bf16 against its emulation (2e-2) and the fp32 oracle (6e-2):
    the tolerances of tests/test_shufflenet_gpu.py."""
    from oracle import shufflenet_oracle as so
    m, sd = net_sd
    x = torch.rand(shape, generator=torch.Generator().manual_seed(34)) - 0.5
    paf_r, heat_r = so.forward(sd, x)
    paf_e, heat_e = so.forward_bf16_emulated(sd, x)
    m.set_compute_dtype("fp32")
    paf, heat = _run(m, x.to(cuda))
    assert paf.shape == paf_r.shape and heat.shape == heat_r.shape
    scale = max(1.0, paf_r.abs().max().item(), heat_r.abs().max().item())
    assert (paf.cpu() - paf_r).abs().max().item() <= 1e-3 * scale
    assert (heat.cpu() - heat_r).abs().max().item() <= 1e-3 * scale
    m.set_compute_dtype("bf16")
    try:
        paf, heat = _run(m, x.to(cuda))
    finally:
        m.set_compute_dtype("fp32")
    for a, e, r in ((paf, paf_e, paf_r), (heat, heat_e, heat_r)):
        scale = max(1.0, r.abs().max().item())
        assert (a.cpu() - e).abs().max().item() <= 2e-2 * scale, "vs bf16 emulation"
        assert (a.cpu() - r).abs().max().item() <= 6e-2 * scale, "vs fp32 oracle"
