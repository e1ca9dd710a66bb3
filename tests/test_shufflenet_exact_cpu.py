"""The conditions under which tests/test_shufflenet_exact_gpu.py may compare both ShuffleNetV2 plans with the float64
restatement of tests/shufflenet_exact.py by ==, asserted per case from the restatement's side only (no GPU, no library
call): the edge tags from the shape chain of csrc/shufflenet.hip's build(), integer activations of magnitude <= 256,
S < 2^24, bf16-exact operands, liveness of every channel, the exact fold through shufflenet.Network, the mutations, and
the restatement itself against oracle/shufflenet_oracle.py on random weights."""
import importlib

import pytest
import torch

import shufflenet_exact as sx
from conftest import PKG_NAME

IDS = [sx.case_id(c) for c in sx.CASES]


def _network():
    """the test's own instance: eps = 0 in every BatchNorm, so that the fold of shufflenet_exact.state_dict is exact"""
    sn = importlib.import_module(PKG_NAME + ".shufflenet")
    m = sn.Network(1.0)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps = 0.0
    return m.eval()


@pytest.fixture(scope="module")
def network(pkg):
    return _network()


def test_cases_are_the_shapes_of_the_issue_and_reach_every_required_edge():
    shapes = [(c.n, c.h, c.w) for c in sx.CASES]
    assert len(set(shapes)) == len(shapes) and len({c.seed for c in sx.CASES}) == len(sx.CASES)
    for s in ((1, 32, 32), (2, 33, 47), (3, 61, 75), (2, 97, 131), (5, 40, 88)):
        assert s in shapes
    reached = {t for c in sx.CASES for t in c.tags}
    assert set(sx.REQUIRED) <= reached, set(sx.REQUIRED) - reached
    assert all(c.h >= 32 and c.w >= 32 for c in sx.CASES)          # rtpose_shufflenet_create_ex: H, W >= 32


@pytest.mark.parametrize("c", sx.CASES, ids=IDS)
def test_edge_tags(c):
    g = sx.chain(c.h, c.w)
    assert c.tags
    for t in c.tags:
        assert sx.EDGES[t](c.n, g), "%s does not reach %r: %s" % (sx.case_id(c), t, vars(g))
    # the chain is torch's own: stem conv, ceil-mode pool, stride-2 depthwise
    a = torch.zeros(1, 1, c.h, c.w)
    a1 = torch.nn.functional.conv2d(a, torch.zeros(1, 1, 3, 3), None, 2, 1)
    a2 = torch.nn.functional.max_pool2d(a1, 3, 2, 0, ceil_mode=True)
    a3 = torch.nn.functional.conv2d(a2, torch.zeros(1, 1, 3, 3), None, 2, 1)
    assert (tuple(a1.shape[2:]), tuple(a2.shape[2:]), tuple(a3.shape[2:])) == ((g.H1, g.W1), (g.H2, g.W2), (g.H3, g.W3))


def test_layer_table_names_the_modules_of_the_network(network):
    sd = network.state_dict()
    for name in sx.TABLE:
        m = network._module_by_prefix(name)
        w = m.weight if not isinstance(m, torch.nn.Sequential) else m[0].weight
        assert tuple(w.shape) == sx.weight_shape(name), name
    assert len(sx.TABLE) == 59 and sum(1 for k in sx.TABLE.values() if k[0] in (sx.K_DW, sx.K_PW, sx.K_STEM)) == 58
    assert len(sd) == 345


@pytest.mark.parametrize("c", sx.CASES, ids=IDS)
def test_conditions_of_equality(c):
    t = sx.tracer(c)
    r = sx.conditions(c)
    assert r.same, "the recorded restatement is not what forward() gives of the operands"
    assert r.integers
    assert r.act_max <= sx.ACT_MAX, "an activation of magnitude %g is no bf16 value" % r.act_max
    assert r.S < sx.LIMIT
    assert r.bf16_operands
    assert not r.dead, "constant channels in %s" % r.dead
    assert r.clipped > 0
    # the family is what it says it is
    assert t.x.min() >= 1 and t.x.max() <= sx.IMAGE_MAX and torch.equal(t.x, t.x.round())
    s, sh = t.ops["network.0"]
    assert set(s.tolist()) <= {1.0, 2.0} and torch.equal(sh, sh.round())
    for name, (kind, cout, cin) in sx.TABLE.items():
        w, b = t.ops[name]
        if kind == sx.K_AFFINE:
            continue
        assert tuple(w.shape) == sx.weight_shape(name) and tuple(b.shape) == (cout,)
        assert set(b.unique().tolist()) <= {0.0, 1.0, 2.0}
        f = w.reshape(cout, -1)
        nz, pos, neg = (f != 0).sum(1), (f == 1).sum(1), (f == -1).sum(1)
        assert torch.equal(pos + neg, nz), name
        if kind == sx.K_STEM:
            assert nz.min() >= 1 and nz.max() <= 3
        elif kind == sx.K_DW:
            assert torch.equal(pos, torch.ones_like(pos)) and neg.sum() == 0
            assert len(f.argmax(1).unique()) >= (9 if cout >= 116 else 7 if cout >= 58 else 5),"taps of the 3x3 that %s never uses" % name
        elif name in ("paf", "heatmap"):
            assert nz.min() >= 1 and nz.max() <= sx.HEAD_TERMS and pos.min() >= 1
        else:
            assert torch.equal(pos, torch.ones_like(pos)) and neg.max() <= 1
            assert 0.25 <= neg.double().mean() <= 0.75, name
    paf, heat = sx.expected(c)
    g = sx.chain(c.h, c.w)
    assert paf.shape == (c.n, 38, g.H3, g.W3) and heat.shape == (c.n, 19, g.H3, g.W3)


@pytest.mark.parametrize("c", sx.CASES, ids=IDS)
def test_network_folds_the_state_dict_to_the_operands_bit_for_bit(network, c):
    """The door of the GPU tests is shufflenet.Network.load_state_dict: what Network._fold, and the scale / shift that
    Network._sync_weights makes of the input BatchNorm, hand to rtpose_shufflenet_load are the intended operands."""
    t = sx.tracer(c)
    network.load_state_dict(sx.state_dict(t.ops, network.state_dict()))
    for name, (kind, _, _) in sx.TABLE.items():
        m = network._module_by_prefix(name)
        w, b = t.ops[name]
        if kind == sx.K_AFFINE:       # (the expressions of Network._sync_weights, kind 0)
            s = m.weight.detach() / torch.sqrt(m.running_var.detach() + m.eps)
            got = s.float().contiguous(), (m.bias.detach() - m.running_mean.detach() * s).float().contiguous()
        elif isinstance(m, torch.nn.Conv2d):
            got = m.weight.detach().float().contiguous(), m.bias.detach().float().contiguous()
        else:
            got = network._fold(m[0], m[1])
        assert got[0].dtype == torch.float32 and torch.equal(got[0], w) and torch.equal(got[1], b), name
    # ... and the float64 fold of the same state dict gives them too
    ops = sx.fold_state_dict(network.state_dict(), 0.0)
    assert all(torch.equal(ops[k][0].float(), t.ops[k][0]) and torch.equal(ops[k][1].float(), t.ops[k][1]) for k in sx.TABLE)


@pytest.mark.parametrize("c", sx.CASES, ids=IDS)
def test_every_mutation_moves_an_output(c):
    table = sx.mutations(c)
    assert len(table) >= 9
    for what, sites in table:
        assert sites, what
        moved = [sx.moves_an_output(c, m) for m in sites]
        assert moved[0], "%s: the outputs of %s do not notice" % (what, sx.case_id(c))
        assert 2 * sum(moved) >= len(moved), (what, moved)


def test_an_image_of_the_restatement_does_not_depend_on_its_batch():
    c = sx.CASES[2]
    t = sx.tracer(c)
    _, paf, heat = sx.forward(t.ops, t.x[1:2])
    assert torch.equal(paf, t.paf[1:2]) and torch.equal(heat, t.heat[1:2])


def test_restatement_matches_the_oracle_on_random_weights(pkg):
    """The new restatement is itself pinned: on the seeded random state dict of tests/test_shufflenet_gpu.py, folded in
    float64 with the oracle's eps, it gives oracle/shufflenet_oracle.forward's maps.  The oracle computes in fp32: its
    own rounding (57 layers, sums of up to 1024 terms at 2^-24 each) is what the bound 1e-4 of the map scale leaves room for."""
    from oracle import shufflenet_oracle as so
    sn = importlib.import_module(PKG_NAME + ".shufflenet")
    sd = so.seeded_state_dict(sn.Network(1.0), seed=0)
    ops = sx.fold_state_dict(sd, so.BN_EPS)
    for shape, seed in (((2, 3, 33, 47), 5), ((1, 3, 61, 75), 6)):
        x = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.5
        paf_r, heat_r = so.forward(sd, x)
        acts, paf, heat = sx.forward(ops, x)
        assert paf.dtype == torch.float64 and paf.shape == paf_r.shape and heat.shape == heat_r.shape
        scale = max(1.0, paf_r.abs().max().item(), heat_r.abs().max().item())
        assert (paf.float() - paf_r).abs().max().item() <= 1e-4 * scale
        assert (heat.float() - heat_r).abs().max().item() <= 1e-4 * scale
        g = sx.chain(shape[2], shape[3])
        assert acts["pool"].shape == (shape[0], 24, g.H2, g.W2) and acts["network.5.3"].shape == (shape[0], 464, g.H3, g.W3)
