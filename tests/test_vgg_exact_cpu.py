"""The conditions under which tests/test_vgg_exact_gpu.py may compare the rtpose_vgg plans with the float64 restatement of
tests/vgg_exact.py by ==, asserted per case from the restatement's side only (no GPU, no library call): the edge tags from
the shape chain of csrc/net.hip's add_trunk, integer activations of magnitude <= 256, S < 2^24, bf16-exact operands,
liveness of every channel, the per-layer conditions of F(2x2,3x3), 1e-3 of the output scale below half a unit, the
mutations, the state dict through network.RtposeVGG, and the restatement itself against oracle/net_oracle.py."""
import importlib

import pytest
import torch

import vgg_exact as vx
from conftest import PKG_NAME

IDS = [vx.case_id(c) for c in vx.CASES]


@pytest.fixture(scope="module")
def network(pkg):
    return importlib.import_module(PKG_NAME + ".network")


@pytest.fixture(scope="module")
def model(network):
    return network.get_model('vgg19')


def test_cases_hold_the_base_shapes_and_reach_every_required_edge():
    shapes = [(c.n, c.h, c.w) for c in vx.CASES]
    assert len(set(shapes)) == len(shapes) and len({c.seed for c in vx.CASES}) == len(vx.CASES)
    assert tuple(shapes[:len(vx.BASE_SHAPES)]) == vx.BASE_SHAPES
    reached = {t for c in vx.CASES for t in c.tags}
    assert set(vx.REQUIRED) <= reached, set(vx.REQUIRED) - reached
    assert all(c.h >= 8 and c.w >= 8 for c in vx.CASES)                      # rtpose_net_create_opts: H, W >= 8
    assert all(c.h * c.w <= 64 * 72 and c.n <= 5 for c in vx.CASES)          # no image above 64x72 is compared with ==
    # the dtypes: the first five shapes run in every plan, the others in fp32 only
    assert [vx.admits(c, "bf16") for c in vx.CASES] == [True] * 5 + [False] * (len(vx.CASES) - 5)
    assert all(("multiple of 8" in c.tags) == vx.admits(c, "bf16x3") and vx.admits(c, "fp32") for c in vx.CASES)


@pytest.mark.parametrize("c", vx.CASES, ids=IDS)
def test_edge_tags(c):
    g = vx.chain(c.n, c.h, c.w)
    assert c.tags
    for t in c.tags:
        assert vx.EDGES[t](g), "%s does not reach %r: %s" % (vx.case_id(c), t, vars(g))
    # the chain is torch's own: three floor-mode pools
    a = torch.zeros(1, 1, c.h, c.w)
    got = []
    for _ in range(3):
        a = torch.nn.functional.max_pool2d(a, 2)
        got.append(tuple(a.shape[2:]))
    assert got == [(g.H1, g.W1), (g.H2, g.W2), (g.H3, g.W3)]
    # the stage map as the restatement has it
    assert tuple(vx.tracer(c).outs[0].shape) == (c.n, 38, g.H3, g.W3) and tuple(vx.tracer(c).outs[11].shape) == (c.n, 19, g.H3, g.W3)


def test_layer_table_names_the_convs_of_the_module(model):
    m = model
    convs = m._convs()
    assert [(name, cv.out_channels, cv.in_channels, cv.kernel_size[0]) for name, cv in convs] == vx.layer_table()
    assert len(vx.layer_table()) == 92 and len(m.state_dict()) == 184

    def relu_follows(name):
        seq, idx = name.split(".")
        mods, i = getattr(m, seq), int(idx) + 1
        return i < len(mods) and isinstance(mods[i], torch.nn.ReLU)
    assert {name: relu_follows(name) for name, _ in convs} == {l.name: l.relu for l in vx.net().table.values()}
    pools = [l.name for l in vx.net().trunk if l.pool]
    assert pools == ["model0.%d" % i for i in (2, 7, 16)]                     # oracle/net_oracle.py: VGG_POOL_AFTER
    assert vx.output_names() == ["model%d_%d.%d" % (s, b, 8 if s == 1 else 12) for s in range(1, 7) for b in (1, 2)]


@pytest.mark.parametrize("c", vx.CASES, ids=IDS)
def test_conditions_of_equality(c):
    t = vx.tracer(c)
    r = vx.conditions(c)
    assert r.same, "the fp32 draw did not see what the float64 restatement gives of the operands"
    assert r.integers
    assert r.act_max <= vx.ACT_MAX, "an activation of magnitude %g is no bf16 value" % r.act_max
    assert r.out_max <= vx.ACT_MAX                                           # the stage 1..5 heads are stored as bf16 too
    assert r.S < vx.LIMIT
    assert r.bf16_operands
    assert not r.dead, "constant channels in %s" % r.dead
    assert r.clipped > 0
    assert all(r.wino.values()), "F(2x2,3x3) is not exact in %s" % [k for k, ok in r.wino.items() if not ok]
    assert len(r.wino) == 12 + 6                                             # the trunk and the 3x3 convs of stage 1
    assert r.tol_below_half
    # the family is what it says it is
    assert t.x.min() >= 1 and t.x.max() <= vx.IMAGE_MAX and torch.equal(t.x, t.x.round())
    hw = {name: tuple(a.shape[2:]) for name, a in t.acts.items()}
    for l in vx.net().table.values():
        w, b = t.ops[l.name]
        assert tuple(w.shape) == (l.cout, l.cin, l.k, l.k) and tuple(b.shape) == (l.cout,)
        assert set(b.unique().tolist()) <= {0.0, 1.0, 2.0}
        f = w.reshape(l.cout, -1)
        nz, pos, neg = (f != 0).sum(1), (f == 1).sum(1), (f == -1).sum(1)
        assert torch.equal(pos + neg, nz) and torch.equal(pos, torch.ones_like(pos)) and neg.max() <= 1, l.name
        assert l.cout < 128 or 0.2 <= neg.double().mean() <= 0.8, l.name      # "every second time"
        # no tap outside what can reach a pixel of the layer's map
        kys, kxs = vx.reach(l.k, *hw[l.name])
        used = (w != 0).any(0).any(0)
        assert not used[[k for k in range(l.k) if k not in kys]].any() and not used[:, [k for k in range(l.k) if k not in kxs]].any()
    outs = vx.expected(c)
    assert len(outs) == 12 and all(o.dtype == torch.float32 for o in outs)
    assert all(torch.equal(o.double(), y) for o, y in zip(outs, t.outs))     # the cast to fp32 loses nothing
    for name, o in zip(vx.output_names(), outs):
        assert not vx._dead(o).any(), name


@pytest.mark.parametrize("c", vx.CASES, ids=IDS)
def test_first_convs_of_the_stages_read_every_head_channel(c):
    """The PAF / heat slices are what the plan permutes: the 2 x 128 rows of a stage's two first convs read each of the 57
    head channels of the concat with at least one non-zero tap (the first draw covers them in each conv; a redrawn row may
    give its channel up, the other branch still holds it), and out1 too."""
    t = vx.tracer(c)
    for s in range(2, 7):
        read = torch.zeros(vx.N_CAT, dtype=torch.bool)
        for b in (1, 2):
            read |= (t.ops["model%d_%d.0" % (s, b)][0] != 0).flatten(2).any(2).any(0)
        unread = (~read[:vx.N_HEADS]).nonzero().flatten().tolist()
        # (on a one-pixel map a head that is negative in every image has no live row of its own: up to two may go unread)
        assert len(unread) <= (2 if t.outs[0][0, 0].numel() == 1 else 0), "stage %d: head channels %s unread" % (s, unread)
        assert read[vx.N_HEADS:].sum() >= 64


@pytest.mark.parametrize("c", vx.CASES, ids=IDS)
def test_state_dict_loads_into_the_module_bit_for_bit(model, c):
    """The door of the GPU tests is RtposeVGG.load_state_dict: the 184 keys, and what _sync_weights hands to
    rtpose_net_load_conv - conv.weight / conv.bias of _convs(), fp32, contiguous - are the operands."""
    t = vx.tracer(c)
    m = model
    sd = vx.state_dict(t.ops)
    assert list(sd) == list(m.state_dict()) and len(sd) == 184
    m.load_state_dict(sd)
    for name, cv in m._convs():
        w, b = t.ops[name]
        assert cv.weight.dtype == torch.float32 and cv.weight.is_contiguous()
        assert torch.equal(cv.weight.detach(), w) and torch.equal(cv.bias.detach(), b), name
    back = vx.ops_of(m.state_dict())
    assert all(torch.equal(back[k][0].float(), t.ops[k][0]) and torch.equal(back[k][1].float(), t.ops[k][1]) for k in t.ops)


@pytest.mark.parametrize("c", vx.CASES, ids=IDS)
def test_every_mutation_moves_an_output(c):
    table = vx.mutations(c)
    g = vx.chain(c.n, c.h, c.w)
    assert len(table) == (10 if not all(g.fused) else 9)
    assert len(dict(table)["one concat channel read from its neighbour"]) == 8     # every group of channels has its site
    for what, sites in table:
        assert sites, what
        moved = [vx.moves_an_output(c, m) for m in sites]
        assert moved[0], "%s: the outputs of %s do not notice" % (what, vx.case_id(c))
        assert 2 * sum(moved) >= len(moved), (what, moved)


def test_other_operands_of_a_case_differ_and_hold_the_conditions_too():
    """tracer B of the A-B-A test and the other image of the fresh / after-other-data test"""
    c = vx.by_shape(5, 24, 24)
    a, b = vx.tracer(c), vx.tracer(c, 1)
    assert not torch.equal(a.x, b.x) and not torch.equal(a.ops["model3_1.0"][0], b.ops["model3_1.0"][0])
    assert all(torch.equal(y, y.round()) and y.abs().max() <= vx.ACT_MAX for y in list(b.acts.values()) + b.outs)
    assert not any(torch.equal(p, q) for p, q in zip(vx.expected(c), vx.expected(c, 1)))
    x2 = vx.image(c, 2)
    acts, outs = vx.forward(a.ops, x2)
    assert all(torch.equal(y, y.round()) and y.abs().max() <= vx.ACT_MAX for y in list(acts.values()) + outs)
    assert not any(torch.equal(p, q) for p, q in zip(vx.expected(c), vx.expected_of(c, x2)))


def test_an_image_of_the_restatement_does_not_depend_on_its_batch():
    c = vx.by_shape(5, 24, 24)
    t = vx.tracer(c)
    _, outs = vx.forward(t.ops, t.x[3:4])
    assert all(torch.equal(o, w[3:4]) for o, w in zip(outs, t.outs))


def test_restatement_matches_the_oracle_on_random_weights(model):
    """The new restatement is itself pinned on the seeded random state dict of tests/test_net_gpu.py.  Double precision
    against double precision: the oracle's own trunk() / branch() on the float64 state dict, composed as its forward()
    composes them, give the restatement's bits (both are ATen's float64 conv2d, called alike).  oracle forward() itself
    computes in fp32: 47 layers in sequence, sums of up to 185 * 49 terms at 2^-24 each, is what 1e-4 of the map scale
    leaves room for."""
    from oracle import net_oracle as no
    sd = no.he_init_state_dict(model, seed=0)
    ops = vx.ops_of(sd)
    sd64 = {k: v.double() for k, v in sd.items()}
    for shape, seed in (((2, 3, 24, 40), 5), ((1, 3, 29, 35), 6)):
        x = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.5
        acts, outs = vx.forward(ops, x)
        assert len(outs) == 12 and all(o.dtype == torch.float64 for o in outs)
        with torch.no_grad():
            out1 = no.trunk(sd64, x.double())
            inp, saved = out1, []
            for s in range(1, 7):
                n = 5 if s == 1 else 7
                l1, l2 = no.branch(sd64, 'model%d_1' % s, inp, n), no.branch(sd64, 'model%d_2' % s, inp, n)
                saved += [l1, l2]
                inp = torch.cat([l1, l2, out1], 1)
        assert torch.equal(acts["model0.25"], out1)
        for o, r in zip(outs, saved):
            assert r.dtype == torch.float64 and o.shape == r.shape
            assert (o - r).abs().max().item() <= 1e-12 * max(1.0, r.abs().max().item())
        (paf_r, heat_r), saved32 = no.forward(sd, x)
        scale = max(1.0, max(r.abs().max().item() for r in saved32))
        for o, r in zip(outs, saved32):
            assert (o.float() - r).abs().max().item() <= 1e-4 * scale
        assert torch.equal(paf_r, saved32[10]) and torch.equal(heat_r, saved32[11])
