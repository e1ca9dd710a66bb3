"""GPU suite of layout-resident dense stages: train.dense_stage - a StageBlock of an OpenPose_Model as one autograd node whose
PReLU outputs, concatenations and gradients stay in the library's layouts - and resident='dense' of forward_train / train_step.

The contract is the per-conv bf16 path's (tests/test_train_bf16_gpu.py), because no rounding point moves and no conv launch
changes: conv_backward_bf16_restate.EmulConv with float64 F.prelu and torch.cat between, and float64 on exact integer operands.

* Exact stage: B = 2 dense blocks (the smallest in which a block's first conv writes the concat gradient of the block below),
  C = 16, 9 input channels, Mconv6 -> 16, 5 outputs, N = 2 on 9 x 11; integer operands and slopes in {-1, 0, 1} so sparse that
  every activation and gradient is an integer bf16 holds and every sum stays below 2^24 - asserted on the host: the emulation
  with its roundings equals the one without.  Output and every gradient torch.equal float64 autograd of the plain torch
  restatement AND the per-conv path, for seven requires_grad subsets, with every fallback counter 0.
* Random stage: r_native <= 4 max r_emul (test_train_bf16_gpu.check_ratios); the elements that differ from the per-conv path
  are printed and noted, not asserted.
* The whole OpenPose_Model(2, 2, 52, 26) with resident='dense'; one optimizer step; a frozen trunk and first stage; the
  fallbacks; NaN and Inf; the refusals."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_backward_bf16_restate as cb
import conv_driver as cd
import test_train_bf16_gpu as tb
from test_train_bf16_gpu import train, encode, openpose  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N, H, W = 2, 9, 11
BLOCKS, C, CIN, C6, COUT = 2, 16, 9, 16, 5


def stage_shapes(cin=CIN, c=C, c6=C6, cout=COUT, blocks=BLOCKS):
    """(k, cin, cout) of the 3 B + 2 layers in the reference's order"""
    shapes = []
    for b in range(blocks):
        shapes += [(3, cin if b == 0 else 3 * c, c), (3, c, c), (3, c, c)]
    return shapes + [(1, 3 * c, c6), (1, c6, cout)]


SUBSETS = ("all", "x_only", "last_layer_only", "first_block_frozen", "slopes_frozen", "x_not_required", "upper_block_only")


def required(subset, L):
    """(x requires a gradient, per layer: its filters and bias do, per layer: its slope does)"""
    yes, no = [True] * L, [False] * L
    return {"all": (True, yes, yes),
            "x_only": (True, no, no),
            "last_layer_only": (False, no[:-1] + [True], no),
            "first_block_frozen": (True, no[:3] + yes[3:], no[:3] + yes[3:]),
            "slopes_frozen": (True, yes, no),
            "x_not_required": (False, yes, yes),
            "upper_block_only": (False, no[:3] + yes[3:], no[:3] + yes[3:])}[subset]     # the walk stops inside the stage


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def exact_operands(shapes, seed):
    """x in {0, 1}; per output channel two filter taps of +-1, a bias in {0, 1} and a slope in {-1, 0, 1}: |y_i| <= 2 max|input|
    + 1; the top gradient in {-1, 0, 1}, half of it zero.  (x, [(w, b, slope or None)], G)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 2, (N, shapes[0][1], H, W), generator=g).float()
    layers = []
    for i, (k, cin, cout) in enumerate(shapes):
        wt = torch.zeros(cout, cin * k * k)
        for o in range(cout):
            at = torch.randperm(cin * k * k, generator=g)[:2]
            wt[o, at] = torch.tensor([1.0, 1.0 if o % 3 else -1.0])
        b = torch.randint(0, 2, (cout,), generator=g).float()
        a = torch.randint(-1, 2, (cout,), generator=g).float() if i + 1 < len(shapes) else None
        layers.append((wt.view(cout, cin, k, k), b, a))
    G = torch.randint(-1, 2, (N, shapes[-1][2], H, W), generator=g).float() * (torch.rand(N, shapes[-1][2], H, W, generator=g) < 0.5)
    return x, layers, G


def random_operands(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, shapes[0][1], H, W, generator=g)
    layers = []
    for i, (k, cin, cout) in enumerate(shapes):
        a = torch.randn(cout, generator=g) * 0.25 if i + 1 < len(shapes) else None
        layers.append((cd.weights("he", cout, cin, k, g), torch.randn(cout, generator=g) * 0.1, a))
    target = torch.randn(N, shapes[-1][2], H, W, generator=g)
    return x, layers, target


def stage_graph(x, params, conv):
    """the plain restatement of StageBlock.forward: conv(x, w, b) -> z, F.prelu, torch.cat.  (y, [z of every layer])"""
    L, zs = len(params), []
    for b in range((L - 2) // 3):
        outs = []
        for wt, bias, a in params[3 * b:3 * b + 3]:
            zs.append(conv(x, wt, bias))
            x = F.prelu(zs[-1], a)
            outs.append(x)
        x = torch.cat(outs, 1)
    wt, bias, a = params[L - 2]
    zs.append(conv(x, wt, bias))
    wt7, bias7, _ = params[L - 1]
    zs.append(conv(F.prelu(zs[-1], a), wt7, bias7))
    return zs[-1], zs


def named_grads(xin, params):
    grads = {"x": xin.grad}
    for i, (wt, b, a) in enumerate(params):
        grads["w%d" % i], grads["b%d" % i] = wt.grad, b.grad
        if a is not None:
            grads["a%d" % i] = a.grad
    return grads


def host_stage(x, layers, conv, top):
    """the stage on the CPU in float64 with conv(x, w, b); every tensor requires a gradient.  (y, {name: gradient}, [z])"""
    xin = x.clone().double().requires_grad_(True)
    params = [tuple(None if t is None else t.clone().double().requires_grad_(True) for t in layer) for layer in layers]
    y, zs = stage_graph(xin, params, conv)
    top(y).backward()
    return y.detach(), named_grads(xin, params), [z.detach() for z in zs]


def torch_conv(x, wt, b):
    return F.conv2d(x, wt, b, padding=wt.shape[2] // 2)


def device_stage(train, cuda, x, layers, top, form, subset="all"):
    """form 'dense': train.dense_stage; 'per_conv': train.conv2d(prelu=, compute_dtype='bf16') and torch.cat"""
    need_x, need_p, need_a = required(subset, len(layers))
    xin = x.clone().to(cuda).requires_grad_(need_x)
    params = [(wt.clone().to(cuda).requires_grad_(p), b.clone().to(cuda).requires_grad_(p),
               None if a is None else a.clone().to(cuda).requires_grad_(s))
              for (wt, b, a), p, s in zip(layers, need_p, need_a)]
    if form == "dense":
        y = train.dense_stage(xin, params)
    else:
        L, y = len(params), xin
        for blk in range((L - 2) // 3):
            outs = []
            for wt, b, a in params[3 * blk:3 * blk + 3]:
                y = train.conv2d(y, wt, b, prelu=a, compute_dtype='bf16')
                outs.append(y)
            y = torch.cat(outs, 1)
        for wt, b, a in params[L - 2:]:
            y = train.conv2d(y, wt, b, prelu=a, compute_dtype='bf16')
    top(y).backward()
    return y.detach(), named_grads(xin, params)


def per_conv_stage(train, cuda, x, layers, top, subset="all"):
    return device_stage(train, cuda, x, layers, top, "per_conv", subset)


def counters(train):
    return dict(train.bf16_fallbacks, chain=train.chain_fallbacks, dense=train.dense_fallbacks)


def reset(train):
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()
    train.reset_dense_fallbacks()


NONE = {'fwd': 0, 'dgrad': 0, 'chain': 0, 'dense': 0}


# ---- the exact stage ------------------------------------------------------------------------------------------------------------------
_exact = {}


def exact_case(shapes=None, seed=5):
    """operands and the float64 reference of the exact stage, computed once and left unchanged; the host-side conditions (the
    seeds are ones under which no gradient of these sparse operands is all zero)"""
    shapes = shapes or stage_shapes()
    key = (tuple(shapes), seed)
    if key in _exact:
        return _exact[key]
    x, layers, G = exact_operands(shapes, seed)
    top = lambda y: (y * G.to(device=y.device, dtype=y.dtype)).sum()     # noqa: E731
    y_r, g_r, z_r = host_stage(x, layers, lambda t, wt, b: cb.emul_conv(t, wt, b, False, rounding=True), top)
    y_u, g_u, z_u = host_stage(x, layers, lambda t, wt, b: cb.emul_conv(t, wt, b, False, rounding=False), top)
    y64, g64, z64 = host_stage(x, layers, torch_conv, top)
    # every rounding of the bf16 step is the identity on these operands, and the unrounded emulation is torch's autograd
    assert torch.equal(y_r, y_u) and torch.equal(y_u, y64)
    assert set(g_r) == set(g_u) == set(g64) and len(g64) == 1 + 3 * len(shapes) - 1
    for n in g64:
        assert torch.equal(g_r[n], g_u[n]) and torch.equal(g_u[n], g64[n]), n
        assert g64[n].abs().max().item() > 0, "%s: the gradient is all zero" % n
    for z, (_, _, a) in zip(z64[:-1], layers):
        act = F.prelu(z, a.double())
        assert torch.equal(act, act.round()) and 0 < act.abs().max().item() <= 256, "an activation bf16 does not hold"
        assert (z > 0).any() and (z < 0).any() and (z == 0).any(), "a PReLU decides nothing"
    assert all((a > 0).any() and (a < 0).any() and (a == 0).any() for _, _, a in layers[:-1])
    # fp32 sums of integers are exact below 2^24: the largest sum of absolute terms, forward and backward, from the
    # all-positive stage (|x|, |w|, |b|, slopes 1) under |G|, which bounds every partial sum of the real one
    xa = x.abs()
    la = [(wt.abs(), b.abs(), None if a is None else torch.ones_like(a)) for wt, b, a in layers]
    ya, ga, _ = host_stage(xa, la, torch_conv, lambda y: (y * G.abs().double()).sum())
    assert max([ya.max().item()] + [t.max().item() for t in ga.values()]) < 2 ** 24
    _exact[key] = (x, layers, top, y64, g64)
    return _exact[key]


def same_bits(what, y, g, y_want, g_want, subset, L):
    need_x, need_p, need_a = required(subset, L)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y_want.double().cpu()), what + ": y"
    for n, want in g_want.items():
        needed = need_x if n == "x" else (need_a if n[0] == "a" else need_p)[int(n[1:])]
        if not needed:
            assert g[n] is None, (what, n)
            continue
        assert g[n] is not None and g[n].dtype == torch.float32 and g[n].shape == want.shape, (what, n)
        wrong = int((g[n].double().cpu() != want.double().cpu()).sum())
        assert wrong == 0, "%s: d%s: %d of %d elements differ" % (what, n, wrong, want.numel())


@pytest.mark.parametrize("subset", SUBSETS)
def test_exact_stage_equals_float64_and_the_per_conv_path(cuda, train, subset):
    x, layers, top, y64, g64 = exact_case()
    reset(train)
    y, g = device_stage(train, cuda, x, layers, top, "dense", subset)
    assert counters(train) == NONE, "the stage did not stay resident: %s" % counters(train)
    same_bits("dense_stage against float64", y, g, y64, g64, subset, len(layers))
    yp, gp = per_conv_stage(train, cuda, x, layers, top, subset)
    same_bits("dense_stage against the per-conv path", y, g, yp, {n: t for n, t in gp.items() if t is not None}, subset,
              len(layers))
    assert counters(train) == NONE


def test_a_second_backward_needs_retain_graph_and_gives_the_same_bits(cuda, train):
    x, layers, top, y64, g64 = exact_case()
    xin = x.clone().to(cuda).requires_grad_(True)
    params = [tuple(None if t is None else t.clone().to(cuda).requires_grad_(True) for t in layer) for layer in layers]
    y = train.dense_stage(xin, params)
    loss = top(y)
    loss.backward(retain_graph=True)
    first = {n: t.clone() for n, t in named_grads(xin, params).items()}
    for t in [xin] + [t for layer in params for t in layer if t is not None]:
        t.grad = None
    loss.backward()
    second = named_grads(xin, params)
    assert all(torch.equal(first[n], second[n]) for n in first)


# ---- the fallbacks ----------------------------------------------------------------------------------------------------------------------
def test_a_width_that_is_no_multiple_of_16_runs_per_conv_and_is_counted(cuda, train):
    """C = 24: a slice of the concat buffer would not own its 16-channel groups"""
    shapes = stage_shapes(c=24)
    x, layers, top, y64, g64 = exact_case(shapes, seed=7)
    reset(train)
    y, g = device_stage(train, cuda, x, layers, top, "dense")
    assert counters(train) == dict(NONE, dense=1)
    yp, gp = per_conv_stage(train, cuda, x, layers, top)
    same_bits("the fallback against the per-conv path", y, g, yp, gp, "all", len(layers))
    same_bits("the fallback against float64", y, g, y64, g64, "all", len(layers))
    # and so for Mconv6's width alone
    shapes = stage_shapes(c6=24)
    x, layers, top, y64, g64 = exact_case(shapes, seed=6)
    y, g = device_stage(train, cuda, x, layers, top, "dense")
    assert counters(train) == dict(NONE, dense=2)
    same_bits("the fallback against float64", y, g, y64, g64, "all", len(layers))
    reset(train)


def test_refused_convs_fall_back_and_are_counted(cuda, train, monkeypatch):
    """rtpose_conv2d_bf16 refuses none of the shapes at hand, so the refusal is played: train._dense_conv_into answers False
    (what it answers when the launcher returns RTPOSE_E_INVAL before launching) for chosen launches.  A refused forward conv:
    the stage runs conv by conv through conv2d and dense_fallbacks counts it once.  Refused data gradients: each runs in fp32
    on the widened gradient and is counted in bf16_fallbacks['dgrad'].  On exact operands both give float64's values."""
    x, layers, top, y64, g64 = exact_case()
    L = len(layers)
    real, calls = train._dense_conv_into, []

    def refuse(which):
        def conv_into(bf16, *a, **kw):
            calls.append(bf16)
            return False if which(len(calls)) else real(bf16, *a, **kw)
        return conv_into

    yp, gp = per_conv_stage(train, cuda, x, layers, top)
    for which, want_dense, want_dgrad in ((lambda i: i == 5, 1, 0),                 # the second conv of the second block
                                          (lambda i: i > L, 0, L)):                  # every data gradient
        del calls[:]
        monkeypatch.setattr(train, "_dense_conv_into", refuse(which))
        reset(train)
        y, g = device_stage(train, cuda, x, layers, top, "dense")
        monkeypatch.setattr(train, "_dense_conv_into", real)
        assert counters(train) == dict(NONE, dense=want_dense, dgrad=want_dgrad)
        assert len(calls) == (5 if want_dense else 2 * L) and all(calls)
        same_bits("after the fallback, against float64", y, g, y64, g64, "all", L)
        if want_dense:
            same_bits("after the fallback, against the per-conv path", y, g, yp, gp, "all", L)
    reset(train)


# ---- the random stage ---------------------------------------------------------------------------------------------------------------------
def named(g):
    return {n: t for n, t in g.items() if t is not None}


def test_random_stage_against_the_emulation(cuda, train):
    shapes = stage_shapes()
    x, layers, target = random_operands(shapes, seed=41)
    assert all((a > 0).any() and (a < 0).any() for _, _, a in layers[:-1])
    top = lambda y: F.mse_loss(y, target.to(device=y.device, dtype=y.dtype))      # noqa: E731
    _, g64, _ = host_stage(x, layers, torch_conv, top)
    _, ge, _ = host_stage(x, layers, lambda t, wt, b: cb.emul_conv(t, wt, b, False), top)
    reset(train)
    y, g = device_stage(train, cuda, x, layers, top, "dense")
    fallbacks = counters(train)
    assert all(t.dtype == torch.float32 for t in g.values()) and set(g) == set(g64)
    tb.check_ratios("dense_stage", named(g), ge, g64, fallbacks)
    assert fallbacks == NONE
    # against the per-conv path: counted, not asserted
    yp, gp = per_conv_stage(train, cuda, x, layers, top)
    differ = {n: int((g[n] != gp[n]).sum()) for n in g}
    differ["y"] = int((y != yp).sum())
    total = sum(t.numel() for t in g.values()) + y.numel()
    print("dense stage against the per-conv path: %d of %d elements differ %s"
          % (sum(differ.values()), total, {n: d for n, d in differ.items() if d}))
    cd.note("train_dense_vs_per_conv_stage.json", {"elements": total, "differ": differ})


# ---- NaN and Inf ------------------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_travel_as_on_the_per_conv_path(cuda, train):
    shapes = stage_shapes()
    x, layers, target = random_operands(shapes, seed=43)
    x[1, 3, 4, 5] = float("nan")
    G = torch.randn(N, COUT, H, W, generator=torch.Generator().manual_seed(44))
    G[0, 2, 3, 3] = float("inf")
    top = lambda y: (y * G.to(y.device)).sum()      # noqa: E731
    got = []
    for run in (lambda xx: device_stage(train, cuda, xx, layers, top, "dense"), lambda xx: per_conv_stage(train, cuda, xx, layers, top)):
        y, _ = run(x)
        x_ok = torch.where(torch.isnan(x), torch.zeros(()), x)
        _, g = run(x_ok)
        got.append((y, g))
    (yd, gd), (yp, gp) = got
    assert torch.isnan(yd).any(), "the NaN of x did not reach the stage output"
    assert int(torch.isnan(yd).sum()) == int(torch.isnan(yp).sum()) and torch.equal(torch.isnan(yd), torch.isnan(yp))
    bad = ~torch.isfinite(gd["x"])
    assert bad.any(), "the Inf of gy did not reach dx"
    for n in gd:
        assert int(torch.isnan(gd[n]).sum()) == int(torch.isnan(gp[n]).sum()), n
        assert torch.equal(torch.isfinite(gd[n]), torch.isfinite(gp[n])), n


# ---- the whole model ----------------------------------------------------------------------------------------------------------------------
TOPO = tb.TOPO


@pytest.fixture(scope="module")
def net(cuda, train, encode, openpose):
    """OpenPose_Model(2, 2, 52, 26), initialised as test_whole_openpose_model_gradients does: its gradients in float64,
    through the emulation, on the per-conv bf16 path and with resident='dense' - computed once, left unchanged"""
    torch.manual_seed(0)
    base = openpose.OpenPose_Model(*TOPO)
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, nn.Conv2d):
                tb.he_init([m], int(torch.randint(1 << 30, (1,), generator=g)))
            elif isinstance(m, nn.PReLU):
                m.weight.copy_(torch.randn(m.weight.shape[0], generator=g) * 0.25)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 3, 32, 32, generator=g)
    heat, paf = torch.rand(1, TOPO[3], 4, 4, generator=g), torch.randn(1, TOPO[2], 4, 4, generator=g) * 0.5
    r = tb.three_ways(base, x, heat, paf, tb.openpose_forward, encode.get_loss_openpose, cuda, train)
    m = copy.deepcopy(base).to(cuda)
    reset(train)
    _, saved = train.forward_train(m, x.to(cuda), compute_dtype='bf16', resident='dense')
    total, _ = encode.get_loss_openpose(saved, heat.to(cuda), paf.to(cuda))
    r["dense"] = tb.grads_of(list(m.named_parameters()), total)
    r["dense_saved"] = [t.detach() for s in saved for t in s]
    r["dense_fallbacks"] = counters(train)
    return r


def test_whole_openpose_model_gradients_dense(net):
    g = net["dense"]
    assert len(g) == 227 and set(g) == set(net["ref64"]) == set(net["emul"])
    assert all(t.dtype == torch.float32 for t in g.values())
    tb.check_ratios("openpose_dense", g, net["emul"], net["ref64"], net["dense_fallbacks"])
    assert net["dense_fallbacks"] == NONE
    differ = {n: int((g[n] != net["native"][n]).sum()) for n in g}
    total = sum(t.numel() for t in g.values())
    stages = sum(d for n, d in differ.items() if not n.startswith("feature_extractor."))
    print("dense OpenPose_Model against the per-conv path: %d of %d gradient elements differ, %d of them in the stages "
          "(dense_stage), the rest in feature_extractor (conv_chain) %s"
          % (sum(differ.values()), total, stages, {n: d for n, d in differ.items() if d}))
    cd.note("train_dense_vs_per_conv_openpose.json", {"elements": total, "differ": sum(differ.values()), "in_stages": stages,
                                                      "parameters": {n: d for n, d in differ.items() if d}})


def test_dense_train_step_is_torch_sgd_on_the_nodes_gradients_and_inference_resyncs(net, openpose, cuda, train, encode):
    x, heat, paf = net["x"].to(cuda), net["heat"].to(cuda), net["paf"].to(cuda)
    a = copy.deepcopy(net["base"]).to(cuda)
    with torch.no_grad():
        before = [t.clone() for s in a(x)[1] for t in s]           # packs the inference arena from the initial parameters
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf, compute_dtype='bf16', resident='dense')
    assert total.dtype == torch.float32
    assert all(p.dtype == torch.float32 and p.grad.dtype == torch.float32 for p in a.parameters())
    b = copy.deepcopy(net["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = net["dense"][n].clone()
    opt_b.step()
    start = dict(net["base"].named_parameters())
    moved_slopes = 0
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
        if n.endswith("weight"):
            assert not torch.equal(pa.detach().cpu(), start[n].detach()), "%s did not move" % n
            moved_slopes += pa.dim() == 1
    assert moved_slopes == 3 + 4 * 16                               # every PReLU of the trunk and of the four stages
    # inference after the step: the plan reloads filters AND slopes from the updated parameters
    fresh = openpose.OpenPose_Model(*TOPO)
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda)
    with torch.no_grad():
        got, want = [t for s in a(x)[1] for t in s], [t for s in fresh(x)[1] for t in s]
    assert len(got) == 4 and all(torch.equal(s, t) for s, t in zip(got, want))
    assert any(not torch.equal(got[i], before[i]) for i in range(4))
    # a second dense step packs the stepped filters anew: the gradients are those of a fresh copy
    def grads(m):
        m.zero_grad(set_to_none=True)
        _, saved = train.forward_train(m, x, compute_dtype='bf16', resident='dense')
        encode.get_loss_openpose(saved, heat, paf)[0].backward()
        return {n: p.grad.clone() for n, p in m.named_parameters()}
    ga, gf = grads(a), grads(fresh)
    assert all(torch.equal(ga[n], gf[n]) for n in ga)
    assert any(not torch.equal(ga[n], net["dense"][n]) for n in ga)


def test_frozen_trunk_and_first_stage_leave_the_other_gradients_unchanged(net, cuda, train, encode):
    """freeze_trunk plus a frozen first stage: that stage's node walks down to its input only (the trunk's trainable convs
    below it still need the data gradient); every remaining gradient is the unfrozen run's, bit for bit"""
    m = train.freeze_trunk(copy.deepcopy(net["base"]).to(cuda))
    for p in m.l2_stages[0].parameters():
        p.requires_grad = False
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    reset(train)
    _, saved = train.forward_train(m, net["x"].to(cuda), compute_dtype='bf16', resident='dense')
    encode.get_loss_openpose(saved, net["heat"].to(cuda), net["paf"].to(cuda))[0].backward()
    assert counters(train) == NONE
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert len(frozen) == 18 + 16 * 3 + 2 and set(got) == set(net["dense"]) - frozen
    for n, t in got.items():
        assert torch.equal(t, net["dense"][n]), n
    for s, t in zip([t for s in saved for t in s], net["dense_saved"]):
        assert torch.equal(s, t)


# ---- the keyword and the refusals -----------------------------------------------------------------------------------------------------
def test_the_other_values_of_resident_are_what_they_were(net, cuda, train, encode):
    x, heat, paf = net["x"].to(cuda), net["heat"].to(cuda), net["paf"].to(cuda)
    for kw in ({}, {"resident": False}):
        m = copy.deepcopy(net["base"]).to(cuda)
        _, saved = train.forward_train(m, x, compute_dtype='bf16', **kw)
        encode.get_loss_openpose(saved, heat, paf)[0].backward()
        assert all(torch.equal(p.grad, net["native"][n]) for n, p in m.named_parameters())


def test_the_keyword_refuses_on_the_device(pkg, capi, cuda, train, openpose):
    hourglass = importlib.import_module(pkg.__name__ + ".hourglass")
    shufflenet = importlib.import_module(pkg.__name__ + ".shufflenet")
    x = torch.zeros(1, 3, 32, 32, device=cuda)
    for model, text in ((pkg.get_model('vgg19'), "no dense blocks and no PReLU"),
                        (hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3), "BatchNorm kernels"),
                        (shufflenet.Network(), "BatchNorm and depthwise kernels")):
        model = model.to(cuda).train()
        with pytest.raises(capi.RtposeError, match="resident='dense' is for an openpose.OpenPose_Model only.*" + text):
            train.forward_train(model, x, compute_dtype='bf16' if text.startswith("no dense") else 'fp32', resident='dense')
        with pytest.raises(capi.RtposeError, match="resident='dense' is for an openpose.OpenPose_Model only.*" + text):
            train.train_step(model, None, x, None, None, compute_dtype='bf16' if text.startswith("no dense") else 'fp32',
                             resident='dense')
    model = openpose.OpenPose_Model(*TOPO).to(cuda)
    with pytest.raises(capi.RtposeError, match="resident='dense' needs compute_dtype='bf16'.*fp32 node is not built"):
        train.forward_train(model, x, resident='dense')
    with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*two consumers"):
        train.forward_train(model, x, compute_dtype='bf16', resident=True)
    for wrong in ('Dense', 'chain', 2, None, 0.5):
        with pytest.raises(capi.RtposeError, match="resident is False, True or 'dense'"):
            train.forward_train(model, x, compute_dtype='bf16', resident=wrong)


def test_dense_stage_refuses_what_it_does_not_run(capi, cuda, train):
    x, layers, _ = random_operands(stage_shapes(), seed=1)
    x = x.to(cuda)
    layers = [tuple(None if t is None else t.to(cuda) for t in layer) for layer in layers]

    def swap(i, j, value):
        out = [list(layer) for layer in layers]
        out[i][j] = value
        return [tuple(layer) for layer in out]

    def z(*shape, **kw):
        return torch.zeros(*shape, device=cuda, **kw)

    for bad in (layers[:4], layers[:6], layers[:1], []):
        with pytest.raises(capi.RtposeError, match=r"3 B \+ 2 .* triples"):
            train.dense_stage(x, bad)
    with pytest.raises(capi.RtposeError, match="triples; got"):
        train.dense_stage(x, swap(0, 0, None))
    for i, wt in ((0, z(C, CIN, 1, 1)), (0, z(C, CIN + 1, 3, 3)), (1, z(C + 16, C, 3, 3)), (3, z(C, C, 3, 3)), (6, z(C6, 3 * C, 3, 3)),
                  (7, z(COUT, C6 + 1, 1, 1)), (2, z(C, C, 3, 3, dtype=torch.float64)), (4, z(C, C, 3))):
        with pytest.raises(capi.RtposeError, match="layer %d: fp32 OIHW filters" % i):
            train.dense_stage(x, swap(i, 0, wt))
    with pytest.raises(capi.RtposeError, match="layer 2 has a PReLU: its slope is missing"):
        train.dense_stage(x, swap(2, 2, None))
    with pytest.raises(capi.RtposeError, match=r"layer 7 \(Mconv7\) has no activation"):
        train.dense_stage(x, swap(7, 2, z(COUT)))
    for wrong in (z(C - 1), z(1), z(C, 1), z(C, dtype=torch.float64), 0.25, torch.zeros(C)):
        with pytest.raises(capi.RtposeError, match=r"layer 1: the slope is the fp32 \[16\] weight of an nn.PReLU"):
            train.dense_stage(x, swap(1, 2, wrong))
    with pytest.raises(capi.RtposeError, match="the bias is None or an fp32"):
        train.dense_stage(x, swap(1, 1, z(3)))
    with pytest.raises(capi.RtposeError, match="takes an NCHW fp32 input"):
        train.dense_stage(x.double(), layers)
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.dense_stage(x.cpu(), layers)
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.dense_stage(x, swap(3, 0, layers[3][0].cpu()))
    # a bias-free stage is fine
    y = train.dense_stage(x, [(wt, None, a) for wt, _, a in layers])
    assert y.shape == (N, COUT, H, W) and torch.isfinite(y).all()
