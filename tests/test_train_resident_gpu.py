"""GPU suite of layout-resident training: train.conv_chain - a run of convs as one autograd node whose inner activations and
gradients stay in the library's layouts - and the resident= keyword of run_sequential / forward_train / train_step.

The contract is the one of the per-conv bf16 path (tests/test_train_bf16_gpu.py), because no rounding point moves:
conv_backward_bf16_restate.EmulConv chained, and float64 on exact integer operands.

* Exact chains: three and four layers mixing k = 7, 3 and 1 (layer shapes of the existing bf16 suites: their acceptance by
  rtpose_conv2d_bf16 is known), N = 2 on 9 x 11 maps, integer operands so sparse that every activation and every gradient is
  an integer bf16 holds and every sum stays below 2^24 - asserted on the host: the emulation with its roundings equals the
  one without.  conv_chain's output and every gradient then torch.equal float64 AND the per-conv path, for both compute dtypes
  and five requires_grad subsets.
* Random chains, bf16: r_native <= 4 max r_emul (test_train_bf16_gpu.check_ratios); the number of elements that differ from
  the per-conv path is printed and noted, not asserted (the header says where the two may differ).
* Random chains, fp32: against torch's float64 autograd under test_train_gpu's rule (torch's fp32 CPU gradients the yardstick).
* The whole rtpose_vgg fixture of the bf16 suite with resident=True; one optimizer step; the keyword's default; the refusals."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_backward_bf16_restate as cb
import conv_backward_restate as cbr
import conv_driver as cd
import test_train_bf16_gpu as tb
import test_train_gpu as tg
from test_train_bf16_gpu import train, encode, openpose, vgg  # noqa: F401  (fixtures; vgg: the three_ways of the small network)

pytestmark = pytest.mark.gpu

N, H, W = 2, 9, 11

# every (k, cin, cout) the existing bf16 suites run
KNOWN = ({(s.k, s.cin, s.cout) for s in tb.RELU_SHAPES} | set(tb.LAYERS) | {(c.k, c.cin, c.cout) for c in cb.CASES}
         | {(c.k, c.cin, c.cout) for c in cb.EXACT_CASES})
CHAINS = {
    "k7_k3_k1": [(7, 8, 72), (3, 72, 8), (1, 8, 19)],
    "k3_k7_k3_k1": [(3, 9, 8), (7, 8, 72), (3, 72, 8), (1, 8, 19)],
}
for _shapes in CHAINS.values():
    assert all(s in KNOWN for s in _shapes) and all(a[2] == b[1] for a, b in zip(_shapes, _shapes[1:]))
assert {s[0] for v in CHAINS.values() for s in v} == {1, 3, 7}

SUBSETS = ("all", "x_only", "last_layer_only", "first_layer_frozen", "x_not_required")


def required(subset, nlayers):
    """(x requires a gradient, per layer: its parameters do)"""
    return {"all": (True, [True] * nlayers),
            "x_only": (True, [False] * nlayers),
            "last_layer_only": (False, [False] * (nlayers - 1) + [True]),
            "first_layer_frozen": (True, [False] + [True] * (nlayers - 1)),
            "x_not_required": (False, [True] * nlayers)}[subset]


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def exact_operands(shapes, relu_last, seed):
    """x in {0, 1}; per output channel two filter taps of +-1 and a bias in {0, 1}: |y_i| <= 2 |y_(i-1)| + 1; the top gradient
    in {-1, 0, 1}, two thirds of it zero.  (x, [(w, b, relu)], G)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 2, (N, shapes[0][1], H, W), generator=g).float()
    layers = []
    for i, (k, cin, cout) in enumerate(shapes):
        wt = torch.zeros(cout, cin * k * k)
        for o in range(cout):
            at = torch.randperm(cin * k * k, generator=g)[:2]
            wt[o, at] = torch.tensor([1.0, 1.0 if o % 3 else -1.0])
        b = torch.randint(0, 2, (cout,), generator=g).float()
        layers.append((wt.view(cout, cin, k, k), b, relu_last or i + 1 < len(shapes)))
    G = torch.randint(-1, 2, (N, shapes[-1][2], H, W), generator=g).float() * (torch.rand(N, shapes[-1][2], H, W, generator=g) < 0.5)
    return x, layers, G


def random_operands(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, shapes[0][1], H, W, generator=g)
    layers = [(cd.weights("he", cout, cin, k, g), torch.randn(cout, generator=g) * 0.1, i + 1 < len(shapes))
              for i, (k, cin, cout) in enumerate(shapes)]
    target = torch.randn(N, shapes[-1][2], H, W, generator=g)
    return x, layers, target


def host_chain(x, layers, conv, dt, top):
    """the chain on the CPU in dtype dt with conv(x, w, b, relu); every tensor requires a gradient.  top(y) -> the scalar
    loss.  (y, {name: gradient}, [inputs of the layers and y]: the activations as the next layer reads them)"""
    xin = x.clone().to(dt).requires_grad_(True)
    params = [(wt.clone().to(dt).requires_grad_(True), b.clone().to(dt).requires_grad_(True)) for wt, b, _ in layers]
    acts, t = [xin], xin
    for (wt, b), (_, _, relu) in zip(params, layers):
        t = conv(t, wt, b, relu)
        acts.append(t)
    top(t).backward()
    grads = {"x": xin.grad}
    for i, (wt, b) in enumerate(params):
        grads["w%d" % i], grads["b%d" % i] = wt.grad, b.grad
    return t.detach(), grads, [a.detach() for a in acts]


def torch_conv(x, wt, b, relu):
    y = F.conv2d(x, wt, b, padding=wt.shape[2] // 2)
    return F.relu(y) if relu else y


def device_chain(train, cuda, x, layers, top, dt, form, subset="all"):
    """form 'chain': train.conv_chain; 'per_conv' / 'sequential_resident': train.run_sequential on the same modules"""
    need_x, need_p = required(subset, len(layers))
    xin = x.clone().to(cuda).requires_grad_(need_x)
    params = [(wt.clone().to(cuda).requires_grad_(need), b.clone().to(cuda).requires_grad_(need))
              for (wt, b, _), need in zip(layers, need_p)]
    if form == "chain":
        y = train.conv_chain(xin, [(wt, b, relu) for (wt, b), (_, _, relu) in zip(params, layers)], compute_dtype=dt)
    else:
        mods = []
        for (wt, b), (_, _, relu) in zip(params, layers):
            m = nn.Conv2d(wt.shape[1], wt.shape[0], wt.shape[2], 1, wt.shape[2] // 2).to(cuda)
            m.weight, m.bias = nn.Parameter(wt, requires_grad=wt.requires_grad), nn.Parameter(b, requires_grad=b.requires_grad)
            mods += [m, nn.ReLU()] if relu else [m]
        y = train.run_sequential(nn.Sequential(*mods), xin, compute_dtype=dt, resident=form == "sequential_resident")
        params = [(m.weight, m.bias) for m in mods if isinstance(m, nn.Conv2d)]
    top(y).backward()
    grads = {"x": xin.grad}
    for i, (wt, b) in enumerate(params):
        grads["w%d" % i], grads["b%d" % i] = wt.grad, b.grad
    return y.detach(), grads


def no_activation_bf16_flushes(acts):
    """the one place the two forms may differ: an activation 0 < y <= 2^-134, which bf16 rounds to +0"""
    return all(not ((a > 0) & (a <= 2.0 ** -134)).any() for a in acts)


# ---- exact chains -----------------------------------------------------------------------------------------------------------------------
_exact = {}


def exact_case(name, relu_last):
    """operands and the float64 reference of an exact chain, computed once and left unchanged; the host-side conditions"""
    key = (name, relu_last)
    if key in _exact:
        return _exact[key]
    shapes = CHAINS[name]
    x, layers, G = exact_operands(shapes, relu_last, seed=len(shapes) + 10 * relu_last)
    top = lambda y: (y * G.to(device=y.device, dtype=y.dtype)).sum()     # noqa: E731
    y_r, g_r, a_r = host_chain(x, layers, lambda t, wt, b, r: cb.emul_conv(t, wt, b, r, rounding=True), torch.float64, top)
    y_u, g_u, a_u = host_chain(x, layers, lambda t, wt, b, r: cb.emul_conv(t, wt, b, r, rounding=False), torch.float64, top)
    y64, g64, _ = host_chain(x, layers, torch_conv, torch.float64, top)
    # every rounding of the bf16 step is the identity on these operands, and the unrounded emulation is torch's autograd
    assert torch.equal(y_r, y_u) and torch.equal(y_u, y64)
    assert set(g_r) == set(g_u) == set(g64) and len(g64) == 1 + 2 * len(shapes)
    for n in g64:
        assert torch.equal(g_r[n], g_u[n]) and torch.equal(g_u[n], g64[n]), n
        assert g64[n].abs().max().item() > 0, "%s: the gradient is all zero" % n
    for a in a_u:
        assert torch.equal(a, a.round()) and a.abs().max().item() <= 256, "an activation bf16 does not hold"
        assert a.abs().max().item() > 0
    assert all((a > 0).any() and (a == 0).any() for a, (_, _, relu) in zip(a_u[1:], layers) if relu), "a ReLU decides nothing"
    assert no_activation_bf16_flushes(a_u)
    # every sum of absolute terms below 2^24: forward, data, weight and bias gradients of every layer
    g = G.double()
    worst = 0.0
    for i in range(len(layers) - 1, -1, -1):
        wt, b, relu = layers[i]
        if relu:
            g = g * (a_u[i + 1] > 0)
        assert torch.equal(g, cb.rb(g.float()).double()), "a gradient bf16 does not hold"
        k = wt.shape[2]
        dx, s_dx = cbr.dgrad64(g, wt)
        worst = max(worst, s_dx.max().item(), cbr.wgrad64(a_u[i], g, k)[1].max().item(), cbr.dbias64(g)[1].max().item(),
                    F.conv2d(a_u[i].abs(), wt.double().abs(), b.double().abs(), padding=k // 2).max().item())
        g = dx
    assert torch.equal(g, g64["x"]) and worst < 2 ** 24
    _exact[key] = (x, layers, top, y64, g64)
    return _exact[key]


def same_bits(what, y, g, y_want, g_want, subset, nlayers):
    need_x, need_p = required(subset, nlayers)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y_want.double().cpu()), what + ": y"
    for n, want in g_want.items():
        needed = need_x if n == "x" else need_p[int(n[1:])]
        if not needed:
            assert g[n] is None, (what, n)
            continue
        assert g[n] is not None and g[n].dtype == torch.float32 and g[n].shape == want.shape, (what, n)
        wrong = int((g[n].double().cpu() != want.double().cpu()).sum())
        assert wrong == 0, "%s: d%s: %d of %d elements differ" % (what, n, wrong, want.numel())


@pytest.mark.parametrize("subset", SUBSETS)
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_exact_chains_equal_float64_and_the_per_conv_path(cuda, train, name, dt, subset):
    x, layers, top, y64, g64 = exact_case(name, relu_last=False)
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()
    y, g = device_chain(train, cuda, x, layers, top, dt, "chain", subset)
    same_bits("conv_chain against float64", y, g, y64, g64, subset, len(layers))
    yp, gp = device_chain(train, cuda, x, layers, top, dt, "per_conv", subset)
    same_bits("conv_chain against the per-conv path", y, g, yp, {n: t for n, t in gp.items() if t is not None}, subset,
              len(layers))
    assert train.bf16_fallbacks == {'fwd': 0, 'dgrad': 0} and train.chain_fallbacks == 0


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_exact_chain_with_a_relu_behind_its_last_conv_through_run_sequential(cuda, train, dt):
    """a run as model0 has them (every conv with a ReLU), handed over by run_sequential(resident=True)"""
    x, layers, top, y64, g64 = exact_case("k7_k3_k1", relu_last=True)
    train.reset_chain_fallbacks()
    for form in ("chain", "sequential_resident"):
        y, g = device_chain(train, cuda, x, layers, top, dt, form)
        same_bits(form + " against float64", y, g, y64, g64, "all", len(layers))
    assert train.chain_fallbacks == 0


def test_refused_convs_fall_back_and_are_counted(cuda, train, monkeypatch):
    """rtpose_conv2d_bf16 refuses none of the shapes at hand, so the refusal is played here: train._conv_into answers False
    (what it answers when the launcher returns RTPOSE_E_INVAL before launching) for chosen bf16 launches.  A refused forward
    conv: the chain runs layer by layer through conv2d and chain_fallbacks counts it.  Refused data gradients: each runs in
    fp32 on the widened gradient, is rounded at the store and counted in bf16_fallbacks['dgrad'].  On exact operands both
    still give float64's values."""
    x, layers, top, y64, g64 = exact_case("k3_k7_k3_k1", relu_last=False)
    real, calls = train._conv_into, []

    def refuse(which):
        def conv_into(bf16, *a, **kw):
            calls.append(bf16)
            return False if bf16 and which(len(calls)) else real(bf16, *a, **kw)
        return conv_into

    for which, want_chain, want_dgrad in ((lambda i: i == 2, 1, 0),                 # the second forward conv
                                          (lambda i: i > len(layers), 0, len(layers))):     # every data gradient
        del calls[:]
        monkeypatch.setattr(train, "_conv_into", refuse(which))
        train.reset_bf16_fallbacks()
        train.reset_chain_fallbacks()
        y, g = device_chain(train, cuda, x, layers, top, "bf16", "chain")
        monkeypatch.setattr(train, "_conv_into", real)
        assert train.chain_fallbacks == want_chain and train.bf16_fallbacks == {'fwd': 0, 'dgrad': want_dgrad}
        assert len(calls) == (2 if want_chain else 2 * len(layers)) and all(calls)
        same_bits("after the fallback, against float64", y, g, y64, g64, "all", len(layers))
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()


# ---- random chains ------------------------------------------------------------------------------------------------------------------------
def named(g):
    return {n: t for n, t in g.items() if t is not None}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_random_chains_bf16_against_the_chained_emulation(cuda, train, name):
    shapes = CHAINS[name]
    x, layers, target = random_operands(shapes, seed=40 + len(shapes))
    top = lambda y: F.mse_loss(y, target.to(device=y.device, dtype=y.dtype))      # noqa: E731
    _, g64, _ = host_chain(x, layers, torch_conv, torch.float64, top)
    _, ge, acts = host_chain(x, layers, lambda t, wt, b, r: cb.emul_conv(t, wt, b, r), torch.float64, top)
    assert no_activation_bf16_flushes(acts)
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()
    y, g = device_chain(train, cuda, x, layers, top, "bf16", "chain")
    fallbacks = dict(train.bf16_fallbacks, chain=train.chain_fallbacks)
    assert all(t.dtype == torch.float32 for t in g.values()) and set(g) == set(g64)
    tb.check_ratios("resident_" + name, named(g), ge, g64, fallbacks)
    assert fallbacks == {'fwd': 0, 'dgrad': 0, 'chain': 0}
    # against the per-conv path: counted, not asserted (another kernel instance may sum in another order)
    yp, gp = device_chain(train, cuda, x, layers, top, "bf16", "per_conv")
    differ = {n: int((g[n] != gp[n]).sum()) for n in g}
    differ["y"] = int((y != yp).sum())
    total = sum(t.numel() for t in g.values()) + y.numel()
    print("resident %s against the per-conv path: %d of %d elements differ %s" % (name, sum(differ.values()), total, differ))
    cd.note("train_resident_vs_per_conv_%s.json" % name, {"elements": total, "differ": differ})


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_random_chains_fp32_against_float64_autograd(cuda, train, name):
    shapes = CHAINS[name]
    x, layers, target = random_operands(shapes, seed=60 + len(shapes))
    top = lambda y: F.mse_loss(y, target.to(device=y.device, dtype=y.dtype))      # noqa: E731
    y64, g64, _ = host_chain(x, layers, torch_conv, torch.float64, top)
    _, g32, _ = host_chain(x, layers, torch_conv, torch.float32, top)
    y, g = device_chain(train, cuda, x, layers, top, "fp32", "chain")
    assert (y.double().cpu() - y64).abs().max().item() <= cd.TOL * max(1.0, y64.abs().max().item())
    tg.check_ratios("resident_" + name, named(g), g32, g64)


# ---- the whole network ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resident(vgg, cuda, train, encode):
    """the gradients of the small rtpose_vgg with resident=True, bf16: computed once, left unchanged"""
    m = copy.deepcopy(vgg["base"]).to(cuda)
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()
    _, saved = train.forward_train(m, vgg["x"].to(cuda), compute_dtype='bf16', resident=True)
    total, _ = encode.get_loss(saved, vgg["heat"].to(cuda), vgg["paf"].to(cuda))
    grads = tb.grads_of(list(m.named_parameters()), total)
    return {"grads": grads, "saved": [t.detach() for t in saved],
            "fallbacks": dict(train.bf16_fallbacks, chain=train.chain_fallbacks)}


def test_whole_rtpose_vgg_gradients_resident(vgg, resident):
    g = resident["grads"]
    assert len(g) == 184 and set(g) == set(vgg["ref64"]) == set(vgg["emul"])
    assert all(t.dtype == torch.float32 for t in g.values())
    tb.check_ratios("rtpose_vgg_resident", g, vgg["emul"], vgg["ref64"], resident["fallbacks"])
    assert resident["fallbacks"] == {'fwd': 0, 'dgrad': 0, 'chain': 0}
    differ = sum(int((g[n] != vgg["native"][n]).sum()) for n in g)
    total = sum(t.numel() for t in g.values())
    print("resident rtpose_vgg against the per-conv path: %d of %d gradient elements differ" % (differ, total))
    cd.note("train_resident_vs_per_conv_rtpose_vgg.json", {"elements": total, "differ": differ})


def test_resident_train_step_is_torch_sgd_on_the_chains_gradients_and_inference_resyncs(vgg, resident, pkg, cuda, train, encode):
    x, heat, paf = vgg["x"].to(cuda), vgg["heat"].to(cuda), vgg["paf"].to(cuda)
    a = copy.deepcopy(vgg["base"]).to(cuda)
    with torch.no_grad():
        before = [t.clone() for t in a(x)[1]]            # packs the inference arena from the initial parameters
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf, compute_dtype='bf16', resident=True)
    assert total.dtype == torch.float32
    assert total.item() == pytest.approx(sum(log[n] for n in encode.build_names()), rel=1e-5)
    assert all(p.dtype == torch.float32 and p.grad.dtype == torch.float32 for p in a.parameters())
    # the same step applied by torch to the chain's own gradients of the untouched parameters
    b = copy.deepcopy(vgg["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = resident["grads"][n].clone()
    opt_b.step()
    start = dict(vgg["base"].named_parameters())
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
        if n.endswith("weight"):
            assert not torch.equal(pa.detach().cpu(), start[n].detach()), "%s did not move" % n
    # inference after the step: the plan repacks from the updated parameters
    fresh = pkg.get_model('vgg19')
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda)
    with torch.no_grad():
        got, want = a(x)[1], fresh(x)[1]
    for i in range(12):
        assert torch.equal(got[i], want[i]), i
    assert any(not torch.equal(got[i], before[i]) for i in range(12))
    # a second resident step packs the stepped filters anew: the gradients are those of a fresh copy
    def grads(m):
        m.zero_grad(set_to_none=True)
        _, saved = train.forward_train(m, x, compute_dtype='bf16', resident=True)
        encode.get_loss(saved, heat, paf)[0].backward()
        return {n: p.grad.clone() for n, p in m.named_parameters()}
    ga, gf = grads(a), grads(fresh)
    assert all(torch.equal(ga[n], gf[n]) for n in ga)
    assert any(not torch.equal(ga[n], resident["grads"][n]) for n in ga)


def test_frozen_trunk_stops_the_walk(vgg, resident, cuda, train, encode):
    """freeze_trunk: the chains of the frozen convs launch no backward, the first trainable run no data gradient below its
    lowest trainable layer; every other gradient is the unfrozen run's, bit for bit"""
    m = train.freeze_trunk(copy.deepcopy(vgg["base"]).to(cuda))
    _, saved = train.forward_train(m, vgg["x"].to(cuda), compute_dtype='bf16', resident=True)
    encode.get_loss(saved, vgg["heat"].to(cuda), vgg["paf"].to(cuda))[0].backward()
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert len(got) == 184 - 18 and all(p.grad is None for p in m.parameters() if not p.requires_grad)
    for n, t in got.items():
        assert torch.equal(t, resident["grads"][n]), n


# ---- the keyword and the refusals -----------------------------------------------------------------------------------------------------
def test_resident_false_is_the_call_without_the_keyword(vgg, cuda, train, encode):
    x, layers, target = random_operands(CHAINS["k7_k3_k1"], seed=3)
    mods = []
    for wt, b, relu in layers:
        m = nn.Conv2d(wt.shape[1], wt.shape[0], wt.shape[2], 1, wt.shape[2] // 2)
        with torch.no_grad():
            m.weight.copy_(wt)
            m.bias.copy_(b)
        mods += [m, nn.ReLU()] if relu else [m]
    seq = nn.Sequential(*mods).to(cuda)
    got = []
    for kw in ({}, {"resident": False}):
        for dt in ("fp32", "bf16"):
            seq.zero_grad(set_to_none=True)
            xin = x.clone().to(cuda).requires_grad_(True)
            y = train.run_sequential(seq, xin, compute_dtype=dt, **kw)
            F.mse_loss(y, target.to(cuda)).backward()
            got.append([y.detach(), xin.grad] + [p.grad.clone() for p in seq.parameters()])
    for a, b in ((got[0], got[2]), (got[1], got[3])):
        assert len(a) == 8 and all(torch.equal(s, t) for s, t in zip(a, b))
    xd, heat, paf = vgg["x"].to(cuda), vgg["heat"].to(cuda), vgg["paf"].to(cuda)
    outs = []
    for kw in ({}, {"resident": False}):
        m = copy.deepcopy(vgg["base"]).to(cuda)
        _, saved = train.forward_train(m, xd, compute_dtype='bf16', **kw)
        encode.get_loss(saved, heat, paf)[0].backward()
        outs.append(([t.detach() for t in saved], {n: p.grad for n, p in m.named_parameters()}))
    assert all(torch.equal(s, t) for s, t in zip(outs[0][0], outs[1][0]))
    assert all(torch.equal(outs[0][1][n], outs[1][1][n]) and torch.equal(outs[0][1][n], vgg["native"][n]) for n in outs[0][1])


def test_resident_is_refused_for_the_other_three_networks(pkg, capi, cuda, train, openpose):
    hourglass = importlib.import_module(pkg.__name__ + ".hourglass")
    shufflenet = importlib.import_module(pkg.__name__ + ".shufflenet")
    x = torch.zeros(1, 3, 32, 32, device=cuda)
    for model, texts in ((openpose.OpenPose_Model(*tb.TOPO), ("PReLU needs the fp32 pre-activation", "two consumers")),
                         (hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3), ("BatchNorm kernels",)),
                         (shufflenet.Network(), ("BatchNorm and depthwise kernels",))):
        model = model.to(cuda).train()
        for text in texts:
            with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*" + text):
                train.forward_train(model, x, resident=True)
            with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*" + text):
                train.train_step(model, None, x, None, None, resident=True)


def test_conv_chain_refuses_what_it_does_not_run(capi, cuda, train):
    x = torch.zeros(1, 8, 4, 4, device=cuda)
    w1, w2 = torch.zeros(16, 8, 3, 3, device=cuda), torch.zeros(4, 12, 1, 1, device=cuda)
    with pytest.raises(capi.RtposeError, match="input channels are the output channels of the layer before"):
        train.conv_chain(x, [(w1, None, True), (w2, None, False)])
    with pytest.raises(capi.RtposeError, match=r"k in \{1, 3, 7\}"):
        train.conv_chain(x, [(torch.zeros(16, 8, 5, 5, device=cuda), None, True)])
    with pytest.raises(capi.RtposeError, match="no layers"):
        train.conv_chain(x, [])
    with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
        train.conv_chain(x, [(w1, None, True)], compute_dtype='fp16')
    with pytest.raises(capi.RtposeError, match="the bias is None or an fp32"):
        train.conv_chain(x, [(w1, torch.zeros(3, device=cuda), True)])
