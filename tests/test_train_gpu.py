"""GPU suite of train.py: gradients of a small chain and of the whole rtpose_vgg through the library's kernels against the
same module tree run by torch on the CPU in float64.

For every parameter p, r(p) = max|g - g64| / max|g64|.  Required: r_native(p) <= 4 * max_q r_cpu32(q), r_cpu32 the same
quantity for torch's own fp32 CPU autograd on the same inputs - the yardstick is the reference arithmetic's own error, not
the code under test; the margin of 4 covers two equally precise fp32 paths that differ in summation order and in the few
ReLU decisions that fall on opposite sides of zero.  Both ratios per parameter are written through conv_driver.note
(profiles/r16_conv_backward.txt)."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_driver as cd

pytestmark = pytest.mark.gpu

MARGIN = 4.0


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


def ratios(grads, grads64):
    return {n: ((grads[n].double().cpu() - g64).abs().max() / g64.abs().max()).item() for n, g64 in grads64.items()}


def check_ratios(name, native, cpu32, grads64):
    rn, rc = ratios(native, grads64), ratios(cpu32, grads64)
    yard = max(rc.values())
    worst = max(rn, key=rn.get)
    print("%s: worst native ratio %.3g (%s), yardstick max r_cpu32 %.3g" % (name, rn[worst], worst, yard))
    cd.note("train_grad_ratios_%s.json" % name, {"yardstick_max_r_cpu32": yard,
                                                  "per_parameter": {n: {"native": rn[n], "cpu32": rc[n]} for n in rn}})
    bad = {n: r for n, r in rn.items() if not r <= MARGIN * yard}
    assert not bad, "r_native above %g x %.3g: %s" % (MARGIN, yard, bad)


def he_init(convs, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in convs:
            co, ci, k = m.weight.shape[0], m.weight.shape[1], m.weight.shape[2]
            m.weight.copy_(cd.weights("he", co, ci, k, g))
            m.bias.copy_(torch.randn(co, generator=g) * 0.1)


def grads_of(params, loss):
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in params if p.grad is not None}


# ---- (a) a small chain: conv3 + ReLU, pool, conv7 + ReLU, concat with the conv7's input, conv1 ---------------------------------
class Chain(nn.Module):
    def __init__(self):
        super().__init__()
        self.c3 = nn.Conv2d(8, 12, 3, 1, 1)
        self.c7 = nn.Conv2d(12, 10, 7, 1, 3)
        self.c1 = nn.Conv2d(22, 5, 1, 1, 0)
        he_init([self.c3, self.c7, self.c1], 5)

    def forward(self, x, conv):
        a = F.max_pool2d(conv(x, self.c3, True), 2, 2, 0)
        b = conv(a, self.c7, True)
        return conv(torch.cat([b, a], 1), self.c1, False)


def torch_conv(x, m, relu):
    y = F.conv2d(x, m.weight, m.bias, padding=m.padding)
    return F.relu(y) if relu else y


def test_small_chain_gradients(cuda, train):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 8, 12, 10, generator=g)
    target = torch.randn(2, 5, 6, 5, generator=g)
    base = Chain()
    out = {}
    for name, dt, dev in (("ref64", torch.float64, "cpu"), ("cpu32", torch.float32, "cpu"), ("native", torch.float32, cuda)):
        m = copy.deepcopy(base).to(device=dev, dtype=dt)
        xin = x.clone().to(device=dev, dtype=dt).requires_grad_(True)      # (a leaf of its own in every arithmetic)
        conv = (lambda t, mod, relu: train.conv2d(t, mod.weight, mod.bias, relu)) if name == "native" else torch_conv
        y = m(xin, conv)
        out[name] = grads_of(list(m.named_parameters()) + [("input", xin)], F.mse_loss(y, target.to(device=dev, dtype=dt)))
        out[name + "_y"] = y.detach().double().cpu()
    ref = {n: t.double() for n, t in out["ref64"].items()}
    assert set(out["native"]) == set(ref) and len(ref) == 7
    scale = max(1.0, out["ref64_y"].abs().max().item())
    assert (out["native_y"] - out["ref64_y"]).abs().max().item() <= cd.TOL * scale
    check_ratios("chain", out["native"], out["cpu32"], ref)


# ---- (b) the whole network at 1 x 3 x 32 x 32 (4 x 4 maps) -------------------------------------------------------------------
def torch_forward(model, x):
    """lib/network/rtpose_vgg.py:158-198 over the module tree, by torch"""
    out1 = model.model0(x)
    saved, feed = [], out1
    for s in range(1, 7):
        o1, o2 = getattr(model, 'model%d_1' % s)(feed), getattr(model, 'model%d_2' % s)(feed)
        saved += [o1, o2]
        feed = torch.cat([o1, o2, out1], 1)
    return saved


@pytest.fixture(scope="module")
def net(pkg, cuda, train, encode):
    """The model, its inputs, and the gradients of the 12-term loss three ways; computed once, left unchanged."""
    torch.manual_seed(0)
    base = pkg.get_model('vgg19')
    he_init([m for _, m in base._convs()], 23)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 3, 32, 32, generator=g)
    heat, paf = torch.rand(1, 19, 4, 4, generator=g), torch.randn(1, 38, 4, 4, generator=g) * 0.5
    r = dict(base=base, x=x, heat=heat, paf=paf)
    for name, dt in (("ref64", torch.float64), ("cpu32", torch.float32)):
        m = copy.deepcopy(base).to(dtype=dt)
        total, _ = encode.get_loss(torch_forward(m, x.to(dt)), heat.to(dt), paf.to(dt))
        r[name] = grads_of(list(m.named_parameters()), total)
    m = copy.deepcopy(base).to(cuda)
    _, saved = train.forward_train(m, x.to(cuda))
    total, log = encode.get_loss(saved, heat.to(cuda), paf.to(cuda))
    r["native"] = grads_of(list(m.named_parameters()), total)
    r["native_log"], r["native_model"] = log, m
    r["ref64"] = {n: t.double() for n, t in r["ref64"].items()}
    return r


def test_whole_network_gradients(net):
    assert len(net["native"]) == 184 and set(net["native"]) == set(net["ref64"])
    check_ratios("rtpose_vgg", net["native"], net["cpu32"], net["ref64"])


def test_training_losses_equal_the_inference_plan(net, cuda, encode):
    """the 12 terms of forward_train against get_loss on model(x), the inference plan of the same parameters"""
    m = net["native_model"]
    with torch.no_grad():
        _, saved = m(net["x"].to(cuda))
        _, log = encode.get_loss(saved, net["heat"].to(cuda), net["paf"].to(cuda))
    for name in encode.build_names():
        a, b = net["native_log"][name], log[name]
        assert abs(a - b) <= cd.TOL * max(1.0, abs(b)), (name, a, b)


def test_frozen_trunk_gets_no_gradient(net, cuda, train, encode):
    m = train.freeze_trunk(copy.deepcopy(net["base"]).to(cuda))
    _, saved = train.forward_train(m, net["x"].to(cuda))
    total, _ = encode.get_loss(saved, net["heat"].to(cuda), net["paf"].to(cuda))
    total.backward()
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert len(frozen) == 18 and all(p.grad is None for p in m.parameters() if not p.requires_grad)
    got = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    assert len(got) == 184 - 18
    keep = lambda d: {n: d[n] for n in got}     # noqa: E731
    check_ratios("rtpose_vgg_frozen_trunk", got, keep(net["cpu32"]), keep(net["ref64"]))
    # the gradients that remain are the very ones of the unfrozen run: the same launches on the same data
    for n, gr in got.items():
        assert torch.equal(gr, net["native"][n]), n


def test_train_step_is_torch_sgd_on_the_native_gradients_and_inference_resyncs(net, pkg, cuda, train, encode):
    x, heat, paf = net["x"].to(cuda), net["heat"].to(cuda), net["paf"].to(cuda)
    a = copy.deepcopy(net["base"]).to(cuda)
    with torch.no_grad():
        before = [t.clone() for t in a(x)[1]]            # packs the inference arena from the initial parameters
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf)
    assert total.item() == pytest.approx(sum(log[n] for n in encode.build_names()), rel=1e-5)
    assert {"max_ht", "min_ht", "max_paf", "min_paf"} <= set(log)
    # the same step applied by torch to the native gradients of the untouched parameters
    b = copy.deepcopy(net["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = net["native"][n].clone()
    opt_b.step()
    start = dict(net["base"].named_parameters())
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
        if n.endswith("weight"):
            assert not torch.equal(pa.detach().cpu(), start[n].detach()), "%s did not move" % n
    # inference after the step: the plan repacks from the updated parameters (weight-sync path)
    fresh = pkg.get_model('vgg19')
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda)
    with torch.no_grad():
        got, want = a(x)[1], fresh(x)[1]
    for i in range(12):
        assert torch.equal(got[i], want[i]), i
    assert any(not torch.equal(got[i], before[i]) for i in range(12))
