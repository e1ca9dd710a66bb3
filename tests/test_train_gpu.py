"""GPU suite of train.py: gradients of a small chain and of the whole rtpose_vgg through the library's kernels against the
same module tree run by torch on the CPU in float64.

For every parameter p, r(p) = max|g - g64| / max|g64|.  Required: r_native(p) <= 4 * max_q r_cpu32(q), r_cpu32 the same
quantity for torch's own fp32 CPU autograd on the same inputs - the yardstick is the reference arithmetic's own error, not
the code under test; the margin of 4 covers two equally precise fp32 paths that differ in summation order and in the few
ReLU decisions that fall on opposite sides of zero.  Both ratios per parameter are written through conv_driver.note
(profiles/r16_conv_backward.txt).

Those ratios judge a gradient against its tensor's maximum; a single wrong tap hides in them.  test_conv2d_function_exact
runs train.conv2d on the integer operands of conv_backward_restate.exact_tensors, where fp32 arithmetic in any order is
exact, and compares with F.conv2d (+ F.relu) in float64 by torch.equal; the tests behind it hold the packed-filter cache of
train.py to the contract of _native_state.py (a second step, copy_, load_state_dict, .data edits announced by
invalidate_weights(), always_resync) by torch.equal against a model whose parameters are new objects."""
import collections
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_backward_restate as cb
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
    r["native_log"], r["native_model"], r["native_total"] = log, m, total.detach().clone()
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


# ---- (c) train.conv2d on exact integer operands ------------------------------------------------------------------------------------
Spec = collections.namedtuple("Spec", "k cin cout n h w relu bias req variant")
KS, CHANNELS, SHAPES = (1, 3, 7), ((3, 5), (9, 8), (70, 66)), ((1, 1, 1), (2, 5, 3), (3, 19, 18))
SUBSETS = ("x", "w", "b", "xw", "xb", "wb", "xwb")          # which of input, weight, bias require a gradient
VARIANTS = ("x_slice", "x_channels_last", "gy_transposed", "gy_expanded", "two_branches", "shared_weight", "backward_twice",
            "side_stream")


def _specs():
    out = []
    for relu in (0, 1):
        for i, req in enumerate(SUBSETS):
            ci, co = CHANNELS[(i + relu) % 3]
            # a conv without a bias has no bias gradient to ask for: the subsets without "b" alternate
            out.append(Spec(KS[(i + 2 * relu) % 3], ci, co, *SHAPES[(i + i // 3 + relu) % 3], relu, "b" in req or i == 3, req, None))
    for i, v in enumerate(VARIANTS):
        ci, co = CHANNELS[i % 3]
        out.append(Spec(KS[(i + 1) % 3], ci, co, *SHAPES[1 + i % 2], i % 2, True, "xwb", v))
    out.append(Spec(7, 70, 66, 3, 19, 18, 1, True, "xwb", None))        # the largest
    out.append(Spec(1, 9, 8, 3, 19, 18, 0, False, "xw", None))          # several slabs (k = 1, 1026 pixels), no bias
    return out


SPECS = _specs()
for _relu in (0, 1):        # every value of every axis with the ReLU and without
    _mine = [s for s in SPECS if s.relu == _relu]
    assert {s.k for s in _mine} == set(KS) and {(s.cin, s.cout) for s in _mine} == set(CHANNELS)
    assert {(s.n, s.h, s.w) for s in _mine} == set(SHAPES) and {s.bias for s in _mine} == {True, False}
    assert {s.req for s in _mine} == set(SUBSETS)
assert {s.variant for s in SPECS} == set(VARIANTS) | {None}


def spec_id(s):
    return "k%d_%dto%d_%dx%dx%d_%s%s_%s%s" % (s.k, s.cin, s.cout, s.n, s.h, s.w, "relu" if s.relu else "lin",
                                              "" if s.bias else "_nobias", s.req, "_" + s.variant if s.variant else "")


def exact_run(s, conv, dev, dt):
    """The spec's graph in `dt` arithmetic on `dev`: (y, {name: gradient or None for every leaf that exists})."""
    x, G, wt, b = (t.to(device=dev, dtype=dt) for t in cb.exact_tensors(s, seed=s.k + s.cin + 1))
    leaves = {}
    if s.variant == "x_slice":              # the conv's input is a channel slice of a wider leaf
        wide = torch.cat([x[:, :2] + 1, x, x[:, :1] + 2], 1).requires_grad_("x" in s.req)
        leaves["x"], xin = wide, wide[:, 2:2 + s.cin]
    elif s.variant == "x_channels_last":
        leaves["x"] = xin = x.contiguous(memory_format=torch.channels_last).requires_grad_("x" in s.req)
    else:
        leaves["x"] = xin = x.requires_grad_("x" in s.req)
    assert s.variant not in ("x_slice", "x_channels_last") or not xin.is_contiguous()
    leaves["w"] = wt.requires_grad_("w" in s.req)
    if s.bias:
        leaves["b"] = b.requires_grad_("b" in s.req)
    y = conv(xin, leaves["w"], leaves.get("b"), bool(s.relu))
    if s.variant == "gy_transposed":        # the gradient arrives as a transposed view of a contiguous [n, c, w, h] tensor
        loss = (y.transpose(2, 3) * G.transpose(2, 3).contiguous()).sum()
    elif s.variant == "gy_expanded":        # ... as an expanded scalar
        loss = y.sum()
    elif s.variant == "two_branches":       # y feeds two consumers: their gradients are added in front of the conv
        loss = (y * G).sum() + (F.max_pool2d(y, 1, 1) * (2 * G.flip(0))).sum()
    elif s.variant == "shared_weight":      # one filter bank, two convs in one graph: dw, db (and dx) accumulate
        y2 = conv(xin.flip(3), leaves["w"], leaves.get("b"), bool(s.relu))
        loss = (y * G).sum() + (y2 * G.flip(2)).sum()
    else:
        loss = (y * G).sum()
    if s.variant == "backward_twice":       # .grad doubles
        loss.backward(retain_graph=True)
    loss.backward()
    return y.detach(), {n: t.grad for n, t in leaves.items()}


@pytest.mark.parametrize("s", SPECS, ids=spec_id)
def test_conv2d_function_exact(cuda, train, s):
    assert 4 * cb.exact_margin(s, seed=s.k + s.cin + 1) < 2 ** 24       # two accumulated gradients, doubled, stay exact
    y64, g64 = exact_run(s, lambda x, w, b, relu: (F.relu if relu else (lambda t: t))(F.conv2d(x, w, b, padding=s.k // 2)),
                         "cpu", torch.float64)
    if s.variant == "side_stream":
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            y, g = exact_run(s, train.conv2d, cuda, torch.float32)
        side.synchronize()
    else:
        y, g = exact_run(s, train.conv2d, cuda, torch.float32)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y64), "y"
    assert set(g) == set(g64) == ({"x", "w", "b"} if s.bias else {"x", "w"})
    for n in g:
        if n[0] in s.req:
            assert g64[n] is not None and g[n] is not None, n
            assert g[n].dtype == torch.float32 and g[n].shape == g64[n].shape
            wrong = int((g[n].double().cpu() != g64[n]).sum())
            assert torch.equal(g[n].double().cpu(), g64[n]), "d%s: %d of %d elements differ" % (n, wrong, g64[n].numel())
            assert g64[n].abs().max().item() > 0
        else:
            assert g[n] is None and g64[n] is None, n


# ---- (d) the packed-filter cache of train.py ---------------------------------------------------------------------------------------
def chain_grads(m, conv, x, target):
    m.zero_grad(set_to_none=True)
    F.mse_loss(m(x, conv), target).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def test_second_step_uses_the_updated_filters(cuda, train):
    """After every way of changing the parameters in place, the native gradients equal those of a deep copy: new Parameters,
    so new cache entries, packed from the values of now.  c3's gradients come through the data gradients of c7 and c1."""
    g = torch.Generator().manual_seed(31)
    x, target = torch.randn(2, 8, 12, 10, generator=g).to(cuda), torch.randn(2, 5, 6, 5, generator=g).to(cuda)
    conv = lambda t, mod, relu: train.conv2d(t, mod.weight, mod.bias, relu)   # noqa: E731
    m = Chain().to(cuda)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    last = chain_grads(m, conv, x, target)
    opt.step()

    def changed_and_current(what):
        nonlocal last
        got, want = chain_grads(m, conv, x, target), chain_grads(copy.deepcopy(m), conv, x, target)
        assert len(got) == 6
        for n in got:
            assert torch.equal(got[n], want[n]), "%s: %s is not the gradient at the current parameters" % (what, n)
            assert not torch.equal(got[n], last[n]), "%s: %s did not change" % (what, n)
        last = got
    changed_and_current("optimizer.step()")
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p * 0.5 + 0.01)
    changed_and_current("copy_")
    other = Chain()
    he_init([other.c3, other.c7, other.c1], 6)
    m.load_state_dict(other.state_dict())
    changed_and_current("load_state_dict")


def training_run(m, net, cuda, train, encode):
    """(total, log, {name: gradient}) of one forward_train + get_loss + backward of the fixture's inputs"""
    m.zero_grad(set_to_none=True)
    _, saved = train.forward_train(m, net["x"].to(cuda))
    total, log = encode.get_loss(saved, net["heat"].to(cuda), net["paf"].to(cuda))
    total.backward()
    return total.detach(), log, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def edit_through_data(m):
    """edits that bump no _version: the first trainable conv's weight, the last conv's bias, and a stage conv whose flipped
    packing the data gradient uses"""
    convs = [mod for _, mod in m._convs()]
    versions = [p._version for p in m.parameters()]
    m.model0[0].weight.data.mul_(0.5)
    convs[-1].bias.data.add_(0.25)
    m.model1_1[0].weight.data.mul_(-0.75)
    assert versions == [p._version for p in m.parameters()]


def same_as_fresh(m, net, pkg, cuda, train, encode, what):
    fresh = pkg.get_model('vgg19')
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(cuda)
    total, log, grads = training_run(m, net, cuda, train, encode)
    total_f, log_f, grads_f = training_run(fresh, net, cuda, train, encode)
    assert torch.equal(total, total_f), (what, total.item(), total_f.item())
    for name in encode.build_names():
        assert log[name] == log_f[name], (what, name, log[name], log_f[name])
    assert len(grads) == 184 and set(grads) == set(grads_f)
    for n in grads:
        assert torch.equal(grads[n], grads_f[n]), (what, n)
    assert not torch.equal(total, net["native_total"]), what + ": the edit changed nothing"
    return log


def test_invalidate_weights_reaches_training(net, pkg, cuda, train, encode):
    """_native_state.py's contract for .data edits holds for forward_train as for the inference plan"""
    m = copy.deepcopy(net["base"]).to(cuda)
    total, _, _ = training_run(m, net, cuda, train, encode)          # packs forward and flipped filters
    assert torch.equal(total, net["native_total"])
    edit_through_data(m)
    m.invalidate_weights()
    log = same_as_fresh(m, net, pkg, cuda, train, encode, "invalidate_weights()")
    with torch.no_grad():                                            # training and inference agree on the same module
        _, saved = m(net["x"].to(cuda))
        _, log_inf = encode.get_loss(saved, net["heat"].to(cuda), net["paf"].to(cuda))
    for name in encode.build_names():
        a, b = log[name], log_inf[name]
        assert abs(a - b) <= cd.TOL * max(1.0, abs(b)), (name, a, b)
    # always_resync: the edit is seen without the call
    m = copy.deepcopy(net["base"]).to(cuda)
    m.always_resync = True
    training_run(m, net, cuda, train, encode)
    edit_through_data(m)
    same_as_fresh(m, net, pkg, cuda, train, encode, "always_resync")


def test_dropping_the_packed_filters_reaches_a_bare_conv2d(cuda, train):
    """train.drop_packed_filters() is invalidate_weights() for callers of conv2d that own no model"""
    x, gy, wt, b = (t.to(cuda) for t in cb.exact_tensors(cb.Case(3, 9, 8, 2, 5, 3, 0, 0, "")))
    w = wt.clone().requires_grad_(True)
    xin = x.clone().requires_grad_(True)

    def run():
        w.grad = xin.grad = None
        y = train.conv2d(xin, w, b, False)
        (y * gy).sum().backward()
        return y.detach().clone(), xin.grad.clone()
    y1, dx1 = run()
    w.data.mul_(2)
    train.drop_packed_filters(w)
    y2, dx2 = run()
    assert torch.equal(dx2, 2 * dx1) and torch.equal(y2 - b.view(1, -1, 1, 1), 2 * (y1 - b.view(1, -1, 1, 1)))
    w.data.mul_(2)
    train.drop_packed_filters()
    y3, dx3 = run()
    assert torch.equal(dx3, 4 * dx1) and torch.equal(y3 - b.view(1, -1, 1, 1), 4 * (y1 - b.view(1, -1, 1, 1)))
    assert dx1.abs().max().item() > 0


def test_unfreezing_the_trunk_restores_its_gradients(net, cuda, train, encode):
    """train/train_VGG19.py:323-327: the trunk trains again after the first epochs"""
    m = train.freeze_trunk(copy.deepcopy(net["base"]).to(cuda))
    _, _, grads = training_run(m, net, cuda, train, encode)
    assert len(grads) == 184 - 18
    for p in m.parameters():
        p.requires_grad = True
    _, _, grads = training_run(m, net, cuda, train, encode)
    assert len(grads) == 184 and set(grads) == set(net["native"])
    for n in grads:
        assert torch.equal(grads[n], net["native"][n]), n
