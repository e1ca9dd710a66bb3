"""GPU suite of training an openpose.OpenPose_Model through the library's kernels (train.conv2d(prelu=), train.forward_train,
train.freeze_trunk, train.train_step, encode.get_loss_openpose).

(a) train.conv2d(prelu=) on the exact operands of prelu_restate.SPECS (integers and quarter slopes; tests/
test_prelu_backward_cpu.py holds every spec to 8 S < 2^24 on torch alone): y and the gradients of x, w, b and the slope equal
F.prelu(F.conv2d(...)) in float64 by torch.equal, over every subset of {x, w, b, a} that requires a gradient.
(b), (c) a dense block and the whole network against the same module tree run by torch on the CPU in float64.  For every
parameter p, r(p) = max|g - g64| / max|g64|; required: r_native(p) <= 4 * max_q r_cpu32(q), r_cpu32 the same quantity for
torch's own fp32 CPU autograd - the yardstick and the margin of tests/test_train_gpu.py, for the same reason: two equally
precise fp32 paths that differ in summation order and in the few sign decisions that fall on opposite sides of zero.  The
ratios go through conv_driver.note (profiles/r22_openpose_train.txt).
(d) - (g) the loss terms against the inference plan, the frozen trunk, one train_step against torch's SGD with the weight-sync
path behind it (slopes included), and a slope edited through .data."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_driver as cd
import prelu_restate as pr

pytestmark = pytest.mark.gpu

MARGIN = 4.0
TOPO = (2, 2, 52, 26)


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


@pytest.fixture(scope="module")
def openpose(pkg):
    return importlib.import_module(pkg.__name__ + ".openpose")


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


def init(model, seed):
    """He-initialised convs, slopes randn * 0.25"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                co, ci, k = m.weight.shape[0], m.weight.shape[1], m.weight.shape[2]
                m.weight.copy_(cd.weights("he", co, ci, k, g))
                m.bias.copy_(torch.randn(co, generator=g) * 0.1)
            elif isinstance(m, nn.PReLU):
                m.weight.copy_(torch.randn(m.weight.shape[0], generator=g) * 0.25)


def grads_of(params, loss):
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in params if p.grad is not None}


# ---- (a) train.conv2d(prelu=) on exact operands --------------------------------------------------------------------------------------
def exact_run(s, conv, dev, dt):
    """The spec's graph in `dt` arithmetic on `dev`: (y, {name: gradient or None})"""
    x, G, wt, b, a = (t.to(device=dev, dtype=dt).clone() for t in pr.spec_tensors(s))
    leaves = {"x": x.requires_grad_("x" in s.req), "w": wt.requires_grad_("w" in s.req), "b": b.requires_grad_("b" in s.req),
              "a": a.requires_grad_("a" in s.req)}
    y = conv(x, wt, b, a)
    if s.variant == "shared_slope":         # one slope (and filter bank), two convs in one graph: the gradients accumulate
        loss = (y * G).sum() + (conv(x.flip(3), wt, b, a) * G.flip(2)).sum()
    else:
        loss = (y * G).sum()
    if s.variant == "backward_twice":       # .grad doubles
        loss.backward(retain_graph=True)
    loss.backward()
    return y.detach(), {n: t.grad for n, t in leaves.items()}


@pytest.mark.parametrize("s", pr.SPECS, ids=pr.spec_id)
def test_conv2d_prelu_exact(cuda, train, s):
    y64, g64 = exact_run(s, lambda x, w, b, a: F.prelu(F.conv2d(x, w, b, padding=s.k // 2), a), "cpu", torch.float64)
    native = lambda x, w, b, a: train.conv2d(x, w, b, prelu=a)      # noqa: E731
    if s.variant == "side_stream":
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            y, g = exact_run(s, native, cuda, torch.float32)
        side.synchronize()
    else:
        y, g = exact_run(s, native, cuda, torch.float32)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y64), "y"
    assert (y64 < 0).any() or y64.numel() < 8
    for n in "xwba":
        if n in s.req:
            assert g64[n] is not None and g[n] is not None, n
            assert g[n].dtype == torch.float32 and g[n].shape == g64[n].shape
            wrong = int((g[n].double().cpu() != g64[n]).sum())
            assert wrong == 0, "d%s: %d of %d elements differ" % (n, wrong, g64[n].numel())
            assert g64[n].abs().max().item() > 0 or g64[n].numel() < 8
        else:
            assert g[n] is None and g64[n] is None, n


# ---- (b) a dense block ------------------------------------------------------------------------------------------------------------------
class Dense(nn.Module):
    """ConvBlock x 3 (8 -> 12 -> 12 -> 12, 3x3), concat, 1x1 ConvBlock (36 -> 10), 1x1 conv (10 -> 5): a fifth of a StageBlock"""

    def __init__(self, openpose):
        super().__init__()
        self.b0, self.b1, self.b2 = openpose.ConvBlock(8, 12), openpose.ConvBlock(12, 12), openpose.ConvBlock(12, 12)
        self.m6 = openpose.ConvBlock(36, 10, kernel_size=1, stride=1, padding=0)
        self.m7 = nn.Conv2d(10, 5, 1, 1, 0)
        init(self, 5)

    def forward(self, x, conv):
        o1 = conv(x, self.b0.Mconv, self.b0.MPrelu)
        o2 = conv(o1, self.b1.Mconv, self.b1.MPrelu)
        o3 = conv(o2, self.b2.Mconv, self.b2.MPrelu)
        return conv(conv(torch.cat([o1, o2, o3], 1), self.m6.Mconv, self.m6.MPrelu), self.m7, None)


def torch_conv(x, m, p):
    y = F.conv2d(x, m.weight, m.bias, padding=m.padding)
    return y if p is None else F.prelu(y, p.weight)


def test_dense_block_gradients(cuda, train, openpose):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 8, 12, 10, generator=g)
    target = torch.randn(2, 5, 12, 10, generator=g)
    base = Dense(openpose)
    assert all((p.weight < 0).any() and (p.weight > 0).any() for p in base.modules() if isinstance(p, nn.PReLU))
    native_conv = lambda t, m, p: train.conv2d(t, m.weight, m.bias, prelu=None if p is None else p.weight)   # noqa: E731
    out = {}
    for name, dt, dev in (("ref64", torch.float64, "cpu"), ("cpu32", torch.float32, "cpu"), ("native", torch.float32, cuda)):
        m = copy.deepcopy(base).to(device=dev, dtype=dt)
        xin = x.clone().to(device=dev, dtype=dt).requires_grad_(True)
        y = m(xin, native_conv if name == "native" else torch_conv)
        out[name] = grads_of(list(m.named_parameters()) + [("input", xin)], F.mse_loss(y, target.to(device=dev, dtype=dt)))
        out[name + "_y"] = y.detach().double().cpu()
    ref = {n: t.double() for n, t in out["ref64"].items()}
    assert set(out["native"]) == set(ref) and len(ref) == 15            # 5 convs x (weight, bias), 4 slopes, the input
    scale = max(1.0, out["ref64_y"].abs().max().item())
    assert (out["native_y"] - out["ref64_y"]).abs().max().item() <= cd.TOL * scale
    check_ratios("openpose_dense_block", out["native"], out["cpu32"], ref)


# ---- (c) the whole network at 1 x 3 x 32 x 32 (4 x 4 maps) --------------------------------------------------------------------------
def torch_block(blk, x):
    return F.prelu(F.conv2d(x, blk.Mconv.weight, blk.Mconv.bias, padding=blk.Mconv.padding), blk.MPrelu.weight)


def torch_stage(st, x):
    """lib/network/openpose.py:86-109 over the module tree, by torch"""
    for b in range(1, 6):
        o1 = torch_block(getattr(st, "Mconv%d_0" % b), x)
        o2 = torch_block(getattr(st, "Mconv%d_1" % b), o1)
        o3 = torch_block(getattr(st, "Mconv%d_2" % b), o2)
        x = torch.cat([o1, o2, o3], 1)
    return st.Mconv7(torch_block(st.Mconv6, x))


def torch_forward(model, x):
    """lib/network/openpose.py:160-177"""
    features = model.feature_extractor(x)
    paf_ret, heat_ret, x_in = [], [], features
    for st in model.l2_stages:
        paf = torch_stage(st, x_in)
        x_in = torch.cat([features, paf], 1)
        paf_ret.append(paf)
    for st in model.l1_stages:
        heat = torch_stage(st, x_in)
        x_in = torch.cat([features, heat, paf], 1)
        heat_ret.append(heat)
    return [paf_ret, heat_ret]


def names_of(log):
    return [n for n in log if n.startswith("loss_")]


@pytest.fixture(scope="module")
def net(cuda, train, encode, openpose):
    """The model, its inputs, and the gradients of the loss three ways; computed once, left unchanged."""
    torch.manual_seed(0)
    base = openpose.OpenPose_Model(*TOPO)
    init(base, 23)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 3, 32, 32, generator=g)
    heat, paf = torch.rand(1, TOPO[3], 4, 4, generator=g), torch.randn(1, TOPO[2], 4, 4, generator=g) * 0.5
    r = dict(base=base, x=x, heat=heat, paf=paf, count=sum(1 for _ in base.named_parameters()))
    for name, dt in (("ref64", torch.float64), ("cpu32", torch.float32)):
        m = copy.deepcopy(base).to(dtype=dt)
        total, _ = encode.get_loss_openpose(torch_forward(m, x.to(dt)), heat.to(dt), paf.to(dt))
        r[name] = grads_of(list(m.named_parameters()), total)
    m = copy.deepcopy(base).to(cuda)
    outs, saved = train.forward_train(m, x.to(cuda))
    assert outs[0][0] is saved[0][-2] and outs[0][1] is saved[1][-2] and outs[1][0] is saved[0][-1] and outs[1][1] is saved[1][-1]
    assert len(saved[0]) == TOPO[0] and len(saved[1]) == TOPO[1] and all(t.grad_fn is not None for s in saved for t in s)
    total, log = encode.get_loss_openpose(saved, heat.to(cuda), paf.to(cuda))
    r["native"] = grads_of(list(m.named_parameters()), total)
    r["native_log"], r["native_model"], r["native_total"] = log, m, total.detach().clone()
    r["ref64"] = {n: t.double() for n, t in r["ref64"].items()}
    return r


def test_whole_network_gradients(net):
    assert net["count"] == 227 and len(net["native"]) == 227 and set(net["native"]) == set(net["ref64"])
    slopes = [t for n, t in net["base"].named_parameters() if "MPrelu" in n or (n.startswith("feature_extractor") and t.dim() == 1
                                                                                 and n.endswith("weight"))]
    assert sum(int((t < 0).sum()) for t in slopes) > 1000            # slopes of either sign: sign(y) would not do
    check_ratios("openpose", net["native"], net["cpu32"], net["ref64"])


def test_training_losses_equal_the_inference_plan(net, cuda, encode):
    """(d) the terms of forward_train against get_loss_openpose on model(x), the inference plan of the same parameters"""
    m = net["native_model"]
    with torch.no_grad():
        _, saved = m(net["x"].to(cuda))
        _, log = encode.get_loss_openpose(saved, net["heat"].to(cuda), net["paf"].to(cuda))
    names = names_of(log)
    assert names == ["loss_paf_stage1", "loss_paf_stage2", "loss_heat_stage1", "loss_heat_stage2"] == names_of(net["native_log"])
    for name in names:
        a, b = net["native_log"][name], log[name]
        assert abs(a - b) <= cd.TOL * max(1.0, abs(b)), (name, a, b)


def training_run(m, net, cuda, train, encode):
    """(total, log, {name: gradient}) of one forward_train + get_loss_openpose + backward of the fixture's inputs"""
    m.zero_grad(set_to_none=True)
    _, saved = train.forward_train(m, net["x"].to(cuda))
    total, log = encode.get_loss_openpose(saved, net["heat"].to(cuda), net["paf"].to(cuda))
    total.backward()
    return total.detach(), log, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_frozen_trunk_gets_no_gradient_and_unfreezing_restores_it(net, cuda, train, encode):
    """(e)"""
    m = train.freeze_trunk(copy.deepcopy(net["base"]).to(cuda))
    _, _, got = training_run(m, net, cuda, train, encode)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert len(frozen) == 18 and all(p.grad is None for p in m.parameters() if not p.requires_grad)
    assert len(got) == 227 - 18 and not set(got) & set(frozen)
    for n, gr in got.items():          # the very gradients of the unfrozen run: the same launches on the same data
        assert torch.equal(gr, net["native"][n]), n
    for p in m.parameters():
        p.requires_grad = True
    _, _, got = training_run(m, net, cuda, train, encode)
    assert len(got) == 227 and set(got) == set(net["native"])
    for n in got:
        assert torch.equal(got[n], net["native"][n]), n


def test_train_step_is_torch_sgd_on_the_native_gradients_and_inference_resyncs(net, openpose, cuda, train, encode):
    """(f)"""
    x, heat, paf = net["x"].to(cuda), net["heat"].to(cuda), net["paf"].to(cuda)
    a = copy.deepcopy(net["base"]).to(cuda)
    with torch.no_grad():
        before = [t.clone() for s in a(x)[1] for t in s]           # packs the inference arena from the initial parameters
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf)
    assert total.item() == pytest.approx(sum(log[n] for n in names_of(log)), rel=1e-5) and len(names_of(log)) == 4
    assert {"max_ht", "min_ht", "max_paf", "min_paf"} <= set(log)
    b = copy.deepcopy(net["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = net["native"][n].clone()
    opt_b.step()
    start = dict(net["base"].named_parameters())
    moved_slopes = 0
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
        if n.endswith("weight"):
            assert not torch.equal(pa.detach().cpu(), start[n].detach()), "%s did not move" % n
            moved_slopes += pa.dim() == 1
    assert moved_slopes == 3 + 4 * 16                               # every PReLU of the trunk and of the four stages
    # inference after the step: the plan reloads filters AND slopes from the updated parameters (weight-sync path)
    fresh = openpose.OpenPose_Model(*TOPO)
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda)
    with torch.no_grad():
        got, want = [t for s in a(x)[1] for t in s], [t for s in fresh(x)[1] for t in s]
    assert len(got) == 4
    for i in range(4):
        assert torch.equal(got[i], want[i]), i
    assert any(not torch.equal(got[i], before[i]) for i in range(4))


def test_a_slope_edited_through_data_is_seen_without_invalidate_weights(net, cuda, train, encode):
    """(g) slopes are read from the parameter's storage by every launch: no cache to tell"""
    m = copy.deepcopy(net["base"]).to(cuda)
    total, _, first = training_run(m, net, cuda, train, encode)
    assert torch.equal(total, net["native_total"])
    versions = [p._version for p in m.parameters()]
    m.feature_extractor[22].weight.data.add_(0.125)                  # conv4_2's PReLU
    m.l2_stages[0].Mconv1_0.MPrelu.weight.data.mul_(-1.5)
    m.l1_stages[1].Mconv6.MPrelu.weight.data.neg_()
    assert isinstance(m.feature_extractor[22], nn.PReLU) and versions == [p._version for p in m.parameters()]
    total2, log2, got = training_run(m, net, cuda, train, encode)
    total3, log3, want = training_run(copy.deepcopy(m), net, cuda, train, encode)
    assert torch.equal(total2, total3) and log2 == log3 and not torch.equal(total2, total)
    assert len(got) == 227 and set(got) == set(want)
    for n in got:
        assert torch.equal(got[n], want[n]), n
    assert not torch.equal(got["l2_stages.0.Mconv1_0.MPrelu.weight"], first["l2_stages.0.Mconv1_0.MPrelu.weight"])
