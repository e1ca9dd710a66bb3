"""GPU suite of training an hourglass.HourglassNet through the library's kernels (train.batch_norm, train.conv7x7_s2,
train.hourglass_forward / forward_train, train.train_step, encode.get_loss_hourglass).

(a) train.batch_norm against float64 F.batch_norm autograd within the bounds tests/bn_restate.py derives, over the seven
requires_grad subsets of (x, weight, bias), a non-contiguous x and gy, two consumers and backward() twice.
(b) train.conv7x7_s2 on exact integer operands: y, dW and dbias equal F.conv2d(stride=2)'s float64 autograd with ==.
(c) a whole Bottleneck, with and without `downsample`: for every parameter p, r(p) = max|g - g64| / max|g64| (for a conv
bias in front of a BatchNorm, whose true gradient is zero, over max|g64| of that conv's weight); required:
r_native(p) <= 4 * max_q r_cpu32(q), r_cpu32 the same quantity for torch's own fp32 CPU autograd - the yardstick and margin
of tests/test_train_gpu.py.  The seeds are fixed ones for which no float64 BatchNorm output lies within 64 x the measured
fp32 forward error of zero (asserted here on the CPU), so no ReLU mask can flip.  "Measured at an output": the larger of
torch's fp32 CPU error at that very output and the RMS fp32 error of its BatchNorm layer.  (With the layer's WORST error
instead - 1.9e-6 at 2 x 64 x 16 x 16, where the three layers have 98 K outputs of unit scale - about ten outputs lie inside
64 x 1.9e-6 of zero whatever the seed: none of 150 seeds met that reading; the 2 x 256 x 4 x 4 seed meets it as well.)
(d) the whole network, hg(2, 1, 38, 19) at 2 x 3 x 128 x 128: only what is continuous or exact is asserted - the outputs and
the updated running statistics within 4 x torch's fp32 CPU error against float64, num_batches_tracked, finite gradients of
the right shapes, two runs bit-identical, one train_step equal to torch's SGD on the native gradients bit for bit, the
inference plan after .eval() equal to a freshly built model's, the refusals.  The per-parameter gradient errors of the native
path and of torch's fp32 CPU path against float64 are noted (profiles/r23_hourglass_train.txt), NOT asserted: one ReLU
sign flip reaches every parameter through the batch statistics, and the count of flips differs between any two fp32 paths
(DESIGN.md 3.3g)."""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_restate as br
import conv_driver as cd
import hourglass_restate as hr
import hourglass_train_restate as htr

pytestmark = pytest.mark.gpu

MARGIN = 4.0
TOPO = dict(num_stacks=2, num_blocks=1, paf_classes=38, ht_classes=19)


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


@pytest.fixture(scope="module")
def hgm(pkg):
    return importlib.import_module(pkg.__name__ + ".hourglass")


def f64(t):
    return t.detach().double().cpu().numpy()


# ---- (a) train.batch_norm -------------------------------------------------------------------------------------------------------------
BN_CASE = br.CASES[12]          # 8 channels, 3 x 19 x 18: several slabs across image boundaries
SUBSETS = ("x", "w", "b", "xw", "xb", "wb", "xwb")
VARIANTS = (None, "noncontiguous", "two_consumers", "backward_twice")
BN_RUNS = [(s, None, False) for s in SUBSETS] + [("xwb", v, True) for v in VARIANTS] + [("xwb", v, False) for v in VARIANTS[1:]]


def make_bn(w, b, rm, rv, dev, req):
    bn = nn.BatchNorm2d(w.numel())
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    bn.weight.requires_grad_("w" in req), bn.bias.requires_grad_("b" in req)
    return bn.to(dev).train()


@pytest.mark.parametrize("req,variant,relu", BN_RUNS, ids=["%s_%s_%s" % (r, v or "plain", "relu" if u else "id") for r, v, u in BN_RUNS])
def test_batch_norm_against_float64(cuda, train, req, variant, relu):
    c = BN_CASE
    if relu:
        x, gy, w, b, rm, rv, t, bd, margin = br.relu_operands(c)
        assert margin > 0
    else:
        x, gy = br.random_operands(c, seed=3)
        w, b, rm, rv = br.affine(c.channels, False)
        t = br.bn64(x, gy, w, b, rm, rv)
        bd = br.bounds(x.numpy(), gy.numpy(), w.numpy(), b.numpy(), t, rm.numpy(), rv.numpy())
    bn = make_bn(w, b, rm, rv, cuda, req)
    if variant == "noncontiguous":          # NHWC storage behind NCHW shapes
        xd = x.permute(0, 2, 3, 1).contiguous().to(cuda).permute(0, 3, 1, 2)
        gd = gy.permute(0, 3, 2, 1).contiguous().to(cuda).permute(0, 3, 2, 1)
        assert not xd.is_contiguous() and not gd.is_contiguous()
    else:
        xd, gd = x.to(cuda), gy.to(cuda)
    xd = xd.requires_grad_("x" in req)
    y = train.batch_norm(xd, bn, relu=relu)
    times = 1
    if variant == "two_consumers":
        (y * gd).sum().add((y * gd).sum()).backward()
        times = 2
    elif variant == "backward_twice":
        loss = (y * gd).sum()
        loss.backward(retain_graph=True)
        loss.backward()
        times = 2
    else:
        y.backward(gd)
    assert int(bn.num_batches_tracked) == 1
    assert (np.abs(f64(y) - t["y"].numpy()) <= br.y_bound(x.numpy(), t, bd)).all(), "y"
    if relu:
        assert ((y.detach().cpu().numpy() > 0) == (t["y"].numpy() > 0)).all()
    assert (np.abs(f64(bn.running_mean) - t["running_mean"].numpy()) <= bd["running_mean"]).all()
    assert (np.abs(f64(bn.running_var) - t["running_var"].numpy()) <= bd["running_var"]).all()
    got = {"x": xd.grad, "w": bn.weight.grad, "b": bn.bias.grad}
    want = {"x": (t["dx"].numpy(), br.dx_bound(x.numpy(), gy.numpy(), w.numpy(), t, bd, relu)),
            "w": (t["dweight"].numpy(), bd["dweight"]), "b": (t["dbias"].numpy(), bd["dbias"])}
    for n in "xwb":
        if n not in req:
            assert got[n] is None, n
            continue
        ref, bound = want[n]
        # accumulated twice: both terms within the bound, and their fp32 sum rounds once more
        err = np.abs(f64(got[n]) - times * ref)
        assert got[n].dtype == torch.float32 and tuple(got[n].shape) == ref.shape
        assert (err <= times * bound + (times - 1) * br.U32 * np.abs(times * ref)).all(), (n, float((err / np.maximum(bound, 1e-300)).max()))


# ---- (b) train.conv7x7_s2 on exact integers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 2, 2), (2, 5, 7), (1, 8, 6), (2, 64, 64)])
@pytest.mark.parametrize("req", ["wb", "w", "b"])
def test_conv7x7_s2_exact(cuda, train, n, h, w, req):
    """integers: |x| <= 3, |w| <= 2, |gy| <= 3, so every sum of y (147 terms) and of dW (at most n * 32 * 32 terms) stays
    below 2^24 and fp32 arithmetic in any order is exact"""
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    x = torch.randint(-3, 4, (n, 3, h, w), generator=g).float()
    wt = torch.randint(-2, 3, (64, 3, 7, 7), generator=g).float()
    b = torch.randint(-4, 5, (64,), generator=g).float()
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = F.conv2d(x.double(), w64, b64, stride=2, padding=3)
    gy = torch.randint(-3, 4, y64.shape, generator=g).float()
    assert n * y64.shape[2] * y64.shape[3] * 9 < 2 ** 24 and 147 * 6 + 4 < 2 ** 24
    dw64, db64 = torch.autograd.grad(y64, (w64, b64), gy.double())
    wd, bd_ = wt.to(cuda).requires_grad_("w" in req), b.to(cuda).requires_grad_("b" in req)
    y = train.conv7x7_s2(x.to(cuda), wd, bd_)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y64.detach())
    y.backward(gy.to(cuda))
    if "w" in req:
        assert torch.equal(wd.grad.double().cpu(), dw64) and dw64.abs().max() > 0
    else:
        assert wd.grad is None
    if "b" in req:
        assert torch.equal(bd_.grad.double().cpu(), db64)
    else:
        assert bd_.grad is None


def test_conv7x7_s2_refuses_an_image_that_requires_a_gradient(cuda, train):
    x = torch.zeros(1, 3, 8, 8, device=cuda, requires_grad=True)
    with pytest.raises(RuntimeError, match="must not require a gradient"):
        train.conv7x7_s2(x, torch.zeros(64, 3, 7, 7, device=cuda, requires_grad=True))
    with pytest.raises(RuntimeError, match=r"nn.Conv2d\(3, 64, 7, stride 2, padding 3\)"):
        train.conv7x7_s2(torch.zeros(1, 3, 8, 8, device=cuda), torch.zeros(64, 3, 3, 3, device=cuda))


# ---- (c) a Bottleneck --------------------------------------------------------------------------------------------------------------------
FLIP_MARGIN = 64.0
# (inplanes, planes, downsample, n, h, w, seed): fixed seeds that meet the no-flip condition asserted below
BLOCKS = [(64, 64, True, 2, 16, 16, 4), (256, 128, False, 2, 4, 4, 3)]


def seed_block(blk, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    with torch.no_grad():
        for name, m in blk.named_modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                var = hr.STRONG_GAIN if name == "conv3" else 2.0
                m.weight.copy_(torch.from_numpy(rng.standard_normal(tuple(m.weight.shape)) * np.sqrt(var / fan_in)).float())
                m.bias.copy_(torch.from_numpy(rng.standard_normal(m.bias.shape[0]) * 0.05).float())
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.weight.shape[0])).float())
                m.bias.copy_(torch.from_numpy(rng.standard_normal(m.bias.shape[0]) * 0.1).float())
    return blk


def block_run(train, blk, x, target, conv, bn):
    """(y, {name: grad}, [BatchNorm pre-activations]) of one forward + backward of the block"""
    pre = []

    def bn_spy(t, m):
        if conv is not None:
            return bn(t, m)
        z = F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps)
        pre.append(z.detach())
        return F.relu(z)
    tconv, _, _ = htr.torch_ops()
    y = train.hourglass_bottleneck(blk, x, conv or tconv, bn_spy)
    F.mse_loss(y, target).backward()
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    grads["input"] = x.grad.detach().clone()
    return y.detach(), grads, pre


def block_ratios(grads, ref):
    out = {}
    for n, g64 in ref.items():
        den = g64.abs().max()
        if n in ("conv1.bias", "conv2.bias"):       # in front of a BatchNorm: the true gradient is zero
            den = ref[n[:-4] + "weight"].abs().max()
        out[n] = ((grads[n].double().cpu() - g64).abs().max() / den).item()
    return out


@pytest.mark.parametrize("cin,planes,ds,n,h,w,seed", BLOCKS, ids=["downsample_2x64x16x16", "plain_2x256x4x4"])
def test_bottleneck_gradients(cuda, train, hgm, cin, planes, ds, n, h, w, seed):
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(n, cin, h, w, generator=g)
    target = torch.randn(n, 2 * planes, h, w, generator=g)
    base = seed_block(hgm.Bottleneck(cin, planes, ds), seed).train()
    b64, b32 = copy.deepcopy(base).double(), copy.deepcopy(base)
    y64, ref, pre64 = block_run(train, b64, x.double().requires_grad_(True), target.double(), None, None)
    y32, cpu32, pre32 = block_run(train, b32, x.clone().requires_grad_(True), target, None, None)
    # the no-flip condition, on the CPU (module docstring): the forward error measured at an output is the larger of that
    # output's own fp32 error and its layer's RMS fp32 error
    assert len(pre64) == 3
    for a, z in zip(pre32, pre64):
        err = (a.double() - z).abs()
        assert (z.abs() > FLIP_MARGIN * torch.maximum(err, err.pow(2).mean().sqrt())).all(), "seed %d: a BatchNorm output may flip" % seed
        assert ((a > 0) == (z > 0)).all()
    found = seed
    nb = copy.deepcopy(base).to(cuda)
    conv = lambda t, m: train.conv2d(t, m.weight, m.bias)                           # noqa: E731
    bn = lambda t, m: train.batch_norm(t, m, relu=True)                             # noqa: E731
    y, native, _ = block_run(train, nb, x.to(cuda).requires_grad_(True), target.to(cuda), conv, bn)
    fwd_native = (y.double().cpu() - y64).abs().max().item()
    fwd_cpu32 = (y32.double() - y64).abs().max().item()
    rn, rc = block_ratios(native, ref), block_ratios(cpu32, ref)
    yard = max(rc.values())
    worst = max(rn, key=rn.get)
    print("bottleneck %d->%d seed %d: forward err native %.3g cpu32 %.3g; worst native ratio %.3g (%s), yardstick %.3g"
          % (cin, 2 * planes, found, fwd_native, fwd_cpu32, rn[worst], worst, yard))
    cd.note("train_grad_ratios_bottleneck_%d.json" % cin, {"seed": found, "yardstick_max_r_cpu32": yard, "forward_err_native": fwd_native,
                                                             "forward_err_cpu32": fwd_cpu32,
                                                             "per_parameter": {k: {"native": rn[k], "cpu32": rc[k]} for k in rn}})
    assert set(native) == set(ref) and len(ref) == (14 if ds else 12) + 1
    assert fwd_native <= MARGIN * fwd_cpu32
    bad = {k: r for k, r in rn.items() if not r <= MARGIN * yard}
    assert not bad, "r_native above %g x %.3g: %s" % (MARGIN, yard, bad)
    for k in ("bn1", "bn2", "bn3"):
        mod, m64 = getattr(nb, k), getattr(b64, k)
        assert int(mod.num_batches_tracked) == 1
        assert torch.allclose(mod.running_mean.double().cpu(), m64.running_mean, rtol=1e-5, atol=1e-6)
        assert torch.allclose(mod.running_var.double().cpu(), m64.running_var, rtol=1e-5, atol=1e-6)


# ---- (d) the whole network ------------------------------------------------------------------------------------------------------------------
def stats_of(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}


def norm_err(a, ref):
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def grad_errs(grads, ref):
    """max|g - g64| / max|g64| per parameter; a conv bias over its conv's weight-gradient magnitude: a per-channel constant
    in front of a BatchNorm has a true gradient of zero, and so has, up to the borders of the 3x3 convs, one added to the
    256-channel trunk (conv3, the hand-over convs)"""
    out = {}
    for k, g64 in ref.items():
        den = g64.abs().max()
        mod = k[:-len(".bias")] if k.endswith(".bias") else None
        if mod is not None and ref[mod + ".weight"].dim() == 4:
            den = ref[mod + ".weight"].abs().max()
        out[k] = ((grads[k].double().cpu() - g64).abs().max() / den).item()
    return out


def quantiles(d):
    v = np.sort(np.array(list(d.values())))
    return {"median": float(np.median(v)), "p90": float(v[int(0.9 * (len(v) - 1))]), "worst": float(v[-1])}


@pytest.fixture(scope="module")
def net(cuda, train, encode, hgm):
    """The model, its inputs and one training forward + backward three ways; computed once, left unchanged."""
    torch.manual_seed(0)
    base = htr.seed_model(hgm.hg(**TOPO), 7).train()
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, 128, 128, generator=g)
    heat, paf = torch.rand(2, 19, 32, 32, generator=g), torch.randn(2, 38, 32, 32, generator=g) * 0.5
    hmask = (torch.rand(2, 19, 32, 32, generator=g) > 0.2).float()
    pmask = (torch.rand(2, 38, 32, 32, generator=g) > 0.2).float()
    r = dict(base=base, x=x, heat=heat, paf=paf, hmask=hmask, pmask=pmask)
    for name, dt in (("ref64", torch.float64), ("cpu32", torch.float32)):
        m = copy.deepcopy(base).to(dtype=dt)
        (p, h), saved = train.hourglass_forward(m, x.to(dt), *htr.torch_ops())
        total, _ = encode.get_loss_hourglass(saved, heat.to(dt), hmask.to(dt), paf.to(dt), pmask.to(dt))
        total.backward()
        r[name] = dict(paf=p.detach().double(), ht=h.detach().double(), stats={k: v.double() for k, v in stats_of(m).items()},
                       grads={n: q.grad.detach().double() for n, q in m.named_parameters()},
                       tracked={k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")})
    m = copy.deepcopy(base).to(cuda)
    dev = [t.to(cuda) for t in (x, heat, hmask, paf, pmask)]
    (p, h), saved = train.forward_train(m, dev[0])
    assert saved[0] is p and saved[1] is h and p.grad_fn is not None
    total, log = encode.get_loss_hourglass(saved, *dev[1:])
    total.backward()
    r["native"] = dict(paf=p.detach(), ht=h.detach(), stats=stats_of(m), grads={n: q.grad.detach().clone() for n, q in m.named_parameters()},
                       tracked={k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}, log=log,
                       total=total.detach().clone())
    r["dev"] = dev
    return r


def test_forward_and_running_statistics_within_the_yardstick(net):
    ref, cpu, nat = net["ref64"], net["cpu32"], net["native"]
    report = {}
    for k in ("paf", "ht"):
        e_n, e_c = (nat[k].double().cpu() - ref[k]).abs().max().item(), (cpu[k] - ref[k]).abs().max().item()
        report[k] = {"native": e_n, "cpu32": e_c}
        assert tuple(nat[k].shape) == tuple(ref[k].shape) and e_n <= MARGIN * e_c, (k, e_n, e_c)
    rn = {k: norm_err(v, ref["stats"][k]) for k, v in nat["stats"].items()}
    rc = {k: norm_err(v, ref["stats"][k]) for k, v in cpu["stats"].items()}
    yard = max(rc.values())
    report["running_statistics"] = {"native": quantiles(rn), "cpu32": quantiles(rc)}
    assert len(rn) == 2 * sum(1 for m in net["base"].modules() if isinstance(m, nn.BatchNorm2d)) == 2 * (1 + 3 * 3 + 2 * 3 * 14 + 2)
    assert nat["tracked"] == ref["tracked"] and set(nat["tracked"].values()) == {1}
    # the gradients: recorded, not asserted (module docstring)
    gn, gc = grad_errs(nat["grads"], ref["grads"]), grad_errs(cpu["grads"], ref["grads"])
    report["parameter_gradients_not_asserted"] = {"native": quantiles(gn), "cpu32": quantiles(gc)}
    print("hourglass hg(2,1,38,19) 2x3x128x128:", report)
    cd.note("train_hourglass_whole_network.json", report)
    bad = {k: r for k, r in rn.items() if not r <= MARGIN * yard}
    assert not bad, "running statistics above %g x %.3g: %s" % (MARGIN, yard, bad)


def test_every_parameter_gets_a_finite_gradient_and_runs_repeat(net, cuda, train, encode):
    grads = net["native"]["grads"]
    params = dict(net["base"].named_parameters())
    assert set(grads) == set(params)
    for n, g in grads.items():
        assert g.dtype == torch.float32 and g.shape == params[n].shape and torch.isfinite(g).all(), n
    assert all(g.abs().max() > 0 for n, g in grads.items() if n.endswith('weight')), "a weight without a gradient"
    m = copy.deepcopy(net["base"]).to(cuda)
    _, saved = train.forward_train(m, net["dev"][0])
    total, log = encode.get_loss_hourglass(saved, *net["dev"][1:])
    total.backward()
    assert torch.equal(total, net["native"]["total"]) and log == net["native"]["log"]
    for n, q in m.named_parameters():
        assert torch.equal(q.grad, grads[n]), n
    for k, v in stats_of(m).items():
        assert torch.equal(v, net["native"]["stats"][k]), k


def test_train_step_is_torch_sgd_on_the_native_gradients_and_inference_resyncs(net, hgm, cuda, train):
    x, heat, hmask, paf, pmask = net["dev"]
    a = copy.deepcopy(net["base"]).to(cuda)
    with torch.no_grad():
        before = a.eval()(x)[0]                                  # packs the inference arena from the initial parameters
    a.train()
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf, heat_mask=hmask, paf_mask=pmask)
    assert torch.equal(total.detach(), net["native"]["total"]) and list(log)[:2] == ["paf", "heatmap"]
    b = copy.deepcopy(net["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = net["native"]["grads"][n].clone()
    opt_b.step()
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
    for k, v in stats_of(a).items():
        assert torch.equal(v, net["native"]["stats"][k]), k
    # inference after the step: the plan folds the UPDATED running statistics (written through raw pointers) and parameters
    fresh = hgm.hg(**TOPO)
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda).eval()
    with torch.no_grad():
        got, want = a.eval()(x)[0], fresh(x)[0]
    for i in range(2):
        assert torch.equal(got[i], want[i]), i
        assert not torch.equal(got[i], before[i])


def test_refusals(net, cuda, train):
    m = copy.deepcopy(net["base"]).to(cuda)
    x = net["dev"][0]
    with pytest.raises(RuntimeError, match=r"call \.train\(\) first"):
        train.forward_train(m.eval(), x)
    m.train()
    with pytest.raises(TypeError, match="freezes nothing of a HourglassNet"):
        train.freeze_trunk(m)
    with pytest.raises(RuntimeError, match="must not require a gradient"):
        train.forward_train(m, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="call .eval"):
        m(x)                                                     # model.forward, the inference plan, is untouched
