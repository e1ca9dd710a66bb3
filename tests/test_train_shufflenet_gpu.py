"""GPU suite of training a shufflenet.Network through the library's kernels (train.dwconv3x3, train.conv3x3_s2,
train.shufflenet_forward / forward_train, train.train_step, encode.get_loss_shufflenet).

(a) train.dwconv3x3 and train.conv3x3_s2 on exact integer operands: y and every gradient equal F.conv2d's float64 autograd
with ==, over every requires_grad subset of (x, weight).
(b) one two-branch stride-2 block (24 -> 116 at 2 x 16 x 16) and one split block (116 at 2 x 8 x 8) by the method of
tests/test_train_hourglass_gpu.py::test_bottleneck_gradients, with that file's MARGIN and FLIP_MARGIN: for every parameter
p and the input, r(p) = max|g - g64| / max|g64|; required: r_native(p) <= MARGIN * max_q r_cpu32(q), r_cpu32 the same
quantity for torch's own fp32 CPU autograd.  The seeds are fixed ones for which no float64 pre-activation of a BatchNorm
that is followed by a ReLU lies within FLIP_MARGIN x the measured fp32 forward error of zero (asserted here on the CPU), so
no ReLU mask can flip.  The ratios are noted as json (conv_driver.note).
(c) the whole network at 2 x 3 x 72 x 88 (maps 36 x 44 at the stem, 18 x 22 at the pool, 9 x 11 at the heads) and at
2 x 3 x 36 x 44 (18 x 22, 9 x 11 and 5 x 6: every stride-2 layer sees an odd or an even edge), as the hourglass's is: only
what is continuous or exact is asserted - the outputs and the updated running statistics within MARGIN x torch's fp32 CPU
error against float64, num_batches_tracked == 1 everywhere, a finite gradient of its own shape for every parameter, two
runs bit-identical, one train_step equal to torch's SGD on the native gradients bit for bit, the inference plan after
.eval() different from before and equal to a freshly built model's, the refusals.  The per-parameter gradient errors of
the native path and of torch's fp32 CPU path against float64 are noted, NOT asserted: one ReLU sign flip reaches every
parameter through the batch statistics."""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_driver as cd
import dwconv_restate as dr
from test_train_hourglass_gpu import FLIP_MARGIN, MARGIN, norm_err, quantiles, stats_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


@pytest.fixture(scope="module")
def shuf(pkg):
    return importlib.import_module(pkg.__name__ + ".shufflenet")


# ---- (a) exact integer sets ------------------------------------------------------------------------------------------------------------
DW_SHAPES = [(1, 4, 1, 1), (2, 3, 5, 7), (1, 58, 8, 6), (2, 8, 9, 11), (3, 6, 16, 23)]


@pytest.mark.parametrize("req", ["xw", "x", "w"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n,c,h,w", DW_SHAPES)
def test_dwconv3x3_exact(cuda, train, n, c, h, w, stride, req):
    """integers: |x| <= 4, |w| <= 3, |gy| <= 3: y (9 terms), dx (9 terms) and dW (at most n * 16 * 23 terms of at most 12)
    stay far below 2^24, so fp32 arithmetic in any order is exact"""
    x, gy, wt = dr.exact_operands(dr.Case(n, c, h, w, stride, None, None, None, ""), seed=stride)
    y64, dx64, dw64 = dr.autograd64(x, wt, gy, stride)
    xd, wd = x.to(cuda).requires_grad_("x" in req), wt.to(cuda).requires_grad_("w" in req)
    y = train.dwconv3x3(xd, wd, stride)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y64)
    y.backward(gy.to(cuda))
    if "x" in req:
        assert xd.grad.dtype == torch.float32 and torch.equal(xd.grad.double().cpu(), dx64)
    else:
        assert xd.grad is None
    if "w" in req:
        assert wd.grad.shape == wt.shape and torch.equal(wd.grad.double().cpu(), dw64) and (c * h * w < 8 or dw64.abs().max() > 0)
    else:
        assert wd.grad is None


def test_dwconv3x3_without_a_gradient_and_refusals(cuda, train, capi):
    x, _, wt = dr.exact_operands(dr.Case(2, 8, 9, 11, 2, None, None, None, ""))
    y = train.dwconv3x3(x.to(cuda), wt.to(cuda), 2)
    assert not y.requires_grad and torch.equal(y.double().cpu(), dr.autograd64(x, wt, torch.zeros(2, 8, 5, 6), 2)[0])
    err = capi.RtposeError
    with pytest.raises(err, match="stride must be 1 or 2"):
        train.dwconv3x3(x.to(cuda), wt.to(cuda), 3)
    with pytest.raises(err, match=r"filters \[C, 1, 3, 3\]"):
        train.dwconv3x3(x.to(cuda), wt[:4].to(cuda), 1)
    with pytest.raises(err, match=r"filters \[C, 1, 3, 3\]"):
        train.dwconv3x3(x.to(cuda).double(), wt.to(cuda).double(), 1)
    with pytest.raises(err, match="no CPU fallback"):
        train.dwconv3x3(x, wt.to(cuda), 1)


@pytest.mark.parametrize("req", ["xw", "x", "w"])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 5, 7), (1, 8, 6), (2, 8, 9), (2, 36, 44)])
def test_conv3x3_s2_exact(cuda, train, n, h, w, req):
    """integers: |x| <= 3, |w| <= 2, |gy| <= 3: y (27 terms), dx (at most 24 * 9 terms) and dW (at most n * 18 * 22 terms) stay
    below 2^24, so fp32 arithmetic in any order is exact"""
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    x = torch.randint(-3, 4, (n, 3, h, w), generator=g).float()
    wt = torch.randint(-2, 3, (24, 3, 3, 3), generator=g).float()
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, stride=2, padding=1)
    gy = torch.randint(-3, 4, y64.shape, generator=g).float()
    dx64, dw64 = torch.autograd.grad(y64, (x64, w64), gy.double())
    xd, wd = x.to(cuda).requires_grad_("x" in req), wt.to(cuda).requires_grad_("w" in req)
    y = train.conv3x3_s2(xd, wd)
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y64.detach())
    y.backward(gy.to(cuda))
    if "x" in req:
        assert torch.equal(xd.grad.double().cpu(), dx64)
    else:
        assert xd.grad is None
    if "w" in req:
        assert torch.equal(wd.grad.double().cpu(), dw64) and (h * w < 8 or dw64.abs().max() > 0)
    else:
        assert wd.grad is None


def test_conv3x3_s2_refusals(cuda, train, capi):
    with pytest.raises(capi.RtposeError, match=r"nn.Conv2d\(3, 24, 3, stride 2, padding 1, bias=False\)"):
        train.conv3x3_s2(torch.zeros(1, 3, 8, 8, device=cuda), torch.zeros(64, 3, 7, 7, device=cuda))
    with pytest.raises(capi.RtposeError, match=r"nn.Conv2d\(3, 24, 3, stride 2, padding 1, bias=False\)"):
        train.conv3x3_s2(torch.zeros(1, 4, 8, 8, device=cuda), torch.zeros(24, 3, 3, 3, device=cuda))
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.conv3x3_s2(torch.zeros(1, 3, 8, 8), torch.zeros(24, 3, 3, 3, device=cuda))


# ---- (b) two blocks ----------------------------------------------------------------------------------------------------------------------
# (in_channels, out_channels, stride, two_branch, n, h, w, seed): fixed seeds that meet the no-flip condition asserted below
BLOCKS = [(24, 116, 2, True, 2, 16, 16, 0), (116, 116, 1, False, 2, 8, 8, 1)]


def block_run(train, blk, x, target, ops):
    """(y, {name: grad}, [pre-activations of the BatchNorms in front of a ReLU]) of one forward + backward of the block"""
    pre = []
    conv, bn, dw, _ = ops if ops is not None else dr.torch_ops(pre)
    y = train.shufflenet_block(blk, x, conv, bn, dw)
    F.mse_loss(y, target).backward()
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    grads["input"] = x.grad.detach().clone()
    return y.detach(), grads, pre


def no_flip(pre32, pre64):
    """the no-flip condition of tests/test_train_hourglass_gpu.py: the forward error measured at an output is the larger of
    that output's own fp32 error and its layer's RMS fp32 error"""
    for a, z in zip(pre32, pre64):
        err = (a.double() - z).abs()
        if not (z.abs() > FLIP_MARGIN * torch.maximum(err, err.pow(2).mean().sqrt())).all() or not ((a > 0) == (z > 0)).all():
            return False
    return True


def block_operands(shuf, cin, cout, stride, two, n, h, w, seed):
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(n, cin, h, w, generator=g)
    ho, wo = dr.out_size(h, w, stride)
    target = torch.randn(n, cout, ho, wo, generator=g)
    return x, target, dr.seed_module(shuf.BasicBlock(cin, cout, stride, two), seed).train()


def block_ratios(grads, ref):
    """max|g - g64| / max|g64| per parameter.  The bias of a BatchNorm without a ReLU (behind a depthwise conv: conv0.0.1,
    conv.1.1) feeds a 1x1 conv and ITS training-mode BatchNorm, which removes a per-channel constant: the true gradient is
    zero, so it is measured over the magnitude of the same BatchNorm's weight gradient (the hourglass file's rule for a
    conv bias in front of a BatchNorm)."""
    out = {}
    for n, g64 in ref.items():
        den = g64.abs().max()
        if n in ("conv0.0.1.bias", "conv.1.1.bias"):
            den = ref[n[:-4] + "weight"].abs().max()
        out[n] = ((grads[n].double().cpu() - g64).abs().max() / den).item()
    return out


@pytest.mark.parametrize("cin,cout,stride,two,n,h,w,seed", BLOCKS, ids=["two_branch_s2_24_116_2x16x16", "split_116_2x8x8"])
def test_block_gradients(cuda, train, shuf, cin, cout, stride, two, n, h, w, seed):
    x, target, base = block_operands(shuf, cin, cout, stride, two, n, h, w, seed)
    b64, b32 = copy.deepcopy(base).double(), copy.deepcopy(base)
    y64, ref, pre64 = block_run(train, b64, x.double().requires_grad_(True), target.double(), None)
    y32, cpu32, pre32 = block_run(train, b32, x.clone().requires_grad_(True), target, None)
    assert len(pre64) == (3 if two else 2)
    assert no_flip(pre32, pre64), "seed %d: a BatchNorm output in front of a ReLU may flip" % seed
    nb = copy.deepcopy(base).to(cuda)
    ops = (lambda t, m: train.conv2d(t, m.weight, m.bias), lambda t, m, relu: train.batch_norm(t, m, relu=relu),
           lambda t, m: train.dwconv3x3(t, m.weight, m.stride[0]), None)
    y, native, _ = block_run(train, nb, x.to(cuda).requires_grad_(True), target.to(cuda), ops)
    fwd_native = (y.double().cpu() - y64).abs().max().item()
    fwd_cpu32 = (y32.double() - y64).abs().max().item()
    rn, rc = block_ratios(native, ref), block_ratios(cpu32, ref)
    yard = max(rc.values())
    worst = max(rn, key=rn.get)
    print("shufflenet block %d->%d stride %d seed %d: forward err native %.3g cpu32 %.3g; worst native ratio %.3g (%s), yardstick %.3g"
          % (cin, cout, stride, seed, fwd_native, fwd_cpu32, rn[worst], worst, yard))
    cd.note("train_grad_ratios_shufflenet_block_%d_s%d.json" % (cin, stride),
            {"seed": seed, "yardstick_max_r_cpu32": yard, "forward_err_native": fwd_native, "forward_err_cpu32": fwd_cpu32,
             "per_parameter": {k: {"native": rn[k], "cpu32": rc[k]} for k in rn}})
    assert set(native) == set(ref) and len(ref) == (5 if two else 3) * 3 + 1
    assert fwd_native <= MARGIN * fwd_cpu32
    bad = {k: r for k, r in rn.items() if not r <= MARGIN * yard}
    assert not bad, "r_native above %g x %.3g: %s" % (MARGIN, yard, bad)
    for (k, mod), (_, m64) in zip(nb.named_modules(), b64.named_modules()):
        if isinstance(mod, nn.BatchNorm2d):
            assert int(mod.num_batches_tracked) == 1, k
            assert torch.allclose(mod.running_mean.double().cpu(), m64.running_mean, rtol=1e-5, atol=1e-6), k
            assert torch.allclose(mod.running_var.double().cpu(), m64.running_var, rtol=1e-5, atol=1e-6), k


# ---- (c) the whole network ------------------------------------------------------------------------------------------------------------------
def grad_errs(grads, ref):
    """max|g - g64| / max|g64| per parameter; the bias of a BatchNorm without a ReLU (conv0.0.1, conv.1.1: its constant is
    removed by the next training-mode BatchNorm, the true gradient is zero) and a head's conv bias over the magnitude of the
    same module's weight gradient"""
    out = {}
    for k, g64 in ref.items():
        den = g64.abs().max()
        if k.endswith((".conv0.0.1.bias", ".conv.1.1.bias")) or k in ("paf.bias", "heatmap.bias"):
            den = ref[k[:-4] + "weight"].abs().max()
        out[k] = ((grads[k].double().cpu() - g64).abs().max() / den).item()
    return out


def maps_of(size):
    """the stem (3x3, stride 2, padding 1), the ceil-mode 3x3 stride-2 pool, the stride-2 stage"""
    stem = (size - 1) // 2 + 1
    pool = (stem - 3 + 1) // 2 + 1
    return (pool - 1) // 2 + 1


@pytest.fixture(scope="module", params=[(72, 88), (36, 44)], ids=["72x88", "36x44"])
def net(request, cuda, train, encode, shuf):
    """The model, its inputs and one training forward + backward three ways; computed once, left unchanged."""
    ih, iw = request.param
    torch.manual_seed(0)
    base = dr.seed_module(shuf.Network(1.0), 7).train()
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, ih, iw, generator=g)
    mh, mw = maps_of(ih), maps_of(iw)
    heat, paf = torch.rand(2, 19, mh, mw, generator=g), torch.randn(2, 38, mh, mw, generator=g) * 0.5
    hmask = (torch.rand(2, 19, mh, mw, generator=g) > 0.2).float()
    pmask = (torch.rand(2, 38, mh, mw, generator=g) > 0.2).float()
    r = dict(base=base, x=x, maps=(mh, mw), size=(ih, iw))
    for name, dt in (("ref64", torch.float64), ("cpu32", torch.float32)):
        m = copy.deepcopy(base).to(dtype=dt)
        (p, h), saved = train.shufflenet_forward(m, x.to(dt), *dr.torch_ops())
        total, _ = encode.get_loss_shufflenet(saved, heat.to(dt), hmask.to(dt), paf.to(dt), pmask.to(dt))
        total.backward()
        r[name] = dict(paf=p.detach().double(), ht=h.detach().double(), stats={k: v.double() for k, v in stats_of(m).items()},
                       grads={n: q.grad.detach().double() for n, q in m.named_parameters()},
                       tracked={k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")})
    m = copy.deepcopy(base).to(cuda)
    dev = [t.to(cuda) for t in (x, heat, hmask, paf, pmask)]
    (p, h), saved = train.forward_train(m, dev[0])
    assert saved[0] is p and saved[1] is h and p.grad_fn is not None
    total, log = encode.get_loss_shufflenet(saved, *dev[1:])
    total.backward()
    r["native"] = dict(paf=p.detach(), ht=h.detach(), stats=stats_of(m), grads={n: q.grad.detach().clone() for n, q in m.named_parameters()},
                       tracked={k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}, log=log,
                       total=total.detach().clone())
    r["dev"] = dev
    return r


def test_forward_and_running_statistics_within_the_yardstick(net):
    ref, cpu, nat = net["ref64"], net["cpu32"], net["native"]
    report = {}
    for k, ch in (("paf", 38), ("ht", 19)):
        e_n, e_c = (nat[k].double().cpu() - ref[k]).abs().max().item(), (cpu[k] - ref[k]).abs().max().item()
        report[k] = {"native": e_n, "cpu32": e_c}
        assert tuple(nat[k].shape) == tuple(ref[k].shape) == (2, ch) + net["maps"] and e_n <= MARGIN * e_c, (k, e_n, e_c)
    rn = {k: norm_err(v, ref["stats"][k]) for k, v in nat["stats"].items()}
    rc = {k: norm_err(v, ref["stats"][k]) for k, v in cpu["stats"].items()}
    yard = max(rc.values())
    report["running_statistics"] = {"native": quantiles(rn), "cpu32": quantiles(rc)}
    # data/bn, the stem, 3 two-branch blocks of 5, 13 split blocks of 3, conv5
    assert len(rn) == 2 * sum(1 for m in net["base"].modules() if isinstance(m, nn.BatchNorm2d)) == 2 * (1 + 1 + 3 * 5 + 13 * 3 + 1)
    assert nat["tracked"] == ref["tracked"] and set(nat["tracked"].values()) == {1}
    # the gradients: recorded, not asserted (module docstring)
    gn, gc = grad_errs(nat["grads"], ref["grads"]), grad_errs(cpu["grads"], ref["grads"])
    report["parameter_gradients_not_asserted"] = {"native": quantiles(gn), "cpu32": quantiles(gc)}
    print("shufflenet 2x3x%dx%d:" % net["size"], report)
    cd.note("train_shufflenet_whole_network_%dx%d.json" % net["size"], report)
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
    total, log = encode.get_loss_shufflenet(saved, *net["dev"][1:])
    total.backward()
    assert torch.equal(total, net["native"]["total"]) and log == net["native"]["log"]
    for n, q in m.named_parameters():
        assert torch.equal(q.grad, grads[n]), n
    for k, v in stats_of(m).items():
        assert torch.equal(v, net["native"]["stats"][k]), k


def test_train_step_is_torch_sgd_on_the_native_gradients_and_inference_resyncs(net, shuf, cuda, train):
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
    fresh = shuf.Network(1.0)
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda).eval()
    with torch.no_grad():
        got, want = a.eval()(x)[0], fresh(x)[0]
    for i in range(2):
        assert tuple(got[i].shape[2:]) == net["maps"]
        assert torch.equal(got[i], want[i]), i
        assert not torch.equal(got[i], before[i])


def test_refusals(net, cuda, train):
    m = copy.deepcopy(net["base"]).to(cuda)
    x = net["dev"][0]
    with pytest.raises(RuntimeError, match=r"call \.train\(\) first"):
        train.forward_train(m.eval(), x)
    m.train()
    with pytest.raises(TypeError, match="freezes nothing of a shufflenet.Network"):
        train.freeze_trunk(m)
    with pytest.raises(RuntimeError, match="call .eval"):
        m(x)                                                     # model.forward, the inference plan, is untouched
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.forward_train(m, x.cpu())
