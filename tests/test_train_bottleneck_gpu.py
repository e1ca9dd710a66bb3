"""GPU suite of the layout-resident bf16 Bottleneck (train.preact_chain; resident='bottleneck' of train.forward_train and
train.train_step on an hourglass.HourglassNet).

The contract is bit equality with the per-conv bf16 composition conv2d(batch_norm(x, bn, relu=True), w, b, compute_dtype='bf16')
repeated L times - the output, every gradient, the running statistics and num_batches_tracked with torch.equal -, for the main
branches of the network's Bottlenecks, a k = 7, 3, 1 run and L = 1, over the requires_grad subsets whose walks differ; for a
played refusal of a forward conv (the fallback, counted, statistics updated once); and for the whole network against
train.hourglass_forward with the per-conv bf16 callables.  The parts carry their own error bounds
(tests/test_batchnorm_gpu.py, tests/test_conv_backward_bf16_gpu.py); the node's error against torch float64 is recorded next
to the fp32 native path's through conv_driver.note, not asserted."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_driver as cd
import hourglass_train_restate as htr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


@pytest.fixture(scope="module")
def hgm(pkg):
    return importlib.import_module(pkg.__name__ + ".hourglass")


def counters(train):
    return dict(train.bf16_fallbacks, chain=train.chain_fallbacks, dense=train.dense_fallbacks, preact=train.preact_fallbacks)


def reset(train):
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()
    train.reset_dense_fallbacks()
    train.reset_preact_fallbacks()


NONE = {'fwd': 0, 'dgrad': 0, 'chain': 0, 'dense': 0, 'preact': 0}

# (name, widths, kernel sizes, n, h, w): the main branches of the network's Bottlenecks - the third with P = 70, a partial slab
# across an image boundary, the fourth with widths that are no multiples of 4 (the element-wise path of every pass and pad
# channels in every bf16 buffer) -, a k = 7, 3, 1 run and a single triple
SPECS = [("b64_2x16x16", (64, 64, 64, 128), (1, 3, 1), 2, 16, 16),
         ("b256_2x4x4", (256, 128, 128, 256), (1, 3, 1), 2, 4, 4),
         ("b64_2x5x7", (64, 32, 32, 64), (1, 3, 1), 2, 5, 7),
         ("b38_2x5x7", (38, 19, 19, 38), (1, 3, 1), 2, 5, 7),
         ("k731_1x6x6", (16, 16, 16, 16), (7, 3, 1), 1, 6, 6),
         ("single_2x5x7", (24, 40), (3,), 2, 5, 7)]
SUBSETS = ("all", "x_only", "last_triple_only", "bn_frozen", "first_triple_frozen", "x_not_required")


def make_run(spec, seed=0):
    """(x, gy, [(BatchNorm2d, weight, bias)]) on the CPU: He-scaled filters, BatchNorm weights in [0.5, 1.5), running
    statistics that are not the initial ones"""
    _, widths, ks, n, h, w = spec
    g = torch.Generator().manual_seed(500 + seed)
    layers = []
    for i, k in enumerate(ks):
        cin, cout = widths[i], widths[i + 1]
        bn = nn.BatchNorm2d(cin)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(cin, generator=g) + 0.5), bn.bias.copy_(torch.randn(cin, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(cin, generator=g)), bn.running_var.copy_(torch.rand(cin, generator=g) + 0.5)
        wt = nn.Parameter(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        b = nn.Parameter(torch.randn(cout, generator=g) * 0.05)
        layers.append((bn.train(), wt, b))
    x = torch.randn(n, widths[0], h, w, generator=g) * 1.5 + 0.3
    return x, torch.randn(n, widths[-1], h, w, generator=g), layers


def on_device(layers, dev, subset):
    """a deep copy of the triples on the device with the subset's requires_grad flags"""
    out = []
    L = len(layers)
    for i, (bn, wt, b) in enumerate(layers):
        bn, wt, b = copy.deepcopy(bn).to(dev), nn.Parameter(wt.detach().clone().to(dev)), nn.Parameter(b.detach().clone().to(dev))
        conv_on = subset not in ("x_only",) and not (subset == "last_triple_only" and i < L - 1) \
            and not (subset == "first_triple_frozen" and i == 0)
        bn_on = conv_on and subset != "bn_frozen"
        wt.requires_grad_(conv_on), b.requires_grad_(conv_on)
        bn.weight.requires_grad_(bn_on), bn.bias.requires_grad_(bn_on)
        out.append((bn, wt, b))
    return out


def needs_x(subset):
    return subset in ("all", "x_only", "bn_frozen")


def composition(train, x, layers):
    for bn, wt, b in layers:
        x = train.conv2d(train.batch_norm(x, bn, relu=True), wt, b, compute_dtype='bf16')
    return x


def native_fp32(train, x, layers):
    for bn, wt, b in layers:
        x = train.conv2d(train.batch_norm(x, bn, relu=True), wt, b)
    return x


def run(fn, x, gy, layers, dev, subset):
    """(y, {name: grad or None}, {name: statistic}) of one forward + backward"""
    layers = on_device(layers, dev, subset)
    xd = x.to(dev).requires_grad_(needs_x(subset))
    y = fn(xd, layers)
    if y.requires_grad:
        y.backward(gy.to(dev))
    grads = {"x": xd.grad}
    stats = {}
    for i, (bn, wt, b) in enumerate(layers):
        grads.update({"bn%d.weight" % i: bn.weight.grad, "bn%d.bias" % i: bn.bias.grad, "conv%d.weight" % i: wt.grad,
                      "conv%d.bias" % i: b.grad})
        stats.update({"bn%d.running_mean" % i: bn.running_mean.clone(), "bn%d.running_var" % i: bn.running_var.clone(),
                      "bn%d.num_batches_tracked" % i: bn.num_batches_tracked.clone()})
    return y.detach(), grads, stats


def assert_equal(what, got, want):
    y, grads, stats = got
    y2, grads2, stats2 = want
    assert y.dtype == torch.float32 and torch.equal(y, y2), "%s: the output differs in %d elements" % (what, int((y != y2).sum()))
    assert set(grads) == set(grads2)
    for k, g in grads.items():
        assert (g is None) == (grads2[k] is None), "%s: %s" % (what, k)
        if g is not None:
            assert g.dtype == torch.float32 and g.shape == grads2[k].shape, k
            assert torch.equal(g, grads2[k]), "%s: %s differs in %d of %d elements" % (what, k, int((g != grads2[k]).sum()), g.numel())
    for k, v in stats.items():
        assert torch.equal(v, stats2[k]), "%s: %s" % (what, k)


# ---- 1. the node against the per-conv composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", SUBSETS)
@pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])
def test_preact_chain_equals_the_per_conv_composition(cuda, train, spec, subset):
    x, gy, layers = make_run(spec)
    reset(train)
    want = run(lambda t, ls: composition(train, t, ls), x, gy, layers, cuda, subset)
    got = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, subset)
    assert counters(train) == NONE
    assert_equal("%s %s" % (spec[0], subset), got, want)
    L = len(layers)
    assert all(int(got[2]["bn%d.num_batches_tracked" % i]) == 1 for i in range(L))
    required = {k for k, g in got[1].items() if g is not None}
    if subset == "all":
        assert len(required) == 4 * L + 1
    elif subset == "x_only":
        assert required == {"x"}
    elif subset == "last_triple_only":
        assert required == {"%s%d.%s" % (m, L - 1, p) for m in ("bn", "conv") for p in ("weight", "bias")}
    elif subset == "bn_frozen":
        assert required == {"x"} | {k for k in got[1] if k.startswith("conv")}
    elif subset == "first_triple_frozen":
        assert required == {k for k in got[1] if k != "x" and not k.startswith(("bn0.", "conv0."))}
    else:
        assert required == {k for k in got[1] if k != "x"}


def test_two_runs_give_the_same_bits(cuda, train):
    x, gy, layers = make_run(SPECS[2], seed=1)
    a = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, "all")
    b = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, "all")
    assert_equal("second run", b, a)


def test_a_list_of_lists_and_an_epoch_are_taken(cuda, train):
    x, gy, layers = make_run(SPECS[5])
    want = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, "all")
    got = run(lambda t, ls: train.preact_chain(t, [list(l) for l in ls], epoch=3, resync=True), x, gy, layers, cuda, "all")
    assert_equal("lists, epoch 3, resync", got, want)


# ---- 2. the error against float64: recorded, not asserted -----------------------------------------------------------------------------
@pytest.mark.parametrize("spec", SPECS[:2], ids=[s[0] for s in SPECS[:2]])
def test_error_against_float64_is_recorded(cuda, train, spec):
    x, gy, layers = make_run(spec)
    ls64 = [(copy.deepcopy(bn).double(), wt.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True))
            for bn, wt, b in layers]
    x64 = x.double().requires_grad_(True)
    t = x64
    for bn, wt, b in ls64:
        t = F.conv2d(F.relu(F.batch_norm(t, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)), wt, b,
                     padding=wt.shape[2] // 2)
    t.backward(gy.double())
    ref = {"x": x64.grad}
    for i, (bn, wt, b) in enumerate(ls64):
        ref.update({"bn%d.weight" % i: bn.weight.grad, "bn%d.bias" % i: bn.bias.grad, "conv%d.weight" % i: wt.grad,
                    "conv%d.bias" % i: b.grad})
    report = {}
    for name, fn in (("preact_chain_bf16", lambda a, ls: train.preact_chain(a, ls)), ("native_fp32", lambda a, ls: native_fp32(train, a, ls))):
        y, grads, _ = run(fn, x, gy, layers, cuda, "all")
        assert torch.isfinite(y).all() and all(torch.isfinite(g).all() for g in grads.values())
        err = {"forward": ((y.double().cpu() - t.detach()).abs().max() / t.detach().abs().max()).item()}
        for k, g64 in ref.items():
            den = g64.abs().max()
            if k.startswith("conv") and k.endswith(".bias") and int(k[4]) < len(layers) - 1:   # in front of a BatchNorm: true gradient zero
                den = ref[k[:-4] + "weight"].abs().max()
            err[k] = ((grads[k].double().cpu() - g64).abs().max() / den).item()
        report[name] = err
    print("preact_chain %s: max|err| / max|ref| against float64: %s" % (spec[0], report))
    cd.note("train_bottleneck_float64_%s.json" % spec[0], report)


# ---- 3. fallbacks ---------------------------------------------------------------------------------------------------------------------
def test_a_refused_forward_conv_falls_back_and_updates_the_statistics_once(cuda, train, monkeypatch):
    """rtpose_conv2d_bf16 refuses none of the shapes at hand, so the refusal is played: train._preact_conv_into answers False
    (what it answers when the launcher returns RTPOSE_E_INVAL before launching) for the second forward conv - after the
    node has updated the running statistics of two BatchNorms"""
    x, gy, layers = make_run(SPECS[2])
    reset(train)
    want = run(lambda t, ls: composition(train, t, ls), x, gy, layers, cuda, "all")
    real, calls = train._preact_conv_into, []

    def conv_into(bf16, *a, **kw):
        calls.append(len(calls))
        return False if calls[-1] == 1 else real(bf16, *a, **kw)

    monkeypatch.setattr(train, "_preact_conv_into", conv_into)
    got = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, "all")
    monkeypatch.setattr(train, "_preact_conv_into", real)
    assert len(calls) == 2 and counters(train) == dict(NONE, preact=1)
    assert_equal("after the fallback", got, want)
    assert all(int(got[2]["bn%d.num_batches_tracked" % i]) == 1 for i in range(3))
    reset(train)


def test_refused_data_gradients_are_counted(cuda, train, monkeypatch):
    x, gy, layers = make_run(SPECS[2])
    L = len(layers)
    reset(train)
    want = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, "all")
    real, calls = train._preact_conv_into, []

    def conv_into(bf16, *a, **kw):
        calls.append(len(calls))
        return False if calls[-1] >= L else real(bf16, *a, **kw)

    monkeypatch.setattr(train, "_preact_conv_into", conv_into)
    got = run(lambda t, ls: train.preact_chain(t, ls), x, gy, layers, cuda, "all")
    monkeypatch.setattr(train, "_preact_conv_into", real)
    assert len(calls) == 2 * L and counters(train) == dict(NONE, dgrad=L)
    # what no data gradient feeds is untouched; the rest comes from fp32 convs on the widened gradient and the fp32 filters
    # (the bits differ: the filters are not rounded there) and is only held to be finite
    assert torch.equal(got[0], want[0])
    for k in ("conv%d.weight" % (L - 1), "conv%d.bias" % (L - 1)):
        assert torch.equal(got[1][k], want[1][k]), k
    for k, g in got[1].items():
        assert g.shape == want[1][k].shape and torch.isfinite(g).all(), k
    reset(train)


# ---- 4. the whole network -------------------------------------------------------------------------------------------------------------
TOPO = dict(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3)


def stats_of(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


@pytest.fixture(scope="module")
def net(cuda, train, encode, hgm):
    """hg(1, 1, 4, 3) at 2 x 3 x 64 x 64 (the deepest BatchNorms see P = 2): one forward + backward through
    resident='bottleneck' and one through hourglass_forward with the per-conv bf16 callables; computed once, left unchanged"""
    torch.manual_seed(0)
    base = htr.seed_model(hgm.hg(**TOPO), 7).train()
    g = torch.Generator().manual_seed(41)
    x = torch.randn(2, 3, 64, 64, generator=g)
    heat, paf = torch.rand(2, 3, 16, 16, generator=g), torch.randn(2, 4, 16, 16, generator=g) * 0.5
    hmask = (torch.rand(2, 3, 16, 16, generator=g) > 0.2).float()
    pmask = (torch.rand(2, 4, 16, 16, generator=g) > 0.2).float()
    dev = [t.to(cuda) for t in (x, heat, hmask, paf, pmask)]
    r = dict(base=base, dev=dev)

    def finish(m, out):
        (p, h), saved = out
        assert saved[0] is p and saved[1] is h and p.grad_fn is not None
        total, log = encode.get_loss_hourglass(saved, *dev[1:])
        total.backward()
        return dict(paf=p.detach(), ht=h.detach(), total=total.detach().clone(), log=log, stats=stats_of(m),
                    grads={n: q.grad.detach().clone() for n, q in m.named_parameters()})

    reset(train)
    m = copy.deepcopy(base).to(cuda)
    r["resident"] = finish(m, train.forward_train(m, dev[0], compute_dtype='bf16', resident='bottleneck'))
    r["resident_counters"] = counters(train)
    reset(train)
    m = copy.deepcopy(base).to(cuda)
    conv = lambda t, c: train.conv2d(t, c.weight, c.bias, compute_dtype='bf16')                         # noqa: E731
    r["per_conv"] = finish(m, train.hourglass_forward(m, dev[0], conv, lambda t, b: train.batch_norm(t, b, relu=True),
                                                      lambda t, c: train.conv7x7_s2(t, c.weight, c.bias)))
    r["per_conv_counters"] = counters(train)
    reset(train)
    return r


def test_whole_network_equals_the_per_conv_bf16_forward(net):
    a, b = net["resident"], net["per_conv"]
    assert net["resident_counters"] == NONE and net["per_conv_counters"] == NONE
    assert torch.equal(a["paf"], b["paf"]) and torch.equal(a["ht"], b["ht"]) and torch.equal(a["total"], b["total"])
    assert tuple(a["paf"].shape) == (2, 4, 16, 16) and tuple(a["ht"].shape) == (2, 3, 16, 16) and a["log"] == b["log"]
    params = dict(net["base"].named_parameters())
    assert set(a["grads"]) == set(b["grads"]) == set(params)
    for n, g in a["grads"].items():
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), n
        assert torch.equal(g, b["grads"][n]), "%s differs in %d of %d elements" % (n, int((g != b["grads"][n]).sum()), g.numel())
    assert all(g.abs().max() > 0 for n, g in a["grads"].items() if n.endswith("weight"))
    assert set(a["stats"]) == set(b["stats"])
    for k, v in a["stats"].items():
        assert torch.equal(v, b["stats"][k]), k
    tracked = [int(v) for k, v in a["stats"].items() if k.endswith("num_batches_tracked")]
    assert len(tracked) == sum(1 for m in net["base"].modules() if isinstance(m, nn.BatchNorm2d)) and set(tracked) == {1}


def test_train_step_is_torch_sgd_on_those_gradients_and_inference_resyncs(net, hgm, cuda, train):
    x, heat, hmask, paf, pmask = net["dev"]
    a = copy.deepcopy(net["base"]).to(cuda)
    with torch.no_grad():
        before = a.eval()(x)[0]                                  # packs the inference arena from the initial parameters
    a.train()
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    reset(train)
    total, log = train.train_step(a, opt_a, x, heat, paf, heat_mask=hmask, paf_mask=pmask, compute_dtype='bf16',
                                  resident='bottleneck')
    assert counters(train) == NONE
    assert torch.equal(total.detach(), net["resident"]["total"]) and list(log)[:2] == ["paf", "heatmap"]
    b = copy.deepcopy(net["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = net["resident"]["grads"][n].clone()
    opt_b.step()
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
    for k, v in stats_of(a).items():
        assert torch.equal(v, net["resident"]["stats"][k]), k
    # inference after the step: the plan folds the UPDATED running statistics (written through raw pointers) and parameters
    fresh = hgm.hg(**TOPO)
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda).eval()
    with torch.no_grad():
        got, want = a.eval()(x)[0], fresh(x)[0]
    for i in range(2):
        assert torch.equal(got[i], want[i]), i
        assert not torch.equal(got[i], before[i])


def test_refusals(net, pkg, cuda, train):
    capi = importlib.import_module(pkg.__name__ + "._capi")
    m = copy.deepcopy(net["base"]).to(cuda)
    x = net["dev"][0]
    with pytest.raises(capi.RtposeError, match=r"call \.train\(\) first"):
        train.forward_train(m.eval(), x, compute_dtype='bf16', resident='bottleneck')
    m.train()
    with pytest.raises(capi.RtposeError, match="resident='bottleneck' needs compute_dtype='bf16'.*fp32 node is not built"):
        train.forward_train(m, x, resident='bottleneck')
    with pytest.raises(capi.RtposeError, match="must not require a gradient"):
        train.forward_train(m, x.clone().requires_grad_(True), compute_dtype='bf16', resident='bottleneck')
    with pytest.raises(capi.RtposeError, match="BatchNorm kernels"):
        train.forward_train(m, x, compute_dtype='bf16')          # without the keyword a HourglassNet still takes no 'bf16'
    openpose = importlib.import_module(pkg.__name__ + ".openpose")
    shufflenet = importlib.import_module(pkg.__name__ + ".shufflenet")
    for other in (pkg.get_model('vgg19'), openpose.OpenPose_Model(2, 2, 52, 26), shufflenet.Network()):
        for dt in ('bf16', 'fp32'):
            with pytest.raises(capi.RtposeError, match="resident='bottleneck' is for an hourglass.HourglassNet only"):
                train.forward_train(other, x, compute_dtype=dt, resident='bottleneck')
    with pytest.raises(capi.RtposeError, match="resident is False, True or 'dense'; got 'Bottleneck'.*'bottleneck' is"):
        train.forward_train(m, x, resident='Bottleneck')
