"""GPU suite of the layout-resident bf16 training of a shufflenet.Network: train.unit_chain and
forward_train / train_step(compute_dtype='bf16', resident='branch').

No rounding point moves against the per-op bf16 composition, so everything here is bit for bit:

(a) train.unit_chain against batch_norm(op(x, compute_dtype='bf16'), bn, relu) repeated L times, op being train.conv2d or
    train.dwconv3x3, on separate copies of the modules: the output, every gradient (None where none is required), the
    running means and variances and num_batches_tracked are torch.equal, over six requires_grad subsets of each run.  The
    runs: pointwise / depthwise stride 1 / pointwise at 2 x 5 x 7; depthwise stride 2 / pointwise 24 -> 10 at 2 x 7 x 9 (odd
    sizes, a width that is no multiple of 16); 58 channels with a depthwise stride 2 at 1 x 8 x 6; one pointwise unit
    20 -> 32 with a bias and a ReLU; and 3 x 5 x 5, whose 75 pixels make a partial second slab that starts inside the third
    image.  A played forward refusal falls back (every BatchNorm updated once, the composition's bits, unit_fallbacks == 1);
    a played data-gradient refusal is counted in bf16_fallbacks['dgrad'].
(b) the seeded shufflenet.Network(1.0) at 2 x 3 x 36 x 44 and 2 x 3 x 72 x 88: forward_train(resident='branch') +
    get_loss_shufflenet + backward against train.shufflenet_forward with the per-op bf16 callables - outputs, all gradients,
    all running statistics torch.equal, every fallback counter 0; one train_step equal to torch's SGD on those gradients
    bit for bit, and the inference plan reloads the stepped parameters and statistics.  The error of outputs and gradients
    against the float64 run is RECORDED (conv_driver.note), not asserted: a ReLU flip travels through the batch statistics
    (DESIGN.md 3.3g).  And the refusals of the keyword."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn

import conv_driver as cd
import dwconv_restate as dr
from test_train_hourglass_gpu import quantiles, stats_of
from test_train_shufflenet_gpu import grad_errs, maps_of

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


def reset_counters(train):
    train.reset_unit_fallbacks(), train.reset_bf16_fallbacks(), train.reset_chain_fallbacks()
    train.reset_dense_fallbacks(), train.reset_preact_fallbacks()


def counters(train):
    return dict(unit=train.unit_fallbacks, chain=train.chain_fallbacks, dense=train.dense_fallbacks, preact=train.preact_fallbacks,
                **train.bf16_fallbacks)


ZERO = dict(unit=0, chain=0, dense=0, preact=0, fwd=0, dgrad=0)


# ---- (a) unit_chain against the per-op composition ------------------------------------------------------------------------------------------
def pw(cin, cout, bias=False):
    return nn.Conv2d(cin, cout, 1, 1, 0, bias=bias)


def dw(c, stride):
    return nn.Conv2d(c, c, 3, stride, 1, groups=c, bias=False)


# name: (n, channels, h, w, [(op, relu)])
RUNS = {
    "pw_dw1_pw_2x5x7": (2, 12, 5, 7, lambda: [(pw(12, 12), True), (dw(12, 1), False), (pw(12, 12), True)]),
    "dw2_pw_2x7x9": (2, 24, 7, 9, lambda: [(dw(24, 2), False), (pw(24, 10), True)]),
    "pw_dw2_pw_58_1x8x6": (1, 58, 8, 6, lambda: [(pw(58, 58), True), (dw(58, 2), False), (pw(58, 58), True)]),
    "one_pw_20_32_relu": (2, 20, 5, 7, lambda: [(pw(20, 32, bias=True), True)]),
    "partial_slab_3x5x5": (3, 8, 5, 5, lambda: [(pw(8, 8), True), (dw(8, 1), False), (pw(8, 16, bias=True), False)]),
}
# what requires a gradient: x, the filters (and biases), the BatchNorm parameters; `top`: of the last unit only, x not - the
# walk stops there
SUBSETS = {"all": (True, True, True, False), "x": (True, False, False, False), "parameters": (False, True, True, False),
           "filters": (False, True, False, False), "batchnorms": (False, False, True, False), "top": (False, True, True, True)}


def build_run(name, seed=0):
    n, c, h, w, make = RUNS[name]
    torch.manual_seed(0)
    ops = make()
    mods = nn.ModuleList([nn.Sequential(m, nn.BatchNorm2d(m.out_channels)) for m, _ in ops])
    dr.seed_module(mods, 11 + seed).train()
    g = torch.Generator().manual_seed(200 + seed)
    x = torch.randn(n, c, h, w, generator=g)
    ho, wo = h, w
    for m, _ in ops:
        ho, wo = (ho - 1) // m.stride[0] + 1, (wo - 1) // m.stride[0] + 1
    gy = torch.randn(n, ops[-1][0].out_channels, ho, wo, generator=g)
    return mods, [r for _, r in ops], x, gy


def set_requires(mods, x, subset):
    need_x, need_f, need_bn, top = SUBSETS[subset]
    x.requires_grad_(need_x)
    for i, seq in enumerate(mods):
        on = not top or i == len(mods) - 1
        for p in seq[0].parameters():
            p.requires_grad_(need_f and on)
        for p in seq[1].parameters():
            p.requires_grad_(need_bn and on)


def composition(train, mods, relus, x):
    for seq, relu in zip(mods, relus):
        m = seq[0]
        if m.groups > 1:
            t = train.dwconv3x3(x, m.weight, m.stride[0], compute_dtype='bf16')
        else:
            t = train.conv2d(x, m.weight, m.bias, compute_dtype='bf16')
        x = train.batch_norm(t, seq[1], relu=relu)
    return x


def outcome(mods, x, y):
    out = {"y": y.detach().clone(), "dx": None if x.grad is None else x.grad.clone()}
    for k, p in mods.named_parameters():
        out["grad " + k] = None if p.grad is None else p.grad.clone()
    for k, v in mods.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out[k] = v.detach().clone()
    return out


def run_both(train, cuda, name, subset, chain=None):
    """(outcome of unit_chain - or of `chain(mods, relus, x)` -, outcome of the composition) on separate copies"""
    base, relus, x, gy = build_run(name)
    res = []
    for which in ("chain", "composition"):
        mods = copy.deepcopy(base).to(cuda)
        xd = x.to(cuda)
        set_requires(mods, xd, subset)
        if which == "composition":
            y = composition(train, mods, relus, xd)
        elif chain is None:
            y = train.unit_chain(xd, [(seq[0], seq[1], r) for seq, r in zip(mods, relus)])
        else:
            y = chain(mods, relus, xd)
        if y.requires_grad:
            y.backward(gy.to(cuda))
        res.append(outcome(mods, xd, y))
    return res


def assert_same(got, want):
    assert set(got) == set(want)
    for k in want:
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k] is not None and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("name", list(RUNS))
def test_unit_chain_equals_the_per_op_composition(cuda, train, name, subset):
    reset_counters(train)
    got, want = run_both(train, cuda, name, subset)
    assert_same(got, want)
    assert counters(train) == ZERO
    need_x, need_f, need_bn, top = SUBSETS[subset]
    grads = [k for k, v in want.items() if k.startswith("grad ") and v is not None]
    units = len(RUNS[name][4]())
    assert (want["dx"] is not None) == need_x and bool(grads) == (need_f or need_bn)
    if top:
        assert all(k.startswith("grad %d." % (units - 1)) for k in grads)
    assert all(int(v) == 1 for k, v in got.items() if k.endswith("num_batches_tracked"))


def test_the_partial_slab_run_is_what_its_name_says(capi):
    n, c, h, w, _ = RUNS["partial_slab_3x5x5"]
    assert capi.lib.rtpose_bn_slabs(c, n, h, w) == 2 and n * h * w == 75 and 64 % (h * w) != 0


def test_a_played_forward_refusal_falls_back(cuda, train, monkeypatch):
    """the second pointwise conv of pw -> dw -> pw is refused: the two BatchNorms updated so far are put back, the run goes
    through the composition, every BatchNorm is updated once"""
    reset_counters(train)
    calls = []
    real = train._unit_conv_into

    def refuse_second(*a, **kw):
        calls.append(1)
        return False if len(calls) == 2 else real(*a, **kw)

    monkeypatch.setattr(train, "_unit_conv_into", refuse_second)
    got, want = run_both(train, cuda, "pw_dw1_pw_2x5x7", "all")
    assert len(calls) == 2, "the node's own launches only: the fallback's conv2d nodes launch through their own name"
    assert_same(got, want)
    assert all(int(v) == 1 for k, v in got.items() if k.endswith("num_batches_tracked"))
    assert counters(train) == dict(ZERO, unit=1)
    train.reset_unit_fallbacks()
    assert train.unit_fallbacks == 0


def test_a_played_data_gradient_refusal_is_counted(cuda, train, monkeypatch):
    reset_counters(train)
    want = run_both(train, cuda, "pw_dw1_pw_2x5x7", "all")[1]

    def chain(mods, relus, x):
        y = train.unit_chain(x, [(seq[0], seq[1], r) for seq, r in zip(mods, relus)])
        monkeypatch.setattr(train, "_unit_conv_into", lambda *a, **kw: False)       # from here on: the backward's launches
        return y

    got = run_both(train, cuda, "pw_dw1_pw_2x5x7", "all", chain)[0]
    monkeypatch.undo()
    assert counters(train) == dict(ZERO, dgrad=2)          # both pointwise convs; the depthwise one has no such door
    # the same bf16 gradient convolved in fp32 on fp32 filters where the composition convolves it in bf16 on bf16 ones: every
    # gradient below a refused conv is another number of the same shape; what lies above both is untouched
    for k in want:
        if want[k] is not None and want[k].is_floating_point():
            assert got[k].shape == want[k].shape and torch.isfinite(got[k]).all(), k
    for k in ("y", "grad 2.0.weight", "grad 2.1.weight", "grad 2.1.bias"):
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["dx"], want["dx"])


def test_unit_chain_refusals(cuda, train, capi):
    x = torch.randn(2, 8, 5, 5, device=cuda)
    ok = [(pw(8, 8).to(cuda), nn.BatchNorm2d(8).to(cuda), True)]
    err = capi.RtposeError
    with pytest.raises(err, match="takes an NCHW fp32 input"):
        train.unit_chain(x.double(), ok)
    with pytest.raises(err, match="unit 0: the op is a pointwise nn.Conv2d"):
        train.unit_chain(x, [(nn.Conv2d(8, 8, 3, 1, 1).to(cuda), ok[0][1], True)])
    with pytest.raises(err, match="unit 1: fp32 filters on the 8 channels the unit before writes"):
        train.unit_chain(x, ok + [(pw(4, 8).to(cuda), nn.BatchNorm2d(8).to(cuda), True)])
    with pytest.raises(err, match="training mode"):
        train.unit_chain(x, [(ok[0][0], nn.BatchNorm2d(8).to(cuda).eval(), True)])
    with pytest.raises(err, match="takes an NCHW fp32 input with 4 channels"):
        train.unit_chain(x, [(ok[0][0], nn.BatchNorm2d(4).to(cuda), True)])
    with pytest.raises(err, match="runs only on an MI355X"):
        train.unit_chain(x, [(pw(8, 8), nn.BatchNorm2d(8), True)])
    with pytest.raises(err, match="more than 1 value per channel"):
        train.unit_chain(x[:1, :, :1, :1], ok)
    assert int(ok[0][1].num_batches_tracked) == 0


# ---- (b) the whole network -----------------------------------------------------------------------------------------------------------------
def per_op_bf16(train):
    """the four callables of train.shufflenet_forward: the per-op bf16 path"""
    return (lambda t, m: train.conv2d(t, m.weight, m.bias, compute_dtype='bf16'),
            lambda t, m, relu: train.batch_norm(t, m, relu=relu),
            lambda t, m: train.dwconv3x3(t, m.weight, m.stride[0], compute_dtype='bf16'),
            lambda t, m: train.conv3x3_s2(t, m.weight))


def one_run(model, forward, encode, dev):
    (p, h), saved = forward(model, dev[0])
    total, log = encode.get_loss_shufflenet(saved, *dev[1:])
    total.backward()
    return dict(paf=p.detach(), ht=h.detach(), total=total.detach().clone(), log=log, stats=stats_of(model),
                grads={n: q.grad.detach().clone() for n, q in model.named_parameters()},
                tracked={k: int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")})


@pytest.fixture(scope="module", params=[(36, 44), (72, 88)], ids=["36x44", "72x88"])
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
    host = (x, heat, hmask, paf, pmask)
    dev = [t.to(cuda) for t in host]
    r = dict(base=base, maps=(mh, mw), size=(ih, iw), dev=dev)
    m64 = copy.deepcopy(base).double()
    r["ref64"] = one_run(m64, lambda m, t: train.shufflenet_forward(m, t, *dr.torch_ops()), encode, [t.double() for t in host])
    reset_counters(train)
    r["per_op"] = one_run(copy.deepcopy(base).to(cuda), lambda m, t: train.shufflenet_forward(m, t, *per_op_bf16(train)), encode, dev)
    r["per_op_counters"] = counters(train)
    reset_counters(train)
    r["branch"] = one_run(copy.deepcopy(base).to(cuda),
                          lambda m, t: train.forward_train(m, t, compute_dtype='bf16', resident='branch'), encode, dev)
    r["branch_counters"] = counters(train)
    return r


def test_the_network_equals_the_per_op_bf16_path_bit_for_bit(net):
    got, want = net["branch"], net["per_op"]
    assert net["branch_counters"] == ZERO and net["per_op_counters"] == ZERO
    assert tuple(got["paf"].shape) == (2, 38) + net["maps"] and tuple(got["ht"].shape) == (2, 19) + net["maps"]
    assert torch.equal(got["paf"], want["paf"]) and torch.equal(got["ht"], want["ht"]) and torch.equal(got["total"], want["total"])
    assert got["log"] == want["log"]
    assert set(got["grads"]) == set(want["grads"]) == set(dict(net["base"].named_parameters()))
    for k, g in want["grads"].items():
        assert torch.isfinite(g).all() and torch.equal(got["grads"][k], g), k
    assert len(want["stats"]) == 2 * (1 + 1 + 3 * 5 + 13 * 3 + 1)
    for k, v in want["stats"].items():
        assert torch.equal(got["stats"][k], v), k
    assert got["tracked"] == want["tracked"] and set(got["tracked"].values()) == {1}


def test_the_error_against_float64_is_recorded(net):
    """recorded, not asserted: one ReLU sign flip reaches every parameter through the batch statistics"""
    ref, got = net["ref64"], net["branch"]
    report = {k: (got[k].double().cpu() - ref[k]).abs().max().item() / ref[k].abs().max().item() for k in ("paf", "ht")}
    report["parameter_gradients"] = quantiles(grad_errs(got["grads"], ref["grads"]))
    print("shufflenet bf16 resident='branch' 2x3x%dx%d against float64:" % net["size"], report)
    cd.note("train_branch_whole_network_%dx%d.json" % net["size"], report)


def test_train_step_is_torch_sgd_on_those_gradients_and_inference_resyncs(net, shuf, cuda, train):
    x, heat, hmask, paf, pmask = net["dev"]
    reset_counters(train)
    a = copy.deepcopy(net["base"]).to(cuda)
    with torch.no_grad():
        before = a.eval()(x)[0]                                  # packs the inference arena from the initial parameters
    a.train()
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf, heat_mask=hmask, paf_mask=pmask, compute_dtype='bf16', resident='branch')
    assert torch.equal(total.detach(), net["branch"]["total"]) and list(log)[:2] == ["paf", "heatmap"]
    assert counters(train) == ZERO
    b = copy.deepcopy(net["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = net["branch"]["grads"][n].clone()
    opt_b.step()
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n
    for k, v in stats_of(a).items():
        assert torch.equal(v, net["branch"]["stats"][k]), k
    # inference after the step: the plan folds the UPDATED running statistics (written through raw pointers) and parameters
    fresh = shuf.Network(1.0)
    fresh.load_state_dict(a.state_dict())
    fresh = fresh.to(cuda).eval()
    with torch.no_grad():
        got, want = a.eval()(x)[0], fresh(x)[0]
    for i in range(2):
        assert torch.equal(got[i], want[i]), i
        assert not torch.equal(got[i], before[i])


def test_the_keyword_refuses(net, pkg, cuda, train, capi):
    openpose = importlib.import_module(pkg.__name__ + ".openpose")
    hourglass = importlib.import_module(pkg.__name__ + ".hourglass")
    x = net["dev"][0]
    m = copy.deepcopy(net["base"]).to(cuda)
    err = capi.RtposeError
    with pytest.raises(err, match="resident='branch' needs compute_dtype='bf16'.*fp32 node is not built"):
        train.forward_train(m, x, resident='branch')
    with pytest.raises(err, match=r"resident='branch' is the training-mode forward.*call \.train\(\) first"):
        train.forward_train(m.eval(), x, compute_dtype='bf16', resident='branch')
    m.train()
    with pytest.raises(err, match="no CPU fallback"):
        train.forward_train(m, x.cpu(), compute_dtype='bf16', resident='branch')
    with pytest.raises(err, match="BatchNorm and depthwise kernels"):
        train.forward_train(m, x, compute_dtype='bf16')
    with pytest.raises(err, match="resident is False, True or 'dense'; got 'Branch'.*'bottleneck' is.*'branch' their fifth"):
        train.forward_train(m, x, resident='Branch')
    others = (pkg.get_model('vgg19'), openpose.OpenPose_Model(2, 2, 52, 26),
              hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3))
    for other in others:
        with pytest.raises(err, match="resident='branch' is for a shufflenet.Network only.*%s" % type(other).__name__):
            train.forward_train(other.to(cuda), x, compute_dtype='bf16', resident='branch')
    assert all(int(v) == 0 for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")), "a refused call ran a BatchNorm"
