"""GPU suite of mixed-precision training, train.py's compute_dtype='bf16': bf16 operands of all three convs of a layer
(rtpose_conv2d_bf16 forward and data gradient, rtpose_conv2d_wgrad_bf16), fp32 accumulation, fp32 parameters.

The reference project has no reduced-precision training; the contract is conv_backward_bf16_restate.EmulConv, which states
the rounding points in float64 on the CPU.

* Exact operands (integers bf16 holds, every sum below 2^24): outputs and every gradient torch.equal the float64 graph.
* Rounded operands, one layer: y, dx, dw, db within 2 gamma_(n+1) S of EmulConv fed the same tensors, n the terms of the
  sum and S the sum of their absolute values (the factor 2: tests/test_conv_backward_bf16_gpu.py).  The ReLU mask is taken
  from the native y, so no bound hinges on a y that rounds to either side of zero.
* Chains and whole networks: r(p) = max|g - g64| / max|g64| against the UNROUNDED float64 graph, required
  r_native(p) <= 4 max_q r_emul(q) with r_emul the same quantity for the model run through EmulConv on the CPU - the yardstick is
  the arithmetic's own error, not the code under test; the margin 4 is test_train_gpu.py's for two equally precise paths that
  differ in summation order, a few ReLU decisions and, here, a few re-roundings.  Both ratios go through conv_driver.note."""
import copy
import importlib
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_backward_bf16_restate as cb
import conv_driver as cd
from conv_backward_restate import Case as Shape, exact_margin

pytestmark = pytest.mark.gpu

MARGIN = 4.0


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(pkg.__name__ + ".encode")


@pytest.fixture(scope="module")
def openpose(pkg):
    return importlib.import_module(pkg.__name__ + ".openpose")


def shape(k, cin, cout, n, h, w):
    return Shape(k, cin, cout, n, h, w, 0, 0, "")


def subsets(names):
    return ["".join(s) for r in range(1, len(names) + 1) for s in itertools.combinations(names, r)]


# ---- (a) exact operands -------------------------------------------------------------------------------------------------------------
RELU_SHAPES = [shape(3, 9, 8, 2, 5, 3), shape(7, 3, 5, 3, 19, 18), shape(1, 70, 66, 1, 1, 1), shape(1, 9, 8, 3, 19, 18)]


def exact_graph(s, req, conv, act, dev, dt, slopes=None):
    x, G, wt, b = (t.to(device=dev, dtype=dt) for t in cb.exact_tensors(s, seed=s.k + s.cin + 1))
    leaves = {"x": x.requires_grad_("x" in req), "w": wt.requires_grad_("w" in req), "b": b.requires_grad_("b" in req)}
    if slopes is not None:
        leaves["a"] = slopes.to(device=dev, dtype=dt).requires_grad_("a" in req)
    y = act(conv, leaves)
    (y * G).sum().backward()
    return y.detach(), {n: t.grad for n, t in leaves.items()}


def same_as_float64(y, g, y64, g64, req):
    assert y.dtype == torch.float32 and torch.equal(y.double().cpu(), y64), "y"
    for n in g:
        if n in req:
            assert g[n] is not None and g[n].dtype == torch.float32 and g[n].shape == g64[n].shape
            wrong = int((g[n].double().cpu() != g64[n]).sum())
            assert torch.equal(g[n].double().cpu(), g64[n]), "d%s: %d of %d elements differ" % (n, wrong, g64[n].numel())
            assert g64[n].abs().max().item() > 0
        else:
            assert g[n] is None and g64[n] is None, n


@pytest.mark.parametrize("req", subsets("xwb"))
@pytest.mark.parametrize("s", RELU_SHAPES, ids=cb.case_id)
def test_conv2d_bf16_exact_with_relu_and_bias(cuda, train, s, req):
    """integers up to 3 as operands: bf16 holds them, so the bf16 path must give the float64 graph's values, bit for bit"""
    assert 4 * exact_margin(s, seed=s.k + s.cin + 1) < 2 ** 24
    y64, g64 = exact_graph(s, req, None, lambda _, l: F.relu(F.conv2d(l["x"], l["w"], l["b"], padding=s.k // 2)), "cpu",
                           torch.float64)
    train.reset_bf16_fallbacks()
    y, g = exact_graph(s, req, None, lambda _, l: train.conv2d(l["x"], l["w"], l["b"], True, compute_dtype='bf16'), cuda,
                       torch.float32)
    same_as_float64(y, g, y64, g64, req)
    assert train.bf16_fallbacks == {'fwd': 0, 'dgrad': 0}


@pytest.mark.parametrize("req", subsets("xwba"))
def test_conv2d_bf16_exact_with_prelu(cuda, train, req):
    """the 15 requires_grad subsets of (x, w, b, slopes): integer slopes of both signs keep every value an integer bf16 holds"""
    s = shape(3, 9, 8, 2, 5, 3)
    slopes = torch.tensor([2.0, -1.0, 0.0, -2.0, 1.0, 2.0, -1.0, 1.0])
    y64, g64 = exact_graph(s, req, None, lambda _, l: F.prelu(F.conv2d(l["x"], l["w"], l["b"], padding=1), l["a"]), "cpu",
                           torch.float64, slopes)
    train.reset_bf16_fallbacks()
    y, g = exact_graph(s, req, None, lambda _, l: train.conv2d(l["x"], l["w"], l["b"], prelu=l["a"], compute_dtype='bf16'),
                       cuda, torch.float32, slopes)
    same_as_float64(y, g, y64, g64, req)
    assert train.bf16_fallbacks == {'fwd': 0, 'dgrad': 0}


def test_operands_bf16_does_not_hold_are_rounded(cuda, train):
    """an input holding 257 gives the float64 conv of rb(x) = 256, not of x: the path really rounds; so for a filter 1 + 2^-8"""
    s = shape(3, 9, 8, 2, 5, 3)
    x, G, wt, b = cb.exact_tensors(s)
    x[:, 1] = 257.0
    wt[0, 0] = 1.0 + 2.0 ** -8
    assert not torch.equal(cb.rb(x), x) and not torch.equal(cb.rb(wt), wt)
    want = F.conv2d(cb.rb(x).double(), cb.rb(wt).double(), b.double(), padding=1)
    unrounded = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    xd, wd = x.to(cuda), wt.to(cuda).requires_grad_(True)
    y = train.conv2d(xd, wd, b.to(cuda), compute_dtype='bf16')
    assert torch.equal(y.double().cpu(), want) and not torch.equal(want, unrounded)
    (y * G.to(cuda)).sum().backward()
    assert torch.equal(wd.grad.double().cpu(), cb.wgrad64(cb.rb(x), G, 3)[0])          # the kept input is the rounded one
    y32 = train.conv2d(xd, wd, b.to(cuda))
    assert torch.equal(y32.double().cpu(), unrounded)                                  # 257 and 1 + 2^-8 are fp32 values


# ---- (b) one random layer -----------------------------------------------------------------------------------------------------------
def within(name, got, want, bound, note):
    err = (got.double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    note[name + "_err_over_bound"] = ratio
    print("  %s: worst err / bound %.4g" % (name, ratio))
    assert (err <= bound).all(), "%s: worst err / bound %g" % (name, ratio)


LAYERS = [(3, 24, 38), (7, 185, 128), (1, 128, 19)]


@pytest.mark.parametrize("k,cin,cout", LAYERS, ids=["k%d_%dto%d" % l for l in LAYERS])
def test_one_layer_against_the_emulation(cuda, train, k, cin, cout):
    n, h, w = 2, 9, 7
    g = torch.Generator().manual_seed(100 + k)
    x, gy = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)
    wt, b = cd.weights("he", cout, cin, k, g), torch.randn(cout, generator=g) * 0.1
    xd, wd, bd = (t.to(cuda).requires_grad_(True) for t in (x, wt, b))
    train.reset_bf16_fallbacks()
    y = train.conv2d(xd, wd, bd, True, compute_dtype='bf16')
    y.backward(gy.to(cuda))
    mask = (y > 0).cpu()
    xe, we, be = (t.double().requires_grad_(True) for t in (x, wt, b))
    ye = cb.emul_conv(xe, we, be, True, mask=mask)
    ye.backward(gy.double())
    xr, wr, gr = cb.rb(x).double(), cb.rb(wt).double(), cb.rb(gy * mask).double()
    note = {"fallbacks": dict(train.bf16_fallbacks)}
    print("layer k%d %d -> %d, fallbacks %s" % (k, cin, cout, train.bf16_fallbacks))
    s_y = F.conv2d(xr.abs(), wr.abs(), b.double().abs(), padding=k // 2)
    within("y", y.detach(), ye.detach(), 2 * cb.gamma(cin * k * k + 2) * s_y, note)
    within("dx", xd.grad, xe.grad, 2 * cb.gamma(cout * k * k + 1) * cb.dgrad64(gr, wr)[1], note)
    within("dw", wd.grad, we.grad, 2 * cb.gamma(n * h * w + 1) * cb.wgrad64(xr, gr, k)[1], note)
    within("db", bd.grad, be.grad, 2 * cb.gamma(n * h * w + 1) * cb.dbias64(gr)[1], note)
    cd.note("train_bf16_layer_k%d_%dto%d.json" % (k, cin, cout), note)


def test_prelu_layer_against_the_emulation(cuda, train):
    """slopes of both signs.  The native gradient through the PReLU is fp32 - gz = z > 0 ? gy : fp32(slope * gy), one rounding
    per product (header, rtpose_prelu_grad) - and is stated so here, on the signs of the emulated z; the conv behind it is
    EmulConv without an activation, the forward's PReLU float64 F.prelu.  dslope = sum over z <= 0 of z gy has the native z in
    it, which is within e_z = 2 gamma_(K+2) S_z of the emulated one: |err| <= sum |gy| e_z + gamma_(n+1) sum |z gy|."""
    k, cin, cout, n, h, w = 3, 24, 38, 2, 9, 7
    g = torch.Generator().manual_seed(77)
    x, gy = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cout, h, w, generator=g)
    wt, b = cd.weights("he", cout, cin, k, g), torch.randn(cout, generator=g) * 0.1
    a = torch.randn(cout, generator=g) * 0.25
    assert (a > 0).any() and (a < 0).any()
    xd, wd, bd, ad = (t.to(cuda).requires_grad_(True) for t in (x, wt, b, a))
    y = train.conv2d(xd, wd, bd, prelu=ad, compute_dtype='bf16')
    y.backward(gy.to(cuda))
    xe, we, be = (t.double().requires_grad_(True) for t in (x, wt, b))
    ze = cb.emul_conv(xe, we, be, False)
    pos = ze.detach() > 0
    gz = torch.where(pos, gy, a.view(1, -1, 1, 1) * gy)            # fp32 products, as the kernel's
    ze.backward(gz.double())
    xr, wr, gr = cb.rb(x).double(), cb.rb(wt).double(), cb.rb(gz).double()
    note = {}
    s_z = F.conv2d(xr.abs(), wr.abs(), b.double().abs(), padding=1)
    e_z = 2 * cb.gamma(cin * k * k + 2) * s_z
    y64 = F.prelu(ze.detach(), a.double())
    within("y", y.detach(), y64, e_z * torch.where(pos, torch.ones_like(s_z), a.double().abs().view(1, -1, 1, 1)) +
           cb.U * y64.abs(), note)
    within("dx", xd.grad, xe.grad, 2 * cb.gamma(cout * k * k + 1) * cb.dgrad64(gr, wr)[1], note)
    within("dw", wd.grad, we.grad, 2 * cb.gamma(n * h * w + 1) * cb.wgrad64(xr, gr, k)[1], note)
    within("db", bd.grad, be.grad, 2 * cb.gamma(n * h * w + 1) * cb.dbias64(gr)[1], note)
    zg = torch.where(pos, torch.zeros_like(ze.detach()), ze.detach() * gy.double())
    bound_a = (torch.where(pos, torch.zeros_like(e_z), e_z * gy.double().abs()).sum((0, 2, 3)) +
               cb.gamma(n * h * w + 1) * zg.abs().sum((0, 2, 3)))
    within("dslope", ad.grad, zg.sum((0, 2, 3)), bound_a, note)
    cd.note("train_bf16_prelu_layer.json", note)


# ---- (c) chains and whole networks ----------------------------------------------------------------------------------------------------
def ratios(grads, grads64):
    return {n: ((grads[n].double().cpu() - g64).abs().max() / g64.abs().max()).item() for n, g64 in grads64.items()}


def check_ratios(name, native, emul, grads64, fallbacks):
    rn, re = ratios(native, grads64), ratios(emul, grads64)
    yard = max(re.values())
    worst = max(rn, key=rn.get)
    print("%s: worst native ratio %.3g (%s), yardstick max r_emul %.3g, fallbacks %s" % (name, rn[worst], worst, yard, fallbacks))
    cd.note("train_bf16_grad_ratios_%s.json" % name, {"yardstick_max_r_emul": yard, "worst_native": rn[worst],
                                                       "fallbacks": fallbacks,
                                                       "per_parameter": {n: {"native": rn[n], "emul": re[n]} for n in rn}})
    bad = {n: r for n, r in rn.items() if not r <= MARGIN * yard}
    assert not bad, "r_native above %g x %.3g: %s" % (MARGIN, yard, bad)


def grads_of(params, loss):
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in params if p.grad is not None}


def he_init(convs, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in convs:
            co, ci, k = m.weight.shape[0], m.weight.shape[1], m.weight.shape[2]
            m.weight.copy_(cd.weights("he", co, ci, k, g))
            m.bias.copy_(torch.randn(co, generator=g) * 0.1)


class Chain(nn.Module):
    """the small chain of test_train_gpu.py: conv3 + ReLU, pool, conv7 + ReLU, concat with the conv7's input, conv1"""
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


def emul_module_conv(x, m, relu):
    return cb.emul_conv(x, m.weight, m.bias, relu)


def test_small_chain_gradients(cuda, train):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 8, 12, 10, generator=g)
    target = torch.randn(2, 5, 6, 5, generator=g)
    base = Chain()
    out = {}
    train.reset_bf16_fallbacks()
    native_conv = lambda t, mod, relu: train.conv2d(t, mod.weight, mod.bias, relu, compute_dtype='bf16')   # noqa: E731
    for name, dt, dev, conv in (("ref64", torch.float64, "cpu", torch_conv), ("emul", torch.float64, "cpu", emul_module_conv),
                                ("native", torch.float32, cuda, native_conv)):
        m = copy.deepcopy(base).to(device=dev, dtype=dt)
        xin = x.clone().to(device=dev, dtype=dt).requires_grad_(True)
        y = m(xin, conv)
        out[name] = grads_of(list(m.named_parameters()) + [("input", xin)], F.mse_loss(y, target.to(device=dev, dtype=dt)))
    ref = {n: t.double() for n, t in out["ref64"].items()}
    assert set(out["native"]) == set(ref) == set(out["emul"]) and len(ref) == 7
    assert all(t.dtype == torch.float32 for t in out["native"].values())
    check_ratios("chain", out["native"], out["emul"], ref, dict(train.bf16_fallbacks))


def run_modules(mods, x, conv):
    """an nn.Sequential of the two trees (Conv2d [+ ReLU | PReLU], MaxPool2d) with `conv(x, module, relu)` for the convs and
    float64 F.prelu behind a conv without an activation"""
    mods, i = list(mods), 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        if isinstance(m, nn.Conv2d):
            relu, prelu = isinstance(nxt, nn.ReLU), isinstance(nxt, nn.PReLU)
            x = conv(x, m, relu)
            if prelu:
                x = F.prelu(x, nxt.weight)
            i += 2 if relu or prelu else 1
        else:
            assert isinstance(m, nn.MaxPool2d)
            x = F.max_pool2d(x, m.kernel_size, m.stride, m.padding)
            i += 1
    return x


def vgg_forward(model, x, conv):
    """lib/network/rtpose_vgg.py:158-198 over the module tree"""
    out1 = run_modules(model.model0, x, conv)
    saved, feed = [], out1
    for s in range(1, 7):
        o1 = run_modules(getattr(model, 'model%d_1' % s), feed, conv)
        o2 = run_modules(getattr(model, 'model%d_2' % s), feed, conv)
        saved += [o1, o2]
        feed = torch.cat([o1, o2, out1], 1)
    return saved


def openpose_forward(model, x, conv):
    """lib/network/openpose.py:86-109, :160-177 over the module tree"""
    def block(blk, t):
        return run_modules([blk.Mconv, blk.MPrelu], t, conv)

    def stage(st, t):
        for b in range(1, 6):
            o1 = block(getattr(st, "Mconv%d_0" % b), t)
            o2 = block(getattr(st, "Mconv%d_1" % b), o1)
            o3 = block(getattr(st, "Mconv%d_2" % b), o2)
            t = torch.cat([o1, o2, o3], 1)
        return run_modules([st.Mconv7], block(st.Mconv6, t), conv)
    features = run_modules(model.feature_extractor, x, conv)
    paf_ret, heat_ret, x_in = [], [], features
    for st in model.l2_stages:
        paf = stage(st, x_in)
        x_in = torch.cat([features, paf], 1)
        paf_ret.append(paf)
    for st in model.l1_stages:
        heat = stage(st, x_in)
        x_in = torch.cat([features, heat, paf], 1)
        heat_ret.append(heat)
    return [paf_ret, heat_ret]


def three_ways(base, x, heat, paf, forward, loss, cuda, train):
    """the gradients of the loss in float64, through the emulation, and natively in bf16: computed once, left unchanged"""
    r = dict(base=base, x=x, heat=heat, paf=paf)
    for name, conv in (("ref64", torch_conv), ("emul", emul_module_conv)):
        m = copy.deepcopy(base).double()
        total, _ = loss(forward(m, x.double(), conv), heat.double(), paf.double())
        r[name] = {n: t.double() for n, t in grads_of(list(m.named_parameters()), total).items()}
    m = copy.deepcopy(base).to(cuda)
    train.reset_bf16_fallbacks()
    _, saved = train.forward_train(m, x.to(cuda), compute_dtype='bf16')
    total, _ = loss(saved, heat.to(cuda), paf.to(cuda))
    r["native"] = grads_of(list(m.named_parameters()), total)
    r["fallbacks"] = dict(train.bf16_fallbacks)
    return r


@pytest.fixture(scope="module")
def vgg(pkg, cuda, train, encode):
    torch.manual_seed(0)
    base = pkg.get_model('vgg19')
    he_init([m for _, m in base._convs()], 23)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 3, 32, 32, generator=g)
    heat, paf = torch.rand(1, 19, 4, 4, generator=g), torch.randn(1, 38, 4, 4, generator=g) * 0.5
    return three_ways(base, x, heat, paf, vgg_forward, encode.get_loss, cuda, train)


def test_whole_rtpose_vgg_gradients(vgg):
    assert len(vgg["native"]) == 184 and set(vgg["native"]) == set(vgg["ref64"]) == set(vgg["emul"])
    assert all(t.dtype == torch.float32 for t in vgg["native"].values())
    check_ratios("rtpose_vgg", vgg["native"], vgg["emul"], vgg["ref64"], vgg["fallbacks"])


TOPO = (2, 2, 52, 26)


def test_whole_openpose_model_gradients(cuda, train, encode, openpose):
    torch.manual_seed(0)
    base = openpose.OpenPose_Model(*TOPO)
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, nn.Conv2d):
                he_init([m], int(torch.randint(1 << 30, (1,), generator=g)))
            elif isinstance(m, nn.PReLU):
                m.weight.copy_(torch.randn(m.weight.shape[0], generator=g) * 0.25)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 3, 32, 32, generator=g)
    heat, paf = torch.rand(1, TOPO[3], 4, 4, generator=g), torch.randn(1, TOPO[2], 4, 4, generator=g) * 0.5
    r = three_ways(base, x, heat, paf, openpose_forward, encode.get_loss_openpose, cuda, train)
    assert set(r["native"]) == set(r["ref64"]) == set(r["emul"]) and len(r["native"]) == sum(1 for _ in base.parameters())
    check_ratios("openpose", r["native"], r["emul"], r["ref64"], r["fallbacks"])


# ---- (d) the default path, the optimizer step, the refusals -----------------------------------------------------------------------------
def test_fp32_keyword_is_the_call_without_it(cuda, train):
    g = torch.Generator().manual_seed(3)
    x, target = torch.randn(2, 8, 12, 10, generator=g).to(cuda), torch.randn(2, 5, 6, 5, generator=g).to(cuda)
    base = Chain().to(cuda)
    got = []
    for conv in (lambda t, mod, relu: train.conv2d(t, mod.weight, mod.bias, relu),
                 lambda t, mod, relu: train.conv2d(t, mod.weight, mod.bias, relu, compute_dtype='fp32')):
        m = copy.deepcopy(base)
        xin = x.clone().requires_grad_(True)
        y = m(xin, conv)
        got.append((y.detach(), grads_of(list(m.named_parameters()) + [("input", xin)], F.mse_loss(y, target))))
    assert torch.equal(got[0][0], got[1][0])
    assert len(got[0][1]) == 7 and all(torch.equal(got[0][1][n], got[1][1][n]) for n in got[0][1])
    # and bf16 is another arithmetic
    m = copy.deepcopy(base)
    y16 = m(x, lambda t, mod, relu: train.conv2d(t, mod.weight, mod.bias, relu, compute_dtype='bf16'))
    assert not torch.equal(y16, got[0][0])
    seq = nn.Sequential(base.c3, nn.ReLU(), nn.MaxPool2d(2, 2, 0), base.c7, nn.ReLU())
    assert torch.equal(train.run_sequential(seq, x), train.run_sequential(seq, x, compute_dtype='fp32'))


def test_bf16_train_step_is_torch_sgd_on_the_native_gradients_and_inference_resyncs(vgg, pkg, cuda, train, encode):
    x, heat, paf = vgg["x"].to(cuda), vgg["heat"].to(cuda), vgg["paf"].to(cuda)
    a = copy.deepcopy(vgg["base"]).to(cuda)
    with torch.no_grad():
        before = [t.clone() for t in a(x)[1]]            # packs the inference arena from the initial parameters
    opt_a = torch.optim.SGD(a.parameters(), lr=0.05, momentum=0.9)
    total, log = train.train_step(a, opt_a, x, heat, paf, compute_dtype='bf16')
    assert total.dtype == torch.float32
    assert total.item() == pytest.approx(sum(log[n] for n in encode.build_names()), rel=1e-5)
    assert all(p.dtype == torch.float32 and p.grad.dtype == torch.float32 for p in a.parameters())
    # the same step applied by torch to the native bf16-path gradients of the untouched parameters
    b = copy.deepcopy(vgg["base"]).to(cuda)
    opt_b = torch.optim.SGD(b.parameters(), lr=0.05, momentum=0.9)
    for n, p in b.named_parameters():
        p.grad = vgg["native"][n].clone()
    opt_b.step()
    start = dict(vgg["base"].named_parameters())
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
    # a second bf16 step packs the stepped filters anew: the gradients are those of a fresh copy
    def grads(m):
        m.zero_grad(set_to_none=True)
        _, saved = train.forward_train(m, x, compute_dtype='bf16')
        encode.get_loss(saved, heat, paf)[0].backward()
        return {n: p.grad.clone() for n, p in m.named_parameters()}
    ga, gf = grads(a), grads(fresh)
    assert all(torch.equal(ga[n], gf[n]) for n in ga)
    assert any(not torch.equal(ga[n], vgg["native"][n]) for n in ga)


def test_bf16_is_refused_for_the_batchnorm_networks_on_the_device(pkg, capi, cuda, train):
    hourglass = importlib.import_module(pkg.__name__ + ".hourglass")
    shufflenet = importlib.import_module(pkg.__name__ + ".shufflenet")
    x = torch.zeros(1, 3, 32, 32, device=cuda)
    for model, text in ((hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3), "BatchNorm kernels"),
                        (shufflenet.Network(), "BatchNorm and depthwise kernels")):
        model = model.to(cuda).train()
        with pytest.raises(capi.RtposeError, match=text):
            train.forward_train(model, x, compute_dtype='bf16')
        with pytest.raises(capi.RtposeError, match=text):
            train.train_step(model, None, x, None, None, compute_dtype='bf16')
    with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
        train.conv2d(x, torch.zeros(4, 3, 3, 3, device=cuda), compute_dtype='fp16')
