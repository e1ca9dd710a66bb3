"""The launch sequence of train.py, recorded: which entry points of the library a training operation calls, in which
order and with which geometry.  tests/golden/train_launch_trace.json (tools/make_golden_train_trace.py) holds it for the
cases below as one commit's train.py made it; tests/test_train_trace_gpu.py holds every later train.py to it.

``recording(train)`` replaces the module global ``train.lib`` - looked up at call time by every call in train.py - with a
proxy that passes every call through to the real library and appends one entry per call:

    [entry point, normalised arguments ...]                 a launch (status return; its last argument, the stream, left out)
    [entry point, normalised arguments ..., return value]   a size / geometry query (size_t return; they take no stream)

Normalised: an int or a float as it is; a bare pointer "ptr" or "null"; a byref(Layout) its five fields; a byref of a
ConvDesc / WgradDesc / WgradBf16Desc [class name, every field in _fields_ order], its layouts as five fields, its pointers
"ptr" or "null".  No address and no buffer identity is recorded: the caching allocator makes them a matter of object
lifetimes, which a rewrite may move.  Nor is zero-filled against uninitialised allocation: that is torch's, not a call.

The cases (``CASES``: name -> Case) are the smallest shapes the bf16 suites know rtpose_conv2d_bf16 accepts, with operands
from seeded CPU generators.  ``run_case`` returns (trace, {name: sha256 of y and of every gradient} or None); the golden
file (``dump`` / ``load``) holds every distinct call once, the traces as indices, and one sha256 over a case's digests."""
import contextlib
import copy
import ctypes as C
import hashlib
import importlib
import json
from collections import namedtuple

import torch
import torch.nn as nn

import test_train_bf16_gpu as tb
import test_train_resident_gpu as tr

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
_capi = importlib.import_module(PKG + "._capi")

_BYREF = type(C.byref(C.c_int()))


def _fields(s):
    out = [type(s).__name__]
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if ctype is C.c_void_p:
            out.append("ptr" if v else "null")
        elif ctype is _capi.Layout:
            out.append(_layout(v))
        else:
            out.append(v)
    return out


def _layout(lay):
    return [lay.cstride, lay.choff, lay.ws, lay.hs, lay.lead]


def _normalise(a):
    if a is None:
        return "null"
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, _BYREF):
        obj = a._obj
        if isinstance(obj, _capi.Layout):
            return _layout(obj)
        if isinstance(obj, (_capi.ConvDesc, _capi.WgradDesc, _capi.WgradBf16Desc)):
            return _fields(obj)
    raise TypeError("train_trace: no normal form for the argument %r" % (a,))


class _Recorder:
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        query = fn.restype is C.c_size_t

        def call(*args):
            ret = fn(*args)
            if query:
                self._calls.append([name] + [_normalise(a) for a in args] + [ret])
            else:       # a launch: (..., stream) -> status
                assert fn.restype is C.c_int and fn.argtypes[-1] is C.c_void_p and len(args) == len(fn.argtypes), name
                self._calls.append([name] + [_normalise(a) for a in args[:-1]])
            return ret
        return call


@contextlib.contextmanager
def recording(train):
    """``with recording(train) as calls``: every call train.py makes into the library is appended to `calls`"""
    real, calls = train.lib, []
    train.lib = _Recorder(real, calls)
    try:
        yield calls
    finally:
        train.lib = real


def canonical(trace):
    return json.dumps(trace, sort_keys=True, separators=(",", ":"))


def trace_digest(trace):
    return hashlib.sha256(canonical(trace).encode()).hexdigest()


def histogram(trace):
    h = {}
    for call in trace:
        h[call[0]] = h.get(call[0], 0) + 1
    return h


def tensor_digests(named):
    return {n: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for n, t in named.items()
            if t is not None}


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# store: 'full' the whole trace, 'summary' (the whole networks) the number of calls, the calls per entry point and the trace's
# digest.  run(train, dev) -> {name: tensor or None} or None.
Case = namedtuple("Case", "store run")
CASES = {}


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


REQUIRED = {"all": "xwba", "x_only": "x", "w_and_b_only": "wba", "b_only": "b"}


def _conv2d_case(s, dt, act, req, seed, refuse=None):
    def run(train, dev):
        g = torch.Generator().manual_seed(seed)
        leaves = {"x": _randn(g, s.n, s.cin, s.h, s.w), "w": _randn(g, s.cout, s.cin, s.k, s.k) * (s.cin * s.k * s.k) ** -0.5,
                  "b": _randn(g, s.cout) * 0.1}
        if act == "prelu":
            leaves["a"] = _randn(g, s.cout) * 0.25
        gy = _randn(g, s.n, s.cout, s.h, s.w)
        leaves = {n: t.to(dev).requires_grad_(n in req) for n, t in leaves.items()}
        with _refusing_conv2d(train, refuse):
            y = train.conv2d(leaves["x"], leaves["w"], leaves["b"], act == "relu", prelu=leaves.get("a"), compute_dtype=dt)
            y.backward(gy.to(dev))
        return dict({"d" + n: t.grad for n, t in leaves.items()}, y=y)
    return run


@contextlib.contextmanager
def _refusing_conv2d(train, which):
    """plays a refusal of rtpose_conv2d_bf16 in the per-conv path: its `which`-th bf16 launch (1: the forward, 2: the data
    gradient) answers as the launcher does when it returns RTPOSE_E_INVAL, before anything is launched"""
    if which is None:
        yield
        return
    real, count = train._launch_conv, [0]

    def launch(bf16, *a, **kw):
        count[0] += bf16
        return None if bf16 and count[0] == which else real(bf16, *a, **kw)
    train._launch_conv = launch
    try:
        yield
    finally:
        train._launch_conv = real


@contextlib.contextmanager
def _refusing_chain(train, which):
    """the seam of test_refused_convs_fall_back_and_are_counted: the chain's bf16 launches for which `which`(their
    1-based number) holds are refused"""
    if which is None:
        yield
        return
    real, count = train._conv_into, [0]

    def conv_into(bf16, *a, **kw):
        count[0] += 1
        return False if bf16 and which(count[0]) else real(bf16, *a, **kw)
    train._conv_into = conv_into
    try:
        yield
    finally:
        train._conv_into = real


def _chain_case(name, dt, relu_last, subset, seed, refuse=None):
    def run(train, dev):
        shapes = tr.CHAINS[name]
        x, layers, gy = tr.random_operands(shapes, seed)
        need_x, need_p = tr.required(subset, len(layers))
        xin = x.to(dev).requires_grad_(need_x)
        params = [(wt.to(dev).requires_grad_(need), b.to(dev).requires_grad_(need)) for (wt, b, _), need in zip(layers, need_p)]
        relus = [relu_last or i + 1 < len(layers) for i in range(len(layers))]
        with _refusing_chain(train, refuse):
            y = train.conv_chain(xin, [(wt, b, r) for (wt, b), r in zip(params, relus)], compute_dtype=dt)
            y.backward(gy.to(dev))
        out = {"y": y, "dx": xin.grad}
        for i, (wt, b) in enumerate(params):
            out["dw%d" % i], out["db%d" % i] = wt.grad, b.grad
        return out
    return run


def _sequential_case(dt, resident):
    """conv + ReLU, conv + ReLU, pool, conv + PReLU, conv: with `resident` a chain of two, a conv2d with a PReLU, which breaks
    the run, and a run of one conv"""
    def run(train, dev):
        torch.manual_seed(0)
        mods = [nn.Conv2d(9, 8, 3, 1, 1), nn.ReLU(), nn.Conv2d(8, 72, 7, 1, 3), nn.ReLU(), nn.MaxPool2d(2, 2, 0),
                nn.Conv2d(72, 8, 3, 1, 1), nn.PReLU(8), nn.Conv2d(8, 19, 1, 1, 0)]
        tb.he_init([m for m in mods if isinstance(m, nn.Conv2d)], 31)
        g = torch.Generator().manual_seed(37)
        with torch.no_grad():
            mods[6].weight.copy_(_randn(g, 8) * 0.25)
        x, gy = _randn(g, 2, 9, 10, 12), _randn(g, 2, 19, 5, 6)
        seq = nn.Sequential(*mods).to(dev)
        xin = x.to(dev).requires_grad_(True)
        y = train.run_sequential(seq, xin, compute_dtype=dt, resident=resident)
        y.backward(gy.to(dev))
        return dict({"d" + n.replace(".", "_"): p.grad for n, p in seq.named_parameters()}, y=y, dx=xin.grad)
    return run


def _conv7x7_s2_case(train, dev):
    g = torch.Generator().manual_seed(41)
    x, wt, b, gy = _randn(g, 2, 3, 5, 7), _randn(g, 64, 3, 7, 7) * 0.1, _randn(g, 64) * 0.1, _randn(g, 2, 64, 3, 4)
    wd, bd = wt.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = train.conv7x7_s2(x.to(dev), wd, bd)
    y.backward(gy.to(dev))
    return {"y": y, "dw": wd.grad, "db": bd.grad}


def _conv3x3_s2_case(train, dev):
    g = torch.Generator().manual_seed(43)
    x, wt, gy = _randn(g, 2, 3, 5, 7), _randn(g, 24, 3, 3, 3) * 0.2, _randn(g, 2, 24, 3, 4)
    xd, wd = x.to(dev).requires_grad_(True), wt.to(dev).requires_grad_(True)
    y = train.conv3x3_s2(xd, wd)
    y.backward(gy.to(dev))
    return {"y": y, "dx": xd.grad, "dw": wd.grad}


def _dwconv_case(stride):
    def run(train, dev):
        g = torch.Generator().manual_seed(47 + stride)
        x, wt = _randn(g, 2, 8, 9, 11), _randn(g, 8, 1, 3, 3) * 0.3
        gy = _randn(g, 2, 8, (9 - 1) // stride + 1, (11 - 1) // stride + 1)
        xd, wd = x.to(dev).requires_grad_(True), wt.to(dev).requires_grad_(True)
        y = train.dwconv3x3(xd, wd, stride)
        y.backward(gy.to(dev))
        return {"y": y, "dx": xd.grad, "dw": wd.grad}
    return run


def _batch_norm_case(train, dev):
    g = torch.Generator().manual_seed(53)
    x, gy = _randn(g, 2, 12, 5, 7), _randn(g, 2, 12, 5, 7)
    bn = nn.BatchNorm2d(12)
    with torch.no_grad():
        bn.weight.copy_(_randn(g, 12) * 0.5 + 1)
        bn.bias.copy_(_randn(g, 12) * 0.1)
    bn = bn.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    y = train.batch_norm(xd, bn, relu=True)
    y.backward(gy.to(dev))
    return {"y": y, "dx": xd.grad, "dw": bn.weight.grad, "db": bn.bias.grad, "running_mean": bn.running_mean,
            "running_var": bn.running_var}


_nets = {}


def _network(kind):
    """the models and inputs of the whole-network tests of test_train_bf16_gpu.py (their seeds and sizes), built once"""
    if kind in _nets:
        return _nets[kind]
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(29)
    x = torch.randn(1, 3, 32, 32, generator=g)
    if kind == "vgg":
        base = importlib.import_module(PKG).get_model('vgg19')
        tb.he_init([m for _, m in base._convs()], 23)
        heat, paf = torch.rand(1, 19, 4, 4, generator=g), torch.randn(1, 38, 4, 4, generator=g) * 0.5
    else:
        base = importlib.import_module(PKG + ".openpose").OpenPose_Model(*tb.TOPO)
        gi = torch.Generator().manual_seed(23)
        with torch.no_grad():
            for m in base.modules():
                if isinstance(m, nn.Conv2d):
                    tb.he_init([m], int(torch.randint(1 << 30, (1,), generator=gi)))
                elif isinstance(m, nn.PReLU):
                    m.weight.copy_(torch.randn(m.weight.shape[0], generator=gi) * 0.25)
        heat, paf = torch.rand(1, tb.TOPO[3], 4, 4, generator=g), torch.randn(1, tb.TOPO[2], 4, 4, generator=g) * 0.5
    _nets[kind] = (base, x, heat, paf)
    return _nets[kind]


def _network_case(kind, dt, resident):
    def run(train, dev):
        encode = importlib.import_module(PKG + ".encode")
        base, x, heat, paf = _network(kind)
        m = copy.deepcopy(base).to(dev)
        _, saved = train.forward_train(m, x.to(dev), compute_dtype=dt, resident=resident)
        loss = encode.get_loss if kind == "vgg" else encode.get_loss_openpose
        loss(saved, heat.to(dev), paf.to(dev))[0].backward()
        return None
    return run


def _build():
    seed = 1000
    for s in tb.RELU_SHAPES:
        for dt in ("fp32", "bf16"):
            for act in ("none", "relu", "prelu"):
                for sub, req in REQUIRED.items():
                    seed += 1
                    CASES["conv2d-k%d_%dto%d_%dx%dx%d-%s-%s-%s" % (s.k, s.cin, s.cout, s.n, s.h, s.w, dt, act, sub)] = \
                        Case("full", _conv2d_case(s, dt, act, req, seed))
    for name in sorted(tr.CHAINS):
        for dt in ("fp32", "bf16"):
            for relu_last in (False, True):
                for sub in tr.SUBSETS:
                    seed += 1
                    CASES["conv_chain-%s-%s-%s-%s" % (name, dt, "relu_last" if relu_last else "plain_last", sub)] = \
                        Case("full", _chain_case(name, dt, relu_last, sub, seed))
    nl = len(tr.CHAINS["k3_k7_k3_k1"])
    CASES["refused-conv_chain-second_forward_conv"] = Case("full", _chain_case("k3_k7_k3_k1", "bf16", False, "all", 2001,
                                                                                lambda i: i == 2))
    CASES["refused-conv_chain-every_data_gradient"] = Case("full", _chain_case("k3_k7_k3_k1", "bf16", False, "all", 2002,
                                                                                lambda i: i > nl))
    CASES["refused-conv2d-forward"] = Case("full", _conv2d_case(tb.RELU_SHAPES[0], "bf16", "relu", "xwb", 2003, refuse=1))
    CASES["refused-conv2d-data_gradient"] = Case("full", _conv2d_case(tb.RELU_SHAPES[0], "bf16", "relu", "xwb", 2004, refuse=2))
    for dt in ("fp32", "bf16"):
        for resident in (False, True):
            CASES["run_sequential-%s-%s" % (dt, "resident" if resident else "per_conv")] = Case("full", _sequential_case(dt, resident))
    CASES["conv7x7_s2"] = Case("full", _conv7x7_s2_case)
    CASES["conv3x3_s2"] = Case("full", _conv3x3_s2_case)
    CASES["dwconv3x3-stride1"] = Case("full", _dwconv_case(1))
    CASES["dwconv3x3-stride2"] = Case("full", _dwconv_case(2))
    CASES["batch_norm"] = Case("full", _batch_norm_case)
    for kind, modes in (("vgg", (("fp32", False), ("bf16", False), ("bf16", True))), ("openpose", (("fp32", False), ("bf16", False)))):
        for dt, resident in modes:
            CASES["forward_train-%s-%s%s" % (kind, dt, "-resident" if resident else "")] = \
                Case("summary", _network_case(kind, dt, resident))


_build()


def run_case(train, dev, name):
    """(trace, digests or None) of one case, on a cold packing cache"""
    train.drop_packed_filters()
    train.reset_bf16_fallbacks()
    train.reset_chain_fallbacks()
    with recording(train) as calls:
        out = CASES[name].run(train, dev)
    trace = json.loads(canonical(calls))
    return trace, (tensor_digests(out) if out is not None else None)


def with_tensors(entry, digests):
    """`entry` with what the golden file holds of a case's tensors: their names, and ONE sha256 over the sha256 of each"""
    return dict(entry, tensors=sorted(digests), tensors_sha256=trace_digest(digests))


def stored(name, trace):
    """what the golden file holds of a case's trace"""
    if CASES[name].store == "full":
        return {"trace": trace}
    return {"calls": len(trace), "histogram": histogram(trace), "trace_sha256": trace_digest(trace)}


def dump(path, entries):
    """Writes {case: stored(...) [with_tensors]} as the golden file: every distinct call once, in "calls", and
    the full traces as lists of indices into it - the cases repeat a few hundred calls some four thousand times"""
    index, cases = {}, {}
    for name, e in entries.items():
        cases[name] = dict(e, trace=[index.setdefault(canonical(c), len(index)) for c in e["trace"]]) if "trace" in e else e
    lines = [""]
    for c in index:     # several to a line, up to the width of the code
        if lines[-1] and len(lines[-1]) + len(c) > 158:
            lines.append("")
        lines[-1] += ("," if lines[-1] else "") + c
    with open(path, "w") as f:
        f.write('{"calls": [\n' + ",\n".join(lines) + '\n],\n"cases": {\n'
                + ",\n".join("%s: %s" % (json.dumps(n), canonical(e)) for n, e in cases.items()) + "\n}}\n")


def load(path):
    """{case: entry} of a golden file, the traces whole again"""
    with open(path) as f:
        gold = json.load(f)
    return {n: dict(e, trace=[gold["calls"][i] for i in e["trace"]]) if "trace" in e else e for n, e in gold["cases"].items()}
