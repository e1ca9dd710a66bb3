"""CPU suite of the layout-resident Bottleneck's public door (train.preact_chain, train.hourglass_forward(block=),
resident='bottleneck' of train.forward_train / train.train_step): the keyword's refusals, which need no device, and the call
order of hourglass_forward with spy callables - block=None is the order it had before the argument existed, block= is called
once per Bottleneck with the module and its input and takes that Bottleneck's convs and BatchNorms off the other callables."""
import importlib

import pytest
import torch
import torch.nn as nn

import hourglass_train_restate as htr

from conftest import PKG_NAME


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


@pytest.fixture(scope="module")
def hgm(pkg):
    return importlib.import_module(PKG_NAME + ".hourglass")


TOPO = dict(num_stacks=2, num_blocks=1, paf_classes=4, ht_classes=3)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_the_keyword_is_refused_without_a_device_and_for_everything_but_a_bf16_hourglass(pkg, capi, train, hgm):
    openpose = importlib.import_module(PKG_NAME + ".openpose")
    shufflenet = importlib.import_module(PKG_NAME + ".shufflenet")
    x = torch.zeros(1, 3, 64, 64)
    model = hgm.hg(**TOPO).train()
    with pytest.raises(capi.RtposeError, match="runs only on an MI355X"):
        train.forward_train(model, x, compute_dtype='bf16', resident='bottleneck')
    with pytest.raises(capi.RtposeError, match="resident='bottleneck' needs compute_dtype='bf16'.*fp32 node is not built"):
        train.forward_train(model, x, resident='bottleneck')
    with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
        train.forward_train(model, x, compute_dtype='fp16', resident='bottleneck')
    # without the keyword a HourglassNet still takes no 'bf16', and the other keywords say what they said
    with pytest.raises(capi.RtposeError, match="BatchNorm kernels"):
        train.forward_train(model, x, compute_dtype='bf16')
    with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*BatchNorm kernels"):
        train.forward_train(model, x, resident=True)
    with pytest.raises(capi.RtposeError, match="resident='dense' is for an openpose.OpenPose_Model only"):
        train.forward_train(model, x, resident='dense')
    for wrong in ('Bottleneck', 'bottlenecks', '', 2, None, ('bottleneck',)):
        with pytest.raises(capi.RtposeError, match="resident is False, True or 'dense'; got .*'bottleneck' is"):
            train.forward_train(model, x, resident=wrong)
    for other in (pkg.get_model('vgg19'), openpose.OpenPose_Model(2, 2, 52, 26), shufflenet.Network()):
        for dt in ('fp32', 'bf16'):
            with pytest.raises(capi.RtposeError, match="resident='bottleneck' is for an hourglass.HourglassNet only.*%s"
                               % type(other).__name__):
                train.forward_train(other, x, compute_dtype=dt, resident='bottleneck')
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    heat, paf = torch.zeros(1, 3, 16, 16), torch.zeros(1, 4, 16, 16)
    with pytest.raises(capi.RtposeError, match="resident='bottleneck' needs compute_dtype='bf16'"):
        train.train_step(model, opt, x, heat, paf, resident='bottleneck')
    with pytest.raises(capi.RtposeError, match="runs only on an MI355X"):
        train.train_step(model, opt, x, heat, paf, compute_dtype='bf16', resident='bottleneck')


def test_preact_chain_refusals_without_a_device(capi, train):
    bn, wt, b = nn.BatchNorm2d(4).train(), torch.zeros(8, 4, 3, 3), torch.zeros(8)
    x = torch.zeros(2, 4, 3, 3)
    assert train.preact_fallbacks == 0 and callable(train.reset_preact_fallbacks) and train._preact_conv_into is train._conv_launch
    with pytest.raises(capi.RtposeError, match="train.preact_chain runs only on an MI355X"):
        train.preact_chain(x, [(bn, wt, b)])
    with pytest.raises(capi.RtposeError, match="train.preact_chain: no layers"):
        train.preact_chain(x, [])
    with pytest.raises(capi.RtposeError, match=r"layers are \(nn.BatchNorm2d, weight, bias_or_None\) triples; got 'Tensor' at 0"):
        train.preact_chain(x, [wt])
    with pytest.raises(capi.RtposeError, match="triples; got 'tuple' at 1"):
        train.preact_chain(x, [(bn, wt, b), (wt, b)])
    assert train.preact_fallbacks == 0


# ---- the call order -----------------------------------------------------------------------------------------------------------------
def spies(log, names):
    conv, bn, stem = htr.torch_ops()

    def wrap(kind, op):
        def f(t, m):
            log.append((kind, names[m], tuple(t.shape)))
            return op(t, m)
        return f
    return wrap("conv", conv), wrap("bn", bn), wrap("stem", stem)


def test_block_none_is_the_call_order_without_the_argument(train, hgm):
    """every operation of the network once, in the reference's order: the stem and bn1, then per Bottleneck bn1, conv1, bn2,
    conv2, bn3, conv3 and downsample last; the same log and the same output bits with the argument absent, None, and a block
    that is hourglass_bottleneck itself"""
    torch.manual_seed(0)
    x = torch.randn(2, 3, 64, 64)
    base = htr.seed_model(hgm.hg(**TOPO), 3).train()
    names = {m: n for n, m in base.named_modules()}
    logs, outs = [], []
    for how in ("absent", "none", "bottleneck"):
        for m in base.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.reset_running_stats()
        log = []
        conv, bn, stem = spies(log, names)
        with torch.no_grad():
            if how == "absent":
                out = train.hourglass_forward(base, x, conv, bn, stem)
            elif how == "none":
                out = train.hourglass_forward(base, x, conv, bn, stem, None)
            else:
                out = train.hourglass_forward(base, x, conv, bn, stem, block=lambda blk, t: train.hourglass_bottleneck(blk, t, conv, bn))
        logs.append(log)
        outs.append(out[0])
    assert logs[0] == logs[1] == logs[2]
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
    log = logs[0]
    assert log[0] == ("stem", "conv1", (2, 3, 64, 64)) and log[1] == ("bn", "bn1", (2, 64, 32, 32))
    called = [n for _, n, _ in log]
    ops = {n for n, m in base.named_modules() if isinstance(m, (nn.Conv2d, nn.BatchNorm2d))}
    assert sorted(called) == sorted(ops), "every conv and BatchNorm of the network exactly once"
    blocks = [n for n, m in base.named_modules() if isinstance(m, hgm.Bottleneck)]
    for pre in blocks:
        i = called.index(pre + ".bn1")
        want = [pre + s for s in (".bn1", ".conv1", ".bn2", ".conv2", ".bn3", ".conv3")]
        if getattr(base.get_submodule(pre), "downsample") is not None:
            want.append(pre + ".downsample.0")
        assert called[i:i + len(want)] == want, pre


def test_block_is_called_once_per_bottleneck_with_the_module_and_its_input(train, hgm):
    torch.manual_seed(0)
    x = torch.randn(2, 3, 64, 64)
    base = htr.seed_model(hgm.hg(**TOPO), 3).train()
    names = {m: n for n, m in base.named_modules()}
    log, seen = [], []
    conv, bn, stem = spies(log, names)

    def block(blk, t):
        assert isinstance(blk, hgm.Bottleneck) and torch.is_tensor(t) and t.shape[1] == blk.bn1.num_features
        seen.append(names[blk])
        log.append(("block", names[blk], tuple(t.shape)))
        return t.new_full((t.shape[0], blk.conv3.out_channels, t.shape[2], t.shape[3]), 0.5)

    with torch.no_grad():
        (paf, ht), saved = train.hourglass_forward(base, x, conv, bn, stem, block=block)
    assert tuple(paf.shape) == (2, 4, 16, 16) and tuple(ht.shape) == (2, 3, 16, 16) and saved[0] is paf
    blocks = [n for n, m in base.named_modules() if isinstance(m, hgm.Bottleneck)]
    assert sorted(seen) == sorted(blocks) and len(set(seen)) == len(seen) == 3 + 2 * (3 * 4 + 1 + 1)
    # the other callables see nothing that lives in a Bottleneck
    rest = [n for k, n, _ in log if k != "block"]
    assert not any(n.startswith(tuple(b + "." for b in blocks)) for n in rest)
    outside = {n for n, m in base.named_modules() if isinstance(m, (nn.Conv2d, nn.BatchNorm2d))
               and not n.startswith(tuple(b + "." for b in blocks))}
    assert sorted(rest) == sorted(outside) and "fc.0.1" in outside and "fc_.0" in outside
    # the first Bottleneck reads bn1's output, the first of layer2 the pooled map
    first = [e for e in log if e[0] == "block"]
    assert first[0] == ("block", "layer1.0", (2, 64, 32, 32)) and first[1] == ("block", "layer2.0", (2, 128, 16, 16))
