"""CPU suite of the bf16 depthwise 3x3 kernels (header section 2b continued) and of what stands on them without a device:
the host emulation of tests/dwconv_bf16_restate.py against torch's float64 autograd on integer operands, the cases held to
what their tags say, the symbols, every refusal of the three launchers with its text before any HIP call, and the refusals
of train.dwconv3x3(compute_dtype=...), train.unit_chain and forward_train / train_step(resident='branch') that fire before
the device is touched."""
import importlib
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import dwconv_bf16_restate as db
import dwconv_restate as dr

from conftest import PKG_NAME, ROOT


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


@pytest.fixture(scope="module")
def shufflenet(pkg):
    return importlib.import_module(PKG_NAME + ".shufflenet")


# ---- the emulation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_emulation_equals_float64_autograd_on_integers(c):
    """small integers are bf16 numbers and every product and sum of them is an fp32 number: the emulation - round, widen,
    the fp32 restatements - must give torch's float64 autograd, =="""
    x, gy, wt = db.exact_operands(c)
    y64, dx64, dw64 = dr.autograd64(x, wt, gy, c.stride)
    y, dx, dw = db.emulate(x.numpy(), wt.numpy(), gy.numpy(), c.stride)
    assert y.dtype == dx.dtype == np.float32
    assert np.array_equal(y.astype(np.float64), y64.numpy())
    assert np.array_equal(dx.astype(np.float64), dx64.numpy())
    assert np.array_equal(dw, dw64.numpy())
    assert db.sums_exact_in_fp64(x.numpy(), gy.numpy(), c.stride)


def test_forward_restatement_is_the_fp32_order():
    """against float64 the fp32 forward differs on random operands (it rounds), and equals a scalar loop written from the
    header's sentence: from the bias, ky then kx ascending, a product rounded, then the add rounded"""
    c = dr.CASES[2]
    x, gy, wt = db.random_operands(c)
    bias = torch.randn(c.c, generator=torch.Generator().manual_seed(3)).numpy()
    y = db.forward_restate(x.numpy(), wt.numpy(), c.stride, bias)
    xp = np.zeros((c.n, c.c, c.h + 2, c.w + 2), np.float32)
    xp[:, :, 1:-1, 1:-1] = x.numpy()
    w = wt.numpy()
    for n, ch, yo, xo in ((0, 0, 0, 0), (1, 2, c.h - 1, c.w - 1), (0, 1, 2, 3)):
        acc = np.float32(bias[ch])
        for ky in range(3):
            for kx in range(3):
                acc = np.float32(acc + np.float32(xp[n, ch, yo + ky, xo + kx] * w[ch, 0, ky, kx]))
        assert acc.view(np.uint32) == y[n, ch, yo, xo].view(np.uint32)
    y64 = db.forward_restate(x.numpy(), wt.numpy(), c.stride, bias, np.float64)
    assert np.abs(y - y64).max() > 0 and np.abs(y - y64).max() < 1e-5


@pytest.mark.parametrize("c", db.CASES, ids=db.case_id)
def test_random_operands_sum_exactly_in_fp64(c):
    """what lets the GPU suite hold the bf16 weight gradient to numpy's float64 sum bit for bit on random operands too"""
    x, gy, _ = db.random_operands(c)
    assert torch.equal(db.round_bf16(x), x) and torch.equal(db.round_bf16(gy), gy)
    assert db.sums_exact_in_fp64(x.numpy(), gy.numpy(), c.stride)


def test_cases_are_what_their_tags_say():
    shapes = {(c.n, c.c, c.h, c.w, c.stride) for c in db.CASES}
    assert shapes >= {(c.n, c.c, c.h, c.w, c.stride) for c in dr.CASES}           # the slab cases included
    assert shapes >= {(1, 58, 8, 6, 1), (1, 58, 8, 6, 2), (1, 6, 8, 6, 1), (1, 6, 8, 6, 2)}
    for s in shapes:
        assert {c.tags for c in db.CASES if (c.n, c.c, c.h, c.w, c.stride) == s} == {"x8", "x4", "odd"}
    for c in db.CASES:
        assert db.load_path(c) == {"x8": 8, "x4": 4, "odd": 1}[c.tags], c
        for cs, off in (c.x, c.gy, c.dx):
            assert off + c.c <= cs, c
        if c.tags != "odd":
            assert c.dx[0] % 4 == 0 and c.dx[1] % 4 == 0, c
    assert len({db.case_id(c) for c in db.CASES}) == len(db.CASES)
    # a last unit of fewer live channels than a thread owns, in both aligned classes
    assert any(c.c % 4 and c.tags == "x8" for c in db.CASES) and any(c.c % 4 and c.tags == "x4" for c in db.CASES)


# ---- symbols ----------------------------------------------------------------------------------------------------------------------------
def test_every_new_header_function_has_a_prototype(capi):
    header = open(ROOT + "/include/rtpose_mi355x.h").read()
    for name in db.ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    # the workspace query is the fp32 kernel's: none of their own
    assert not any(n.startswith("rtpose_dwconv3x3_wgrad_bf16_") for n in capi.EXPORTED)


# ---- the launchers' refusals --------------------------------------------------------------------------------------------------------------
_FAULTS = [(name, fault[0], fault[1], fault[2]) for name, (_, _, faults) in db.ENTRY_POINTS.items() for fault in faults]


@pytest.mark.parametrize("entry,name,fault,text", _FAULTS, ids=["%s-%s" % (f[0][7:], f[1]) for f in _FAULTS])
def test_launchers_refuse_on_the_host(capi, entry, name, fault, text):
    who, make, _ = db.ENTRY_POINTS[entry]
    lays, a = make(capi)
    fault(a, lays)
    db.refused(capi, getattr(capi.lib, entry), who, a, text)


def test_host_checks_pass_valid_arguments(capi):
    """with every host check passed the refusal is the pointer's (fake: no device owns it); dbias = NULL is accepted"""
    for entry, (who, make, _) in db.ENTRY_POINTS.items():
        lays, a = make(capi)
        assert getattr(capi.lib, entry)(*a) != 0 and "device memory" in capi.last_error(), entry
    lays, a = db.wgrad_args(capi)
    a[5] = None
    assert capi.lib.rtpose_dwconv3x3_wgrad_bf16(*a) != 0 and "device memory" in capi.last_error()


# ---- train.dwconv3x3, train.unit_chain and the keyword -----------------------------------------------------------------------------------------
def test_dwconv3x3_refusals_without_a_device(capi, train):
    x, w = torch.zeros(1, 4, 5, 5), torch.zeros(4, 1, 3, 3)
    for wrong in ('fp16', 'BF16', '', None, 16):
        with pytest.raises(capi.RtposeError, match="train.dwconv3x3: compute_dtype is 'fp32' or 'bf16'"):
            train.dwconv3x3(x, w, 1, wrong)
    for dt in ('fp32', 'bf16'):
        with pytest.raises(capi.RtposeError, match="train.dwconv3x3 runs only on an MI355X"):
            train.dwconv3x3(x, w, 1, dt)
        with pytest.raises(capi.RtposeError, match="train.dwconv3x3 runs only on an MI355X"):
            train.dwconv3x3(x, w, compute_dtype=dt)


def test_unit_chain_refusals_without_a_device(capi, train):
    x = torch.zeros(2, 4, 5, 5)
    pw, dw, bn = nn.Conv2d(4, 4, 1), nn.Conv2d(4, 4, 3, 1, 1, groups=4, bias=False), nn.BatchNorm2d(4)
    with pytest.raises(capi.RtposeError, match="train.unit_chain: no units"):
        train.unit_chain(x, [])
    with pytest.raises(capi.RtposeError, match=r"units are \(nn.Conv2d, nn.BatchNorm2d, relu\) triples; got 'Conv2d' at 0"):
        train.unit_chain(x, [pw])
    with pytest.raises(capi.RtposeError, match="triples; got 'tuple' at 1"):
        train.unit_chain(x, [(pw, bn, True), (dw, bn)])
    with pytest.raises(capi.RtposeError, match="train.unit_chain runs only on an MI355X"):
        train.unit_chain(x, [(pw, bn, True), (dw, bn, False)])
    assert train.unit_fallbacks == 0
    train.reset_unit_fallbacks()
    assert [train._unit_kind(m) for m in (pw, dw, nn.Conv2d(4, 4, 3, 2, 1, groups=4, bias=False))] == ['pw', 'dw', 'dw']
    for m in (nn.Conv2d(4, 4, 3, 1, 1), nn.Conv2d(4, 4, 3, 1, 1, groups=4), nn.Conv2d(4, 4, 1, 2), nn.Conv2d(4, 8, 3, 1, 1, groups=4, bias=False),
              nn.Conv2d(4, 4, 3, 3, 1, groups=4, bias=False), nn.Conv2d(4, 4, 3, 1, 0, groups=4, bias=False), nn.ReLU()):
        assert train._unit_kind(m) is None, m


def test_the_keyword_is_refused_without_a_device_and_for_everything_but_a_bf16_shufflenet(pkg, capi, train, shufflenet):
    openpose = importlib.import_module(PKG_NAME + ".openpose")
    hourglass = importlib.import_module(PKG_NAME + ".hourglass")
    x = torch.zeros(1, 3, 64, 64)
    model = shufflenet.Network().train()
    with pytest.raises(capi.RtposeError, match="runs only on an MI355X"):
        train.forward_train(model, x, compute_dtype='bf16', resident='branch')
    with pytest.raises(capi.RtposeError, match="resident='branch' needs compute_dtype='bf16'.*fp32 node is not built"):
        train.forward_train(model, x, resident='branch')
    with pytest.raises(capi.RtposeError, match="resident='branch' needs compute_dtype='bf16'"):
        train.forward_train(model, x, compute_dtype='fp32', resident='branch')
    with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
        train.forward_train(model, x, compute_dtype='fp16', resident='branch')
    with pytest.raises(capi.RtposeError, match=r"resident='branch' is the training-mode forward.*call \.train\(\) first"):
        train.forward_train(shufflenet.Network().eval(), x, compute_dtype='bf16', resident='branch')
    # without the keyword a shufflenet.Network still takes no 'bf16', and the other keywords say what they said
    with pytest.raises(capi.RtposeError, match="BatchNorm and depthwise kernels"):
        train.forward_train(model, x, compute_dtype='bf16')
    with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*BatchNorm and depthwise kernels"):
        train.forward_train(model, x, resident=True)
    with pytest.raises(capi.RtposeError, match="resident='dense' is for an openpose.OpenPose_Model only"):
        train.forward_train(model, x, resident='dense')
    with pytest.raises(capi.RtposeError, match="resident='bottleneck' is for an hourglass.HourglassNet only"):
        train.forward_train(model, x, compute_dtype='bf16', resident='bottleneck')
    for wrong in ('Branch', 'branches', '', 2, None, ('branch',)):
        with pytest.raises(capi.RtposeError, match="resident is False, True or 'dense'; got .*'bottleneck' is.*'branch' their fifth"):
            train.forward_train(model, x, resident=wrong)
    others = (pkg.get_model('vgg19'), openpose.OpenPose_Model(2, 2, 52, 26),
              hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3))
    for other in others:
        for dt in ('fp32', 'bf16'):
            with pytest.raises(capi.RtposeError, match="resident='branch' is for a shufflenet.Network only.*%s" % type(other).__name__):
                train.forward_train(other, x, compute_dtype=dt, resident='branch')
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    heat, paf = torch.zeros(1, 19, 8, 8), torch.zeros(1, 38, 8, 8)
    with pytest.raises(capi.RtposeError, match="resident='branch' needs compute_dtype='bf16'"):
        train.train_step(model, opt, x, heat, paf, resident='branch')
    with pytest.raises(capi.RtposeError, match="runs only on an MI355X"):
        train.train_step(model, opt, x, heat, paf, compute_dtype='bf16', resident='branch')


def test_shufflenet_forward_takes_six_arguments_or_a_block(train, shufflenet):
    """existing callers pass six arguments and see no change: with torch's float64 operations the forward with block=None,
    the forward without the argument and one whose block callable restates shufflenet_block are equal"""
    model = dr.seed_module(shufflenet.Network(), 1).double().train()
    x = torch.randn(2, 3, 36, 44, generator=torch.Generator().manual_seed(0)).double()
    conv, bn, dw, stem = dr.torch_ops()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    outs = []
    calls = []

    def block(m, t):
        calls.append(type(m).__name__)
        if not hasattr(m, 'conv'):
            return bn(conv(t, m[0]), m[1], True)
        return train.shufflenet_block(m, t, conv, bn, dw)

    for extra in ((), (None,), (block,)):
        model.load_state_dict(state)
        with torch.no_grad():
            outs.append(train.shufflenet_forward(model, x, conv, bn, dw, stem, *extra)[0])
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(outs[0], o))
    assert len(calls) == 16 + 1 and calls[-1] == 'Sequential'
