"""CPU suite of layout-resident training (train.conv_chain, the resident= keyword): what is decided without a device - the
refusals of resident=True for the networks conv_chain cannot run yet, each with its reason, the argument checks, the counters -
and the host-side conditions of the exact chains tests/test_train_resident_gpu.py runs."""
import importlib
import inspect

import pytest
import torch

import test_train_resident_gpu as rg


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(pkg.__name__ + ".train")


def test_the_keyword_defaults_to_the_per_conv_path(train):
    for fn in (train.run_sequential, train.forward_train, train.train_step):
        p = inspect.signature(fn).parameters
        assert p["resident"].default is False and list(p)[-1] == "resident", fn.__name__
    p = inspect.signature(train.conv_chain).parameters
    assert list(p) == ["x", "layers", "epoch", "resync", "compute_dtype"] and p["compute_dtype"].default == 'fp32'


def test_resident_is_refused_with_its_reason(pkg, capi, train):
    openpose = importlib.import_module(pkg.__name__ + ".openpose")
    hourglass = importlib.import_module(pkg.__name__ + ".hourglass")
    shufflenet = importlib.import_module(pkg.__name__ + ".shufflenet")
    x = torch.zeros(1, 3, 32, 32)
    for model, text in ((openpose.OpenPose_Model(2, 2, 52, 26), "PReLU needs the fp32 pre-activation.*two consumers"),
                        (hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3), "BatchNorm kernels"),
                        (shufflenet.Network(), "BatchNorm and depthwise kernels")):
        with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*" + text):
            train.forward_train(model.train(), x, resident=True)
    # an RtposeVGG passes that check and meets the next one: there is no CPU path
    with pytest.raises(capi.RtposeError, match="runs only on an MI355X"):
        train.forward_train(pkg.get_model('vgg19'), x, resident=True)


def test_conv_chain_has_no_cpu_path_and_counts_from_zero(capi, train):
    x, w = torch.zeros(1, 8, 4, 4), torch.zeros(16, 8, 3, 3)
    with pytest.raises(capi.RtposeError, match="runs only on an MI355X"):
        train.conv_chain(x, [(w, None, True), (torch.zeros(4, 16, 1, 1), None, False)])
    with pytest.raises(capi.RtposeError, match="no layers"):
        train.conv_chain(x, [])
    with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
        train.conv_chain(x, [(w, None, True)], compute_dtype='fp16')
    train.reset_chain_fallbacks()
    assert train.chain_fallbacks == 0 and train.bf16_fallbacks.keys() == {'fwd', 'dgrad'}


@pytest.mark.parametrize("relu_last", [False, True])
@pytest.mark.parametrize("name", sorted(rg.CHAINS))
def test_the_exact_chains_are_exact(name, relu_last):
    """exact_case asserts it: the emulation with its roundings equals the one without and torch's float64 autograd, every
    activation and gradient is an integer bf16 holds, every sum of absolute terms stays below 2^24, every ReLU decides"""
    x, layers, top, y64, g64 = rg.exact_case(name, relu_last)
    assert len(g64) == 1 + 2 * len(layers) and y64.shape == (rg.N, layers[-1][0].shape[0], rg.H, rg.W)
    assert [tuple(wt.shape[:2][::-1]) + (wt.shape[2],) for wt, _, _ in layers] == [(cin, cout, k) for k, cin, cout in rg.CHAINS[name]]
