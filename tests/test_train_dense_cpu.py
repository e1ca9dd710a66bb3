"""CPU suite of layout-resident dense stages (train.dense_stage, resident='dense' of forward_train / train_step): what is refused
without a device, and the state the counters start in."""
import importlib

import pytest
import torch

from conftest import PKG_NAME


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


@pytest.fixture(scope="module")
def openpose(pkg):
    return importlib.import_module(PKG_NAME + ".openpose")


def stage_layers(cin=9, c=16, c6=16, cout=5, blocks=2):
    layers = []
    for b in range(blocks):
        for j in range(3):
            layers.append((torch.zeros(c, (cin if b == 0 else 3 * c) if j == 0 else c, 3, 3), torch.zeros(c), torch.zeros(c)))
    return layers + [(torch.zeros(c6, 3 * c, 1, 1), torch.zeros(c6), torch.zeros(c6)), (torch.zeros(cout, c6, 1, 1), None, None)]


def test_counters_and_the_launch_name(train):
    assert train.dense_fallbacks == 0
    train.reset_dense_fallbacks()
    assert train.dense_fallbacks == 0
    # the node launches through a name of its own; the chain's stays the chain's
    assert train._dense_conv_into is train._conv_launch and train._conv_into is train._conv_launch
    for name in ("rtpose_prelu_bf16", "rtpose_prelu_grad_bf16", "rtpose_prelu_grad_bf16_workspace_floats"):
        assert hasattr(train.lib, name)


def test_dense_stage_refuses_cpu_tensors(capi, train):
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.dense_stage(torch.zeros(1, 9, 4, 4), stage_layers())
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.dense_stage(None, stage_layers())
    assert train.dense_fallbacks == 0


def test_the_keyword_refuses_without_a_device(pkg, capi, train, openpose):
    hourglass = importlib.import_module(PKG_NAME + ".hourglass")
    shufflenet = importlib.import_module(PKG_NAME + ".shufflenet")
    x = torch.zeros(1, 3, 32, 32)
    model = openpose.OpenPose_Model(2, 2, 6, 4)
    keys = list(model.state_dict().keys())
    for dt in ('fp32',):
        with pytest.raises(capi.RtposeError, match="resident='dense' needs compute_dtype='bf16'.*an fp32 node is not built"):
            train.forward_train(model, x, compute_dtype=dt, resident='dense')
        with pytest.raises(capi.RtposeError, match="resident='dense' needs compute_dtype='bf16'"):
            train.train_step(model, None, x, None, None, compute_dtype=dt, resident='dense')
    with pytest.raises(capi.RtposeError, match="resident='dense' needs compute_dtype='bf16'"):
        train.forward_train(model, x, resident='dense')
    for wrong in ('Dense', 'true', '', 2, -1, None, 0.5, ('dense',)):
        for dt in ('fp32', 'bf16'):
            with pytest.raises(capi.RtposeError, match="resident is False, True or 'dense'; got"):
                train.forward_train(model, x, compute_dtype=dt, resident=wrong)
    # today's text for resident=True on this topology
    with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only.*PReLU needs the fp32 pre-activation"):
        train.forward_train(model, x, compute_dtype='bf16', resident=True)
    # accepted values reach the device check
    for kw in ({}, {"resident": False}, {"resident": 'dense'}):
        with pytest.raises(capi.RtposeError, match="no CPU fallback"):
            train.forward_train(model, x, compute_dtype='bf16', **kw)
    for other, dt, text in ((pkg.get_model('vgg19'), 'bf16', "no dense blocks and no PReLU"),
                            (pkg.get_model('vgg19'), 'fp32', "no dense blocks and no PReLU"),
                            (hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3), 'fp32',
                             "BatchNorm kernels.*dense_stage runs the dense blocks"),
                            (shufflenet.Network(), 'fp32', "BatchNorm and depthwise kernels.*dense_stage runs the dense blocks")):
        with pytest.raises(capi.RtposeError, match="resident='dense' is for an openpose.OpenPose_Model only; .*" + text):
            train.forward_train(other, x, compute_dtype=dt, resident='dense')
    with pytest.raises(capi.RtposeError, match="resident=True is for a network.RtposeVGG only"):
        train.forward_train(shufflenet.Network(), x, resident=True)
    assert list(model.state_dict().keys()) == keys and train.dense_fallbacks == 0
