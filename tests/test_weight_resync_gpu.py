"""A re-pack reaches the device: after the parameters of a module that has already run change, its next forward gives,
bit for bit, what a freshly built module with those parameters gives - for each front of the rtpose_net executor
(network.RtposeVGG, openpose.OpenPose_Model, hourglass.HourglassNet) at its smallest input, with the direct kernels forced
so that the two modules cannot choose different forms."""
import importlib
import os
import sys

import pytest
import torch

from conftest import PKG_NAME

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hourglass_restate as HR  # noqa: E402
import openpose_restate as OR  # noqa: E402

pytestmark = pytest.mark.gpu


def _vgg():
    from oracle import net_oracle
    m = importlib.import_module(PKG_NAME + ".network").get_model('vgg19')
    m.load_state_dict(net_oracle.he_init_state_dict(m, seed=0))
    return m.set_winograd(winograd3=0, winograd7=0)


def _openpose():
    m = importlib.import_module(PKG_NAME + ".openpose").OpenPose_Model(2, 2, 3, 2)
    m.load_state_dict(OR.seeded_state_dict(OR.state_dict_spec(2, 2, 3, 2), 4))
    return m.set_winograd(winograd3=0)


def _hourglass():
    m = importlib.import_module(PKG_NAME + ".hourglass").hg(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3)
    m.load_state_dict(HR.seeded_state_dict(HR.state_dict_spec(1, 1, 4, 3), 4, HR.STRONG_GAIN))
    return m.set_winograd(winograd3=0).eval()


# front -> (builder, input shape, outputs read_output knows after a forward that keeps the intermediates)
FRONTS = {"rtpose_vgg": (_vgg, (1, 3, 64, 64), 12), "openpose": (_openpose, (1, 3, 40, 24), 4),
          "hourglass": (_hourglass, (1, 3, 64, 64), 4)}


def _outputs(m, x, n_out):
    with torch.no_grad():
        plan = m.forward_native(x, keep_intermediates=True)
        return plan, [m.read_output(plan, i) for i in range(n_out)]


def _fresh_outputs(build, edited, x, n_out):
    fresh = build()
    fresh.load_state_dict(edited.state_dict())
    plan, outs = _outputs(fresh.cuda(), x, n_out)
    assert fresh.device_status(plan) == 0
    return outs


@pytest.mark.parametrize("front", sorted(FRONTS))
def test_edited_parameters_reach_the_device(cuda, front):
    build, shape, n_out = FRONTS[front]
    x = (torch.rand(*shape, generator=torch.Generator().manual_seed(9)) - 0.5).to(cuda)
    m = build().cuda()
    first, last = m._convs()[0][1], m._convs()[-1][1]
    plan, before = _outputs(m, x, n_out)
    assert all(float(o.abs().max()) > 0.0 for o in before)

    with torch.no_grad():                   # an edit the version counters see
        first.weight.mul_(1.5)
        last.bias.add_(0.25)
    plan2, after = _outputs(m, x, n_out)
    assert plan2 is plan
    want = _fresh_outputs(build, m, x, n_out)
    for i in range(n_out):
        assert torch.equal(after[i], want[i]), (front, i, float((after[i] - want[i]).abs().max()))
        assert not torch.equal(after[i], before[i]), (front, i)

    first.weight.data.mul_(0.5)             # an edit through .data, which they do not see: the caller says so
    last.bias.data.sub_(0.125)
    m.invalidate_weights()
    _, again = _outputs(m, x, n_out)
    want = _fresh_outputs(build, m, x, n_out)
    for i in range(n_out):
        assert torch.equal(again[i], want[i]), (front, i, float((again[i] - want[i]).abs().max()))
        assert not torch.equal(again[i], after[i]), (front, i)
    assert m.device_status(plan) == 0
