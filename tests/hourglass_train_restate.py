"""CPU restatement of the reference stacked hourglass (lib/network/rtpose_hourglass.py) in TRAINING mode, on a dict of
tensors: ``forward`` states the reference's forward with ``F.conv2d`` / ``F.batch_norm(training=True)`` / ``F.relu`` /
``F.max_pool2d`` / ``F.interpolate(nearest)``, in the reference's order of operations and additions, and updates the
running statistics of the dict in place as nn.BatchNorm2d does (momentum 0.1, eps 1e-5, num_batches_tracked + 1).

A helper of tests/test_batchnorm_cpu.py and tests/test_train_hourglass_gpu.py, written from the reference's text and
independent of train.hourglass_forward, which it is compared with: both run the same torch operations in the same order,
so in one dtype on one device outputs, gradients and running statistics are equal bit for bit.
"""
import torch
import torch.nn.functional as F

import hourglass_restate as hr

MOMENTUM = 0.1


def tensors_of(model, dtype=torch.float64, device="cpu"):
    """{key: tensor} of the module's state_dict, detached copies in `dtype` (num_batches_tracked stays int64); the
    parameters require a gradient"""
    params = set(k for k, _ in model.named_parameters())
    out = {}
    for k, v in model.state_dict().items():
        t = v.detach().clone().to(device)
        if t.is_floating_point():
            t = t.to(dtype)
        out[k] = t.requires_grad_(True) if k in params else t
    return out


def _bn_relu(sd, pre, x):
    sd[pre + '.num_batches_tracked'] += 1
    return F.relu(F.batch_norm(x, sd[pre + '.running_mean'], sd[pre + '.running_var'], sd[pre + '.weight'], sd[pre + '.bias'],
                               True, MOMENTUM, hr.EPS))


def _cv(sd, pre, x, **kw):
    return F.conv2d(x, sd[pre + '.weight'], sd[pre + '.bias'], **kw)


def bottleneck(sd, pre, x):
    """rtpose_hourglass.py:26-46"""
    out = _cv(sd, pre + '.conv1', _bn_relu(sd, pre + '.bn1', x))
    out = _cv(sd, pre + '.conv2', _bn_relu(sd, pre + '.bn2', out), padding=1)
    out = _cv(sd, pre + '.conv3', _bn_relu(sd, pre + '.bn3', out))
    res = _cv(sd, pre + '.downsample.0', x) if (pre + '.downsample.0.weight') in sd else x
    return out + res


def _seq(sd, pre, x, nb):
    for b in range(nb):
        x = bottleneck(sd, '%s.%d' % (pre, b), x)
    return x


def _hourglass(sd, pre, n, x, nb):
    """rtpose_hourglass.py:74-86"""
    up1 = _seq(sd, '%s.hg.%d.0' % (pre, n - 1), x, nb)
    low1 = _seq(sd, '%s.hg.%d.1' % (pre, n - 1), F.max_pool2d(x, 2, stride=2), nb)
    low2 = _hourglass(sd, pre, n - 1, low1, nb) if n > 1 else _seq(sd, '%s.hg.0.3' % pre, low1, nb)
    low3 = _seq(sd, '%s.hg.%d.2' % (pre, n - 1), low2, nb)
    return up1 + F.interpolate(low3, scale_factor=2, mode='nearest')


def forward(sd, x, num_stacks, num_blocks):
    """rtpose_hourglass.py:162-189 in training mode -> (score_paf, score_ht) of the last stack"""
    x = _bn_relu(sd, 'bn1', _cv(sd, 'conv1', x, stride=2, padding=3))
    x = bottleneck(sd, 'layer1.0', x)
    x = F.max_pool2d(x, 2, stride=2)
    x = bottleneck(sd, 'layer2.0', x)
    x = bottleneck(sd, 'layer3.0', x)
    paf = ht = None
    for i in range(num_stacks):
        y = _hourglass(sd, 'hg.%d' % i, 4, x, num_blocks)
        y = _seq(sd, 'res.%d' % i, y, num_blocks)
        y = _bn_relu(sd, 'fc.%d.1' % i, _cv(sd, 'fc.%d.0' % i, y))
        paf = _cv(sd, 'score_paf.%d' % i, y)
        ht = _cv(sd, 'score_ht.%d' % i, y)
        if i < num_stacks - 1:
            fc_ = _cv(sd, 'fc_.%d' % i, y)
            paf_ = _cv(sd, 'paf_score_.%d' % i, paf)
            ht_ = _cv(sd, 'ht_score_.%d' % i, ht)
            x = x + fc_ + paf_ + ht_
    return paf, ht


# ---- the callables train.hourglass_forward takes, in torch -----------------------------------------------------------------------------
def torch_ops():
    """(conv, bn, stem) of torch's own modules' functional forms, in the modules' dtype: what train.hourglass_forward runs
    when the tests hand it torch instead of the library"""
    def conv(x, m):
        return F.conv2d(x, m.weight, m.bias, stride=m.stride, padding=m.padding)

    def bn(x, m):
        m.num_batches_tracked += 1
        return F.relu(F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps))

    return conv, bn, conv


def seed_model(model, seed, gain=None):
    """hourglass_restate.seeded_state_dict into `model` (He-scaled filters, conv3 and the hand-over convs damped)"""
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(hr.seeded_state_dict(spec, seed, hr.STRONG_GAIN if gain is None else gain))
    return model
