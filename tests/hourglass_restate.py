"""CPU restatement of the reference stacked hourglass (lib/network/rtpose_hourglass.py) and its seeded weights.

A helper module for the hourglass tests and ``tools/make_golden_hourglass.py`` (not a test file): ``forward`` states the
reference's eval-mode forward with ``F.conv2d`` / ``F.batch_norm`` / ``F.relu`` / ``F.max_pool2d`` /
``F.interpolate(nearest)`` on a state_dict, ``state_dict_spec`` lists the reference's state_dict keys and shapes in its
order, ``seeded_state_dict`` draws the weights the fixtures use from numpy's PCG64 (no dependence on torch's RNG).  The
generator checks ``forward`` against the reference module before it writes the fixture; the tests check it against the
fixture.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5                  # nn.BatchNorm2d default, what every BatchNorm of the reference has
BRANCH_GAIN = 0.006         # variance gain of the residual branches (see seeded_state_dict)
STRONG_GAIN = 0.25          # ... of the shallow configuration whose branches carry as much as the skip


def _bn(pre, c):
    return [(pre + '.weight', (c,)), (pre + '.bias', (c,)), (pre + '.running_mean', (c,)),
            (pre + '.running_var', (c,)), (pre + '.num_batches_tracked', ())]


def _conv(pre, co, ci, k):
    return [(pre + '.weight', (co, ci, k, k)), (pre + '.bias', (co,))]


def _bottleneck(pre, cin, planes, downsample):
    spec = _bn(pre + '.bn1', cin) + _conv(pre + '.conv1', planes, cin, 1) + _bn(pre + '.bn2', planes) \
        + _conv(pre + '.conv2', planes, planes, 3) + _bn(pre + '.bn3', planes) + _conv(pre + '.conv3', 2 * planes, planes, 1)
    if downsample:
        spec += _conv(pre + '.downsample.0', 2 * planes, cin, 1)
    return spec


def state_dict_spec(num_stacks, num_blocks, paf, heat):
    """[(key, shape)] of the reference module's state_dict, in its order (num_batches_tracked included)."""
    spec = _conv('conv1', 64, 3, 7) + _bn('bn1', 64)
    spec += _bottleneck('layer1.0', 64, 64, True) + _bottleneck('layer2.0', 128, 128, True) \
        + _bottleneck('layer3.0', 256, 128, False)
    for s in range(num_stacks):
        for i in range(4):
            for j in range(4 if i == 0 else 3):
                for b in range(num_blocks):
                    spec += _bottleneck('hg.%d.hg.%d.%d.%d' % (s, i, j, b), 256, 128, False)
    for s in range(num_stacks):
        for b in range(num_blocks):
            spec += _bottleneck('res.%d.%d' % (s, b), 256, 128, False)
    for s in range(num_stacks):
        spec += _conv('fc.%d.0' % s, 256, 256, 1) + _bn('fc.%d.1' % s, 256)
    for s in range(num_stacks):
        spec += _conv('score_ht.%d' % s, heat, 256, 1)
    for s in range(num_stacks):
        spec += _conv('score_paf.%d' % s, paf, 256, 1)
    for s in range(num_stacks - 1):
        spec += _conv('fc_.%d' % s, 256, 256, 1)
    for s in range(num_stacks - 1):
        spec += _conv('paf_score_.%d' % s, 256, paf, 1)
    for s in range(num_stacks - 1):
        spec += _conv('ht_score_.%d' % s, 256, heat, 1)
    return spec


def seeded_state_dict(spec, seed, gain=BRANCH_GAIN):
    """Weights whose maps neither vanish nor explode through 115 residual additions.  The reference init (N(0, 0.01))
    makes the maps vanish; plain He init explodes, because seeded BatchNorm statistics do not normalise.  Filters are
    N(0, v / fan_in): v = 2 in front of a ReLU (conv1, conv2, the stem, downsample, fc), v = 1 for the score heads,
    v = `gain` for what is added to a skip (conv3, fc_, paf_score_, ht_score_).  Biases N(0, 0.05); BatchNorm weight
    U(0.5, 1.5), bias N(0, 0.1), running_mean N(0, 0.1), running_var U(0.5, 1.5).  Drawn in state_dict order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    norms = set(k[:-len('.running_mean')] for k, _ in spec if k.endswith('.running_mean'))
    sd = {}
    for k, shp in spec:
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros((), dtype=torch.int64)
            continue
        if len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            mod = k[:-len('.weight')]
            if mod.startswith('score_'):
                var = 1.0
            elif mod.endswith('.conv3') or mod.split('.')[0] in ('fc_', 'paf_score_', 'ht_score_'):
                var = gain
            else:
                var = 2.0
            v = rng.standard_normal(shp) * np.sqrt(var / fan_in)
        elif k.endswith('running_var'):
            v = rng.uniform(0.5, 1.5, shp)
        elif k.endswith('running_mean'):
            v = rng.standard_normal(shp) * 0.1
        elif k.rsplit('.', 1)[0] in norms:
            v = rng.uniform(0.5, 1.5, shp) if k.endswith('weight') else rng.standard_normal(shp) * 0.1
        else:   # conv bias
            v = rng.standard_normal(shp) * 0.05
        sd[k] = torch.from_numpy(np.asarray(v, np.float32))
    return sd


def _bnf(sd, pre, x):
    return F.batch_norm(x, sd[pre + '.running_mean'], sd[pre + '.running_var'], sd[pre + '.weight'], sd[pre + '.bias'],
                        False, 0.0, EPS)


def _cv(sd, pre, x, **kw):
    return F.conv2d(x, sd[pre + '.weight'], sd[pre + '.bias'], **kw)


def bottleneck(sd, pre, x):
    """rtpose_hourglass.py:26-46."""
    out = _cv(sd, pre + '.conv1', F.relu(_bnf(sd, pre + '.bn1', x)))
    out = _cv(sd, pre + '.conv2', F.relu(_bnf(sd, pre + '.bn2', out)), padding=1)
    out = _cv(sd, pre + '.conv3', F.relu(_bnf(sd, pre + '.bn3', out)))
    res = _cv(sd, pre + '.downsample.0', x) if (pre + '.downsample.0.weight') in sd else x
    return out + res


def _seq(sd, pre, x, num_blocks):
    for b in range(num_blocks):
        x = bottleneck(sd, '%s.%d' % (pre, b), x)
    return x


def _hourglass(sd, pre, n, x, nb):
    """rtpose_hourglass.py:74-86."""
    up1 = _seq(sd, '%s.hg.%d.0' % (pre, n - 1), x, nb)
    low1 = _seq(sd, '%s.hg.%d.1' % (pre, n - 1), F.max_pool2d(x, 2, stride=2), nb)
    low2 = _hourglass(sd, pre, n - 1, low1, nb) if n > 1 else _seq(sd, '%s.hg.0.3' % pre, low1, nb)
    low3 = _seq(sd, '%s.hg.%d.2' % (pre, n - 1), low2, nb)
    return up1 + F.interpolate(low3, scale_factor=2, mode='nearest')


def forward(sd, x, num_stacks, num_blocks, all_stacks=False):
    """rtpose_hourglass.py:162-189 (eval mode) on a state_dict -> (score_paf, score_ht) of the last stack, fp32 NCHW;
    all_stacks: the list of every stack's pair instead."""
    x = F.relu(_bnf(sd, 'bn1', _cv(sd, 'conv1', x, stride=2, padding=3)))
    x = bottleneck(sd, 'layer1.0', x)
    x = F.max_pool2d(x, 2, stride=2)
    x = bottleneck(sd, 'layer2.0', x)
    x = bottleneck(sd, 'layer3.0', x)
    outs = []
    for i in range(num_stacks):
        y = _hourglass(sd, 'hg.%d' % i, 4, x, num_blocks)
        y = _seq(sd, 'res.%d' % i, y, num_blocks)
        y = F.relu(_bnf(sd, 'fc.%d.1' % i, _cv(sd, 'fc.%d.0' % i, y)))
        paf, ht = _cv(sd, 'score_paf.%d' % i, y), _cv(sd, 'score_ht.%d' % i, y)
        outs.append((paf, ht))
        if i < num_stacks - 1:
            x = x + _cv(sd, 'fc_.%d' % i, y) + _cv(sd, 'paf_score_.%d' % i, paf) + _cv(sd, 'ht_score_.%d' % i, ht)
    return outs if all_stacks else outs[-1]
