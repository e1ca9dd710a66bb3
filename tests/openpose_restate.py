"""CPU restatement of reference ``OpenPose_Model`` (lib/network/openpose.py:114-177) and its seeded weights.

A helper module for the OpenPose tests and ``tools/make_golden_openpose.py`` (not a test file): ``forward`` states
the reference's forward with ``F.conv2d`` / ``F.prelu`` / ``F.relu`` / ``F.max_pool2d`` / ``torch.cat`` on a
state_dict, ``seeded_state_dict`` draws the weights the fixtures use from numpy's PCG64 (no dependence on torch's
RNG).  The generator checks ``forward`` against the reference module before it writes the fixture; the tests check it
against the fixture.
"""
import numpy as np
import torch
import torch.nn.functional as F

# feature_extractor: (index, PReLU follows) per conv; 'P' = MaxPool2d(2, 2, 0)   (openpose.py:13-49)
TRUNK = [(0, False), (2, False), 'P', (5, False), (7, False), 'P', (10, False), (12, False), (14, False), (16, False),
         'P', (19, False), (21, True), (23, True), (25, True)]
SLOPE_RANGE = (-0.5, 1.5)   # per-channel PReLU slopes: negative ones and ones above 1 included


def state_dict_spec(l2_stages, l1_stages, paf, heat):
    """[(key, shape)] of the reference module's state_dict, in its order."""
    spec = []
    trunk = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 512),
             (512, 512), (512, 256), (256, 128)]
    convs = [e for e in TRUNK if e != 'P']
    for (i, pr), (ci, co) in zip(convs, trunk):
        spec += [('feature_extractor.%d.weight' % i, (co, ci, 3, 3)), ('feature_extractor.%d.bias' % i, (co,))]
        if pr:
            spec.append(('feature_extractor.%d.weight' % (i + 1), (co,)))
    for br, n in (('l2_stages', l2_stages), ('l1_stages', l1_stages)):
        for s in range(n):
            inner = 96 if s == 0 else 128
            n1 = 256 if s == 0 else 512
            out = paf if br == 'l2_stages' else heat
            cin0 = (128 if s == 0 else 128 + paf) if br == 'l2_stages' else (128 + paf if s == 0 else 128 + paf + heat)
            pre = '%s.%d.' % (br, s)
            for b in range(1, 6):
                for j in range(3):
                    ci = (cin0 if b == 1 else 3 * inner) if j == 0 else inner
                    k = pre + 'Mconv%d_%d.' % (b, j)
                    spec += [(k + 'Mconv.weight', (inner, ci, 3, 3)), (k + 'Mconv.bias', (inner,)),
                             (k + 'MPrelu.weight', (inner,))]
            spec += [(pre + 'Mconv6.Mconv.weight', (n1, 3 * inner, 1, 1)), (pre + 'Mconv6.Mconv.bias', (n1,)),
                     (pre + 'Mconv6.MPrelu.weight', (n1,)), (pre + 'Mconv7.weight', (out, n1, 1, 1)),
                     (pre + 'Mconv7.bias', (out,))]
    return spec


def seeded_state_dict(spec, seed):
    """Weights whose maps neither vanish nor explode through the ~100 layers (the reference init, N(0, 0.01), drives the
    outputs to ~1e-3 of the bias: useless for a parity test): conv filters N(0, 2 / (fan_in (1 + E[a^2]))) where a PReLU
    with slopes a follows, N(0, 2 / fan_in) before a ReLU, N(0, 1 / fan_in) for the linear Mconv7; biases N(0, 0.05);
    slopes uniform in SLOPE_RANGE."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = SLOPE_RANGE
    ea2 = (hi ** 3 - lo ** 3) / (3.0 * (hi - lo))
    keys = [k for k, _ in spec]
    sd = {}
    for i, (k, shp) in enumerate(spec):
        if len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            nxt = keys[i + 2] if i + 2 < len(keys) else ''
            prelu_next = nxt.endswith('MPrelu.weight') or (k.startswith('feature_extractor') and
                                                           dict(spec).get(nxt, (0, 0))[:1] == shp[:1] and
                                                           len(dict(spec)[nxt]) == 1)
            if k.endswith('Mconv7.weight'):
                var = 1.0 / fan_in
            elif prelu_next:
                var = 2.0 / (fan_in * (1.0 + ea2))
            else:
                var = 2.0 / fan_in
            v = rng.standard_normal(shp) * np.sqrt(var)
        elif k.endswith('bias'):
            v = rng.standard_normal(shp) * 0.05
        else:  # PReLU slopes
            v = rng.uniform(lo, hi, shp)
        sd[k] = torch.from_numpy(v.astype(np.float32))
    return sd


def _stage(sd, pre, x):
    def cb(name, t):
        k = pre + name
        y = F.conv2d(t, sd[k + '.Mconv.weight'], sd[k + '.Mconv.bias'], padding=sd[k + '.Mconv.weight'].shape[-1] // 2)
        return F.prelu(y, sd[k + '.MPrelu.weight'])
    for b in range(1, 6):
        o1 = cb('Mconv%d_0' % b, x)
        o2 = cb('Mconv%d_1' % b, o1)
        o3 = cb('Mconv%d_2' % b, o2)
        x = torch.cat([o1, o2, o3], 1)
    y = cb('Mconv6', x)
    return F.conv2d(y, sd[pre + 'Mconv7.weight'], sd[pre + 'Mconv7.bias'])


def forward(sd, x, l2_stages, l1_stages):
    """openpose.py:160-177 on a state_dict -> (paf_ret, heat_ret) lists, fp32 NCHW."""
    t = x
    for e in TRUNK:
        if e == 'P':
            t = F.max_pool2d(t, 2, 2, 0)
            continue
        i, pr = e
        t = F.conv2d(t, sd['feature_extractor.%d.weight' % i], sd['feature_extractor.%d.bias' % i], padding=1)
        t = F.prelu(t, sd['feature_extractor.%d.weight' % (i + 1)]) if pr else F.relu(t)
    features = t
    paf_ret, heat_ret = [], []
    x_in = features
    paf = None
    for s in range(l2_stages):
        paf = _stage(sd, 'l2_stages.%d.' % s, x_in)
        x_in = torch.cat([features, paf], 1)
        paf_ret.append(paf)
    for s in range(l1_stages):
        heat = _stage(sd, 'l1_stages.%d.' % s, x_in)
        x_in = torch.cat([features, heat, paf], 1)
        heat_ret.append(heat)
    return paf_ret, heat_ret
