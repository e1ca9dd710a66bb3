"""Host-side mirror of ``lib/network/rtpose_hourglass.py``, the stacked hourglass of ``train/train_SH.py:279``.

``hg(num_stacks=8, num_blocks=1, paf_classes=38, ht_classes=19)`` builds a ``HourglassNet`` with the reference's module
tree (``conv1``, ``bn1``, ``layer1..3``, ``hg``, ``res``, ``fc``, ``score_ht``, ``score_paf``, ``fc_``, ``paf_score_``,
``ht_score_``; pre-activation ``Bottleneck``) so that its state_dict keys, shapes and order, ``load_state_dict`` and
``_initialize_weights_norm`` are the reference's.  ``forward`` does not run those children: it hands the input to the
native executor (csrc/net.hip, ``rtpose_hourglass_create``), an fp32 inference plan of hand-written HIP kernels.

BatchNorm runs on its running statistics only (``.eval()``).  A BatchNorm that follows a conv is folded into that conv
on the host (``fold_bn``); ``bn1`` of a Bottleneck precedes its conv and is handed to the plan as a per-channel
(scale, shift) the conv applies while it stages its input (``bn_scale_shift``).  torch is used for device memory and
streams.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _capi
from ._capi import lib, check
from ._native_state import ConvRecord, NativeStateMixin, NetPlanMixin, bn_scale_shift, fold_bn  # noqa: F401 (re-exported)

NUM_JOINTS = 18
NUM_LIMBS = 38


# ---- the topology, as the plan builder (csrc/net.hip, build_plan_hourglass) and tests/hourglass_restate.py state it ----
FEATS = 256                 # channels of every map from layer2 on; a Bottleneck there is 256 -> 128 -> 128 -> 256
DEPTH = 4                   # levels of an hourglass: maps of H/4 .. H/64
# the three Bottlenecks in front of the stacks: (attribute, cin, planes, a 1x1 `downsample` on the skip)
_FRONT = (('layer1', 64, 64, True), ('layer2', 128, 128, True), ('layer3', FEATS, FEATS // 2, False))


def _conv1x1(cin, cout):
    return nn.Conv2d(cin, cout, kernel_size=1)


def _chain(num_blocks):
    """num_blocks 256 -> 256 Bottlenecks, children '0', '1', ..."""
    return nn.Sequential(*[Bottleneck(FEATS, FEATS // 2) for _ in range(num_blocks)])


class Bottleneck(nn.Module):
    """Parameter container of the pre-activation Bottleneck (reference :9-46): children in state_dict order bn1, conv1
    (1x1, cin -> planes), bn2, conv2 (3x3), bn3, conv3 (1x1, planes -> 2 planes) and, where the skip changes width,
    downsample.0 (1x1, cin -> 2 planes)."""
    expansion = 2

    def __init__(self, inplanes, planes, downsample=False):
        super(Bottleneck, self).__init__()
        widths = (inplanes, planes, planes, self.expansion * planes)
        for i, k in enumerate((1, 3, 1)):
            self.add_module('bn%d' % (i + 1), nn.BatchNorm2d(widths[i]))
            self.add_module('conv%d' % (i + 1), nn.Conv2d(widths[i], widths[i + 1], kernel_size=k, padding=k // 2))
        self.downsample = nn.Sequential(_conv1x1(inplanes, widths[3])) if downsample else None

    def convs(self, pre):
        """[(conv prefix, Conv2d, BatchNorm folded behind it or None, pre-activation prefix or None, its BatchNorm)]"""
        out = [(pre + '.conv1', self.conv1, self.bn2, pre + '.bn1', self.bn1),
               (pre + '.conv2', self.conv2, self.bn3, None, None),
               (pre + '.conv3', self.conv3, None, None, None)]
        if self.downsample is not None:
            out.append((pre + '.downsample.0', self.downsample[0], None, None, None))
        return out


class Hourglass(nn.Module):
    """Parameter container of one depth-`depth` hourglass (reference :49-89): hg[i][j] is the Bottleneck chain j (0 up1,
    1 low1, 2 low3; 3 low2, at the innermost level i = 0 only) of level i."""

    def __init__(self, num_blocks, depth=DEPTH):
        super(Hourglass, self).__init__()
        self.depth = depth
        self.hg = nn.ModuleList(nn.ModuleList(_chain(num_blocks) for _ in range(3 if i else 4)) for i in range(depth))


class HourglassNet(NativeStateMixin, NetPlanMixin, nn.Module):
    """Drop-in for reference ``HourglassNet`` (lib/network/rtpose_hourglass.py:92).  fp32, inference (``.eval()``) only;
    runs on an MI355X.  Its maps are at stride 4 (``output_stride``); H and W must be multiples of 64."""

    output_stride = 4
    _front_name = 'HourglassNet'
    _plan_stride = output_stride
    _probe_hw = 64
    _WINO_DEFAULT = (_capi.WINO_DEFAULT, 0.0)   # (winograd3, amp_limit)

    def __init__(self, block=Bottleneck, num_stacks=2, num_blocks=4, paf_classes=2 * NUM_LIMBS, ht_classes=NUM_JOINTS + 1):
        super(HourglassNet, self).__init__()
        if block is not Bottleneck:
            raise ValueError("HourglassNet: block must be hourglass.Bottleneck")
        for nm, v, hi in (('num_stacks', num_stacks, 64), ('num_blocks', num_blocks, 16),
                          ('paf_classes', paf_classes, 64), ('ht_classes', ht_classes, 64)):
            if not isinstance(v, int) or not 1 <= v <= hi:
                raise ValueError("HourglassNet: %s must be an int in 1..%d; got %r" % (nm, hi, v))
        self.num_stacks = num_stacks
        self._topo = (num_stacks, num_blocks, paf_classes, ht_classes)
        self.paf_out_channels, self.heat_out_channels = paf_classes, ht_classes
        # children in the reference's registration (== state_dict) order: stem, front, then one ModuleList per role with
        # an entry per stack - the heat-map head before the PAF head, the three hand-over convs for every stack but the last
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.bn1 = nn.BatchNorm2d(64)
        for name, cin, planes, ds in _FRONT:
            self.add_module(name, nn.Sequential(Bottleneck(cin, planes, ds)))
        per_stack = (('hg', lambda: Hourglass(num_blocks), 0),
                     ('res', lambda: _chain(num_blocks), 0),
                     ('fc', lambda: nn.Sequential(_conv1x1(FEATS, FEATS), nn.BatchNorm2d(FEATS)), 0),
                     ('score_ht', lambda: _conv1x1(FEATS, ht_classes), 0),
                     ('score_paf', lambda: _conv1x1(FEATS, paf_classes), 0),
                     ('fc_', lambda: _conv1x1(FEATS, FEATS), 1),
                     ('paf_score_', lambda: _conv1x1(paf_classes, FEATS), 1),
                     ('ht_score_', lambda: _conv1x1(ht_classes, FEATS), 1))
        for name, make, fewer in per_stack:
            self.add_module(name, nn.ModuleList(make() for _ in range(num_stacks - fewer)))
        self._initialize_weights_norm()
        self._init_native_state()
        self.compute_dtype = 'fp32'
        self._wino = self._WINO_DEFAULT

    def _initialize_weights_norm(self):
        """The reference's initial values (:191-199): filters N(0, 0.01), biases 0, BatchNorm weight 1 and bias 0."""
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.normal_(0.0, 0.01)
                    m.bias.zero_()
                elif isinstance(m, nn.BatchNorm2d):
                    m.weight.fill_(1.0)
                    m.bias.zero_()

    def set_winograd(self, winograd3=None, amp_limit=None):
        """Arithmetic of the 3x3 convs (conv2 of every Bottleneck) of plans created from now on, as
        ``OpenPose_Model.set_winograd``: None = library default ('auto'), False / 0 = direct, True / 1 / 2 = F(2x2,3x3),
        4 = F(4x4,3x3) forced, 'auto' = per layer F(4x4,3x3) if its amplification estimate is <= ``amp_limit`` (default
        256), else F(2x2,3x3)."""
        w3 = self._parse_winograd3(winograd3)
        self._wino = (w3, float(amp_limit or 0.0))
        return self

    def set_compute_dtype(self, dtype):
        if dtype != 'fp32':
            raise ValueError("HourglassNet runs in fp32 only (bf16 / bf16x3 plans exist for rtpose_vgg); got %r" % (dtype,))
        self.compute_dtype = dtype
        return self

    # ---- native side -------------------------------------------------------
    def _convs(self):
        """[(conv prefix, Conv2d, BatchNorm2d folded behind it or None, pre-activation prefix or None, its BatchNorm2d
        or None)] in the executor's index order (== the order of the nn.Conv2d in the state_dict)."""
        out = [('conv1', self.conv1, self.bn1, None, None)]

        def seq(pre, s):
            for b, blk in enumerate(s):
                out.extend(blk.convs('%s.%d' % (pre, b)))
        for nm in ('layer1', 'layer2', 'layer3'):
            seq(nm, getattr(self, nm))
        for s, h in enumerate(self.hg):
            for i, level in enumerate(h.hg):
                for j, res in enumerate(level):
                    seq('hg.%d.hg.%d.%d' % (s, i, j), res)
        for s, res in enumerate(self.res):
            seq('res.%d' % s, res)
        for s, fc in enumerate(self.fc):
            out.append(('fc.%d.0' % s, fc[0], fc[1], None, None))
        for nm in ('score_ht', 'score_paf', 'fc_', 'paf_score_', 'ht_score_'):
            for s, m in enumerate(getattr(self, nm)):
                out.append(('%s.%d' % (nm, s), m, None, None, None))
        return out

    def _conv_record(self, entry):
        nm, m, bn, pnm, pbn = entry
        return ConvRecord(nm, m, bn, None, (pnm, pbn) if pbn is not None else None)

    def _create(self, n, h, w, dtype, wino):
        handle = C.c_void_p()
        opts = _capi.HourglassOptions.make(*(self._topo + wino))
        check(lib.rtpose_hourglass_create(n, h, w, C.byref(opts), C.byref(handle)), "rtpose_hourglass_create")
        return handle

    def _check_ready(self):
        if self.training:
            raise _capi.RtposeError(
                "HourglassNet runs its BatchNorm layers on their running statistics only: call .eval() first (a fresh "
                "nn.Module is in training mode; there is no training-mode forward and no CPU fallback)")

    def _out_channels(self, which):
        """0 / 1: score_paf / score_ht of the last stack; 2 + 2 s / 3 + 2 s: of stack s (kept only by a forward with
        keep_intermediates)"""
        return self._topo[2] if which % 2 == 0 else self._topo[3]

    def forward(self, x):
        """reference :162-189 - ``(score_paf, score_ht), [score_paf, score_ht]`` of the last stack, NCHW fp32."""
        self._check_ready()
        if not x.is_cuda:
            self.plan_for(x)  # raises: no CPU fallback
        with torch.cuda.device(x.device):
            plan = self.forward_native(x)
            score_paf, score_ht = self.read_output(plan, 0), self.read_output(plan, 1)
        return (score_paf, score_ht), [score_paf, score_ht]


def hg(**kwargs):
    """``hg(num_stacks=, num_blocks=, paf_classes=, ht_classes=)`` -> HourglassNet (reference :201); all four are required."""
    names = ('num_stacks', 'num_blocks', 'paf_classes', 'ht_classes')
    return HourglassNet(Bottleneck, *[kwargs[k] for k in names])
