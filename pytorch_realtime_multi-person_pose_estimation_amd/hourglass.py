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
from ._capi import lib, check, ptr, current_stream
from ._native_state import NativeStateMixin, NetPlanMixin
from .network import _ShapeOnly

NUM_JOINTS = 18
NUM_LIMBS = 38


def _bn_affine64(bn):
    """Inference BatchNorm2d as y = scale * x + shift, float64, with the module's own eps."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def bn_scale_shift(bn):
    """(scale, shift) of an inference BatchNorm2d as fp32 vectors (float64 arithmetic)."""
    scale, shift = _bn_affine64(bn)
    return scale.float(), shift.float()


def fold_bn(weight, bias, bn):
    """Filters and bias of ``bn(conv(x))`` as one conv: w * scale[cout], b * scale + shift."""
    scale, shift = _bn_affine64(bn)
    w = weight.detach().double() * scale.view(-1, 1, 1, 1)
    b = (bias.detach().double() if bias is not None else torch.zeros_like(scale)) * scale + shift
    return w.float(), b.float()


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


class _Plan(object):
    """One native stacked-hourglass executor instance (fixed N, H, W) + its workspace."""

    def __init__(self, n, h, w, weights, device, topo, wino):
        handle = C.c_void_p()
        opts = _capi.HourglassOptions.make(*(topo + wino))
        check(lib.rtpose_hourglass_create(n, h, w, C.byref(opts), C.byref(handle)), "rtpose_hourglass_create")
        self.handle = handle
        self.shape = (n, h, w)
        self.dtype = _capi.DTYPE_F32
        self.wino = wino
        ws_bytes = lib.rtpose_net_workspace_bytes(handle)
        self.workspace = torch.empty(ws_bytes // 4 + 64, dtype=torch.float32, device=device)
        check(lib.rtpose_net_bind(handle, ptr(self.workspace), ws_bytes, ptr(weights),
                                  weights.numel() * 4, 1, current_stream()), "rtpose_net_bind")
        self.h3 = h // 4
        self.w3 = w // 4

    def __del__(self):
        try:
            lib.rtpose_net_destroy(self.handle)
        except Exception:
            pass


class HourglassNet(NativeStateMixin, NetPlanMixin, nn.Module):
    """Drop-in for reference ``HourglassNet`` (lib/network/rtpose_hourglass.py:92).  fp32, inference (``.eval()``) only;
    runs on an MI355X.  Its maps are at stride 4 (``output_stride``); H and W must be multiples of 64."""

    output_stride = 4

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
        self._wino = (_capi.WINO_DEFAULT, 0.0)

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
        if winograd3 is None:
            w3 = _capi.WINO_DEFAULT
        elif winograd3 == 'auto':
            w3 = _capi.WINO3_AUTO
        elif winograd3 in (1, 2):
            w3 = 1
        elif winograd3 in (0, 4):
            w3 = int(winograd3)
        else:
            raise ValueError("winograd3 must be None, False / 0, True / 1 / 2, 4 or 'auto'")
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

    def _sync_weights(self, plan, device):
        convs = self._convs()
        wkey = (device.index, plan.dtype)
        tensors = []
        for _, m, bn, _, pbn in convs:
            tensors += [m.weight, m.bias]
            for b in (bn, pbn):
                if b is not None:
                    tensors += [b.weight, b.bias, b.running_mean, b.running_var]
        key = self._params_key(tensors)
        if key == self._weights_key.get(wkey) and not self.always_resync:
            return
        n = lib.rtpose_net_num_convs(plan.handle)
        if n != len(convs):
            raise _capi.RtposeError("native plan has %d convs, module has %d" % (n, len(convs)))
        name = C.create_string_buffer(96)
        co, ci, k = C.c_int(), C.c_int(), C.c_int()
        stream = current_stream()
        keep = []  # temporaries stay alive until the stream has consumed them

        def dev(t):
            t = t.detach()
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t
        for i, (nm, m, bn, pnm, pbn) in enumerate(convs):
            check(lib.rtpose_net_conv_info(plan.handle, i, name, 96, C.byref(co), C.byref(ci), C.byref(k)))
            if name.value.decode() != nm or tuple(m.weight.shape) != (co.value, ci.value, k.value, k.value):
                raise _capi.RtposeError("conv %d mismatch: native %s vs module %s" % (i, name.value, nm))
            w, b = (m.weight, m.bias) if bn is None else fold_bn(m.weight, m.bias, bn)
            check(lib.rtpose_net_load_conv(plan.handle, i, ptr(dev(w)), ptr(dev(b)), stream), "rtpose_net_load_conv")
            has = lib.rtpose_net_preact_info(plan.handle, i, name, 96)
            if has < 0 or bool(has) != (pbn is not None) or (pbn is not None and name.value.decode() != pnm):
                raise _capi.RtposeError("pre-activation of conv %d mismatch: native %s vs module %s" % (i, name.value, pnm))
            if pbn is not None:
                sc, sh = bn_scale_shift(pbn)
                if sc.numel() != ci.value:
                    raise _capi.RtposeError("%s has %d channels, the conv reads %d" % (pnm, sc.numel(), ci.value))
                check(lib.rtpose_net_load_preact(plan.handle, i, ptr(dev(sc)), ptr(dev(sh)), stream),
                      "rtpose_net_load_preact")
        torch.cuda.current_stream().synchronize()  # temporaries above may be freed
        del keep
        self._weights_key[wkey] = key

    def _require_eval(self):
        if self.training:
            raise _capi.RtposeError(
                "HourglassNet runs its BatchNorm layers on their running statistics only: call .eval() first (a fresh "
                "nn.Module is in training mode; there is no training-mode forward and no CPU fallback)")

    def plan_for(self, x):
        if not x.is_cuda:
            raise _capi.RtposeError(
                "HourglassNet forward runs only on an MI355X (HIP) device tensor; got a %s tensor - "
                "there is deliberately no CPU fallback" % x.device)
        n, c, h, w = x.shape
        if c != 3:
            raise _capi.RtposeError("expected NCHW input with 3 channels")
        return self.plan_for_shape(n, h, w, x.device)

    def plan_for_shape(self, n, h, w, device):
        """The executor instance for N x 3 x H x W inputs on `device` (created on first use)."""
        self._require_eval()
        x = _ShapeOnly(device)
        key = (n, h, w, x.device.index, _capi.DTYPE_F32, self._wino)
        with self._native_lock, torch.cuda.device(x.device):
            plan = self._plans.get(key)
            if plan is None:
                wkey = (x.device.index, _capi.DTYPE_F32)
                weights = self._weights.get(wkey)
                if weights is None:
                    probe = C.c_void_p()
                    opts = _capi.HourglassOptions.make(*self._topo)
                    check(lib.rtpose_hourglass_create(1, 64, 64, C.byref(opts), C.byref(probe)))
                    wb = lib.rtpose_net_weight_bytes(probe)
                    lib.rtpose_net_destroy(probe)
                    weights = torch.zeros(wb // 4 + 64, dtype=torch.float32, device=x.device)
                    self._weights[wkey] = weights
                    self._weights_key.pop(wkey, None)
                plan = self._build_plan(key, lambda: _Plan(n, h, w, weights, x.device, self._topo, self._wino))
            self._sync_weights(plan, x.device)
            check(lib.rtpose_net_finalize_weights(plan.handle, current_stream()), "rtpose_net_finalize_weights")
        return plan

    def read_output(self, plan, which):
        """0 / 1: score_paf / score_ht of the last stack; 2 + 2 s / 3 + 2 s: of stack s (kept only by a forward with
        keep_intermediates).  NCHW fp32."""
        _, _, p, h = self._topo
        out = torch.empty((plan.shape[0], p if which % 2 == 0 else h, plan.h3, plan.w3), dtype=torch.float32,
                          device=plan.workspace.device)
        check(lib.rtpose_net_read_output(plan.handle, which, ptr(out), current_stream()), "rtpose_net_read_output")
        return out

    def forward(self, x):
        """reference :162-189 - ``(score_paf, score_ht), [score_paf, score_ht]`` of the last stack, NCHW fp32."""
        self._require_eval()
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
