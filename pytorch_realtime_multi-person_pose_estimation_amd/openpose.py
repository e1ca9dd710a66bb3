"""Host-side mirror of ``lib/network/openpose.py`` (reference :114-210), the later OpenPose architecture.

``OpenPose_Model(l2_stages, l1_stages, paf_out_channels, heat_out_channels)`` has the reference's module tree
(``feature_extractor``, ``l2_stages``, ``l1_stages``; ``ConvBlock`` = ``Mconv`` + ``MPrelu``) so that its state_dict
keys and shapes, ``load_state_dict`` and ``init_w_pretrained_weights`` are the reference's.  ``forward`` does not run
those children: it hands the input to the native executor (csrc/net.hip, ``rtpose_openpose_create``), an fp32 plan
whose convolutions and PReLU epilogues are the hand-written HIP kernels.  torch is used for device memory and streams.
"""
import ctypes as C
import pickle

import torch
import torch.nn as nn

from . import _capi
from ._capi import lib, check
from ._native_state import ConvRecord, NativeStateMixin, NetPlanMixin

# reference :13-49: (name, cin, cout) or 'P' = MaxPool2d(2, 2, 0); conv4_2, conv4_3_CPM, conv4_4_CPM end in a PReLU
_VGG = [('conv1_1', 3, 64), ('conv1_2', 64, 64), 'P', ('conv2_1', 64, 128), ('conv2_2', 128, 128), 'P',
        ('conv3_1', 128, 256), ('conv3_2', 256, 256), ('conv3_3', 256, 256), ('conv3_4', 256, 256), 'P',
        ('conv4_1', 256, 512), ('conv4_2', 512, 512), ('conv4_3_CPM', 512, 256), ('conv4_4_CPM', 256, 128)]
_PRELU_TRUNK = ('conv4_2', 'conv4_3_CPM', 'conv4_4_CPM')


def make_vgg19_block():
    """reference :13-49."""
    layers = []
    for e in _VGG:
        if e == 'P':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2, padding=0))
            continue
        name, cin, cout = e
        layers.append(nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1))
        layers.append(nn.PReLU(num_parameters=cout) if name in _PRELU_TRUNK else nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


class ConvBlock(nn.Module):
    """reference :51-63 (parameter container only)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1):
        super(ConvBlock, self).__init__()
        self.Mconv = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                               stride=stride, padding=padding)
        self.MPrelu = nn.PReLU(num_parameters=out_channels)


class StageBlock(nn.Module):
    """reference :65-84 (parameter container only)."""

    def __init__(self, in_channels, inner_channels, innerout_channels, out_channels):
        super(StageBlock, self).__init__()
        for b in range(1, 6):
            for j in range(3):
                cin = (in_channels if b == 1 else inner_channels * 3) if j == 0 else inner_channels
                setattr(self, 'Mconv%d_%d' % (b, j), ConvBlock(cin, inner_channels))
        self.Mconv6 = ConvBlock(inner_channels * 3, innerout_channels, kernel_size=1, stride=1, padding=0)
        self.Mconv7 = nn.Conv2d(in_channels=innerout_channels, out_channels=out_channels, kernel_size=1, stride=1,
                                padding=0)

    def conv_blocks(self):
        """[(attribute, ConvBlock)] in registration (== state_dict) order, Mconv6 included."""
        return [('Mconv%d_%d' % (b, j), getattr(self, 'Mconv%d_%d' % (b, j))) for b in range(1, 6) for j in range(3)] \
            + [('Mconv6', self.Mconv6)]


class OpenPose_Model(NativeStateMixin, NetPlanMixin, nn.Module):
    """Drop-in for reference ``OpenPose_Model`` (lib/network/openpose.py:114).  fp32 only; runs on an MI355X."""

    _front_name = 'OpenPose_Model'
    _plan_stride = 8
    _probe_hw = 8
    _WINO_DEFAULT = (_capi.WINO_DEFAULT, 0.0)   # (winograd3, amp_limit)

    def __init__(self, l2_stages=4, l1_stages=2, paf_out_channels=14, heat_out_channels=9):
        super(OpenPose_Model, self).__init__()
        for nm, v in (('l2_stages', l2_stages), ('l1_stages', l1_stages)):
            if not isinstance(v, int) or v < 2:
                raise ValueError("OpenPose_Model: %s must be an int >= 2 (forward returns the last two stages of each "
                                 "branch); got %r" % (nm, v))
        for nm, v in (('paf_out_channels', paf_out_channels), ('heat_out_channels', heat_out_channels)):
            if not isinstance(v, int) or not 1 <= v <= 64:
                raise ValueError("OpenPose_Model: %s must be an int in 1..64; got %r" % (nm, v))
        self.stages = [0, 1]
        self.feature_extractor = make_vgg19_block()
        p, h = paf_out_channels, heat_out_channels
        # reference :133-158: stage 0 of each branch has 96 inner / 256 head channels, the others 128 / 512
        self.l2_stages = nn.ModuleList([StageBlock(128 if i == 0 else 128 + p, 96 if i == 0 else 128,
                                                   256 if i == 0 else 512, p) for i in range(l2_stages)])
        self.l1_stages = nn.ModuleList([StageBlock(128 + p if i == 0 else 128 + p + h, 96 if i == 0 else 128,
                                                   256 if i == 0 else 512, h) for i in range(l1_stages)])
        self._topo = (l2_stages, l1_stages, p, h)
        self.paf_out_channels, self.heat_out_channels = p, h
        self._initialize_weights_norm()
        self._init_native_state()
        self.compute_dtype = 'fp32'
        self._wino = self._WINO_DEFAULT

    def _initialize_weights_norm(self):
        # reference :179-187: N(0, 0.01) weights and slopes, bias 0.001
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0.001)
            elif isinstance(m, nn.PReLU):
                nn.init.normal_(m.weight, std=0.01)

    def init_w_pretrained_weights(self, pkl_weights):
        """reference :189-210: CMU's converted caffe weights (a pickled list of {'name', 'weights'}): the convs and
        PReLUs of the list, in order, go to this module's Conv2d / PReLU modules in module order."""
        with open(pkl_weights, 'rb') as f:
            weights = pickle.load(f, encoding='latin1')
        keep = lambda d: 'split' not in d['name'] and 'concat' not in d['name']  # noqa: E731
        conv_idxs = iter([i for i, d in enumerate(weights) if 'conv' in d['name'] and keep(d)])
        prelu_idxs = iter([i for i, d in enumerate(weights) if 'prelu' in d['name'] and keep(d)])
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                idx = next(conv_idxs)
                m.weight = nn.Parameter(torch.Tensor(weights[idx]['weights'][0]))
                m.bias = nn.Parameter(torch.Tensor(weights[idx]['weights'][1]))
            elif isinstance(m, nn.PReLU):
                idx = next(prelu_idxs)
                m.weight = nn.Parameter(torch.Tensor(weights[idx]['weights'][0]))
        self.invalidate_weights()

    def set_winograd(self, winograd3=None, amp_limit=None):
        """Arithmetic of the 3x3 convs of plans created from now on, as ``RtposeVGG.set_winograd``: None = library
        default ('auto'), False / 0 = direct, True / 1 / 2 = F(2x2,3x3), 4 = F(4x4,3x3) forced, 'auto' = per layer
        F(4x4,3x3) if its amplification estimate is <= ``amp_limit`` (default 256), else F(2x2,3x3)."""
        w3 = self._parse_winograd3(winograd3)
        self._wino = (w3, float(amp_limit or 0.0))
        return self

    def set_compute_dtype(self, dtype):
        if dtype != 'fp32':
            raise ValueError("OpenPose_Model runs in fp32 only (bf16 / bf16x3 plans exist for rtpose_vgg); got %r" % (dtype,))
        self.compute_dtype = dtype
        return self

    # ---- native side -------------------------------------------------------
    def _convs(self):
        """[(conv prefix, Conv2d, PReLU prefix or None, PReLU or None)] in the executor's index order (== state_dict)."""
        out = []
        fe = self.feature_extractor
        for i, m in enumerate(fe):
            if isinstance(m, nn.Conv2d):
                nxt = fe[i + 1]
                pr = isinstance(nxt, nn.PReLU)
                out.append(('feature_extractor.%d' % i, m, 'feature_extractor.%d' % (i + 1) if pr else None,
                            nxt if pr else None))
        for br in ('l2_stages', 'l1_stages'):
            for s, stage in enumerate(getattr(self, br)):
                pre = '%s.%d.' % (br, s)
                for attr, blk in stage.conv_blocks():
                    out.append((pre + attr + '.Mconv', blk.Mconv, pre + attr + '.MPrelu', blk.MPrelu))
                out.append((pre + 'Mconv7', stage.Mconv7, None, None))
        return out

    def _conv_record(self, entry):
        nm, m, pnm, pm = entry
        return ConvRecord(nm, m, None, (pnm, pm) if pm is not None else None, None)

    def _create(self, n, h, w, dtype, wino):
        handle = C.c_void_p()
        opts = _capi.OpenPoseOptions.make(*(self._topo + wino))
        check(lib.rtpose_openpose_create(n, h, w, C.byref(opts), C.byref(handle)), "rtpose_openpose_create")
        return handle

    def _out_channels(self, which):
        """saved_for_loss flattened: 0 .. l2_stages - 1 the PAF maps, then the heat maps"""
        l2, _, p, h = self._topo
        return p if which < l2 else h

    def forward(self, x):
        """reference :160-177 - ``[(paf[-2], heat[-2]), (paf[-1], heat[-1])], [paf_ret, heat_ret]``, NCHW fp32."""
        if not x.is_cuda:
            self.plan_for(x)  # raises: no CPU fallback
        l2, l1 = self._topo[0], self._topo[1]
        with torch.cuda.device(x.device):
            plan = self.forward_native(x, keep_intermediates=True)
            outs = [self.read_output(plan, i) for i in range(l2 + l1)]
        paf_ret, heat_ret = outs[:l2], outs[l2:]
        return [(paf_ret[-2], heat_ret[-2]), (paf_ret[-1], heat_ret[-1])], [paf_ret, heat_ret]


def use_vgg(model):  # reference :213-231 downloads ImageNet weights; no network here
    raise RuntimeError("use_vgg() needs network access to fetch vgg19-dcbb9e9d.pth; load a state_dict instead")
