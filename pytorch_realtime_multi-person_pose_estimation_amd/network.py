"""Host-side mirror of ``lib/network/rtpose_vgg.py`` (reference :60-225).

``get_model('vgg19')`` returns an ``nn.Module`` with the reference's 13
``nn.Sequential`` children (``model0``, ``model{1..6}_{1,2}``) so that the 184
state_dict keys, ``load_state_dict``, ``.cuda()``, ``.float()``, ``.eval()`` and
``nn.DataParallel`` wrapping (demo/picture_demo.py:45-49) keep working, but
``forward`` does not run those children: it hands the input to the native
executor in librtpose_mi355x.so (csrc/net.hip), whose convolutions are the
hand-written fp32-MFMA HIP kernels.  torch is used for device memory and
streams only.

The parameter containers are plain ``nn.Conv2d`` modules (weights OIHW as in the
reference checkpoints); they are re-packed into the kernel layout on the device
whenever a parameter's version counter changes.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _capi
from ._capi import lib, check
from ._native_state import ConvRecord, NativeStateMixin, NetPlanMixin

# (cin, cout, k) tables; 'P' = MaxPool2d(2, 2, 0).  reference :69-83, :95-127
_VGG = [(3, 64, 3), (64, 64, 3), 'P', (64, 128, 3), (128, 128, 3), 'P', (128, 256, 3),
        (256, 256, 3), (256, 256, 3), (256, 256, 3), 'P', (256, 512, 3), (512, 512, 3),
        (512, 256, 3), (256, 128, 3)]


def _stage1(nout):
    return [(128, 128, 3)] * 3 + [(128, 512, 1), (512, nout, 1)]


def _stage_t(nout):
    return [(185, 128, 7)] + [(128, 128, 7)] * 4 + [(128, 128, 1), (128, nout, 1)]


def _sequential(table, relu_after_last):
    mods = []
    for i, e in enumerate(table):
        if e == 'P':
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2, padding=0))
            continue
        cin, cout, k = e
        mods.append(nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=k // 2))
        if relu_after_last or i + 1 < len(table):
            mods.append(nn.ReLU(inplace=True))
    return nn.Sequential(*mods)


_DTYPES = {'fp32': _capi.DTYPE_F32, 'bf16': _capi.DTYPE_BF16, 'bf16x3': _capi.DTYPE_BF16X3}


class RtposeVGG(NativeStateMixin, NetPlanMixin, nn.Module):
    """Drop-in for the module built by reference ``get_model('vgg19')``."""

    _front_name = 'rtpose_vgg'
    _plan_stride = 8
    _probe_hw = 8
    _WINO_DEFAULT = (_capi.WINO_DEFAULT, _capi.WINO_DEFAULT, 0.0)   # (winograd3, winograd7, amp_limit)

    def __init__(self):
        super(RtposeVGG, self).__init__()
        # registration order == reference :141-155 (it fixes the state_dict order)
        self.model0 = _sequential(_VGG, True)
        for s in range(1, 7):
            setattr(self, 'model%d_1' % s, _sequential(_stage1(38) if s == 1 else _stage_t(38), False))
        for s in range(1, 7):
            setattr(self, 'model%d_2' % s, _sequential(_stage1(19) if s == 1 else _stage_t(19), False))
        self._initialize_weights_norm()
        self._init_native_state()   # plans / weight arenas per (device, dtype), see _native_state.py
        self.keep_intermediates = True   # reference forward returns all 12 stage outputs
        self.compute_dtype = 'fp32'
        self._wino = self._WINO_DEFAULT

    def set_winograd(self, winograd3=None, winograd7=None, amp_limit=None):
        """Arithmetic of the fp32 convs of plans created from now on (``rtpose_net_options``):
        ``winograd3``: None = library default ('auto' since round 4), False / 0 = direct kernels, True / 1 / 2 =
        F(2x2,3x3), 4 = F(4x4,3x3) forced, 'auto' = per layer F(4x4,3x3) if its amplification estimate is <=
        ``amp_limit``, else F(2x2,3x3);
        ``winograd7``: None = library default ('auto'), 0 = direct, 4 / 6 = F(4,7) / F(6,7) forced, 'auto' = per layer
        the fastest form whose amplification estimate for the loaded filters is <= ``amp_limit`` (default 256);
        8 = F(8,7) forced: opt-in only ('auto' never chooses it), 12.5 % fewer matrix multiplies than F(6,7) for ~8x
        its error bound; such plans keep a weight arena of their own (the standard one followed by the F(8,7) packings).
        All other forms read one weight arena; results of different forms differ by rounding only."""
        w3 = self._parse_winograd3(winograd3)
        if winograd7 is None:
            w7 = _capi.WINO_DEFAULT
        elif winograd7 == 'auto':
            w7 = _capi.WINO7_AUTO
        elif winograd7 in (0, 4, 6, 8):
            w7 = int(winograd7)
        else:
            raise ValueError("winograd7 must be None, 0, 4, 6, 8 or 'auto'")
        self._wino = (w3, w7, float(amp_limit or 0.0))
        return self

    def set_compute_dtype(self, dtype):
        """'fp32' (reference arithmetic, v_mfma_f32_32x32x2_f32), 'bf16' (BASELINE config 3:
        bf16 operands, fp32 accumulate, v_mfma_f32_32x32x16_bf16) or 'bf16x3' (every fp32
        operand split into two bf16s, three bf16 MFMAs per product: fp32-grade maps from the
        16x faster pipe).  Parameters, inputs and outputs stay fp32 tensors either way."""
        if dtype not in _DTYPES:
            raise ValueError("compute dtype must be one of %s" % (sorted(_DTYPES),))
        self.compute_dtype = dtype
        return self

    def _initialize_weights_norm(self):
        # reference :200-222: N(0, 0.01) weights, zero bias
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0.0)

    # ---- native side -------------------------------------------------------
    def _convs(self):
        """Conv modules in the native executor's index order (== state_dict order)."""
        out = []
        names = ['model0'] + ['model%d_1' % s for s in range(1, 7)] + ['model%d_2' % s for s in range(1, 7)]
        for nm in names:
            seq = getattr(self, nm)
            for idx, m in enumerate(seq):
                if isinstance(m, nn.Conv2d):
                    out.append(('%s.%d' % (nm, idx), m))
        return out

    def _conv_record(self, entry):
        return ConvRecord(entry[0], entry[1], None, None, None)

    def _create(self, n, h, w, dtype, wino):
        handle = C.c_void_p()
        opts = _capi.NetOptions.make(dtype, *wino)
        check(lib.rtpose_net_create_opts(n, h, w, C.byref(opts), C.byref(handle)), "rtpose_net_create_opts")
        return handle

    def _plan_options(self):
        return _DTYPES[self.compute_dtype], getattr(self, '_wino', self._WINO_DEFAULT)   # (unpickled from before _wino)

    def _arena(self, index, dtype, wino):
        """As every front - except the fp32 plans that force F(8,7): their arena is the standard layout followed by the
        F(8,7) packings of the 7x7 convs, it is kept apart and sized by a probe plan with the same option."""
        if dtype == _capi.DTYPE_F32 and wino[1] == 8:
            return (index, dtype, 'f87'), (_capi.WINO_DEFAULT, 8, 0.0)
        return (index, dtype), self._WINO_DEFAULT

    def _out_channels(self, which):
        return 38 if which % 2 == 0 else 19

    def forward(self, x):
        """reference :158-198 — returns ((out6_1, out6_2), saved_for_loss[12]), NCHW fp32."""
        if not x.is_cuda:
            self.plan_for(x)  # raises: no CPU fallback
        with torch.cuda.device(x.device):
            plan = self.forward_native(x, keep_intermediates=self.keep_intermediates)
            if self.keep_intermediates:
                saved = [self.read_output(plan, i) for i in range(12)]
            else:
                last = [self.read_output(plan, 10), self.read_output(plan, 11)]
                saved = [None] * 10 + last
        return (saved[10], saved[11]), saved


def get_model(trunk='vgg19'):
    """reference lib/network/rtpose_vgg.py:60.  Only the VGG19 trunk exists (the
    reference's 'mobilenet' branch never registers block0 and cannot run)."""
    if trunk != 'vgg19':
        raise ValueError("only trunk='vgg19' is implemented (reference 'mobilenet' branch is dead code)")
    return RtposeVGG()


def use_vgg(model):  # reference :235-251 downloads ImageNet weights; no network here
    raise RuntimeError("use_vgg() needs network access to fetch vgg19-dcbb9e9d.pth; load a state_dict instead")
