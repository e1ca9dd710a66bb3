"""Training through the library's kernels: ``loss.backward()`` and ``optimizer.step()`` of the reference's loops
(train/train_VGG19.py:194-217, train/train_SH.py:160-172, train/train_ShuffleNetV2.py:126-172) on an ``RtposeVGG``, an
``openpose.OpenPose_Model``, an ``hourglass.HourglassNet`` or a ``shufflenet.Network``.

PyTorch keeps the graph and the optimizer; every convolution of it, forward and backward, is hand-written HIP:

* ``conv2d(x, weight, bias, relu)`` is a ``torch.autograd.Function`` on NCHW fp32 device tensors.  Forward: the library's
  NCHW -> layout conversion, ``rtpose_conv2d`` (fp32 direct kernel, bias and ReLU fused as in inference), layout -> NCHW.
  Backward: ``rtpose_relu_grad`` through the fused ReLU, the data gradient as ``rtpose_conv2d`` on the flipped, transposed
  filter (``dgrad_weights``), the weight and bias gradients by ``rtpose_conv2d_wgrad``.  A conv whose parameters are
  frozen launches no weight gradient, a conv whose input needs no gradient (the first trainable conv behind a frozen trunk
  or behind the image) no data gradient.  With ``prelu=`` (the ``weight`` of an ``nn.PReLU(num_parameters=cout)``) the conv
  is launched without an activation into the pre-activation ``z``, ``rtpose_prelu`` makes ``y`` from it - the bits of the
  inference kernels' fused epilogue - and the backward runs ``rtpose_prelu_grad`` on the saved ``z`` (the slope gradient
  only if the slope requires one); ``y``'s layout buffer is not kept.  All launches go on the current stream; every buffer comes from torch's caching
  allocator.  The Winograd forms are not used here: their error contracts were set for the forward statistics.
* ``forward_train(model, x)`` is the reference's forward order over the module tree of an ``RtposeVGG``
  (lib/network/rtpose_vgg.py:158-198) or of an ``OpenPose_Model`` (lib/network/openpose.py:86-109, :160-177; the
  dense-block ``torch.cat``s stay in torch) with graph-carrying tensors; ``model.forward`` (the inference plan) is untouched.
* ``train_step`` is one iteration of the reference's loop, ``freeze_trunk`` its ``requires_grad = False`` preamble (:305-307).
  For an ``OpenPose_Model``, for which the reference ships no training script, the loss is ``encode.get_loss_openpose``.
* Packed filters are cached per parameter, one packing for the forward and one of the flipped, transposed filter for the
  data gradient, and re-packed under the contract ``_native_state.py`` states for the inference arenas: when the
  parameter's ``_version`` / ``data_ptr()`` changed (optimiser steps, ``copy_``, ``load_state_dict``, ``.to()``), when the
  model's weight epoch moved (``model.invalidate_weights()``, the way to announce edits through ``.data``, which bump no
  ``_version``), and on every forward and backward while ``model.always_resync`` is set.  ``forward_train`` and
  ``run_sequential`` hand both to ``conv2d`` (``epoch=``, ``resync=``); a bare ``conv2d`` caller that edits ``.data`` calls
  ``drop_packed_filters()``.
* PReLU slopes are neither packed nor cached: every ``rtpose_prelu`` / ``rtpose_prelu_grad`` launch reads the parameter's
  own storage, so a slope edited through ``.data`` needs no ``invalidate_weights()`` and the packed-filter cache is as it
  was.

* The stacked hourglass (training mode only): ``batch_norm(x, bn, relu)`` is training-mode ``nn.BatchNorm2d`` (+ ReLU) through
  ``rtpose_bn_stats`` / ``rtpose_bn_apply`` / ``rtpose_bn_grad`` (batch statistics in fp64, running statistics updated by the
  kernel); ``conv7x7_s2`` the 7x7 stride-2 stem, whose weight gradient is ``rtpose_conv2d_wgrad`` (k = 7) on the zero-stuffed
  output gradient; ``hourglass_forward(model, x, conv, bn, stem)`` the reference's forward order written once over three
  callables, which ``forward_train`` calls with the native operations (and the tests with torch's float64 ones).

* ShuffleNetV2 (training mode only): ``dwconv3x3(x, weight, stride)`` is the depthwise 3x3 conv of the blocks, forward
  ``rtpose_dwconv3x3``, backward ``rtpose_dwconv3x3_wgrad`` / ``rtpose_dwconv3x3_dgrad``; ``conv3x3_s2`` the 3 -> 24 stride-2
  stem, forward ``rtpose_stem_conv3x3_s2``, both gradients from the stride-1 kernels on the zero-stuffed output gradient;
  ``shufflenet_forward(model, x, conv, bn, dw, stem)`` the reference's forward order written once over four callables (the
  split, ``torch.cat``, the channel shuffle and the ceil-mode max-pool stay torch's); the pointwise convs and the heads are
  ``conv2d``, every BatchNorm ``batch_norm``.

* Mixed precision (``compute_dtype='bf16'`` of ``conv2d``, ``run_sequential``, ``forward_train`` and ``train_step``; RtposeVGG
  and OpenPose_Model): bf16 operands, fp32 accumulation, fp32 master weights, no loss scaling (bf16 has fp32's exponent
  range).  Tensors at the autograd boundary stay NCHW fp32 and parameters stay fp32.  Forward: ``rtpose_nchw_to_layout_bf16``
  (round to nearest even, channels padded to 16), the filters packed by ``rtpose_pack_conv_weights_bf16`` (cached as
  'fwd16' / 'bwd16' beside the fp32 packings), ``rtpose_conv2d_bf16(out_f32=1)`` with bias and ReLU fused; the bf16 input
  buffer is what is kept for the weight gradient.  Backward: ``rtpose_relu_grad`` / ``rtpose_prelu_grad`` in fp32 as above,
  ``rtpose_layout_f32_to_bf16`` of the masked gradient (its one rounding point), the data gradient as
  ``rtpose_conv2d_bf16(out_f32=1)`` on the bf16 packing of ``dgrad_weights``, the weight and bias gradients by
  ``rtpose_conv2d_wgrad_bf16``.  A shape ``rtpose_conv2d_bf16`` refuses (it refuses before launching) runs that direction of
  that conv on the fp32 path and is counted in ``bf16_fallbacks``.  The default ``'fp32'`` is the path above, launch for launch:
  one node, ``_Conv2d``, runs both, and tests/test_train_trace_gpu.py holds the launch sequence of either to a recorded one.

* Layout-resident dense stages (``dense_stage``; ``resident='dense'`` of ``forward_train`` and ``train_step``, OpenPose_Model
  with ``compute_dtype='bf16'`` only): a ``StageBlock`` is one autograd node.  Its conv launches are the per-conv bf16 path's
  (``out_f32 = 1``); between them ``rtpose_prelu_bf16`` writes the PReLU output as bf16 straight into the slice of the
  block's concat buffer the next convs read, and ``rtpose_prelu_grad_bf16`` makes a layer's bf16 output gradient from its
  kept fp32 pre-activation and the fp32 data gradients of its one or two consumers.  No NCHW tensor, ``torch.cat`` or fp32
  PReLU output exists inside a stage.  Opt-in.

* Layout-resident runs (``conv_chain``; ``resident=True`` of ``run_sequential``, ``forward_train`` and ``train_step``, RtposeVGG
  only): a run of convs with one consumer each is one autograd node; its inner activations and gradients stay in the gapped
  layout buffers (bf16 ones for ``compute_dtype='bf16'``: ``rtpose_conv2d_bf16(out_f32=0)`` forward and data gradient,
  ``rtpose_relu_grad_bf16`` in place), and NCHW fp32 exists only where the run begins and ends.  Opt-in; the default is the
  per-conv path, launch for launch.

* Layout-resident Bottlenecks (``preact_chain``; ``resident='bottleneck'`` of ``forward_train`` and ``train_step``, HourglassNet
  with ``compute_dtype='bf16'`` only): the BatchNorm -> ReLU -> conv triples of a pre-activation Bottleneck's main branch are
  one autograd node.  Its conv launches are the per-conv bf16 path's (``out_f32 = 1``); between them ``rtpose_bn_apply_bf16``
  writes relu(bn(.)) as bf16 straight into the gapped buffer the next conv reads and ``rtpose_bn_grad_bf16`` the bf16
  gradient the conv below reads.  No NCHW tensor and no fp32 BatchNorm output exists inside a run.  Opt-in.

* Layout-resident branches (``unit_chain``; ``resident='branch'`` of ``forward_train`` and ``train_step``, shufflenet.Network
  with ``compute_dtype='bf16'`` only): a run of conv -> BatchNorm (-> ReLU) units, the conv pointwise or depthwise 3x3, is one
  autograd node.  Its pointwise launches are the per-conv bf16 path's (``out_f32 = 1``), its depthwise ones
  ``rtpose_dwconv3x3_bf16_f32`` / ``_wgrad_bf16`` / ``_dgrad_bf16`` - bf16 activations, fp32 taps, fp32 outputs -; between them
  ``rtpose_bn_apply_bf16`` writes bn(.) (+ ReLU) as bf16 straight into the gapped buffer the next op reads and
  ``rtpose_bn_grad_bf16`` the bf16 gradient the op below reads.  ``dwconv3x3(compute_dtype='bf16')`` is the depthwise conv's
  own bf16 node.  No NCHW tensor and no fp32 BatchNorm output exists inside a run.  Opt-in.

On the default path the NCHW <-> layout conversion around every operation is known overhead.

A non-finite activation reaches the loss: the entry points called here carry NaN and Inf through their sums and their
fused ReLU is torch's (NaN stays NaN), in every mode - fp32, bf16 and layout-resident -, so a run that diverges prints a NaN
loss as the reference's loops do (header section 2, "Non-finite values"; tests/test_nonfinite_gpu.py).  ``model.forward``,
the inference plan, promises nothing of the kind.
"""
import ctypes as C
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi, encode
from ._capi import lib, check, ptr, current_stream
from .hourglass import HourglassNet
from .network import RtposeVGG
from .openpose import OpenPose_Model
from .shufflenet import Network as ShuffleNetV2


def dgrad_weights(weight):
    """The filter whose stride-1 "same" conv of gy is the gradient with respect to the input of conv(x, weight):
    taps flipped, in / out axes swapped.  [cout, cin, k, k] -> [cin, cout, k, k]."""
    return weight.flip(2, 3).transpose(0, 1).contiguous()


def _up8(c):
    return (c + 7) // 8 * 8


def _up16(c):
    return (c + 15) // 16 * 16


COMPUTE_DTYPES = ('fp32', 'bf16')
# convs of a compute_dtype='bf16' run whose forward / data gradient rtpose_conv2d_bf16 refused and the fp32 path ran instead
bf16_fallbacks = {'fwd': 0, 'dgrad': 0}


def reset_bf16_fallbacks():
    bf16_fallbacks['fwd'] = bf16_fallbacks['dgrad'] = 0


def _check_compute_dtype(who, compute_dtype):
    if compute_dtype not in COMPUTE_DTYPES:
        raise _capi.RtposeError("%s: compute_dtype is 'fp32' or 'bf16'; got %r" % (who, compute_dtype))


# ---- packed filters, per parameter (epoch, _version, data_ptr), as _native_state.py keys the forward arenas -----------------
_packed = {}   # id(weight) -> {'fwd': (key, w_packed, b_packed), 'bwd': (key, w_packed, b_packed)}; 'fwd16' / 'bwd16': in bf16


def drop_packed_filters(weight=None):
    """Forget the cached packings of `weight` (None: of every parameter): the next ``conv2d`` forward and backward pack
    from the values the parameters hold then.  For callers of ``conv2d`` that edit a parameter through ``.data``; a model
    run by ``forward_train`` announces such edits with ``model.invalidate_weights()`` instead."""
    if weight is None:
        _packed.clear()
    else:
        _packed.pop(id(weight), None)


def _pack(weight, bias, cin_p):
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    wp = torch.zeros(lib.rtpose_packed_weight_floats(cout, cin_p, k), dtype=torch.float32, device=weight.device)
    bp = torch.zeros(lib.rtpose_packed_bias_floats(cout), dtype=torch.float32, device=weight.device)
    check(lib.rtpose_pack_conv_weights(ptr(weight), ptr(bias), cout, cin, k, None, cin_p, ptr(wp), ptr(bp), current_stream()),
          "rtpose_pack_conv_weights")
    return wp, bp


def _pack_bf16(weight, bias, cin_p):
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    wp = torch.zeros(lib.rtpose_packed_weight_bytes_bf16(cout, cin_p, k) // 2, dtype=torch.bfloat16, device=weight.device)
    bp = torch.zeros(lib.rtpose_packed_bias_floats(cout), dtype=torch.float32, device=weight.device)
    check(lib.rtpose_pack_conv_weights_bf16(ptr(weight), ptr(bias), cout, cin, k, None, cin_p, ptr(wp), ptr(bp),
                                            current_stream()), "rtpose_pack_conv_weights_bf16")
    return wp, bp


def _packed_for(weight, bias, which, epoch=0, resync=False):
    """The packing of `weight` (+ `bias`) for the forward ('fwd') or of its flipped, transposed form for the data gradient
    ('bwd', zero bias) - 'fwd16' / 'bwd16': the same two rounded to bf16, input channels padded to 16 -, re-packed when `epoch` (the owning model's weight epoch) or the parameter's (_version, data_ptr)
    changed, and always if `resync`."""
    entry = _packed.get(id(weight))
    if entry is None or entry['ref']() is not weight:
        entry = _packed[id(weight)] = {'ref': weakref.ref(weight)}
        weakref.finalize(weight, _packed.pop, id(weight), None)
    key = (epoch, weight._version, weight.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if which in ('fwd', 'fwd16', 'stem') and bias is not None:
        key += (bias._version, bias.data_ptr())
    hit = entry.get(which)
    if hit is not None and hit[0] == key and not resync:
        return hit[1], hit[2]
    w = weight.detach()
    if which == 'stem':      # the 7x7 stride-2 stem's own packing, from the unfolded filter
        wp = torch.zeros(lib.rtpose_conv7x7_s2_packed_floats(), dtype=torch.float32, device=w.device)
        check(lib.rtpose_pack_conv7x7_s2(ptr(w.contiguous()), ptr(bias.detach().contiguous()) if bias is not None else None,
                                         ptr(wp), current_stream()), "rtpose_pack_conv7x7_s2")
        entry[which] = (key, wp, None)
        return wp, None
    pack, up = (_pack_bf16, _up16) if which in ('fwd16', 'bwd16') else (_pack, _up8)
    if which in ('fwd', 'fwd16'):
        b = bias.detach() if bias is not None else torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
        wp, bp = pack(w.contiguous(), b.contiguous(), up(w.shape[1]))
    else:
        wt = dgrad_weights(w)
        wp, bp = pack(wt, torch.zeros(wt.shape[0], dtype=torch.float32, device=w.device), up(wt.shape[1]))
    entry[which] = (key, wp, bp)
    return wp, bp


# ---- layout buffers ---------------------------------------------------------------------------------------------------------
def _buffer(lay, n, h, w, device, zero, bf16=False):
    """A buffer for n maps of h x w in the layout `lay`: fp32, zero-filled if `zero`, or bf16, which is always zero-filled"""
    numel = lib.rtpose_layout_pixels(C.byref(lay), n, h, w) * lay.cstride
    return (torch.zeros if zero or bf16 else torch.empty)(numel, dtype=torch.bfloat16 if bf16 else torch.float32, device=device)


def _to_layout(t, pad, bf16=False):
    """NCHW fp32 -> a zero-gapped layout buffer with the channels rounded up to 8 (the extra ones zero); `bf16`: a bf16
    buffer (round to nearest even) with the channels rounded up to 16"""
    n, c, h, w = t.shape
    lay = _capi.Layout.padded((_up16 if bf16 else _up8)(c), h, w, pad)
    buf = _buffer(lay, n, h, w, t.device, True, bf16)
    name = "rtpose_nchw_to_layout_bf16" if bf16 else "rtpose_nchw_to_layout"
    check(getattr(lib, name)(ptr(t), ptr(buf), C.byref(lay), c, lay.cstride, n, h, w, current_stream()), name)
    return buf, lay


def _from_layout(buf, lay, n, c, h, w):
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=buf.device)
    check(lib.rtpose_layout_to_nchw(ptr(buf), C.byref(lay), ptr(out), c, n, h, w, current_stream()), "rtpose_layout_to_nchw")
    return out


def _round_to_bf16(src, lsrc, c, n, h, w, pad=None, into=None):
    """rtpose_layout_f32_to_bf16 of the c channels of an fp32 layout buffer, into a new bf16 buffer with a zero gap of `pad`
    and the channels rounded up to 16, or into the slice `into` = (buffer, layout): (buffer, layout)"""
    if into is None:
        ldst = _capi.Layout.padded(_up16(c), h, w, pad)
        into = _buffer(ldst, n, h, w, src.device, True, True), ldst
    dst, ldst = into
    check(lib.rtpose_layout_f32_to_bf16(ptr(src), C.byref(lsrc), ptr(dst), C.byref(ldst), c, ldst.cstride, n, h, w,
                                        current_stream()), "rtpose_layout_f32_to_bf16")
    return dst, ldst


def _conv_launch(bf16, inp, lin, wp, bp, cin_p, cout, k, relu, n, h, w, out, lout, out_f32=0):
    """One conv of a layout buffer into the slice out / lout - the one place a ConvDesc is filled: rtpose_conv2d, or
    rtpose_conv2d_bf16 writing bf16 (out_f32 = 0) or fp32.  True, or False if the bf16 launcher refused the shape
    (RTPOSE_E_INVAL: returned before any launch)."""
    d = _capi.ConvDesc()
    d.inp, d.w_packed, d.bias_packed, d.out = inp.data_ptr(), wp.data_ptr(), bp.data_ptr(), out.data_ptr()
    d.lin, d.lout = lin, lout
    d.cin, d.cout, d.k, d.relu = cin_p, cout, k, 1 if relu else 0
    if not bf16:
        check(lib.rtpose_conv2d(C.byref(d), 1, n, h, w, current_stream()), "rtpose_conv2d")
        return True
    rc = lib.rtpose_conv2d_bf16(C.byref(d), 1, n, h, w, 1 if out_f32 else 0, current_stream())
    if rc == -1:
        return False
    check(rc, "rtpose_conv2d_bf16")
    return True


# the name _ConvChain launches through, and nothing else does: replacing it plays a refusal of a chain's own launches and
# leaves alone the conv2d nodes the chain falls back to (tests/test_train_resident_gpu.py)
_conv_into = _conv_launch


def _launch_conv(bf16, inp, lin, wp, bp, cin_p, cout, k, relu, n, h, w):
    """_conv_launch into a new dense fp32 buffer: (buffer, layout), or None if the bf16 launcher refused the shape"""
    lout = _capi.Layout.dense(_up8(cout), h, w)
    out = _buffer(lout, n, h, w, inp.device, False)
    return (out, lout) if _conv_launch(bf16, inp, lin, wp, bp, cin_p, cout, k, relu, n, h, w, out, lout, 1) else None


def _dgrad_fp32_fallback(g, lg, wt, n, h, w, epoch, resync):
    """the data gradient of one conv whose bf16 launch was refused: the bf16 gradient g widened
    (rtpose_layout_bf16_to_f32) and convolved in fp32 on the flipped, transposed filter of `wt` into a new dense fp32
    buffer, (buffer, layout); counted in ``bf16_fallbacks['dgrad']``"""
    cout, cin, k = wt.shape[0], wt.shape[1], wt.shape[2]
    bf16_fallbacks['dgrad'] += 1
    l32 = _capi.Layout.padded(_up8(cout), h, w, k // 2)
    g32 = _buffer(l32, n, h, w, g.device, True)
    check(lib.rtpose_layout_bf16_to_f32(ptr(g), C.byref(lg), ptr(g32), C.byref(l32), cout, n, h, w, current_stream()),
          "rtpose_layout_bf16_to_f32")
    wp, bp = _packed_for(wt, None, 'bwd', epoch, resync)
    return _launch_conv(False, g32, l32, wp, bp, l32.cstride, cin, k, False, n, h, w)


def _wgrad(bf16, xbuf, lx, gbuf, lg, like_weight, cin, cout, k, n, h, w, need_b):
    """rtpose_conv2d_wgrad - `bf16`: rtpose_conv2d_wgrad_bf16 - of the layout buffers of x and of the output gradient (an
    h x w map, gaps of k // 2; both fp32 or both bf16): (dw shaped like `like_weight`, db or None), fp32"""
    name = "rtpose_conv2d_wgrad_bf16" if bf16 else "rtpose_conv2d_wgrad"
    dw = torch.empty_like(like_weight, memory_format=torch.contiguous_format)
    db = torch.empty(cout, dtype=torch.float32, device=gbuf.device) if need_b else None
    floats = getattr(lib, name + "_workspace_floats")(cin, cout, k, n, h, w)
    ws = torch.empty(floats, dtype=torch.float32, device=gbuf.device)
    d = (_capi.WgradBf16Desc if bf16 else _capi.WgradDesc)()
    d.x, d.gy, d.dw, d.dbias = xbuf.data_ptr(), gbuf.data_ptr(), dw.data_ptr(), db.data_ptr() if need_b else None
    d.workspace, d.workspace_floats = ws.data_ptr(), floats
    d.lx, d.lgy = lx, lg
    d.cin, d.cout, d.k = cin, cout, k
    check(getattr(lib, name)(C.byref(d), n, h, w, current_stream()), name)
    return dw, db


def _relu_grad(bf16, ybuf, ly, gbuf, lg, c, n, h, w):
    """g = y > 0 ? g : 0 in place on the gradient's layout buffer: rtpose_relu_grad, or rtpose_relu_grad_bf16 on bf16 buffers"""
    name = "rtpose_relu_grad_bf16" if bf16 else "rtpose_relu_grad"
    check(getattr(lib, name)(ptr(ybuf), C.byref(ly), ptr(gbuf), C.byref(lg), ptr(gbuf), C.byref(lg), c, n, h, w,
                             current_stream()), name)


def _prelu(zbuf, lz, slopes, c, n, h, w):
    """rtpose_prelu of the pre-activation's layout buffer into a new one of the same layout"""
    ybuf = _buffer(lz, n, h, w, zbuf.device, False)
    check(lib.rtpose_prelu(ptr(zbuf), C.byref(lz), ptr(slopes.detach().contiguous()), ptr(ybuf), C.byref(lz), c, n, h, w,
                           current_stream()), "rtpose_prelu")
    return ybuf


def _prelu_grad(zbuf, lz, slopes, gbuf, lg, c, n, h, w, need_a):
    """rtpose_prelu_grad in place on the gradient's layout buffer; the slope gradient, or None unless `need_a`"""
    floats = lib.rtpose_prelu_grad_workspace_floats(c, n, h, w) if need_a else 0
    ws = torch.empty(floats, dtype=torch.float32, device=gbuf.device) if need_a else None
    da = torch.empty(c, dtype=torch.float32, device=gbuf.device) if need_a else None
    check(lib.rtpose_prelu_grad(ptr(zbuf), C.byref(lz), ptr(slopes.detach().contiguous()), ptr(gbuf), C.byref(lg), ptr(gbuf),
                                C.byref(lg), ptr(da), ptr(ws), floats, c, n, h, w, current_stream()), "rtpose_prelu_grad")
    return da


def _zero_stuffed_layout(gy, h, w, pad):
    """The output gradient of a stride-2 conv as the h x w map gyz[n, :, 2 y, 2 x] = gy[n, :, y, x], zero elsewhere, in a
    layout with a gap of `pad`: the stride-1 kernels on it give the stride-2 gradients exactly (the zeros add nothing)."""
    gyz = torch.zeros((gy.shape[0], gy.shape[1], h, w), dtype=torch.float32, device=gy.device)
    gyz[:, :, ::2, ::2] = gy.detach().float()
    return _to_layout(gyz, pad)


def _require_device(who, *tensors, names=("x", "weight")):
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise _capi.RtposeError("%s runs only on an MI355X (HIP) device; got %s - there is deliberately no CPU fallback"
                                % (who, ", ".join("%s on %s" % (nm, getattr(t, 'device', None))
                                                  for nm, t in zip(names, tensors))))


def _check_prelu(prelu, weight, relu):
    if relu:
        raise _capi.RtposeError("train.conv2d: relu and prelu are exclusive")
    if not torch.is_tensor(prelu) or prelu.dtype != torch.float32 or tuple(prelu.shape) != (weight.shape[0],):
        raise _capi.RtposeError("train.conv2d: prelu is the fp32 [cout] weight of an nn.PReLU(num_parameters=cout), cout = %d; "
                                "got %s" % (weight.shape[0], "%s %s" % (prelu.dtype, tuple(prelu.shape))
                                            if torch.is_tensor(prelu) else type(prelu).__name__))
    if prelu.device != weight.device:
        raise _capi.RtposeError("train.conv2d: prelu on %s, the filters on %s" % (prelu.device, weight.device))


def _is_same_conv_filter(weight, cin):
    """an fp32 OIHW filter of a stride-1 "same" conv on `cin` channels that the kernels here run: square, k in {1, 3, 7}"""
    return (weight.dtype == torch.float32 and weight.dim() == 4 and weight.shape[3] == weight.shape[2]
            and weight.shape[2] in (1, 3, 7) and weight.shape[1] == cin)


def _check_input(x, weight):
    _require_device("train.conv2d", x, weight)
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 4 or weight.dim() != 4:
        raise _capi.RtposeError("train.conv2d takes NCHW fp32 inputs and OIHW fp32 filters")
    if not _is_same_conv_filter(weight, x.shape[1]):
        raise _capi.RtposeError("train.conv2d: stride-1 'same' convs with k in {1, 3, 7}; got filters %s for input %s"
                                % (tuple(weight.shape), tuple(x.shape)))


class _Conv2d(torch.autograd.Function):
    """conv2d's node.  Inputs: x, weight, bias (or None), relu, epoch, resync, the PReLU slopes (or None), bf16.  With `bf16`
    the operands of all three convs are bf16: what is rounded, and where, is in the module docstring.  Everything fp32 - the
    activation gradients, the buffers y / z they read, the outputs of all three convs - is the same in both."""
    @staticmethod
    def forward(ctx, x, weight, bias, relu, epoch, resync, prelu, bf16):
        if prelu is not None:
            _check_prelu(prelu, weight, relu)
        _check_input(x, weight)
        with torch.cuda.device(x.device):
            n, cin, h, w = x.shape
            cout, k = weight.shape[0], weight.shape[2]
            xc = x.detach().contiguous()
            xbuf, lx = _to_layout(xc, k // 2, bf16)
            wp, bp = _packed_for(weight, bias, 'fwd16' if bf16 else 'fwd', epoch, resync)
            done = _launch_conv(bf16, xbuf, lx, wp, bp, lx.cstride, cout, k, relu, n, h, w)
            if done is None:             # refused before any launch: this direction of this conv in fp32
                bf16_fallbacks['fwd'] += 1
                xbuf32, lx32 = _to_layout(xc, k // 2)
                wp, bp = _packed_for(weight, bias, 'fwd', epoch, resync)
                done = _launch_conv(False, xbuf32, lx32, wp, bp, lx32.cstride, cout, k, relu, n, h, w)
            ybuf, ly = done
            zbuf = None
            if prelu is not None:        # ybuf so far holds the pre-activation: keep it as z, y goes to a buffer of its own
                zbuf, ybuf = ybuf, _prelu(ybuf, ly, prelu, cout, n, h, w)
            y = _from_layout(ybuf, ly, n, cout, h, w)
        ctx.geom = (n, cin, cout, k, h, w)
        ctx.relu, ctx.bf16 = bool(relu), bf16
        ctx.has_bias = bias is not None
        ctx.weight = weight
        ctx.epoch, ctx.resync = epoch, resync
        ctx.has_prelu = prelu is not None
        # (for autograd's check that the filters and slopes were not modified in place since)
        ctx.save_for_backward(*((weight, prelu) if ctx.has_prelu else (weight,)))
        wants_w = ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2])
        ctx.xbuf, ctx.lx = (xbuf, lx) if wants_w else (None, None)      # with bf16 the bf16 buffer, also after a fallback
        ctx.ybuf, ctx.ly = (ybuf, ly) if relu and any(ctx.needs_input_grad) else (None, None)
        ctx.zbuf, ctx.lz = (zbuf, ly) if ctx.has_prelu and any(ctx.needs_input_grad) else (None, None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        saved = ctx.saved_tensors
        n, cin, cout, k, h, w = ctx.geom
        bf16 = ctx.bf16
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        need_a = ctx.has_prelu and ctx.needs_input_grad[6]
        dx = dw = db = da = None
        with torch.cuda.device(gy.device):
            gbuf, lg = _to_layout(gy.detach().float().contiguous(), k // 2)
            if ctx.relu:
                _relu_grad(False, ctx.ybuf, ctx.ly, gbuf, lg, cout, n, h, w)
            if ctx.has_prelu:
                da = _prelu_grad(ctx.zbuf, ctx.lz, saved[1], gbuf, lg, cout, n, h, w, need_a)
            g, lgr = gbuf, lg            # what the two gradients below read
            if bf16 and (need_x or need_w or need_b):
                # the one rounding point of the output gradient: both gradients below read these bf16 values
                g, lgr = _round_to_bf16(gbuf, lg, cout, n, h, w, k // 2)
            if need_x:
                wp, bp = _packed_for(ctx.weight, None, 'bwd16' if bf16 else 'bwd', ctx.epoch, ctx.resync)
                done = _launch_conv(bf16, g, lgr, wp, bp, lgr.cstride, cin, k, False, n, h, w)
                if done is None:         # refused: on the fp32 masked gradient
                    bf16_fallbacks['dgrad'] += 1
                    wp, bp = _packed_for(ctx.weight, None, 'bwd', ctx.epoch, ctx.resync)
                    done = _launch_conv(False, gbuf, lg, wp, bp, lg.cstride, cin, k, False, n, h, w)
                dx = _from_layout(done[0], done[1], n, cin, h, w)
            if need_w or need_b:
                dw, db = _wgrad(bf16, ctx.xbuf, ctx.lx, g, lgr, ctx.weight, cin, cout, k, n, h, w, need_b)
                if not need_w:
                    dw = None
        return dx, dw, db, None, None, None, da, None


def conv2d(x, weight, bias=None, relu=False, epoch=0, resync=False, prelu=None, compute_dtype='fp32'):
    """``relu(conv2d(x, weight, bias, padding=k // 2))`` (ReLU only if `relu`) with the library's kernels in both directions;
    NCHW fp32 device tensors, k in {1, 3, 7}.  `epoch` (an int) is part of what the cached packings of `weight` are keyed
    by, `resync` packs anew in this forward and its backward: the owning model's weight epoch and ``always_resync``.
    `prelu`: an fp32 [cout] device tensor, the ``weight`` of an ``nn.PReLU(num_parameters=cout)`` applied to the conv's
    output (exclusive with `relu`); read from its storage by every launch, never packed or cached.
    `compute_dtype`: 'fp32', or 'bf16' for bf16 operands of all three convs with fp32 accumulation (module docstring);
    inputs, outputs, gradients and parameters are fp32 either way."""
    _check_compute_dtype("train.conv2d", compute_dtype)
    return _Conv2d.apply(x, weight, bias, bool(relu), int(epoch), bool(resync), prelu, compute_dtype == 'bf16')


# ---- a run of convs as one autograd node: the inner activations and gradients stay in the layouts ---------------------------------
# chains of a compute_dtype='bf16' run that gave up residency because rtpose_conv2d_bf16 refused one of their forward convs
chain_fallbacks = 0


def reset_chain_fallbacks():
    global chain_fallbacks
    chain_fallbacks = 0


class _ChainRefused(Exception):
    """rtpose_conv2d_bf16 refused a forward conv of a chain (before any launch of that conv)"""


def _chain_buffer(bf16, c, k_next, n, h, w, device):
    """Where a conv of a chain writes its c channels: a zero-initialised buffer gapped for the conv of size `k_next` that reads
    it next, the channels padded as that conv reads them (16 for bf16, 8 for fp32; the conv writes c channels only, so the
    pad channels stay zero) - or, for `k_next` None, where the chain ends: a dense fp32 one.  (buffer, layout)"""
    if k_next is None:
        lay = _capi.Layout.dense(_up8(c), h, w)
        return _buffer(lay, n, h, w, device, False), lay
    lay = _capi.Layout.padded((_up16 if bf16 else _up8)(c), h, w, k_next // 2)
    return _buffer(lay, n, h, w, device, True, bf16), lay


def _check_chain(x, layers):
    if len(layers) < 1:
        raise _capi.RtposeError("train.conv_chain: no layers")
    c = x.shape[1] if torch.is_tensor(x) and x.dim() == 4 else None
    for i, layer in enumerate(layers):
        if not isinstance(layer, (tuple, list)) or len(layer) != 3 or not torch.is_tensor(layer[0]):
            raise _capi.RtposeError("train.conv_chain: layers are (weight, bias_or_None, relu) triples; got %r at %d"
                                    % (type(layer).__name__, i))
        weight, bias, _ = layer
        if i == 0:
            _check_input(x, weight)
        _require_device("train.conv_chain", weight, names=("a weight",))
        if not _is_same_conv_filter(weight, c):
            raise _capi.RtposeError("train.conv_chain: layer %d: stride-1 'same' convs with fp32 OIHW filters, k in {1, 3, 7}, "
                                    "whose input channels are the output channels of the layer before (%s); got filters %s %s"
                                    % (i, c, weight.dtype, tuple(weight.shape)))
        if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (weight.shape[0],)
                                 or bias.device != weight.device):
            raise _capi.RtposeError("train.conv_chain: layer %d: the bias is None or an fp32 [%d] tensor beside the filters"
                                    % (i, weight.shape[0]))
        c = weight.shape[0]


class _ConvChain(torch.autograd.Function):
    """conv_chain's node.  Inputs: x, (relus, epoch, resync, bf16), then weight and bias (or None) of every layer."""
    @staticmethod
    def forward(ctx, x, meta, *params):
        relus, epoch, resync, bf16 = meta
        weights, biases = params[0::2], params[1::2]
        L = len(weights)
        fwd = 'fwd16' if bf16 else 'fwd'
        with torch.cuda.device(x.device):
            n, _, h, w = x.shape
            ks = [wt.shape[2] for wt in weights]
            couts = [wt.shape[0] for wt in weights]
            buf, lay = _to_layout(x.detach().contiguous(), ks[0] // 2, bf16)
            bufs, lays = [buf], [lay]
            for i in range(L):
                wp, bp = _packed_for(weights[i], biases[i], fwd, epoch, resync)
                out, lout = _chain_buffer(bf16, couts[i], ks[i + 1] if i + 1 < L else None, n, h, w, x.device)
                if not _conv_into(bf16, bufs[i], lays[i], wp, bp, lays[i].cstride, couts[i], ks[i], relus[i], n, h, w, out, lout,
                                  out_f32=i + 1 == L):
                    raise _ChainRefused()
                bufs.append(out)
                lays.append(lout)
            y = _from_layout(bufs[L], lays[L], n, couts[L - 1], h, w)
        need_x = ctx.needs_input_grad[0]
        wants = [ctx.needs_input_grad[2 + 2 * i] or (biases[i] is not None and ctx.needs_input_grad[3 + 2 * i]) for i in range(L)]
        # the lowest layer whose backward anything needs: the walk stops there
        low = 0 if need_x else next((i for i in range(L) if wants[i]), L)
        ctx.geom = (n, h, w)
        ctx.meta = meta
        ctx.weights = weights
        ctx.has_bias = [b is not None for b in biases]
        ctx.low, ctx.wants = low, wants
        ctx.save_for_backward(*weights)   # (for autograd's check that the filters were not modified in place since)
        # per layer only the input buffer, where the weight gradient or the mask of the layer below reads it; of the last
        # layer's fp32 output only what a ReLU behind it needs
        keep = [low < L and (wants[i] or (i > low and relus[i - 1])) for i in range(L)] + [low < L and relus[L - 1]]
        ctx.bufs = [b if kp else None for b, kp in zip(bufs, keep)]
        ctx.lays = lays
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        relus, epoch, resync, bf16 = ctx.meta
        ctx.saved_tensors
        weights, bufs, lays, low, wants = ctx.weights, ctx.bufs, ctx.lays, ctx.low, ctx.wants
        L = len(weights)
        n, h, w = ctx.geom
        need_x = ctx.needs_input_grad[0]
        bwd = 'bwd16' if bf16 else 'bwd'
        grads = [None] * (2 * L)
        dx = None
        if low >= L:
            return (None, None) + tuple(grads)
        with torch.cuda.device(gy.device):
            dev = gy.device
            gyc = gy.detach().float().contiguous()
            k, cout = weights[L - 1].shape[2], weights[L - 1].shape[0]
            if relus[L - 1] or not bf16:
                g, lg = _to_layout(gyc, k // 2)
                if relus[L - 1]:     # a ReLU behind the last conv: masked by the fp32 output, as conv2d does
                    _relu_grad(False, bufs[L], lays[L], g, lg, cout, n, h, w)
                if bf16:
                    g, lg = _round_to_bf16(g, lg, cout, n, h, w, k // 2)
            else:
                g, lg = _to_layout(gyc, k // 2, True)
            for i in range(L - 1, low - 1, -1):
                wt = weights[i]
                cout, cin, k = wt.shape[0], wt.shape[1], wt.shape[2]
                if wants[i]:
                    need_b = ctx.has_bias[i] and ctx.needs_input_grad[3 + 2 * i]
                    dw, db = _wgrad(bf16, bufs[i], lays[i], g, lg, wt, cin, cout, k, n, h, w, need_b)
                    grads[2 * i] = dw if ctx.needs_input_grad[2 + 2 * i] else None
                    grads[2 * i + 1] = db
                if i == low and not (i == 0 and need_x):
                    break
                # the data gradient: the conv of g on the flipped, transposed filter, straight into the buffer the layer
                # below reads its output gradient from (gapped for that layer), or into a dense fp32 one for dx
                wp, bp = _packed_for(wt, None, bwd, epoch, resync)
                d, ld = _chain_buffer(bf16, cin, weights[i - 1].shape[2] if i > 0 else None, n, h, w, dev)
                if not _conv_into(bf16, g, lg, wp, bp, lg.cstride, cin, k, False, n, h, w, d, ld, out_f32=i == 0):
                    # refused: this one conv in fp32 on the widened gradient, rounded again at its store inside the chain
                    d32, ld32 = _dgrad_fp32_fallback(g, lg, wt, n, h, w, epoch, resync)
                    d, ld = _round_to_bf16(d32, ld32, cin, n, h, w, into=(d, ld)) if i > 0 else (d32, ld32)
                if i == 0:
                    dx = _from_layout(d, ld, n, cin, h, w)
                    break
                if relus[i - 1]:     # in place, by the layer below's output as stored: this layer's kept input buffer
                    _relu_grad(bf16, bufs[i], lays[i], d, ld, cin, n, h, w)
                g, lg = d, ld
        return (dx, None) + tuple(grads)


def conv_chain(x, layers, epoch=0, resync=False, compute_dtype='fp32'):
    """A run of stride-1 "same" convs, each read by the next alone, as ONE autograd node whose inner activations and
    gradients never leave the library's layouts.  `layers`: a sequence of (weight, bias_or_None, relu), k in {1, 3, 7},
    every layer's input channels the output channels of the one before; `x` NCHW fp32 on the device; the result is the last
    conv's output (after its ReLU, if it has one), NCHW fp32.  `epoch` / `resync` / `compute_dtype`: see ``conv2d``; the
    packings are the same cached ones.

    Forward: x is converted once into a buffer gapped for layer 0; every inner conv writes into a zero-initialised buffer
    gapped by the next layer's k // 2 with the channels padded as that layer reads them (16 for bf16, 8 for fp32; the
    conv writes its cout channels only, so the pad channels stay zero) - ``rtpose_conv2d_bf16(out_f32 = 0)`` or
    ``rtpose_conv2d``; the last conv writes fp32 into a dense buffer, and one ``rtpose_layout_to_nchw`` leaves.
    Backward: gy is converted once (``rtpose_nchw_to_layout_bf16`` / ``rtpose_nchw_to_layout``); then, from the last layer
    down to the lowest one anything still needs: the weight and bias gradients from the kept input buffer and the current
    gradient buffer (if that layer's parameters want them), the data gradient as the conv on the cached 'bwd16' / 'bwd'
    packing straight into a buffer gapped for the layer below (``out_f32 = 0``), masked in place by that layer's ReLU with
    ``rtpose_relu_grad_bf16`` / ``rtpose_relu_grad`` against the kept input buffer of the current layer - the layer below's
    output as stored.  The first layer's data gradient leaves as fp32 NCHW, only if x needs one.  Per layer only the input
    buffer is kept; no fp32 copy of an inner y and no NCHW intermediate exists.  A ReLU behind the LAST conv is masked as
    ``conv2d`` masks it, by the kept fp32 output, before the gradient's one rounding.

    The rounding points are ``conv2d(compute_dtype='bf16')``'s: an activation rounded at the conv's store is what the next
    conv's input conversion produced, a data gradient rounded at the store and then masked is the masked fp32 gradient
    rounded.  Two differences remain: the mask is taken from y rounded to bf16, so an activation 0 < y <= 2^-134 (which bf16
    rounds to +0) masks its gradient here and not there; and ``out_f32 = 0`` may reach another kernel instance (the
    64-input-channel 3x3 kernel takes only such launches) whose fp32 sums run in another order.  On exact integer operands
    the two forms are equal bit for bit.

    A forward conv ``rtpose_conv2d_bf16`` refuses (before launching) makes the chain give up residency: it runs layer by layer
    through ``conv2d`` (whose own fallback counters apply) and ``chain_fallbacks`` counts it.  A refused data gradient runs
    that one conv in fp32 on the widened gradient (``rtpose_layout_bf16_to_f32``) and is counted in
    ``bf16_fallbacks['dgrad']``; inside the chain its result is rounded to bf16 at the store like every other, and its
    operand is the gradient already rounded - so its bits differ from the per-conv fallback's, which convolves the fp32
    masked gradient."""
    global chain_fallbacks
    _check_compute_dtype("train.conv_chain", compute_dtype)
    layers = [tuple(layer) if isinstance(layer, (tuple, list)) else layer for layer in layers]
    _check_chain(x, layers)
    meta = (tuple(bool(r) for _, _, r in layers), int(epoch), bool(resync), compute_dtype == 'bf16')
    try:
        return _ConvChain.apply(x, meta, *[p for wt, b, _ in layers for p in (wt, b)])
    except _ChainRefused:
        chain_fallbacks += 1
    for wt, b, relu in layers:
        x = conv2d(x, wt, b, relu, epoch, resync, None, compute_dtype)
    return x


# ---- a StageBlock of an OpenPose_Model as one autograd node: dense blocks and PReLU inside the layouts (bf16) ---------------------
# stages of a resident='dense' run that gave up residency: a width that is no multiple of 16, or a forward conv that
# rtpose_conv2d_bf16 refused
dense_fallbacks = 0


def reset_dense_fallbacks():
    global dense_fallbacks
    dense_fallbacks = 0


class _DenseRefused(Exception):
    """rtpose_conv2d_bf16 refused a forward conv of a dense stage (before any launch of that conv)"""


# the name _DenseStage launches its convs through, and nothing else does: replacing it plays a refusal of the node's own
# launches and leaves alone the conv2d nodes the stage falls back to (tests/test_train_dense_gpu.py)
_dense_conv_into = _conv_launch


def _prelu_bf16(zbuf, lz, slope, ybuf, ly, c, n, h, w):
    """rtpose_prelu_bf16 of the fp32 pre-activation into the bf16 slice ybuf / ly"""
    check(lib.rtpose_prelu_bf16(ptr(zbuf), C.byref(lz), ptr(slope.detach().contiguous()), ptr(ybuf), C.byref(ly), c, n, h, w,
                                current_stream()), "rtpose_prelu_bf16")


def _prelu_grad_bf16(zbuf, lz, slope, ga, lga, gb, lgb, out, lout, c, n, h, w, need_a):
    """rtpose_prelu_grad_bf16 of the fp32 gradient slice ga (+ gb, or None) into the bf16 slice out / lout; the slope
    gradient, or None unless `need_a`"""
    floats = lib.rtpose_prelu_grad_bf16_workspace_floats(c, n, h, w) if need_a else 0
    ws = torch.empty(floats, dtype=torch.float32, device=out.device) if need_a else None
    da = torch.empty(c, dtype=torch.float32, device=out.device) if need_a else None
    check(lib.rtpose_prelu_grad_bf16(ptr(zbuf), C.byref(lz), ptr(slope.detach().contiguous()), ptr(ga), C.byref(lga), ptr(gb),
                                     C.byref(lgb) if gb is not None else None, ptr(out), C.byref(lout), ptr(da), ptr(ws),
                                     floats, c, n, h, w, current_stream()), "rtpose_prelu_grad_bf16")
    return da


def _check_dense(x, layers):
    who = "train.dense_stage"
    _require_device(who, x, names=("x",))
    if x.dtype != torch.float32 or x.dim() != 4:
        raise _capi.RtposeError("%s takes an NCHW fp32 input; got %s %s" % (who, x.dtype, tuple(x.shape)))
    L = len(layers)
    if L < 5 or (L - 2) % 3:
        raise _capi.RtposeError("%s: layers are 3 B + 2 (weight, bias_or_None, slope_or_None) triples, B >= 1 dense blocks of "
                                "three 3x3 convs, then the 1x1 convs Mconv6 and Mconv7; got %d" % (who, L))
    for i, layer in enumerate(layers):
        if not isinstance(layer, tuple) or len(layer) != 3 or not torch.is_tensor(layer[0]):
            raise _capi.RtposeError("%s: layers are (weight, bias_or_None, slope_or_None) triples; got %r at %d"
                                    % (who, type(layer).__name__, i))
        _require_device(who, layer[0], names=("the filters of layer %d" % i,))
    def rows(t):
        return t.shape[0] if t.dim() else 0

    width = rows(layers[0][0])
    for i, (weight, bias, slope) in enumerate(layers):
        block, j = divmod(i, 3)
        k = 3 if i < L - 2 else 1
        cin = (width if j else (x.shape[1] if block == 0 else 3 * width)) if i < L - 2 else \
            (3 * width if i == L - 2 else rows(layers[L - 2][0]))
        if (weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[1:]) != (cin, k, k)
                or (i < L - 2 and weight.shape[0] != width)):
            raise _capi.RtposeError("%s: layer %d: fp32 OIHW filters [%s, %d, %d, %d] (a dense block is three 3x3 convs of "
                                    "layer 0's width %d, the first on the stage input or on the 3 x %d channels of the block "
                                    "before; Mconv6 and Mconv7 are 1x1); got %s %s"
                                    % (who, i, width if i < L - 2 else "cout", cin, k, k, width, width, weight.dtype,
                                       tuple(weight.shape)))
        cout = weight.shape[0]
        if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (cout,)
                                 or bias.device != weight.device):
            raise _capi.RtposeError("%s: layer %d: the bias is None or an fp32 [%d] tensor beside the filters" % (who, i, cout))
        if i == L - 1:
            if slope is not None:
                raise _capi.RtposeError("%s: layer %d (Mconv7) has no activation: its slope must be None" % (who, i))
        elif slope is None:
            raise _capi.RtposeError("%s: layer %d has a PReLU: its slope is missing" % (who, i))
        elif (not torch.is_tensor(slope) or slope.dtype != torch.float32 or tuple(slope.shape) != (cout,)
              or slope.device != weight.device):
            raise _capi.RtposeError("%s: layer %d: the slope is the fp32 [%d] weight of an nn.PReLU(num_parameters=%d) on the "
                                    "filters' device %s; got %s"
                                    % (who, i, cout, cout, weight.device,
                                       "%s %s on %s" % (slope.dtype, tuple(slope.shape), slope.device)
                                       if torch.is_tensor(slope) else type(slope).__name__))


class _DenseStage(torch.autograd.Function):
    """dense_stage's node.  Inputs: x, (epoch, resync), then weight, bias (or None) and slope (None for the last) of every
    layer.  Layer i < 3 B is conv (b, j) = divmod(i, 3) of the dense blocks, 3 B is Mconv6, 3 B + 1 is Mconv7."""
    @staticmethod
    def forward(ctx, x, meta, *params):
        epoch, resync = meta
        weights, biases, slopes = params[0::3], params[1::3], params[2::3]
        L = len(weights)
        B = (L - 2) // 3
        width, c6, cout = weights[0].shape[0], weights[L - 2].shape[0], weights[L - 1].shape[0]
        with torch.cuda.device(x.device):
            n, cin, h, w = x.shape
            dev = x.device
            xbuf, lx = _to_layout(x.detach().contiguous(), 1, True)
            lz = _capi.Layout.dense(width, h, w)
            lcat = _capi.Layout.padded(3 * width, h, w, 1)              # a block's concat buffer, whole
            lsl = [_capi.Layout.padded(3 * width, h, w, 1, j * width) for j in range(3)]     # and its three slices
            ybufs, zbufs = [], []
            src, lsrc, csrc = xbuf, lx, lx.cstride
            for b in range(B):
                ycat = _buffer(lcat, n, h, w, dev, True, True)
                for j in range(3):
                    i = 3 * b + j
                    wp, bp = _packed_for(weights[i], biases[i], 'fwd16', epoch, resync)
                    z = _buffer(lz, n, h, w, dev, False)
                    inp, lin, cin_p = (src, lsrc, csrc) if j == 0 else (ycat, lsl[j - 1], width)
                    if not _dense_conv_into(True, inp, lin, wp, bp, cin_p, width, 3, False, n, h, w, z, lz, out_f32=1):
                        raise _DenseRefused()
                    _prelu_bf16(z, lz, slopes[i], ycat, lsl[j], width, n, h, w)
                    zbufs.append(z)
                ybufs.append(ycat)
                src, lsrc, csrc = ycat, lcat, 3 * width
            wp, bp = _packed_for(weights[L - 2], biases[L - 2], 'fwd16', epoch, resync)
            lz6 = _capi.Layout.dense(c6, h, w)
            z6 = _buffer(lz6, n, h, w, dev, False)
            if not _dense_conv_into(True, src, lsrc, wp, bp, csrc, c6, 1, False, n, h, w, z6, lz6, out_f32=1):
                raise _DenseRefused()
            y6 = _buffer(lz6, n, h, w, dev, True, True)
            _prelu_bf16(z6, lz6, slopes[L - 2], y6, lz6, c6, n, h, w)
            zbufs.append(z6)
            wp, bp = _packed_for(weights[L - 1], biases[L - 1], 'fwd16', epoch, resync)
            lo = _capi.Layout.dense(_up8(cout), h, w)
            obuf = _buffer(lo, n, h, w, dev, False)
            if not _dense_conv_into(True, y6, lz6, wp, bp, c6, cout, 1, False, n, h, w, obuf, lo, out_f32=1):
                raise _DenseRefused()
            y = _from_layout(obuf, lo, n, cout, h, w)
        need = ctx.needs_input_grad
        wants = [need[2 + 3 * i] or (biases[i] is not None and need[3 + 3 * i]) for i in range(L)]
        need_a = [slopes[i] is not None and need[4 + 3 * i] for i in range(L)]
        # the lowest layer whose backward anything needs: the walk stops there
        low = 0 if need[0] else next((i for i in range(L) if wants[i] or need_a[i]), L)
        ctx.geom = (n, cin, h, w)
        ctx.meta = meta
        ctx.weights, ctx.slopes = weights, slopes
        ctx.has_bias = [b is not None for b in biases]
        ctx.low, ctx.wants, ctx.need_a = low, wants, need_a
        # (for autograd's check that the filters and slopes were not modified in place since)
        ctx.save_for_backward(*(weights + tuple(s for s in slopes if s is not None)))
        # the fp32 pre-activations from the lowest layer up, and a bf16 input buffer where a weight gradient reads it
        ctx.zbufs = [z if i >= low else None for i, z in enumerate(zbufs)]
        ctx.xbuf, ctx.lx = (xbuf, lx) if wants[0] else (None, None)
        ctx.ybufs = [yc if any(wants[3 * b + 1:3 * b + 4]) else None for b, yc in enumerate(ybufs)]
        ctx.y6 = y6 if wants[L - 1] else None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        epoch, resync = ctx.meta
        ctx.saved_tensors
        weights, slopes, low, wants, need_a = ctx.weights, ctx.slopes, ctx.low, ctx.wants, ctx.need_a
        L = len(weights)
        B = (L - 2) // 3
        n, cin0, h, w = ctx.geom
        need_x = ctx.needs_input_grad[0]
        grads = [None] * (3 * L)
        dx = None
        if low >= L:
            return (None, None) + tuple(grads)
        width, c6 = weights[0].shape[0], weights[L - 2].shape[0]
        with torch.cuda.device(gy.device):
            dev = gy.device
            lz, lz6 = _capi.Layout.dense(width, h, w), _capi.Layout.dense(c6, h, w)
            lcat = _capi.Layout.padded(3 * width, h, w, 1)
            lsl = [_capi.Layout.padded(3 * width, h, w, 1, j * width) for j in range(3)]
            ldc = [_capi.Layout.dense(3 * width, h, w, j * width) for j in range(3)]    # the slices of a concat gradient

            def weight_grads(i, inp, lin, g, lg):
                if wants[i]:
                    wt = weights[i]
                    need_b = ctx.has_bias[i] and ctx.needs_input_grad[3 + 3 * i]
                    dw, db = _wgrad(True, inp, lin, g, lg, wt, wt.shape[1], wt.shape[0], wt.shape[2], n, h, w, need_b)
                    grads[3 * i] = dw if ctx.needs_input_grad[2 + 3 * i] else None
                    grads[3 * i + 1] = db

            def data_grad(i, g, lg):
                """the conv of the bf16 gradient g on the flipped, transposed filter of layer i into a new dense fp32
                buffer: (buffer, layout)"""
                wt = weights[i]
                cin, k = wt.shape[1], wt.shape[2]
                wp, bp = _packed_for(wt, None, 'bwd16', epoch, resync)
                ld = _capi.Layout.dense(_up8(cin), h, w)
                d = _buffer(ld, n, h, w, dev, False)
                if _dense_conv_into(True, g, lg, wp, bp, lg.cstride, cin, k, False, n, h, w, d, ld, out_f32=1):
                    return d, ld
                # refused: this one conv in fp32 on the widened gradient
                return _dgrad_fp32_fallback(g, lg, wt, n, h, w, epoch, resync)

            # Mconv7: no activation behind it, gy is rounded as it enters
            g, lg = _to_layout(gy.detach().float().contiguous(), 0, True)
            weight_grads(L - 1, ctx.y6, lz6, g, lg)
            if low < L - 1:
                d, ld = data_grad(L - 1, g, lg)
                # Mconv6
                g = _buffer(lz6, n, h, w, dev, True, True)
                grads[3 * (L - 2) + 2] = _prelu_grad_bf16(ctx.zbufs[L - 2], lz6, slopes[L - 2], d, ld, None, None, g, lz6, c6,
                                                          n, h, w, need_a[L - 2])
                weight_grads(L - 2, ctx.ybufs[B - 1], lcat, g, lz6)
            if low < L - 2:
                dc, _ = data_grad(L - 2, g, lz6)     # the gradient of the last block's concat: dense fp32, 3 x width
                # every 3x3 conv's gradient goes through ONE bf16 buffer gapped by 1: a launch writes all its valid pixels
                # and none of its gaps, which stay the zeros they were made
                lg = _capi.Layout.padded(width, h, w, 1)
                g = _buffer(lg, n, h, w, dev, True, True)
                d = ld = None
                for i in range(L - 3, low - 1, -1):
                    b, j = divmod(i, 3)
                    # the activation of conv (b, j) is read by the concat and, for j < 2, by conv (b, j + 1) as well
                    grads[3 * i + 2] = _prelu_grad_bf16(ctx.zbufs[i], lz, slopes[i], dc, ldc[j], d if j < 2 else None,
                                                        ld if j < 2 else None, g, lg, width, n, h, w, need_a[i])
                    if j:
                        weight_grads(i, ctx.ybufs[b], lsl[j - 1], g, lg)
                    elif b:
                        weight_grads(i, ctx.ybufs[b - 1], lcat, g, lg)
                    else:
                        weight_grads(i, ctx.xbuf, ctx.lx, g, lg)
                    if i == low and not (i == 0 and need_x):
                        break
                    if j:
                        d, ld = data_grad(i, g, lg)
                    elif b:
                        dc, _ = data_grad(i, g, lg)   # the gradient of the concat of the block below
                    else:
                        d, ld = data_grad(i, g, lg)
                        dx = _from_layout(d, ld, n, cin0, h, w)
        return (dx, None) + tuple(grads)


def _dense_per_conv(x, layers, epoch, resync):
    """the stage through conv2d(compute_dtype='bf16') and torch.cat: what dense_stage falls back to"""
    L = len(layers)
    for b in range((L - 2) // 3):
        outs = []
        for wt, bias, slope in layers[3 * b:3 * b + 3]:
            x = conv2d(x, wt, bias, False, epoch, resync, slope, 'bf16')
            outs.append(x)
        x = torch.cat(outs, 1)
    for wt, bias, slope in layers[L - 2:]:
        x = conv2d(x, wt, bias, False, epoch, resync, slope, 'bf16')
    return x


def dense_stage(x, layers, epoch=0, resync=False):
    """A ``StageBlock`` of an ``OpenPose_Model`` (lib/network/openpose.py:86-109) as ONE autograd node, bf16 operands: B
    dense blocks of three 3x3 convs with PReLU whose outputs are concatenated, the 1x1 conv Mconv6 with PReLU, the 1x1
    conv Mconv7.  `x`: NCHW fp32 on the device; `layers`: 3 B + 2 triples (weight, bias_or_None, slope_or_None) in that
    order - the first conv of a block reads x or the 3 C channels of the block before, the other two C channels; every slope
    the fp32 [cout] weight of an ``nn.PReLU``, None for Mconv7.  Returns Mconv7's output, NCHW fp32.  `epoch` / `resync`: see
    ``conv2d``; the packings are the cached 'fwd16' / 'bwd16' ones.

    Every conv launch is ``conv2d(compute_dtype='bf16')``'s: ``rtpose_conv2d_bf16(out_f32 = 1)`` forward and data gradient,
    ``rtpose_conv2d_wgrad_bf16``.  What lies between them is two kernels.  Forward: x is converted once
    (``rtpose_nchw_to_layout_bf16``, gap 1); a block has ONE zero-initialised bf16 buffer of 3 C channels (gap 1): conv
    (b, j) reads x or the whole buffer of the block before (j = 0) or slice j - 1 of its own block's, writes its fp32
    pre-activation z into a dense buffer - the only fp32 activation kept - and ``rtpose_prelu_bf16`` writes slice j.  The
    concat is never made: it is the buffer.  Mconv6 reads the last one whole; Mconv7's fp32 output leaves through one
    ``rtpose_layout_to_nchw``.  Backward: gy is converted once; a layer's bf16 output gradient is
    ``rtpose_prelu_grad_bf16`` of its z and the fp32 data gradient(s) of its consumer(s) - the slice of the concat's
    gradient and, for the first two convs of a block, the next conv's as well, summed in fp32 as autograd sums them -; its
    weight gradient reads the kept bf16 slice, its data gradient is a dense fp32 buffer.  The walk stops at the lowest
    layer anything needs, a slope gradient is computed only where that slope requires one, dx only if x does.

    The rounding points are the per-conv path's: the fp32 PReLU output rounded at the store is what the next conv's input
    conversion made of it, the fp32 PReLU gradient rounded at the store is ``rtpose_layout_f32_to_bf16`` of it.

    The stage gives up residency - it runs conv by conv through ``conv2d`` and ``torch.cat``, and ``dense_fallbacks``
    counts it - when C or Mconv6's width is no multiple of 16 (the bf16 conv reads 16-channel groups: a slice must own
    its groups), decided before any launch, or when ``rtpose_conv2d_bf16`` refuses a forward conv (it refuses before
    launching; the node's earlier launches are abandoned).  A refused data gradient runs that one conv in fp32 on the
    widened gradient (``rtpose_layout_bf16_to_f32``) and is counted in ``bf16_fallbacks['dgrad']``."""
    global dense_fallbacks
    layers = [tuple(layer) if isinstance(layer, (tuple, list)) else layer for layer in layers]
    _check_dense(x, layers)
    epoch, resync = int(epoch), bool(resync)
    if layers[0][0].shape[0] % 16 == 0 and layers[-2][0].shape[0] % 16 == 0:
        try:
            return _DenseStage.apply(x, (epoch, resync), *[p for layer in layers for p in layer])
        except _DenseRefused:
            pass
    dense_fallbacks += 1
    return _dense_per_conv(x, layers, epoch, resync)


# ---- the stacked hourglass: its stem and training-mode BatchNorm -------------------------------------------------------------
class _Conv7x7S2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, epoch, resync):
        _require_device("train.conv7x7_s2", x, weight)
        if (x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3
                or tuple(weight.shape) != (64, 3, 7, 7) or (bias is not None and tuple(bias.shape) != (64,))):
            raise _capi.RtposeError("train.conv7x7_s2 is nn.Conv2d(3, 64, 7, stride 2, padding 3) on an NCHW fp32 image; got "
                                    "filters %s for input %s" % (tuple(weight.shape), tuple(x.shape)))
        if ctx.needs_input_grad[0]:
            raise _capi.RtposeError("train.conv7x7_s2: the stem reads the image and has no data gradient; x must not require "
                                    "a gradient")
        with torch.cuda.device(x.device):
            n, _, h, w = x.shape
            ho, wo = (h + 1) // 2, (w + 1) // 2
            xc = x.detach().contiguous()
            wp, _ = _packed_for(weight, bias, 'stem', epoch, resync)
            ly = _capi.Layout.dense(64, ho, wo)
            ybuf = _buffer(ly, n, ho, wo, x.device, False)
            check(lib.rtpose_conv7x7_s2(ptr(xc), None, None, ptr(wp), ptr(ybuf), C.byref(ly), 0, n, h, w, current_stream()),
                  "rtpose_conv7x7_s2")
            y = _from_layout(ybuf, ly, n, 64, ho, wo)
        ctx.geom = (n, h, w, ho, wo)
        ctx.has_bias = bias is not None
        ctx.x = xc if (ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2])) else None
        ctx.save_for_backward(weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        """The weight gradient as the stride-1 k = 7 one on the zero-stuffed gradient: gyz[n, :, 2 y, 2 x] = gy[n, :, y, x]
        and zero elsewhere, an H x W map; then dW[o][c][dy][dx] = sum gyz[n, Y, X, o] * x[n, Y + dy - 3, X + dx - 3, c]
        exactly (the zeros add nothing), which is rtpose_conv2d_wgrad on the image layout with a gap of 3."""
        (weight,) = ctx.saved_tensors
        n, h, w, ho, wo = ctx.geom
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dw = db = None
        with torch.cuda.device(gy.device):
            gbuf, lg = _zero_stuffed_layout(gy, h, w, 3)
            xbuf, lx = _to_layout(ctx.x, 3)
            dw, db = _wgrad(False, xbuf, lx, gbuf, lg, weight, 3, 64, 7, n, h, w, need_b)
            if not need_w:
                dw = None
        return None, dw, db, None, None


def conv7x7_s2(x, weight, bias=None, epoch=0, resync=False):
    """``conv2d(x, weight, bias, stride=2, padding=3)`` of the hourglass stem (nn.Conv2d(3, 64, 7, 2, 3), no activation):
    forward ``rtpose_conv7x7_s2`` on the packing of the unfolded filter, weight and bias gradients from
    ``rtpose_conv2d_wgrad`` (k = 7) on the zero-stuffed output gradient - four times the necessary multiplies, on a
    3 -> 64 layer.  `x` is the image: one that requires a gradient is refused.  `epoch` / `resync`: see ``conv2d``."""
    return _Conv7x7S2.apply(x, weight, bias, int(epoch), bool(resync))


# ---- ShuffleNetV2: its depthwise 3x3 convs and its stem --------------------------------------------------------------------------
def _dw_taps(weight, cp):
    """[C, 1, 3, 3] -> the [9][cp] tap-major packing rtpose_dwconv3x3 reads (channels past C zero), and a zero bias"""
    c = weight.shape[0]
    taps = torch.zeros((9, cp), dtype=torch.float32, device=weight.device)
    taps[:, :c] = weight.detach().reshape(c, 9).t()
    return taps, torch.zeros(cp, dtype=torch.float32, device=weight.device)


def _dw_forward_into(bf16, xbuf, lx, taps, zero, cp, n, h, w, stride):
    """rtpose_dwconv3x3 - `bf16`: rtpose_dwconv3x3_bf16_f32 on a bf16 buffer - of the first `cp` channels of a gapped layout
    buffer into a new dense fp32 one: (buffer, layout)"""
    name = "rtpose_dwconv3x3_bf16_f32" if bf16 else "rtpose_dwconv3x3"
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ly = _capi.Layout.dense(cp, ho, wo)
    ybuf = _buffer(ly, n, ho, wo, xbuf.device, False)
    check(getattr(lib, name)(ptr(xbuf), C.byref(lx), ptr(taps), ptr(zero), ptr(ybuf), C.byref(ly), cp, n, h, w, stride,
                             current_stream()), name)
    return ybuf, ly


def _dw_dgrad(bf16, gbuf, lg, taps, cp, n, h, w, stride):
    """rtpose_dwconv3x3_dgrad - `bf16`: rtpose_dwconv3x3_dgrad_bf16 on a bf16 gradient - of `cp` channels into a new dense fp32
    buffer of the conv's h x w input: (buffer, layout)"""
    name = "rtpose_dwconv3x3_dgrad_bf16" if bf16 else "rtpose_dwconv3x3_dgrad"
    ld = _capi.Layout.dense(cp, h, w)
    dbuf = _buffer(ld, n, h, w, gbuf.device, False)
    check(getattr(lib, name)(ptr(gbuf), C.byref(lg), ptr(taps), ptr(dbuf), C.byref(ld), cp, n, h, w, stride, current_stream()),
          name)
    return dbuf, ld


def _dw_wgrad(bf16, xbuf, lx, gbuf, lg, like_weight, c, n, h, w, stride):
    """rtpose_dwconv3x3_wgrad - `bf16`: rtpose_dwconv3x3_wgrad_bf16 on bf16 buffers - : dw shaped like `like_weight`, fp32"""
    name = "rtpose_dwconv3x3_wgrad_bf16" if bf16 else "rtpose_dwconv3x3_wgrad"
    dw = torch.empty_like(like_weight, memory_format=torch.contiguous_format)
    doubles = lib.rtpose_dwconv3x3_wgrad_workspace_doubles(c, n, h, w, stride)
    ws = torch.empty(doubles, dtype=torch.float64, device=gbuf.device)
    check(getattr(lib, name)(ptr(xbuf), C.byref(lx), ptr(gbuf), C.byref(lg), ptr(dw), None, ptr(ws), doubles, c, n, h, w, stride,
                             current_stream()), name)
    return dw


class _DwConv3x3(torch.autograd.Function):
    """dwconv3x3's node.  With `bf16` the activations of all three kernels are bf16 (x and gy rounded as they enter, the
    channels rounded up to 16); the taps, the outputs and the gradients are fp32 in both."""
    @staticmethod
    def forward(ctx, x, weight, stride, bf16):
        _require_device("train.dwconv3x3", x, weight)
        if stride not in (1, 2):
            raise _capi.RtposeError("train.dwconv3x3: stride must be 1 or 2; got %r" % (stride,))
        if (x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 4
                or tuple(weight.shape) != (x.shape[1], 1, 3, 3)):
            raise _capi.RtposeError("train.dwconv3x3 is nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False) on an NCHW fp32 input: "
                                    "filters [C, 1, 3, 3]; got filters %s %s for input %s %s"
                                    % (weight.dtype, tuple(weight.shape), x.dtype, tuple(x.shape)))
        with torch.cuda.device(x.device):
            n, c, h, w = x.shape
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            xbuf, lx = _to_layout(x.detach().contiguous(), 1, bf16)
            taps, zero = _dw_taps(weight, lx.cstride)
            ybuf, ly = _dw_forward_into(bf16, xbuf, lx, taps, zero, lx.cstride, n, h, w, stride)
            y = _from_layout(ybuf, ly, n, c, ho, wo)
        ctx.geom = (n, c, h, w, ho, wo, stride)
        ctx.bf16 = bf16
        ctx.save_for_backward(weight)    # (for autograd's check that the filters were not modified in place since)
        ctx.xbuf, ctx.lx = (xbuf, lx) if ctx.needs_input_grad[1] else (None, None)
        ctx.taps = taps if ctx.needs_input_grad[0] else None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (weight,) = ctx.saved_tensors
        n, c, h, w, ho, wo, stride = ctx.geom
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        with torch.cuda.device(gy.device):
            gbuf, lg = _to_layout(gy.detach().float().contiguous(), 1, ctx.bf16)
            if need_x:
                dbuf, ld = _dw_dgrad(ctx.bf16, gbuf, lg, ctx.taps, lg.cstride, n, h, w, stride)
                dx = _from_layout(dbuf, ld, n, c, h, w)
            if need_w:
                dw = _dw_wgrad(ctx.bf16, ctx.xbuf, ctx.lx, gbuf, lg, weight, c, n, h, w, stride)
        return dx, dw, None, None


def dwconv3x3(x, weight, stride=1, compute_dtype='fp32'):
    """``conv2d(x, weight, None, stride, 1, groups=C)`` of an ``nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)``, stride 1
    or 2, with the library's kernels in both directions; NCHW fp32 device tensors, `weight` [C, 1, 3, 3].  Forward:
    ``rtpose_dwconv3x3`` on the channels rounded up to 8, with the taps permuted to its [9][C] packing by torch ops on the
    device on every call (9 C floats: nothing is cached, so nothing needs invalidating) and a zero bias.  Backward:
    ``rtpose_dwconv3x3_dgrad`` on the same taps and ``rtpose_dwconv3x3_wgrad`` on the kept layout copy of x, each only if its
    gradient is needed.
    `compute_dtype`: 'fp32', the path above launch for launch, or 'bf16' for bf16 activations with fp32 taps and fp32
    accumulation: x enters through ``rtpose_nchw_to_layout_bf16`` (round to nearest even, gap 1, channels rounded up to 16)
    and is what is kept for the weight gradient, ``rtpose_dwconv3x3_bf16_f32`` writes a dense fp32 buffer that leaves as
    NCHW fp32; gy enters through ``rtpose_nchw_to_layout_bf16`` (gap 1) and ``rtpose_dwconv3x3_dgrad_bf16`` /
    ``rtpose_dwconv3x3_wgrad_bf16`` run, each only if its gradient is needed.  The two roundings are the only difference from
    'fp32': parameters, outputs and gradients are fp32 either way (tests/dwconv_bf16_restate.py is the host emulation)."""
    _check_compute_dtype("train.dwconv3x3", compute_dtype)
    return _DwConv3x3.apply(x, weight, stride, compute_dtype == 'bf16')


class _Conv3x3S2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, epoch, resync):
        _require_device("train.conv3x3_s2", x, weight)
        if (x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3
                or tuple(weight.shape) != (24, 3, 3, 3)):
            raise _capi.RtposeError("train.conv3x3_s2 is nn.Conv2d(3, 24, 3, stride 2, padding 1, bias=False) on an NCHW fp32 "
                                    "image; got filters %s %s for input %s %s"
                                    % (weight.dtype, tuple(weight.shape), x.dtype, tuple(x.shape)))
        with torch.cuda.device(x.device):
            n, _, h, w = x.shape
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            xbuf, lx = _to_layout(x.detach().contiguous(), 1)
            # the kernel's packing: [tap][input channel, padded to 8][output channel]
            taps = torch.zeros((9, 8, 24), dtype=torch.float32, device=x.device)
            taps[:, :3] = weight.detach().permute(2, 3, 1, 0).reshape(9, 3, 24)
            zero = torch.zeros(24, dtype=torch.float32, device=x.device)
            ly = _capi.Layout.dense(24, ho, wo)
            ybuf = _buffer(ly, n, ho, wo, x.device, False)
            check(lib.rtpose_stem_conv3x3_s2(ptr(xbuf), C.byref(lx), ptr(taps), ptr(zero), ptr(ybuf), C.byref(ly), 8, 24, n, h, w,
                                             0, current_stream()), "rtpose_stem_conv3x3_s2")
            y = _from_layout(ybuf, ly, n, 24, ho, wo)
        ctx.geom = (n, h, w)
        ctx.weight, ctx.epoch, ctx.resync = weight, epoch, resync
        ctx.save_for_backward(weight)
        ctx.xbuf, ctx.lx = (xbuf, lx) if ctx.needs_input_grad[1] else (None, None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        """Both gradients from the stride-1 k = 3 kernels on the zero-stuffed gradient: gyz[n, :, 2 y, 2 x] = gy[n, :, y, x] and
        zero elsewhere, an H x W map.  dW[o][c][ky][kx] = sum gyz[n, Y, X, o] * x[n, Y + ky - 1, X + kx - 1, c] and
        dx[n, Y, X, c] = sum w[o][c][ky][kx] * gyz[n, Y + 1 - ky, X + 1 - kx, o] exactly: the zeros add nothing."""
        (weight,) = ctx.saved_tensors
        n, h, w = ctx.geom
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        with torch.cuda.device(gy.device):
            gbuf, lg = _zero_stuffed_layout(gy, h, w, 1)
            if need_x:
                wp, bp = _packed_for(ctx.weight, None, 'bwd', ctx.epoch, ctx.resync)
                dbuf, ld = _launch_conv(False, gbuf, lg, wp, bp, lg.cstride, 3, 3, False, n, h, w)
                dx = _from_layout(dbuf, ld, n, 3, h, w)
            if need_w:
                dw, _ = _wgrad(False, ctx.xbuf, ctx.lx, gbuf, lg, weight, 3, 24, 3, n, h, w, False)
        return dx, dw, None, None


def conv3x3_s2(x, weight, epoch=0, resync=False):
    """``conv2d(x, weight, None, stride=2, padding=1)`` of the ShuffleNetV2 stem (nn.Conv2d(3, 24, 3, 2, 1, bias=False), no
    activation): forward ``rtpose_stem_conv3x3_s2`` (relu = 0, a zero bias; the taps permuted to its packing on every call).
    Unlike the hourglass stem this one has a data gradient - ``data/bn`` in front of it trains: the weight gradient is
    ``rtpose_conv2d_wgrad`` (k = 3) and the data gradient ``rtpose_conv2d`` (k = 3, the cached ``dgrad_weights`` packing) of
    the zero-stuffed H x W output gradient.  Both reuses spend four times the necessary multiplies, on a 3 -> 24 layer.
    `epoch` / `resync`: see ``conv2d``."""
    return _Conv3x3S2.apply(x, weight, int(epoch), bool(resync))


def _check_bn(x, bn):
    if not isinstance(bn, nn.BatchNorm2d):
        raise _capi.RtposeError("train.batch_norm takes an nn.BatchNorm2d; got %s" % type(bn).__name__)
    if not bn.training:
        raise _capi.RtposeError("train.batch_norm computes batch statistics: the nn.BatchNorm2d must be in training mode "
                                "(eval-mode fine-tuning on frozen statistics is out of scope)")
    if not bn.affine or not bn.track_running_stats:
        raise _capi.RtposeError("train.batch_norm: the nn.BatchNorm2d must have affine=True and track_running_stats=True")
    if bn.momentum is None:
        raise _capi.RtposeError("train.batch_norm: momentum=None (the cumulative moving average) is not supported; give the "
                                "nn.BatchNorm2d a momentum")
    _require_device("train.batch_norm", x, bn.weight, names=("x", "the BatchNorm"))
    if x.dtype != torch.float32 or bn.weight.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != bn.num_features:
        raise _capi.RtposeError("train.batch_norm takes an NCHW fp32 input with %d channels; got %s %s"
                                % (bn.num_features, x.dtype, tuple(x.shape)))
    if x.shape[0] * x.shape[2] * x.shape[3] < 2:
        raise _capi.RtposeError("train.batch_norm: expected more than 1 value per channel when training; got input size %s"
                                % (tuple(x.shape),))


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu):
        _check_bn(x, bn)
        with torch.cuda.device(x.device):
            stream = current_stream()
            n, c, h, w = x.shape
            xbuf, lx = _to_layout(x.detach().contiguous(), 0)
            doubles = lib.rtpose_bn_workspace_doubles(c, n, h, w)
            ws = torch.empty(doubles, dtype=torch.float64, device=x.device)
            save = torch.empty(_capi.BN_SAVE_ROWS * c, dtype=torch.float32, device=x.device)
            rm, rv = bn.running_mean, bn.running_var
            if not (rm.is_contiguous() and rv.is_contiguous() and rm.dtype == rv.dtype == torch.float32):
                raise _capi.RtposeError("train.batch_norm: running_mean / running_var must be contiguous fp32 tensors")
            check(lib.rtpose_bn_stats(ptr(xbuf), C.byref(lx), ptr(weight.detach().contiguous()), ptr(bias.detach().contiguous()),
                                      ptr(rm), ptr(rv), float(bn.momentum), float(bn.eps), ptr(save), ptr(ws), doubles,
                                      c, n, h, w, stream), "rtpose_bn_stats")
            bn.num_batches_tracked.add_(1)
            ybuf = _buffer(lx, n, h, w, x.device, False)
            check(lib.rtpose_bn_apply(ptr(xbuf), C.byref(lx), ptr(save), ptr(ybuf), C.byref(lx), 1 if relu else 0, c, n, h, w,
                                      stream), "rtpose_bn_apply")
            y = _from_layout(ybuf, lx, n, c, h, w)
        ctx.geom = (n, c, h, w)
        ctx.relu = bool(relu)
        ctx.save_for_backward(weight)    # (for autograd's check that the weight was not modified in place since)
        ctx.xbuf, ctx.lx, ctx.save = (xbuf, lx, save) if any(ctx.needs_input_grad[:3]) else (None, None, None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        (weight,) = ctx.saved_tensors
        n, c, h, w = ctx.geom
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = dw = db = None
        with torch.cuda.device(gy.device):
            gbuf, lg = _to_layout(gy.detach().float().contiguous(), 0)
            doubles = lib.rtpose_bn_workspace_doubles(c, n, h, w)
            ws = torch.empty(doubles, dtype=torch.float64, device=gy.device)
            dw = torch.empty(c, dtype=torch.float32, device=gy.device) if need_w else None
            db = torch.empty(c, dtype=torch.float32, device=gy.device) if need_b else None
            # dx onto gy's own buffer: every element reads only its own gy element
            check(lib.rtpose_bn_grad(ptr(ctx.xbuf), C.byref(ctx.lx), ptr(gbuf), C.byref(lg), ptr(ctx.save),
                                     ptr(weight.detach().contiguous()), 1 if ctx.relu else 0, ptr(gbuf) if need_x else None,
                                     C.byref(lg) if need_x else None, ptr(dw), ptr(db), ptr(ws), doubles, c, n, h, w,
                                     current_stream()), "rtpose_bn_grad")
            if need_x:
                dx = _from_layout(gbuf, lg, n, c, h, w)
        return dx, dw, db, None, None


def batch_norm(x, bn, relu=False):
    """``bn(x)`` of an ``nn.BatchNorm2d`` in training mode (affine, track_running_stats, a momentum), then ReLU if `relu`,
    with the library's kernels in both directions; NCHW fp32 device tensors.  Forward: ``rtpose_bn_stats`` (batch
    statistics in fp64; ``running_mean`` / ``running_var`` updated in place by the kernel, ``num_batches_tracked`` + 1) and
    ``rtpose_bn_apply``; backward: ``rtpose_bn_grad`` on the kept layout copy of x (the ReLU mask is recomputed from it; no y
    is kept), for any ``requires_grad`` subset of (x, weight, bias).  The kernels write the running statistics through raw
    pointers, which bumps no ``_version``: a model whose inference plan folds them calls ``invalidate_weights()``
    (``forward_train`` does)."""
    return _BatchNorm.apply(x, bn.weight, bn.bias, bn, bool(relu))


# ---- a run of BatchNorm -> ReLU -> conv triples as one autograd node: a pre-activation Bottleneck's main branch (bf16) ---------
# runs that gave up residency because rtpose_conv2d_bf16 refused one of their forward convs
preact_fallbacks = 0


def reset_preact_fallbacks():
    global preact_fallbacks
    preact_fallbacks = 0


class _PreactRefused(Exception):
    """rtpose_conv2d_bf16 refused a forward conv of a pre-activation run (before any launch of that conv)"""


# the name _PreactChain launches its convs through, and nothing else does: replacing it plays a refusal of the node's own
# launches and leaves alone the conv2d nodes the run falls back to (tests/test_train_bottleneck_gpu.py)
_preact_conv_into = _conv_launch


def _bn_workspace(c, n, h, w, device):
    doubles = lib.rtpose_bn_workspace_doubles(c, n, h, w)
    return torch.empty(doubles, dtype=torch.float64, device=device), doubles


def _check_preact(x, layers):
    who = "train.preact_chain"
    if len(layers) < 1:
        raise _capi.RtposeError("%s: no layers" % who)
    for i, layer in enumerate(layers):
        if not isinstance(layer, tuple) or len(layer) != 3 or not torch.is_tensor(layer[1]):
            raise _capi.RtposeError("%s: layers are (nn.BatchNorm2d, weight, bias_or_None) triples; got %r at %d"
                                    % (who, type(layer).__name__, i))
    _require_device(who, x, names=("x",))
    if x.dtype != torch.float32 or x.dim() != 4:
        raise _capi.RtposeError("%s takes an NCHW fp32 input; got %s %s" % (who, x.dtype, tuple(x.shape)))
    c = x.shape[1]
    for i, (bn, weight, bias) in enumerate(layers):
        # (the BatchNorm's input has the run's n, h, w and c channels: a view of that shape stands for it)
        _check_bn(x[:, :1].expand(-1, c, -1, -1), bn)
        rm, rv = bn.running_mean, bn.running_var
        if not (rm.is_contiguous() and rv.is_contiguous() and rm.dtype == rv.dtype == torch.float32):
            raise _capi.RtposeError("%s: running_mean / running_var must be contiguous fp32 tensors" % who)
        _require_device(who, weight, names=("a weight",))
        if not _is_same_conv_filter(weight, c):
            raise _capi.RtposeError("%s: layer %d: stride-1 'same' convs with fp32 OIHW filters, k in {1, 3, 7}, whose input "
                                    "channels are those of the BatchNorm in front (%s); got filters %s %s"
                                    % (who, i, c, weight.dtype, tuple(weight.shape)))
        if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (weight.shape[0],)
                                 or bias.device != weight.device):
            raise _capi.RtposeError("%s: layer %d: the bias is None or an fp32 [%d] tensor beside the filters"
                                    % (who, i, weight.shape[0]))
        c = weight.shape[0]


class _PreactChain(torch.autograd.Function):
    """preact_chain's node.  Inputs: x, (the BatchNorm modules, epoch, resync), then the BatchNorm's weight and bias and the
    conv's weight and bias (or None) of every triple."""
    @staticmethod
    def forward(ctx, x, meta, *params):
        bns, epoch, resync = meta
        gammas, betas, weights, biases = params[0::4], params[1::4], params[2::4], params[3::4]
        L = len(weights)
        with torch.cuda.device(x.device):
            stream = current_stream()
            dev = x.device
            n, _, h, w = x.shape
            # what a refusal puts back: the kernels below update the running statistics, and the per-conv run the node
            # falls back to updates them again
            stats = torch.cat([t for bn in bns for t in (bn.running_mean, bn.running_var)])
            cur, lcur = _to_layout(x.detach().contiguous(), 0)
            xins, lxins, saves, abufs, lays = [], [], [], [], []
            for i in range(L):
                cout, c, k = weights[i].shape[0], weights[i].shape[1], weights[i].shape[2]
                ws, doubles = _bn_workspace(c, n, h, w, dev)
                save = torch.empty(_capi.BN_SAVE_ROWS * c, dtype=torch.float32, device=dev)
                check(lib.rtpose_bn_stats(ptr(cur), C.byref(lcur), ptr(gammas[i].detach().contiguous()),
                                          ptr(betas[i].detach().contiguous()), ptr(bns[i].running_mean),
                                          ptr(bns[i].running_var), float(bns[i].momentum), float(bns[i].eps), ptr(save), ptr(ws),
                                          doubles, c, n, h, w, stream), "rtpose_bn_stats")
                # relu(bn(.)) rounded straight into the buffer the conv reads: gapped for it, its pad channels zero
                la = _capi.Layout.padded(_up16(c), h, w, k // 2)
                abuf = _buffer(la, n, h, w, dev, True, True)
                check(lib.rtpose_bn_apply_bf16(ptr(cur), C.byref(lcur), ptr(save), ptr(abuf), C.byref(la), 1, c, n, h, w, stream),
                      "rtpose_bn_apply_bf16")
                wp, bp = _packed_for(weights[i], biases[i], 'fwd16', epoch, resync)
                lz = _capi.Layout.dense(_up8(cout), h, w)
                z = _buffer(lz, n, h, w, dev, False)
                if not _preact_conv_into(True, abuf, la, wp, bp, la.cstride, cout, k, False, n, h, w, z, lz, out_f32=1):
                    for j, bn in enumerate(bns):
                        cj = bn.num_features
                        off = 2 * sum(b.num_features for b in bns[:j])
                        bn.running_mean.copy_(stats[off:off + cj])
                        bn.running_var.copy_(stats[off + cj:off + 2 * cj])
                    raise _PreactRefused()
                xins.append(cur), lxins.append(lcur), saves.append(save), abufs.append(abuf), lays.append(la)
                cur, lcur = z, lz
            for bn in bns:
                bn.num_batches_tracked.add_(1)
            y = _from_layout(cur, lcur, n, weights[L - 1].shape[0], h, w)
        need = ctx.needs_input_grad
        wants = [need[4 + 4 * i] or (biases[i] is not None and need[5 + 4 * i]) for i in range(L)]
        wants_bn = [need[2 + 4 * i] or need[3 + 4 * i] for i in range(L)]
        # the lowest triple whose backward anything needs: the walk stops there
        low = 0 if need[0] else next((i for i in range(L) if wants[i] or wants_bn[i]), L)
        ctx.geom = (n, h, w)
        ctx.meta = (epoch, resync)
        ctx.gammas, ctx.weights = gammas, weights
        ctx.has_bias = [b is not None for b in biases]
        ctx.low, ctx.wants, ctx.wants_bn = low, wants, wants_bn
        ctx.save_for_backward(*(gammas + weights))   # (for autograd's check that none was modified in place since)
        # per triple: the fp32 input of its BatchNorm and its save rows where the BatchNorm's backward runs, the bf16
        # activation where a weight gradient reads it; nothing else
        bn_runs = [i > low or (i == low and (wants_bn[i] or (i == 0 and need[0]))) for i in range(L)]
        ctx.bn_runs = bn_runs
        ctx.xins = [(b, l) if run else None for b, l, run in zip(xins, lxins, bn_runs)]
        ctx.saves = [s if run else None for s, run in zip(saves, bn_runs)]
        ctx.abufs = [(b, l) if i >= low and wants[i] else None for i, (b, l) in enumerate(zip(abufs, lays))]
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        epoch, resync = ctx.meta
        ctx.saved_tensors
        gammas, weights, low, wants, wants_bn = ctx.gammas, ctx.weights, ctx.low, ctx.wants, ctx.wants_bn
        L = len(weights)
        n, h, w = ctx.geom
        need = ctx.needs_input_grad
        grads = [None] * (4 * L)
        dx = None
        if low >= L:
            return (None, None) + tuple(grads)
        with torch.cuda.device(gy.device):
            dev = gy.device
            stream = current_stream()
            # no activation behind the last conv: gy is rounded as it enters
            g, lg = _to_layout(gy.detach().float().contiguous(), weights[L - 1].shape[2] // 2, True)
            for i in range(L - 1, low - 1, -1):
                wt = weights[i]
                cout, c, k = wt.shape[0], wt.shape[1], wt.shape[2]
                if wants[i]:
                    need_b = ctx.has_bias[i] and need[5 + 4 * i]
                    dw, db = _wgrad(True, ctx.abufs[i][0], ctx.abufs[i][1], g, lg, wt, c, cout, k, n, h, w, need_b)
                    grads[4 * i + 2] = dw if need[4 + 4 * i] else None
                    grads[4 * i + 3] = db
                if not ctx.bn_runs[i]:
                    break
                # the data gradient: the conv of g on the flipped, transposed filter into a dense fp32 buffer
                wp, bp = _packed_for(wt, None, 'bwd16', epoch, resync)
                ld = _capi.Layout.dense(_up8(c), h, w)
                d = _buffer(ld, n, h, w, dev, False)
                if not _preact_conv_into(True, g, lg, wp, bp, lg.cstride, c, k, False, n, h, w, d, ld, out_f32=1):
                    d, ld = _dgrad_fp32_fallback(g, lg, wt, n, h, w, epoch, resync)   # refused: this one conv in fp32
                xin, lxin = ctx.xins[i]
                ws, doubles = _bn_workspace(c, n, h, w, dev)
                dgam = torch.empty(c, dtype=torch.float32, device=dev) if need[2 + 4 * i] else None
                dbet = torch.empty(c, dtype=torch.float32, device=dev) if need[3 + 4 * i] else None
                gamma = ptr(gammas[i].detach().contiguous())
                if i > 0:
                    # through the ReLU and the BatchNorm straight into the bf16 gradient the conv below reads, gapped for it
                    need_dx = i > low
                    if need_dx:
                        lg = _capi.Layout.padded(_up16(c), h, w, weights[i - 1].shape[2] // 2)
                        g = _buffer(lg, n, h, w, dev, True, True)
                    check(lib.rtpose_bn_grad_bf16(ptr(xin), C.byref(lxin), ptr(d), C.byref(ld), ptr(ctx.saves[i]), gamma, 1,
                                                  ptr(g) if need_dx else None, C.byref(lg) if need_dx else None, ptr(dgam),
                                                  ptr(dbet), ptr(ws), doubles, c, n, h, w, stream), "rtpose_bn_grad_bf16")
                else:
                    # the lowest BatchNorm: its dx leaves as NCHW fp32 (onto the data gradient's own buffer, as batch_norm does)
                    check(lib.rtpose_bn_grad(ptr(xin), C.byref(lxin), ptr(d), C.byref(ld), ptr(ctx.saves[i]), gamma, 1,
                                             ptr(d) if need[0] else None, C.byref(ld) if need[0] else None, ptr(dgam), ptr(dbet),
                                             ptr(ws), doubles, c, n, h, w, stream), "rtpose_bn_grad")
                    if need[0]:
                        dx = _from_layout(d, ld, n, c, h, w)
                grads[4 * i], grads[4 * i + 1] = dgam, dbet
        return (dx, None) + tuple(grads)


def preact_chain(x, layers, epoch=0, resync=False):
    """A run of L >= 1 triples BatchNorm -> ReLU -> stride-1 "same" conv (k in {1, 3, 7}) - the main branch of a
    pre-activation Bottleneck - as ONE autograd node, bf16 operands.  `layers`: (``nn.BatchNorm2d`` in training mode, conv
    weight, conv bias or None) triples, every BatchNorm on the channels the conv before it writes; `x` NCHW fp32 on the
    device.  Returns the last conv's output, NCHW fp32.  The BatchNorm checks are ``batch_norm``'s, the conv checks
    ``conv_chain``'s; `epoch` / `resync`: see ``conv2d``; the packings are the cached 'fwd16' / 'bwd16' ones.

    Forward: x enters through one ``rtpose_nchw_to_layout`` as fp32 and is kept for the first BatchNorm's backward.  Per
    triple: ``rtpose_bn_stats`` on the fp32 buffer (the running statistics updated by the kernel, ``num_batches_tracked``
    + 1, as ``batch_norm`` does), ``rtpose_bn_apply_bf16(relu = 1)`` into a zero-initialised bf16 buffer gapped for the
    conv that reads it with the channels rounded up to 16, ``rtpose_conv2d_bf16(out_f32 = 1)`` on the 'fwd16' packing into
    a dense fp32 pre-activation buffer - the next BatchNorm's input.  The last one leaves through one
    ``rtpose_layout_to_nchw``.  Kept per triple: the fp32 input of its BatchNorm, its ``save`` rows, and the bf16 activation
    where a weight gradient reads it.
    Backward (``once_differentiable``; any ``requires_grad`` subset of x, the BatchNorm weights and biases, the filters and
    biases): gy enters through one ``rtpose_nchw_to_layout_bf16``; per triple, top down, ``rtpose_conv2d_wgrad_bf16`` on the
    kept bf16 activation, the data gradient as ``rtpose_conv2d_bf16(out_f32 = 1)`` on the 'bwd16' packing into a dense fp32
    buffer, and ``rtpose_bn_grad_bf16(relu = 1)`` on the kept fp32 input, which writes the bf16 gradient the conv below
    reads (gapped for it).  The lowest BatchNorm runs ``rtpose_bn_grad``: its dx leaves as NCHW fp32, only if x needs one.
    The walk stops at the lowest triple anything needs; a parameter gradient is computed only where it is required.

    No rounding point moves against ``conv2d(batch_norm(x, bn, relu=True), weight, bias, compute_dtype='bf16')`` repeated L
    times: the output, every gradient and the running statistics are equal to that composition's bit for bit.

    A forward conv ``rtpose_conv2d_bf16`` refuses (before launching) makes the run give up residency: the running statistics
    the node has updated so far are put back, the run goes triple by triple through ``batch_norm`` and
    ``conv2d(compute_dtype='bf16')`` - so every BatchNorm is updated once - and ``preact_fallbacks`` counts it.  A refused data
    gradient runs that one conv in fp32 on the widened gradient and is counted in ``bf16_fallbacks['dgrad']``."""
    global preact_fallbacks
    layers = [tuple(layer) if isinstance(layer, (tuple, list)) else layer for layer in layers]
    _check_preact(x, layers)
    epoch, resync = int(epoch), bool(resync)
    meta = (tuple(bn for bn, _, _ in layers), epoch, resync)
    try:
        return _PreactChain.apply(x, meta, *[p for bn, wt, b in layers for p in (bn.weight, bn.bias, wt, b)])
    except _PreactRefused:
        preact_fallbacks += 1
    for bn, wt, b in layers:
        x = conv2d(batch_norm(x, bn, relu=True), wt, b, False, epoch, resync, None, 'bf16')
    return x


# ---- a run of op -> BatchNorm -> (ReLU) units as one autograd node: a ShuffleNetV2 block's branch (bf16) -------------------------
# runs that gave up residency because rtpose_conv2d_bf16 refused one of their forward convs
unit_fallbacks = 0


def reset_unit_fallbacks():
    global unit_fallbacks
    unit_fallbacks = 0


class _UnitRefused(Exception):
    """rtpose_conv2d_bf16 refused a forward conv of a run of units (before any launch of that conv)"""


# the name _UnitChain launches its pointwise convs through, and nothing else does: replacing it plays a refusal of the node's
# own launches and leaves alone the conv2d nodes the run falls back to (tests/test_train_branch_gpu.py)
_unit_conv_into = _conv_launch


def _unit_kind(m):
    """'pw' for a pointwise nn.Conv2d (1x1, stride 1), 'dw' for a depthwise 3x3 (padding 1, stride 1 or 2, groups = channels,
    no bias), None for anything else"""
    if not isinstance(m, nn.Conv2d) or m.dilation != (1, 1) or m.padding_mode != 'zeros':
        return None
    if m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0) and m.groups == 1:
        return 'pw'
    if (m.kernel_size == (3, 3) and m.stride in ((1, 1), (2, 2)) and m.padding == (1, 1) and m.groups == m.in_channels
            and m.out_channels == m.in_channels and m.bias is None):
        return 'dw'
    return None


def _unit_out_size(m, h, w):
    s = m.stride[0]
    return (h - 1) // s + 1, (w - 1) // s + 1


def _check_units(x, units):
    who = "train.unit_chain"
    if len(units) < 1:
        raise _capi.RtposeError("%s: no units" % who)
    for i, unit in enumerate(units):
        if not isinstance(unit, tuple) or len(unit) != 3 or not isinstance(unit[0], nn.Module):
            raise _capi.RtposeError("%s: units are (nn.Conv2d, nn.BatchNorm2d, relu) triples; got %r at %d"
                                    % (who, type(unit).__name__, i))
    _require_device(who, x, names=("x",))
    if x.dtype != torch.float32 or x.dim() != 4:
        raise _capi.RtposeError("%s takes an NCHW fp32 input; got %s %s" % (who, x.dtype, tuple(x.shape)))
    n, c, h, w = x.shape
    for i, (m, bn, _) in enumerate(units):
        if _unit_kind(m) is None:
            raise _capi.RtposeError("%s: unit %d: the op is a pointwise nn.Conv2d (1x1, stride 1) or a depthwise 3x3 (padding 1, "
                                    "stride 1 or 2, groups = channels, no bias); got %r" % (who, i, m))
        _require_device(who, m.weight, names=("a weight",))
        if m.weight.dtype != torch.float32 or m.in_channels != c:
            raise _capi.RtposeError("%s: unit %d: fp32 filters on the %d channels the unit before writes; got %r (%s)"
                                    % (who, i, c, m, m.weight.dtype))
        if m.bias is not None and (m.bias.dtype != torch.float32 or m.bias.device != m.weight.device):
            raise _capi.RtposeError("%s: unit %d: the bias is None or an fp32 [%d] tensor beside the filters"
                                    % (who, i, m.out_channels))
        c = m.out_channels
        h, w = _unit_out_size(m, h, w)
        # (the BatchNorm's input has the op's n, c, h, w: a view of that shape stands for it)
        _check_bn(x[:1, :1, :1, :1].expand(n, c, h, w), bn)
        rm, rv = bn.running_mean, bn.running_var
        if not (rm.is_contiguous() and rv.is_contiguous() and rm.dtype == rv.dtype == torch.float32):
            raise _capi.RtposeError("%s: running_mean / running_var must be contiguous fp32 tensors" % who)


class _UnitChain(torch.autograd.Function):
    """unit_chain's node.  Inputs: x, (the conv modules, the BatchNorm modules, the ReLU flags, epoch, resync), then the
    BatchNorm's weight and bias and the op's weight and bias (or None) of every unit."""
    @staticmethod
    def forward(ctx, x, meta, *params):
        mods, bns, relus, epoch, resync = meta
        gammas, betas, weights, biases = params[0::4], params[1::4], params[2::4], params[3::4]
        L = len(mods)
        kinds = [_unit_kind(m) for m in mods]
        strides = [m.stride[0] for m in mods]
        with torch.cuda.device(x.device):
            stream = current_stream()
            dev = x.device
            n, _, h, w = x.shape
            # what a refusal puts back: the kernels below update the running statistics, and the per-op run the node falls
            # back to updates them again
            stats = torch.cat([t for bn in bns for t in (bn.running_mean, bn.running_var)])
            cur, lcur = _to_layout(x.detach().contiguous(), 1 if kinds[0] == 'dw' else 0, True)
            xins, zs, saves, taps_of, sizes = [], [], [], [], []
            y = None
            for i in range(L):
                wt = weights[i]
                cout, c = wt.shape[0], lcur.cstride
                if kinds[i] == 'dw':
                    # (the first up8(C) channels of the buffer: the layout batch_norm gives the pre-activation)
                    taps, zero = _dw_taps(wt, _up8(cout))
                    z, lz = _dw_forward_into(True, cur, lcur, taps, zero, _up8(cout), n, h, w, strides[i])
                else:
                    taps = None
                    wp, bp = _packed_for(wt, biases[i], 'fwd16', epoch, resync)
                    lz = _capi.Layout.dense(_up8(cout), h, w)
                    z = _buffer(lz, n, h, w, dev, False)
                    if not _unit_conv_into(True, cur, lcur, wp, bp, c, cout, 1, False, n, h, w, z, lz, out_f32=1):
                        for j, bn in enumerate(bns):
                            cj = bn.num_features
                            off = 2 * sum(b.num_features for b in bns[:j])
                            bn.running_mean.copy_(stats[off:off + cj])
                            bn.running_var.copy_(stats[off + cj:off + 2 * cj])
                        raise _UnitRefused()
                ho, wo = _unit_out_size(mods[i], h, w)
                ws, doubles = _bn_workspace(cout, n, ho, wo, dev)
                save = torch.empty(_capi.BN_SAVE_ROWS * cout, dtype=torch.float32, device=dev)
                check(lib.rtpose_bn_stats(ptr(z), C.byref(lz), ptr(gammas[i].detach().contiguous()),
                                          ptr(betas[i].detach().contiguous()), ptr(bns[i].running_mean),
                                          ptr(bns[i].running_var), float(bns[i].momentum), float(bns[i].eps), ptr(save), ptr(ws),
                                          doubles, cout, n, ho, wo, stream), "rtpose_bn_stats")
                xins.append((cur, lcur)), zs.append((z, lz)), saves.append(save), taps_of.append(taps)
                sizes.append((h, w, ho, wo))
                relu = 1 if relus[i] else 0
                if i + 1 < L:
                    # bn(.) (+ ReLU) rounded straight into the buffer the next op reads: gapped for it, its pad channels zero
                    la = _capi.Layout.padded(_up16(cout), ho, wo, 1 if kinds[i + 1] == 'dw' else 0)
                    abuf = _buffer(la, n, ho, wo, dev, True, True)
                    check(lib.rtpose_bn_apply_bf16(ptr(z), C.byref(lz), ptr(save), ptr(abuf), C.byref(la), relu, cout, n, ho, wo,
                                                   stream), "rtpose_bn_apply_bf16")
                    cur, lcur = abuf, la
                else:
                    ybuf = _buffer(lz, n, ho, wo, dev, False)
                    check(lib.rtpose_bn_apply(ptr(z), C.byref(lz), ptr(save), ptr(ybuf), C.byref(lz), relu, cout, n, ho, wo,
                                              stream), "rtpose_bn_apply")
                    y = _from_layout(ybuf, lz, n, cout, ho, wo)
                h, w = ho, wo
            for bn in bns:
                bn.num_batches_tracked.add_(1)
        need = ctx.needs_input_grad
        wants = [need[4 + 4 * i] or (biases[i] is not None and need[5 + 4 * i]) for i in range(L)]
        wants_bn = [need[2 + 4 * i] or need[3 + 4 * i] for i in range(L)]
        # the lowest unit whose backward anything needs: the walk stops there
        low = 0 if need[0] else next((i for i in range(L) if wants[i] or wants_bn[i]), L)
        ctx.n = n
        ctx.meta = (kinds, strides, [bool(r) for r in relus], epoch, resync)
        ctx.gammas, ctx.weights = gammas, weights
        ctx.has_bias = [b is not None for b in biases]
        ctx.low, ctx.wants = low, wants
        ctx.save_for_backward(*(gammas + weights))   # (for autograd's check that none was modified in place since)
        # per unit from `low` up: the fp32 pre-activation and the save rows its BatchNorm's backward reads, the bf16 input
        # where a weight gradient reads it, the taps where a depthwise data gradient runs; nothing else
        ctx.sizes = sizes
        ctx.zs = [zs[i] if i >= low else None for i in range(L)]
        ctx.saves = [saves[i] if i >= low else None for i in range(L)]
        ctx.xins = [xins[i] if i >= low and wants[i] else None for i in range(L)]
        ctx.taps = [taps_of[i] if (i > low or (i == low and need[0])) else None for i in range(L)]
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        kinds, strides, relus, epoch, resync = ctx.meta
        ctx.saved_tensors
        gammas, weights, low, wants = ctx.gammas, ctx.weights, ctx.low, ctx.wants
        L = len(weights)
        n = ctx.n
        need = ctx.needs_input_grad
        grads = [None] * (4 * L)
        dx = None
        if low >= L:
            return (None, None) + tuple(grads)
        with torch.cuda.device(gy.device):
            dev = gy.device
            stream = current_stream()
            d, ld = _to_layout(gy.detach().float().contiguous(), 0)      # the fp32 gradient of the last BatchNorm's output
            for i in range(L - 1, low - 1, -1):
                wt = weights[i]
                cout, cin = wt.shape[0], (wt.shape[0] if kinds[i] == 'dw' else wt.shape[1])
                h, w, ho, wo = ctx.sizes[i]
                need_d = i > low or need[0]          # the op's data gradient
                need_g = need_d or wants[i]          # the bf16 gradient of the op's output
                z, lz = ctx.zs[i]
                ws, doubles = _bn_workspace(cout, n, ho, wo, dev)
                dgam = torch.empty(cout, dtype=torch.float32, device=dev) if need[2 + 4 * i] else None
                dbet = torch.empty(cout, dtype=torch.float32, device=dev) if need[3 + 4 * i] else None
                g = lg = None
                if need_g:
                    # through the ReLU and the BatchNorm straight into the bf16 gradient the op's backward reads, gapped for it
                    lg = _capi.Layout.padded(_up16(cout), ho, wo, 1 if kinds[i] == 'dw' else 0)
                    g = _buffer(lg, n, ho, wo, dev, True, True)
                check(lib.rtpose_bn_grad_bf16(ptr(z), C.byref(lz), ptr(d), C.byref(ld), ptr(ctx.saves[i]),
                                              ptr(gammas[i].detach().contiguous()), 1 if relus[i] else 0, ptr(g),
                                              C.byref(lg) if need_g else None, ptr(dgam), ptr(dbet), ptr(ws), doubles, cout, n,
                                              ho, wo, stream), "rtpose_bn_grad_bf16")
                grads[4 * i], grads[4 * i + 1] = dgam, dbet
                if wants[i]:
                    xin, lxin = ctx.xins[i]
                    if kinds[i] == 'dw':
                        grads[4 * i + 2] = _dw_wgrad(True, xin, lxin, g, lg, wt, cout, n, h, w, strides[i])
                    else:
                        need_b = ctx.has_bias[i] and need[5 + 4 * i]
                        dw, db = _wgrad(True, xin, lxin, g, lg, wt, cin, cout, 1, n, h, w, need_b)
                        grads[4 * i + 2] = dw if need[4 + 4 * i] else None
                        grads[4 * i + 3] = db
                if not need_d:
                    break
                # the data gradient into a dense fp32 buffer: the gy of the BatchNorm below
                if kinds[i] == 'dw':
                    d, ld = _dw_dgrad(True, g, lg, ctx.taps[i], _up8(cin), n, h, w, strides[i])
                else:
                    wp, bp = _packed_for(wt, None, 'bwd16', epoch, resync)
                    ld = _capi.Layout.dense(_up8(cin), h, w)
                    d = _buffer(ld, n, h, w, dev, False)
                    if not _unit_conv_into(True, g, lg, wp, bp, lg.cstride, cin, 1, False, n, h, w, d, ld, out_f32=1):
                        d, ld = _dgrad_fp32_fallback(g, lg, wt, n, h, w, epoch, resync)   # refused: this one conv in fp32
                if i == 0:
                    dx = _from_layout(d, ld, n, cin, h, w)
        return (dx, None) + tuple(grads)


def _unit_op(x, m, epoch, resync):
    """the op of one unit through its own bf16 node"""
    if _unit_kind(m) == 'dw':
        return dwconv3x3(x, m.weight, m.stride[0], 'bf16')
    return conv2d(x, m.weight, m.bias, False, epoch, resync, None, 'bf16')


def unit_chain(x, units, epoch=0, resync=False):
    """A run of L >= 1 units op -> BatchNorm (training mode) -> optional ReLU - a ShuffleNetV2 block's branch - as ONE
    autograd node, bf16 operands.  `units`: (``nn.Conv2d``, ``nn.BatchNorm2d`` in training mode, relu) triples; the conv is a
    pointwise one (1x1, stride 1, bias or none) or a depthwise 3x3 (padding 1, stride 1 or 2, groups = channels, no bias) on
    the channels the unit before it writes; `x` NCHW fp32 on the device.  Returns the last unit's output, NCHW fp32.  The
    BatchNorm checks are ``batch_norm``'s; `epoch` / `resync`: see ``conv2d``; the pointwise packings are the cached 'fwd16' /
    'bwd16' ones, the depthwise taps are permuted on every call as ``dwconv3x3`` does.

    Forward: x enters through one ``rtpose_nchw_to_layout_bf16``, gapped for the first op.  Per unit: the op writes a dense
    fp32 pre-activation z - ``rtpose_conv2d_bf16(out_f32 = 1)`` or ``rtpose_dwconv3x3_bf16_f32`` -, ``rtpose_bn_stats`` runs on z
    (the running statistics updated by the kernel, ``num_batches_tracked`` + 1, as ``batch_norm`` does) and
    ``rtpose_bn_apply_bf16(relu)`` writes straight into the zero-initialised bf16 buffer the next op reads: gap 1 in front of a
    depthwise conv, gap 0 in front of a pointwise one, the channels rounded up to 16.  The last unit runs ``rtpose_bn_apply``
    (fp32) and leaves through one ``rtpose_layout_to_nchw``.  Kept per unit: the bf16 input where a weight gradient reads it,
    the fp32 z and the ``save`` rows where the BatchNorm's backward runs; nothing else.
    Backward (``once_differentiable``; any ``requires_grad`` subset of x, the filters and biases, the BatchNorm weights and
    biases): gy enters once as an fp32 layout; per unit, top down, ``rtpose_bn_grad_bf16`` on the kept z writes the bf16
    gradient the op's backward reads, gapped for it, and the BatchNorm's two parameter gradients; the op's weight gradient
    is ``rtpose_conv2d_wgrad_bf16`` or ``rtpose_dwconv3x3_wgrad_bf16`` on the kept bf16 input, its data gradient
    ``rtpose_conv2d_bf16(out_f32 = 1)`` on the 'bwd16' packing or ``rtpose_dwconv3x3_dgrad_bf16`` into a dense fp32 buffer,
    the gy of the BatchNorm below.  The lowest op's data gradient leaves as NCHW fp32, only if x needs one.  The walk stops
    at the lowest unit anything needs; a parameter gradient is computed only where it is required.

    No rounding point moves against ``batch_norm(op(x, compute_dtype='bf16'), bn, relu)`` repeated L times, op being
    ``conv2d`` or ``dwconv3x3``: the output, every gradient and the running statistics are equal to that composition's bit
    for bit.

    A forward conv ``rtpose_conv2d_bf16`` refuses (before launching) makes the run give up residency: the running statistics
    the node has updated so far are put back, the run goes unit by unit through that composition - so every BatchNorm is
    updated once - and ``unit_fallbacks`` counts it.  A refused data gradient runs that one conv in fp32 on the widened
    gradient and is counted in ``bf16_fallbacks['dgrad']``."""
    global unit_fallbacks
    units = [tuple(unit) if isinstance(unit, (tuple, list)) else unit for unit in units]
    _check_units(x, units)
    epoch, resync = int(epoch), bool(resync)
    meta = (tuple(m for m, _, _ in units), tuple(bn for _, bn, _ in units), tuple(bool(r) for _, _, r in units), epoch, resync)
    try:
        return _UnitChain.apply(x, meta, *[p for m, bn, _ in units for p in (bn.weight, bn.bias, m.weight, m.bias)])
    except _UnitRefused:
        unit_fallbacks += 1
    for m, bn, relu in units:
        x = batch_norm(_unit_op(x, m, epoch, resync), bn, relu=bool(relu))
    return x


def _check_same_conv(m):
    k = m.kernel_size[0]
    if m.kernel_size != (k, k) or m.stride != (1, 1) or m.padding != (k // 2, k // 2) or m.dilation != (1, 1) or m.groups != 1:
        raise _capi.RtposeError("train: only stride-1 'same' convs have a backward here; got %r" % (m,))


def run_sequential(seq, x, epoch=0, resync=False, compute_dtype='fp32', resident=False):
    """An nn.Sequential of the RtposeVGG / OpenPose_Model trees (nn.Conv2d [+ nn.ReLU | nn.PReLU] and
    nn.MaxPool2d(2, 2, 0)): the convs through ``conv2d`` with their ReLU or PReLU fused, the pools through torch.
    `epoch` / `resync` / `compute_dtype`: see ``conv2d``.  `resident`: every maximal run of nn.Conv2d (+ nn.ReLU) goes to
    ``conv_chain`` as one node (a run of one conv to ``conv2d``); a conv with a PReLU ends a run and stays ``conv2d``'s."""
    _check_compute_dtype("train.run_sequential", compute_dtype)
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if resident and isinstance(m, nn.Conv2d):
            run = []
            while i < len(mods) and isinstance(mods[i], nn.Conv2d):
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                if isinstance(nxt, nn.PReLU):
                    break
                _check_same_conv(mods[i])
                run.append((mods[i].weight, mods[i].bias, isinstance(nxt, nn.ReLU)))
                i += 2 if isinstance(nxt, nn.ReLU) else 1
            if len(run) > 1:
                x = conv_chain(x, run, epoch, resync, compute_dtype)
                continue
            if len(run) == 1:
                x = conv2d(x, run[0][0], run[0][1], run[0][2], epoch, resync, None, compute_dtype)
                continue
            m = mods[i]     # a conv with a PReLU: below
        if isinstance(m, nn.Conv2d):
            _check_same_conv(m)
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            relu, prelu = isinstance(nxt, nn.ReLU), isinstance(nxt, nn.PReLU)
            if prelu and nxt.num_parameters != m.out_channels:
                raise _capi.RtposeError("train: a PReLU behind a conv has one slope per output channel (num_parameters = %d); "
                                        "got %r behind %r" % (m.out_channels, nxt, m))
            x = conv2d(x, m.weight, m.bias, relu, epoch, resync, nxt.weight if prelu else None, compute_dtype)
            i += 2 if relu or prelu else 1
        elif isinstance(m, nn.MaxPool2d):
            x = F.max_pool2d(x, m.kernel_size, m.stride, m.padding)
            i += 1
        elif isinstance(m, nn.ReLU):
            x = F.relu(x)
            i += 1
        else:
            raise _capi.RtposeError("train: no backward for %r" % (m,))
    return x


def _conv_block(blk, x, epoch, resync, dt):
    """openpose.ConvBlock (reference :59-62): Mconv + MPrelu as one fused conv2d"""
    return run_sequential([blk.Mconv, blk.MPrelu], x, epoch, resync, dt)


def _stage_block(st, x, epoch, resync, dt):
    """openpose.StageBlock.forward of the reference (:86-109): five dense blocks of three ConvBlocks whose outputs are
    concatenated (torch.cat), the 1x1 ConvBlock Mconv6 and the 1x1 conv Mconv7."""
    for b in range(1, 6):
        o1 = _conv_block(getattr(st, 'Mconv%d_0' % b), x, epoch, resync, dt)
        o2 = _conv_block(getattr(st, 'Mconv%d_1' % b), o1, epoch, resync, dt)
        o3 = _conv_block(getattr(st, 'Mconv%d_2' % b), o2, epoch, resync, dt)
        x = torch.cat([o1, o2, o3], 1)
    return run_sequential([st.Mconv7], _conv_block(st.Mconv6, x, epoch, resync, dt), epoch, resync, dt)


def _forward_train_vgg(model, x, epoch, resync, dt, resident=False):
    """`resident`: model0 between the pools and each of the twelve stage branches as one ``conv_chain`` node; the pools and
    the torch.cat between the stages stay torch's"""
    saved_for_loss = []
    out1 = run_sequential(model.model0, x, epoch, resync, dt, resident)
    feed = out1
    for s in range(1, 7):
        o1 = run_sequential(getattr(model, 'model%d_1' % s), feed, epoch, resync, dt, resident)
        o2 = run_sequential(getattr(model, 'model%d_2' % s), feed, epoch, resync, dt, resident)
        saved_for_loss += [o1, o2]
        if s < 6:
            feed = torch.cat([o1, o2, out1], 1)
    return (saved_for_loss[10], saved_for_loss[11]), saved_for_loss


def _dense_stage_block(st, x, epoch, resync, dt):
    """openpose.StageBlock.forward as one ``dense_stage`` node (bf16)"""
    blocks = [blk for _, blk in st.conv_blocks()]
    for blk in blocks:
        _check_same_conv(blk.Mconv)
        if blk.MPrelu.num_parameters != blk.Mconv.out_channels:
            raise _capi.RtposeError("train: a PReLU behind a conv has one slope per output channel (num_parameters = %d); "
                                    "got %r behind %r" % (blk.Mconv.out_channels, blk.MPrelu, blk.Mconv))
    _check_same_conv(st.Mconv7)
    layers = [(blk.Mconv.weight, blk.Mconv.bias, blk.MPrelu.weight) for blk in blocks]
    return dense_stage(x, layers + [(st.Mconv7.weight, st.Mconv7.bias, None)], epoch, resync)


def _forward_train_openpose(model, x, epoch, resync, dt, dense=False):
    """`dense`: every StageBlock as one ``dense_stage`` node, the ReLU runs of feature_extractor as ``conv_chain`` nodes (its
    three PReLU convs stay ``conv2d``'s); the torch.cat between the stages stays torch's"""
    stage = _dense_stage_block if dense else _stage_block
    features = run_sequential(model.feature_extractor, x, epoch, resync, dt, dense)
    paf_ret, heat_ret = [], []
    x_in = features
    for st in model.l2_stages:
        paf_pred = stage(st, x_in, epoch, resync, dt)
        x_in = torch.cat([features, paf_pred], 1)
        paf_ret.append(paf_pred)
    for st in model.l1_stages:
        heat_pred = stage(st, x_in, epoch, resync, dt)
        x_in = torch.cat([features, heat_pred, paf_pred], 1)
        heat_ret.append(heat_pred)
    return [(paf_ret[-2], heat_ret[-2]), (paf_ret[-1], heat_ret[-1])], [paf_ret, heat_ret]


# ---- the stacked hourglass (lib/network/rtpose_hourglass.py), written once over three callables ------------------------------
def hourglass_bottleneck(blk, x, conv, bn):
    """reference :26-46: bn -> relu -> conv three times, the skip (through `downsample` where the width changes) added last"""
    out = conv(bn(x, blk.bn1), blk.conv1)
    out = conv(bn(out, blk.bn2), blk.conv2)
    out = conv(bn(out, blk.bn3), blk.conv3)
    residual = conv(x, blk.downsample[0]) if blk.downsample is not None else x
    return out + residual


def _hg_chain(seq, x, conv, bn, block=None):
    for blk in seq:
        x = hourglass_bottleneck(blk, x, conv, bn) if block is None else block(blk, x)
    return x


def _hg_level(hg, n, x, conv, bn, block=None):
    """reference :74-86"""
    up1 = _hg_chain(hg[n - 1][0], x, conv, bn, block)
    low1 = _hg_chain(hg[n - 1][1], F.max_pool2d(x, 2, stride=2), conv, bn, block)
    low2 = _hg_level(hg, n - 1, low1, conv, bn, block) if n > 1 else _hg_chain(hg[n - 1][3], low1, conv, bn, block)
    low3 = _hg_chain(hg[n - 1][2], low2, conv, bn, block)
    return up1 + F.interpolate(low3, scale_factor=2)


def hourglass_forward(model, x, conv, bn, stem, block=None):
    """The reference's training-mode forward (lib/network/rtpose_hourglass.py:26-46, :74-89, :162-189) over the module
    tree of a ``HourglassNet``, with the three operations as callables: ``conv(x, m)`` an ``nn.Conv2d`` m (stride 1,
    "same"), ``bn(x, m)`` ReLU of an ``nn.BatchNorm2d`` m in training mode (every BatchNorm of this network is followed by
    one), ``stem(x, m)`` the 7x7 stride-2 ``conv1``.  Max-pool, nearest upsampling, the residual sums and the hand-over
    ``x + fc_ + paf_score_ + ht_score_`` are torch's, in the reference's order of additions.  `block`: None, or a callable
    ``block(blk, x)`` that stands for ``hourglass_bottleneck(blk, x, conv, bn)`` of every Bottleneck.  Returns
    ((score_paf, score_ht), [score_paf, score_ht]) of the last stack - the only one the reference supervises."""
    if not isinstance(model, HourglassNet):
        raise TypeError("train.hourglass_forward takes an hourglass.HourglassNet; got %s" % type(model).__name__)
    if not model.training:
        raise _capi.RtposeError("train.hourglass_forward is the training-mode forward (batch statistics): call .train() "
                                "first; fine-tuning on frozen statistics (.eval()) is out of scope")
    x = bn(stem(x, model.conv1), model.bn1)
    x = _hg_chain(model.layer1, x, conv, bn, block)
    x = F.max_pool2d(x, 2, stride=2)
    x = _hg_chain(model.layer2, x, conv, bn, block)
    x = _hg_chain(model.layer3, x, conv, bn, block)
    score_paf = score_ht = None
    for i in range(model.num_stacks):
        y = _hg_level(model.hg[i].hg, model.hg[i].depth, x, conv, bn, block)
        y = _hg_chain(model.res[i], y, conv, bn, block)
        y = bn(conv(y, model.fc[i][0]), model.fc[i][1])
        score_paf = conv(y, model.score_paf[i])
        score_ht = conv(y, model.score_ht[i])
        if i < model.num_stacks - 1:
            fc_ = conv(y, model.fc_[i])
            paf_score_ = conv(score_paf, model.paf_score_[i])
            ht_score_ = conv(score_ht, model.ht_score_[i])
            x = x + fc_ + paf_score_ + ht_score_
    return (score_paf, score_ht), [score_paf, score_ht]


def _begin_bn_forward(model, what):
    """What the forward of a network with BatchNorms does first: (epoch, resync) for its convs"""
    if not model.training:
        raise _capi.RtposeError("train.forward_train of a %s is the training-mode forward (batch statistics): call "
                                ".train() first; fine-tuning on frozen statistics (.eval()) is out of scope" % what)
    # the BatchNorm kernels write the running statistics through raw pointers (no _version bump): the inference plan,
    # which folds them, re-packs after .eval() only if the weight epoch moves
    model.invalidate_weights()
    return model._weights_epoch[0], bool(getattr(model, 'always_resync', False))


def _forward_train_hourglass(model, x, bottleneck=False):
    """`bottleneck`: every Bottleneck's main branch as one ``preact_chain`` node and every other stride-1 conv through
    ``conv2d(compute_dtype='bf16')``; the stem and the BatchNorms outside the Bottlenecks are the default's"""
    if x.requires_grad:
        raise _capi.RtposeError("train.forward_train of a HourglassNet: the stem has no data gradient; the image must not "
                                "require a gradient")
    epoch, resync = _begin_bn_forward(model, "HourglassNet")
    dt = 'bf16' if bottleneck else 'fp32'

    def conv(t, m):
        _check_same_conv(m)
        return conv2d(t, m.weight, m.bias, False, epoch, resync, None, dt)

    def block(blk, t):
        convs = (blk.conv1, blk.conv2, blk.conv3)
        for m in convs:
            _check_same_conv(m)
        out = preact_chain(t, [(b, m.weight, m.bias) for b, m in zip((blk.bn1, blk.bn2, blk.bn3), convs)], epoch, resync)
        residual = conv(t, blk.downsample[0]) if blk.downsample is not None else t
        return out + residual

    return hourglass_forward(model, x, conv, lambda t, m: batch_norm(t, m, relu=True),
                             lambda t, m: conv7x7_s2(t, m.weight, m.bias, epoch, resync), block if bottleneck else None)


# ---- ShuffleNetV2 (lib/network/rtpose_shufflenetV2.py), written once over four callables -------------------------------------------
def _channel_shuffle(x):
    n, c, h, w = x.shape
    return x.view(n, 2, c // 2, h, w).transpose(1, 2).reshape(n, c, h, w)


def shufflenet_block(blk, x, conv, bn, dw):
    """reference :31-63: conv_bn_relu 1x1, conv_bn depthwise 3x3, conv_bn_relu 1x1 on the second half of the channels (the
    first half passes through), or on all of them beside conv0 (depthwise 3x3, 1x1) where the block has one; then the
    concatenation and the shuffle of two groups"""
    def unit(t, seq, op):
        return bn(op(t, seq[0]), seq[1], len(seq) > 2)

    def branch(t):
        return unit(unit(unit(t, blk.conv[0], conv), blk.conv[1], dw), blk.conv[2], conv)

    if hasattr(blk, 'conv0'):
        x = torch.cat((unit(unit(x, blk.conv0[0], dw), blk.conv0[1], conv), branch(x)), 1)
    else:
        half = x.shape[1] // 2
        x = torch.cat((x[:, :half], branch(x[:, half:])), 1)
    return _channel_shuffle(x)


def shufflenet_forward(model, x, conv, bn, dw, stem, block=None):
    """The reference's training-mode forward (lib/network/rtpose_shufflenetV2.py:56-63, :96-104, :144-148) over the module
    tree of a ``shufflenet.Network``, with the four operations as callables: ``conv(x, m)`` a pointwise ``nn.Conv2d`` m,
    ``bn(x, m, relu)`` an ``nn.BatchNorm2d`` m in training mode followed by a ReLU if `relu`, ``dw(x, m)`` a depthwise 3x3
    ``nn.Conv2d`` m of stride 1 or 2, ``stem(x, m)`` the 3x3 stride-2 ``stage1/conv``.  The split, ``torch.cat``, the channel
    shuffle and ``MaxPool2d(3, 2, 0, ceil_mode=True)`` are torch's.  `block`: None, or a callable ``block(m, x)`` that stands
    for ``shufflenet_block(m, x, conv, bn, dw)`` of every block m and, for the conv -> BatchNorm -> ReLU ``nn.Sequential`` m in
    front of the heads, for ``bn(conv(x, m[0]), m[1], True)``.  Returns ([PAF, HEAT], [PAF, HEAT])."""
    if not isinstance(model, ShuffleNetV2):
        raise TypeError("train.shufflenet_forward takes a shufflenet.Network; got %s" % type(model).__name__)
    if not model.training:
        raise _capi.RtposeError("train.shufflenet_forward is the training-mode forward (batch statistics): call .train() "
                                "first; fine-tuning on frozen statistics (.eval()) is out of scope")
    net = model.network
    x = bn(x, net[0], False)
    x = bn(stem(x, net[1][0]), net[1][1], True)
    pool = net[2]
    x = F.max_pool2d(x, pool.kernel_size, pool.stride, pool.padding, ceil_mode=pool.ceil_mode)
    for stage in (net[3], net[4], net[5]):
        for blk in stage:
            x = shufflenet_block(blk, x, conv, bn, dw) if block is None else block(blk, x)
    x = bn(conv(x, net[6][0]), net[6][1], True) if block is None else block(net[6], x)
    paf = conv(x, model.paf)
    heat = conv(x, model.heatmap)
    return [paf, heat], [paf, heat]


def _forward_train_shufflenet(model, x, branch=False):
    """`branch`: the conv branches of every block and the conv -> BatchNorm -> ReLU in front of the heads as ``unit_chain``
    nodes, the two heads through ``conv2d(compute_dtype='bf16')``; ``data/bn``, the stem and its BatchNorm are the default's"""
    epoch, resync = _begin_bn_forward(model, "shufflenet.Network")
    dt = 'bf16' if branch else 'fp32'

    def conv(t, m):
        if m.kernel_size != (1, 1) or m.stride != (1, 1) or m.padding != (0, 0) or m.dilation != (1, 1) or m.groups != 1:
            raise _capi.RtposeError("train: a pointwise conv of the ShuffleNetV2 tree is 1x1, stride 1; got %r" % (m,))
        return conv2d(t, m.weight, m.bias, False, epoch, resync, None, dt)

    def units(*seqs):
        return [(seq[0], seq[1], len(seq) > 2) for seq in seqs]

    def block(m, t):
        if not hasattr(m, 'conv'):       # the conv -> BatchNorm -> ReLU in front of the heads
            return unit_chain(t, units(m), epoch, resync)
        if hasattr(m, 'conv0'):
            t = torch.cat((unit_chain(t, units(*m.conv0), epoch, resync), unit_chain(t, units(*m.conv), epoch, resync)), 1)
        else:
            half = t.shape[1] // 2
            t = torch.cat((t[:, :half], unit_chain(t[:, half:], units(*m.conv), epoch, resync)), 1)
        return _channel_shuffle(t)

    def dw(t, m):
        s = m.stride[0]
        if (m.kernel_size != (3, 3) or m.stride != (s, s) or m.padding != (1, 1) or m.dilation != (1, 1)
                or m.groups != m.in_channels or m.out_channels != m.in_channels or m.bias is not None):
            raise _capi.RtposeError("train: a depthwise conv of the ShuffleNetV2 tree is 3x3, padding 1, groups = channels, "
                                    "without a bias; got %r" % (m,))
        return dwconv3x3(t, m.weight, s)

    def stem(t, m):
        if m.kernel_size != (3, 3) or m.stride != (2, 2) or m.padding != (1, 1) or m.dilation != (1, 1) or m.bias is not None:
            raise _capi.RtposeError("train: the ShuffleNetV2 stem is nn.Conv2d(3, 24, 3, 2, 1, bias=False); got %r" % (m,))
        return conv3x3_s2(t, m.weight, epoch, resync)

    return shufflenet_forward(model, x, conv, lambda t, m, relu: batch_norm(t, m, relu=relu), dw, stem,
                              block if branch else None)


def _model_kind(model, who):
    if isinstance(model, RtposeVGG):
        return 'vgg'
    if isinstance(model, OpenPose_Model):
        return 'openpose'
    if isinstance(model, HourglassNet):
        return 'hourglass'
    if isinstance(model, ShuffleNetV2):
        return 'shufflenet'
    raise TypeError("%s takes a network.RtposeVGG, an openpose.OpenPose_Model, an hourglass.HourglassNet or a "
                    "shufflenet.Network; got %s" % (who, type(model).__name__))


# why forward_train(resident=True) refuses the networks that are not an RtposeVGG
_NOT_RESIDENT = {
    'openpose': "an openpose.OpenPose_Model's PReLU needs the fp32 pre-activation of every conv, and its dense blocks give an "
                "activation two consumers, whose gradients would have to be summed in the layouts (conv_chain runs convs with "
                "one consumer and a ReLU or no activation)",
    'hourglass': "a HourglassNet trains through BatchNorm kernels between its convs and residual sums, which are fp32 passes "
                 "on NCHW tensors at the autograd boundary (conv_chain runs convs with one consumer and a ReLU or no "
                 "activation)",
    'shufflenet': "a shufflenet.Network trains through BatchNorm and depthwise kernels between its convs, which are fp32 "
                  "passes on NCHW tensors at the autograd boundary (conv_chain runs convs with one consumer and a ReLU or no "
                  "activation)",
}


# why forward_train(resident='dense') refuses the networks that are not an OpenPose_Model
_NOT_DENSE = {
    'vgg': "a network.RtposeVGG has no dense blocks and no PReLU: its runs of convs are conv_chain's (resident=True)",
    'hourglass': _NOT_RESIDENT['hourglass'].replace("conv_chain runs convs with one consumer and a ReLU or no activation",
                                                    "dense_stage runs the dense blocks of an openpose.StageBlock"),
    'shufflenet': _NOT_RESIDENT['shufflenet'].replace("conv_chain runs convs with one consumer and a ReLU or no activation",
                                                      "dense_stage runs the dense blocks of an openpose.StageBlock"),
}


def _check_resident(who, resident):
    """`resident` is False, True or 'dense': whether it is 'dense'"""
    if isinstance(resident, str):
        if resident == 'dense':
            return True
    elif resident in (False, True):
        return False
    raise _capi.RtposeError("%s: resident is False, True or 'dense'; got %r ('bottleneck' is forward_train's and train_step's "
                            "fourth value, for an hourglass.HourglassNet, and 'branch' their fifth, for a shufflenet.Network)"
                            % (who, resident))


def forward_train(model, x, compute_dtype='fp32', resident=False):
    """The reference's forward over the module tree of `model`, with an autograd graph behind the outputs.
    `compute_dtype`: 'fp32', or 'bf16' (``conv2d``) for an ``RtposeVGG`` or an ``OpenPose_Model``; refused for the other two,
    whose BatchNorm and depthwise kernels are fp32.
    `resident`: True, for an ``RtposeVGG`` only - every run of convs between two pools of model0 and each stage branch is one
    ``conv_chain`` node whose inner activations and gradients stay in the layouts; refused for the other three (why: the
    message).  'dense', for an ``OpenPose_Model`` with ``compute_dtype='bf16'`` only - every ``StageBlock`` is one
    ``dense_stage`` node, feature_extractor runs as under ``run_sequential(resident=True)``; refused for the other three
    and for 'fp32'.  'bottleneck', for a ``HourglassNet`` in training mode with ``compute_dtype='bf16'`` only - the main
    branch of every Bottleneck is one ``preact_chain`` node, ``downsample``, ``fc``, the score heads and the hand-over convs
    run through ``conv2d(compute_dtype='bf16')``, ``bn1`` and the BatchNorm of ``fc`` through ``batch_norm``, the stem through
    ``conv7x7_s2`` (fp32); refused for the other three and for 'fp32'.  Without it a ``HourglassNet`` takes no 'bf16'.
    'branch', for a ``shufflenet.Network`` in training mode with ``compute_dtype='bf16'`` only - the three-unit ``conv`` branch
    of every block, the two-unit ``conv0`` of a downsampling block and the conv -> BatchNorm -> ReLU in front of the heads are
    one ``unit_chain`` node each, the two heads run through ``conv2d(compute_dtype='bf16')``, ``data/bn`` and the stem's
    BatchNorm through ``batch_norm``, the stem through ``conv3x3_s2`` (fp32), and the split, ``torch.cat``, the channel shuffle
    and the max-pool stay torch's; refused for the other three, for 'fp32', for a network in ``.eval()`` mode and for a CPU
    tensor.  Without it a ``shufflenet.Network`` takes no 'bf16'.  Any other value is refused.  The default False is the
    per-conv path, launch for launch.
    ``RtposeVGG`` (lib/network/rtpose_vgg.py:158-198): ((out6_1, out6_2), saved_for_loss[12]).
    ``OpenPose_Model`` (lib/network/openpose.py:86-109, :160-177):
    ([(paf[-2], heat[-2]), (paf[-1], heat[-1])], [paf_ret, heat_ret]).
    ``HourglassNet`` in training mode (``hourglass_forward`` with ``conv2d``, ``batch_norm(relu=True)`` and ``conv7x7_s2``):
    ((score_paf, score_ht), [score_paf, score_ht]) of the last stack; every BatchNorm's running statistics are updated and
    ``model.invalidate_weights()`` is called once.
    ``shufflenet.Network`` in training mode (``shufflenet_forward`` with ``conv2d``, ``batch_norm``, ``dwconv3x3`` and
    ``conv3x3_s2``): ([PAF, HEAT], [PAF, HEAT]); running statistics and ``invalidate_weights()`` as for the hourglass."""
    _check_compute_dtype("train.forward_train", compute_dtype)
    kind = _model_kind(model, "train.forward_train")
    if isinstance(resident, str) and resident == 'bottleneck':
        if kind != 'hourglass':
            raise _capi.RtposeError("train.forward_train: resident='bottleneck' is for an hourglass.HourglassNet only: "
                                    "preact_chain runs the BatchNorm -> ReLU -> conv triples of its pre-activation Bottlenecks, "
                                    "and a %s has none" % type(model).__name__)
        if compute_dtype != 'bf16':
            raise _capi.RtposeError("train.forward_train: resident='bottleneck' needs compute_dtype='bf16': preact_chain keeps "
                                    "bf16 activations and gradients in the layouts, and an fp32 node is not built; got "
                                    "compute_dtype=%r" % (compute_dtype,))
        if not x.is_cuda:
            raise _capi.RtposeError("train.forward_train runs only on an MI355X (HIP) device tensor; got a %s tensor - there "
                                    "is deliberately no CPU fallback" % (x.device,))
        return _forward_train_hourglass(model, x, True)
    if isinstance(resident, str) and resident == 'branch':
        if kind != 'shufflenet':
            raise _capi.RtposeError("train.forward_train: resident='branch' is for a shufflenet.Network only: unit_chain runs the "
                                    "conv -> BatchNorm (-> ReLU) units of its blocks' branches, pointwise and depthwise, and a "
                                    "%s has none" % type(model).__name__)
        if compute_dtype != 'bf16':
            raise _capi.RtposeError("train.forward_train: resident='branch' needs compute_dtype='bf16': unit_chain keeps bf16 "
                                    "activations and gradients in the layouts, and an fp32 node is not built; got "
                                    "compute_dtype=%r" % (compute_dtype,))
        if not model.training:
            raise _capi.RtposeError("train.forward_train: resident='branch' is the training-mode forward (batch statistics): "
                                    "call .train() first; fine-tuning on frozen statistics (.eval()) is out of scope")
        if not x.is_cuda:
            raise _capi.RtposeError("train.forward_train runs only on an MI355X (HIP) device tensor; got a %s tensor - there "
                                    "is deliberately no CPU fallback" % (x.device,))
        return _forward_train_shufflenet(model, x, True)
    if compute_dtype != 'fp32' and kind in ('hourglass', 'shufflenet'):
        raise _capi.RtposeError("train.forward_train: compute_dtype=%r is for a network.RtposeVGG or an openpose.OpenPose_Model; "
                                "the BatchNorm%s kernels a %s trains through are fp32 and take no compute dtype"
                                % (compute_dtype, " and depthwise" if kind == 'shufflenet' else "", type(model).__name__))
    dense = _check_resident("train.forward_train", resident)
    if dense:
        if kind != 'openpose':
            raise _capi.RtposeError("train.forward_train: resident='dense' is for an openpose.OpenPose_Model only; "
                                    + _NOT_DENSE[kind])
        if compute_dtype != 'bf16':
            raise _capi.RtposeError("train.forward_train: resident='dense' needs compute_dtype='bf16': dense_stage keeps bf16 "
                                    "activations and gradients in the layouts, and an fp32 node is not built; got "
                                    "compute_dtype=%r" % (compute_dtype,))
    elif resident and kind != 'vgg':
        raise _capi.RtposeError("train.forward_train: resident=True is for a network.RtposeVGG only; " + _NOT_RESIDENT[kind])
    if not x.is_cuda:
        raise _capi.RtposeError("train.forward_train runs only on an MI355X (HIP) device tensor; got a %s tensor - there is "
                                "deliberately no CPU fallback" % (x.device,))
    # the contract of _native_state.py: invalidate_weights() (the epoch) and always_resync decide a re-pack here as well
    if kind == 'hourglass':
        return _forward_train_hourglass(model, x)
    if kind == 'shufflenet':
        return _forward_train_shufflenet(model, x)
    epoch, resync = getattr(model, '_weights_epoch', [0])[0], bool(getattr(model, 'always_resync', False))
    if kind == 'vgg':
        return _forward_train_vgg(model, x, epoch, resync, compute_dtype, bool(resident))
    return _forward_train_openpose(model, x, epoch, resync, compute_dtype, dense)


def freeze_trunk(model, n=20):
    """train/train_VGG19.py:305-307: the parameters of the first `n` modules of model0 - of feature_extractor for an
    OpenPose_Model - (conv1_1 .. conv4_1, nine convs) stop training."""
    kind = _model_kind(model, "train.freeze_trunk")
    if kind == 'hourglass':
        raise TypeError("train.freeze_trunk: the reference freezes nothing of a HourglassNet (train/train_SH.py); it takes a "
                        "network.RtposeVGG or an openpose.OpenPose_Model")
    if kind == 'shufflenet':
        raise TypeError("train.freeze_trunk: the reference freezes nothing of a shufflenet.Network "
                        "(train/train_ShuffleNetV2.py); it takes a network.RtposeVGG or an openpose.OpenPose_Model")
    trunk = model.model0 if kind == 'vgg' else model.feature_extractor
    for i in range(n):
        for p in trunk[i].parameters():
            p.requires_grad = False
    return model


def train_step(model, optimizer, image, heat, paf, heat_mask=None, paf_mask=None, compute_dtype='fp32', resident=False):
    """One iteration of train/train_VGG19.py:206-217: (total_loss, saved_for_log).  The loss is ``encode.get_loss`` for an
    RtposeVGG, ``encode.get_loss_openpose`` for an OpenPose_Model and, for a HourglassNet (train/train_SH.py:160-172),
    ``encode.get_loss_hourglass`` with the optional `heat_mask` / `paf_mask` (None: ones), for a shufflenet.Network
    (train/train_ShuffleNetV2.py:144-156) ``encode.get_loss_shufflenet`` with the same masks; the masks belong to those two
    losses only.  `compute_dtype` / `resident` (False, True, 'dense', 'bottleneck' or 'branch'): see ``forward_train``; the
    optimizer steps the fp32 parameters either way."""
    _check_compute_dtype("train.train_step", compute_dtype)
    kind = _model_kind(model, "train.train_step")
    if kind not in ('hourglass', 'shufflenet') and (heat_mask is not None or paf_mask is not None):
        raise TypeError("train.train_step: heat_mask / paf_mask belong to the HourglassNet and shufflenet.Network losses "
                        "(encode.get_loss_hourglass, encode.get_loss_shufflenet)")
    _, saved_for_loss = forward_train(model, image, compute_dtype, resident)
    if kind == 'hourglass':
        total_loss, saved_for_log = encode.get_loss_hourglass(saved_for_loss, heat, heat_mask, paf, paf_mask)
    elif kind == 'shufflenet':
        total_loss, saved_for_log = encode.get_loss_shufflenet(saved_for_loss, heat, heat_mask, paf, paf_mask)
    else:
        total_loss, saved_for_log = (encode.get_loss if kind == 'vgg' else encode.get_loss_openpose)(saved_for_loss, heat, paf)
    optimizer.zero_grad()
    total_loss.backward()
    optimizer.step()
    return total_loss, saved_for_log
