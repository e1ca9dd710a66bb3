"""People -> heat-map / PAF targets on the device, and the reference's stage losses (csrc/encode.hip, header section 4b).

The way back from the decoder: ``encode_targets`` is lib/datasets/datasets.py:259-308 (``get_ground_truth`` with
``putGaussianMaps`` / ``putVecMaps``) for any ``skeleton.Skeleton`` and a batch of images, ``get_loss`` is
train/train_VGG19.py:143-174 and ``stage_losses`` computes its twelve terms from a native forward without converting a map
to NCHW (``rtpose_stage_mse`` reads the plan's own views; only the four max / min entries of the log are taken from NCHW
copies of the last two stage outputs).

Reference-exact: every decision of the encoder (``e <= 4.6052``, ``|cross| < 1``, the half-even limb box), the PAF values
bit for bit, the heat values within 1 fp32 ulp (``exp``).  Not the reference's: ``np.linalg.norm`` may use a fused
multiply-add inside BLAS's ``dot``, the limb norm here is the unfused ``sqrt(vx * vx + vy * vy)``.

``get_loss_hourglass`` and ``get_loss_shufflenet`` are the masked losses of train/train_SH.py and
train/train_ShuffleNetV2.py.  ``stage_losses`` covers ``network.RtposeVGG`` only (OpenPose_Model and the hourglass return other numbers of stage
outputs); ``get_loss_openpose`` is the loss of an ``openpose.OpenPose_Model`` in torch, as ``get_loss`` is for rtpose_vgg
(train.train_step picks between them); ``encode_targets`` takes any skeleton and any stride, 4 included.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _capi
from ._capi import check, current_stream, lib, ptr
from .skeleton import Skeleton

# lib/datasets/datasets.py:37-61 (get_keypoints) and :13-35 (kp_connections): limb i in PAF channels (2 i, 2 i + 1)
_TRAIN_PAIRS = [(1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 2), (2, 3), (3, 4), (2, 14), (1, 5), (5, 6),
                (6, 7), (5, 15), (1, 0), (0, 14), (0, 15), (14, 16), (15, 17)]
COCO18_TRAIN = Skeleton(
    "COCO18_TRAIN",
    ["Nose", "Neck", "RShoulder", "RElbow", "RWrist", "LShoulder", "LElbow", "LWrist", "RHip", "RKnee", "RAnkle", "LHip",
     "LKnee", "LAnkle", "REye", "LEye", "REar", "LEar"],
    [(a, b, 2 * i, 2 * i + 1) for i, (a, b) in enumerate(_TRAIN_PAIRS)])
COCO18_TRAIN.__doc__ = (
    "The reference's TRAINING table: kp_connections over get_keypoints() (lib/datasets/datasets.py:13-61), limb i in PAF "
    "channels (2 i, 2 i + 1).  It differs from the decoder's preset skeleton.COCO18 (lib/pafprocess/pafprocess.h) in two "
    "limbs: training joins shoulder to EYE (datasets.py:24, :28: RShoulder-REye in channels 18 / 19, LShoulder-LEye in "
    "26 / 27) where the decoder joins shoulder to EAR on the same channels.  encode_targets encodes with whichever table "
    "the caller passes; use skeleton.COCO18 for maps the decoder is to read back.")

# Row of the COCO-17 annotation behind each of this work's 18 parts (datasets.py:241-242); the neck has none
_NECK = 1
_FROM_COCO17 = {0: 0, 2: 6, 3: 8, 4: 10, 5: 5, 6: 7, 7: 9, 8: 12, 9: 14, 10: 16, 11: 11, 12: 13, 13: 15, 14: 2, 15: 1,
                16: 4, 17: 3}
_COCO17_LSHOULDER, _COCO17_RSHOULDER = 5, 6


def add_neck(keypoints17, dtype=np.float64):
    """lib/datasets/datasets.py:227-257: (17, 3) COCO keypoints (x, y, v) -> (18, 3) float64 in this work's order, with
    the neck midway between the shoulders: v = 2 if both shoulders have v == 2, else the product of their v; the neck
    row alone goes through np.round (half to even).  ``dtype=None`` keeps a floating-point input's own dtype, as the
    reference does: the float32 keypoints of its loader get a neck computed in float32 (augment.train_batch)."""
    coco = np.asarray(keypoints17, dtype=dtype).reshape(17, 3)
    if not np.issubdtype(coco.dtype, np.floating):
        coco = coco.astype(np.float64)
    out = np.empty((18, 3), coco.dtype)
    for part, row in _FROM_COCO17.items():
        out[part] = coco[row]
    ls, rs = coco[_COCO17_LSHOULDER], coco[_COCO17_RSHOULDER]
    both_labelled_visible = rs[2] == 2 and ls[2] == 2
    out[_NECK, :2] = np.round((rs[:2] + ls[:2]) / 2)
    out[_NECK, 2] = np.round(2.0 if both_labelled_visible else rs[2] * ls[2])
    return out


def pack_people(people, num_parts, counts=None):
    """-> (float64 [N, K, P, 3], int32 [N]) from a list per image of (P, 3) arrays (or one (k, P, 3) array per image),
    or from a padded [N, K, P, 3] array plus counts (None = K everywhere).  K is at least 1."""
    if isinstance(people, np.ndarray) and people.ndim == 4:
        kp = np.ascontiguousarray(people, dtype=np.float64)
        n, k = kp.shape[:2]
        cnt = np.full(n, k, np.int32) if counts is None else np.asarray(counts, np.int32).reshape(n)
    else:
        if counts is not None:
            raise ValueError("counts go with a padded [N, K, P, 3] array")
        per = [np.asarray(p, np.float64).reshape(-1, num_parts, 3) for p in people]
        cnt = np.array([p.shape[0] for p in per], np.int32)
        kp = np.zeros((len(per), max(1, int(cnt.max()) if len(per) else 1), num_parts, 3), np.float64)
        for i, p in enumerate(per):
            kp[i, :p.shape[0]] = p
    if kp.shape[2:] != (num_parts, 3):
        raise ValueError("people of %s parts x 3 for a skeleton of %d parts" % (kp.shape[2:], num_parts))
    if kp.shape[1] == 0:
        kp = np.zeros((kp.shape[0], 1, num_parts, 3), np.float64)
    return kp, np.ascontiguousarray(cnt)


def encode_enqueue(kp, counts, cfg, skel, heat, paf, workspace):
    """Enqueue the two encoder launches on the current stream: kp fp64 [N, K, P, 3] and counts int32 [N] (or None)
    device tensors, heat / paf dense NHWC fp32 destinations, workspace a device tensor of
    rtpose_encode_workspace_bytes."""
    check(lib.rtpose_encode_targets_skel(ptr(kp), ptr(counts), kp.shape[0], kp.shape[1], C.byref(cfg), C.byref(skel),
                                         heat.shape[3], paf.shape[3], ptr(heat), ptr(paf), ptr(workspace),
                                         workspace.numel() * workspace.element_size(), current_stream()),
          "rtpose_encode_targets_skel")


def encode_targets(people, skeleton=COCO18_TRAIN, input_size=(368, 368), stride=8, sigma=7.0, device=None, counts=None):
    """Targets of a batch: ``people`` is a list per image of (P, 3) arrays of (x, y, v) in input pixels - or a padded
    [N, K, P, 3] array with ``counts`` -, ``input_size`` is (height, width) of the network input (the reference's
    input_y, input_x).  Returns (heat [N, C_h, h, w], paf [N, C_p, h, w]) fp32 tensors on ``device`` (default: the
    current HIP device): NCHW *views* of the dense NHWC buffers the kernel wrote - the reference's
    ``transpose((2, 0, 1))`` without a copy.  C_h / C_p are the skeleton's heat_channels / paf_channels; the background
    channel is written iff the skeleton has one.  People are summed in list order."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise _capi.RtposeError("encode_targets runs on an MI355X (HIP) device only (no CPU fallback); got %s" % device)
    kp, cnt = pack_people(people, skeleton.num_parts, counts)
    n = kp.shape[0]
    ih, iw = int(input_size[0]), int(input_size[1])
    cfg = _capi.EncodeCfg.make(ih, iw, int(stride), float(sigma), skeleton.background)
    skel = skeleton.native()
    h, w = ih // int(stride), iw // int(stride)
    with torch.cuda.device(device):
        heat = torch.empty((n, max(h, 0), max(w, 0), skeleton.heat_channels), dtype=torch.float32, device=device)
        paf = torch.empty((n, max(h, 0), max(w, 0), skeleton.paf_channels), dtype=torch.float32, device=device)
        wb = lib.rtpose_encode_workspace_bytes(C.byref(cfg), C.byref(skel), n, kp.shape[1])
        if wb == 0:
            raise _capi.RtposeError("bad encode arguments: " + _capi.last_error())
        workspace = torch.empty(wb // 8, dtype=torch.float64, device=device)
        encode_enqueue(torch.from_numpy(kp).to(device), torch.from_numpy(cnt).to(device), cfg, skel, heat, paf, workspace)
    return heat.permute(0, 3, 1, 2), paf.permute(0, 3, 1, 2)


def build_names():
    """train/train_VGG19.py:134-140."""
    return ['loss_stage%d_L%d' % (j, k) for j in range(1, 7) for k in range(1, 3)]


def get_loss(saved_for_loss, heat_temp, vec_temp):
    """train/train_VGG19.py:143-174 with the reference's signature, in torch on whatever device the tensors live on:
    (total_loss, saved_for_log) - the twelve nn.MSELoss(reduction='mean') terms (PAF stages against ``vec_temp``,
    heat-map stages against ``heat_temp``) under the names of build_names(), plus max_ht / min_ht (the last heat map
    without its background channel) and max_paf / min_paf."""
    if len(saved_for_loss) != 12:
        raise ValueError("get_loss wants the 12 stage outputs of rtpose_vgg, got %d" % len(saved_for_loss))
    targets = (vec_temp, heat_temp)
    terms = [torch.nn.functional.mse_loss(out, targets[i % 2]) for i, out in enumerate(saved_for_loss)]
    log = OrderedDict(zip(build_names(), (t.item() for t in terms)))
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    log.update(_extremes(saved_for_loss[11].detach(), saved_for_loss[10].detach()))
    return total, log


def get_loss_openpose(saved_for_loss, heat_temp, vec_temp):
    """The loss of an ``openpose.OpenPose_Model`` from its ``saved_for_loss = [paf_ret, heat_ret]``.  The reference ships
    no training script for this network, so this is the project's definition, after get_loss: one
    nn.MSELoss(reduction='mean') per PAF stage against ``vec_temp`` and per heat stage against ``heat_temp``, added in the
    order PAF stages then heat stages.  (total_loss, saved_for_log): the terms under ``loss_paf_stage%d`` /
    ``loss_heat_stage%d`` (1-based), plus max_ht / min_ht / max_paf / min_paf of the last heat map and the last PAF."""
    if (not isinstance(saved_for_loss, (list, tuple)) or len(saved_for_loss) != 2
            or not all(isinstance(s, (list, tuple)) and len(s) >= 1 for s in saved_for_loss)):
        raise ValueError("get_loss_openpose wants [paf_ret, heat_ret], two non-empty lists of stage outputs")
    paf_ret, heat_ret = saved_for_loss
    names = ['loss_paf_stage%d' % (i + 1) for i in range(len(paf_ret))] \
        + ['loss_heat_stage%d' % (i + 1) for i in range(len(heat_ret))]
    terms = [torch.nn.functional.mse_loss(out, vec_temp) for out in paf_ret] \
        + [torch.nn.functional.mse_loss(out, heat_temp) for out in heat_ret]
    log = OrderedDict(zip(names, (t.item() for t in terms)))
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    log.update(_extremes(heat_ret[-1].detach(), paf_ret[-1].detach()))
    return total, log


def get_loss_hourglass(saved_for_loss, heat_temp, heat_weight, vec_temp, vec_weight):
    """train/train_SH.py:80-126 with the reference's signature: ``saved_for_loss = [score_paf, score_ht]`` of the last
    stack, the masked sum of squares of each over ``2 * batch_size`` (nn.MSELoss(size_average=False) of pred * weight
    against target * weight), PAF term then heat-map term.  (total_loss, saved_for_log) with the reference's keys 'paf',
    'heatmap', max_ht / min_ht (without the background channel), max_paf / min_paf.  A weight of None means ones: the
    multiplications are left out."""
    if not isinstance(saved_for_loss, (list, tuple)) or len(saved_for_loss) != 2:
        raise ValueError("get_loss_hourglass wants [score_paf, score_ht] of the last stack")
    batch_size = heat_temp.size(0)
    pred1 = saved_for_loss[0] if vec_weight is None else saved_for_loss[0] * vec_weight
    gt1 = vec_temp if vec_weight is None else vec_temp * vec_weight
    pred2 = saved_for_loss[1] if heat_weight is None else saved_for_loss[1] * heat_weight
    gt2 = heat_temp if heat_weight is None else heat_weight * heat_temp
    loss1 = torch.nn.functional.mse_loss(pred1, gt1, reduction='sum') / (2 * batch_size)
    loss2 = torch.nn.functional.mse_loss(pred2, gt2, reduction='sum') / (2 * batch_size)
    total = 0 + loss1
    total = total + loss2
    log = OrderedDict([('paf', loss1.item()), ('heatmap', loss2.item())])
    log.update(_extremes(saved_for_loss[-1].detach(), saved_for_loss[-2].detach()))
    return total, log


def get_loss_shufflenet(saved_for_loss, heat_temp, heat_weight, vec_temp, vec_weight):
    """train/train_ShuffleNetV2.py:77-123 with the reference's signature: ``saved_for_loss = [PAF, HEAT]``, the MEAN of the
    masked squares of each (nn.MSELoss(size_average=True) of pred * weight against target * weight), PAF term then
    heat-map term.  (total_loss, saved_for_log) with the reference's keys 'paf', 'heatmap', max_ht / min_ht (without the
    background channel), max_paf / min_paf.  A weight of None means ones: the multiplications are left out."""
    if not isinstance(saved_for_loss, (list, tuple)) or len(saved_for_loss) != 2:
        raise ValueError("get_loss_shufflenet wants [PAF, HEAT], the two outputs of the network")
    pred1 = saved_for_loss[0] if vec_weight is None else saved_for_loss[0] * vec_weight
    gt1 = vec_temp if vec_weight is None else vec_temp * vec_weight
    pred2 = saved_for_loss[1] if heat_weight is None else saved_for_loss[1] * heat_weight
    gt2 = heat_temp if heat_weight is None else heat_weight * heat_temp
    loss1 = torch.nn.functional.mse_loss(pred1, gt1)
    loss2 = torch.nn.functional.mse_loss(pred2, gt2)
    total = 0 + loss1
    total = total + loss2
    log = OrderedDict([('paf', loss1.item()), ('heatmap', loss2.item())])
    log.update(_extremes(saved_for_loss[-1].detach(), saved_for_loss[-2].detach()))
    return total, log


def _extremes(last_heat, last_paf):
    """The four range entries of saved_for_log: the last heat map without its background channel, the last PAF."""
    parts = last_heat[:, :last_heat.shape[1] - 1]
    return OrderedDict([('max_ht', parts.amax().item()), ('min_ht', parts.amin().item()),
                        ('max_paf', last_paf.amax().item()), ('min_paf', last_paf.amin().item())])


def stage_view(plan, which):
    """(base pointer, Layout, C, H, W) of stage output ``which`` (saved_for_loss order) of a plan, in place."""
    base = C.c_void_p()
    lay = _capi.Layout()
    c, h, w = C.c_int(), C.c_int(), C.c_int()
    check(lib.rtpose_net_stage_view(plan.handle, which, C.byref(base), C.byref(lay), C.byref(c), C.byref(h), C.byref(w)),
          "rtpose_net_stage_view")
    return base, lay, c.value, h.value, w.value


def _dense_nhwc(t, what):
    """[N, C, h, w] target -> its dense NHWC form (no copy for what encode_targets returned)."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError("%s must be an fp32 [N, C, h, w] tensor" % what)
    return t.permute(0, 2, 3, 1).contiguous()


def stage_mse_enqueue(plan, heat_nhwc, paf_nhwc, losses, partials):
    """The twelve rtpose_stage_mse calls on the plan's stage views, on the current stream: losses[2 j] = PAF stage j + 1
    against paf_nhwc, losses[2 j + 1] = heat-map stage j + 1 against heat_nhwc (dense NHWC fp32), losses a device
    fp32 [12], partials a device fp64 workspace.  The forward must have run with keep_intermediates."""
    n = plan.shape[0]
    for which in range(12):
        base, lay, c, h, w = stage_view(plan, which)
        tgt = paf_nhwc if which % 2 == 0 else heat_nhwc
        if tuple(tgt.shape) != (n, h, w, c):
            raise ValueError("stage output %d is [%d, %d, %d, %d] (NHWC), its target %s"
                             % (which, n, h, w, c, tuple(tgt.shape)))
        check(lib.rtpose_stage_mse(base, C.byref(lay), ptr(tgt), n, h, w, c, ptr(partials), partials.numel(),
                                   C.c_void_p(losses.data_ptr() + 4 * which), current_stream()), "rtpose_stage_mse")


def stage_losses(model, x, heat, paf):
    """get_loss over a native forward: runs ``model.forward_native(x, keep_intermediates=True)`` and the twelve
    ``rtpose_stage_mse`` reductions on the plan's own padded-NHWC views, all on the current stream.  ``heat`` / ``paf``
    are the targets as [N, C, h, w] fp32 device tensors (what encode_targets returns).  Returns (total_loss,
    saved_for_log) like get_loss: total_loss a 0-dim fp32 device tensor, the terms added in the reference's order.
    The twelve terms convert nothing to NCHW; max_ht / min_ht / max_paf / min_paf come from ``read_output`` copies of
    stage outputs 10 and 11.
    ``network.RtposeVGG`` only."""
    from .network import RtposeVGG
    if not isinstance(model, RtposeVGG):
        raise TypeError("stage_losses covers network.RtposeVGG only (12 stage outputs); got %s" % type(model).__name__)
    with torch.cuda.device(x.device):
        heat_nhwc = _dense_nhwc(heat.to(x.device), "heat")
        paf_nhwc = _dense_nhwc(paf.to(x.device), "paf")
        plan = model.forward_native(x, keep_intermediates=True)
        n, h3, w3 = plan.shape[0], plan.h3, plan.w3
        need = max(lib.rtpose_stage_mse_partials(n, h3, w3, 38), lib.rtpose_stage_mse_partials(n, h3, w3, 19))
        partials = torch.empty(max(int(need), 1), dtype=torch.float64, device=x.device)
        losses = torch.empty(12, dtype=torch.float32, device=x.device)
        stage_mse_enqueue(plan, heat_nhwc, paf_nhwc, losses, partials)
        total_loss = losses[0]
        for i in range(1, 12):
            total_loss = total_loss + losses[i]
        host = losses.cpu()
        saved_for_log = OrderedDict((nm, host[i].item()) for i, nm in enumerate(build_names()))
        # the four range entries are no loss terms: they are read from NCHW copies of the last two stage outputs
        saved_for_log.update(_extremes(model.read_output(plan, 11), model.read_output(plan, 10)))
    return total_loss, saved_for_log
