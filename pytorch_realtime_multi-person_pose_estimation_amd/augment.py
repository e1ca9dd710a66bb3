"""Training batches augmented on the device: flip, rescale, crop, pad, normalise, mask (csrc/augment.hip, header 4c).

What ``CocoKeypoints.__getitem__`` of the reference does before it yields ``(image, heatmaps, pafs)``
(lib/datasets/datasets.py:156-214): the preprocess chain of train/train_VGG19.py:124-130 - ``Normalize``,
``RandomApply(HFlip, 0.5)``, ``RescaleRelative()``, ``Crop(368)``, ``CenterPad(368)`` of lib/datasets/transforms.py -,
then ``image_transform`` (``ToTensor`` + ImageNet ``Normalize``), ``utils.mask_valid_area`` and ``get_ground_truth``.

The split: the random draws (``draw_params``, torch's global generator in the reference's order) and the annotation
bookkeeping (``transform_annotations``, numpy in the reference's dtypes) are host work of a few microseconds per image;
the pixels - a PIL bicubic resize per image in the reference - are one table launch and one fused launch per batch
(``augment_images``), and the targets are ``encode.encode_targets``.  ``train_batch`` is the whole item pipeline for a
batch.  The image is the reference's bits (Pillow's two integer passes restated on the device), the keypoints are its
bits including their dtype (float32 until a flip makes them float64), the targets follow encode.py's contract.

Out of scope: ``image_transform_train``'s ``ColorJitter``, JPEG re-compression and ``RandomGrayscale`` (random and
photometric, torchvision); ``RandomRotate`` (cv2 ``warpAffine``; not in the training script's chain);
``RescaleAbsolute`` / ``MultiScale``; image decoding; the DataLoader.
"""
import copy
import ctypes as C
import math

import numpy as np
import torch

from . import _capi, encode
from ._capi import check, current_stream, lib, ptr

FILL = (124, 116, 104)          # CenterPad's fill (transforms.py:352-353)

# lib/datasets/coco.py:3-41: the row a COCO-17 keypoint moves to under horizontal_swap_coco
_HFLIP_TARGET = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def draw_params(sizes, square_edge=368, scale_range=(0.5, 1.0), hflip_p=0.5):
    """The reference's draws for images of ``sizes`` [(h0, w0), ...] one after another, from torch's global generator:
    per image ``torch.rand(1).item() > hflip_p`` means no flip (transforms.py:398), then the factor
    ``lo + torch.rand(1).item() * (hi - lo)`` (:169-175; no draw when ``scale_range`` is a float), then Crop's offsets
    (:290-297) ``torch.randint(-padding, w - L + padding, (1,))`` clamped to [0, w - L], drawn only where the resized
    side exceeds L, x before y.  -> a list of dicts: hflip, factor, hr, wr (the resized size), crop_x, crop_y,
    square_edge."""
    out = []
    edge = int(square_edge)
    padding = int(edge / 2.0)
    for h0, w0 in sizes:
        hflip = not float(torch.rand(1).item()) > hflip_p
        if isinstance(scale_range, tuple):
            factor = scale_range[0] + torch.rand(1).item() * (scale_range[1] - scale_range[0])
        else:
            factor = scale_range
        wr, hr = int(w0 * factor), int(h0 * factor)
        crop_x = crop_y = 0
        if wr > edge:
            x = torch.randint(-padding, wr - edge + padding, (1,))
            crop_x = torch.clamp(x, min=0, max=wr - edge).item()
        if hr > edge:
            y = torch.randint(-padding, hr - edge + padding, (1,))
            crop_y = torch.clamp(y, min=0, max=hr - edge).item()
        out.append(dict(hflip=bool(hflip), factor=factor, hr=hr, wr=wr, crop_x=int(crop_x), crop_y=int(crop_y),
                        square_edge=edge))
    return out


def _horizontal_swap_coco(keypoints):
    """lib/datasets/utils.py:8-20: a float64 target, whatever the input's dtype."""
    target = np.zeros(keypoints.shape)
    for source_i, xyv in enumerate(keypoints):
        target[_HFLIP_TARGET[source_i]] = xyv
    return target


def valid_mask(valid_area, height, width):
    """The four integers (x0, y0, x1, y1) of utils.mask_valid_area (lib/datasets/utils.py:36-54) on a
    [3, height, width] tensor: it zeroes everything outside [x0, x1) x [y0, y1)."""
    x0 = int(valid_area[0]) if valid_area[0] >= 1.0 else 0
    y0 = int(valid_area[1]) if valid_area[1] >= 1.0 else 0
    y1 = min(int(math.ceil(valid_area[1] + valid_area[3])), height)
    x1 = min(int(math.ceil(valid_area[0] + valid_area[2])), width)
    return (min(x0, width), min(y0, height), max(x1, min(x0, width)), max(y1, min(y0, height)))


def transform_annotations(anns, size, params):
    """Normalize.normalize_annotations, HFlip, RescaleRelative.scale, Crop.crop and CenterPad.center_pad on the
    annotations of one image of ``size`` (h0, w0) under one entry of draw_params, statement for statement in the
    reference's dtypes (float32 keypoints until a flip makes them float64; float32 boxes; a float64 meta).
    ``anns``: dicts with 'keypoints' (51 numbers) and 'bbox'.
    -> (keypoints [K, 17, 3], bboxes [K, 4], meta, mask): meta has offset, scale, valid_area, hflip, width_height;
    mask is valid_mask of the final valid_area on the square canvas."""
    h0, w0 = int(size[0]), int(size[1])
    edge = params["square_edge"]
    kps = [np.asarray(a["keypoints"], dtype=np.float32).reshape(-1, 3) for a in anns]
    boxes = [np.asarray(a["bbox"], dtype=np.float32).copy() for a in anns]
    meta = {"offset": np.array((0.0, 0.0)), "scale": np.array((1.0, 1.0)), "valid_area": np.array((0.0, 0.0, w0, h0)),
            "hflip": False, "width_height": np.array((w0, h0))}
    w, h = w0, h0
    if params["hflip"]:                                                  # transforms.py:373-387
        for i in range(len(kps)):
            kps[i][:, 0] = -kps[i][:, 0] - 1.0 + w
            kps[i] = _horizontal_swap_coco(kps[i])
            boxes[i][0] = -(boxes[i][0] + boxes[i][2]) - 1.0 + w
        meta["hflip"] = True
        meta["valid_area"][0] = -(meta["valid_area"][0] + meta["valid_area"][2]) + w
    wr, hr = params["wr"], params["hr"]                                  # :190-207, :177-182
    x_scale = wr / w
    y_scale = hr / h
    for i in range(len(kps)):
        kps[i][:, 0] = (kps[i][:, 0] + 0.5) * x_scale - 0.5
        kps[i][:, 1] = (kps[i][:, 1] + 0.5) * y_scale - 0.5
        boxes[i][0] *= x_scale
        boxes[i][1] *= y_scale
        boxes[i][2] *= x_scale
        boxes[i][3] *= y_scale
    scale_factors = np.array((x_scale, y_scale))
    meta["offset"] *= scale_factors
    meta["scale"] *= scale_factors
    meta["valid_area"][:2] *= scale_factors
    meta["valid_area"][2:] *= scale_factors
    w, h = wr, hr
    x_offset, y_offset = params["crop_x"], params["crop_y"]              # :288-313, :272-280
    new_w = min(edge, w - x_offset)
    new_h = min(edge, h - y_offset)
    ltrb = np.array((x_offset, y_offset, x_offset + new_w, y_offset + new_h))
    for i in range(len(kps)):
        kps[i][:, 0] -= x_offset
        kps[i][:, 1] -= y_offset
        boxes[i][0] -= x_offset
        boxes[i][1] -= y_offset
    meta["offset"] += ltrb[:2]
    meta["valid_area"][:2] = np.maximum(0.0, meta["valid_area"][:2] - ltrb[:2])
    meta["valid_area"][2:] = np.maximum(0.0, meta["valid_area"][2:] - ltrb[:2])
    meta["valid_area"][2:] = np.minimum(meta["valid_area"][2:], ltrb[2:] - ltrb[:2])
    w, h = new_w, new_h
    left = int((edge - w) / 2.0)                                         # :340-362, :328-332
    top = int((edge - h) / 2.0)
    ltrb = (left, top, edge - w - left, edge - h - top)
    for i in range(len(kps)):
        kps[i][:, 0] += ltrb[0]
        kps[i][:, 1] += ltrb[1]
        boxes[i][0] += ltrb[0]
        boxes[i][1] += ltrb[1]
    meta["offset"] -= ltrb[:2]
    meta["valid_area"][:2] += ltrb[:2]
    dtype = np.float64 if params["hflip"] else np.float32
    keypoints = np.stack(kps) if kps else np.zeros((0, 17, 3), dtype)
    bboxes = np.stack(boxes) if boxes else np.zeros((0, 4), np.float32)
    return keypoints, bboxes, meta, valid_mask(meta["valid_area"], edge, edge)


def _size_of(image):
    return int(image.shape[0]), int(image.shape[1])


def augment_enqueue(descs, count, cfg, dst, layout, workspace):
    """Enqueue rtpose_augment_batch on the current stream: descs a (_capi.AugmentImage * count) array, dst a device
    address or tensor, layout a _capi.Layout or None (cfg.nchw == 1), workspace a device tensor of
    rtpose_augment_workspace_bytes."""
    check(lib.rtpose_augment_batch(descs, count, C.byref(cfg), dst if isinstance(dst, C.c_void_p) else ptr(dst),
                                   C.byref(layout) if layout is not None else None, ptr(workspace),
                                   workspace.numel() * workspace.element_size(), current_stream()),
          "rtpose_augment_batch")


def augment_images(images, params, out=None, norm=1, mask_valid=True, device=None, slots=None):
    """The image side for a batch: ``images`` a list of uint8 RGB [h0, w0, 3] numpy arrays or device tensors of any
    sizes, ``params`` what draw_params returned for their sizes.  -> an [N, 3, S, S] fp32 device tensor (S the
    square_edge of the params): flipped, resized (Pillow's bicubic, bit for bit), cropped, centre-padded with
    (124, 116, 104), ToTensor + ImageNet Normalize (``norm=1``; 0 keeps float(u) in 0..255) and, with ``mask_valid``,
    zero outside the valid area (utils.mask_valid_area).  With ``out=plan`` (a native plan of [>= N, S, S]) the images
    go into the plan's own input view instead, image k into slot slots[k] (default k), as preprocess_into_plan does,
    and the plan is returned.  One table launch and one fused launch per 32 images, on the current stream."""
    if len(images) != len(params):
        raise ValueError("%d images for %d params" % (len(images), len(params)))
    n = len(images)
    edge = params[0]["square_edge"] if n else 368
    if any(p["square_edge"] != edge for p in params):
        raise ValueError("one batch, one square_edge")
    if out is not None:
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    elif device is None:
        dev_imgs = [im for im in images if hasattr(im, "data_ptr")]
        device = dev_imgs[0].device if dev_imgs else torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise _capi.RtposeError("augment_images runs on an MI355X (HIP) device only (no CPU fallback); got %s" % device)
    with torch.cuda.device(device):
        held = []
        descs = (_capi.AugmentImage * max(n, 1))()
        for k, (im, p) in enumerate(zip(images, params)):
            if not hasattr(im, "data_ptr"):
                im = torch.from_numpy(np.ascontiguousarray(im, dtype=np.uint8)).to(device, non_blocking=True)
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
                raise ValueError("image %d must be a contiguous uint8 [h0, w0, 3] array" % k)
            held.append(im)
            h0, w0 = _size_of(im)
            d = descs[k]
            d.img_rgb, d.h0, d.w0, d.hr, d.wr = im.data_ptr(), h0, w0, p["hr"], p["wr"]
            d.hflip, d.crop_x, d.crop_y = int(bool(p["hflip"])), p["crop_x"], p["crop_y"]
            mask = transform_annotations([], (h0, w0), p)[3] if mask_valid else (0, 0, edge, edge)
            for j in range(4):
                d.mask[j] = mask[j]
            d.n_index = slots[k] if slots is not None else k
        if out is None:
            cfg = _capi.AugmentCfg.make(edge, edge, int(norm), 1, FILL)
            dst = torch.empty((n, 3, edge, edge), dtype=torch.float32, device=device)
            base, lay, result = ptr(dst), None, dst
            if slots is not None and n and not all(0 <= s < n for s in slots):
                raise _capi.RtposeError("image slots %s outside the %d-image result" % (list(slots), n))
        else:
            cfg = _capi.AugmentCfg.make(edge, edge, int(norm), 0, FILL)
            base, lay = C.c_void_p(), _capi.Layout()
            check(lib.rtpose_net_input_view(out.handle, C.byref(base), C.byref(lay)), "rtpose_net_input_view")
            pn, ph, pw = out.shape
            if (ph, pw) != (edge, edge):
                raise _capi.RtposeError("a %d x %d plan for a %d x %d canvas" % (ph, pw, edge, edge))
            for k in range(n):
                if not 0 <= descs[k].n_index < pn:
                    raise _capi.RtposeError("image slot %d outside the %d-image plan" % (descs[k].n_index, pn))
            result = out
        if n == 0:
            return result
        wb = lib.rtpose_augment_workspace_bytes(C.byref(cfg), n)
        if wb == 0:
            raise _capi.RtposeError("bad augment arguments: " + _capi.last_error())
        workspace = torch.empty(wb // 4, dtype=torch.int32, device=device)
        augment_enqueue(descs, n, cfg, base, lay, workspace)
        # the launches read the uploads and the tables after this function returns: the caching allocator hands their
        # memory out again only to work queued behind them on this stream
        del held, workspace
    return result


def train_batch(images, annotations, params=None, skeleton=encode.COCO18_TRAIN, stride=8, sigma=7.0, device=None):
    """-> (image [N, 3, S, S], heat [N, C_h, S / stride, S / stride], paf [N, C_p, ...], metas): the tuple
    collate_images_targets_meta makes of CocoKeypoints items (datasets.py:86-92, :193-214), as fp32 device tensors,
    plus the per-image meta dicts (with 'keypoints': the augmented [K, 17, 3] annotations in the reference's dtype, and
    'bboxes').  ``images``: uint8 RGB arrays or device tensors; ``annotations``: per image a list of COCO annotation
    dicts ('keypoints', 'bbox'); ``params=None`` draws them (draw_params on torch's global generator).  The targets come
    from the augmented keypoints through add_neck in their own dtype, remove_illegal_joint and encode_targets, as
    get_ground_truth does (datasets.py:259-274)."""
    if len(images) != len(annotations):
        raise ValueError("%d images for %d annotation lists" % (len(images), len(annotations)))
    sizes = [_size_of(im) for im in images]
    if params is None:
        params = draw_params(sizes)
    edge = params[0]["square_edge"] if params else 368
    people, metas = [], []
    for anns, size, p in zip(annotations, sizes, params):
        kps, boxes, meta, _ = transform_annotations(anns, size, p)
        # datasets.py:268-274: np.array of the persons' add_neck rows keeps their dtype, then remove_illegal_joint
        # (which encode_targets applies itself: an illegal joint is an absent one)
        kp18 = np.array([encode.add_neck(k, dtype=None) for k in kps]).reshape(-1, 18, 3)
        people.append(kp18)
        meta = copy.deepcopy(meta)
        meta["keypoints"], meta["bboxes"] = kps, boxes
        metas.append(meta)
    image = augment_images(images, params, device=device)
    heat, paf = encode.encode_targets(people, skeleton, (edge, edge), stride, sigma, device=image.device)
    return image, heat, paf, metas
