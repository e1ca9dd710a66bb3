"""Training batches augmented on the device: flip, rescale, crop, pad, colour jitter, JPEG re-compression, normalise,
mask (csrc/augment.hip, header 4c; csrc/colorjitter.hip, header 4d; csrc/jpeg_roundtrip.hip, header 4e).

What ``CocoKeypoints.__getitem__`` of the reference does before it yields ``(image, heatmaps, pafs)``
(lib/datasets/datasets.py:156-214): the preprocess chain of train/train_VGG19.py:124-130 - ``Normalize``,
``RandomApply(HFlip, 0.5)``, ``RescaleRelative()``, ``Crop(368)``, ``CenterPad(368)`` of lib/datasets/transforms.py -,
then the image transform, ``utils.mask_valid_area`` and ``get_ground_truth``.  The image transform is ``image_transform``
(``ToTensor`` + ImageNet ``Normalize``) by default and, with ``color``, the one the training script passes
(train_VGG19.py:55,70): ``image_transform_train`` (transforms.py:53-65) = ``ColorJitter(0.1, 0.1, 0.1, 0.1)``,
``RandomApply([jpeg], p=0.1)``, ``RandomGrayscale(p=0.01)``, ``ToTensor``, ``Normalize``.

The split: the random draws (``draw_params``, ``draw_color_params``, ``draw_train_params``: torch's global generator in
the reference's order) and the annotation bookkeeping (``transform_annotations``, numpy in the reference's dtypes) are
host work of a few microseconds per image; the pixels - a PIL bicubic resize and four PIL enhancement passes per image
in the reference - are launches per batch (``augment_images``, ``color_jitter``, ``jpeg_roundtrip``), and the targets
are ``encode.encode_targets``.  ``train_batch`` is the whole item pipeline for a batch.  The image is the reference's bits
(Pillow's two integer resample passes, its ImageEnhance / blend / convert('L' / 'HSV' / 'RGB') arithmetic and
libjpeg-turbo's integer codec chain restated on the device), the keypoints are its bits including their dtype (float32
until a flip makes them float64), the targets follow encode.py's contract.

Not pinned: torchvision is not installed where this was written and the reference pins no version of it, so the order
of ColorJitter's and RandomGrayscale's draws is restated from torchvision 0.9 and later (``draw_color_params``), as
``ToTensor`` was.

Opt-in: the JPEG re-compression of ``RandomApply([jpeg], p=0.1)`` (save at quality 50, re-open).  Its draw is always
consumed, so the generator stays in step with the reference, and recorded as ``jpeg``; the pixels take the round trip
only with ``jpeg=True`` (``color_jitter``, ``augment_images``, ``train_batch``), through the kernels of header section
4e, in libjpeg-turbo's bits.  Without the keyword the launches and the bits are those of the releases in which the step
was not built.

File entries: an image may be given as the ``bytes`` of a JPEG file or as a path (datasets.py:171-172,
``Image.open(f).convert('RGB')``).  ``decode_jpegs`` turns baseline files into the uint8 device tensors the rest takes:
Huffman decoding on host threads (csrc/jpeg_entropy.cpp), de-quantisation, inverse DCT, up-sampling and colour
conversion on the device (csrc/jpeg_decode.hip, header section 4f), in the bits of Pillow on libjpeg-turbo.  A file
outside the served subset (progressive, CMYK, ...) goes through Pillow itself.

Out of scope: ``RandomRotate`` (cv2 ``warpAffine``; not in the training script's chain); ``RescaleAbsolute`` /
``MultiScale``; EXIF orientation (``Image.open`` does not apply it either); PNG; the DataLoader.  (``ColorJitter`` and
``RandomGrayscale`` were out of scope until the colour jitter of header section 4d, JPEG re-compression until section
4e, image decoding until section 4f.)
"""
import copy
import ctypes as C
import io
import math
import os
from concurrent.futures import ThreadPoolExecutor

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


def hue_shift_of(hue_factor):
    """What torchvision's adjust_hue adds to the uint8 H plane of a PIL image: ``np.uint8(hue_factor * 255)``, i.e.
    int(hue_factor * 255) truncated toward zero, modulo 256 (-12.75 -> -12 -> 244)."""
    return int(hue_factor * 255) % 256


def _uniform(lo, hi):
    return float(torch.empty(1).uniform_(lo, hi))


def _draw_color_one(brightness, contrast, saturation, hue, jpeg_p, gray_p):
    fn_idx = [int(v) for v in torch.randperm(4)]
    b = _uniform(max(0.0, 1 - brightness), 1 + brightness) if brightness else None
    c = _uniform(max(0.0, 1 - contrast), 1 + contrast) if contrast else None
    s = _uniform(max(0.0, 1 - saturation), 1 + saturation) if saturation else None
    h = _uniform(-hue, hue) if hue else None
    jpeg = not jpeg_p < float(torch.rand(1))
    gray = float(torch.rand(1)) < gray_p
    present = (b is not None, c is not None, s is not None, h is not None)
    order = [op if present[op] else -1 for op in fn_idx]
    return dict(order=order, brightness=b, contrast=c, saturation=s, hue=h,
                hue_shift=hue_shift_of(h) if h is not None else 0, jpeg=bool(jpeg), gray=bool(gray))


def draw_color_params(n, brightness=0.1, contrast=0.1, saturation=0.1, hue=0.1, jpeg_p=0.1, gray_p=0.01):
    """The draws of ``image_transform_train`` (transforms.py:53-65) for ``n`` images one after another, from torch's
    global generator.  Per image, in the order of torchvision 0.9 and later (``ColorJitter.get_params``, then
    ``RandomApply.forward``, then ``RandomGrayscale.forward``): ``torch.randperm(4)`` (the order of the four operations:
    0 brightness, 1 contrast, 2 saturation, 3 hue); ``float(torch.empty(1).uniform_(lo, hi))`` for brightness, contrast
    and saturation over (max(0, 1 - x), 1 + x) each and for hue over (-x, x), an operation whose x is 0 drawing nothing
    and dropping out (order entry -1); ``torch.rand(1)`` for RandomApply - the JPEG step fires unless ``p < draw``;
    ``torch.rand(1)`` for RandomGrayscale - fires if ``draw < p``.
    torchvision is not installed where this was written and the reference pins no version of it: this order is restated
    from its source, not checked against it.  The JPEG draw is consumed and recorded here whatever happens to the pixels:
    the re-compression itself, not built before header section 4e, is ``jpeg=True`` of color_jitter.
    -> a list of dicts: order, brightness, contrast, saturation, hue (python floats or None), hue_shift, jpeg, gray."""
    return [_draw_color_one(brightness, contrast, saturation, hue, jpeg_p, gray_p) for _ in range(n)]


def draw_train_params(sizes, square_edge=368, scale_range=(0.5, 1.0), hflip_p=0.5, **color):
    """The draws of whole items as ``CocoKeypoints.__getitem__`` makes them (datasets.py:180, :198): for image k the
    geometry (``draw_params``' draws), then its colour (``draw_color_params``' draws, ``color`` its keywords), then image
    k + 1.  -> (params, cparams)."""
    params, cparams = [], []
    for size in sizes:
        params += draw_params([size], square_edge, scale_range, hflip_p)
        cparams += draw_color_params(1, **color)
    return params, cparams


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


def _is_file(image):
    """An entry of ``images`` that stands for a file: its bytes, or a path."""
    return isinstance(image, (bytes, bytearray, memoryview, str, os.PathLike))


def _file_bytes(f):
    if isinstance(f, (str, os.PathLike)):
        with open(f, 'rb') as fh:
            return fh.read()
    return f if isinstance(f, bytes) else bytes(f)


def _probe(data):
    info = _capi.JpegInfo()
    lib.rtpose_jpeg_probe(data, len(data), C.byref(info))
    return info


def _reason(code):
    return lib.rtpose_jpeg_reason_text(int(code)).decode()


def jpeg_probe(data):
    """What the markers of a JPEG file (its ``bytes``, or a path) say, without decoding it (rtpose_jpeg_probe, header
    section 4f).  -> a dict: ``served`` - whether the native decoder takes the file as far as its headers tell; if so
    ``width``, ``height``, ``components`` (1 or 3), ``mode`` ('gray', '4:4:4', '4:2:2', '4:2:0', '4:4:0'), ``sampling``
    (per component (h, v)), ``restart_interval`` and ``coef_count``; if not, ``reason`` (a sentence) and ``reason_code``
    (RTPOSE_JPEG_R_*), the other entries None."""
    info = _probe(_file_bytes(data))
    if info.reason:
        return dict(served=False, reason=_reason(info.reason), reason_code=int(info.reason), width=None, height=None,
                    components=None, mode=None, sampling=None, restart_interval=None, coef_count=None)
    nc = int(info.components)
    return dict(served=True, reason=None, reason_code=0, width=int(info.width), height=int(info.height), components=nc,
                mode=_capi.JPEG_MODES[info.mode], sampling=[(int(info.hsamp[c]), int(info.vsamp[c])) for c in range(nc)],
                restart_interval=int(info.restart_interval), coef_count=int(info.coef_count))


def _pil_open(data):
    from PIL import Image
    return Image.open(io.BytesIO(data))


def decode_jpegs(files, device=None, fallback='pil', workers=8, pinned=True):
    """``Image.open(f).convert('RGB')`` for a batch of JPEG files.  ``files``: ``bytes``, or paths that are read with
    ``open(..., 'rb')``.  -> (images, infos): images uint8 [h, w, 3] device tensors - what augment_images takes as
    sources -, infos per image a dict with width, height, mode, ``native`` (which path it took) and ``reason`` (why
    not, else None).
    The native path (header section 4f): rtpose_jpeg_probe sizes one staging tensor (``pinned``: in page-locked memory)
    that holds per image its three quantiser tables and its quantised coefficients; rtpose_jpeg_entropy_decode fills
    it on a ThreadPoolExecutor of ``workers`` threads (ctypes releases the GIL; capped at 16, never derived from the
    machine's CPU count); one host-to-device copy; then rtpose_jpeg_decode_batch's two launch kinds per 32 images, all on
    the current stream.  Bit for bit what Pillow on libjpeg-turbo returns.
    A file the native path refuses - progressive, CMYK, an Adobe segment, odd sampling, damaged data, a coefficient
    beyond int16: the refusals of section 4f - goes through Pillow and an upload with ``fallback='pil'``; with
    ``fallback=None`` it raises RtposeError with the reason."""
    if fallback not in ('pil', None):
        raise ValueError("fallback is 'pil' or None")
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise _capi.RtposeError("decode_jpegs runs on an MI355X (HIP) device only (no CPU fallback); got %s" % device)
    datas = [_file_bytes(f) for f in files]
    n = len(datas)
    probes = [_probe(d) for d in datas]
    offsets, total = [], 0
    for info in probes:                      # per served image: 192 words of tables, then its coefficients
        offsets.append(total)
        if not info.reason:
            total += 192 + int(info.coef_count)
    reasons = [int(info.reason) for info in probes]
    jobs = [k for k in range(n) if not reasons[k]]
    staging = torch.empty(max(total, 8), dtype=torch.int16, pin_memory=bool(pinned)) if jobs else None

    def host_stage(k):
        at = staging.data_ptr() + 2 * offsets[k]
        return lib.rtpose_jpeg_entropy_decode(datas[k], len(datas[k]), C.byref(probes[k]), C.c_void_p(at + 2 * 192),
                                              int(probes[k].coef_count), C.c_void_p(at))

    threads = max(1, min(int(workers), 16, len(jobs)))
    if threads > 1:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            codes = list(pool.map(host_stage, jobs))
    else:
        codes = [host_stage(k) for k in jobs]
    for k, rc in zip(jobs, codes):
        reasons[k] = int(rc)
    if fallback is None:
        for k in range(n):
            if reasons[k]:
                raise _capi.RtposeError("decode_jpegs: file %d is not served by the native decoder: %s (reason %d)"
                                        % (k, _reason(reasons[k]), reasons[k]))
    native = [k for k in range(n) if not reasons[k]]
    images, infos = [None] * n, [None] * n
    with torch.cuda.device(device):
        if native:
            coef = torch.empty(staging.numel(), dtype=torch.int16, device=device)
            coef.copy_(staging, non_blocking=True)
            descs = (_capi.JpegDecodeImage * len(native))()
            for j, k in enumerate(native):
                info, d = probes[k], descs[j]
                images[k] = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=device)
                d.width, d.height, d.mode, d.reserved = info.width, info.height, info.mode, 0
                d.qtab_offset, d.coef_offset, d.dst = offsets[k], offsets[k] + 192, images[k].data_ptr()
                infos[k] = dict(width=int(info.width), height=int(info.height), mode=_capi.JPEG_MODES[info.mode],
                                native=True, reason=None)
            wb = lib.rtpose_jpeg_decode_workspace_bytes(descs, len(native))
            if wb == 0:
                raise _capi.RtposeError("bad jpeg decode arguments: " + _capi.last_error())
            workspace = torch.empty(wb // 8, dtype=torch.int64, device=device)
            check(lib.rtpose_jpeg_decode_batch(descs, len(native), ptr(coef), coef.numel(), ptr(workspace), wb,
                                               current_stream()), "rtpose_jpeg_decode_batch")
            # the copy reads the staging tensor and the launches read coef and the workspace after this function returns:
            # torch's allocators hand their memory out again only to work queued behind them (as in augment_images)
            del coef, workspace
        for k in range(n):
            if reasons[k]:
                im = _pil_open(datas[k])
                mode = im.mode           # Pillow's own name for what the file holds: 'L', 'RGB', 'CMYK'
                arr = np.array(im.convert('RGB'))
                images[k] = torch.from_numpy(arr).to(device, non_blocking=True)
                infos[k] = dict(width=int(arr.shape[1]), height=int(arr.shape[0]), mode=mode, native=False,
                                reason=_reason(reasons[k]))
    return images, infos


def _size_of(image):
    if _is_file(image):                  # a file entry: its header says the size, nothing is decoded
        data = _file_bytes(image)
        info = _probe(data)
        if not info.reason:
            return int(info.height), int(info.width)
        w, h = _pil_open(data).size
        return int(h), int(w)
    return int(image.shape[0]), int(image.shape[1])


def _decode_entries(images, device):
    """The file entries of ``images`` decoded by decode_jpegs.  -> (images with tensors in their places, {index: info})."""
    which = [k for k, im in enumerate(images) if _is_file(im)]
    if not which:
        return images, {}
    decoded, infos = decode_jpegs([images[k] for k in which], device=device)
    images = list(images)
    for j, k in enumerate(which):
        images[k] = decoded[j]
    return images, {k: infos[j] for j, k in enumerate(which)}


def augment_enqueue(descs, count, cfg, dst, layout, workspace):
    """Enqueue rtpose_augment_batch on the current stream: descs a (_capi.AugmentImage * count) array, dst a device
    address or tensor, layout a _capi.Layout or None (cfg.nchw == 1), workspace a device tensor of
    rtpose_augment_workspace_bytes."""
    check(lib.rtpose_augment_batch(descs, count, C.byref(cfg), dst if isinstance(dst, C.c_void_p) else ptr(dst),
                                   C.byref(layout) if layout is not None else None, ptr(workspace),
                                   workspace.numel() * workspace.element_size(), current_stream()),
          "rtpose_augment_batch")


def jitter_enqueue(descs, count, cfg, src, dst, layout, workspace):
    """Enqueue rtpose_jitter_batch on the current stream: descs a (_capi.JitterImage * count) array, src a dense device
    tensor, dst a device address or tensor, layout a _capi.Layout or None (cfg.nchw == 1), workspace a device tensor of
    rtpose_jitter_workspace_bytes."""
    check(lib.rtpose_jitter_batch(descs, count, C.byref(cfg), ptr(src), dst if isinstance(dst, C.c_void_p) else ptr(dst),
                                  C.byref(layout) if layout is not None else None, ptr(workspace),
                                  workspace.numel() * workspace.element_size(), current_stream()),
          "rtpose_jitter_batch")


def jpeg_enqueue(descs, count, cfg, src, dst, workspace):
    """Enqueue rtpose_jpeg_roundtrip_batch on the current stream: descs a (_capi.JpegImage * count) array, src and dst
    dense device tensors (or addresses; the same one for in place), workspace a device tensor of
    rtpose_jpeg_workspace_bytes."""
    check(lib.rtpose_jpeg_roundtrip_batch(descs, count, C.byref(cfg), src if isinstance(src, C.c_void_p) else ptr(src),
                                          dst if isinstance(dst, C.c_void_p) else ptr(dst), ptr(workspace),
                                          workspace.numel() * workspace.element_size(), current_stream()),
          "rtpose_jpeg_roundtrip_batch")


def _dense_canvas(canvas, who):
    if not hasattr(canvas, "data_ptr") or canvas.dim() != 4 or canvas.shape[1] != 3 or canvas.dtype != torch.float32 \
            or not canvas.is_contiguous():
        raise ValueError("canvas must be a contiguous fp32 [N, 3, h, w] tensor")
    if canvas.device.type != 'cuda':
        raise _capi.RtposeError("%s runs on an MI355X (HIP) device only (no CPU fallback); got %s" % (who, canvas.device))
    return (int(v) for v in canvas.shape)


def jpeg_roundtrip(canvas, which=None, quality=50, out=None, slots=None):
    """Saving as a JPEG at ``quality`` and re-opening, on the device (header section 4e): what
    ``jpeg_compression_augmentation`` of the reference (transforms.py:28-31) does to the pixels, in libjpeg-turbo's bits.
    ``canvas``: a dense fp32 [N, 3, h, w] device tensor holding the integers 0..255; ``which``: the indices of the images
    that take the round trip (default all; each at most once).  ``out=None`` -> a copy of the canvas with those images
    replaced; ``out=canvas`` works in place; another dense [M, 3, h, w] tensor takes listed image which[j] in slot
    slots[j] (default which[j]) and keeps its other slots as they are.  Two launches per 32 listed images, on the current
    stream.  -> the result."""
    n, _, h, w = _dense_canvas(canvas, "jpeg_roundtrip")
    which = list(range(n)) if which is None else [int(k) for k in which]
    if not all(0 <= k < n for k in which):
        raise ValueError("which %s outside the %d canvases" % (which, n))
    if slots is not None and len(slots) != len(which):
        raise ValueError("%d listed images for %d slots" % (len(which), len(slots)))
    if out is None:
        out = canvas.clone()
    if not hasattr(out, "data_ptr") or out.dim() != 4 or tuple(out.shape[1:]) != (3, h, w) or out.dtype != torch.float32 \
            or not out.is_contiguous() or out.device != canvas.device:
        raise ValueError("out must be a contiguous fp32 [M, 3, %d, %d] tensor on the canvas's device" % (h, w))
    count = len(which)
    descs = (_capi.JpegImage * max(count, 1))()
    for j, k in enumerate(which):
        descs[j].n_src, descs[j].n_dst = k, (int(slots[j]) if slots is not None else k)
        if not 0 <= descs[j].n_dst < out.shape[0]:
            raise _capi.RtposeError("image slot %d outside the %d-image result" % (descs[j].n_dst, out.shape[0]))
    if count == 0:
        return out
    with torch.cuda.device(canvas.device):
        cfg = _capi.JpegCfg.make(h, w, int(quality))
        wb = lib.rtpose_jpeg_workspace_bytes(C.byref(cfg), count)
        if wb == 0:
            raise _capi.RtposeError("bad jpeg arguments: " + _capi.last_error())
        workspace = torch.empty(wb // 8, dtype=torch.int64, device=canvas.device)
        jpeg_enqueue(descs, count, cfg, canvas, out, workspace)
        del workspace     # as in augment_images: handed out again only to work queued behind the launches
    return out


def color_jitter(canvas, cparams, masks=None, norm=1, out=None, slots=None, jpeg=False):
    """ColorJitter and RandomGrayscale on the device, then ToTensor + Normalize and the mask (header section 4d).
    ``canvas``: a dense fp32 [N, 3, h, w] device tensor holding the integers 0..255 (what augment_images makes with
    ``norm=0, mask_valid=False``); ``cparams``: what draw_color_params returned for its N images (order, brightness,
    contrast, saturation, hue_shift, gray, jpeg); ``masks``: per
    image (x0, y0, x1, y1), None = the whole canvas.  ``out=None`` -> a new [N, 3, h, w] tensor; ``out=canvas`` works in
    place; another dense [>= N, 3, h, w] tensor or a native plan of [>= N, h, w] takes image k in slot slots[k]
    (default k).  ``norm=1`` normalises, 0 keeps float(u).  Bit for bit what Pillow computes for the same operations
    (ImageEnhance.Brightness / Contrast / Color, convert('HSV') / convert('RGB') around the hue shift, convert('L')).
    Two launches per 32 images - one if none of them has contrast -, on the current stream.
    ``jpeg``: False, the default - an image's ``jpeg`` entry is not applied, the launches and the bits are those of the
    releases where the JPEG re-compression was not built.  True - the images whose entry is true (the reference's
    RandomApply fired) take image_transform_train's middle step where the reference takes it, between ColorJitter and
    RandomGrayscale: their ColorJitter operations alone into an 8-bit canvas of their own (rtpose_jitter_batch with
    gray 0, norm 0, the whole canvas), rtpose_jpeg_roundtrip_batch on it in place at quality 50 (header section 4e),
    then rtpose_jitter_batch with an empty order and the real gray, norm, mask and destination; the other images go
    through one rtpose_jitter_batch call exactly as without the keyword.  -> the result."""
    n, _, h, w = _dense_canvas(canvas, "color_jitter")
    if len(cparams) != n:
        raise ValueError("%d canvases for %d colour params" % (n, len(cparams)))
    if masks is not None and len(masks) != n:
        raise ValueError("%d canvases for %d masks" % (n, len(masks)))
    if slots is not None and len(slots) != n:
        raise ValueError("%d canvases for %d slots" % (n, len(slots)))
    with torch.cuda.device(canvas.device):
        descs = (_capi.JitterImage * max(n, 1))()
        for k, cp in enumerate(cparams):
            d = descs[k]
            for j in range(4):
                d.order[j] = cp["order"][j]
            for j, name in enumerate(("brightness", "contrast", "saturation")):
                d.factor[j] = cp[name] if cp.get(name) is not None else 1.0
            d.hue_shift, d.gray = int(cp.get("hue_shift", 0)), int(bool(cp.get("gray")))
            mask = masks[k] if masks is not None else (0, 0, w, h)
            for j in range(4):
                d.mask[j] = mask[j]
            d.n_src, d.n_dst = k, (slots[k] if slots is not None else k)
        if out is None or hasattr(out, "data_ptr"):
            cfg = _capi.JitterCfg.make(h, w, int(norm), 1)
            if out is None:
                out = torch.empty_like(canvas)
            if out.dim() != 4 or tuple(out.shape[1:]) != (3, h, w) or out.dtype != torch.float32 or not out.is_contiguous() \
                    or out.device != canvas.device:
                raise ValueError("out must be a contiguous fp32 [>= N, 3, %d, %d] tensor on the canvas's device" % (h, w))
            for k in range(n):
                if not 0 <= descs[k].n_dst < out.shape[0]:
                    raise _capi.RtposeError("image slot %d outside the %d-image result" % (descs[k].n_dst, out.shape[0]))
            base, lay = ptr(out), None
        else:
            cfg = _capi.JitterCfg.make(h, w, int(norm), 0)
            base, lay = C.c_void_p(), _capi.Layout()
            check(lib.rtpose_net_input_view(out.handle, C.byref(base), C.byref(lay)), "rtpose_net_input_view")
            pn, ph, pw = out.shape
            if (ph, pw) != (h, w):
                raise _capi.RtposeError("a %d x %d plan for a %d x %d canvas" % (ph, pw, h, w))
            for k in range(n):
                if not 0 <= descs[k].n_dst < pn:
                    raise _capi.RtposeError("image slot %d outside the %d-image plan" % (descs[k].n_dst, pn))
        if n == 0:
            return out
        fire = [k for k, cp in enumerate(cparams) if cp.get("jpeg")] if jpeg else []

        def jitter(some, count, jcfg, src, dst, dlay):
            wb = lib.rtpose_jitter_workspace_bytes(C.byref(jcfg), count)
            if wb == 0:
                raise _capi.RtposeError("bad jitter arguments: " + _capi.last_error())
            workspace = torch.empty(wb // 4, dtype=torch.int32, device=canvas.device)
            jitter_enqueue(some, count, jcfg, src, dst, dlay, workspace)
            del workspace     # as in augment_images: handed out again only to work queued behind the launches

        if not fire:
            jitter(descs, n, cfg, canvas, base, lay)
            return out
        rest = [k for k in range(n) if not cparams[k].get("jpeg")]
        if rest:
            plain = (_capi.JitterImage * len(rest))(*[descs[k] for k in rest])
            jitter(plain, len(rest), cfg, canvas, base, lay)
        # the firing images: ColorJitter alone -> the 8-bit canvas the reference saves; the round trip; the rest of the chain
        nf = len(fire)
        u8 = torch.empty((nf, 3, h, w), dtype=torch.float32, device=canvas.device)
        before, after = (_capi.JitterImage * nf)(), (_capi.JitterImage * nf)()
        for j, k in enumerate(fire):
            a, b, d = before[j], after[j], descs[k]
            for i in range(4):
                a.order[i], b.order[i] = d.order[i], -1
                a.mask[i], b.mask[i] = (0, 0, w, h)[i], d.mask[i]
            for i in range(3):
                a.factor[i], b.factor[i] = d.factor[i], 1.0
            a.hue_shift, a.gray, a.n_src, a.n_dst = d.hue_shift, 0, d.n_src, j
            b.hue_shift, b.gray, b.n_src, b.n_dst = 0, d.gray, j, d.n_dst
        jitter(before, nf, _capi.JitterCfg.make(h, w, 0, 1), canvas, u8, None)
        jpeg_roundtrip(u8, out=u8)
        jitter(after, nf, cfg, u8, base, lay)
        del u8
    return out


def augment_images(images, params, out=None, norm=1, mask_valid=True, device=None, slots=None, color=None, jpeg=False):
    """The image side for a batch: ``images`` a list of uint8 RGB [h0, w0, 3] numpy arrays or device tensors of any
    sizes - or JPEG files, as ``bytes`` or paths, which decode_jpegs decodes first (their sizes for draw_params come
    from jpeg_probe) -, ``params`` what draw_params returned for their sizes.  -> an [N, 3, S, S] fp32 device tensor (S the
    square_edge of the params): flipped, resized (Pillow's bicubic, bit for bit), cropped, centre-padded with
    (124, 116, 104), ToTensor + ImageNet Normalize (``norm=1``; 0 keeps float(u) in 0..255) and, with ``mask_valid``,
    zero outside the valid area (utils.mask_valid_area).  With ``out=plan`` (a native plan of [>= N, S, S]) the images
    go into the plan's own input view instead, image k into slot slots[k] (default k), as preprocess_into_plan does,
    and the plan is returned.  One table launch and one fused launch per 32 images, on the current stream.
    ``color``: what draw_color_params returned for the images; then the geometry launches write the uint8 canvas
    (norm 0, no mask) into a tensor of their own and color_jitter's launches make the result from it with the real
    ``norm`` and mask (ColorJitter and RandomGrayscale of image_transform_train).  The default, None, gives the launches
    and the bits of a call without the keyword.
    ``jpeg``: with ``color``, color_jitter's keyword - True applies image_transform_train's JPEG step (header section
    4e) to the images whose colour params say it fired; False, the default, leaves it out as the releases did in which
    it was not built."""
    if len(images) != len(params):
        raise ValueError("%d images for %d params" % (len(images), len(params)))
    if jpeg and color is None:
        raise ValueError("jpeg=True needs the colour params that say which images fire (color=...)")
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
    images, _ = _decode_entries(images, device)       # file entries (bytes, paths) become device tensors first
    if color is not None:
        if len(color) != n:
            raise ValueError("%d images for %d colour params" % (n, len(color)))
        masks = [transform_annotations([], _size_of(im), p)[3] if mask_valid else (0, 0, edge, edge)
                 for im, p in zip(images, params)]
        with torch.cuda.device(device):
            canvas = augment_images(images, params, norm=0, mask_valid=False, device=device)
            if out is None and slots is None:
                return color_jitter(canvas, color, masks, norm, out=canvas, jpeg=jpeg)
            if out is None:
                if n and not all(0 <= s < n for s in slots):
                    raise _capi.RtposeError("image slots %s outside the %d-image result" % (list(slots), n))
                out = torch.empty_like(canvas)
            return color_jitter(canvas, color, masks, norm, out=out, slots=slots, jpeg=jpeg)
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


def train_batch(images, annotations, params=None, skeleton=encode.COCO18_TRAIN, stride=8, sigma=7.0, device=None,
                color=False, jpeg=False):
    """-> (image [N, 3, S, S], heat [N, C_h, S / stride, S / stride], paf [N, C_p, ...], metas): the tuple
    collate_images_targets_meta makes of CocoKeypoints items (datasets.py:86-92, :193-214), as fp32 device tensors,
    plus the per-image meta dicts (with 'keypoints': the augmented [K, 17, 3] annotations in the reference's dtype, and
    'bboxes').  ``images``: uint8 RGB arrays or device tensors, or JPEG files as ``bytes`` or paths - those are sized by
    jpeg_probe for the draws, decoded by decode_jpegs (header section 4f; Pillow for a file outside the served subset),
    and their metas carry 'decoded_native'; ``annotations``: per image a list of COCO annotation
    dicts ('keypoints', 'bbox'); ``params=None`` draws them (draw_params on torch's global generator).  The targets come
    from the augmented keypoints through add_neck in their own dtype, remove_illegal_joint and encode_targets, as
    get_ground_truth does (datasets.py:259-274).
    ``color``: False - the image is ``image_transform``'s, as before the keyword; True - ``image_transform_train``'s
    ColorJitter and RandomGrayscale are applied to the canvas before normalisation, drawn
    with the geometry in the reference's order where ``params`` is None (draw_train_params), else on their own
    (draw_color_params); or a list of colour params.  The metas then carry 'color' (the params), 'jpeg' (whether the
    reference would have re-compressed this image) and 'jpeg_applied' (whether this call did).
    ``jpeg``: False, the default - the JPEG step is left out, as in the releases where it was not built; True - with
    ``color``, the images whose draw fired are saved at quality 50 and re-opened on the device between ColorJitter and
    RandomGrayscale (header section 4e), which completes image_transform_train."""
    if len(images) != len(annotations):
        raise ValueError("%d images for %d annotation lists" % (len(images), len(annotations)))
    images = [_file_bytes(im) if _is_file(im) else im for im in images]     # a path is read once
    sizes = [_size_of(im) for im in images]
    cparams = None if color is False or color is None else color
    if jpeg and cparams is None:
        raise ValueError("jpeg=True needs color (the JPEG step is part of image_transform_train)")
    if cparams is True:
        if params is None:
            params, cparams = draw_train_params(sizes)
        else:
            cparams = draw_color_params(len(sizes))
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
    if any(_is_file(im) for im in images):
        if device is None:
            on_device = [im for im in images if hasattr(im, "data_ptr")]
            device = on_device[0].device if on_device else None
        images, decoded = _decode_entries(images, device)
        for k, info in decoded.items():
            metas[k]["decoded_native"] = bool(info["native"])
    if cparams is not None:
        for meta, cp in zip(metas, cparams):
            meta["color"], meta["jpeg"] = copy.deepcopy(cp), bool(cp.get("jpeg"))
            meta["jpeg_applied"] = bool(jpeg) and meta["jpeg"]
        image = augment_images(images, params, device=device, color=cparams, jpeg=jpeg)
    else:
        image = augment_images(images, params, device=device)
    heat, paf = encode.encode_targets(people, skeleton, (edge, edge), stride, sigma, device=image.device)
    return image, heat, paf, metas
