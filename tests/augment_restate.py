"""numpy restatement of the image side of the training augmentation (csrc/augment.hip, header section 4c): Pillow's
``Image.resize(size, BICUBIC)`` on 8-bit RGB (ImagingResample: two separable integer passes with a uint8 intermediate,
22-bit coefficients made in float64), then the reference's HFlip / Crop / CenterPad / ToTensor + Normalize /
mask_valid_area (lib/datasets/transforms.py, lib/datasets/utils.py:36-54) on the pixels.  The kernel is tested against
this file, this file against the reference-made fixture and, where PIL imports, against PIL itself.
"""
import math

import numpy as np

MAX_TAPS = 17            # RTPOSE_AUG_MAX_TAPS
PRECISION_BITS = 32 - 8 - 2
FILL = (124, 116, 104)   # CenterPad's fill (transforms.py:352-353)
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def bicubic(t):
    a = -0.5
    if t < 0.0:
        t = -t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def ksize_of(in_size, out_size):
    scale = in_size / out_size
    support = 2.0 * max(scale, 1.0)
    return int(math.ceil(support)) * 2 + 1


def resample_table(in_size, out_size, first=0, count=None):
    """-> (bounds int32 [count, 2] = (xmin, taps), coeffs int32 [count, MAX_TAPS], unused slots 0) of outputs
    [first, first + count) of one axis: python floats are IEEE doubles and nothing here is fused."""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    bounds = np.zeros((count, 2), np.int32)
    coeffs = np.zeros((count, MAX_TAPS), np.int32)
    for i in range(count):
        xx = first + i
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, xmax)
        for x, v in enumerate(w):
            coeffs[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coeffs


def _pass(src, axis, out_size, rounded):
    """One pass along `axis` (0 rows / 1 columns) of an [h, w, c] array; uint8 out when rounded, else float64."""
    in_size = src.shape[axis]
    bounds, coeffs = resample_table(in_size, out_size)
    s = np.moveaxis(src, axis, 0)
    out = np.empty((out_size,) + s.shape[1:], np.uint8 if rounded else np.float64)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        k = coeffs[xx, :n]
        if rounded:
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k.astype(np.int64), s[xmin:xmin + n].astype(np.int64), 1)
            assert np.abs(acc).max() < 2 ** 31       # Pillow accumulates in a C int
            out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
        else:
            out[xx] = np.tensordot(k.astype(np.float64), s[xmin:xmin + n].astype(np.float64), 1) / (1 << PRECISION_BITS)
    return np.moveaxis(out, 0, axis)


def resize_bicubic_u8(img, out_w, out_h, rounded_intermediate=True):
    """Image.resize((out_w, out_h), BICUBIC) of a uint8 [h, w, 3] array: the horizontal pass first and only if the width
    changes, the vertical pass on its uint8 result and only if the height changes.  rounded_intermediate=False keeps the
    horizontal result unrounded in float64 (what a single-pass or float resample would do): NOT Pillow, it exists so
    that a test can show its case tells the two apart."""
    h, w = img.shape[:2]
    cur = img
    if out_w != w:
        cur = _pass(cur, 1, out_w, rounded_intermediate)
    if out_h != h:
        if cur.dtype == np.uint8:
            cur = _pass(cur, 0, out_h, True)
        else:
            cur = np.clip(np.floor(_pass(cur, 0, out_h, False) + 0.5), 0, 255).astype(np.uint8)
    elif cur.dtype != np.uint8:
        cur = np.clip(np.floor(cur + 0.5), 0, 255).astype(np.uint8)
    return np.array(cur, copy=True)


def placement(wr, crop_x, out_w):
    """(left pad, width of the crop window) on one axis: Crop.crop's new_w and CenterPad.center_pad's left."""
    new_w = min(out_w, wr - crop_x)
    return int((out_w - new_w) / 2.0), new_w


def canvas_u8(img, p, out_h, out_w, fill=FILL, rounded_intermediate=True):
    """The uint8 canvas of one image: p has hflip, hr, wr, crop_x, crop_y."""
    src = img[:, ::-1] if p["hflip"] else img
    res = resize_bicubic_u8(src, p["wr"], p["hr"], rounded_intermediate)
    left, new_w = placement(p["wr"], p["crop_x"], out_w)
    top, new_h = placement(p["hr"], p["crop_y"], out_h)
    out = np.empty((out_h, out_w, 3), np.uint8)
    out[:] = np.asarray(fill[:3], np.uint8)
    out[top:top + new_h, left:left + new_w] = res[p["crop_y"]:p["crop_y"] + new_h, p["crop_x"]:p["crop_x"] + new_w]
    return out


def to_tensor(canvas, norm=1, mask=None):
    """[3, H, W] float32: norm 0 = float(u), 1 = ToTensor + Normalize, each fp32 operation rounded on its own; then
    mask = (x0, y0, x1, y1): everything outside [x0, x1) x [y0, y1) is 0 (mask_valid_area runs last)."""
    t = canvas.astype(np.float32).transpose(2, 0, 1)
    if norm:
        t = t / np.float32(255)
        t = t - MEAN[:, None, None]
        t = t / STD[:, None, None]
    t = np.ascontiguousarray(t, np.float32)
    if mask is not None:
        x0, y0, x1, y1 = mask
        keep = np.zeros(t.shape[1:], bool)
        keep[y0:y1, x0:x1] = True
        t[:, ~keep] = 0.0
    return t


def augment(img, p, out_h, out_w, norm=1, mask=None, fill=FILL):
    return to_tensor(canvas_u8(img, p, out_h, out_w, fill), norm, mask)


def synthetic_source(h, w, seed):
    """Smooth plus noise with patches that saturate to 0 and 255."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1)
    img = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    img[h // 8:h // 3, w // 6:w // 2] = 255
    img[h // 2:h // 2 + max(h // 5, 2), w // 3:w // 3 + max(w // 4, 2)] = 0
    img[-max(h // 6, 2):, :max(w // 6, 2)] = 255
    return img


def checkerboard(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
