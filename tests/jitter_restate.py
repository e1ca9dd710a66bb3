"""numpy restatement of the colour jitter (csrc/colorjitter.hip, header section 4d): torchvision's ColorJitter and
RandomGrayscale on an 8-bit RGB PIL image, i.e. Pillow's ImageEnhance.Brightness / Contrast / Color over Image.blend,
convert('L'), convert('HSV') and convert('RGB'), each operation in the number format Pillow's C uses for it.  numpy
rounds every fp32 / fp64 operation on its own, as the kernel does under -ffp-contract=off.  The kernel is tested against
this file, this file against Pillow itself (tests/test_jitter_cpu.py).  Images are uint8 [h, w, 3] (or any [..., 3]).
"""
import numpy as np

from augment_restate import to_tensor

SLAB = 2048              # RTPOSE_JITTER_SLAB
MAX_SLABS = 1024
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32, F64 = np.float32, np.float64


def slab_geometry(h, w):
    """(pixels per slab, slabs) of an h x w canvas: equal multiples of SLAB pixels, at most MAX_SLABS of them."""
    pixels = h * w
    per = SLAB * MAX_SLABS
    slab = SLAB * ((pixels + per - 1) // per)
    return slab, (pixels + slab - 1) // slab


def read_u8(src):
    """What the kernel makes of a source float: (int)v clamped to 0..255, NaN -> 0."""
    v = np.asarray(src, F32)
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, np.minimum(np.where(np.isnan(v), 0, v), 255), 0).astype(np.int32).astype(np.uint8)


def luma(img):
    """convert('L') of RGB: (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16."""
    p = np.asarray(img).astype(np.int64)
    return ((p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, x, alpha):
    """ImagingBlend(degenerate d, image x, alpha) on uint8 arrays (broadcast): t = d + alpha * (x - d) in three fp32
    operations; alpha in [0, 1]: (uint8)(int)t; otherwise clipped to 0..255 before the truncation."""
    a = F32(alpha)
    fd, fx = np.asarray(d).astype(F32), np.asarray(x).astype(F32)
    diff = (fx - fd).astype(F32)
    scaled = (a * diff).astype(F32)
    t = (fd + scaled).astype(F32)
    if F32(0) <= a <= F32(1):
        return (t.astype(np.int32) & 255).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def brightness(img, factor):
    return blend(np.uint8(0), img, factor)


def saturation(img, factor):
    return blend(luma(img)[..., None], img, factor)


def contrast_mean(img):
    """ImageEnhance.Contrast's int(ImageStat.Stat(convert('L')).mean[0] + 0.5): an integer sum, one fp64 division."""
    lum = luma(img)
    return int(float(int(lum.astype(np.int64).sum())) / float(lum.size) + 0.5)


def contrast(img, factor, mean=None):
    m = contrast_mean(img) if mean is None else mean
    return blend(np.uint8(m), img, factor)


def _clip8(v):
    return np.clip(v, 0, 255)


def rgb_to_hsv(img):
    """Pillow's rgb2hsv_row: uint8 [..., 3] -> uint8 [..., 3] (H, S, V)."""
    p = np.asarray(img).astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    maxc, minc = p.max(-1), p.min(-1)
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc = (maxc - r).astype(F32) / cr
        gc = (maxc - g).astype(F32) / cr
        bc = (maxc - b).astype(F32) / cr
        h_r = bc - gc                                                    # fp32
        h_g = ((F64(2.0) + rc.astype(F64)) - bc.astype(F64)).astype(F32)  # fp64, rounded to fp32
        h_b = ((F64(4.0) + gc.astype(F64)) - rc.astype(F64)).astype(F32)
        h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b)).astype(F32)
        h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
        hh = _clip8((h.astype(F64) * 255.0).astype(np.int64))
        ss = _clip8((s.astype(F64) * 255.0).astype(np.int64))
    out = np.empty(p.shape, np.uint8)
    out[..., 0] = np.where(grey, 0, hh)
    out[..., 1] = np.where(grey, 0, ss)
    out[..., 2] = maxc
    return out


def _c_round(v):
    """C's round(): half away from zero."""
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def hsv_to_rgb(hsv):
    """Pillow's hsv2rgb: uint8 [..., 3] (H, S, V) -> uint8 [..., 3]."""
    q = np.asarray(hsv)
    hh, ss, vv = q[..., 0], q[..., 1], q[..., 2]
    hf = hh.astype(F32).astype(F64) * 6.0 / 255.0
    fl = np.floor(hf)
    i = fl.astype(np.int64) % 6
    f = (hf - fl).astype(F32)
    fs = (ss.astype(F64) / 255.0).astype(F32)
    v = vv.astype(F64)
    fsf = (fs * f).astype(F32)                                           # float * float stays fp32 in C
    p_ = _clip8(_c_round(v * (1.0 - fs.astype(F64)))).astype(np.uint8)
    q_ = _clip8(_c_round(v * (1.0 - fsf.astype(F64)))).astype(np.uint8)
    t_ = _clip8(_c_round(v * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64))))).astype(np.uint8)
    table = ((vv, t_, p_), (q_, vv, p_), (p_, vv, t_), (p_, q_, vv), (t_, p_, vv), (vv, p_, q_))
    out = np.empty(q.shape, np.uint8)
    for ch in range(3):
        out[..., ch] = np.where(ss == 0, vv, np.choose(i, [row[ch] for row in table]))
    return out


def hue(img, shift):
    """torchvision's adjust_hue on a PIL image: convert('HSV'), H += shift modulo 256, convert('RGB') - always."""
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def grayscale(img):
    return np.repeat(luma(img)[..., None], 3, -1)


def jitter_u8(img, p):
    """The uint8 image after the operations of p['order'] (-1 = unused) and RandomGrayscale.  p: order, factor (three
    numbers: brightness, contrast, saturation), hue_shift, gray."""
    cur = np.array(img, dtype=np.uint8, copy=True)
    for op in p["order"]:
        if op == BRIGHTNESS:
            cur = brightness(cur, p["factor"][0])
        elif op == CONTRAST:
            cur = contrast(cur, p["factor"][1])
        elif op == SATURATION:
            cur = saturation(cur, p["factor"][2])
        elif op == HUE:
            cur = hue(cur, p["hue_shift"])
    if p.get("gray"):
        cur = grayscale(cur)
    return cur


def jitter(img, p, norm=1, mask=None):
    """[3, h, w] float32: jitter_u8, then ToTensor + Normalize (norm 1) or float(u) (norm 0), then the mask."""
    return to_tensor(jitter_u8(img, p), norm, mask)


def as_planes(img):
    """uint8 [h, w, 3] -> the fp32 [3, h, w] the device call reads."""
    return np.ascontiguousarray(np.asarray(img).astype(F32).transpose(2, 0, 1))


# ---- the cases both suites use -----------------------------------------------------------------------------------------
BLEND_FACTORS = (0.9, 1.0, 1.1, 0.0, 0.5, 1.5, 2.0) + tuple(
    float(v) for v in np.random.default_rng(25).uniform(0.9, 1.1, 6).astype(F32))


def grey(values, shape):
    """A grey uint8 [h, w, 3] image of `values`: L of a grey pixel is its value."""
    v = np.asarray(values, np.uint8).reshape(shape)
    return np.repeat(v[..., None], 3, -1)


def contrast_mean_cases():
    """[(name, uint8 image, the mean ImageEnhance.Contrast must blend with)]: 16 x 16 images holding all 256 values,
    shifted so the mean takes several values; images whose L-mean is exactly k + 0.5 (rounds up) and the nearest value
    below it (rounds down)."""
    cases = []
    for shift in (0, -40, 3, 77, 200):
        vals = np.clip(np.arange(256) + shift, 0, 255)
        cases.append(("all256%+d" % shift, grey(np.random.default_rng(shift + 300).permutation(vals), (16, 16)),
                      int(vals.sum() / 256 + 0.5)))
    cases.append(("two_pixels_10_11", grey([10, 11], (1, 2)), 11))
    cases.append(("half_64_64", grey([10] * 64 + [11] * 64, (2, 64)), 11))
    cases.append(("below_half_65_63", grey([10] * 65 + [11] * 63, (2, 64)), 10))
    cases.append(("half_odd_k", grey([200] * 3 + [201] * 3, (3, 2)), 201))
    cases.append(("below_half_odd_k", grey([200] * 4 + [201] * 2 + [200], (1, 7)), 200))
    return cases
