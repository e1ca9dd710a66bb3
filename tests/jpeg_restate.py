"""numpy restatement of the JPEG round trip of the training canvas (csrc/jpeg_roundtrip.hip, header section 4e): what
``Image.save(f, 'jpeg', quality=q)`` followed by ``Image.open(f)`` does to the pixels of an 8-bit RGB image when Pillow
is built on libjpeg-turbo - 4:2:0, the default JDCT_ISLOW, fancy up-sampling.  Huffman coding is lossless, so the pixels
depend on integer arithmetic alone: colour conversion, the edge rules, chroma down-sampling, jfdctint, the quantiser,
jidctint, the range limit, h2v2 up-sampling (the triangle filter, or box replication when the chroma plane is at most
two samples wide) and colour conversion back.  The kernels are tested against this file, this file against Pillow
itself (tests/test_jpeg_cpu.py).  Images are uint8 [h, w, 3] of any size from 1 x 1."""
import numpy as np

from augment_restate import synthetic_source

# the JPEG specification's Annex K tables in natural (row-major) order; a quality-50 file carries exactly these
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)

# jfdctint.c / jidctint.c: FIX(x) at 13 bits
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def D(x, n):
    """libjpeg's DESCALE: an arithmetic shift with rounding."""
    return (x + (1 << (n - 1))) >> n


def quant_tables(quality):
    """jpeg_set_quality(quality, force_baseline): -> (luma, chroma), int64 [64] in natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality %r outside [1, 100]" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def range_limit(x):
    """The post-IDCT range-limit table as a function of the descaled IDCT output x (before the +128 the table folds
    in): sample_range_limit[CENTERJSAMPLE + (x & 1023)].  For x in [-512, 511] this clamps x + 128 to 0..255; beyond
    it wraps."""
    i = np.asarray(x, np.int64) & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


def rgb_to_ycc(img):
    """jccolor.c rgb_ycc_convert: -> (Y, Cb, Cr) int64 [h, w]."""
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert: -> uint8 [h, w, 3]."""
    cb = cb - 128
    cr = cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def _pad_rows(p, rows):
    return np.concatenate([p, np.repeat(p[-1:], rows - p.shape[0], 0)], 0) if rows > p.shape[0] else p


def _pad_cols(p, cols):
    return np.concatenate([p, np.repeat(p[:, -1:], cols - p.shape[1], 1)], 1) if cols > p.shape[1] else p


def downsample(c):
    """jcsample.c h2v2_downsample on a plane of even height and width: the bias alternates 1, 2 along a row."""
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias) >> 2


def padded_planes(img):
    """The three component planes as the forward DCT sees them: full-resolution columns repeated to the MCU width, the
    last row repeated once when h is odd, chroma down-sampled, then every plane's own last row repeated to the MCU
    height.  -> (Y [H, W], Cb [H / 2, W / 2], Cr), H and W multiples of 16."""
    h, w = img.shape[:2]
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    planes = [_pad_rows(_pad_cols(p, W), h + (h & 1)) for p in rgb_to_ycc(img)]
    return _pad_rows(planes[0], H), _pad_rows(downsample(planes[1]), H // 2), _pad_rows(downsample(planes[2]), H // 2)


def _blocks(p):
    """[H, W] -> [H / 8, W / 8, 8, 8]"""
    H, W = p.shape
    return p.reshape(H // 8, 8, W // 8, 8).swapaxes(1, 2)


def _unblocks(b):
    by, bx = b.shape[:2]
    return b.swapaxes(1, 2).reshape(by * 8, bx * 8)


def _fdct_1d(d, first):
    """One pass of jfdctint.c along the last axis; ``first``: the row pass (scaled up by PASS1_BITS)."""
    d = [d[..., k] for k in range(8)]
    tmp0, tmp7 = d[0] + d[7], d[0] - d[7]
    tmp1, tmp6 = d[1] + d[6], d[1] - d[6]
    tmp2, tmp5 = d[2] + d[5], d[2] - d[5]
    tmp3, tmp4 = d[3] + d[4], d[3] - d[4]
    tmp10, tmp13 = tmp0 + tmp3, tmp0 - tmp3
    tmp11, tmp12 = tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (tmp10 + tmp11) << 2 if first else D(tmp10 + tmp11, 2)
    o[4] = (tmp10 - tmp11) << 2 if first else D(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * F_0_541
    o[2] = D(z1 + tmp13 * F_0_765, n)
    o[6] = D(z1 + tmp12 * (-F_1_847), n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F_1_175
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F_0_298, tmp5 * F_2_053, tmp6 * F_3_072, tmp7 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961) + z5, z4 * (-F_0_390) + z5
    o[7] = D(tmp4 + z1 + z3, n)
    o[5] = D(tmp5 + z2 + z4, n)
    o[3] = D(tmp6 + z2 + z3, n)
    o[1] = D(tmp7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks):
    """jfdctint.c on [..., 8, 8] blocks of (sample - 128): rows, then columns.  The result is 8 times the DCT."""
    rows = _fdct_1d(blocks, True)
    return _fdct_1d(rows.swapaxes(-1, -2), False).swapaxes(-1, -2)


def _idct_1d(c, n):
    """One pass of jidctint.c along the last axis, descaled by ``n`` bits."""
    c = [c[..., k] for k in range(8)]
    z2, z3 = c[2], c[6]
    z1 = (z2 + z3) * F_0_541
    tmp2 = z1 + z3 * (-F_1_847)
    tmp3 = z1 + z2 * F_0_765
    tmp0 = (c[0] + c[4]) << 13
    tmp1 = (c[0] - c[4]) << 13
    tmp10, tmp13 = tmp0 + tmp3, tmp0 - tmp3
    tmp11, tmp12 = tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298, tmp1 * F_2_053, tmp2 * F_3_072, tmp3 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961) + z5, z4 * (-F_0_390) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([D(v, n) for v in o], -1)


def idct(coefs):
    """jidctint.c on de-quantised [..., 8, 8] blocks: columns, then rows, then the range limit.  -> samples 0..255."""
    cols = _idct_1d(coefs.swapaxes(-1, -2), 11).swapaxes(-1, -2)
    return range_limit(_idct_1d(cols, 18))


def quantise(coefs, table):
    """jcdctmgr.c's quantiser on fdct's output (divisors Q * 8) followed by the decoder's de-quantisation."""
    q8 = table.reshape(8, 8) * 8
    a = (np.abs(coefs) + (q8 >> 1)) // q8
    return np.where(coefs < 0, -a, a) * table.reshape(8, 8)


def codec_plane(p, table):
    """A padded component plane through fdct, the quantiser and idct."""
    return _unblocks(idct(quantise(fdct(_blocks(p - 128)), table)))


def upsample(c, h, w):
    """jdsample.c on the real chroma plane c [ceil(h / 2), ceil(w / 2)] -> [h, w]: h2v2_fancy_upsample (the triangle
    filter: 3/4 nearer, 1/4 further sample each way, the missing neighbour at an edge being the sample itself), or, when
    the plane is at most 2 samples wide, h2v2_upsample (box replication)."""
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w]
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2] = 3 * c + up
    s[1::2] = 3 * c + down
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:h, :w]


def decoded_planes(img, quality):
    """-> (Y [h, w], Cb [ceil(h / 2), ceil(w / 2)], Cr): the 8-bit planes the decoder's IDCT leaves, cut to their real
    sizes - what the codec kernel stores in the workspace."""
    h, w = img.shape[:2]
    ql, qc = quant_tables(quality)
    y, cb, cr = padded_planes(np.asarray(img))
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return codec_plane(y, ql)[:h, :w], codec_plane(cb, qc)[:ch, :cw], codec_plane(cr, qc)[:ch, :cw]


def roundtrip(img, quality=50):
    """uint8 [h, w, 3] -> uint8 [h, w, 3]: save as JPEG at ``quality`` and re-open."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or min(img.shape[:2]) < 1:
        raise ValueError("an uint8 [h, w, 3] image of at least 1 x 1")
    h, w = img.shape[:2]
    y, cb, cr = decoded_planes(img, quality)
    return ycc_to_rgb(y, upsample(cb, h, w), upsample(cr, h, w))


def pil_roundtrip(img, quality=50):
    """The same through Pillow itself: transforms.py:28-31 of the reference at ``quality``."""
    import io
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(f, "jpeg", quality=int(quality))
    return np.asarray(Image.open(f).convert("RGB"))


# ---- the four kinds of content the tests use ------------------------------------------------------------------------
def content(kind, h, w, seed=0):
    """uint8 [h, w, 3]: 'noise' uniform, 'binary' 0 / 255 per channel, 'ramp' smooth gradients, 'patches' the saturating
    patches of augment_restate.synthetic_source (hard edges: the IDCT overshoots the 0..255 range there)."""
    rng = np.random.default_rng([seed, h, w, len(kind)])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        r = x * 255 // max(w - 1, 1)
        g = y * 255 // max(h - 1, 1)
        b = (x + y) * 255 // max(h + w - 2, 1)
        return np.stack([r, g, 255 - b], -1).astype(np.uint8)
    if kind == "patches":
        return synthetic_source(h, w, seed)
    raise ValueError(kind)


KINDS = ("noise", "binary", "ramp", "patches")
