"""numpy restatement of the JPEG decoder (csrc/jpeg_entropy.cpp, csrc/jpeg_decode.hip, header section 4f): what
``Image.open(f).convert('RGB')`` computes for a baseline JPEG file when Pillow is built on libjpeg-turbo.  A small marker
parser and a bit-serial Huffman decoder (the specification's Annex F, nothing clever: this is the executable contract,
the library's look-ahead tables are tested against it) give the quantised coefficients; jpeg_restate's ``idct``,
``range_limit``, ``upsample`` (h2v2) and ``ycc_to_rgb`` are reused by import, and the three rules that 4:2:0 did not
need are stated here: h2v1 for 4:2:2, h1v2 for 4:4:0, nothing for 4:4:4 and gray.  The library is tested against this
file, this file against Pillow itself (tests/test_jpeg_decode_cpu.py)."""
import io

import numpy as np

import jpeg_restate as jr

MODES = ("gray", "4:4:4", "4:2:2", "4:2:0", "4:4:0")
_MODE_OF = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0", (1, 2): "4:4:0"}

# zig-zag position -> place in the row-major block
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                    7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                    39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Unserved(ValueError):
    """The file is outside the subset of header section 4f."""


def _huffman(counts, vals):
    """Annex C: {(length, code): symbol}."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def parse(data):
    """The markers up to the scan.  -> a dict: width, height, mode, comps [(id, h, v, tq)], qt {t: int64 [64] natural},
    dc / ac {t: table}, restart_interval, scan (td, ta per component), start (offset of the entropy-coded data)."""
    if data[:2] != b"\xff\xd8":
        raise Unserved("no SOI")
    p, out = 2, dict(qt={}, dc={}, ac={}, restart_interval=0)
    while True:
        if data[p] != 0xFF:
            raise Unserved("no marker at %d" % p)
        while data[p] == 0xFF:
            p += 1
        m = data[p]
        p += 1
        n = int.from_bytes(data[p:p + 2], "big")
        seg = data[p + 2:p + n]
        p += n
        if m == 0xC0:
            if seg[0] != 8:
                raise Unserved("precision")
            out["height"], out["width"] = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            out["comps"] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            raise Unserved("frame type %02x" % m)
        elif m == 0xC4:
            while seg:
                counts = list(seg[1:17])
                total = sum(counts)
                (out["ac"] if seg[0] >> 4 else out["dc"])[seg[0] & 15] = _huffman(counts, list(seg[17:17 + total]))
                seg = seg[17 + total:]
        elif m == 0xDB:
            while seg:
                if seg[0] >> 4:
                    raise Unserved("16-bit quantiser table")
                t = np.zeros(64, np.int64)
                t[NATURAL] = list(seg[1:65])
                out["qt"][seg[0] & 15] = t
                seg = seg[65:]
        elif m == 0xDD:
            out["restart_interval"] = int.from_bytes(seg[:2], "big")
        elif m == 0xEE and seg[:5] == b"Adobe":
            raise Unserved("Adobe segment")
        elif m == 0xDA:
            if seg[0] != len(out["comps"]):
                raise Unserved("a scan of some components")
            out["scan"] = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            out["start"] = p
            break
    comps = out["comps"]
    if len(comps) == 1 and comps[0][1:3] == (1, 1):
        out["mode"] = "gray"
    elif len(comps) == 3 and comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1) and comps[0][1:3] in _MODE_OF:
        out["mode"] = _MODE_OF[comps[0][1:3]]
    else:
        raise Unserved("sampling")
    return out


class _Bits:
    def __init__(self, data, p):
        self.data, self.p, self.acc, self.n = data, p, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.data[self.p]
            self.p += 1
            if b == 0xFF:
                if self.data[self.p] != 0:
                    raise Unserved("a marker inside an MCU")
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def receive(self, s):
        v = 0
        for _ in range(s):
            v = v << 1 | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise Unserved("a code in no table")

    def restart(self, number):
        self.n = 0
        while self.data[self.p + 1] == 0xFF:
            self.p += 1
        if self.data[self.p] != 0xFF or self.data[self.p + 1] != 0xD0 + number:
            raise Unserved("wrong RST")
        self.p += 2


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < 1 << (s - 1) else v


def coefficients(data):
    """-> (header, coefs, qtabs): coefs per component int64 [blocks_y, blocks_x, 8, 8] - the quantised coefficients in
    natural order over the MCU-padded block grid, the layout of section 4f -, qtabs per component int64 [64]."""
    hd = parse(data)
    comps = hd["comps"]
    hmax, vmax = comps[0][1], comps[0][2]
    mx, my = -(-hd["width"] // (8 * hmax)), -(-hd["height"] // (8 * vmax))
    coefs = [np.zeros((my * v, mx * h, 64), np.int64) for _, h, v, _ in comps]
    bits = _Bits(data, hd["start"])
    pred = [0] * len(comps)
    interval, done, rst = hd["restart_interval"], 0, 0
    for y in range(my):
        for x in range(mx):
            for c, (_, h, v, _) in enumerate(comps):
                dc, ac = hd["dc"][hd["scan"][c][0]], hd["ac"][hd["scan"][c][1]]
                for j in range(v):
                    for i in range(h):
                        blk = coefs[c][y * v + j, x * h + i]
                        s = bits.symbol(dc)
                        pred[c] += _extend(bits.receive(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[NATURAL[k]] = _extend(bits.receive(s), s)
                            k += 1
            done += 1
            if interval and done % interval == 0 and done < mx * my:
                bits.restart(rst)
                rst = (rst + 1) & 7
                pred = [0] * len(comps)
    coefs = [c.reshape(c.shape[0], c.shape[1], 8, 8) for c in coefs]
    return hd, coefs, [hd["qt"][tq] for _, _, _, tq in comps]


def h2v1_upsample(c, w):
    """jdsample.c h2v1_fancy_upsample on the real plane c [h, ceil(w / 2)] -> [h, w]; h2v1_upsample (box replication)
    where the plane is at most 2 samples wide."""
    if c.shape[1] <= 2:
        return np.repeat(c, 2, 1)[:, :w]
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :w]


def h1v2_upsample(c, h):
    """jdsample.c h1v2_fancy_upsample on the real plane c [ceil(h / 2), w] -> [h, w]; no width condition."""
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    out[0::2] = (3 * c + up + 1) >> 2
    out[1::2] = (3 * c + down + 2) >> 2
    return out[:h]


def planes(hd, coefs, qtabs):
    """De-quantise, inverse DCT, range limit; each component cut to its real plane."""
    h, w = hd["height"], hd["width"]
    hmax, vmax = hd["comps"][0][1], hd["comps"][0][2]
    out = []
    for (_, hs, vs, _), c, q in zip(hd["comps"], coefs, qtabs):
        p = jr._unblocks(jr.idct(c * q.reshape(8, 8)))
        out.append(p[:-(-h * vs // vmax), :-(-w * hs // hmax)])
    return out


def decode(data):
    """bytes of a served JPEG file -> uint8 [h, w, 3]: ``np.asarray(Image.open(f).convert('RGB'))``."""
    hd, coefs, qtabs = coefficients(data)
    h, w, mode = hd["height"], hd["width"], hd["mode"]
    p = planes(hd, coefs, qtabs)
    if mode == "gray":
        return np.repeat(p[0][..., None], 3, -1).astype(np.uint8)
    y, cb, cr = p
    if mode == "4:2:0":
        cb, cr = jr.upsample(cb, h, w), jr.upsample(cr, h, w)
    elif mode == "4:2:2":
        cb, cr = h2v1_upsample(cb, w), h2v1_upsample(cr, w)
    elif mode == "4:4:0":
        cb, cr = h1v2_upsample(cb, h), h1v2_upsample(cr, h)
    return jr.ycc_to_rgb(y, cb, cr)


# ---- the files the tests use --------------------------------------------------------------------------------------------
# (h, w): widths 4 and 5 on both sides of the "at most 2 chroma samples" switch, odd sizes, one MCU up to several MCU rows
SIZES = ((1, 1), (3, 1), (2, 5), (5, 3), (7, 4), (8, 8), (9, 17), (16, 16), (17, 31), (18, 21), (33, 47), (40, 24))
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}          # Pillow's ``subsampling`` keyword
QUALITIES = (1, 10, 50, 75, 95, 100)


def pil_file(img, mode="4:2:0", quality=75, **save):
    """The bytes Pillow writes for ``img`` uint8 [h, w, 3] (gray: its first channel as an 'L' image)."""
    from PIL import Image
    f = io.BytesIO()
    if mode == "gray":
        Image.fromarray(np.ascontiguousarray(img[..., 0])).save(f, "jpeg", quality=int(quality), **save)
    else:
        Image.fromarray(np.ascontiguousarray(img)).save(f, "jpeg", quality=int(quality), subsampling=SUBSAMPLING[mode],
                                                         **save)
    return f.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def grid_file(size, mode, kind, quality, variant=None):
    """One file of the grid: ``variant`` None, 'optimize', 'restart_blocks' or 'restart_rows'."""
    save = {None: {}, "optimize": dict(optimize=True), "restart_blocks": dict(restart_marker_blocks=1),
            "restart_rows": dict(restart_marker_rows=1)}[variant]
    return pil_file(jr.content(kind, size[0], size[1], seed=quality), mode, quality, **save)
