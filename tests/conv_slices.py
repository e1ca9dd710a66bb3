"""Input slices of wider pixel buffers for the conv launcher tests (tests/test_conv_slices_cpu.py checks this file on the
CPU, tests/test_conv_input_slices_gpu.py uses it).  Plain torch, any element type, no library call.

A conv launcher reads its input through rtpose_conv_desc.lin (include/rtpose_mi355x.h §1/§2): `cin_e` elements of a pixel
of `cstride` elements, from element `choff` on.  `widen` takes a COMPACT buffer (cstride == cin_e, choff == 0) and returns
the same data as a slice of a wider pixel: same ws / hs / lead and pixel count, cstride = cin_e + extra, the slice at
choff.  The other elements of every REAL pixel (n, y < H, x < W) hold decoys; the gap pixels, the lead and the tail slack
stay zero in every channel - the §1 contract the kernels rely on for their padding taps.

Decoys are finite: +-(2^10 .. 2^11), eight significant bits, so exact in bf16 (and in fp32).  A kernel may fetch a 16-byte
piece it then multiplies by a packed zero weight - a NaN or Inf there would poison a correct result; a finite decoy does
not, and one decoy channel that leaks through a He-scaled weight moves an output by 10^4 times the tolerances in use.
"""
import torch

import layout_restate as lr

# a launcher's input alignment unit in ELEMENTS (16 bytes): fp32, bf16, and the split hi / lo form of bf16x3 (two bf16
# elements per channel: a piece of 8 channels is 16 elements - csrc/conv_mfma_bf16.hip, ConvSpec.align = 8 * sp)
UNIT_F32, UNIT_BF16, UNIT_X3 = 4, 8, 16


def geometries(cin_e, unit):
    """[(name, extra, choff)] in a launcher's alignment unit: the slice in the middle (decoys on both sides), at the end
    (choff + cin_e == cstride) and the dense-block shape (cstride = 3 * cin_e, the slice second of three)."""
    return [("mid", 2 * unit, unit), ("end", unit, unit), ("dense", 2 * cin_e, cin_e)]


def real_pixels(lay, n, h, w):
    """Pixel indices q (§1) of the pixels (n, y < h, x < w), int64 [n * h * w], image-major: layout_restate's arithmetic."""
    return lr.offsets(lr.Lay(1, 0, lay.ws, lay.hs, lay.lead), n, h, w).reshape(-1)


def decoys(shape, gen, dtype):
    """+-(2^10 + 8 * j), j in [0, 128): magnitudes in [2^10, 2^11), exactly representable in bf16."""
    mag = 1024.0 + 8.0 * torch.randint(0, 128, shape, generator=gen).to(torch.float32)
    sign = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=gen).to(torch.float32)
    return (mag * sign).to(dtype)


def widen(compact, lay, n, h, w, extra, choff, seed=0):
    """compact: 1-D buffer of layout `lay` (cstride = cin_e, choff = 0) -> (wide 1-D buffer on the same device, its
    lr.Lay).  lay: anything with cstride / ws / hs / lead."""
    cin_e = lay.cstride
    assert compact.dim() == 1 and compact.numel() % cin_e == 0 and extra >= 0 and 0 <= choff <= extra
    npx = compact.numel() // cin_e
    cs = cin_e + extra
    q = torch.from_numpy(real_pixels(lay, n, h, w)).to(compact.device)
    wide = torch.zeros(npx, cs, dtype=compact.dtype, device=compact.device)
    gen = torch.Generator().manual_seed(1000003 * seed + 131 * extra + choff)
    wide[q] = decoys((q.numel(), cs), gen, compact.dtype).to(compact.device)      # real pixels only
    wide[:, choff:choff + cin_e] = compact.view(npx, cin_e)                        # the slice columns of EVERY pixel
    return wide.reshape(-1), lr.Lay(cs, choff, lay.ws, lay.hs, lay.lead)


def relead(buf, lay, by):
    """The same buffer with `by` more pixels of lead (zeros in front): a second branch's buffer whose pixel (0, 0, 0) sits
    elsewhere.  Returns (buffer, lr.Lay)."""
    z = torch.zeros(by * lay.cstride, dtype=buf.dtype, device=buf.device)
    return torch.cat([z, buf]), lr.Lay(lay.cstride, lay.choff, lay.ws, lay.hs, lay.lead + by)


def scatter_nchw(x, lay, npx, dtype=None):
    """x [n, c, h, w] (CPU) -> compact pixel-major buffer of `npx` pixels, cstride = lay.cstride >= c (the channels behind c
    are zero: the packed zero taps), choff = 0."""
    n, c, h, w = x.shape
    buf = torch.zeros(npx, lay.cstride, dtype=dtype or x.dtype)
    q = torch.from_numpy(real_pixels(lay, n, h, w))
    buf[q, :c] = x.permute(0, 2, 3, 1).reshape(-1, c).to(buf.dtype)
    return buf.reshape(-1)


def slice_of(buf, lay, n, h, w, c):
    """The slice read back through lr.index: [n, c, h, w] (CPU tensor of the buffer's type)."""
    idx = torch.from_numpy(lr.index(lay, n, h, w, c))
    return buf.cpu()[idx].permute(0, 3, 1, 2).contiguous()


# ---- the fp32 cases of tests/test_conv_input_slices_gpu.py (shared with the CPU discrimination check) ----------------------
# (k, wino_m or None = the direct kernel, n, h, w, cin, cout, relu, pool, prelu)
TINY_F32 = [
    (1, None, 3, 7, 5, 32, 19, 0, 0, 0),      # rtpose_conv2d 1x1, 16-channel chunks, a head without ReLU
    (1, None, 1, 5, 9, 24, 8, 1, 0, 0),       # 8-channel chunks
    (3, None, 2, 9, 11, 16, 24, 1, 0, 0),     # 3x3 strips
    (3, None, 1, 12, 16, 16, 16, 1, 1, 0),    # fused pool (2-D tiles)
    (3, None, 2, 9, 11, 16, 24, 0, 0, 1),     # PReLU epilogue
    (7, None, 5, 6, 6, 16, 8, 1, 0, 0),       # 7x7, a strip across images
    (3, 2, 3, 7, 5, 24, 64, 1, 0, 0),         # F(2x2,3x3), three 8-channel chunks
    (3, 2, 5, 6, 6, 32, 40, 1, 1, 0),         # F(2x2,3x3) + pool, wtile strips across images
    (3, 4, 5, 7, 9, 48, 24, 1, 0, 0),         # F(4x4,3x3), pixel-major in and out
] + [(7, m, 5, 6, 7, 16, 128, 1, 0, 0) for m in (4, 6, 8)] + [(7, m, 1, 17, 35, 8, 128, 0, 0, 0) for m in (4, 6, 8)]

# the smallest geometries of the existing case tables (tests/test_conv_gpu.py) that select a launcher's main / persistent
# form: bit identity only, no CPU reference.  (k, wino_m, n, h, w, cin, cout, relu, pool, groups)
# (what each Winograd row of the two tables launches on 256 CUs: tests/wino_cases.py, SLICES)
LARGE_F32 = [
    (3, None, 1, 100, 92, 128, 256, 1, 0, 1),   # direct 3x3: 2-D tiles with ragged right / bottom edges
    (7, None, 1, 70, 66, 128, 128, 1, 0, 1),    # direct 7x7 in 2-D tile mode
    (3, 2, 9, 46, 46, 256, 512, 1, 0, 1),       # F(2x2,3x3): whole 32 x 128 tiles (wino_f32)
    (3, 4, 40, 46, 46, 64, 128, 1, 0, 1),       # F(4x4,3x3): persistent blocks + a round of half tiles
] + [(7, m, 12, 46, 46, 128, 128, 1, 0, 2) for m in (4, 6, 8)]   # F(m,7): two branches; persistent split tiles with a scratch for
#                                                                  m = 4 (336 tiles) and 6 (288); m = 8 is 216 tiles: one block each
