"""The host reference of tests/test_layout_ops_gpu.py (tests/layout_restate.py) checked on the CPU, so that
the reference is not itself the unknown; and the rule that every entry point of the data-movement files
(csrc/layout_ops.hip, shufflenet_ops.hip, image_ops.hip, common.hip and the COCO-18 doors of tta.hip) is named
by a GPU test."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layout_restate as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_bf16_bits(f):
    return torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _not_nan(u):
    return u[(u & 0x7FFFFFFF) <= 0x7F800000]


def test_bf16_rne_equals_torch_bit_for_bit():
    rng = np.random.default_rng(0)
    rnd = _not_nan(rng.integers(0, 2 ** 32, size=2_200_000, dtype=np.uint64).astype(np.uint32))
    assert rnd.size >= 2_000_000
    upper = rng.integers(0, 0x7F7F, size=200_000, dtype=np.uint64).astype(np.uint32)      # finite upper halves
    upper[:100_000] &= 0xFFFE                                                                # even: the tie rounds down
    upper[100_000:] |= 1                                                                     # odd: the tie rounds up
    upper[::2] |= 0x8000                                                                     # both signs
    ties = (upper << 16) | 0x8000
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF,
                        0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x3F7FFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x00008000,
                        0x00018000, 0x7F7F8000], dtype=np.uint32)
    for u in (rnd, ties, special):
        f = u.view(np.float32)
        assert np.array_equal(lr.bf16_rne(f), _torch_bf16_bits(f))
    # the tie rule itself, not only agreement with torch
    t = ties.view(np.float32)
    assert np.array_equal(lr.bf16_rne(t[:100_000]), (ties[:100_000] >> 16).astype(np.uint16))
    assert np.array_equal(lr.bf16_rne(t[100_000:]), ((ties[100_000:] >> 16) + 1).astype(np.uint16))
    h = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(lr.bf16_to_f32(h).view(np.uint32), h.astype(np.uint32) << 16)
    fin = h[(h & 0x7FFF) <= 0x7F80]
    assert np.array_equal(lr.bf16_rne(lr.bf16_to_f32(fin)), fin)                            # bf16 values are fixed points
    k = lr.bf16_key(fin)
    o = np.argsort(lr.bf16_to_f32(fin).astype(np.float64) + np.where(fin == 0x8000, -1e-60, 0), kind="stable")
    assert np.all(np.diff(k[o]) > 0)                                                         # the key orders like the values


def test_split_is_exact_and_16_bits_wide():
    rng = np.random.default_rng(1)
    u = _not_nan(rng.integers(0, 2 ** 32, size=2_000_000, dtype=np.uint64).astype(np.uint32))
    f = u.view(np.float32)
    f = f[np.isfinite(f) & (np.abs(f) < 1e30)]
    f = np.concatenate([f, np.float32([0.0, -0.0, 1.0, -1.0, 1.00390625, 0.99609375, 9.9e29])])
    hi, lo = lr.split(f)
    hf = lr.bf16_to_f32(hi)
    assert np.array_equal((f - hf).astype(np.float64), f.astype(np.float64) - hf.astype(np.float64))   # f - hi exact in fp32
    # lo is rounded to 8 bits of a value <= 2^-9 |f|: an error <= 2^-18 |f| - unless lo is a bf16 subnormal, where the
    # error is up to 2^-134 whatever |f|: inside 2^-17 |f| from |f| >= 2^-117 on (normal f whose lo is not flushed)
    normal = np.abs(f) >= np.float32(2.0 ** -116)
    err = np.abs(hf.astype(np.float64) + lr.bf16_to_f32(lo).astype(np.float64) - f.astype(np.float64))
    assert np.all(err[normal] <= 2.0 ** -17 * np.abs(f[normal].astype(np.float64)))


LAYOUTS = [lr.padded(40, 7, 5, 1, choff=8), lr.padded(64, 7, 5, 3, choff=16), lr.dense(32, 7, 5, choff=0)]


@pytest.mark.parametrize("l", LAYOUTS)
def test_scatter_gather_identity_and_disjoint_index_sets(l):
    n, h, w, c = 3, 7, 5, 16
    rng = np.random.default_rng(2)
    total = lr.pixels(l, n) * l.cstride
    # fp32
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    buf = np.full(total, np.float32(-7.5))
    lr.scatter(buf, l, x)
    assert np.array_equal(lr.gather(buf, l, n, h, w, c), x)
    idx = lr.index(l, n, h, w, c)
    assert idx.min() >= 0 and idx.max() < total and np.unique(idx).size == idx.size
    assert np.array_equal(idx[..., 0], lr.offsets(l, n, h, w))
    assert lr.untouched(buf.view(np.uint32), idx, np.float32(-7.5).view(np.uint32))
    buf2 = buf.copy()
    buf2[idx.max() + 1] = -7.25
    assert not lr.untouched(buf2.view(np.uint32), idx, np.float32(-7.5).view(np.uint32))
    buf2 = buf.copy()
    buf2[0 if idx.min() > 0 else total - 1] = np.float32(7.5)
    assert not lr.untouched(buf2.view(np.uint32), idx, np.float32(-7.5).view(np.uint32))
    # images are disjoint; a slice and its neighbour slice are disjoint
    assert np.intersect1d(idx[0], idx[1]).size == 0 and np.intersect1d(idx[1], idx[2]).size == 0
    if l.choff + 2 * c <= l.cstride:
        nb = lr.index(l._replace(choff=l.choff + c), n, h, w, c)
        assert np.intersect1d(idx, nb).size == 0
    # every pixel (n, y, x) sits at header §1's q = lead + (n * hs + y) * ws + x
    assert lr.offsets(l, n, h, w)[2, 6, 4] == (l.lead + (2 * l.hs + 6) * l.ws + 4) * l.cstride + l.choff
    # bf16 (uint16 elements)
    xb = rng.integers(0, 0x10000, size=(n, c, h, w)).astype(np.uint16)
    bb = np.full(total, 0xBEEF, dtype=np.uint16)
    lr.scatter(bb, l, xb)
    assert np.array_equal(lr.gather(bb, l, n, h, w, c), xb)
    assert lr.untouched(bb, idx, 0xBEEF)


@pytest.mark.parametrize("choff_ch, c", [(0, 16), (8, 19), (166, 19), (3, 5)])
def test_split_scatter_gather_identity(choff_ch, c):
    n, h, w = 2, 5, 4
    cpix = 192                                              # channels per pixel -> 384 elements
    l = lr.Lay(2 * cpix, 2 * choff_ch, w + 1, h + 1, w + 2)
    rng = np.random.default_rng(3)
    hi = rng.integers(0, 0x10000, size=(n, c, h, w)).astype(np.uint16)
    lo = rng.integers(0, 0x10000, size=(n, c, h, w)).astype(np.uint16)
    buf = np.full(lr.pixels(l, n) * l.cstride, 0xBEEF, dtype=np.uint16)
    lr.scatter_split(buf, l, hi, lo)
    gh, gl = lr.gather_split(buf, l, n, h, w, c)
    assert np.array_equal(gh, hi) and np.array_equal(gl, lo)
    ih, il = lr.split_index(l, n, h, w, c)
    both = np.concatenate([ih.ravel(), il.ravel()])
    assert np.unique(both).size == both.size
    # channel ca of a pixel: group ca / 8, hi at 16 * group + ca % 8, lo 8 further
    ca = choff_ch + c - 1
    q = l.lead + (1 * l.hs + 2) * l.ws + 3
    assert ih[1, 2, 3, c - 1] == q * l.cstride + (ca // 8) * 16 + ca % 8 and il[1, 2, 3, c - 1] == ih[1, 2, 3, c - 1] + 8
    # the neighbour slice does not overlap
    l2 = l._replace(choff=2 * (choff_ch + c))
    jh, jl = lr.split_index(l2, n, h, w, 4)
    assert np.intersect1d(both, np.concatenate([jh.ravel(), jl.ravel()])).size == 0
    assert lr.untouched(buf, [ih, il], 0xBEEF)


@pytest.mark.parametrize("shape", [(2, 8, 7, 5), (1, 4, 3, 3), (2, 24, 23, 30), (1, 4, 6, 8), (1, 4, 1, 1)])
def test_arithmetic_references_equal_torch_float64(shape):
    g = torch.Generator().manual_seed(shape[2])
    n, c, h, w = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    if h >= 2 and w >= 2:
        assert torch.equal(lr.maxpool2x2(x), F.max_pool2d(x, 2, 2, 0))
        assert torch.equal(lr.maxpool2x2(-x.abs() - 1), F.max_pool2d(-x.abs() - 1, 2, 2, 0))
    if h >= 3 and w >= 3:
        assert torch.equal(lr.maxpool3x3s2_ceil(x), F.max_pool2d(x, 3, 2, 0, ceil_mode=True))
        xn = -x.abs() - 1
        assert torch.equal(lr.maxpool3x3s2_ceil(xn), F.max_pool2d(xn, 3, 2, 0, ceil_mode=True))
    wt = torch.randn(c, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(c, generator=g, dtype=torch.float64)
    for stride in (1, 2):
        v, s = lr.dwconv3x3(x, wt, b, stride)
        ref = F.conv2d(x, wt.view(c, 1, 3, 3), b, stride, 1, 1, c)
        assert v.shape == ref.shape and (v - ref).abs().max().item() <= 1e-13 * s.max().item()
        sref = F.conv2d(x.abs(), wt.abs().view(c, 1, 3, 3), b.abs(), stride, 1, 1, c)
        assert (s - sref).abs().max().item() <= 1e-13 * s.max().item() and bool((s >= v.abs() - 1e-12).all())
    x3 = torch.randn(n, 3, h, w, generator=g, dtype=torch.float64)
    sc = torch.rand(3, generator=g, dtype=torch.float64) + 0.5
    sh = torch.randn(3, generator=g, dtype=torch.float64) + 40.0    # padding must stay 0 AFTER the affine
    w3 = torch.randn(24, 3, 3, 3, generator=g, dtype=torch.float64)
    b3 = torch.randn(24, generator=g, dtype=torch.float64)
    av, asum = lr.affine(x3, sc, sh)
    assert torch.equal(av, x3 * sc.view(1, 3, 1, 1) + sh.view(1, 3, 1, 1))
    assert torch.equal(asum, (x3 * sc.view(1, 3, 1, 1)).abs() + sh.view(1, 3, 1, 1).abs())
    for relu in (True, False):
        v, s = lr.stem_conv3x3_s2(x3, sc, sh, w3, b3, relu)
        ref = F.conv2d(av, w3, b3, 2, 1)
        ref = F.relu(ref) if relu else ref
        assert v.shape == ref.shape and (v - ref).abs().max().item() <= 1e-13 * s.max().item()
        sref = F.conv2d(asum, w3.abs(), b3.abs(), 2, 1)
        assert (s - sref).abs().max().item() <= 1e-13 * s.max().item()
    v, s = lr.stem_conv3x3_s2(x3, None, None, w3, b3, False)
    assert (v - F.conv2d(x3, w3, b3, 2, 1)).abs().max().item() <= 1e-13 * s.max().item()


def test_flip_merge_and_resize_references():
    from oracle import host_oracle as ho
    g = torch.Generator().manual_seed(4)
    heat, heat_f = (torch.randn(2, 6, 7, 19, generator=g, dtype=torch.float64) for _ in range(2))
    paf, paf_f = (torch.randn(2, 6, 7, 38, generator=g, dtype=torch.float64) for _ in range(2))
    hv, hs_ = lr.flip_merge(heat, heat_f, lr.SWAP_HEAT, False)
    pv, ps_ = lr.flip_merge(paf, paf_f, lr.SWAP_PAF, True)
    for i in range(2):
        ap, ah = ho.handle_paf_and_heat(heat[i].numpy(), heat_f[i].numpy(), paf[i].numpy(), paf_f[i].numpy())
        assert np.array_equal(hv[i].numpy(), ah) and np.array_equal(pv[i].numpy(), ap)
    assert bool((hs_ >= hv.abs() - 1e-15).all()) and bool((ps_ >= pv.abs() - 1e-15).all())
    # half-pixel bilinear == F.interpolate(align_corners=False) where the coordinates are exact
    for (hs, ws, hd, wd) in ((6, 7, 12, 14), (6, 7, 3, 14), (8, 8, 2, 4)):
        src = torch.randn(2, hs, ws, 5, generator=g, dtype=torch.float64)
        assert lr.resize_coords_exact(hd, hs, hs) and lr.resize_coords_exact(wd, ws, ws)
        v, s = lr.resize_bilinear(src, hd, wd, hs, ws)
        ref = F.interpolate(src.permute(0, 3, 1, 2), size=(hd, wd), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert (v - ref).abs().max().item() <= 1e-14 * s.max().item()
    assert not lr.resize_coords_exact(46, 31, 31)
    o, so = lr.accumulate(torch.ones(3, dtype=torch.float64), torch.full((3,), 2.0, dtype=torch.float64),
                          torch.full((3,), 2.0, dtype=torch.float64), 0.5, -3.0)
    assert torch.equal(o, torch.full((3,), -2.0, dtype=torch.float64)) and torch.equal(so, torch.full((3,), 4.0, dtype=torch.float64))
    a, s = lr.axpby(torch.tensor([2.0]), torch.tensor([-3.0]), 0.5, 2.0)
    assert a.item() == -5.0 and s.item() == 7.0


def test_every_layout_ops_entry_point_is_named_by_a_gpu_test():
    csrc = os.path.join(ROOT, "pytorch_realtime_multi-person_pose_estimation_amd", "csrc")
    # the files layout_ops.hip was split into; of tta.hip only the two COCO-18 doors that moved there
    src = "".join(open(os.path.join(csrc, f)).read() for f in ("common.hip", "layout_ops.hip", "shufflenet_ops.hip", "image_ops.hip"))
    names = re.findall(r"^(?:int|size_t|const char\*) (rtpose_\w+)\(", src, flags=re.M)
    names += re.findall(r"^int (rtpose_flip_merge|rtpose_tta_accumulate)\(", open(os.path.join(csrc, "tta.hip")).read(), flags=re.M)
    assert len(names) >= 31 and "rtpose_tta_accumulate" in names and "rtpose_layout_copy_cmap_bf16" in names
    tests = ""
    for p in glob.glob(os.path.join(ROOT, "tests", "test_*_gpu.py")):
        tests += open(p).read()
    missing = [n for n in names if not re.search(r"\b%s\b" % n, tests)]
    assert not missing, "data-movement entry points that no GPU test names: %s" % missing
