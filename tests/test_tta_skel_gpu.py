"""Flip merge and fused multi-scale TTA over a skeleton's flip table (csrc/tta.hip) on the MI355X.

Method as in tests/test_layout_ops_gpu.py: sources are built on the host with the header's addressing formula - the
network's padded views with cstride > C and choff != 0, every word outside the view a NaN - destinations are sentinel
words of exactly the needed size plus a guard region, and results are compared bit for bit wherever the arithmetic is
pinned:

  1. rtpose_flip_merge_skel against fp32 host arithmetic, (a + s * g) / 2 with one rounded add;
  2. both `_skel` entries with the table skeleton.COCO18 packs against rtpose_flip_merge / rtpose_tta_accumulate, which run
     the same kernels over the table the library derives for itself: the two tables must be one;
  3. rtpose_tta_accumulate_skel against rtpose_flip_merge_skel followed by rtpose_resize_bilinear_accum;
  4. the fused result against the float64 restatement within n * 2^-24 * (sum of magnitudes), n = 12 roundings for the
     resize and 13 with the flip average in front - the count tests/test_layout_ops_gpu.py uses for the COCO-18 kernel;
  5. refusals before any launch; the empty batch;
  6. uint8 image -> BODY_25 maps with TTA -> decode, over OpenPose_Model(4, 2, 52, 26);
  7. skeleton=COCO18 on rtpose_vgg gives the bits of the call without a skeleton: None means COCO-18, 38 / 19 channels.

Tables: COCO-18, BODY_25, a 3-part table whose limb mirrors onto a limb walked backwards, 32 parts / 32 limbs / 64
scattered channels with an explicit mirror, 2 parts / 1 limb without background (tests/tta_skel_restate.py).
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_restate as lr  # noqa: E402
import tta_skel_restate as tr  # noqa: E402

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC12345          # a quiet NaN with a payload: no kernel here produces it
GUARD = 256                  # words behind each destination that must stay untouched
U24 = 2.0 ** -24
INVAL = -1
B, HS, WST, WV = 2, 5, 9, 7  # images per half batch, map rows, stored width, valid width
DESTS = [(5, 7), (6, 11)]    # identity zoom; a zoom with fractional coordinates


@pytest.fixture(scope="module")
def skm(pkg):
    return importlib.import_module(pkg.__name__ + ".skeleton")


@pytest.fixture(scope="module")
def tables(skm, capi):
    """name -> (Skeleton, rtpose_flip_table, (heat_src, paf_src, paf_sign))"""
    out = {}
    for name in tr.TABLE_NAMES:
        s = tr.make(skm, name)
        out[name] = (s, s.native_flip_table(), s.flip_tables())
    return out


def _up(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dev)


def _sent(words, dev):
    return torch.full((int(words) + GUARD,), SENT32, dtype=torch.int32, device=dev)


def _down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _owned(bits, words, what):
    """The first `words` words of a sentinel buffer, after checking that all of them were written and none behind."""
    assert np.all(bits[words:] == SENT32), "%s: written behind the destination" % what
    assert not np.any(bits[:words] == SENT32), "%s: words of the destination were left unwritten" % what
    return bits[:words]


def _dense_maps(n, h, w, c, seed):
    return np.random.default_rng(seed).standard_normal((n, h, w, c)).astype(np.float32)


# ---- 1. flip merge against fp32 host arithmetic -------------------------------------------------------------------------
@pytest.mark.parametrize("w", [5, 4])
@pytest.mark.parametrize("name", tr.TABLE_NAMES)
def test_flip_merge_skel_is_the_fp32_host_arithmetic(capi, cuda, tables, name, w):
    s, table, (heat_src, paf_src, paf_sign) = tables[name]
    n, h, ch, cp = 2, 3, s.heat_channels, s.paf_channels
    heat, heat_f = _dense_maps(n, h, w, ch, 1), _dense_maps(n, h, w, ch, 2)
    paf, paf_f = _dense_maps(n, h, w, cp, 3), _dense_maps(n, h, w, cp, 4)
    dev = [_up(a, cuda) for a in (heat, heat_f, paf, paf_f)]
    oh, op = _sent(heat.size, cuda), _sent(paf.size, cuda)
    p = capi.ptr
    capi.check(capi.lib.rtpose_flip_merge_skel(p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), n, h, w, p(oh), p(op),
                                               C.byref(table), capi.current_stream()), "rtpose_flip_merge_skel")
    got_h, got_p = _owned(_down(oh), heat.size, "heat"), _owned(_down(op), paf.size, "paf")
    assert np.array_equal(got_h, tr.flip_merge_f32(heat, heat_f, heat_src, [1] * ch).ravel())
    assert np.array_equal(got_p, tr.flip_merge_f32(paf, paf_f, paf_src, paf_sign).ravel())


# ---- the network's views ----------------------------------------------------------------------------------------------
def _views(ch, cp, seed):
    """Two buffers as a net could write them: 2B images, HS x WST maps behind a gap of 3, the heat map at channel 3 of
    ch + 5, the PAF at channel 4 of cp + 7; every word outside the two views is a NaN.
    -> (heat buffer, heat layout, paf buffer, paf layout, heat NHWC [2B,HS,WST,ch], paf NHWC)."""
    lh, lp = lr.padded(ch + 5, HS, WST, 3, 3), lr.padded(cp + 7, HS, WST, 3, 4)
    rng = np.random.default_rng(seed)
    heat = (rng.random((2 * B, ch, HS, WST)) - 0.2).astype(np.float32)
    paf = rng.standard_normal((2 * B, cp, HS, WST)).astype(np.float32)
    bh = np.full(lr.pixels(lh, 2 * B) * lh.cstride, np.nan, dtype=np.float32)
    bp = np.full(lr.pixels(lp, 2 * B) * lp.cstride, np.nan, dtype=np.float32)
    lr.scatter(bh, lh, heat)
    lr.scatter(bp, lp, paf)
    t = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))
    return bh, lh, bp, lp, t(heat), t(paf)


def _acc(dev, n, hd, wd, c, beta, seed):
    """An accumulator of exactly n * hd * wd * c words + guard: random values if it is read (beta != 0), else the
    sentinel NaN, which `beta == 0` must overwrite without reading."""
    words = n * hd * wd * c
    a0 = np.random.default_rng(seed).standard_normal(words).astype(np.float32)
    buf = np.full(words + GUARD, SENT32, dtype=np.uint32)
    if beta != 0:
        buf[:words] = a0.view(np.uint32)
    return _up(buf, dev), a0.reshape(n, hd, wd, c)


def _L(capi, l):
    return C.byref(capi.Layout(*l))


def _fused(capi, cuda, table, src_h, lh, src_p, lp, ch, cp, hd, wd, alpha, beta, flip, old=False):
    fh, h0 = _acc(cuda, B, hd, wd, ch, beta, 11)
    fp, p0 = _acc(cuda, B, hd, wd, cp, beta, 12)
    p = capi.ptr
    args = (p(src_h), _L(capi, lh), p(src_p), _L(capi, lp), B, HS, WV, p(fh), p(fp), hd, wd, float(HS), float(WV), alpha,
            beta, flip)
    if old:
        capi.check(capi.lib.rtpose_tta_accumulate(*args, capi.current_stream()), "rtpose_tta_accumulate")
    else:
        capi.check(capi.lib.rtpose_tta_accumulate_skel(*args, C.byref(table), capi.current_stream()),
                   "rtpose_tta_accumulate_skel")
    return (_owned(_down(fh), B * hd * wd * ch, "heat accumulator"), _owned(_down(fp), B * hd * wd * cp, "paf accumulator"),
            h0, p0)


# ---- 2. the COCO-18 table gives the old entry points' bits ------------------------------------------------------------------
@pytest.mark.parametrize("w", [5, 4])
def test_coco18_table_flip_merge_equals_the_old_entry(capi, cuda, tables, w):
    """One kernel serves both doors, so this no longer compares two kernels: it guards that the table the library derives
    for rtpose_flip_merge (coco18_skeleton() and the part mirror in csrc/tta.hip) is the one skeleton.COCO18 packs.
    tests/test_decode_gpu.py::test_flip_merge pins the old door to the reference's recorded bits independently."""
    _, table, _ = tables["coco18"]
    n, h = 2, 3
    maps = [_up(_dense_maps(n, h, w, c, 20 + i), cuda) for i, c in enumerate((19, 19, 38, 38))]
    p = capi.ptr
    out = []
    for new in (False, True):
        oh, op = _sent(n * h * w * 19, cuda), _sent(n * h * w * 38, cuda)
        args = (p(maps[0]), p(maps[1]), p(maps[2]), p(maps[3]), n, h, w, p(oh), p(op))
        if new:
            capi.check(capi.lib.rtpose_flip_merge_skel(*args, C.byref(table), capi.current_stream()))
        else:
            capi.check(capi.lib.rtpose_flip_merge(*args, capi.current_stream()))
        out.append((_owned(_down(oh), n * h * w * 19, "heat"), _owned(_down(op), n * h * w * 38, "paf")))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("dest", DESTS, ids=["5x7", "6x11"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("flip", [0, 1])
def test_coco18_table_tta_equals_the_old_entry(capi, cuda, tables, flip, beta, dest):
    """As above for the fused kernel: rtpose_tta_accumulate's derived table against skeleton.COCO18's, through views with
    choff != 0 and cstride > C.  tests/test_layout_ops_gpu.py pins the old door to flip merge + resize independently."""
    _, table, _ = tables["coco18"]
    bh, lh, bp, lp, _, _ = _views(19, 38, 30)
    sh, sp = _up(bh, cuda), _up(bp, cuda)
    hd, wd = dest
    old = _fused(capi, cuda, table, sh, lh, sp, lp, 19, 38, hd, wd, 0.25, beta, flip, old=True)
    new = _fused(capi, cuda, table, sh, lh, sp, lp, 19, 38, hd, wd, 0.25, beta, flip)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])


# ---- 3. / 4. fused == flip merge then resize, and the float64 bound ------------------------------------------------------------
@pytest.mark.parametrize("dest", DESTS, ids=["5x7", "6x11"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name", tr.TABLE_NAMES)
def test_tta_accumulate_skel_is_flip_merge_skel_then_resize(capi, cuda, tables, name, flip, beta, dest):
    """Bit for bit, for every table.  For BODY_25 and the 64-channel table the 6 x 11 result (fractional coordinates; the
    library is built without floating-point contraction, so tests/layout_restate.py's fp32 coordinates are the
    kernel's) must also lie within (13 with the flip average, else 12) * 2^-24 * the restatement's sum of magnitudes."""
    s, table, (heat_src, paf_src, paf_sign) = tables[name]
    ch, cp = s.heat_channels, s.paf_channels
    hd, wd = dest
    alpha = 0.25
    bh, lh, bp, lp, heat, paf = _views(ch, cp, 40 + ch)
    sh, sp = _up(bh, cuda), _up(bp, cuda)
    fused_h, fused_p, h0, p0 = _fused(capi, cuda, table, sh, lh, sp, lp, ch, cp, hd, wd, alpha, beta, flip)
    # the two-launch form on dense copies of the valid columns
    dense_h, dense_p = np.ascontiguousarray(heat[:, :, :WV]), np.ascontiguousarray(paf[:, :, :WV])
    p = capi.ptr
    if flip:
        d = [_up(a, cuda) for a in (dense_h[:B], dense_h[B:], dense_p[:B], dense_p[B:])]
        mh, mp = _sent(B * HS * WV * ch, cuda), _sent(B * HS * WV * cp, cuda)
        capi.check(capi.lib.rtpose_flip_merge_skel(p(d[0]), p(d[1]), p(d[2]), p(d[3]), B, HS, WV, p(mh), p(mp), C.byref(table),
                                                   capi.current_stream()), "rtpose_flip_merge_skel")
    else:
        mh, mp = _up(dense_h[:B], cuda), _up(dense_p[:B], cuda)
    for c, m, fused, seed in ((ch, mh, fused_h, 11), (cp, mp, fused_p, 12)):
        two, _ = _acc(cuda, B, hd, wd, c, beta, seed)
        capi.check(capi.lib.rtpose_resize_bilinear_accum(p(m), HS, WV, p(two), hd, wd, c, B, float(HS), float(WV), alpha, beta,
                                                         capi.current_stream()), "rtpose_resize_bilinear_accum")
        got = _owned(_down(two), B * hd * wd * c, "two-launch accumulator")
        diff = np.flatnonzero(got != fused)
        assert diff.size == 0, "C=%d: %d of %d words differ between the fused and the two-launch form" % (c, diff.size, got.size)
    if name not in ("body25", "full32") or dest != (6, 11):
        return
    for c, dense, src, sign, fused, a0 in ((ch, dense_h, heat_src, [1] * ch, fused_h, h0),
                                           (cp, dense_p, paf_src, paf_sign, fused_p, p0)):
        if flip:
            v, _ = tr.flip_merge(dense[:B], dense[B:], src, sign)
        else:
            v = torch.from_numpy(dense[:B]).to(torch.float64)
        rv, rs = lr.resize_bilinear(v, hd, wd, float(HS), float(WV))
        ref, smag = lr.accumulate(torch.from_numpy(a0), rv, rs, float(np.float32(alpha)), float(np.float32(beta)))
        g = fused.view(np.float32).astype(np.float64).reshape(B, hd, wd, c)
        err = np.abs(g - ref.numpy())
        bound = (13 if flip else 12) * U24 * smag.numpy()
        print("%s C=%d flip=%d beta=%g: worst error / bound %.3f" % (name, c, flip, beta,
                                                                      float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound), "accumulate %s C=%d flip=%d" % (name, c, flip)


# ---- 5. refusals and the empty batch -----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(capi, cuda, tables, skm):
    lib, p, s = capi.lib, capi.ptr, capi.current_stream()
    _, table, _ = tables["body25"]
    ch, cp = 26, 52
    bh, lh, bp, lp, _, _ = _views(ch, cp, 50)
    sh, sp = _up(bh, cuda), _up(bp, cuda)
    ah, ap = _sent(B * 5 * 7 * ch, cuda), _sent(B * 5 * 7 * cp, cuda)
    dh = _up(_dense_maps(2, 3, 5, ch, 51), cuda)
    dp = _up(_dense_maps(2, 3, 5, cp, 52), cuda)
    T = C.byref(table)

    def tta(heat=p(sh), lheat=lh, paf=p(sp), lpaf=lp, b=B, wv=WV, acc_h=p(ah), acc_p=p(ap), t=T):
        return lib.rtpose_tta_accumulate_skel(heat, _L(capi, lheat), paf, _L(capi, lpaf), b, HS, wv, acc_h, acc_p, 5, 7, 5.0, 7.0,
                                              1.0, 0.0, 1, t, s)

    def merge(heat=p(dh), heat_f=p(dh), paf=p(dp), paf_f=p(dp), n=2, out_h=p(ah), out_p=p(ap), t=T):
        return lib.rtpose_flip_merge_skel(heat, heat_f, paf, paf_f, n, 3, 5, out_h, out_p, t, s)

    def edited(**kw):
        t = skm.BODY_25.native_flip_table()
        for k, v in kw.items():
            setattr(t, k, v)
        return C.byref(t)
    not_involution = skm.BODY_25.native_flip_table()
    not_involution.paf_src[0] = 2
    bad = {
        "tta NULL heat": lambda: tta(heat=None),
        "tta NULL paf": lambda: tta(paf=None),
        "tta NULL accumulator": lambda: tta(acc_p=None),
        "tta NULL table": lambda: tta(t=None),
        "tta w_valid 0": lambda: tta(wv=0),
        "tta w_valid above the stored width": lambda: tta(wv=lh.ws + 1),
        "tta paf view too narrow": lambda: tta(lpaf=lp._replace(choff=lp.cstride - cp + 1)),
        "tta heat view too narrow": lambda: tta(lheat=lh._replace(cstride=ch + 2)),
        "tta table fails the check": lambda: tta(t=C.byref(not_involution)),
        "tta struct_bytes": lambda: tta(t=edited(struct_bytes=C.sizeof(capi.FlipTable) + 8)),
        "merge NULL map": lambda: merge(paf_f=None),
        "merge NULL output": lambda: merge(out_h=None),
        "merge NULL table": lambda: merge(t=None),
        "merge table fails the check": lambda: merge(t=C.byref(not_involution)),
        "merge struct_bytes": lambda: merge(t=edited(struct_bytes=0)),
        "merge paf_channels 65": lambda: merge(t=edited(paf_channels=65)),
    }
    for name, f in bad.items():
        assert f() == INVAL, "%s: expected RTPOSE_E_INVAL" % name
        assert capi.last_error() != "", name
    assert tta(b=0) == 0 and merge(n=0) == 0
    torch.cuda.synchronize()
    assert np.all(_down(ah) == SENT32) and np.all(_down(ap) == SENT32), "a refused or empty call wrote something"


# ---- 6. uint8 images -> BODY_25 people with TTA ---------------------------------------------------------------------------
def test_body25_tta_end_to_end(pkg, capi, cuda, skm):
    """OpenPose_Model(4, 2, 52, 26) with seeded weights, a 92 x 115 image, IMAGE_SIZE 368: the two passes are 184 x 230
    (zoom 2) and 368 x 460 (zoom 4), so resize(mirror(img)) == mirror(resize(img)) exactly (powers of two).
    IMAGE_SIZE 184 (passes of 92 x 115 and 184 x 230) has exact zooms too but cannot show equivariance: its half-scale
    map is ceil(115 / 8) = 15 cells wide, of which the resize to the 29-cell scale-1 map takes 29 / 2 = 14.5, so mirroring
    inside 15 cells and resizing do not commute - for any table, COCO-18's included.  At 368 the widths are 29 = 58 / 2 and
    58: the sizes of tests/test_dropin_gpu.py's COCO-18 equivariance check."""
    import openpose_restate as R
    op = importlib.import_module(pkg.__name__ + ".openpose")
    pre = importlib.import_module(pkg.__name__ + ".preprocess")
    dec = importlib.import_module(pkg.__name__ + ".decode")
    model = op.OpenPose_Model(4, 2, 52, 26)
    model.load_state_dict(R.seeded_state_dict(R.state_dict_spec(4, 2, 52, 26), 3))
    model = model.cuda().eval()
    sk = skm.BODY_25
    cfg = dec.default_config(sk)
    assert cfg.DATASET.IMAGE_SIZE == 368
    img = np.random.default_rng(61).integers(0, 256, (92, 115, 3), dtype=np.uint8)
    mir = np.ascontiguousarray(img[:, ::-1])
    kw = dict(scales=(0.5, 1.0), config=cfg, skeleton=sk)
    with torch.no_grad():
        paf_b, heat_b, s_b = pre.get_multiscale_outputs_batch([img, mir], model, 'rtpose', flip=True, **kw)
        paf_n, heat_n, s_n = pre.get_multiscale_outputs(img, model, 'rtpose', flip=True, **kw)
        paf_f, heat_f, _ = pre.get_multiscale_outputs(mir, model, 'rtpose', flip=True, **kw)
        paf_u, heat_u, _ = pre.get_multiscale_outputs(img, model, 'rtpose', flip=False, **kw)
        paf_uf, heat_uf, _ = pre.get_multiscale_outputs(mir, model, 'rtpose', flip=False, **kw)
    assert s_b == s_n == 4.0 and paf_n.shape == (46, 58, 52) and heat_n.shape == (46, 58, 26)
    assert tuple(paf_b.shape) == (2, 46, 58, 52) and tuple(heat_b.shape) == (2, 46, 58, 26) and paf_b.is_cuda
    scale = max(1.0, float(np.abs(paf_n).max()))
    print("body25 tta: |paf|max %.4f |heat|max %.4f" % (np.abs(paf_n).max(), np.abs(heat_n).max()))
    # batched == per image (test_multiscale_batch_matches_per_image's tolerance)
    for i, (pp, hh) in enumerate(((paf_n, heat_n), (paf_f, heat_f))):
        dp_, dh_ = np.abs(paf_b[i].cpu().numpy() - pp).max(), np.abs(heat_b[i].cpu().numpy() - hh).max()
        print("batched vs per image %d: paf %.3g heat %.3g (bound %.3g)" % (i, dp_, dh_, 2e-6 * scale))
        assert dp_ <= 2e-6 * scale and dh_ <= 2e-6 * scale
    # TTA of the mirrored image == the table-mirrored TTA of the image
    mir_h, mir_p = tr.mirror_maps(heat_f, paf_f, sk.flip_tables())
    dp_, dh_ = np.abs(paf_n - mir_p).max(), np.abs(heat_n - mir_h).max()
    print("equivariance: paf %.3g heat %.3g (bound %.3g)" % (dp_, dh_, 2e-5 * scale))
    assert dp_ <= 2e-5 * scale and dh_ <= 2e-5 * scale
    # ... which a single un-flipped pass is not
    _, mir_u = tr.mirror_maps(heat_uf, paf_uf, sk.flip_tables())
    du = np.abs(paf_u - mir_u).max()
    print("un-flipped passes differ by %.3g" % du)
    assert du > 1e-2
    # the merged device maps decode as BODY_25
    recs = dec.decode_maps(heat_b, paf_b, config=cfg, skeleton=sk)
    assert len(recs) == 2 and all(r["num_parts"] == 25 and r["parts"].shape[1] == 25 for r in recs)
    # handle_paf_and_heat with the skeleton: the host-side door to the same kernel
    rng = np.random.default_rng(62)
    maps = [rng.standard_normal((4, 6, c)).astype(np.float32) for c in (26, 26, 52, 52)]
    got_p, got_h = pre.handle_paf_and_heat(*maps, skeleton=sk)
    heat_src, paf_src, paf_sign = sk.flip_tables()
    assert np.array_equal(got_h.view(np.uint32), tr.flip_merge_f32(maps[0][None], maps[1][None], heat_src, [1] * 26)[0])
    assert np.array_equal(got_p.view(np.uint32), tr.flip_merge_f32(maps[2][None], maps[3][None], paf_src, paf_sign)[0])
    # a model with other channel counts is refused, as PoseEstimator refuses it
    with pytest.raises(ValueError, match="BODY_25"):
        pre.get_multiscale_outputs_batch([img], op.OpenPose_Model(4, 2, 38, 19).cuda().eval(), 'rtpose', **kw)


# ---- 7. skeleton=COCO18 is the default path's arithmetic -------------------------------------------------------------------
def test_coco18_skeleton_gives_the_bits_of_the_default_path(pkg, cuda, skm):
    """skeleton=None is COCO-18: the same table, accumulators of 38 / 19 channels, without inspecting the model."""
    from oracle import net_oracle
    pre = importlib.import_module(pkg.__name__ + ".preprocess")
    dec = importlib.import_module(pkg.__name__ + ".decode")
    model = pkg.get_model('vgg19')
    model.load_state_dict(net_oracle.he_init_state_dict(model, seed=0))
    model = model.cuda().eval()
    cfg = dec.default_config()
    cfg.DATASET.IMAGE_SIZE = 96
    rng = np.random.default_rng(71)
    imgs = [rng.integers(0, 256, (61, 75, 3), dtype=np.uint8) for _ in range(2)]
    for flip in (True, False):
        with torch.no_grad():
            paf_a, heat_a, s_a = pre.get_multiscale_outputs_batch(imgs, model, 'rtpose', scales=(0.75, 1.0), flip=flip, config=cfg)
            paf_b, heat_b, s_b = pre.get_multiscale_outputs_batch(imgs, model, 'rtpose', scales=(0.75, 1.0), flip=flip, config=cfg,
                                                                  skeleton=skm.COCO18)
        assert s_a == s_b and paf_a.shape == paf_b.shape == (2, 12, 15, 38)
        assert torch.equal(paf_a.view(torch.int32), paf_b.view(torch.int32))
        assert torch.equal(heat_a.view(torch.int32), heat_b.view(torch.int32))
        assert float(paf_a.abs().max()) > 0
    with torch.no_grad():
        one = pre.get_multiscale_outputs(imgs[0], model, 'rtpose', scales=(0.75, 1.0), flip=True, config=cfg)
        two = pre.get_multiscale_outputs(imgs[0], model, 'rtpose', scales=(0.75, 1.0), flip=True, config=cfg, skeleton=skm.COCO18)
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32))
    assert np.array_equal(one[1].view(np.uint32), two[1].view(np.uint32))
