"""GPU suite of the target encoder and the stage losses (csrc/encode.hip, encode.py; header section 4b).

The device is compared with tests/encode_restate.py - the float64 restatement that tests/test_encode_cpu.py pins to the
reference's own get_ground_truth - under one rule (`_same`): the float64 zero pattern is identical, the heat values are
within 1 fp32 ulp (exp), the PAF values are bit-identical to float32(restatement) (only correctly rounded operations),
no NaN of the pre-filled destinations is left.  Every launch writes into NaN-filled maps with a sentinel-filled workspace.
"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import encode_restate as R  # noqa: E402
import skeleton_restate as sr  # noqa: E402
from conftest import PKG_NAME, ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "encode_ref.npz")
SCENES = ("s0", "s1", "s2", "s3", "s4")


@pytest.fixture(scope="module")
def enc(pkg):
    return importlib.import_module(PKG_NAME + ".encode")


@pytest.fixture(scope="module")
def skm(pkg):
    return importlib.import_module(PKG_NAME + ".skeleton")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def run_encode(capi, cuda, kp, counts, skeleton, input_h, input_w, stride, sigma=7.0, heat_channels=None,
               paf_channels=None):
    """One rtpose_encode_targets_skel call on kp [N, K, P, 3] (numpy) with n_people = counts (None = NULL): NaN-filled
    destinations, sentinel-filled workspace of exactly the size the query reports.  -> heat, paf (numpy NHWC)."""
    kp = np.ascontiguousarray(kp, np.float64)
    n, k = kp.shape[:2]
    ch = skeleton.heat_channels if heat_channels is None else heat_channels
    cp = skeleton.paf_channels if paf_channels is None else paf_channels
    cfg = capi.EncodeCfg.make(input_h, input_w, stride, sigma, skeleton.background)
    skel = skeleton.native()
    h, w = input_h // stride, input_w // stride
    heat = torch.full((n, h, w, ch), float("nan"), dtype=torch.float32, device=cuda)
    paf = torch.full((n, h, w, cp), float("nan"), dtype=torch.float32, device=cuda)
    wb = capi.lib.rtpose_encode_workspace_bytes(C.byref(cfg), C.byref(skel), n, k)
    assert wb > 0 and wb % 8 == 0
    ws = torch.full((wb // 8,), -7.25e300, dtype=torch.float64, device=cuda)
    kp_d = torch.from_numpy(kp).to(cuda)
    cnt_d = None if counts is None else torch.from_numpy(np.asarray(counts, np.int32)).to(cuda)
    capi.check(capi.lib.rtpose_encode_targets_skel(capi.ptr(kp_d), capi.ptr(cnt_d), n, k, C.byref(cfg), C.byref(skel), ch, cp,
                                                   capi.ptr(heat), capi.ptr(paf), capi.ptr(ws), wb, capi.current_stream()),
               "rtpose_encode_targets_skel")
    torch.cuda.synchronize()
    return heat.cpu().numpy(), paf.cpu().numpy()


def _same(what, heat, paf, h64, p64):
    """The comparison rule of the module docstring, device (float32) against the restatement (float64)."""
    assert heat.shape == h64.shape and paf.shape == p64.shape, (what, heat.shape, h64.shape, paf.shape, p64.shape)
    assert not np.isnan(heat).any() and not np.isnan(paf).any(), "%s: NaN left in the destinations" % what
    assert np.array_equal(heat == 0, h64 == 0), "%s: heat zero pattern differs in %d cells" % (
        what, int(((heat == 0) != (h64 == 0)).sum()))
    assert np.array_equal(paf == 0, p64 == 0), "%s: PAF zero pattern differs in %d cells" % (
        what, int(((paf == 0) != (p64 == 0)).sum()))
    dh = R.ulp_distance(heat, h64.astype(np.float32))
    dp = R.ulp_distance(paf, p64.astype(np.float32))
    print("%s: heat %d of %d elements differ (max %d ulp); PAF %d of %d differ (max %d ulp, max |d| %.3g)" % (
        what, int((dh > 0).sum()), dh.size, int(dh.max()) if dh.size else 0, int((dp > 0).sum()), dp.size,
        int(dp.max()) if dp.size else 0, float(np.abs(paf.astype(np.float64) - p64).max()) if dp.size else 0.0))
    assert (dh.max() if dh.size else 0) <= 1, "%s: heat off by %d ulp" % (what, int(dh.max()))
    assert int((dp > 0).sum()) == 0, "%s: %d PAF elements are not float32(restatement), worst %d ulp" % (
        what, int((dp > 0).sum()), int(dp.max()))


# ---- golden scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_golden_scenes(capi, enc, cuda, gold, name):
    size = json.loads(str(gold["meta"]))["sizes"][name]
    kp18 = gold["kp18_" + name]
    g_heat, g_paf = gold["heat_" + name], gold["paf_" + name]
    hz = np.unpackbits(gold["heat_zero_" + name])[:g_heat.size].reshape(g_heat.shape).astype(bool)
    pz = np.unpackbits(gold["paf_zero_" + name])[:g_paf.size].reshape(g_paf.shape).astype(bool)
    k = max(1, len(kp18))
    kp = np.zeros((1, k, 18, 3))
    kp[0, :len(kp18)] = kp18
    heat, paf = run_encode(capi, cuda, kp, [len(kp18)], enc.COCO18_TRAIN, size, size, 8)
    assert np.array_equal(heat[0] == 0, hz) and np.array_equal(paf[0] == 0, pz), "zero pattern differs from the reference's"
    dh, dp = R.ulp_distance(heat[0], g_heat), R.ulp_distance(paf[0], g_paf)
    print("%s against the reference: heat %d differ (max %d ulp), PAF %d differ (max %d ulp)" % (
        name, int((dh > 0).sum()), int(dh.max()), int((dp > 0).sum()), int(dp.max())))
    assert dh.max() <= 1 and dp.max() <= 1
    h64, p64 = R.encode(kp18, enc.COCO18_TRAIN, size, size)
    _same(name, heat[0], paf[0], h64, p64)
    # the public door gives the same bits, as NCHW views of NHWC buffers
    ht, pt = enc.encode_targets([kp18], input_size=(size, size), device=cuda)
    assert ht.shape == (1, 19, size // 8, size // 8) and pt.shape == (1, 38, size // 8, size // 8)
    assert ht.permute(0, 2, 3, 1).is_contiguous() and pt.permute(0, 2, 3, 1).is_contiguous()
    assert np.array_equal(ht.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), heat.view(np.uint32))
    assert np.array_equal(pt.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), paf.view(np.uint32))


# ---- tables ----------------------------------------------------------------------------------------------------------
def _random_people(rng, k, P, input_h, input_w):
    """k people of P parts on a half-pixel lattice reaching 4 px outside the input: parts out of range, v in {0, 1, 2},
    coincident parts and exact half-way boxes all occur."""
    kp = np.zeros((k, P, 3))
    kp[:, :, 0] = np.round(rng.uniform(-4, input_w + 4, (k, P)) * 2) / 2
    kp[:, :, 1] = np.round(rng.uniform(-4, input_h + 4, (k, P)) * 2) / 2
    kp[:, :, 2] = rng.choice([0.0, 1.0, 2.0, 2.0], (k, P))
    return kp


def _tables(enc, skm):
    return {"coco18_train": enc.COCO18_TRAIN, "body25": skm.BODY_25,
            "pair2_nobg": skm.Skeleton("pair2_nobg", ["a", "b"], [(0, 1, 0, 1)], background=False),
            "full32": sr.TABLES["full32"].skeleton(skm)}


@pytest.mark.parametrize("geom", [(64, 48, 8), (32, 24, 4)], ids=["64x48s8", "32x24s4"])
@pytest.mark.parametrize("table", ["coco18_train", "body25", "pair2_nobg", "full32"])
def test_tables(capi, enc, skm, cuda, table, geom):
    s = _tables(enc, skm)[table]
    ih, iw, stride = geom
    if table == "full32":
        assert s.paf_channels == 64 and [l[2] for l in s.limbs] != sorted(l[2] for l in s.limbs)
    rng = np.random.default_rng(sum(map(ord, table)) + stride)
    counts = [0, 1, 5]
    kp = np.zeros((3, 5, s.num_parts, 3))
    for i, c in enumerate(counts):
        kp[i, :c] = _random_people(rng, c, s.num_parts, ih, iw)
    h64, p64 = R.encode_batch([kp[i, :c] for i, c in enumerate(counts)], s, ih, iw, stride=stride)
    assert (p64[2] != 0).any() and (h64[2] != 0).any()
    heat, paf = run_encode(capi, cuda, kp, counts, s, ih, iw, stride)
    _same(table + " n_people", heat, paf, h64, p64)
    # n_people = NULL: all 5 slots are people; the padding rows have v = 0 everywhere and are skipped like absent people
    heat2, paf2 = run_encode(capi, cuda, kp, None, s, ih, iw, stride)
    _same(table + " NULL", heat2, paf2, h64, p64)
    # slots behind n_people are never read: garbage there changes nothing
    kp_g = kp.copy()
    for i, c in enumerate(counts):
        kp_g[i, c:] = _random_people(rng, 5 - c, s.num_parts, ih, iw)
    heat3, paf3 = run_encode(capi, cuda, kp_g, counts, s, ih, iw, stride)
    assert np.array_equal(heat3.view(np.uint32), heat.view(np.uint32)) and np.array_equal(paf3.view(np.uint32), paf.view(np.uint32))


def test_spare_channels_are_written_as_zero(capi, enc, skm, cuda):
    """More channels than the table names: heat channels behind parts + background and PAF channels no limb names are 0."""
    s = skm.Skeleton("gap", ["a", "b", "c"], [(0, 1, 4, 1), (1, 2, 6, 3)], background=True)
    rng = np.random.default_rng(5)
    kp = _random_people(rng, 4, 3, 64, 48)[None]
    kp[:, :, :, 2] = 2.0
    heat, paf = run_encode(capi, cuda, kp, None, s, 64, 48, 8, heat_channels=6, paf_channels=9)
    h64, p64 = R.encode(kp[0], s, 64, 48, heat_channels=6, paf_channels=9)
    _same("gap", heat[0], paf[0], h64, p64)
    assert not heat[..., 4:].any() and not paf[..., [0, 2, 5, 7, 8]].any() and paf[..., [1, 3, 4, 6]].any()


# ---- chunking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 16, 17, 33])
def test_people_order_across_lds_chunks(capi, enc, cuda, k):
    """max_people one below, at and one above RTPOSE_ENCODE_CHUNK (and two chunks + 1), every slot a person, on an 8 x 6
    grid where everybody overlaps: the running average depends on the order, which must be the people order across chunk
    boundaries.  15 and 16 are single-chunk launches; for 17 and 33 no single-chunk launch of the same people exists, so
    all four are compared with the restatement - and the first 15 people of each give the bits of the 15-people launch."""
    assert capi.ENCODE_CHUNK == 16
    s = enc.COCO18_TRAIN
    rng = np.random.default_rng(160)
    people = _random_people(rng, 33, 18, 64, 48)
    people[:, :, 0] = np.clip(people[:, :, 0], 0, 47.5)
    people[:, :, 1] = np.clip(people[:, :, 1], 0, 63.5)
    people[:, :, 2] = 2.0
    kp = np.stack([people[:k], people[:k][::-1]])
    heat, paf = run_encode(capi, cuda, kp, None, s, 64, 48, 8)
    h64, p64 = R.encode_batch([kp[0], kp[1]], s, 64, 48)
    assert not np.array_equal(p64[0], p64[1]), "the order of the people does not matter in this scene"
    _same("k=%d" % k, heat, paf, h64, p64)
    heat15, paf15 = run_encode(capi, cuda, kp[:, :15].copy(), None, s, 64, 48, 8)
    heat_c, paf_c = run_encode(capi, cuda, kp, [15, 15], s, 64, 48, 8)
    assert np.array_equal(heat_c.view(np.uint32), heat15.view(np.uint32))
    assert np.array_equal(paf_c.view(np.uint32), paf15.view(np.uint32))


# ---- determinism -----------------------------------------------------------------------------------------------------
def test_two_runs_and_batch_versus_alone(capi, enc, skm, cuda):
    s = skm.BODY_25
    rng = np.random.default_rng(77)
    counts = [4, 0, 7, 2]
    kp = np.zeros((4, 7, 25, 3))
    for i, c in enumerate(counts):
        kp[i, :c] = _random_people(rng, c, 25, 96, 80)
    a = run_encode(capi, cuda, kp, counts, s, 96, 80, 8)
    b = run_encode(capi, cuda, kp, counts, s, 96, 80, 8)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for i, c in enumerate(counts):
        alone = run_encode(capi, cuda, kp[i:i + 1, :max(c, 1)].copy(), [c], s, 96, 80, 8)
        assert np.array_equal(alone[0][0].view(np.uint32), a[0][i].view(np.uint32)), "image %d: heat differs alone" % i
        assert np.array_equal(alone[1][0].view(np.uint32), a[1][i].view(np.uint32)), "image %d: PAF differs alone" % i


# ---- rtpose_stage_mse ------------------------------------------------------------------------------------------------
def run_stage_mse(capi, cuda, pred, target, cstride=64, choff=5, pad=3):
    """pred / target numpy [N, h, w, C]: pred goes into a NaN-filled padded view, target stays dense.  -> fp32 loss."""
    n, h, w, c = pred.shape
    lay = capi.Layout.padded(cstride, h, w, pad, choff=choff)
    pixels = capi.lib.rtpose_layout_pixels(C.byref(lay), n, h, w)
    buf = np.full((pixels, cstride), np.nan, np.float32)
    q = lay.lead + (np.arange(n)[:, None, None] * lay.hs + np.arange(h)[None, :, None]) * lay.ws + np.arange(w)[None, None, :]
    buf[q.reshape(-1), choff:choff + c] = pred.reshape(-1, c)
    buf_d, tgt_d = torch.from_numpy(buf).to(cuda), torch.from_numpy(np.ascontiguousarray(target)).to(cuda)
    need = capi.lib.rtpose_stage_mse_partials(n, h, w, c)
    partials = torch.full((need,), float("nan"), dtype=torch.float64, device=cuda)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=cuda)
    capi.check(capi.lib.rtpose_stage_mse(capi.ptr(buf_d), C.byref(lay), capi.ptr(tgt_d), n, h, w, c, capi.ptr(partials), need,
                                         capi.ptr(loss), capi.current_stream()), "rtpose_stage_mse")
    torch.cuda.synchronize()
    assert not torch.isnan(partials).any()
    return loss.cpu().numpy()[0], need


@pytest.mark.parametrize("shape", [(2, 6, 8, 19), (2, 6, 8, 38), (2, 46, 46, 38)], ids=lambda s: "x".join(map(str, s)))
def test_stage_mse(capi, cuda, shape):
    rng = np.random.default_rng(shape[3] + shape[1])
    pred = rng.normal(0, 0.3, shape).astype(np.float32)
    target = np.clip(rng.normal(0.1, 0.4, shape), -1, 1).astype(np.float32)
    got, need = run_stage_mse(capi, cuda, pred, target)
    assert need == -(-pred.size // 1024) and (shape[1] != 46 or need > 1)
    want = np.float32(R.stage_mse(pred, target))
    ref = torch.nn.functional.mse_loss(torch.from_numpy(pred), torch.from_numpy(target)).item()
    print("%s: device %.9g, float64 restatement %.9g (%d ulp), torch CPU %.9g (rel %.2e), %d partials" % (
        shape, got, want, int(R.ulp_distance(np.array([got]), np.array([want]))[0]), ref, abs(got - ref) / ref, need))
    assert R.ulp_distance(np.array([got]), np.array([want]))[0] <= 1
    assert abs(float(got) - ref) <= 1e-5 * ref
    again, _ = run_stage_mse(capi, cuda, pred, target)
    assert np.float32(again).view(np.uint32) == np.float32(got).view(np.uint32)


# ---- stage_losses ----------------------------------------------------------------------------------------------------
def test_stage_losses_against_get_loss(pkg, enc, cuda):
    synth = importlib.import_module(PKG_NAME + ".synth")
    m = pkg.get_model('vgg19')
    m.load_state_dict(synth.he_init_state_dict(m, seed=0))
    m = m.cuda().float().eval()
    x = (torch.rand(2, 3, 64, 48, generator=torch.Generator().manual_seed(1)) - 0.5).to(cuda)
    rng = np.random.default_rng(9)
    people = [_random_people(rng, 2, 18, 64, 48), _random_people(rng, 3, 18, 64, 48)]
    heat, paf = enc.encode_targets(people, input_size=(64, 48), device=cuda)
    assert heat.shape == (2, 19, 8, 6) and paf.shape == (2, 38, 8, 6)
    total, log = enc.stage_losses(m, x, heat, paf)
    with torch.no_grad():
        _, saved = m(x)
    ref_total, ref_log = enc.get_loss(saved, heat, paf)
    names = enc.build_names()
    assert list(log) == list(ref_log)
    for nm in names:
        print("%s: %.9g  get_loss %.9g  rel %.2e" % (nm, log[nm], ref_log[nm], abs(log[nm] - ref_log[nm]) / ref_log[nm]))
        assert abs(log[nm] - ref_log[nm]) <= 1e-5 * ref_log[nm]
    seq = np.float32(0)
    for nm in names:
        seq = np.float32(seq + np.float32(log[nm]))
    assert total.is_cuda and np.float32(total.item()).view(np.uint32) == seq.view(np.uint32)
    assert abs(total.item() - float(ref_total)) <= 1e-5 * float(ref_total)
    for nm in ('max_ht', 'min_ht', 'max_paf', 'min_paf'):
        assert log[nm] == ref_log[nm]
    other = importlib.import_module(PKG_NAME + ".openpose").OpenPose_Model(2, 2, 38, 19)   # 4 stage outputs, not 12
    with pytest.raises(TypeError, match="RtposeVGG only"):
        enc.stage_losses(other, x, heat, paf)


# ---- round trip ------------------------------------------------------------------------------------------------------
# template, seeds of whole people (spaced_people with drop_prob = 0), seeds with parts dropped (the default drop_prob = 0.1).
# The seeds are those on which the CPU pair - encode_restate into the oracle's NMS and skeleton_restate.process - returns
# every person with exactly its present parts and without a score tie.  Whole people: 38 of the seeds 0..39 for COCO-18
# (19 loses a person, 32 ties), 14 of them for BODY_25, whose foot limbs are shorter than a cell on people 50 - 77 px tall.
# With parts dropped few seeds qualify (4 of 0..39, 4 of 0..699): a part dropped in the middle of a chain cuts the person
# in two for any decoder.  They stay in because only they have people with absent parts.
ROUNDTRIP = {
    "coco18": (sr._COCO_TEMPLATE, tuple(s for s in range(40) if s not in (19, 32)), (13, 23, 24, 28)),
    "body25": (sr._BODY25_TEMPLATE, (0, 5, 8, 9, 10, 13, 15, 23, 25, 28, 33, 34, 35, 39), (270, 385, 402, 633)),
}
# Worst part distance of the CPU pair on those seeds: COCO-18 5.640 px whole (seed 33; 0.90 - 5.60 on the others) and
# 4.509 px with drops (seed 13), BODY_25 5.727 px whole (seed 15) and 5.861 px with drops (seed 385).  Twice the worst is
# 11.7 px, above one stride: T is the stride.
ROUNDTRIP_T = 8.0


def roundtrip_people(name, seed, drop_prob):
    """Three synth.spaced_people on 184 x 184 as (3, P, 3) float64: NaN parts become v = 0."""
    synth = importlib.import_module(PKG_NAME + ".synth")
    pts = synth.spaced_people(np.random.default_rng(seed), ROUNDTRIP[name][0], 3, 184, 184, drop_prob=drop_prob)
    kp = np.zeros((3, pts[0].shape[0], 3))
    for i, p in enumerate(pts):
        ok = ~np.isnan(p[:, 0])
        kp[i, ok, :2] = p[ok]
        kp[i, ok, 2] = 2.0
    return kp


def roundtrip_distance(kp, peaks, parts):
    """Decoded humans (parts [H, P] of peak ids into peaks [n, >= 2]) against the people kp [K, P, 3]: the same number
    of people, each matched to the person whose present parts it has exactly, -> the worst part distance in pixels."""
    assert len(parts) == len(kp), "%d people decoded, %d encoded" % (len(parts), len(kp))
    worst, used = 0.0, set()
    for row in parts:
        have = row >= 0
        xy = np.array([peaks[c, :2] if c >= 0 else (0, 0) for c in row], np.float64)
        best = None
        for k in range(len(kp)):
            if k in used or not np.array_equal(kp[k, :, 2] > 0.5, have):
                continue
            d = np.hypot(*(xy[have] - kp[k, have, :2]).T).max()
            if best is None or d < best[0]:
                best = (d, k)
        assert best is not None, "a decoded person has a set of parts no encoded person has"
        used.add(best[1])
        worst = max(worst, best[0])
    return worst


@pytest.mark.parametrize("name", sorted(ROUNDTRIP))
def test_round_trip_through_the_decoder(pkg, enc, skm, cuda, name):
    """decode(encode(people)) == people with the decoder's presets (the limbs encoded are the limbs decoded).
    T is twice the worst distance of the CPU pair (encode_restate -> oracle NMS + skeleton_restate.process) on the
    same seeds, and at most one stride: measured 5.640 px (COCO-18) and 5.861 px (BODY_25), so T = 8 px, the stride.
    The seeds are ones on which the CPU pair returns every person without a tie (see ROUNDTRIP)."""
    dec = importlib.import_module(PKG_NAME + ".decode")
    s = {"coco18": skm.COCO18, "body25": skm.BODY_25}[name]
    _, whole, dropped = ROUNDTRIP[name]
    cases = [(seed, 0.0) for seed in whole] + [(seed, 0.1) for seed in dropped]
    scenes = [roundtrip_people(name, seed, drop) for seed, drop in cases]
    assert any((kp[:, :, 2] == 0).any() for kp in scenes[len(whole):]), "no scene with an absent part"
    heat, paf = enc.encode_targets(scenes, skeleton=s, input_size=(184, 184), device=cuda)
    recs = dec.decode_maps(heat.permute(0, 2, 3, 1), paf.permute(0, 2, 3, 1), skeleton=s)
    worst = 0.0
    for (seed, drop), kp, rec in zip(cases, scenes, recs):
        d = roundtrip_distance(kp, rec["peaks"], rec["parts"])
        print("%s seed %d drop %.1f: %d people back, worst part distance %.3f px (T = %.3f)" % (name, seed, drop,
                                                                                              len(rec["parts"]), d, ROUNDTRIP_T))
        worst = max(worst, d)
    assert worst <= ROUNDTRIP_T
