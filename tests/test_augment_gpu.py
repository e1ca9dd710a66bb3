"""GPU suite of the training-batch augmentation (csrc/augment.hip, augment.py; header section 4c).

The comparison rule: the device writes the bits of tests/augment_restate.py - Pillow's integer resample, so there is
nothing to tolerate - for the table's integers, the canvas (norm 0) and the normalised, masked tensor (norm 1, whose
fp32 divisions are IEEE).  The restatement is checked against the reference-made fixture and against Pillow in
tests/test_augment_cpu.py; the fixture cases run here once more end to end through train_batch.  Shapes are the
smallest at which the kernel can still go wrong: sources 97 x 131, 64 x 48, 37 x 200 and 40 x 40 (plus 100 x 300 for the
width-only resize), canvases of 48 and 40 - neither a multiple of the 32-pixel tile, so every launch has more than one
block per image and clipped tiles."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_restate as R  # noqa: E402
import encode_restate as ER  # noqa: E402
from conftest import PKG_NAME, ROOT  # noqa: E402
from test_augment_cpu import CASES, case_anns, case_params  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC00ABC          # a NaN with a payload: what the kernel must leave alone


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


@pytest.fixture(scope="module")
def enc(pkg):
    return importlib.import_module(PKG_NAME + ".encode")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "augment_ref.npz"))


# ---- rtpose_resample_table -------------------------------------------------------------------------------------------
TABLE_PAIRS = [(128, 32, 0, None),      # factor 0.25: 17 taps
               (48, 12, 0, None),
               (97, 48, 0, None),       # int(97 * 0.5): a hair above 2, 11 taps
               (96, 48, 0, None),       # exactly 0.5: 9 taps
               (200, 100, 0, None),
               (10000, 5001, 4000, 700),  # 0.5001, first > 0
               (131, 80, 0, None),      # 0.618
               (10000, 9999, 9000, 999),  # 0.9999
               (300, 301, 0, None),     # 1.004: an up-scale by a hair
               (40, 160, 0, None),      # x 4
               (427, 368, 11, 300),
               (37, 37, 0, None)]       # the identity as a table (the batch call copies instead)


@pytest.mark.parametrize("in_size,out_size,first,count", TABLE_PAIRS)
def test_resample_table_equals_the_restatement(capi, cuda, in_size, out_size, first, count):
    count = out_size - first if count is None else count
    b = torch.full((count, 2), -7, dtype=torch.int32, device=cuda)
    c = torch.full((count, capi.AUG_MAX_TAPS), -7, dtype=torch.int32, device=cuda)
    capi.check(capi.lib.rtpose_resample_table(in_size, out_size, first, count, capi.ptr(b), capi.ptr(c),
                                              capi.current_stream()), "rtpose_resample_table")
    torch.cuda.synchronize()
    rb, rc = R.resample_table(in_size, out_size, first, count)
    assert rb[:, 1].max() <= R.ksize_of(in_size, out_size) <= capi.AUG_MAX_TAPS
    assert np.array_equal(b.cpu().numpy(), rb), "bounds differ in %d entries" % int((b.cpu().numpy() != rb).any(1).sum())
    assert np.array_equal(c.cpu().numpy(), rc), "coefficients differ in %d entries" % int((c.cpu().numpy() != rc).any(1).sum())


# ---- rtpose_augment_batch --------------------------------------------------------------------------------------------
def _sources():
    s = {n: R.synthetic_source(h, w, 100 + i) for i, (n, (h, w)) in
         enumerate((("A", (97, 131)), ("B", (64, 48)), ("C", (37, 200)), ("D", (40, 40)), ("E", (100, 300))))}
    s["K"] = R.checkerboard(64, 48)
    return s


SOURCES = _sources()


def P(hr, wr, cx=0, cy=0, flip=False):
    return dict(hflip=flip, hr=hr, wr=wr, crop_x=cx, crop_y=cy)


# (source, params, mask: "valid" = mask_valid_area's, None = off (the fill shows), or four integers)
BATCH = {
    48: [("A", P(66, 90, 0, 0), "valid"),                    # crop on both axes at offset 0: taps clipped at the left / top edge
         ("A", P(66, 90, 42, 18, True), "valid"),            # ... at the maximum: clipped at the right / bottom edge; flipped
         ("A", P(66, 90, 20, 7), None),                      # ... interior
         ("B", P(39, 29), "valid"),                          # pad on both axes, odd remainders 19 and 9: left != right
         ("B", P(39, 29, flip=True), None),                  # the same flipped, mask off: the fill shows
         ("C", P(27, 150, 51, 0), "valid"),                  # crop x, pad y
         ("B", P(50, 33, 0, 2), (5, 7, 30, 41)),             # pad x, crop y, a mask of its own
         ("A", P(48, 65, 17, 0, True), "valid"),             # 0.5 of odd sizes: 131 / 65 is above 2, 11 taps
         ("B", P(32, 24, flip=True), "valid"),               # factor exactly 0.5: 9 taps
         ("B", P(16, 12), None),                             # factor 0.25: 17 taps
         ("A", P(97, 131, 30, 20), "valid"),                 # factor 1.0: no pass at all, a copy
         ("A", P(97, 131, 83, 49, True), None),              # ... mirrored, at the far corner
         ("E", P(100, 301, 100, 30), "valid"),               # 1.004 on 100 x 300: only the width changes
         ("E", P(50, 300, 7, 1, True), None),                # only the height changes, mirrored copy along x
         ("K", P(39, 29), None),                             # 0 / 255 checkerboard: the two-pass uint8 resample
         ("D", P(160, 160, 56, 112), "valid"),               # x 4
         ("D", P(40, 40), (0, 0, 0, 0))],                    # nothing kept: all zeros
    40: [("A", P(62, 83, 43, 0), "valid"),
         ("B", P(57, 43, 3, 17, True), "valid"),
         ("C", P(26, 143, 33, 0), None),
         ("D", P(33, 33), "valid"),
         ("D", P(28, 28, flip=True), None),
         ("K", P(32, 24), "valid"),
         ("B", P(16, 12), "valid")],
}
_EXPECT = {}


def batch_items(aug, edge):
    """[(source array, params, mask)] of BATCH[edge] with the masks resolved."""
    out = []
    for name, p, mask in BATCH[edge]:
        p = dict(p, square_edge=edge, factor=None)
        src = SOURCES[name]
        if mask == "valid":
            mask = aug.transform_annotations([], src.shape[:2], p)[3]
        elif mask is None:
            mask = (0, 0, edge, edge)
        out.append((src, p, tuple(mask)))
    return out


def expected(aug, edge, norm):
    """The restatement of BATCH[edge], computed once per (canvas, norm) and never modified."""
    if (edge, norm) not in _EXPECT:
        if (edge, "u8") not in _EXPECT:
            _EXPECT[(edge, "u8")] = [R.canvas_u8(s, p, edge, edge) for s, p, _ in batch_items(aug, edge)]
        want = np.stack([R.to_tensor(c, norm, m) for c, (_, _, m) in zip(_EXPECT[(edge, "u8")], batch_items(aug, edge))])
        want.setflags(write=False)
        _EXPECT[(edge, norm)] = want
    return _EXPECT[(edge, norm)]


def run_batch(capi, cuda, items, edge, norm, slots, n_slots, layout=None, fill=R.FILL):
    """Raw rtpose_augment_batch into a destination of n_slots images pre-filled with SENTINEL.
    -> the destination as uint32: [n_slots, 3, edge, edge] (nchw) or the whole padded buffer (layout)."""
    ups = [torch.from_numpy(s).to(cuda) for s, _, _ in items]
    descs = (capi.AugmentImage * len(items))()
    for k, (s, p, mask) in enumerate(items):
        d = descs[k]
        d.img_rgb, d.h0, d.w0, d.hr, d.wr = ups[k].data_ptr(), s.shape[0], s.shape[1], p["hr"], p["wr"]
        d.hflip, d.crop_x, d.crop_y, d.n_index = int(p["hflip"]), p["crop_x"], p["crop_y"], slots[k]
        for j in range(4):
            d.mask[j] = mask[j]
    cfg = capi.AugmentCfg.make(edge, edge, norm, 1 if layout is None else 0, fill)
    if layout is None:
        numel = n_slots * 3 * edge * edge
    else:
        numel = capi.lib.rtpose_layout_pixels(C.byref(layout), n_slots, edge, edge) * layout.cstride
    dst = torch.full((numel,), SENTINEL, dtype=torch.int32, device=cuda)
    wb = capi.lib.rtpose_augment_workspace_bytes(C.byref(cfg), len(items))
    assert wb > 0
    ws = torch.empty(wb // 4, dtype=torch.int32, device=cuda)
    capi.check(capi.lib.rtpose_augment_batch(descs, len(items), C.byref(cfg), capi.ptr(dst),
                                             C.byref(layout) if layout is not None else None, capi.ptr(ws), wb,
                                             capi.current_stream()), "rtpose_augment_batch")
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    return out.reshape(n_slots, 3, edge, edge) if layout is None else out


def permuted_slots(n, n_slots):
    return [int(v) for v in np.random.default_rng(n).permutation(n_slots)[:n]]


@pytest.mark.parametrize("norm", (0, 1))
@pytest.mark.parametrize("edge", (48, 40))
def test_batch_equals_the_restatement_nchw(capi, aug, cuda, edge, norm):
    """One batch of mixed source sizes into permuted slots of a destination with two more slots than images: every
    element of the named slots is the restatement's, the unnamed slots keep the sentinel."""
    items = batch_items(aug, edge)
    want = expected(aug, edge, norm).view(np.uint32)
    n_slots = len(items) + 2
    slots = permuted_slots(len(items), n_slots)
    got = run_batch(capi, cuda, items, edge, norm, slots, n_slots)
    for k, s in enumerate(slots):
        diff = got[s] != want[k]
        assert not diff.any(), "image %d %s: %d of %d elements differ, first at %s" % (
            k, BATCH[edge][k][:2], int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())
    for s in set(range(n_slots)) - set(slots):
        assert (got[s] == SENTINEL).all(), "unnamed slot %d was written" % s


@pytest.mark.parametrize("norm", (0, 1))
@pytest.mark.parametrize("edge", (48, 40))
def test_batch_equals_the_restatement_layout(capi, aug, cuda, edge, norm):
    """The same batch through a padded view (lead, ws > W, cstride 8, choff 2): channels 2..4 of the valid pixels of the
    named slots are written, every other float of the buffer keeps the sentinel."""
    items = batch_items(aug, edge)
    want = expected(aug, edge, norm).view(np.uint32)
    n_slots = len(items) + 1
    slots = permuted_slots(len(items) + 100, n_slots)[:len(items)]
    lay = capi.Layout.padded(8, edge, edge, 3, choff=2)
    assert lay.ws > edge and lay.lead > 0 and lay.cstride == 8
    got = run_batch(capi, cuda, items, edge, norm, slots, n_slots, layout=lay)
    untouched = np.ones(got.shape, bool)
    pix = got.reshape(-1, 8)
    keep = untouched.reshape(-1, 8)
    yy, xx = np.mgrid[0:edge, 0:edge]
    for k, s in enumerate(slots):
        q = lay.lead + (s * lay.hs + yy) * lay.ws + xx
        for ch in range(3):
            diff = pix[q, 2 + ch] != want[k, ch]
            assert not diff.any(), "image %d channel %d: %d elements differ" % (k, ch, int(diff.sum()))
            keep[q, 2 + ch] = False
    assert (got[untouched] == SENTINEL).all(), "%d floats outside the named slots' three channels were written" % int(
        (got[untouched] != SENTINEL).sum())


def test_the_cases_discriminate(aug):
    """What the batch of canvas 48 is there to catch, shown on the restatement: the checkerboard tells the two-pass uint8
    resample from one with an unrounded intermediate; the 1.004 case changes only the width and the 50 x 300 one only the
    height; the taps are clipped at both source edges; the mask-off cases show the fill and the odd pad is uneven."""
    items = batch_items(aug, 48)
    want = expected(aug, 48, 0)
    names = [b[0] for b in BATCH[48]]
    k = names.index("K")
    src, p, _ = items[k]
    assert (R.canvas_u8(src, p, 48, 48) != R.canvas_u8(src, p, 48, 48, rounded_intermediate=False)).any()
    e = [i for i, n in enumerate(names) if n == "E"]
    assert (items[e[0]][1]["hr"], items[e[0]][1]["wr"]) == (100, 301) and items[e[0]][0].shape[:2] == (100, 300)
    assert (items[e[1]][1]["hr"], items[e[1]][1]["wr"]) == (50, 300)
    b, _ = R.resample_table(131, 90)
    assert b[0, 0] == 0 and b[0, 1] < b[45, 1] and b[-1].sum() == 131 and b[-1, 1] < b[45, 1]
    assert R.ksize_of(48, 24) == 9 and R.ksize_of(131, 65) == 11 and R.ksize_of(48, 12) == 17
    fill = np.array(R.FILL, np.float32)
    assert (want[4][:, 0, 0] == fill).all() and (want[4][:, 47, 47] == fill).all()
    left, new_w = R.placement(29, 0, 48)
    assert left == 9 and 48 - new_w - left == 10
    assert (want[3][:, :, :9] == 0).all() and (want[3][:, 4:43, 9:38] != 0).any()      # masked: the pad is zero
    assert (want[len(names) - 1] == 0).all()


def test_alone_equals_in_batch_and_two_runs_agree(capi, aug, cuda):
    items = batch_items(aug, 48)
    n = len(items)
    first = run_batch(capi, cuda, items, 48, 1, list(range(n)), n)
    again = run_batch(capi, cuda, items, 48, 1, list(range(n)), n)
    assert np.array_equal(first, again)
    for k in (1, 9, 12, 15):
        alone = run_batch(capi, cuda, [items[k]], 48, 1, [0], 1)
        assert np.array_equal(alone[0], first[k]), "image %d differs alone" % k


def test_more_images_than_one_launch_carries(capi, aug, cuda):
    """35 images: the descriptors travel in chunks of 32, the second chunk has its own table slots."""
    rng = np.random.default_rng(3)
    items = []
    for k in range(35):
        side = int(rng.integers(20, 41))
        items.append((SOURCES["D"], dict(P(side, int(rng.integers(20, 41)), flip=bool(k & 1)), square_edge=40), (0, 0, 40, 40)))
    got = run_batch(capi, cuda, items, 40, 0, list(range(35)), 35)
    for k, (s, p, m) in enumerate(items):
        want = R.to_tensor(R.canvas_u8(s, p, 40, 40), 0, m).view(np.uint32)
        assert np.array_equal(got[k], want), "image %d differs" % k


# ---- the public door -------------------------------------------------------------------------------------------------
def _zero_pattern(gold, key, case, shape):
    return np.unpackbits(gold[key + "_" + case])[:int(np.prod(shape))].reshape(shape).astype(bool)


def test_fixture_cases_through_train_batch(gold, aug, enc, cuda):
    """Every fixture case end to end, batched by canvas: the image and the keypoints are the reference's bits, the targets
    follow encode.py's contract against the reference's (PAF bits equal, heat within 1 fp32 ulp, identical zero pattern)
    and equal encode_targets of the same keypoints exactly."""
    for edge in (48, 40):
        cases = [c for c in CASES if int(gold["par_" + c][5]) == edge]
        images = [gold["source_" + str(gold["src_" + c])] for c in cases]
        params = [case_params(gold, c) for c in cases]
        image, heat, paf, metas = aug.train_batch(images, [case_anns(gold, c) for c in cases], params)
        assert image.shape == (len(cases), 3, edge, edge) and image.is_cuda and image.dtype == torch.float32
        assert heat.shape == (len(cases), 19, edge // 8, edge // 8) and paf.shape == (len(cases), 38, edge // 8, edge // 8)
        img, heat, paf = image.cpu().numpy(), heat.cpu().numpy(), paf.cpu().numpy()
        people = []
        for k, c in enumerate(cases):
            want = gold["image_" + c]
            diff = img[k].view(np.uint32) != want.view(np.uint32)
            assert not diff.any(), "%s: %d image elements differ from the reference" % (c, int(diff.sum()))
            kp = metas[k]["keypoints"]
            assert kp.dtype == gold["kp_" + c].dtype and np.array_equal(kp, gold["kp_" + c]), c
            for key in ("offset", "scale", "valid_area"):
                assert np.array_equal(metas[k][key], gold[key + "_" + c]), (c, key)
            g_heat, g_paf = gold["heat_" + c], gold["paf_" + c]
            assert np.array_equal(heat[k] == 0, _zero_pattern(gold, "heat_zero", c, g_heat.shape)), c
            assert np.array_equal(paf[k] == 0, _zero_pattern(gold, "paf_zero", c, g_paf.shape)), c
            dh, dp = ER.ulp_distance(heat[k], g_heat), ER.ulp_distance(paf[k], g_paf)
            print("%s: heat %d differ (max %d ulp), PAF %d differ" % (c, int((dh > 0).sum()), int(dh.max()), int((dp > 0).sum())))
            assert dh.max() <= 1 and int((dp > 0).sum()) == 0, c
            people.append(np.array([enc.add_neck(p, dtype=None) for p in kp]).reshape(-1, 18, 3))
        h2, p2 = enc.encode_targets(people, input_size=(edge, edge), device=cuda)
        assert np.array_equal(h2.cpu().numpy().view(np.uint32), heat.view(np.uint32))
        assert np.array_equal(p2.cpu().numpy().view(np.uint32), paf.view(np.uint32))
        assert (heat[:, :18] > 0).any() and (paf != 0).any()


def test_a_368_canvas_feeds_the_stage_losses(pkg, aug, enc, cuda):
    """One 640 x 427 source under seeded draws: the 368 x 368 image against the restatement, then train_batch's tuple
    through encode.stage_losses on an RtposeVGG against get_loss on the module's outputs (as
    test_encode_gpu.py::test_stage_losses_against_get_loss does)."""
    synth = importlib.import_module(PKG_NAME + ".synth")
    src = R.synthetic_source(427, 640, 7)
    rng = np.random.default_rng(11)
    anns = []
    for k in range(3):
        pts = np.stack([rng.uniform(60, 580, 17), rng.uniform(40, 390, 17), rng.choice([1.0, 2.0], 17)], 1)
        anns.append({"keypoints": pts.reshape(-1).tolist(), "bbox": [60.0, 40.0, 520.0, 350.0]})
    torch.manual_seed(0)
    params = aug.draw_params([(427, 640)])
    p = params[0]
    assert p["wr"] > 368 and 0.5 <= p["factor"] <= 1.0 and p["square_edge"] == 368
    image, heat, paf, metas = aug.train_batch([src], [anns], params)
    mask = aug.transform_annotations([], (427, 640), p)[3]
    want = R.augment(src, p, 368, 368, 1, mask)
    diff = image[0].cpu().numpy().view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), "%d of %d elements differ from the restatement" % (int(diff.sum()), diff.size)
    # params=None draws the same under the same seed
    torch.manual_seed(0)
    image2 = aug.train_batch([torch.from_numpy(src).to(cuda)], [anns])[0]
    assert torch.equal(image, image2)
    m = pkg.get_model('vgg19')
    m.load_state_dict(synth.he_init_state_dict(m, seed=0))
    m = m.cuda().float().eval()
    total, log = enc.stage_losses(m, image, heat, paf)
    with torch.no_grad():
        _, saved = m(image)
    ref_total, ref_log = enc.get_loss(saved, heat, paf)
    assert list(log) == list(ref_log)
    for nm in enc.build_names():
        print("%s: %.9g  get_loss %.9g" % (nm, log[nm], ref_log[nm]))
        assert np.isfinite(log[nm]) and abs(log[nm] - ref_log[nm]) <= 1e-5 * ref_log[nm]
    assert np.isfinite(total.item()) and abs(total.item() - float(ref_total)) <= 1e-5 * float(ref_total)
    # the same pixels written straight into a plan's input view
    plan = m.plan_for_shape(2, 368, 368, cuda)
    assert aug.augment_images([src], params, out=plan, slots=[1]) is plan
    capi = importlib.import_module(PKG_NAME + "._capi")
    base, lay = C.c_void_p(), capi.Layout()
    capi.check(capi.lib.rtpose_net_input_view(plan.handle, C.byref(base), C.byref(lay)), "rtpose_net_input_view")
    first = (base.value - plan.workspace.data_ptr()) // 4          # the view lives in the plan's workspace tensor
    floats = capi.lib.rtpose_layout_pixels(C.byref(lay), 2, 368, 368) * lay.cstride
    assert first >= 0 and first + floats <= plan.workspace.numel()
    buf = plan.workspace[first:first + floats].cpu().numpy().reshape(-1, lay.cstride)
    yy, xx = np.mgrid[0:368, 0:368]
    got = buf[lay.lead + (1 * lay.hs + yy) * lay.ws + xx][:, :, lay.choff:lay.choff + 3]
    assert np.array_equal(got.view(np.uint32), want.transpose(1, 2, 0).view(np.uint32))
