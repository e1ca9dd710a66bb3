"""GPU suite of the colour jitter (csrc/colorjitter.hip, augment.py; header section 4d).

The comparison rule: the device writes the bits of tests/jitter_restate.py - Pillow's integer, fp32 and fp64 arithmetic
restated, so there is nothing to tolerate: ``==`` on floats that are exact integers under norm 0, on the bit patterns
under norm 1.  The restatement is checked against Pillow itself in tests/test_jitter_cpu.py; the sweep over all 2^24
colours compares with Pillow directly.  Shapes are the smallest at which the kernels can still go wrong: operand images
that hold every operand pair, 37 x 53 canvases (no vector width divides a row, 8 pieces of 256 pixels, the last one
partial), canvases around one slab of the L-sum pass (2048 pixels), and 368 x 368 for the width of the sum."""
import ctypes as C
import importlib
import itertools
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_restate as R  # noqa: E402
import jitter_restate as J  # noqa: E402
from conftest import PKG_NAME, ROOT  # noqa: E402
from test_augment_cpu import CASES as AUG_CASES, case_anns, case_params  # noqa: E402
from test_jitter_cpu import CASES, case_cparams, restate_params  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC00ABC          # a NaN with a payload: what the kernels must leave alone


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


def P(order=(-1, -1, -1, -1), factor=(1.0, 1.0, 1.0), hue_shift=0, gray=0):
    return dict(order=list(order), factor=list(factor), hue_shift=hue_shift, gray=gray)


def only(op, value):
    """The operation alone, the other slots -1."""
    factor = [1.0, 1.0, 1.0]
    if op < 3:
        factor[op] = value
    return P((op, -1, -1, -1), factor, value if op == 3 else 0)


def run_jitter(capi, cuda, canvases, plist, norm=0, masks=None, src_slots=None, dst_slots=None, n_dst=None, layout=None,
               in_place=False):
    """Raw rtpose_jitter_batch.  canvases: uint8 [h, w, 3] arrays of one size, uploaded as the dense fp32 source; image k
    reads source slot src_slots[k] (default k) and writes destination slot dst_slots[k] (default k) of a destination
    of n_dst images pre-filled with SENTINEL.  -> the destination as uint32: [n_dst, 3, h, w] (dense; the source tensor
    itself when in_place) or the whole padded buffer (layout)."""
    n = len(plist)
    h, w = canvases[0].shape[:2]
    src = torch.from_numpy(np.stack([J.as_planes(c) for c in canvases])).to(cuda)
    src_slots = list(range(n)) if src_slots is None else src_slots
    dst_slots = list(range(n)) if dst_slots is None else dst_slots
    n_dst = max(dst_slots) + 1 if n_dst is None else n_dst
    descs = (capi.JitterImage * n)()
    for k, p in enumerate(plist):
        d = descs[k]
        for j in range(4):
            d.order[j] = p["order"][j]
        for j in range(3):
            d.factor[j] = p["factor"][j]
        d.hue_shift, d.gray, d.n_src, d.n_dst = p["hue_shift"], int(p["gray"]), src_slots[k], dst_slots[k]
        mask = masks[k] if masks is not None else (0, 0, w, h)
        for j in range(4):
            d.mask[j] = mask[j]
    cfg = capi.JitterCfg.make(h, w, norm, 1 if layout is None else 0)
    if in_place:
        dst = src
    else:
        numel = n_dst * 3 * h * w if layout is None else capi.lib.rtpose_layout_pixels(C.byref(layout), n_dst, h, w) * layout.cstride
        dst = torch.full((numel,), SENTINEL, dtype=torch.int32, device=cuda)
    wb = capi.lib.rtpose_jitter_workspace_bytes(C.byref(cfg), n)
    assert wb > 0
    ws = torch.full((wb // 4,), -1, dtype=torch.int32, device=cuda)
    capi.check(capi.lib.rtpose_jitter_batch(descs, n, C.byref(cfg), capi.ptr(src), capi.ptr(dst),
                                            C.byref(layout) if layout is not None else None, capi.ptr(ws), wb,
                                            capi.current_stream()), "rtpose_jitter_batch")
    torch.cuda.synchronize()
    if in_place:
        return dst.cpu().numpy().view(np.uint32)
    out = dst.cpu().numpy().view(np.uint32)
    return out.reshape(n_dst, 3, h, w) if layout is None else out


def bits(t):
    return np.ascontiguousarray(t, np.float32).view(np.uint32)


def assert_images_equal(got, canvases, plist, norm=0, masks=None, what=""):
    for k, p in enumerate(plist):
        want = bits(J.jitter(canvases[k], p, norm, masks[k] if masks is not None else None))
        diff = got[k] != want
        assert not diff.any(), "%s image %d %s: %d of %d elements differ, first at %s" % (
            what, k, p, int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())


# ---- each operation alone --------------------------------------------------------------------------------------------
def operand_planes():
    """256 x 256 planes of (channel, other) pairs: channel ch runs along x, the two others along y."""
    y, x = np.mgrid[0:256, 0:256].astype(np.uint8)
    return [np.stack([x if ch == k else y for k in range(3)], -1) for ch in range(3)]


def test_brightness_and_saturation_alone_on_a_ramp(capi, cuda):
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, 2)           # 1 x 256, grey
    tint = ramp.copy()
    tint[..., 1] = 255 - tint[..., 1]
    tint[..., 2] = 128
    plist = [only(op, f) for op in (J.BRIGHTNESS, J.SATURATION) for f in J.BLEND_FACTORS]
    for canvas in (ramp, tint):
        canvases = [canvas] * len(plist)
        got = run_jitter(capi, cuda, [canvas], plist, src_slots=[0] * len(plist))
        assert_images_equal(got, canvases, plist, what="ramp")


def test_brightness_and_saturation_alone_on_all_operand_pairs(capi, cuda):
    """Brightness sees every channel value, saturation every (channel, L) neighbourhood the three planes hold, at the CPU
    suite's factors: 78 images in three chunks reading three source slots."""
    planes = operand_planes()
    plist, slots = [], []
    for s in range(3):
        for op in (J.BRIGHTNESS, J.SATURATION):
            for f in J.BLEND_FACTORS:
                plist.append(only(op, f))
                slots.append(s)
    got = run_jitter(capi, cuda, planes, plist, src_slots=slots)
    assert_images_equal(got, [planes[s] for s in slots], plist, what="operand plane")


# ---- contrast --------------------------------------------------------------------------------------------------------
def test_contrast_mean_cases(capi, cuda):
    """Factor 0 shows the mean itself: all 256 values shifted, means of exactly k + 0.5 and the nearest value below."""
    for name, img, mean in J.contrast_mean_cases():
        plist = [only(J.CONTRAST, f) for f in (0.0, 0.9, 1.1)]
        got = run_jitter(capi, cuda, [img], plist, src_slots=[0, 0, 0])
        assert (got[0].view(np.float32) == mean).all(), "%s: mean %s, expected %d" % (name, np.unique(got[0].view(np.float32)), mean)
        assert_images_equal(got, [img] * 3, plist, what=name)


def test_contrast_shapes_around_a_slab_and_the_width_of_the_sum(capi, cuda):
    rng = np.random.default_rng(5)
    slab = J.SLAB
    shapes = [(1, 1), (1, slab + 1), (2, slab), (3, slab - 1)]
    assert [J.slab_geometry(h, w)[1] for h, w in shapes] == [1, 2, 2, 3]
    for h, w in shapes:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[-1, -1] = (255, 255, 255)                   # the pixel beyond the whole slabs weighs in
        dark = (img // 8).astype(np.uint8)
        plist = [only(J.CONTRAST, 0.0), only(J.CONTRAST, 1.1), P((0, 1, -1, -1), (1.5, 0.0, 1.0))]
        got = run_jitter(capi, cuda, [img, dark], plist + plist, src_slots=[0] * 3 + [1] * 3)
        assert_images_equal(got, [img] * 3 + [dark] * 3, plist + plist, what="%d x %d" % (h, w))
    # one pixel beyond a slab decides the mean: 10.619 with it (11), 10.495 without (10)
    edge = J.grey([10] * 1024 + [11] * 1024 + [255], (1, slab + 1))
    got = run_jitter(capi, cuda, [edge], [only(J.CONTRAST, 0.0)], src_slots=[0])
    assert J.contrast_mean(edge) == 11 and int(21504 / 2049 + 0.5) == 10
    assert (got.view(np.float32) == 11.0).all()
    # 368 x 368 of 255: the sum is 34,533,120 - beyond 24 bits of a float and 25 bits of anything narrower
    white = np.full((368, 368, 3), 255, np.uint8)
    assert int(J.luma(white).astype(np.int64).sum()) == 255 * 368 * 368 > 1 << 25
    got = run_jitter(capi, cuda, [white], [only(J.CONTRAST, 0.0), only(J.CONTRAST, 0.9)], src_slots=[0, 0])
    assert (got.view(np.float32) == 255.0).all()
    almost = white.copy()
    almost[:184] = 254                                   # mean 254.5 exactly -> 255
    got = run_jitter(capi, cuda, [almost], [only(J.CONTRAST, 0.0)], src_slots=[0])
    assert J.contrast_mean(almost) == 255 and (got.view(np.float32) == 255.0).all()
    almost[0, 0] = 253                                   # the nearest value below -> 254
    got = run_jitter(capi, cuda, [almost], [only(J.CONTRAST, 0.0)], src_slots=[0])
    assert J.contrast_mean(almost) == 254 and (got.view(np.float32) == 254.0).all()


# ---- hue and saturation over every colour ----------------------------------------------------------------------------
def test_hue_and_saturation_over_all_colours_against_pillow(capi, cuda):
    c = np.arange(1 << 24, dtype=np.uint32)
    allc = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    pil = Image.fromarray(allc)
    plist = [only(J.HUE, 0), only(J.HUE, 244), only(J.SATURATION, float(np.float32(1.0731)))]
    got = run_jitter(capi, cuda, [allc], plist, src_slots=[0, 0, 0])
    for k, shift in enumerate((0, 244)):
        h, s, v = pil.convert("HSV").split()
        moved = Image.fromarray((np.array(h, dtype=np.uint8) + np.uint8(shift)).astype(np.uint8))
        want = np.asarray(Image.merge("HSV", (moved, s, v)).convert("RGB")).transpose(2, 0, 1)
        diff = got[k].view(np.float32) != want
        assert not diff.any(), "hue shift %d: %d of 2^24 colours differ from Pillow" % (shift, int(diff.any(0).sum()))
    want = np.asarray(ImageEnhance.Color(pil).enhance(plist[2]["factor"][2])).transpose(2, 0, 1)
    diff = got[2].view(np.float32) != want
    assert not diff.any(), "saturation: %d of 2^24 colours differ from Pillow" % int(diff.any(0).sum())


# ---- all 24 orders at once -------------------------------------------------------------------------------------------
ORDER_H, ORDER_W = 37, 53
_ORDERS = {}


def order_batch():
    """24 canvases of 37 x 53, one per order of the four operations, each with its own factors, hue shift and mask;
    image 5 has gray; the orders that put hue (and others) before contrast make the L-sum pass run them on the fly."""
    if not _ORDERS:
        rng = np.random.default_rng(24)
        orders = list(itertools.permutations(range(4)))
        canvases, plist, masks = [], [], []
        for k, order in enumerate(orders):
            img = R.synthetic_source(ORDER_H, ORDER_W, 400 + k)
            img[:, :3] = R.FILL                                                   # the pad is part of the mean
            canvases.append(img)
            factor = [float(np.float32(v)) for v in rng.uniform(0.9, 1.1, 3)]
            if k % 6 == 1:
                factor[int(rng.integers(0, 3))] = 1.6                             # beyond [0, 1]: the clipping blend
            plist.append(P(order, factor, int(rng.integers(0, 256)), int(k == 5)))
            x0, y0 = int(rng.integers(0, 10)), int(rng.integers(0, 10))
            masks.append((x0, y0, int(rng.integers(x0, ORDER_W + 1)), int(rng.integers(y0, ORDER_H + 1))))
        masks[0] = (0, 0, ORDER_W, ORDER_H)
        masks[7] = (4, 4, 4, 9)                                                   # nothing kept
        assert any(p["order"].index(J.HUE) < p["order"].index(J.CONTRAST) for p in plist)
        _ORDERS["items"] = (canvases, plist, masks)
        for norm in (0, 1):
            want = np.stack([bits(J.jitter(c, p, norm, m)) for c, p, m in zip(canvases, plist, masks)])
            want.setflags(write=False)
            _ORDERS[norm] = want
    return _ORDERS


@pytest.mark.parametrize("norm", (0, 1))
def test_all_orders_dense(capi, cuda, norm):
    """Into permuted slots of a destination with two more slots than images: the unnamed slots keep the sentinel."""
    canvases, plist, masks = order_batch()["items"]
    want = order_batch()[norm]
    n_dst = len(plist) + 2
    slots = [int(v) for v in np.random.default_rng(norm).permutation(n_dst)[:len(plist)]]
    got = run_jitter(capi, cuda, canvases, plist, norm, masks, dst_slots=slots, n_dst=n_dst)
    for k, s in enumerate(slots):
        diff = got[s] != want[k]
        assert not diff.any(), "image %d %s: %d of %d elements differ, first at %s" % (
            k, plist[k], int(diff.sum()), diff.size, np.argwhere(diff)[0].tolist())
    for s in set(range(n_dst)) - set(slots):
        assert (got[s] == SENTINEL).all(), "unnamed slot %d was written" % s


@pytest.mark.parametrize("norm", (0, 1))
def test_all_orders_through_a_layout_view(capi, cuda, norm):
    """A padded view (lead, ws > w, cstride 8, choff 2): channels 2..4 of the canvas pixels of the named slots are
    written, every other float of the buffer - the other channels, the gaps, the unnamed slot - keeps its NaN."""
    canvases, plist, masks = order_batch()["items"]
    want = order_batch()[norm]
    n_dst = len(plist) + 1
    slots = [int(v) for v in np.random.default_rng(norm + 7).permutation(n_dst)[:len(plist)]]
    lay = capi.Layout.padded(8, ORDER_H, ORDER_W, 3, choff=2)
    assert lay.ws > ORDER_W and lay.lead > 0 and lay.cstride == 8
    got = run_jitter(capi, cuda, canvases, plist, norm, masks, dst_slots=slots, n_dst=n_dst, layout=lay)
    untouched = np.ones(got.shape, bool)
    pix, keep = got.reshape(-1, 8), untouched.reshape(-1, 8)
    yy, xx = np.mgrid[0:ORDER_H, 0:ORDER_W]
    for k, s in enumerate(slots):
        q = lay.lead + (s * lay.hs + yy) * lay.ws + xx
        for ch in range(3):
            diff = pix[q, 2 + ch] != want[k, ch]
            assert not diff.any(), "image %d channel %d: %d elements differ" % (k, ch, int(diff.sum()))
            keep[q, 2 + ch] = False
    assert (got[untouched] == SENTINEL).all(), "%d floats outside the named slots' three channels were written" % int(
        (got[untouched] != SENTINEL).sum())


# ---- other behaviours ------------------------------------------------------------------------------------------------
def test_identity_in_place_alone_and_repeatable(capi, aug, cuda):
    canvases, plist, masks = order_batch()["items"]
    want = order_batch()[1]
    # all slots -1 and no gray: the canvas comes back (norm 0, whole mask)
    got = run_jitter(capi, cuda, canvases[:3], [P()] * 3)
    assert all(np.array_equal(got[k], bits(J.as_planes(canvases[k]))) for k in range(3))
    # NaN and out-of-range source floats read as 0 / 0 / 255
    odd = torch.tensor([float("nan"), -4.0, 300.0], device=cuda).reshape(1, 3, 1, 1)
    out = aug.color_jitter(odd, [dict(order=[-1] * 4)], norm=0)
    assert out.flatten().tolist() == [0.0, 0.0, 255.0]
    first = run_jitter(capi, cuda, canvases, plist, 1, masks)
    assert np.array_equal(first, want)
    assert np.array_equal(run_jitter(capi, cuda, canvases, plist, 1, masks), first)                     # two runs agree
    assert np.array_equal(run_jitter(capi, cuda, canvases, plist, 1, masks, in_place=True).reshape(first.shape), first)
    for k in (0, 5, 13, 23):
        alone = run_jitter(capi, cuda, [canvases[k]], [plist[k]], 1, [masks[k]])
        assert np.array_equal(alone[0], first[k]), "image %d differs alone" % k


def test_more_images_than_one_launch_carries(capi, cuda):
    """70 images over 24 source slots: three chunks, the images with and without contrast mixed in each."""
    canvases, plist, masks = order_batch()["items"]
    rng = np.random.default_rng(9)
    src, ps, ms = [], [], []
    for k in range(70):
        s = int(rng.integers(0, 24))
        p = dict(plist[int(rng.integers(0, 24))])
        if k % 3 == 0:
            p["order"] = [-1 if op == J.CONTRAST else op for op in p["order"]]
        src.append(s), ps.append(p), ms.append(masks[int(rng.integers(0, 24))])
    got = run_jitter(capi, cuda, canvases, ps, 1, ms, src_slots=src)
    for k in range(70):
        assert np.array_equal(got[k], bits(J.jitter(canvases[src[k]], ps[k], 1, ms[k]))), "image %d differs" % k


# ---- the public door -------------------------------------------------------------------------------------------------
def test_fixture_cases_through_color_jitter(aug, cuda):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "color_jitter.npz"))
    for case in CASES:
        cp = case_cparams(gold, case)
        canvas = torch.from_numpy(J.as_planes(gold["canvas_" + case])[None]).to(cuda)
        mask = tuple(int(v) for v in gold["mask_" + case])
        u8 = aug.color_jitter(canvas, [cp], norm=0)
        assert np.array_equal(u8[0].cpu().numpy(), gold["u8_" + case].transpose(2, 0, 1).astype(np.float32)), case
        image = aug.color_jitter(canvas, [cp], [mask], norm=1)
        assert np.array_equal(bits(image[0].cpu().numpy()), bits(gold["image_" + case])), case
        assert aug.color_jitter(canvas, [cp], [mask], norm=1, out=canvas) is canvas and torch.equal(canvas, image)


def test_train_batch_with_and_without_color(aug, cuda):
    """On the sources of the geometry fixture: with colour the image is the geometry restatement followed by the jitter
    restatement; without, it is what augment_images returns when called the way train_batch called it before the
    keyword existed."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "augment_ref.npz"))
    for edge in (48, 40):
        cases = [c for c in AUG_CASES if int(gold["par_" + c][5]) == edge]
        images = [gold["source_" + str(gold["src_" + c])] for c in cases]
        params = [case_params(gold, c) for c in cases]
        anns = [case_anns(gold, c) for c in cases]
        torch.manual_seed(edge)
        cparams = aug.draw_color_params(len(cases), gray_p=0.2)
        assert any(cp["gray"] for cp in cparams) and not all(cp["gray"] for cp in cparams)
        image, heat, paf, metas = aug.train_batch(images, anns, params, color=cparams)
        plain, heat0, paf0, metas0 = aug.train_batch(images, anns, params)
        old = aug.augment_images(images, params)
        assert torch.equal(plain, old) and torch.equal(heat, heat0) and torch.equal(paf, paf0)
        assert "color" not in metas0[0] and [m["color"] for m in metas] == cparams
        assert [m["jpeg"] for m in metas] == [cp["jpeg"] for cp in cparams]
        got = image.cpu().numpy()
        for k, c in enumerate(cases):
            src = images[k]
            mask = aug.transform_annotations([], src.shape[:2], params[k])[3]
            want = J.jitter(R.canvas_u8(src, params[k], edge, edge), restate_params(cparams[k]), 1, mask)
            diff = bits(got[k]) != bits(want)
            assert not diff.any(), "%s: %d elements differ" % (c, int(diff.sum()))
            assert np.array_equal(bits(plain[k].cpu().numpy()), bits(gold["image_" + c])), c
        assert not torch.equal(image, plain)
    # params=None, color=True draws geometry and colour per image in turn
    sizes = [im.shape[:2] for im in images]
    torch.manual_seed(1)
    p2, c2 = aug.draw_train_params(sizes)
    torch.manual_seed(1)
    image2, _, _, metas2 = aug.train_batch(images, anns, color=True)
    assert [m["color"] for m in metas2] == c2
    assert torch.equal(image2, aug.augment_images(images, p2, color=c2))


def test_colour_into_a_plan_input_view(pkg, aug, capi, cuda):
    """augment_images(color=..., out=plan): the jitter launches write the plan's own input view, slot 1."""
    src = R.synthetic_source(70, 90, 3)
    torch.manual_seed(4)
    params, cparams = aug.draw_train_params([(70, 90)], square_edge=48)
    m = pkg.get_model('vgg19').cuda().float().eval()
    plan = m.plan_for_shape(2, 48, 48, cuda)
    assert aug.augment_images([src], params, out=plan, slots=[1], color=cparams) is plan
    base, lay = C.c_void_p(), capi.Layout()
    capi.check(capi.lib.rtpose_net_input_view(plan.handle, C.byref(base), C.byref(lay)), "rtpose_net_input_view")
    first = (base.value - plan.workspace.data_ptr()) // 4
    floats = capi.lib.rtpose_layout_pixels(C.byref(lay), 2, 48, 48) * lay.cstride
    buf = plan.workspace[first:first + floats].cpu().numpy().reshape(-1, lay.cstride)
    yy, xx = np.mgrid[0:48, 0:48]
    got = buf[lay.lead + (1 * lay.hs + yy) * lay.ws + xx][:, :, lay.choff:lay.choff + 3]
    mask = aug.transform_annotations([], (70, 90), params[0])[3]
    want = J.jitter(R.canvas_u8(src, params[0], 48, 48), restate_params(cparams[0]), 1, mask)
    assert np.array_equal(bits(got), bits(want.transpose(1, 2, 0)))
