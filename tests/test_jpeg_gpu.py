"""GPU suite of the JPEG round trip (csrc/jpeg_roundtrip.hip, augment.py; header section 4e).

The comparison rule: the device writes the bits of tests/jpeg_restate.py - libjpeg-turbo's integer codec chain restated,
so there is nothing to tolerate: ``==`` on floats that are exact integers.  The restatement is checked against Pillow
itself in tests/test_jpeg_cpu.py; where Pillow is built on libjpeg-turbo some tests here compare with Pillow directly
as well.  Shapes are the smallest at which the kernels can still go wrong: one MCU, two MCUs each way, more than one run
of four MCUs with a partial run (80 wide) and three MCU rows, edges of every kind (odd sizes, an even height that is no
multiple of 16, less than a block, a chroma plane one row high or 2 samples wide), and one 368 x 368 training canvas."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch
from PIL import features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_restate as A  # noqa: E402
import jitter_restate as J  # noqa: E402
import jpeg_restate as R  # noqa: E402
from conftest import PKG_NAME, ROOT  # noqa: E402
from test_jitter_cpu import CASES as JITTER_CASES, case_cparams, restate_params  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC00ABC          # a NaN with a payload: what the kernels must leave alone
TURBO = bool(features.check_feature("libjpeg_turbo"))
SHAPES = [(16, 16), (16, 32), (32, 16), (48, 80), (17, 31), (18, 21), (8, 8), (2, 5), (1, 5), (23, 40), (46, 46),
          (7, 4), (3, 1)]
QUALITIES = (1, 50, 95, 100)


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


_WANT = {}


def want_of(kind, h, w, q, seed=0):
    """The restatement's [3, h, w] fp32 result for one kind of content, computed once."""
    key = (kind, h, w, q, seed)
    if key not in _WANT:
        img = R.content(kind, h, w, seed)
        out = J.as_planes(R.roundtrip(img, q))
        out.setflags(write=False)
        _WANT[key] = (img, out)
    return _WANT[key]


def run_jpeg(capi, cuda, images, quality=50, src_slots=None, dst_slots=None, n_dst=None, in_place=False):
    """Raw rtpose_jpeg_roundtrip_batch.  images: uint8 [h, w, 3] arrays of one size, uploaded as the dense fp32 source;
    image k reads source slot src_slots[k] (default k) and writes destination slot dst_slots[k] (default k) of a
    destination of n_dst images pre-filled with SENTINEL (the source itself when in_place).  -> uint32 [n_dst, 3, h, w]."""
    h, w = images[0].shape[:2]
    src = torch.from_numpy(np.stack([J.as_planes(c) for c in images])).to(cuda)
    src_slots = list(range(len(images))) if src_slots is None else src_slots
    n = len(src_slots)
    dst_slots = list(src_slots) if dst_slots is None else dst_slots
    n_dst = (len(images) if in_place else max(dst_slots) + 1) if n_dst is None else n_dst
    descs = (capi.JpegImage * n)()
    for k in range(n):
        descs[k].n_src, descs[k].n_dst = src_slots[k], dst_slots[k]
    cfg = capi.JpegCfg.make(h, w, quality)
    dst = src if in_place else torch.full((n_dst * 3 * h * w,), SENTINEL, dtype=torch.int32, device=cuda)
    wb = capi.lib.rtpose_jpeg_workspace_bytes(C.byref(cfg), n)
    assert wb > 0 and wb % 256 == 0
    ws = torch.full((wb // 4,), -1, dtype=torch.int32, device=cuda)
    capi.check(capi.lib.rtpose_jpeg_roundtrip_batch(descs, n, C.byref(cfg), capi.ptr(src), capi.ptr(dst), capi.ptr(ws), wb,
                                                    capi.current_stream()), "rtpose_jpeg_roundtrip_batch")
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(np.uint32).reshape(n_dst, 3, h, w)


def bits(t):
    return np.ascontiguousarray(t, np.float32).view(np.uint32)


def assert_same(got, want, what):
    diff = got != bits(want)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s" % (what, int(diff.sum()), diff.size,
                                                                           np.argwhere(diff)[0].tolist())


# ---- the kernels against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_quality_and_kind(capi, cuda, shape):
    """The four kinds of content as one batch per quality."""
    h, w = shape
    for q in QUALITIES:
        pairs = [want_of(kind, h, w, q) for kind in R.KINDS]
        got = run_jpeg(capi, cuda, [p[0] for p in pairs], q)
        for k, kind in enumerate(R.KINDS):
            assert_same(got[k], pairs[k][1], "%s %dx%d quality %d" % (kind, h, w, q))


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_training_canvas(capi, cuda, kind):
    img, want = want_of(kind, 368, 368, 50, 1)
    got = run_jpeg(capi, cuda, [img], 50)
    assert_same(got[0], want, kind)
    if TURBO:
        assert_same(got[0], J.as_planes(R.pil_roundtrip(img, 50)), kind + " against Pillow")


def test_fixture_cases(capi, cuda):
    """Pillow's own results, whatever Pillow is installed here."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_roundtrip.npz"))
    for case in ("one_mcu", "odd", "even_height", "runs", "narrow"):
        for q in (1, 50, 95):
            got = run_jpeg(capi, cuda, [gold["in_" + case]], q)
            assert_same(got[0], J.as_planes(gold["q%d_%s" % (q, case)]), "%s quality %d" % (case, q))


def test_source_floats_read_as_the_jitter_reads_them(capi, aug, cuda):
    """NaN and negative -> 0, above 255 -> 255, a fraction truncates."""
    img, _ = want_of("noise", 17, 31, 50)
    src = torch.from_numpy(J.as_planes(img)[None]).to(cuda)
    odd = src.clone()
    odd[0, 0, 0, 0], odd[0, 1, 3, 4], odd[0, 2, 16, 30], odd[0, 0, 5, 5] = float("nan"), -7.0, 1e9, float(img[5, 5, 0]) + 0.9
    clean = img.copy()
    clean[0, 0, 0], clean[3, 4, 1], clean[16, 30, 2] = 0, 0, 255
    got = aug.jpeg_roundtrip(odd)
    assert_same(bits(got[0].cpu().numpy()), J.as_planes(R.roundtrip(clean, 50)), "odd floats")


# ---- slots, in place, carries, determinism -----------------------------------------------------------------------------
def test_out_of_place_into_other_slots(capi, cuda):
    """4 of 6 sources into permuted slots of a 9-image destination: the other five slots, and nothing else, keep the NaN."""
    h, w = 23, 40
    pairs = [want_of(R.KINDS[k % 4], h, w, 50, k) for k in range(6)]
    src_slots, dst_slots = [5, 0, 3, 2], [7, 1, 0, 4]
    got = run_jpeg(capi, cuda, [p[0] for p in pairs], 50, src_slots, dst_slots, n_dst=9)
    for s, d in zip(src_slots, dst_slots):
        assert_same(got[d], pairs[s][1], "source %d in slot %d" % (s, d))
    for d in set(range(9)) - set(dst_slots):
        assert (got[d] == SENTINEL).all(), "unnamed slot %d was written" % d


def test_in_place_equals_out_of_place(capi, cuda):
    h, w = 48, 80
    pairs = [want_of(R.KINDS[k % 4], h, w, 50, k) for k in range(5)]
    images = [p[0] for p in pairs]
    out = run_jpeg(capi, cuda, images, 50, [0, 2, 4])
    inp = run_jpeg(capi, cuda, images, 50, [0, 2, 4], in_place=True)
    for k in (0, 2, 4):
        assert_same(out[k], pairs[k][1], "image %d" % k)
        assert np.array_equal(inp[k], out[k]), "image %d differs in place" % k
    for k in (1, 3):                                        # not listed: the source stays
        assert np.array_equal(inp[k], bits(J.as_planes(images[k])))


def test_more_images_than_one_launch_carries(capi, cuda):
    """35 images of 16 x 16: two chunks, and every codec launch before the first up-sample launch - in place too."""
    pairs = [want_of(R.KINDS[k % 4], 16, 16, 50, k) for k in range(35)]
    images = [p[0] for p in pairs]
    got = run_jpeg(capi, cuda, images, 50)
    for k in range(35):
        assert_same(got[k], pairs[k][1], "image %d" % k)
    assert np.array_equal(run_jpeg(capi, cuda, images, 50, in_place=True), got)


def test_alone_in_a_batch_and_twice(capi, cuda):
    h, w = 46, 46
    pairs = [want_of(R.KINDS[k % 4], h, w, 95, k) for k in range(4)]
    images = [p[0] for p in pairs]
    first = run_jpeg(capi, cuda, images, 95)
    assert np.array_equal(run_jpeg(capi, cuda, images, 95), first)                       # two runs agree
    for k in range(4):
        assert_same(first[k], pairs[k][1], "image %d" % k)
        assert np.array_equal(run_jpeg(capi, cuda, [images[k]], 95)[0], first[k]), "image %d differs alone" % k


def test_jpeg_roundtrip_door(aug, capi, cuda):
    h, w = 18, 21
    pairs = [want_of(R.KINDS[k], h, w, 50, k) for k in range(4)]
    canvas = torch.from_numpy(np.stack([J.as_planes(p[0]) for p in pairs])).to(cuda)
    keep = canvas.clone()
    out = aug.jpeg_roundtrip(canvas)                                                      # all, a new tensor
    assert out is not canvas and torch.equal(canvas, keep)
    for k in range(4):
        assert_same(bits(out[k].cpu().numpy()), pairs[k][1], "image %d" % k)
    some = aug.jpeg_roundtrip(canvas, which=[3, 1])                                       # the others are copied
    assert torch.equal(some[1], out[1]) and torch.equal(some[3], out[3])
    assert torch.equal(some[0], canvas[0]) and torch.equal(some[2], canvas[2])
    big = torch.full((6, 3, h, w), float("nan"), device=cuda)
    assert aug.jpeg_roundtrip(canvas, which=[0, 2], out=big, slots=[5, 1]) is big
    assert torch.equal(big[5], out[0]) and torch.equal(big[1], out[2])
    assert all(bool(torch.isnan(big[s]).all()) for s in (0, 2, 3, 4))
    q1 = aug.jpeg_roundtrip(canvas, which=[0], quality=1)
    assert_same(bits(q1[0].cpu().numpy()), want_of(R.KINDS[0], h, w, 1, 0)[1], "quality 1")
    assert aug.jpeg_roundtrip(canvas, out=canvas) is canvas and torch.equal(canvas, out)  # in place
    assert aug.jpeg_roundtrip(keep, which=[]) is not keep
    with pytest.raises(capi.RtposeError):
        aug.jpeg_roundtrip(keep, which=[0, 1], out=big, slots=[2, 2])                     # an n_dst twice
    with pytest.raises(capi.RtposeError):
        aug.jpeg_roundtrip(keep, which=[0, 1], out=keep, slots=[1, 0])                    # in place keeps the slot
    with pytest.raises(capi.RtposeError):
        aug.jpeg_roundtrip(keep, which=[1], out=keep[1:], slots=[0])                      # two views of one tensor
    with pytest.raises(capi.RtposeError):
        aug.jpeg_roundtrip(keep, quality=0)


# ---- the colour chain with its JPEG step -------------------------------------------------------------------------------
def host_chain(canvas, cp, norm, mask, jpeg):
    """image_transform_train on the host: ColorJitter (the jitter restatement, checked against Pillow's ImageEnhance
    and convert in test_jitter_cpu), the JPEG step where it fires (Pillow's own save / open under libjpeg-turbo, else
    the restatement), RandomGrayscale, ToTensor + Normalize, the mask."""
    p = restate_params(cp)
    u8 = J.jitter_u8(canvas, dict(p, gray=False))
    if jpeg and cp["jpeg"]:
        u8 = R.pil_roundtrip(u8, 50) if TURBO else R.roundtrip(u8, 50)
    if cp["gray"]:
        u8 = J.grayscale(u8)
    return J.to_tensor(u8, norm, mask)


def fixture_batch(h, w):
    """The six parameter sets of the jitter fixture on canvases of one size, jpeg forced on for four of them: with and
    without gray, with contrast first, with the wide factors; real masks."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "color_jitter.npz"))
    cps = [case_cparams(gold, c) for c in JITTER_CASES]
    fire = {"drawn_a", "contrast_first", "gray", "wide_factors"}
    for c, cp in zip(JITTER_CASES, cps):
        cp["jpeg"] = c in fire
    canvases = []
    for k in range(len(cps)):
        img = A.synthetic_source(h, w, 700 + k)
        img[:, :2] = A.FILL
        canvases.append(img)
    masks = [(0, 0, w, h), (2, 0, w - 3, h), (0, 5, w, h - 4), (0, 0, w, h), (2, 1, w - 1, h - 3), (4, 4, 4, 9)]
    assert sum(cp["gray"] and cp["jpeg"] for cp in cps) == 1 and sum(cp["jpeg"] for cp in cps) == 4
    return canvases, cps, masks


@pytest.mark.parametrize("norm", (0, 1))
def test_color_jitter_with_the_jpeg_step(aug, cuda, norm):
    h, w = 37, 53
    canvases, cps, masks = fixture_batch(h, w)
    canvas = torch.from_numpy(np.stack([J.as_planes(c) for c in canvases])).to(cuda)
    keep = canvas.clone()
    want = [host_chain(c, cp, norm, m, True) for c, cp, m in zip(canvases, cps, masks)]
    out = aug.color_jitter(canvas, cps, masks, norm, jpeg=True)
    assert torch.equal(canvas, keep)
    for k in range(6):
        assert_same(bits(out[k].cpu().numpy()), want[k], "image %d" % k)
    # the step changes the firing images and only them
    plain = aug.color_jitter(canvas, cps, masks, norm)
    for k, cp in enumerate(cps):
        assert torch.equal(plain[k], out[k]) == (not cp["jpeg"] or masks[k][0] == masks[k][2]), k
    # a dense result with permuted slots: the two unnamed slots keep their NaN
    big = torch.full((8, 3, h, w), float("nan"), device=cuda)
    slots = [6, 0, 3, 7, 1, 4]
    assert aug.color_jitter(canvas, cps, masks, norm, out=big, slots=slots, jpeg=True) is big
    for k, s in enumerate(slots):
        assert torch.equal(big[s], out[k]), k
    assert bool(torch.isnan(big[2]).all()) and bool(torch.isnan(big[5]).all())
    # in place
    assert aug.color_jitter(canvas, cps, masks, norm, out=canvas, jpeg=True) is canvas and torch.equal(canvas, out)


def test_the_default_is_the_call_without_the_keyword(aug, cuda):
    """jpeg=False, and jpeg=True with no image firing, are the launches and the bits of the call without the keyword."""
    h, w = 37, 53
    canvases, cps, masks = fixture_batch(h, w)
    canvas = torch.from_numpy(np.stack([J.as_planes(c) for c in canvases])).to(cuda)
    old = aug.color_jitter(canvas, cps, masks, 1)
    want = [host_chain(c, cp, 1, m, False) for c, cp, m in zip(canvases, cps, masks)]
    for k in range(6):
        assert_same(bits(old[k].cpu().numpy()), want[k], "image %d" % k)
    assert torch.equal(aug.color_jitter(canvas, cps, masks, 1, jpeg=False), old)
    none = [dict(cp, jpeg=False) for cp in cps]
    assert torch.equal(aug.color_jitter(canvas, none, masks, 1, jpeg=True), old)
    images = [A.synthetic_source(60 + 4 * k, 70 - 3 * k, k) for k in range(3)]
    torch.manual_seed(3)
    params, cparams = aug.draw_train_params([im.shape[:2] for im in images], square_edge=48)
    for cp in cparams:
        cp["jpeg"] = True
    old = aug.augment_images(images, params, color=cparams)
    assert torch.equal(aug.augment_images(images, params, color=cparams, jpeg=False), old)
    t_old = aug.train_batch(images, [[]] * 3, params, color=cparams)
    t_new = aug.train_batch(images, [[]] * 3, params, color=cparams, jpeg=False)
    assert all(torch.equal(a, b) for a, b in zip(t_old[:3], t_new[:3])) and torch.equal(t_old[0], old)
    assert [m["jpeg_applied"] for m in t_new[3]] == [False] * 3 and [m["jpeg"] for m in t_new[3]] == [True] * 3
    assert not torch.equal(aug.augment_images(images, params, color=cparams, jpeg=True), old)


def test_colour_and_jpeg_into_a_plan_input_view(pkg, aug, capi, cuda):
    """augment_images(color=..., jpeg=True, out=plan): the last jitter launch writes the plan's own input view, slot 1."""
    src = A.synthetic_source(70, 90, 3)
    torch.manual_seed(4)
    params, cparams = aug.draw_train_params([(70, 90)], square_edge=48)
    cparams[0]["jpeg"] = True
    m = pkg.get_model('vgg19').cuda().float().eval()
    plan = m.plan_for_shape(2, 48, 48, cuda)
    assert aug.augment_images([src], params, out=plan, slots=[1], color=cparams, jpeg=True) is plan
    base, lay = C.c_void_p(), capi.Layout()
    capi.check(capi.lib.rtpose_net_input_view(plan.handle, C.byref(base), C.byref(lay)), "rtpose_net_input_view")
    first = (base.value - plan.workspace.data_ptr()) // 4
    floats = capi.lib.rtpose_layout_pixels(C.byref(lay), 2, 48, 48) * lay.cstride
    buf = plan.workspace[first:first + floats].cpu().numpy().reshape(-1, lay.cstride)
    yy, xx = np.mgrid[0:48, 0:48]
    got = buf[lay.lead + (1 * lay.hs + yy) * lay.ws + xx][:, :, lay.choff:lay.choff + 3]
    mask = aug.transform_annotations([], (70, 90), params[0])[3]
    want = host_chain(A.canvas_u8(src, params[0], 48, 48), cparams[0], 1, mask, True)
    assert np.array_equal(bits(got), bits(want.transpose(1, 2, 0)))
    assert not np.array_equal(bits(want), bits(host_chain(A.canvas_u8(src, params[0], 48, 48), cparams[0], 1, mask, False)))


@pytest.mark.parametrize("seed,fires", [(4, [4]), (16, [2, 4])])
def test_train_batch_with_the_jpeg_step(aug, cuda, seed, fires):
    """8 images under seeds whose draws fire the JPEG step (jpeg_p is 0.1; seed 4 fires RandomGrayscale on the same
    image): the whole image tensor against the host chain on the geometry restatement's canvas."""
    images = [A.synthetic_source(96 + 8 * k, 140 - 6 * k, 50 + k) for k in range(8)]
    sizes = [im.shape[:2] for im in images]
    torch.manual_seed(seed)
    params, cparams = aug.draw_train_params(sizes)
    assert [k for k, cp in enumerate(cparams) if cp["jpeg"]] == fires
    if seed == 4:
        assert cparams[4]["gray"]
    torch.manual_seed(seed)
    image, heat, paf, metas = aug.train_batch(images, [[]] * 8, color=True, jpeg=True)
    assert [m["color"] for m in metas] == cparams
    assert [m["jpeg_applied"] for m in metas] == [k in fires for k in range(8)] == [m["jpeg"] for m in metas]
    got = image.cpu().numpy()
    for k in range(8):
        mask = aug.transform_annotations([], sizes[k], params[k])[3]
        want = host_chain(A.canvas_u8(images[k], params[k], 368, 368), cparams[k], 1, mask, True)
        assert_same(bits(got[k]), want, "image %d" % k)
    torch.manual_seed(seed)
    plain = aug.train_batch(images, [[]] * 8, color=True)
    assert [m["jpeg_applied"] for m in plain[3]] == [False] * 8
    for k in range(8):
        assert torch.equal(plain[0][k], image[k]) == (k not in fires), k
