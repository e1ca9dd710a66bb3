"""CPU suite of the colour jitter (augment.py, header section 4d): the numpy restatement the kernels are tested against
(tests/jitter_restate.py) against Pillow itself - the two HSV conversions and convert('L') over all 2^24 colours,
Image.blend over all 65,536 operand pairs, the three ImageEnhance classes on images -, the fixture made by Pillow
(tools/make_golden_jitter.py -> tests/golden/color_jitter.npz), the draws against the literal sequence of torch calls,
and the argument refusals of the C entry points, which run before any launch and need no device."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from conftest import PKG_NAME, ROOT

import jitter_restate as J

GOLD = os.path.join(ROOT, "tests", "golden", "color_jitter.npz")
CASES = ["drawn_a", "drawn_b", "contrast_first", "hue_zero", "gray", "wide_factors"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


@pytest.fixture(scope="module")
def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    a = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    a.setflags(write=False)
    return a


def case_cparams(gold, case):
    f = [float(v) for v in gold["factor_" + case]]
    hue = float(gold["hue_" + case])
    return dict(order=[int(v) for v in gold["order_" + case]], brightness=f[0], contrast=f[1], saturation=f[2], hue=hue,
                hue_shift=int(hue * 255) % 256, gray=bool(int(gold["gray_" + case])), jpeg=False)


def restate_params(cp):
    return dict(order=cp["order"], factor=[cp["brightness"], cp["contrast"], cp["saturation"]], hue_shift=cp["hue_shift"],
                gray=cp["gray"])


def hsv_image(hsv):
    return Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(hsv[..., k])) for k in range(3)])


# ---- the restatement against Pillow ----------------------------------------------------------------------------------
def test_rgb_to_hsv_over_all_colours(all_colours):
    want = np.asarray(Image.fromarray(all_colours).convert("HSV"))
    assert int((J.rgb_to_hsv(all_colours) != want).sum()) == 0


def test_hsv_to_rgb_over_all_triples(all_colours):
    want = np.asarray(hsv_image(all_colours).convert("RGB"))
    assert int((J.hsv_to_rgb(all_colours) != want).sum()) == 0


def test_luminance_over_all_colours(all_colours):
    want = np.asarray(Image.fromarray(all_colours).convert("L"))
    assert int((J.luma(all_colours) != want).sum()) == 0


def test_blend_over_all_operand_pairs():
    d, x = np.mgrid[0:256, 0:256].astype(np.uint8)
    assert len(set(J.BLEND_FACTORS)) == 13 and sum(0.9 < f < 1.1 and f != 1.0 for f in J.BLEND_FACTORS) == 6
    for f in J.BLEND_FACTORS:
        want = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(x), f))
        diff = J.blend(d, x, f) != want
        assert not diff.any(), "factor %r: %d of 65536 pairs differ" % (f, int(diff.sum()))


def test_enhance_classes_on_random_images():
    rng = np.random.default_rng(7)
    for k in range(12):
        h, w = (int(v) for v in rng.integers(1, 70, 2))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 3 == 0:
            img = (img // 4 + 180).astype(np.uint8)          # bright: factors above 1 saturate
        pil = Image.fromarray(img)
        for f in (float(np.float32(rng.uniform(0.9, 1.1))), 0.9, 1.1, 1.7):
            assert np.array_equal(J.brightness(img, f), np.asarray(ImageEnhance.Brightness(pil).enhance(f))), (k, f)
            assert np.array_equal(J.contrast(img, f), np.asarray(ImageEnhance.Contrast(pil).enhance(f))), (k, f)
            assert np.array_equal(J.saturation(img, f), np.asarray(ImageEnhance.Color(pil).enhance(f))), (k, f)


def test_contrast_mean_cases_against_pillow():
    """The mean rounds half up: exactly k + 0.5 gives k + 1, the nearest value below gives k."""
    cases = J.contrast_mean_cases()
    assert dict((n, m) for n, _, m in cases)["two_pixels_10_11"] == 11
    assert len({m for _, _, m in cases}) >= 7
    for name, img, mean in cases:
        assert J.contrast_mean(img) == mean, name
        for f in (0.9, 1.1, 0.0):
            want = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f))
            assert np.array_equal(J.contrast(img, f), want), (name, f)
        # factor 0 leaves the mean itself
        assert (J.contrast(img, 0.0) == mean).all(), name


def test_read_u8_clamps_and_drops_nan():
    v = np.array([-3.0, -0.0, 0.0, 0.9, 1.0, 254.99, 255.0, 255.5, 1e9, np.nan, np.inf, -np.inf], np.float32)
    assert J.read_u8(v).tolist() == [0, 0, 0, 0, 1, 254, 255, 255, 255, 0, 255, 0]


# ---- the fixture -----------------------------------------------------------------------------------------------------
def test_the_fixture_lists_its_cases(gold):
    meta = json.loads(str(gold["meta"]))
    assert meta["cases"] == CASES
    assert re.match(r"\d+\.\d+", meta["pillow"]) and "not installed" in meta["torchvision"] and "not built" in meta["jpeg"]
    assert os.path.getsize(GOLD) < 200 * 1024
    for c in CASES:
        assert max(gold["canvas_" + c].shape[:2]) <= 48
    assert int(gold["gray_gray"]) == 1 and list(gold["order_contrast_first"])[0] == 1


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_fixture(gold, case):
    p = restate_params(case_cparams(gold, case))
    got = J.jitter_u8(gold["canvas_" + case], p)
    assert np.array_equal(got, gold["u8_" + case]), "%d bytes differ" % int((got != gold["u8_" + case]).sum())
    t = J.jitter(gold["canvas_" + case], p, 1, tuple(int(v) for v in gold["mask_" + case]))
    want = gold["image_" + case]
    assert t.dtype == want.dtype == np.float32 and np.array_equal(t.view(np.uint32), want.view(np.uint32))


# ---- the draws -------------------------------------------------------------------------------------------------------
def literal_color_draws(brightness=0.1, contrast=0.1, saturation=0.1, hue=0.1, jpeg_p=0.1, gray_p=0.01):
    """The torch calls of torchvision's ColorJitter.get_params, RandomApply.forward and RandomGrayscale.forward."""
    fn_idx = torch.randperm(4)
    b = float(torch.empty(1).uniform_(1 - brightness, 1 + brightness))
    c = float(torch.empty(1).uniform_(1 - contrast, 1 + contrast))
    s = float(torch.empty(1).uniform_(1 - saturation, 1 + saturation))
    h = float(torch.empty(1).uniform_(-hue, hue))
    jpeg = not (jpeg_p < torch.rand(1))
    gray = bool(torch.rand(1) < gray_p)
    return fn_idx.tolist(), b, c, s, h, bool(jpeg), gray


def same_draw(cp, lit):
    return (cp["order"], cp["brightness"], cp["contrast"], cp["saturation"], cp["hue"], cp["jpeg"], cp["gray"]) == lit


def test_draw_color_params_is_the_literal_sequence(aug):
    for seed in range(6):
        torch.manual_seed(seed)
        want = [literal_color_draws() for _ in range(5)]
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        got = aug.draw_color_params(5)
        assert torch.equal(torch.get_rng_state(), state)
        for cp, lit in zip(got, want):
            assert same_draw(cp, lit), (cp, lit)
            assert sorted(cp["order"]) == [0, 1, 2, 3] and cp["hue_shift"] == int(cp["hue"] * 255) % 256
            assert 0.9 <= cp["brightness"] <= 1.1 and -0.1 <= cp["hue"] <= 0.1


def test_a_jpeg_draw_keeps_the_next_image_in_step(aug):
    """With p = 1 every image's JPEG draw fires (and p = 0.5 some do): it is consumed and recorded, and the draws of the
    image after it are the literal sequence's."""
    for p in (1.0, 0.5):
        torch.manual_seed(3)
        want = [literal_color_draws(jpeg_p=p, gray_p=0.5) for _ in range(8)]
        state = torch.get_rng_state()
        torch.manual_seed(3)
        got = aug.draw_color_params(8, jpeg_p=p, gray_p=0.5)
        assert torch.equal(torch.get_rng_state(), state)
        assert all(same_draw(cp, lit) for cp, lit in zip(got, want))
        fired = [cp["jpeg"] for cp in got]
        assert any(fired[:-1]) and (all(fired) if p == 1.0 else not all(fired))
        assert 0 < sum(cp["gray"] for cp in got) < 8


def test_draw_train_params_interleaves_geometry_and_colour(aug):
    sizes = [(427, 640), (100, 80), (500, 375), (640, 480)]
    torch.manual_seed(11)
    want = []
    for size in sizes:
        g = aug.draw_params([size])[0]
        want.append((g, literal_color_draws()))
    state = torch.get_rng_state()
    torch.manual_seed(11)
    params, cparams = aug.draw_train_params(sizes)
    assert torch.equal(torch.get_rng_state(), state)
    for (g, lit), p, cp in zip(want, params, cparams):
        assert p == g and same_draw(cp, lit)
    # not the same as all geometry first, then all colour
    torch.manual_seed(11)
    assert aug.draw_params(sizes) != params


def test_an_operation_with_range_zero_draws_nothing_and_drops_out(aug):
    torch.manual_seed(2)
    fn_idx = torch.randperm(4).tolist()
    b = float(torch.empty(1).uniform_(0.9, 1.1))
    s = float(torch.empty(1).uniform_(0.8, 1.2))
    torch.rand(1), torch.rand(1)
    state = torch.get_rng_state()
    torch.manual_seed(2)
    cp = aug.draw_color_params(1, contrast=0, saturation=0.2, hue=0)[0]
    assert torch.equal(torch.get_rng_state(), state)
    assert cp["brightness"] == b and cp["saturation"] == s and cp["contrast"] is None and cp["hue"] is None
    assert cp["order"] == [op if op in (0, 2) else -1 for op in fn_idx] and cp["hue_shift"] == 0


def test_hue_shift_truncates_toward_zero_modulo_256(aug):
    assert aug.hue_shift_of(-0.05) == 244                     # -12.75 -> -12 -> 244
    assert aug.hue_shift_of(0.05) == 12
    assert aug.hue_shift_of(0.0) == 0 and aug.hue_shift_of(-0.001) == 0 and aug.hue_shift_of(0.1) == 25
    assert aug.hue_shift_of(-0.1) == 231 and aug.hue_shift_of(0.5) == 127 and aug.hue_shift_of(-0.5) == 129
    for f in np.random.default_rng(1).uniform(-0.5, 0.5, 50):
        with np.errstate(over="ignore"):
            assert aug.hue_shift_of(float(f)) == int(np.array(int(f * 255)).astype(np.uint8))


# ---- the C entry points ----------------------------------------------------------------------------------------------
def _img(capi, **over):
    d = capi.JitterImage()
    v = dict(order=(0, 1, 2, 3), factor=(1.0, 0.9, 1.1), hue_shift=3, gray=0, mask=(0, 0, 48, 40), n_src=0, n_dst=0)
    v.update(over)
    for k, x in v.items():
        if k in ("order", "factor", "mask"):
            for j in range(len(x)):
                getattr(d, k)[j] = x[j]
        else:
            setattr(d, k, x)
    return d


def _call(capi, imgs=None, count=None, cfg="default", src=64, dst=128, lay=None, ws=64, wsb=1 << 20):
    if imgs is None:
        imgs = [_img(capi)]
    arr = (capi.JitterImage * max(len(imgs), 1))(*imgs) if imgs != "null" else None
    if cfg == "default":
        cfg = capi.JitterCfg.make(40, 48, 1, 1)
    return capi.lib.rtpose_jitter_batch(arr, len(imgs) if count is None else count, C.byref(cfg) if cfg is not None else None,
                                        C.c_void_p(src) if src else None, C.c_void_p(dst) if dst else None,
                                        C.byref(lay) if lay is not None else None, C.c_void_p(ws) if ws else None, wsb, None)


def test_jitter_refusals_name_the_argument(capi):
    """Every refusal comes before any launch (and before the pointers are looked at): no device needed."""
    def refused(text, **kw):
        rc = _call(capi, **kw)
        assert rc == -1, (kw, rc)
        assert text in capi.last_error(), (text, capi.last_error())
    refused("NULL images", imgs="null", count=1)
    refused("NULL src", src=None)
    refused("NULL dst", dst=None)
    refused("NULL workspace", ws=None)
    refused("NULL cfg", cfg=None)
    cfg = capi.JitterCfg.make(40, 48)
    cfg.struct_bytes = 8
    refused("struct_bytes", cfg=cfg)
    refused("cfg.norm", cfg=capi.JitterCfg.make(40, 48, 2, 1))
    refused("cfg.nchw", cfg=capi.JitterCfg.make(40, 48, 1, -1))
    refused("h 0", cfg=capi.JitterCfg.make(0, 48))
    refused("h 65536", cfg=capi.JitterCfg.make(65536, 48))
    refused("w 0", cfg=capi.JitterCfg.make(40, 0))
    refused("w 65536", cfg=capi.JitterCfg.make(40, 65536))
    refused("count", count=-1)
    ok = _img(capi)
    refused("image 1: order[2] 4", imgs=[ok, _img(capi, order=(0, 1, 4, -1))])
    refused("image 0: order[0] -2", imgs=[_img(capi, order=(-2, 1, 2, 3))])
    refused("image 2: order[3] names operation 1 twice", imgs=[ok, ok, _img(capi, order=(1, -1, 0, 1))])
    refused("image 0: factor[0] (brightness)", imgs=[_img(capi, factor=(-0.5, 1.0, 1.0))])
    refused("image 1: factor[1] (contrast)", imgs=[ok, _img(capi, factor=(1.0, float("nan"), 1.0))])
    refused("image 0: factor[2] (saturation)", imgs=[_img(capi, factor=(1.0, 1.0, float("inf")))])
    refused("image 0: hue_shift 256", imgs=[_img(capi, hue_shift=256)])
    refused("image 1: hue_shift -1", imgs=[ok, _img(capi, hue_shift=-1)])
    refused("image 0: mask x", imgs=[_img(capi, mask=(0, 0, 49, 40))])
    refused("image 0: mask x", imgs=[_img(capi, mask=(30, 0, 20, 40))])
    refused("image 0: mask x", imgs=[_img(capi, mask=(-1, 0, 20, 40))])
    refused("image 0: mask y", imgs=[_img(capi, mask=(0, 0, 48, 41))])
    refused("image 1: mask y", imgs=[ok, _img(capi, mask=(0, 9, 48, 8))])
    refused("image 0: n_src -1", imgs=[_img(capi, n_src=-1)])
    refused("image 0: n_src 65536", imgs=[_img(capi, n_src=65536)])
    refused("image 1: n_dst 65536", imgs=[ok, _img(capi, n_dst=65536)])
    lcfg = capi.JitterCfg.make(40, 48, 1, 0)
    refused("NULL ldst", cfg=lcfg)
    refused("ldst addresses 2 channels", cfg=lcfg, lay=capi.Layout.padded(8, 40, 48, 3, choff=6))
    refused("canvas in a ldst view", cfg=lcfg, lay=capi.Layout.dense(8, 40, 40))
    refused("dst == src with cfg.nchw == 0", cfg=lcfg, lay=capi.Layout.dense(8, 40, 48), dst=64)
    refused("image 1: dst == src with n_dst 2 != n_src 1", imgs=[ok, _img(capi, n_src=1, n_dst=2)], dst=64)
    refused("workspace_bytes", wsb=8)
    # count == 0 is a no-op; an empty mask, an empty order and factors above 1 are legal (nothing more to refuse:
    # the next check is the pointers', which needs a device)
    assert _call(capi, imgs=[], count=0) == 0
    # the size query: one uint32 per slab and image, rounded up to 256; 0 on bad arguments
    q = capi.lib.rtpose_jitter_workspace_bytes
    cfg = capi.JitterCfg.make(368, 368)
    assert J.slab_geometry(368, 368) == (2048, 67)
    assert q(C.byref(cfg), 32) == (32 * 67 * 4 + 255) // 256 * 256
    assert q(C.byref(cfg), 0) == 256 and q(C.byref(cfg), -1) == 0 and q(None, 1) == 0
    big = capi.JitterCfg.make(65535, 65535)
    assert J.slab_geometry(65535, 65535) == (2048 * 2048, 1024) and q(C.byref(big), 1) == 4096
    assert J.slab_geometry(1, 2049) == (2048, 2) and J.slab_geometry(1, 2048) == (2048, 1)
    assert capi.JITTER_SLAB == 2048 == J.SLAB


def test_jitter_structs_mirror_the_header(capi, tmp_path):
    """rtpose_jitter_image / rtpose_jitter_cfg against their ctypes mirrors (sizes and offsets from gcc)."""
    import shutil
    import subprocess
    assert shutil.which("gcc"), "gcc compiles the header as C"
    mirrors = {"rtpose_jitter_image": capi.JitterImage, "rtpose_jitter_cfg": capi.JitterCfg}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {',
             '  printf("slab %d\\n", RTPOSE_JITTER_SLAB);']
    for st, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "jitter_layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "jitter_layout")],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "jitter_layout")], check=True, stdout=subprocess.PIPE,
                                                   text=True).stdout.splitlines())
    assert int(got["slab"]) == capi.JITTER_SLAB
    for st, cls in mirrors.items():
        assert int(got[st]) == C.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)


def test_colorjitter_is_built_with_the_decoder_flags():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert re.search(r"build/colorjitter\.o: CXXFLAGS \+= -fno-slp-vectorize -fno-vectorize", mk)
    assert re.search(r"^SRCS := .*\bcolorjitter\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS := .*-ffp-contract=off", mk, flags=re.M)


def test_host_entry_points_check_their_arguments(aug, capi):
    cp = aug.draw_color_params(1)
    with pytest.raises(capi.RtposeError):
        aug.color_jitter(torch.zeros(1, 3, 8, 8), cp)                          # no CPU fallback
    with pytest.raises(ValueError):
        aug.color_jitter(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), cp)
    with pytest.raises(ValueError):
        aug.color_jitter(torch.zeros(3, 8, 8), cp)
    p = aug.draw_params([(40, 40)], square_edge=48, scale_range=1.0)
    with pytest.raises(capi.RtposeError):
        aug.augment_images([np.zeros((40, 40, 3), np.uint8)], p, device="cpu", color=cp)
    for fn in (aug.color_jitter, aug.augment_images, aug.train_batch, aug.draw_color_params):
        assert "JPEG" in fn.__doc__ and "not built" in fn.__doc__
    assert "torchvision is not installed" in aug.draw_color_params.__doc__
    for word in ("JPEG re-compression", "RandomRotate", "RescaleAbsolute", "MultiScale", "decoding", "DataLoader"):
        assert word in aug.__doc__
