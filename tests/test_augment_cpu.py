"""CPU suite of the training-batch augmentation (augment.py, header section 4c): the numpy restatement the kernel is
tested against (tests/augment_restate.py) and the host mirror (draw_params, transform_annotations) against the fixture
made by the reference's own transforms.py / utils.py / datasets.py (tools/make_golden_augment.py ->
tests/golden/augment_ref.npz), the restatement against Pillow where it imports, and the argument refusals of the C entry
points, which run before any launch and need no device."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

import augment_restate as R

GOLD = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")
SOURCES = ("A", "B", "C", "D")
CASES = ["s%d_%d" % (s, k) for s in range(4) for k in range(4)] + ["t_half_flip", "t_copy_crop", "t_pad_odd", "t_crop_pad",
                                                                  "t_quarter"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


def case_params(gold, case):
    hflip, hr, wr, cx, cy, edge = (int(v) for v in gold["par_" + case])
    return dict(hflip=bool(hflip), factor=float(gold["factor_" + case]), hr=hr, wr=wr, crop_x=cx, crop_y=cy, square_edge=edge)


def case_anns(gold, case):
    src = str(gold["src_" + case])
    return [{"keypoints": k.tolist(), "bbox": b.tolist()} for k, b in zip(gold["anns_kp_" + src], gold["anns_bbox_" + src])]


def test_the_fixture_lists_its_cases(gold):
    meta = json.loads(str(gold["meta"]))
    assert meta["cases"] == CASES
    assert "ToTensor" in json.dumps(meta["restated"]) and "div(255)" in json.dumps(meta["restated"])
    assert os.path.getsize(GOLD) < 600 * 1024
    flips = [int(gold["par_" + c][0]) for c in CASES]
    dtypes = {str(gold["kp_" + c].dtype) for c in CASES}
    assert 0 < sum(flips) < len(flips) and dtypes == {"float32", "float64"}


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference(gold, aug, case):
    """uint8 canvas, normalised and masked tensor: bit for bit."""
    p = case_params(gold, case)
    src = gold["source_" + str(gold["src_" + case])]
    edge = p["square_edge"]
    canvas = R.canvas_u8(src, p, edge, edge)
    assert np.array_equal(canvas, gold["canvas_" + case]), "%d canvas bytes differ" % int((canvas != gold["canvas_" + case]).sum())
    mask = aug.transform_annotations([], src.shape[:2], p)[3]
    t = R.to_tensor(canvas, 1, mask)
    want = gold["image_" + case]
    assert t.dtype == want.dtype == np.float32 and t.shape == want.shape
    assert np.array_equal(t.view(np.uint32), want.view(np.uint32)), "%d tensor elements differ" % int(
        (t.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("case", CASES)
def test_transform_annotations_equals_the_reference(gold, aug, case):
    """Keypoints including their dtype, boxes, meta - exactly - and the mask integers against the zeroed area."""
    p = case_params(gold, case)
    src = gold["source_" + str(gold["src_" + case])]
    kp, bbox, meta, mask = aug.transform_annotations(case_anns(gold, case), src.shape[:2], p)
    want = gold["kp_" + case]
    assert kp.dtype == want.dtype and kp.shape == want.shape
    assert np.array_equal(kp, want)
    assert bbox.dtype == gold["bbox_" + case].dtype and np.array_equal(bbox, gold["bbox_" + case])
    for key in ("offset", "scale", "valid_area", "width_height"):
        assert meta[key].dtype == gold[key + "_" + case].dtype, key
        assert np.array_equal(meta[key], gold[key + "_" + case]), (key, meta[key], gold[key + "_" + case])
    assert meta["hflip"] == p["hflip"]
    # the mask integers: exactly the reference's zeroed frame (a normalised pixel is never 0.0)
    x0, y0, x1, y1 = mask
    nz = (gold["image_" + case] != 0).any(0)
    keep = np.zeros_like(nz)
    keep[y0:y1, x0:x1] = True
    assert np.array_equal(nz, keep)


def test_draw_params_reproduces_the_reference(gold, aug):
    import torch
    sizes = [gold["source_" + s].shape[:2] for s in SOURCES]
    for seed in range(4):
        edge = int(gold["par_s%d_0" % seed][5])
        torch.manual_seed(seed)
        got = aug.draw_params(sizes, square_edge=edge)
        for k, g in enumerate(got):
            want = case_params(gold, "s%d_%d" % (seed, k))
            assert g == want, (seed, k, g, want)
    # a float scale_range draws no factor: the flip and the two crop draws only
    torch.manual_seed(5)
    r = float(torch.rand(1).item())
    x = int(torch.randint(-24, 131 - 48 + 24, (1,)))
    y = int(torch.randint(-24, 97 - 48 + 24, (1,)))
    torch.manual_seed(5)
    g = aug.draw_params([(97, 131)], square_edge=48, scale_range=1.0)[0]
    assert g["hflip"] == (not r > 0.5) and g["factor"] == 1.0 and (g["hr"], g["wr"]) == (97, 131)
    assert (g["crop_x"], g["crop_y"]) == (min(max(x, 0), 83), min(max(y, 0), 49))


GRID_SIZES = ((40, 40), (97, 131), (64, 48), (37, 200))
GRID_FACTORS = (0.5, 0.5001, 0.618, 0.75, 0.987, 0.9999, 1.0)


def test_restatement_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    for i, (h, w) in enumerate(GRID_SIZES):
        img = R.synthetic_source(h, w, i)
        assert (img == 0).any() and (img == 255).any()
        for f in GRID_FACTORS + (0.25, 1.004, 4.0):
            ow, oh = int(w * f), int(h * f)
            ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
            assert np.array_equal(R.resize_bicubic_u8(img, ow, oh), ref), (h, w, f)
        flipped = np.asarray(Image.fromarray(img).transpose(Image.FLIP_LEFT_RIGHT).resize((int(w * 0.618), h), Image.BICUBIC))
        assert np.array_equal(R.resize_bicubic_u8(img[:, ::-1], int(w * 0.618), h), flipped)


def test_the_checkerboard_tells_the_two_pass_resample_from_a_float_one():
    img = R.checkerboard(64, 48)
    two = R.resize_bicubic_u8(img, 29, 39)
    one = R.resize_bicubic_u8(img, 29, 39, rounded_intermediate=False)
    assert (two != one).sum() > 0


def test_table_shapes_and_taps():
    assert R.ksize_of(100, 50) == 9 and R.ksize_of(100, 25) == 17 and R.ksize_of(100, 100) == 5 and R.ksize_of(100, 24) == 19
    b, c = R.resample_table(131, 65)
    assert b.shape == (65, 2) and c.shape == (65, R.MAX_TAPS) and b[:, 1].max() <= 9
    assert np.abs(c.sum(1) - (1 << 22)).max() <= 9                  # each row sums to 2^22 up to the taps' roundings
    assert b[0, 0] == 0 and b[-1].sum() == 131                       # clipped at both source edges
    b2, c2 = R.resample_table(131, 65, first=7, count=11)
    assert np.array_equal(b2, b[7:18]) and np.array_equal(c2, c[7:18])


def test_add_neck_keeps_its_default_and_can_keep_float32(pkg):
    enc = importlib.import_module(PKG_NAME + ".encode")
    kp = np.zeros((17, 3), np.float32)
    kp[5], kp[6] = (11.25, 20.5, 2), (20.5, 31, 1)
    assert enc.add_neck(kp).dtype == np.float64
    assert enc.add_neck(kp.tolist()).dtype == np.float64
    got = enc.add_neck(kp, dtype=None)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), enc.add_neck(kp))
    assert enc.add_neck(kp.astype(np.float64), dtype=None).dtype == np.float64
    # the neck in float32 arithmetic: (a + b) rounds in float32 before the halving
    kp[5, 0], kp[6, 0] = np.float32(33554432.0), np.float32(6.0)
    assert enc.add_neck(kp, dtype=None)[1, 0] == np.round((kp[5, 0] + kp[6, 0]) / 2)
    assert enc.add_neck(kp)[1, 0] == np.round((33554432.0 + 6.0) / 2)
    assert enc.add_neck(kp, dtype=None)[1, 0] != enc.add_neck(kp)[1, 0]


def _img(capi, **over):
    d = capi.AugmentImage()
    v = dict(img_rgb=64, h0=97, w0=131, hr=48, wr=65, hflip=0, crop_x=0, crop_y=0, mask=(0, 0, 48, 48), n_index=0)
    v.update(over)
    for k, x in v.items():
        if k == "mask":
            for j in range(4):
                d.mask[j] = x[j]
        else:
            setattr(d, k, x)
    return d


def _call(capi, imgs=None, count=None, cfg="default", dst=64, lay=None, ws=64, wsb=1 << 24):
    if imgs is None:
        imgs = [_img(capi)]
    arr = (capi.AugmentImage * max(len(imgs), 1))(*imgs) if imgs != "null" else None
    if cfg == "default":
        cfg = capi.AugmentCfg.make(48, 48, 1, 1)
    return capi.lib.rtpose_augment_batch(arr, len(imgs) if count is None else count, C.byref(cfg) if cfg is not None else None,
                                         C.c_void_p(dst) if dst else None, C.byref(lay) if lay is not None else None,
                                         C.c_void_p(ws) if ws else None, wsb, None)


def test_augment_refusals_name_the_argument(capi):
    """Every refusal comes before any launch (and before the pointers are looked at): no device needed."""
    def refused(text, **kw):
        rc = _call(capi, **kw)
        assert rc == -1, (kw, rc)
        assert text in capi.last_error(), (text, capi.last_error())
    refused("NULL images", imgs="null", count=1)
    refused("NULL dst", dst=None)
    refused("NULL workspace", ws=None)
    refused("NULL cfg", cfg=None)
    cfg = capi.AugmentCfg.make(48, 48)
    cfg.struct_bytes = 8
    refused("struct_bytes", cfg=cfg)
    refused("cfg.norm", cfg=capi.AugmentCfg.make(48, 48, 2, 1))
    refused("cfg.nchw", cfg=capi.AugmentCfg.make(48, 48, 1, -1))
    refused("out_h 0", cfg=capi.AugmentCfg.make(0, 48))
    refused("out_h 65536", cfg=capi.AugmentCfg.make(65536, 48))
    refused("out_w 0", cfg=capi.AugmentCfg.make(48, 0))
    refused("count", count=-1)
    refused("image 0: NULL img_rgb", imgs=[_img(capi, img_rgb=None)])
    ok = _img(capi)
    refused("image 1: source size h0 0", imgs=[ok, _img(capi, h0=0)])
    refused("image 1: source size", imgs=[ok, _img(capi, w0=-3)])
    refused("image 2: resized size hr 0", imgs=[ok, ok, _img(capi, hr=0)])
    refused("image 0: resized size", imgs=[_img(capi, wr=0)])
    refused("image 1: wr 32 from w0 131 needs 19 taps", imgs=[ok, _img(capi, wr=32)])
    refused("image 0: hr 24 from h0 97 needs 19 taps", imgs=[_img(capi, hr=24)])
    refused("image 0: crop_x 18 outside [0,17]", imgs=[_img(capi, crop_x=18)])
    refused("image 0: crop_x -1", imgs=[_img(capi, crop_x=-1)])
    refused("image 1: crop_y 1 outside [0,0]", imgs=[ok, _img(capi, crop_y=1)])
    refused("image 0: mask x", imgs=[_img(capi, mask=(0, 0, 49, 48))])
    refused("image 0: mask x", imgs=[_img(capi, mask=(30, 0, 20, 48))])
    refused("image 0: mask x", imgs=[_img(capi, mask=(-1, 0, 20, 48))])
    refused("image 0: mask y", imgs=[_img(capi, mask=(0, 0, 48, 49))])
    refused("image 0: mask y", imgs=[_img(capi, mask=(0, 9, 48, 8))])
    refused("image 0: n_index", imgs=[_img(capi, n_index=-1)])
    lcfg = capi.AugmentCfg.make(48, 48, 1, 0)
    refused("NULL ldst", cfg=lcfg)
    refused("ldst addresses 2 channels", cfg=lcfg, lay=capi.Layout.padded(8, 48, 48, 3, choff=6))
    refused("canvas in a ldst view", cfg=lcfg, lay=capi.Layout.dense(8, 40, 48))
    refused("workspace_bytes", wsb=8)
    # count == 0 is a no-op, and an empty mask is legal
    assert _call(capi, imgs=[], count=0) == 0
    # the size query: (out_w + out_h) entries of 2 + 17 ints per image, rounded up to 256; 0 on bad arguments
    q = capi.lib.rtpose_augment_workspace_bytes
    cfg = capi.AugmentCfg.make(48, 40)
    assert q(C.byref(cfg), 3) == (3 * 88 * 19 * 4 + 255) // 256 * 256
    assert q(C.byref(cfg), 0) == 256 and q(C.byref(cfg), -1) == 0 and q(None, 1) == 0
    assert capi.AUG_MAX_TAPS == 17 == R.MAX_TAPS


def test_resample_table_refusals(capi):
    f = capi.lib.rtpose_resample_table
    p = C.c_void_p(64)

    def refused(text, *a):
        assert f(*a) == -1
        assert text in capi.last_error(), (text, capi.last_error())
    refused("NULL bounds", 100, 50, 0, 50, None, p, None)
    refused("NULL coeffs", 100, 50, 0, 50, p, None, None)
    refused("in_size 0", 0, 50, 0, 50, p, p, None)
    refused("out_size 0", 100, 0, 0, 0, p, p, None)
    refused("needs 19 taps", 100, 24, 0, 24, p, p, None)
    refused("first -1", 100, 50, -1, 2, p, p, None)
    refused("first 40 + count 11", 100, 50, 40, 11, p, p, None)
    refused("count -1", 100, 50, 0, -1, p, p, None)
    assert f(100, 50, 50, 0, p, p, None) == 0


def test_new_structs_mirror_the_header(capi, tmp_path):
    """rtpose_augment_image / rtpose_augment_cfg against their ctypes mirrors (sizes and offsets from gcc)."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    mirrors = {"rtpose_augment_image": capi.AugmentImage, "rtpose_augment_cfg": capi.AugmentCfg}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {',
             '  printf("taps %d\\n", RTPOSE_AUG_MAX_TAPS);']
    for st, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "aug_layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "aug_layout")],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "aug_layout")], check=True, stdout=subprocess.PIPE,
                                                   text=True).stdout.splitlines())
    assert int(got["taps"]) == capi.AUG_MAX_TAPS
    for st, cls in mirrors.items():
        assert int(got[st]) == C.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)


def test_augment_is_built_with_the_decoder_flags():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert re.search(r"build/augment\.o: CXXFLAGS \+= -fno-slp-vectorize -fno-vectorize", mk)
    assert re.search(r"^SRCS := .*\baugment\.hip\b", mk, flags=re.M)


def test_host_entry_points_refuse_a_cpu_device(aug, capi):
    p = aug.draw_params([(40, 40)], square_edge=48, scale_range=1.0)
    with pytest.raises(capi.RtposeError):
        aug.augment_images([np.zeros((40, 40, 3), np.uint8)], p, device="cpu")
    with pytest.raises(ValueError):
        aug.augment_images([np.zeros((40, 40, 3), np.uint8)] * 2, p, device="cpu")
    doc = aug.__doc__
    for word in ("ColorJitter", "RandomGrayscale", "RandomRotate", "RescaleAbsolute", "MultiScale", "DataLoader"):
        assert word in doc
