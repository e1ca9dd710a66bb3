"""CPU suite of the JPEG round trip (augment.py, header section 4e): the numpy restatement the kernels are tested
against (tests/jpeg_restate.py) against the fixture Pillow made (tools/make_golden_jpeg.py ->
tests/golden/jpeg_roundtrip.npz) and, where Pillow is built on libjpeg-turbo, against Pillow itself over sizes, qualities
and kinds of content; the derived quantiser tables against ``Image.quantization``; the range-limit function against a
literal construction of libjpeg's table; and the argument refusals of the C entry points, which run before any launch
and need no device."""
import ctypes as C
import importlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, features

from conftest import PKG_NAME, ROOT

import jpeg_restate as R

GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_roundtrip.npz")
CASES = ["one_mcu", "odd", "even_height", "runs", "narrow"]
QUALITIES = (1, 5, 10, 25, 50, 51, 75, 90, 95, 100)
TURBO = bool(features.check_feature("libjpeg_turbo"))
needs_turbo = pytest.mark.skipif(not TURBO, reason="this Pillow is not built on libjpeg-turbo: another libjpeg legitimately "
                                                   "gives other bits (the fixture still pins the restatement)")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


def differing(img, q):
    return int((R.roundtrip(img, q) != R.pil_roundtrip(img, q)).sum())


# ---- the fixture -----------------------------------------------------------------------------------------------------
def test_the_fixture_lists_its_cases(gold):
    meta = json.loads(str(gold["meta"]))
    assert meta["cases"] == CASES and meta["qualities"] == [1, 50, 95]
    assert re.match(r"\d+\.\d+", meta["pillow"]) and meta["jpg"] and meta["libjpeg_turbo"] is True
    assert os.path.getsize(GOLD) < 100 * 1024
    for c in CASES:
        h, w = gold["in_" + c].shape[:2]
        assert h <= 48 and w <= 80
    assert gold["in_even_height"].shape[0] % 16 not in (0, 1) and gold["in_even_height"].shape[0] % 2 == 0
    assert gold["in_narrow"].shape[1] <= 4 and gold["in_runs"].shape[:2] == (48, 80)


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_fixture(gold, case):
    for q in (1, 50, 95):
        got, want = R.roundtrip(gold["in_" + case], q), gold["q%d_%s" % (q, case)]
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), "quality %d: %d bytes differ" % (q, int((got != want).sum()))
    assert not np.array_equal(gold["q1_" + case], gold["q95_" + case])


def test_base_tables_are_the_fixtures(gold):
    assert np.array_equal(R.BASE_LUMA, gold["table_luma"]) and np.array_equal(R.BASE_CHROMA, gold["table_chroma"])
    luma, chroma = R.quant_tables(50)
    assert np.array_equal(luma, gold["table_luma"]) and np.array_equal(chroma, gold["table_chroma"])


# ---- the restatement against Pillow itself --------------------------------------------------------------------------
@needs_turbo
def test_every_height_residue_and_width_parity_against_pillow():
    """Heights 1..35, 46..48 and 100 cover every residue mod 16, odd and even, with and without padded MCU rows; widths
    both sides of 4 (box replication up to 4, the triangle filter from 5), of the block and of the MCU."""
    bad = []
    for h in list(range(1, 36)) + [46, 47, 48, 100]:
        for w in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 31, 32, 33, 46, 77):
            img = R.content("noise", h, w, 3)
            for q in (50, 1):
                d = differing(img, q)
                if d:
                    bad.append((h, w, q, d))
    assert not bad, "%d of the (h, w, quality) cases differ, the first: %s" % (len(bad), bad[:5])


@needs_turbo
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_quality_and_kind_of_content_against_pillow(kind):
    bad = []
    for q in QUALITIES:
        for h, w in ((16, 16), (18, 21), (23, 40), (46, 46), (48, 80), (2, 5), (8, 8), (13, 4)):
            d = differing(R.content(kind, h, w, q), q)
            if d:
                bad.append((q, h, w, d))
    assert not bad, "%s: %s" % (kind, bad[:5])


@needs_turbo
def test_a_training_canvas_against_pillow():
    for kind in R.KINDS:
        assert differing(R.content(kind, 368, 368, 1), 50) == 0, kind


@needs_turbo
def test_derived_tables_against_image_quantization():
    img = R.content("noise", 16, 16)
    for q in range(1, 101):
        f = io.BytesIO()
        Image.fromarray(img).save(f, "jpeg", quality=q)
        tables = Image.open(f).quantization
        luma, chroma = R.quant_tables(q)
        assert list(tables[0]) == luma.tolist() and list(tables[1]) == chroma.tolist(), q
    assert R.quant_tables(100)[0].tolist() == [1] * 64 and R.quant_tables(1)[1].max() == 255
    for q in (0, 101):
        with pytest.raises(ValueError):
            R.quant_tables(q)


def test_range_limit_against_libjpegs_table():
    """prepare_range_limit_table of jdmaster.c, literally: 256 zeros, the identity, 255s to the middle of the post-IDCT
    part, zeros, and the first half of the identity again; the IDCT indexes it at CENTERJSAMPLE + (x & RANGE_MASK)."""
    MAXJSAMPLE, CENTERJSAMPLE = 255, 128
    table = np.zeros(5 * (MAXJSAMPLE + 1) + CENTERJSAMPLE, np.int64)
    base = MAXJSAMPLE + 1                                   # sample_range_limit: negative subscripts reach the zeros
    table[base:base + MAXJSAMPLE + 1] = np.arange(MAXJSAMPLE + 1)
    post = base + CENTERJSAMPLE                             # where the post-IDCT table starts
    table[post + CENTERJSAMPLE:post + 2 * (MAXJSAMPLE + 1)] = MAXJSAMPLE
    table[post + 2 * (MAXJSAMPLE + 1):post + 4 * (MAXJSAMPLE + 1) - CENTERJSAMPLE] = 0
    table[post + 4 * (MAXJSAMPLE + 1) - CENTERJSAMPLE:post + 4 * (MAXJSAMPLE + 1)] = table[base:base + CENTERJSAMPLE]
    x = np.arange(-1024, 1024)
    want = table[post + (x & 1023)]
    assert np.array_equal(R.range_limit(x), want)
    inside = (x >= -512) & (x <= 511)
    assert np.array_equal(want[inside], np.clip(x[inside] + 128, 0, 255))
    assert R.range_limit(512) == 0 and R.range_limit(-513) == 255 and R.range_limit(1023) == 127     # the wrap


def test_the_edge_rule_is_not_padding_the_picture():
    """An even height that is no multiple of 16: chroma's padded rows repeat the chroma plane's last row, which differs
    from down-sampling a picture padded by its last row."""
    img = R.content("noise", 18, 21, 5)
    y, cb, cr = R.padded_planes(img)
    assert y.shape == (32, 32) and cb.shape == (16, 16)
    assert (cb[9:] == cb[8]).all() and (y[18:] == y[17]).all() and (y[:, 21:] == y[:, 20:21]).all()
    naive = R.downsample(R._pad_rows(R._pad_cols(R.rgb_to_ycc(img)[1], 32), 32))
    assert not np.array_equal(naive, cb)


def test_read_u8_is_the_jitters():
    import jitter_restate as J
    v = np.array([-3.0, 0.9, 254.99, 255.5, np.nan, np.inf], np.float32)
    assert J.read_u8(v).tolist() == [0, 0, 254, 255, 0, 255]


# ---- the C entry points ----------------------------------------------------------------------------------------------
def _imgs(capi, pairs):
    arr = (capi.JpegImage * max(len(pairs), 1))()
    for k, (s, d) in enumerate(pairs):
        arr[k].n_src, arr[k].n_dst = s, d
    return arr


def _call(capi, pairs=((0, 0),), count=None, cfg="default", src=1 << 20, dst=1 << 24, ws=64, wsb=1 << 20, null_images=False):
    if cfg == "default":
        cfg = capi.JpegCfg.make(40, 48, 50)
    return capi.lib.rtpose_jpeg_roundtrip_batch(None if null_images else _imgs(capi, pairs),
                                                len(pairs) if count is None else count,
                                                C.byref(cfg) if cfg is not None else None, C.c_void_p(src) if src else None,
                                                C.c_void_p(dst) if dst else None, C.c_void_p(ws) if ws else None, wsb, None)


def test_jpeg_refusals_name_the_argument(capi):
    """Every refusal comes before any launch (and before the pointers are looked at): no device needed."""
    def refused(text, **kw):
        rc = _call(capi, **kw)
        assert rc == -1, (kw, rc)
        assert "jpeg: " in capi.last_error() and text in capi.last_error(), (text, capi.last_error())
    refused("NULL images", null_images=True, count=1)
    refused("NULL src", src=None)
    refused("NULL dst", dst=None)
    refused("NULL workspace", ws=None)
    refused("NULL cfg", cfg=None)
    cfg = capi.JpegCfg.make(40, 48)
    cfg.struct_bytes = 8
    refused("struct_bytes", cfg=cfg)
    refused("cfg.quality 0", cfg=capi.JpegCfg.make(40, 48, 0))
    refused("cfg.quality 101", cfg=capi.JpegCfg.make(40, 48, 101))
    refused("h 0", cfg=capi.JpegCfg.make(0, 48))
    refused("h 65536", cfg=capi.JpegCfg.make(65536, 48))
    refused("w 0", cfg=capi.JpegCfg.make(40, 0))
    refused("w 65536", cfg=capi.JpegCfg.make(40, 65536))
    refused("count -1", count=-1)
    refused("not aligned to 8 bytes", ws=68)
    refused("image 0: n_src -1", pairs=[(-1, 0)])
    refused("image 1: n_src 65536", pairs=[(0, 0), (65536, 1)])
    refused("image 0: n_dst -1", pairs=[(0, -1)])
    refused("image 1: n_dst 65536", pairs=[(0, 0), (1, 65536)])
    refused("image 2: n_dst 7 appears twice", pairs=[(0, 7), (1, 3), (2, 7)])
    refused("image 1: dst == src with n_dst 2 != n_src 1", pairs=[(0, 0), (1, 2)], dst=1 << 20)
    image = 3 * 40 * 48 * 4
    refused("overlap", pairs=[(0, 0), (1, 1)], dst=(1 << 20) + image)                  # two views of one tensor
    refused("overlap", pairs=[(2, 0)], dst=(1 << 20) + 2 * image + 16)
    refused("workspace_bytes", wsb=8)
    # count == 0 is a no-op; the next check after these is the pointers', which needs a device.  A narrow canvas
    # (w < 5: the chroma plane is at most 2 samples wide, box replication) is served, not refused
    assert _call(capi, pairs=[], count=0) == 0
    rc = _call(capi, cfg=capi.JpegCfg.make(3, 4, 50))
    assert rc == -1 and "not device memory" in capi.last_error()
    # views of one tensor that do not touch: past the overlap check, on to the pointers'
    rc = _call(capi, pairs=[(0, 0), (1, 1)], dst=(1 << 20) + 2 * image)
    assert rc == -1 and "not device memory" in capi.last_error()


def test_jpeg_workspace_query(capi):
    """The decoded planes: Y h rows of w rounded up to 8, Cb and Cr ceil(h / 2) rows of ceil(w / 2) rounded up to 8,
    per image, the total rounded up to 256; 0 on bad arguments."""
    q = capi.lib.rtpose_jpeg_workspace_bytes

    def per_image(h, w):
        return (w + 7) // 8 * 8 * h + 2 * (((w + 1) // 2 + 7) // 8 * 8) * ((h + 1) // 2)

    for h, w in ((368, 368), (17, 31), (1, 1), (2, 5), (65535, 65535)):
        cfg = capi.JpegCfg.make(h, w)
        for n in (1, 3, 32, 35):
            assert q(C.byref(cfg), n) == (n * per_image(h, w) + 255) // 256 * 256, (h, w, n)
    cfg = capi.JpegCfg.make(368, 368)
    assert per_image(368, 368) == 368 * 368 + 2 * 184 * 184
    assert q(C.byref(cfg), 0) == 256 and q(C.byref(cfg), -1) == 0 and q(None, 1) == 0
    assert q(C.byref(capi.JpegCfg.make(368, 368, 0)), 1) == 0 and "quality" in capi.last_error()


def test_jpeg_structs_mirror_the_header(capi, tmp_path):
    """rtpose_jpeg_image / rtpose_jpeg_cfg against their ctypes mirrors (sizes and offsets from gcc)."""
    import shutil
    import subprocess
    assert shutil.which("gcc"), "gcc compiles the header as C"
    mirrors = {"rtpose_jpeg_image": capi.JpegImage, "rtpose_jpeg_cfg": capi.JpegCfg}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {']
    for st, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "jpeg_layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "jpeg_layout")],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "jpeg_layout")], check=True, stdout=subprocess.PIPE,
                                                   text=True).stdout.splitlines())
    for st, cls in mirrors.items():
        assert int(got[st]) == C.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)
    assert capi.JpegCfg.make(3, 4).quality == 50


def test_jpeg_roundtrip_is_built_with_the_decoder_flags():
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert re.search(r"build/jpeg_roundtrip\.o: CXXFLAGS \+= -fno-slp-vectorize -fno-vectorize", mk)
    assert re.search(r"^SRCS := .*\bjpeg_roundtrip\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS := .*-ffp-contract=off", mk, flags=re.M)
    src = open(os.path.join(ROOT, PKG_NAME, "csrc", "jpeg_roundtrip.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(double|atomic\w*)\b", code)
    assert len(re.findall(r"\(float\)\w", code)) == 1        # one cast to float: the final store


# ---- the host entry points -------------------------------------------------------------------------------------------
def test_host_entry_points_check_their_arguments(aug, capi):
    with pytest.raises(capi.RtposeError):
        aug.jpeg_roundtrip(torch.zeros(1, 3, 8, 8))                            # no CPU fallback
    with pytest.raises(ValueError):
        aug.jpeg_roundtrip(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        aug.jpeg_roundtrip(torch.zeros(3, 8, 8))
    cp = aug.draw_color_params(1)
    with pytest.raises(capi.RtposeError):
        aug.color_jitter(torch.zeros(1, 3, 8, 8), cp, jpeg=True)
    p = aug.draw_params([(40, 40)], square_edge=48, scale_range=1.0)
    with pytest.raises(ValueError):
        aug.augment_images([np.zeros((40, 40, 3), np.uint8)], p, device="cpu", jpeg=True)          # jpeg needs color
    with pytest.raises(ValueError):
        aug.train_batch([np.zeros((40, 40, 3), np.uint8)], [[]], jpeg=True)
    for fn in (aug.jpeg_roundtrip, aug.color_jitter, aug.augment_images, aug.train_batch):
        assert "section 4e" in " ".join(fn.__doc__.split()), fn.__name__
    doc = " ".join(aug.__doc__.split())
    out_of_scope = doc[doc.index("Out of scope:"):]
    assert "JPEG re-compression until section 4e" in out_of_scope and not out_of_scope.startswith("Out of scope: JPEG")
    for word in ("RandomRotate", "RescaleAbsolute", "MultiScale", "decoding", "DataLoader"):
        assert word in out_of_scope


def test_the_jpeg_keyword_draws_nothing(aug, capi):
    """The draws are draw_train_params' with or without the keyword: the generator ends in the same state."""
    images = [np.zeros((40 + k, 50, 3), np.uint8) for k in range(3)]
    sizes = [im.shape[:2] for im in images]
    torch.manual_seed(11)
    want_params = aug.draw_train_params(sizes)
    want = torch.get_rng_state()
    states = []
    for kw in (dict(color=True), dict(color=True, jpeg=False), dict(color=True, jpeg=True)):
        torch.manual_seed(11)
        with pytest.raises(capi.RtposeError):                # the draws are made, then the device path refuses the CPU
            aug.train_batch(images, [[]] * 3, device="cpu", **kw)
        states.append(torch.get_rng_state())
    assert all(torch.equal(s, want) for s in states)
    torch.manual_seed(11)
    assert aug.draw_train_params(sizes) == want_params
    import inspect
    assert "jpeg" not in inspect.signature(aug.draw_color_params).parameters
    assert inspect.signature(aug.color_jitter).parameters["jpeg"].default is False
    assert inspect.signature(aug.augment_images).parameters["jpeg"].default is False
    assert inspect.signature(aug.train_batch).parameters["jpeg"].default is False
