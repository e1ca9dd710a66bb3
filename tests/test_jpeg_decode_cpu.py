"""CPU suite of the JPEG decoder (augment.decode_jpegs, header section 4f): the numpy restatement
(tests/jpeg_decode_restate.py) against Pillow itself over the file grid, where Pillow is built on libjpeg-turbo, and
against the fixtures Pillow made (tools/make_golden_jpeg_decode.py -> tests/golden/jpeg_decode.npz,
jpeg_decode_ski.npz) everywhere; the library's host stage (csrc/jpeg_entropy.cpp, called through ctypes: it needs no
device) against the restatement's coefficients and tables, word for word, with no file of the grid refused; and every
refusal on hand-made files."""
import ctypes as C
import importlib
import io
import json
import os

import numpy as np
import pytest
from PIL import Image, features

from conftest import PKG_NAME, ROOT

import jpeg_decode_restate as D
import jpeg_restate as R

GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
GOLD_SKI = os.path.join(ROOT, "tests", "golden", "jpeg_decode_ski.npz")
TURBO = bool(features.check_feature("libjpeg_turbo"))
needs_turbo = pytest.mark.skipif(not TURBO, reason="this Pillow is not built on libjpeg-turbo: another libjpeg legitimately "
                                                   "gives other bits (the fixtures still pin the restatement)")
PIL_MODES = ("4:4:4", "4:2:2", "4:2:0", "gray")
# RTPOSE_JPEG_R_* of the header
(R_ARGUMENT, R_NOT_JPEG, R_SYNTAX, R_TRUNCATED, R_FRAME, R_PRECISION, R_QTABLE16, R_COMPONENTS, R_ADOBE, R_COLORSPACE,
 R_SAMPLING, R_SCANS, R_DNL, R_SIZE, R_CATEGORY, R_RUN, R_CODE, R_TABLE, R_RST, R_CAPACITY, R_RANGE, R_TRAILING) = range(1, 23)


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    ends = [int(e) for e in g["file_ends"]]
    files = [g["files"][a:b].tobytes() for a, b in zip([0] + ends[:-1], ends)]
    sizes = [int(h) * int(w) * 3 for h, w in g["shapes"]]
    pend = np.cumsum(sizes)
    pixels = [g["pixels"][b - n:b].reshape(int(h), int(w), 3) for b, n, (h, w) in zip(pend, sizes, g["shapes"])]
    return dict(names=[str(n) for n in g["names"]], files=files, pixels=pixels, ski=g["file_ski"].tobytes(),
                ski_pixels=np.load(GOLD_SKI)["pixels"], meta=json.loads(str(g["meta"])))


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


def host_stage(capi, data, capacity=None):
    """-> (reason, info, coef int16 [coef_count] or None, qtab uint16 [3, 64]): probe, then the entropy decode."""
    info = capi.JpegInfo()
    rc = capi.lib.rtpose_jpeg_probe(data, len(data), C.byref(info))
    assert rc == info.reason
    if rc:
        assert (info.width, info.height, info.coef_count) == (0, 0, 0), "a refused probe carries no geometry"
        return rc, info, None, None
    n = int(info.coef_count)
    coef = np.full(n + 64, 0x5a5a, np.int16)
    qtab = np.full((3, 64), 0xa5a5, np.uint16)
    rc = capi.lib.rtpose_jpeg_entropy_decode(data, len(data), C.byref(info), coef.ctypes.data,
                                             n if capacity is None else capacity, qtab.ctypes.data)
    assert (coef[n:] == 0x5a5a).all(), "the decode wrote behind coef_count"
    if rc:
        assert (qtab == 0xa5a5).all(), "a refused decode left tables"
    return rc, info, coef[:n], qtab


def check_file(capi, data, want_pixels=None):
    """The restatement against ``want_pixels``, the library's words against the restatement's."""
    hd, coefs, qtabs = D.coefficients(data)
    if want_pixels is not None:
        got = D.decode(data)
        assert got.shape == want_pixels.shape and np.array_equal(got, want_pixels), \
            "%d bytes differ from Pillow" % int((got != want_pixels).sum())
    rc, info, coef, qtab = host_stage(capi, data)
    assert rc == 0, "refused: " + capi.lib.rtpose_jpeg_reason_text(rc).decode()
    assert (info.width, info.height, D.MODES[info.mode]) == (hd["width"], hd["height"], hd["mode"])
    for c, blocks in enumerate(coefs):
        assert (info.blocks_y[c], info.blocks_x[c]) == blocks.shape[:2]
        mine = coef[int(info.coef_offset[c]):int(info.coef_offset[c]) + blocks.size]
        assert np.array_equal(mine, blocks.reshape(-1)), "component %d: coefficients differ" % c
        assert np.array_equal(qtab[c], qtabs[c])
    assert int(info.coef_count) == sum(b.size for b in coefs)


# ---- the grid, against Pillow itself ---------------------------------------------------------------------------------
@needs_turbo
@pytest.mark.parametrize("mode", PIL_MODES)
def test_the_grid_against_pillow_and_the_library_against_the_restatement(capi, mode):
    """12 sizes x 4 kinds x 6 qualities per mode, and the optimize / restart-marker variants: 0 differing bytes, 0
    differing words, 0 refusals."""
    n = 0
    for size in D.SIZES:
        for kind in R.KINDS:
            for quality in D.QUALITIES:
                data = D.grid_file(size, mode, kind, quality)
                check_file(capi, data, D.pil_decode(data))
                n += 1
        for variant in ("optimize", "restart_blocks", "restart_rows"):
            for kind in ("noise", "ramp"):
                data = D.grid_file(size, mode, kind, 75, variant)
                check_file(capi, data, D.pil_decode(data))
                n += 1
    assert n == 12 * 4 * 6 + 12 * 6


@needs_turbo
def test_restart_files_carry_restart_markers(capi):
    data = D.grid_file((33, 47), "4:2:0", "noise", 75, "restart_blocks")
    assert D.parse(data)["restart_interval"] == 1 and b"\xff\xd0" in data and b"\xff\xd7" in data
    rows = D.grid_file((33, 47), "4:2:0", "noise", 75, "restart_rows")
    assert D.parse(rows)["restart_interval"] == 3


@needs_turbo
def test_probe_agrees_with_pillow(aug):
    for size in D.SIZES:
        for mode in PIL_MODES:
            data = D.grid_file(size, mode, "ramp", 75)
            im = Image.open(io.BytesIO(data))
            p = aug.jpeg_probe(data)
            assert p["served"] and p["reason"] is None and p["mode"] == mode
            assert (p["width"], p["height"]) == im.size
            assert p["sampling"] == [(h, v) for _, h, v, _ in im.layer] and p["components"] == im.layers


# ---- the fixtures ----------------------------------------------------------------------------------------------------
def test_the_fixture_names_its_maker(gold):
    assert gold["meta"]["libjpeg_turbo"] is True and gold["meta"]["pillow"] and gold["meta"]["libjpeg"]
    assert len(gold["names"]) == len(gold["files"]) == len(gold["pixels"]) == 12 * 4 * 3 + 12
    assert os.path.getsize(GOLD) < 1 << 20 and os.path.getsize(GOLD_SKI) < 1 << 20


def test_restatement_and_library_on_the_fixture_files(capi, gold):
    for name, data, want in zip(gold["names"], gold["files"], gold["pixels"]):
        try:
            check_file(capi, data, want)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


def test_the_photo_from_the_fixture(capi, aug, gold):
    """The reference's demo picture: 712 x 674, luma sampled 1 x 2 - the only 4:4:0 file (Pillow cannot write one)."""
    p = aug.jpeg_probe(gold["ski"])
    assert (p["width"], p["height"], p["mode"], p["sampling"][0]) == (712, 674, "4:4:0", (1, 2))
    check_file(capi, gold["ski"], gold["ski_pixels"])
    if TURBO:
        assert np.array_equal(D.pil_decode(gold["ski"]), gold["ski_pixels"])


# ---- refusals --------------------------------------------------------------------------------------------------------
def _base(mode="4:2:0", quality=75, size=(33, 47), kind="noise", **save):
    return D.pil_file(R.content(kind, size[0], size[1]), mode, quality, **save)


def _segment(data, marker):
    """Offset of the first 0xFF ``marker`` segment in front of the scan."""
    p = 2
    while data[p + 1] != marker:
        assert data[p] == 0xFF and data[p + 1] != 0xDA
        p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
    return p


def _patched(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


def refused(capi, data, reason, stage):
    rc, info, coef, _ = host_stage(capi, data)
    assert rc == reason, "reason %d (%s), expected %d" % (rc, capi.lib.rtpose_jpeg_reason_text(rc).decode(), reason)
    assert (coef is None) == (stage == "probe")


def test_frames_that_are_not_baseline(capi):
    refused(capi, _base(progressive=True), R_FRAME, "probe")
    data = _base()
    sof = _segment(data, 0xC0)
    refused(capi, _patched(data, sof + 1, 0xC1), R_FRAME, "probe")      # extended sequential
    refused(capi, _patched(data, sof + 1, 0xC9), R_FRAME, "probe")      # arithmetic
    refused(capi, _patched(data, sof + 4, 12), R_PRECISION, "probe")


def test_cmyk_and_adobe(capi):
    f = io.BytesIO()
    Image.fromarray(R.content("noise", 16, 16)).convert("CMYK").save(f, "jpeg")
    rc = host_stage(capi, f.getvalue())[0]
    assert rc in (R_ADOBE, R_COMPONENTS)         # Pillow's CMYK files carry both an Adobe segment and four components
    data = _base()
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    refused(capi, data[:2] + adobe + data[2:], R_ADOBE, "probe")
    sof = _segment(data, 0xC0)
    four = bytearray(data)
    four[sof + 9] = 4
    assert host_stage(capi, bytes(four))[0] in (R_COMPONENTS, R_SYNTAX)
    rgb = bytearray(data)
    rgb[sof + 10], rgb[sof + 13], rgb[sof + 16] = b"RGB"
    refused(capi, bytes(rgb), R_COLORSPACE, "probe")


def test_sampling_size_and_tables(capi):
    data = _base()
    sof = _segment(data, 0xC0)
    for hv in (0x41, 0x14, 0x31, 0x44):
        refused(capi, _patched(data, sof + 11, hv), R_SAMPLING, "probe")
    refused(capi, _patched(data, sof + 14, 0x21), R_SAMPLING, "probe")            # chroma not 1 x 1
    gray = _base("gray")
    refused(capi, _patched(gray, _segment(gray, 0xC0) + 11, 0x22), R_SAMPLING, "probe")
    zero_w = bytearray(data)
    zero_w[sof + 7:sof + 9] = b"\x00\x00"
    refused(capi, bytes(zero_w), R_SIZE, "probe")
    wide = bytearray(data)
    wide[sof + 7:sof + 9] = (16385).to_bytes(2, "big")
    refused(capi, bytes(wide), R_SIZE, "probe")
    zero_h = bytearray(data)
    zero_h[sof + 5:sof + 7] = b"\x00\x00"
    refused(capi, bytes(zero_h), R_DNL, "probe")
    dqt = _segment(data, 0xDB)
    refused(capi, _patched(data, dqt + 4, 0x10 | data[dqt + 4]), R_QTABLE16, "probe")
    sos = _segment(data, 0xDA)
    refused(capi, _patched(data, sos + 6, 0x33), R_TABLE, "probe")               # Huffman tables 3 / 3: never defined
    refused(capi, _patched(data, sof + 12, 3), R_TABLE, "probe")                 # quantiser table 3
    refused(capi, _patched(data, sos + 4, 1), R_SCANS, "probe")                  # a scan of one component
    refused(capi, b"\x89PNG\r\n\x1a\n" + data, R_NOT_JPEG, "probe")
    refused(capi, b"", R_NOT_JPEG, "probe")


def test_a_second_scan_dnl_and_trailing_bytes(capi):
    data = _base()
    sos = _segment(data, 0xDA)
    n = 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    refused(capi, data[:-2] + data[sos:sos + n] + b"\x00\xff\xd9", R_SCANS, "decode")
    refused(capi, data[:-2] + b"\xff\xdc\x00\x04\x00\x21\xff\xd9", R_DNL, "decode")
    refused(capi, data[:-2] + b"\x12\x34\xff\xd9", R_TRAILING, "decode")
    refused(capi, data[:sos] + b"\xff\xdc\x00\x04\x00\x21" + data[sos:], R_DNL, "probe")
    assert host_stage(capi, data[:-2] + b"\xff\xff\xff\xd9")[0] == 0             # fill bytes in front of EOI are legal


def test_a_wrong_restart_number(capi):
    data = _base(restart_marker_blocks=1)
    assert host_stage(capi, data)[0] == 0
    at = data.index(b"\xff\xd1", _segment(data, 0xDA))
    refused(capi, _patched(data, at + 1, 0xD3), R_RST, "decode")
    first = data.index(b"\xff\xd0", _segment(data, 0xDA))
    assert host_stage(capi, data[:first] + data[first + 2:])[0] != 0             # a marker taken out


def test_truncation_is_refused_at_every_length_tried(capi):
    for data in (_base(), _base("gray", restart_marker_rows=1), _base("4:4:4", 95)):
        scan = _segment(data, 0xDA)
        for cut in sorted(set([0, 1, 2, 3, 20, scan, scan + 4, scan + 14, scan + 15, (scan + len(data)) // 2,
                               len(data) - 40, len(data) - 3, len(data) - 2, len(data) - 1])):
            rc = host_stage(capi, data[:cut])[0]
            assert rc != 0, "a file cut to %d of %d bytes was served" % (cut, len(data))
            if cut > scan + 14:
                assert rc == R_TRUNCATED, (cut, rc)


def test_a_product_beyond_int16_is_refused(capi):
    """Quality 100 keeps coefficients up to about +-1000; with every quantiser entry patched to 255 their products leave
    int16, where libjpeg-turbo's SIMD inverse DCT and its C code part ways."""
    data = _base("4:4:4", 100, kind="binary")
    assert host_stage(capi, data)[0] == 0
    b = bytearray(data)
    dqt = _segment(data, 0xDB)
    b[dqt + 5:dqt + 5 + 64] = bytes([255]) * 64
    refused(capi, bytes(b), R_RANGE, "decode")


def test_capacity_arguments_and_reason_texts(capi):
    data = _base()
    rc, info, coef, _ = host_stage(capi, data)
    assert rc == 0
    assert host_stage(capi, data, capacity=int(info.coef_count) - 1)[0] == R_CAPACITY
    other = _base(size=(8, 8))
    q = np.zeros((3, 64), np.uint16)
    assert capi.lib.rtpose_jpeg_entropy_decode(other, len(other), C.byref(info), coef.ctypes.data, coef.size,
                                               q.ctypes.data) == R_ARGUMENT     # another file's info
    assert capi.lib.rtpose_jpeg_entropy_decode(data, len(data), C.byref(info), None, coef.size, q.ctypes.data) == R_ARGUMENT
    assert capi.lib.rtpose_jpeg_probe(data, len(data), None) == R_ARGUMENT
    texts = [capi.lib.rtpose_jpeg_reason_text(r).decode() for r in range(0, 23)]
    assert len(set(texts)) == 23 and texts[0] == "served" and "int16" in texts[R_RANGE]
    assert capi.lib.rtpose_jpeg_reason_text(99).decode() == "unknown reason"


def test_corrupted_scans_are_served_or_refused(capi, gold):
    """One byte of a fixture file's scan overwritten, 2000 variants from a fixed seed: every call a result or a reason of
    the header - and the reasons that only damaged entropy-coded data can show are among them.  (The sweep under the
    sanitizers is tools/jpeg_entropy_check.cpp.)"""
    data = gold["files"][gold["names"].index("33x47_4:2:0_noise_q50")]
    scan = _segment(data, 0xDA) + 14
    rng = np.random.default_rng(27)
    seen = set()
    for _ in range(2000):
        b = bytearray(data)
        b[int(rng.integers(scan, len(data) - 2))] = int(rng.integers(0, 256))
        rc = host_stage(capi, bytes(b))[0]
        assert 0 <= rc <= R_TRAILING
        seen.add(rc)
    assert {0, R_RUN, R_CODE, R_TRUNCATED} <= seen, sorted(seen)
    # the standard tables hold no DC category above 11: give the first DC table nothing but 12s
    dht = _segment(data, 0xC4)
    assert data[dht + 4] == 0x00 and sum(data[dht + 5:dht + 21]) == 12
    b = bytearray(data)
    b[dht + 21:dht + 33] = bytes([12]) * 12
    refused(capi, bytes(b), R_CATEGORY, "decode")
    b[dht + 21:dht + 33] = bytes([16]) * 12            # a DC symbol above 15: libjpeg calls the table itself bad
    refused(capi, bytes(b), R_SYNTAX, "probe")


def test_ctypes_mirrors_have_the_layout_of_the_header_structs(capi, tmp_path):
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    mirrors = {"rtpose_jpeg_info": capi.JpegInfo, "rtpose_jpeg_decode_image": capi.JpegDecodeImage}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {']
    for st, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        for f, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f))
    lines += ['  printf("R_TRAILING %d\\n", (int)RTPOSE_JPEG_R_TRAILING);', '  printf("M_440 %d\\n", (int)RTPOSE_JPEG_440);',
              '  return 0;', '}']
    src = tmp_path / "abi_layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines())
    for st, cls in mirrors.items():
        assert int(got[st]) == C.sizeof(cls), (st, got[st], C.sizeof(cls))
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)
    assert int(got["R_TRAILING"]) == R_TRAILING == 22 and int(got["M_440"]) == 4 == D.MODES.index("4:4:0")
    assert capi.JPEG_MODES == D.MODES and (capi.JPEG_R_CAPACITY, capi.JPEG_R_RANGE) == (R_CAPACITY, R_RANGE)


def test_the_launcher_checks_its_arguments_on_the_host(capi):
    """The refusals that come before any HIP call need no device (the rest: tests/test_jpeg_decode_gpu.py)."""
    d = (capi.JpegDecodeImage * 2)()
    for k, (h, w, mode) in enumerate(((17, 31, 3), (5, 3, 0))):
        d[k].width, d[k].height, d[k].mode, d[k].dst = w, h, mode, 4096 * (k + 1)
    # 4:2:0 at 17 x 31: Y 17 rows of 32 bytes, Cb and Cr 9 rows of 16; gray 5 x 3: 5 rows of 8
    assert capi.lib.rtpose_jpeg_decode_workspace_bytes(d, 1) == 1024 >= 17 * 32 + 2 * 9 * 16
    assert capi.lib.rtpose_jpeg_decode_workspace_bytes(d, 2) == 1024 >= 17 * 32 + 2 * 9 * 16 + 5 * 8
    assert capi.lib.rtpose_jpeg_decode_workspace_bytes(d, 0) == 256
    assert capi.lib.rtpose_jpeg_decode_workspace_bytes(None, 1) == 0
    buf = np.zeros(4096, np.int16)
    at = buf.ctypes.data + (-buf.ctypes.data) % 16

    def call(images=d, count=2, coef=at, words=2048, ws=at, ws_bytes=1024):
        rc = capi.lib.rtpose_jpeg_decode_batch(images, count, C.c_void_p(coef), words, C.c_void_p(ws), ws_bytes, None)
        return rc, capi.last_error()

    for kw, text in ((dict(images=None), "NULL images"), (dict(coef=0), "NULL coef"), (dict(ws=0), "NULL workspace"),
                     (dict(count=-1), "negative"), (dict(coef=at + 2), "16 bytes"), (dict(ws=at + 4), "8 bytes")):
        rc, err = call(**kw)
        assert rc == -1 and text in err, (kw, err)
    d[1].mode = 7
    assert call()[0] == -1 and "unknown mode" in capi.last_error()
    d[1].mode, d[1].width = 0, 16385
    assert call()[0] == -1 and "outside [1,16384]" in capi.last_error()
    d[1].width = 3
    rc, err = call(words=24 * 64 - 1)                                    # image 0 has 16 + 4 + 4 blocks of 64 words
    assert rc == -1 and "image 0" in err and "beyond" in err
    d[1].dst = 4096 + 17 * 31 * 3                                        # 5677: right behind image 0, but odd
    rc, err = call()
    assert rc == -1 and "4 bytes" in err
    d[1].dst = 4096 + 17 * 31 * 3 - 1                                    # aligned, and on image 0's last byte
    rc, err = call()
    assert rc == -1 and "overlap" in err
    d[1].dst = 8192
    rc, err = call(ws_bytes=1023)
    assert rc == -1 and "below" in err
    rc, err = call()                                                     # all of the above in order; host memory is no device memory
    assert rc != 0 and "device" in err


def test_jpeg_probe_reports_a_refusal(aug):
    p = aug.jpeg_probe(_base(progressive=True))
    assert p["served"] is False and p["reason_code"] == R_FRAME and "baseline" in p["reason"] and p["width"] is None
