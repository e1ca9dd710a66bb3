"""GPU suite of the JPEG decoder (augment.decode_jpegs, csrc/jpeg_decode.hip, header section 4f): the device's pixels
against the numpy restatement (tests/jpeg_decode_restate.py), the fixtures Pillow made and - where it is built on
libjpeg-turbo - Pillow itself, byte for byte; batches of mixed sizes and modes; the C entry point inside sentinel-filled
buffers and every one of its refusals; the Pillow fallback; and train_batch from file bytes against train_batch from
Pillow-decoded arrays."""
import ctypes as C
import importlib
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

from conftest import PKG_NAME, ROOT

import jpeg_decode_restate as D
import jpeg_restate as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
GOLD_SKI = os.path.join(ROOT, "tests", "golden", "jpeg_decode_ski.npz")
TURBO = bool(features.check_feature("libjpeg_turbo"))
PIL_MODES = ("4:4:4", "4:2:2", "4:2:0", "gray")


@pytest.fixture(scope="module")
def aug(pkg):
    return importlib.import_module(PKG_NAME + ".augment")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    ends = [int(e) for e in g["file_ends"]]
    files = [g["files"][a:b].tobytes() for a, b in zip([0] + ends[:-1], ends)]
    sizes = [int(h) * int(w) * 3 for h, w in g["shapes"]]
    pend = np.cumsum(sizes)
    pixels = [g["pixels"][b - n:b].reshape(int(h), int(w), 3) for b, n, (h, w) in zip(pend, sizes, g["shapes"])]
    return dict(names=[str(n) for n in g["names"]], files=files, pixels=pixels, ski=g["file_ski"].tobytes(),
                ski_pixels=np.load(GOLD_SKI)["pixels"])


@pytest.fixture(scope="module")
def mixed():
    """35 files of mixed sizes and modes - two chunks of the launcher - and what the restatement makes of them."""
    files = []
    for k in range(35):
        size, mode = D.SIZES[(5 * k + 3) % 12], PIL_MODES[k % 4]
        variant = (None, "optimize", "restart_blocks", "restart_rows")[(k // 4) % 4]
        files.append(D.grid_file(size, mode, R.KINDS[k % 3], (50, 95, 10)[k % 3], variant))
    return files, [D.decode(f) for f in files]


def same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d of %d bytes differ" % (what, int((got != want).sum()), want.size)


# ---- bit equality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", PIL_MODES)
def test_the_grid_equals_the_restatement_and_pillow(cuda, aug, mode):
    """All 12 sizes x 2 kinds x qualities 50 and 95, the quality-1 and the restart-marker files of a mode, one batch."""
    files = [D.grid_file(size, mode, kind, q) for size in D.SIZES for kind in ("noise", "patches") for q in (50, 95)]
    files += [D.grid_file(size, mode, "binary", 1) for size in D.SIZES]
    files += [D.grid_file((33, 47), mode, "ramp", 75, v) for v in ("restart_blocks", "restart_rows", "optimize")]
    images, infos = aug.decode_jpegs(files, device=cuda, fallback=None)
    assert len(images) == len(files) == 63 and all(i["native"] and i["mode"] == mode for i in infos)
    for k, (f, im) in enumerate(zip(files, images)):
        assert im.device.type == "cuda" and im.is_contiguous()
        same(im, D.decode(f), "file %d against the restatement" % k)
        if TURBO:
            same(im, D.pil_decode(f), "file %d against Pillow" % k)


def test_the_fixture_files(cuda, aug, gold):
    images, infos = aug.decode_jpegs(gold["files"], device=cuda, fallback=None)
    for name, im, want in zip(gold["names"], images, gold["pixels"]):
        same(im, want, name)


def test_the_photo_and_full_size_files(cuda, aug, gold):
    """The reference's demo picture - 712 x 674, 4:4:0 - against the fixture, and one 368 x 368 file per mode."""
    files = [gold["ski"]] + [D.grid_file((368, 368), mode, "patches", 90) for mode in PIL_MODES]
    images, infos = aug.decode_jpegs(files, device=cuda, fallback=None)
    assert [i["mode"] for i in infos] == ["4:4:0"] + list(PIL_MODES) and infos[0]["width"] == 712
    same(images[0], gold["ski_pixels"], "the photo against the fixture")
    for k in range(1, 5):
        if TURBO:
            same(images[k], D.pil_decode(files[k]), "368 x 368 %s against Pillow" % PIL_MODES[k - 1])
        else:                # (the bit-serial restatement takes a second per file of this size)
            same(images[k], D.decode(files[k]), "368 x 368 %s against the restatement" % PIL_MODES[k - 1])
    paths = aug.decode_jpegs([gold["ski"]], device=cuda, workers=1, pinned=False)[0]
    assert torch.equal(paths[0], images[0])


# ---- batching --------------------------------------------------------------------------------------------------------
def test_a_batch_of_two_chunks_and_an_image_alone(cuda, aug, mixed):
    files, want = mixed
    images, infos = aug.decode_jpegs(files, device=cuda, fallback=None)
    for k in range(35):
        same(images[k], want[k], "image %d of the batch" % k)
    again, _ = aug.decode_jpegs(files, device=cuda, fallback=None)
    assert all(torch.equal(a, b) for a, b in zip(images, again))
    for k in (0, 17, 33, 34):
        alone, _ = aug.decode_jpegs([files[k]], device=cuda, fallback=None)
        assert torch.equal(alone[0], images[k]), k


def test_files_may_be_paths(cuda, aug, mixed, tmp_path):
    files, want = mixed
    paths = []
    for k in range(3):
        paths.append(tmp_path / ("f%d.jpg" % k))
        paths[-1].write_bytes(files[k])
    images, _ = aug.decode_jpegs([str(paths[0]), paths[1], files[2]], device=cuda)
    for k in range(3):
        same(images[k], want[k], "path %d" % k)


# ---- the C entry point -----------------------------------------------------------------------------------------------
def stage(capi, files, device):
    """The host stage by hand: -> (coef device tensor, descriptors without destinations, infos)."""
    infos, words = [], 0
    for f in files:
        info = capi.JpegInfo()
        assert capi.lib.rtpose_jpeg_probe(f, len(f), C.byref(info)) == 0
        infos.append(info)
        words += 192 + int(info.coef_count)
    host = np.zeros(words, np.int16)
    descs = (capi.JpegDecodeImage * len(files))()
    at = 0
    for f, info, d in zip(files, infos, descs):
        base = host.ctypes.data + 2 * at
        assert capi.lib.rtpose_jpeg_entropy_decode(f, len(f), C.byref(info), base + 384, int(info.coef_count), base) == 0
        d.width, d.height, d.mode, d.qtab_offset, d.coef_offset = info.width, info.height, info.mode, at, at + 192
        at += 192 + int(info.coef_count)
    return torch.from_numpy(host).to(device), descs, infos


def test_nothing_outside_the_images_is_written(cuda, capi, mixed):
    files, want = mixed
    files, want = files[:9], want[:9]
    coef, descs, infos = stage(capi, files, cuda)
    gap = 64
    sizes = [w.size for w in want]
    starts = np.cumsum([gap] + [(s + gap + 3) // 4 * 4 for s in sizes])[:-1]
    buf = torch.full((int(starts[-1]) + sizes[-1] + gap,), 0xC3, dtype=torch.uint8, device=cuda)
    for d, s in zip(descs, starts):
        d.dst = buf.data_ptr() + int(s)
    wb = capi.lib.rtpose_jpeg_decode_workspace_bytes(descs, len(files))
    assert wb > 0 and wb % 256 == 0
    ws = torch.full((wb // 8 + 8,), 0x3c3c3c3c3c3c3c3c, dtype=torch.int64, device=cuda)
    capi.check(capi.lib.rtpose_jpeg_decode_batch(descs, len(files), capi.ptr(coef), coef.numel(), capi.ptr(ws), wb,
                                                 capi.current_stream()))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    covered = np.zeros(got.size, bool)
    for k, (s, n) in enumerate(zip(starts, sizes)):
        same(got[s:s + n].reshape(want[k].shape), want[k], "image %d in the sentinel buffer" % k)
        covered[s:s + n] = True
    assert (got[~covered] == 0xC3).all(), "a byte outside h * w * 3 changed"
    assert (ws[wb // 8:].cpu().numpy() == 0x3c3c3c3c3c3c3c3c).all(), "the workspace was overrun"


def test_every_refusal_of_the_launcher(cuda, capi, mixed):
    files = mixed[0][:2]
    coef, descs, infos = stage(capi, files, cuda)
    outs = [torch.zeros((i.height, i.width, 3), dtype=torch.uint8, device=cuda) for i in infos]
    for d, o in zip(descs, outs):
        d.dst = o.data_ptr()
    wb = capi.lib.rtpose_jpeg_decode_workspace_bytes(descs, 2)
    ws = torch.empty(wb // 8 + 1, dtype=torch.int64, device=cuda)

    def call(descs=descs, count=2, coef_ptr=None, words=None, ws_ptr=None, ws_bytes=wb):
        return capi.lib.rtpose_jpeg_decode_batch(descs, count, C.c_void_p(coef.data_ptr() if coef_ptr is None else coef_ptr),
                                                 coef.numel() if words is None else words,
                                                 C.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), ws_bytes,
                                                 capi.current_stream())

    def refused(text, **kw):
        assert call(**kw) == -1, text
        assert text in capi.last_error(), capi.last_error()

    def variant(**fields):
        v = (capi.JpegDecodeImage * 2)()
        for k in range(2):
            for name, _ in capi.JpegDecodeImage._fields_:
                setattr(v[k], name, getattr(descs[k], name))
        for name, value in fields.items():
            setattr(v[1], name, value)
        return v

    assert call() == 0
    assert call(count=0) == 0
    refused("NULL images", descs=None)
    refused("NULL coef", coef_ptr=0)
    refused("NULL workspace", ws_ptr=0)
    refused("negative", count=-1)
    refused("16 bytes", coef_ptr=coef.data_ptr() + 2)
    refused("8 bytes", ws_ptr=ws.data_ptr() + 4)
    refused("below", ws_bytes=wb - 1)
    for w, h in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5)):
        refused("outside [1,16384]", descs=variant(width=w, height=h))
    refused("unknown mode", descs=variant(mode=5))
    refused("unknown mode", descs=variant(mode=-1))
    refused("reserved", descs=variant(reserved=1))
    refused("NULL dst", descs=variant(dst=None))
    refused("4 bytes", descs=variant(dst=outs[1].data_ptr() + 1))
    refused("beyond", descs=variant(coef_offset=descs[1].coef_offset + 8))           # its last block ends behind coef
    refused("beyond", descs=variant(coef_offset=descs[1].coef_offset + 4))           # no multiple of 8
    refused("beyond", descs=variant(coef_offset=1 << 62))
    refused("beyond", words=coef.numel() - 1)
    refused("beyond", descs=variant(qtab_offset=coef.numel() - 184))
    refused("beyond", descs=variant(qtab_offset=4))
    refused("overlap", descs=variant(dst=outs[0].data_ptr()))
    assert capi.lib.rtpose_jpeg_decode_workspace_bytes(variant(mode=9), 2) == 0
    assert capi.lib.rtpose_jpeg_decode_workspace_bytes(descs, -1) == 0
    host = np.zeros(16, np.uint8)
    refused("not device memory", descs=variant(dst=host.ctypes.data))
    torch.cuda.synchronize()


# ---- the fallback ----------------------------------------------------------------------------------------------------
def test_a_progressive_file_among_baseline_ones(cuda, aug, mixed):
    files, want = mixed
    img = R.content("patches", 40, 56)
    f = io.BytesIO()
    Image.fromarray(img).save(f, "jpeg", quality=80, progressive=True)
    prog = f.getvalue()
    images, infos = aug.decode_jpegs([files[0], prog, files[1]], device=cuda)
    assert [i["native"] for i in infos] == [True, False, True] and "baseline" in infos[1]["reason"]
    assert (infos[1]["height"], infos[1]["width"]) == (40, 56)
    same(images[1], D.pil_decode(prog), "the progressive file through Pillow")
    same(images[0], want[0], "its neighbour 0")
    same(images[2], want[1], "its neighbour 2")
    with pytest.raises(aug._capi.RtposeError, match="baseline"):
        aug.decode_jpegs([files[0], prog], device=cuda, fallback=None)
    with pytest.raises(ValueError):
        aug.decode_jpegs([files[0]], device=cuda, fallback="cv2")
    assert aug.decode_jpegs([], device=cuda) == ([], [])


# ---- the training item from file bytes -------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
def test_train_batch_from_file_bytes(cuda, aug, color):
    sizes = ((200, 260), (427, 640), (97, 131), (368, 368))
    files = [D.pil_file(R.content("patches", h, w, seed=k), PIL_MODES[k], 90) for k, (h, w) in enumerate(sizes)]
    arrays = [D.pil_decode(f) for f in files]
    anns = [[dict(keypoints=sum([[30.0 + 5 * j, 40.0 + 4 * j, 2.0] for j in range(17)], []), bbox=[10, 10, 80, 90])], [], [], []]
    kw = dict(color=True, jpeg=True) if color else {}
    torch.manual_seed(11)
    want = aug.train_batch(arrays, anns, device=cuda, **kw)
    torch.manual_seed(11)
    got = aug.train_batch(files, anns, device=cuda, **kw)
    if TURBO:
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b)
    else:                    # another libjpeg: Pillow's arrays differ legitimately; the restatement's do not
        torch.manual_seed(11)
        want = aug.train_batch([D.decode(f) for f in files], anns, device=cuda, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
    assert [m["decoded_native"] for m in got[3]] == [True] * 4 and "decoded_native" not in want[3][0]
    assert [m["width_height"].tolist() for m in got[3]] == [m["width_height"].tolist() for m in want[3]]
    torch.manual_seed(11)
    params = aug.draw_params(sizes)
    mixed_in = [files[0], arrays[1], torch.from_numpy(arrays[2]).to(cuda), files[3]]
    a = aug.augment_images(mixed_in, params, device=cuda)
    b = aug.augment_images([D.decode(f) for f in files], params, device=cuda)
    assert torch.equal(a, b)
