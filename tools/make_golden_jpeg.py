"""Generates tests/golden/jpeg_roundtrip.npz with Pillow itself (needs Pillow; no reference tree, no torchvision).

    python tools/make_golden_jpeg.py [--out PATH]

``jpeg_compression_augmentation`` of the reference (lib/datasets/transforms.py:28-31) saves the PIL image with
``image.save(f, 'jpeg', quality=50)`` and re-opens it.  The fixture holds that round trip, made by Pillow's own ``save``
and ``open``, for a handful of small images at qualities 1, 50 and 95.  Per case <c>: in_<c> the uint8 [h, w, 3] input,
q<quality>_<c> the uint8 [h, w, 3] image Pillow gave back.  ``table_luma`` / ``table_chroma`` are the two quantiser tables
of a quality-50 file as ``Image.quantization`` reports them (the base tables of the JPEG specification's Annex K).  The
bits are libjpeg-turbo's: ``meta`` names the Pillow version, ``features.version('jpg')`` and
``features.check_feature('libjpeg_turbo')``; a Pillow built on another libjpeg may legitimately give other bits.  The file
is written with fixed zip timestamps: a second run reproduces it byte for byte.
"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_restate as R                                              # noqa: E402  (the four kinds of content)
from make_golden_encode import write_npz                              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_roundtrip.npz")
QUALITIES = (1, 50, 95)
# name: (kind of content, h, w): one MCU; an odd size that is no multiple of anything; an even height that is no
# multiple of 16 (the bottom-edge rule); the largest, a partial run of MCUs each way; a chroma plane 2 samples wide
CASES = {
    "one_mcu": ("noise", 16, 16),
    "odd": ("patches", 17, 31),
    "even_height": ("binary", 18, 21),
    "runs": ("ramp", 48, 80),
    "narrow": ("noise", 7, 4),
}


def pil_roundtrip(img, quality):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "jpeg", quality=quality)
    return np.array(Image.open(f).convert("RGB"), dtype=np.uint8)


def main():
    import PIL
    from PIL import Image, features
    out = OUT
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    arrays = {}
    for k, (name, (kind, h, w)) in enumerate(CASES.items()):
        img = R.content(kind, h, w, 300 + k)
        arrays["in_" + name] = img
        for q in QUALITIES:
            arrays["q%d_%s" % (q, name)] = pil_roundtrip(img, q)
    f = io.BytesIO()
    Image.fromarray(arrays["in_one_mcu"]).save(f, "jpeg", quality=50)
    tables = Image.open(f).quantization
    arrays["table_luma"] = np.array(tables[0], np.int32)
    arrays["table_chroma"] = np.array(tables[1], np.int32)
    meta = {"cases": list(CASES), "qualities": list(QUALITIES), "pillow": PIL.__version__, "numpy": np.__version__,
            "jpg": features.version("jpg"), "libjpeg_turbo": bool(features.check_feature("libjpeg_turbo")),
            "what": "Image.save(f, 'jpeg', quality=q) then Image.open(f), transforms.py:28-31 of the reference"}
    arrays["meta"] = np.array(json.dumps(meta))
    write_npz(out, arrays)
    print("wrote %s (%d bytes, %d cases, Pillow %s, jpg %s)" % (out, os.path.getsize(out), len(CASES), PIL.__version__,
                                                                meta["jpg"]))


if __name__ == "__main__":
    main()
