#!/usr/bin/env python
"""Writes tests/golden/jpeg_decode.npz and tests/golden/jpeg_decode_ski.npz: JPEG files and what Pillow decodes from them, for the tests of the JPEG decoder
(header section 4f) on machines whose Pillow sits on another libjpeg - or to notice when Pillow's bits move.

    python tools/make_golden_jpeg_decode.py [--ski PATH]

Pillow's own ``save`` writes the files, its own ``open(...).convert('RGB')`` the pixels: a subset of the grid of
tests/jpeg_decode_restate.py (all sizes x 4 modes x three kind / quality pairs, the restart-marker and optimize files)
and - the only 4:4:0 file, Pillow cannot write that mode - the upstream project's demo picture readme/ski.jpg
(``--ski``; kept from the existing fixture when not given).  ``names`` lists the files; ``files`` holds their bytes one
after another, file k ending at ``file_ends[k]``; ``pixels`` likewise their decoded [h, w, 3] images of ``shapes[k]``;
``file_ski`` the photo's bytes; ``meta`` is a JSON string naming the Pillow and libjpeg versions.  The photo's 1.4 MB of pixels live in a file of their own, jpeg_decode_ski.npz (``pixels``),
so that each fixture stays below the repository's size limit for a committed file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_decode_restate as jd  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
OUT_SKI = os.path.join(ROOT, "tests", "golden", "jpeg_decode_ski.npz")


def subset():
    """-> [(name, bytes)]: a subset of the files of the device tests."""
    out = []
    for size in jd.SIZES:
        for mode in ("4:4:4", "4:2:2", "4:2:0", "gray"):
            for kind, quality in (("noise", 50), ("patches", 95), ("binary", 1)):
                out.append(("%dx%d_%s_%s_q%d" % (size + (mode, kind, quality)), jd.grid_file(size, mode, kind, quality)))
    for mode in ("4:4:4", "4:2:2", "4:2:0", "gray"):
        for variant in ("restart_blocks", "restart_rows", "optimize"):
            out.append(("33x47_%s_ramp_q75_%s" % (mode, variant), jd.grid_file((33, 47), mode, "ramp", 75, variant)))
    return out


def main():
    from PIL import __version__ as pil_version, features
    ap = argparse.ArgumentParser()
    ap.add_argument("--ski", help="path of the upstream project's readme/ski.jpg")
    args = ap.parse_args()
    names, files, pixels = [], [], []
    for name, data in subset():
        names.append(name)
        files.append(np.frombuffer(data, np.uint8))
        pixels.append(jd.pil_decode(data))
    ski = open(args.ski, "rb").read() if args.ski else np.load(OUT)["file_ski"].tobytes()
    meta = np.array(json.dumps(dict(pillow=pil_version, libjpeg=features.version("jpg"),
                                    libjpeg_turbo=bool(features.check_feature("libjpeg_turbo")))))
    np.savez_compressed(OUT, names=np.array(names), files=np.concatenate(files),
                        file_ends=np.cumsum([f.size for f in files]), shapes=np.array([p.shape[:2] for p in pixels]),
                        pixels=np.concatenate([p.reshape(-1) for p in pixels]), file_ski=np.frombuffer(ski, np.uint8),
                        meta=meta)
    np.savez_compressed(OUT_SKI, pixels=jd.pil_decode(ski), meta=meta)
    for path in (OUT, OUT_SKI):
        print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
