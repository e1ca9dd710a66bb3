"""Generates tests/golden/legacy_order.npz with the REFERENCE's own C++.

Run where oracle/_ref was built (`make -C oracle` with the reference sources present):
    python oracle/make_golden_legacy_order.py

The reference pafprocess.cpp - compiled unmodified - on joint lists in CALLER order (tests/crowd_scenes.py's permuted():
a peak's id is its arrival index, not its position in the part-major peak_infos_line) of the 20-person crowd and of the
tied field with 4225 equal-scoring candidates of one limb, on full-resolution maps.  Stored: its humans, scores and
peak getters, and a SHA-256 of the scene (joint list + maps), so that tests/test_decode_crowd_gpu.py can compare the
legacy process_paf with the reference where oracle/_ref is not at hand.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import crowd_scenes as cs  # noqa: E402
from oracle import post_oracle as po  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "legacy_order.npz")
SCENES = ("crowd20", "tied65")
FIELDS = ("parts", "score", "line_x", "line_y", "line_score")


def digest(jl, heat, paf):
    h = hashlib.sha256()
    for a in (jl, heat, paf):
        a = np.ascontiguousarray(a, dtype=np.float32)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def caller_order_list(name):
    """-> (joint list in caller order, heat, paf) of a scene of tests/crowd_scenes.py."""
    heat, paf = cs.scene(name)
    return cs.permuted(po.nms(heat, 18, 0.1, 1)), heat, paf


def main():
    assert po.have_ref(), "oracle/_ref/libpafprocess_ref.so missing: run `make -C oracle` with the reference sources"
    out = {}
    for name in SCENES:
        jl, heat, paf = caller_order_list(name)
        ref = po.ref_process_paf(jl, heat, paf)
        out[name + "_digest"] = np.array(digest(jl, heat, paf))
        for k in FIELDS:
            out[name + "_" + k] = ref[k]
        print("%s: %d peaks, %d humans" % (name, len(jl), len(ref["parts"])))
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH) // 1024, "KiB")


if __name__ == "__main__":
    main()
