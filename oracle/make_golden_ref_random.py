"""Generates tests/golden/post_ref_random.npz with the REFERENCE's own C++.

Run where oracle/_ref was built (`make -C oracle` with the reference sources present):
    python oracle/make_golden_ref_random.py

The scenes are those of tests/test_oracle_cpu.py's comparisons of the process_paf restatement with the compiled
reference: 40 seeded stick-figure scenes (pkg.synth) and 6 pure-noise ones, joint lists from the oracle NMS.  For
each, the reference pafprocess.cpp - compiled unmodified - is called as lib/utils/paf_to_pose.py:381-403 calls it
(x8 INTER_NEAREST up-sampled maps) and its humans / scores / peak getters are stored, with a SHA-256 of the scene
(joint list + maps) so that a test can tell when the scene it regenerates is not the one the vectors were made on.
"""
import hashlib
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import post_oracle as po  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "post_ref_random.npz")
FIELDS = ("parts", "score", "line_x", "line_y")


def random_scenes(synth):
    """The 40 seeded multi-person scenes -> (trial, joint_list, heat, paf) of those with at least one peak."""
    rng = np.random.default_rng(42)
    for trial in range(40):
        hh, ww = int(rng.integers(12, 47)) * 8, int(rng.integers(12, 50)) * 8
        people = synth.random_people(rng, int(rng.integers(1, 12)), hh, ww, drop_prob=float(rng.uniform(0, 0.3)))
        heat, paf = synth.render(people, hh, ww, noise=float(rng.uniform(0.005, 0.08)), rng=rng)
        jl = po.nms(heat)
        if len(jl):
            yield trial, jl, heat, paf


def junk_scenes():
    """6 pure-noise scenes (hundreds of peaks, long candidate lists) -> (trial, joint_list, heat, paf)."""
    rng = np.random.default_rng(7)
    for trial in range(6):
        h, w = 20 + trial, 26 - trial
        heat = rng.uniform(0, 0.35, (h, w, 19)).astype(np.float32)
        paf = rng.uniform(-0.2, 1.0, (h, w, 38)).astype(np.float32)
        yield trial, po.nms(heat), heat, paf


def digest(jl, heat, paf):
    h = hashlib.sha256()
    for a in (jl, heat, paf):
        a = np.ascontiguousarray(a, dtype=np.float32)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def reference(jl, heat, paf):
    ref = po.ref_process_paf(jl, po.upsample_nearest(heat, 8), po.upsample_nearest(paf, 8))
    return {k: ref[k] for k in FIELDS}


def main():
    assert po.have_ref(), "oracle/_ref/libpafprocess_ref.so missing: run `make -C oracle` with the reference sources"
    synth = importlib.import_module("pytorch_realtime_multi-person_pose_estimation_amd.synth")
    out = {}
    for kind, scenes in (("random", random_scenes(synth)), ("junk", junk_scenes())):
        n = 0
        for trial, jl, heat, paf in scenes:
            key = "%s%d" % (kind, trial)
            out[key + "_digest"] = np.array(digest(jl, heat, paf))
            for k, v in reference(jl, heat, paf).items():
                out[key + "_" + k] = v
            n += 1
        out["n_" + kind] = np.int32(n)
        print("%s: %d scenes" % (kind, n))
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH) // 1024, "KiB")


if __name__ == "__main__":
    main()
