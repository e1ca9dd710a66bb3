"""Generates tests/golden/decode_coco18_records.npz: what the COCO-18 entry points write, recorded on an MI355X.

    python tools/make_golden_decode_records.py

The committed fixture was produced by commit 6840708's fixed COCO-18 kernels - the last commit at which
rtpose_decode_batch_ex / rtpose_nms_batch_ex ran kernels with the COCO-18 tables compiled in (__constant__ kPairs /
kPairNet) instead of the table-driven ones.  Since then both doors launch one kernel set, so the two-door equality of
tests/test_skeleton_gpu.py alone would compare a kernel with itself; this file is what pins the decoder to the records of
the kernels it replaced.  Regenerating it from a later commit records that commit's behaviour, not theirs: do that only
when a change of the records is intended, and say so.

Scenes, cases and key names are the test module's own (_door_scenes, DOOR_FLAGS, DOOR_CAPS, SWITCH_CAPS, _gold_key):
  decode  flags {0, 1, 2} x (max_peaks_per_part, max_humans) in {(32, 64), (111, 64)}, and at flags 0 the capacities on
          both sides of every launcher switch: (4, 4), (65, 64), (128, 64), (32, 400)
  nms     flags {0, 1, 2} at (32, 64)
Per case and scene batch the file holds the header words [0:8] of every record, a SHA-256 of the int32 words inside
decode.result_mask, and the records themselves, zero-filled outside the mask (what lets a failing test name the word).
Per scene batch it holds a SHA-256 of the input maps; the scene builder is seeded numpy and is run twice here, the two
runs must be byte-identical.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_skeleton_gpu as T  # noqa: E402

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"


def scenes_twice(synth):
    a, b = T._door_scenes(synth), T._door_scenes(synth)
    for (na, ha, pa), (nb, hb, pb) in zip(a, b):
        assert na == nb and ha.dtype == np.float32 and pa.dtype == np.float32
        assert ha.tobytes() == hb.tobytes() and pa.tobytes() == pb.tobytes(), "%s: the scene builder is not reproducible" % na
    return a


def main():
    synth = importlib.import_module(PKG + ".synth")
    scenes = scenes_twice(synth)
    if "--check-scenes" in sys.argv[1:]:        # no GPU needed
        for name, heat, paf in scenes:
            print("%-12s heat %-18s paf %-18s %s" % (name, heat.shape, paf.shape, T._maps_digest(heat, paf)))
        return
    capi = importlib.import_module(PKG + "._capi")
    dec = importlib.import_module(PKG + ".decode")
    cuda = torch.device("cuda:0")
    cases = [("decode", f, p, h) for f in T.DOOR_FLAGS for p, h in T.DOOR_CAPS]
    cases += [("decode", 0, p, h) for p, h in T.SWITCH_CAPS]
    cases += [("nms", f, 32, 64) for f in T.DOOR_FLAGS]
    out = {}
    for name, heat, paf in scenes:
        out["maps_" + name] = np.array(T._maps_digest(heat, paf))
        heat_d, paf_d = torch.from_numpy(heat).to(cuda), torch.from_numpy(paf).to(cuda)
        for kind, flags, pcap, hcap in cases:
            cfg = capi.DecodeCfg(18, 8, 0.1, pcap, hcap)
            rec = T._run(capi, cuda, heat_d, paf_d, cfg, None, flags, nms_only=(kind == "nms"))
            again = T._run(capi, cuda, heat_d, paf_d, cfg, None, flags, nms_only=(kind == "nms"))
            m = dec.result_mask(rec)
            assert np.array_equal(m, dec.result_mask(again)) and np.array_equal(rec[m], again[m]), "two runs differ"
            key = T._gold_key(kind, flags, pcap, hcap, name)
            out[key + "_header"] = rec[:, :8].copy()
            out[key + "_sha256"] = np.array(T._record_digest(rec, m))
            out[key + "_records"] = np.where(m, rec, 0).astype(np.int32)
            print("%-34s peaks %-20s humans %-14s overflow %s" % (key, rec[:, 0].tolist(), rec[:, 1].tolist(), rec[:, 2].tolist()))
    path = T.GOLD_RECORDS
    if "--out" in sys.argv[1:]:
        path = sys.argv[sys.argv.index("--out") + 1]
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d entries)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
