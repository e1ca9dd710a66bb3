"""The decoder alone on one MI355X, through the COCO-18 entry points and through the table-driven ones: JSON lines.

    python tools/bench_decode_skeleton.py [--iters 200] [--warmup 20] [--variants a,b,c] [--forward] [--bench]

Decode + record D2H of a 32 x 46 x 46 batch of synthetic scenes (decode.decode_enqueue + decode.fetch: the kernels, the
copy of the record block into pinned memory, the stream synchronisation), median / min / max of `iters` timed decodes
after `warmup` untimed ones, host clock:

  a  rtpose_decode_batch_ex                      COCO-18 scenes (synth.make_batch)
  b  rtpose_decode_batch_skel, COCO-18 preset    the same scenes
  c  rtpose_decode_batch_skel, BODY_25           BODY_25 scenes (synth.render_skeleton; 26 / 52 channels)

a and b time the SAME kernels through two doors (since the fixed COCO-18 copy was dropped, profiles/r12_one_decoder.txt):
a passes the library's built-in COCO-18 table and leaves header words 5 / 6 zero, b passes the caller's.  A difference
between them is run-to-run noise plus b's skeleton check on the host.

--forward: ms per OpenPose_Model(4, 2, 52, 26) forward of the same batch (32 x 3 x 368 x 368): the shortest forward a
BODY_25 decode has to hide under in the pipelined flow.  --bench: runs `python bench.py` (defaults) as a child process and
repeats its JSON line.  Variant a alone also runs on a tree that has no table-driven decoder (--variants a), which is how
two builds are compared: alternate them on one box.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
N, S = 32, 368


def timed_decodes(dec, heat, paf, skeleton, iters, warmup):
    n, h, w, ch = heat.shape
    capi = importlib.import_module(PKG + "._capi")
    lheat, lpaf = capi.Layout.dense(ch, h, w), capi.Layout.dense(paf.shape[3], h, w)
    cfg = dec.make_cfg(dec.default_config(skeleton) if skeleton is not None else None)
    bufs = dec.DecodeBuffers(cfg, n, heat.device, skeleton) if skeleton is not None else dec.DecodeBuffers(cfg, n, heat.device)
    ms = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode_enqueue(capi.ptr(heat), lheat, capi.ptr(paf), lpaf, n, h, w, bufs)
        recs = dec.fetch(bufs)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert not recs[:, dec.RES_HEADER + 2].any(), "a decode table overflowed"
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "iters": iters, "humans": int(recs[:, dec.RES_HEADER + 1].sum()), "peaks": int(recs[:, dec.RES_HEADER].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--variants", default="a,b,c")
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_skeleton needs an MI355X")
    dev = torch.device("cuda", 0)
    dec = importlib.import_module(PKG + ".decode")
    synth = importlib.import_module(PKG + ".synth")
    variants = a.variants.split(",")
    out = {"workload": "decode + record D2H, %d x 46 x 46 maps" % N, "tag": a.tag}
    h, p, _ = synth.make_batch(N, S, S, seed=1)
    heat, paf = torch.from_numpy(h).to(dev), torch.from_numpy(p).to(dev)
    if "a" in variants:
        out["a_old_entry_coco18"] = timed_decodes(dec, heat, paf, None, a.iters, a.warmup)
    if "b" in variants or "c" in variants:
        skm = importlib.import_module(PKG + ".skeleton")
    if "b" in variants:
        out["b_skel_entry_coco18"] = timed_decodes(dec, heat, paf, skm.COCO18, a.iters, a.warmup)
    if "c" in variants:
        import skeleton_restate as sr
        counts = [int(c) for c in np.random.default_rng(1).integers(1, 9, N)]      # 1..8 figures, like make_batch
        h25, p25 = sr.make_scenes(sr.TABLES["body25"], counts, S // 8, S // 8, 8, seed=1)
        out["c_skel_entry_body25"] = timed_decodes(dec, torch.from_numpy(h25).to(dev), torch.from_numpy(p25).to(dev),
                                                   skm.BODY_25, a.iters, a.warmup)
    if "a" in variants and "b" in variants:
        out["b_over_a"] = round(out["b_skel_entry_coco18"]["median_ms"] / out["a_old_entry_coco18"]["median_ms"], 3)
    if "a" in variants and "c" in variants:
        out["c_over_a"] = round(out["c_skel_entry_body25"]["median_ms"] / out["a_old_entry_coco18"]["median_ms"], 3)
    if a.forward:
        import openpose_restate as R
        op = importlib.import_module(PKG + ".openpose")
        m = op.OpenPose_Model(4, 2, 52, 26)
        m.load_state_dict(R.seeded_state_dict(R.state_dict_spec(4, 2, 52, 26), 3))
        m = m.cuda().eval()
        x = (torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(0)) - 0.5).to(dev)
        with torch.no_grad():
            for _ in range(3):
                m.forward_native(x)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                m.forward_native(x)
            e1.record()
            torch.cuda.synchronize()
        out["openpose_4_2_52_26_forward_ms"] = round(e0.elapsed_time(e1) / 10, 3)
    print(json.dumps(out), flush=True)
    if a.bench:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], stdout=subprocess.PIPE, text=True, check=True)
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
