"""The fused TTA merge and the flip merge alone on one MI355X, through the COCO-18 entry points and through the table-driven
ones: JSON lines.

    timeout -k 10 300 python tools/bench_tta_skeleton.py [--iters 200] [--warmup 20] [--rounds 3] [--out FILE]

The shapes are the four scales of BASELINE configs[2] for 368 x 368 images (B = 32, flip on): the stage-6 maps of 64
images at 23 x 23, 46 x 46, 69 x 69 and 92 x 92, read in place from a padded buffer laid out as a plan's output views are
(PAF and heat map as channel slices of one wider pixel, a gap of 3 around every image), accumulated into dense
32 x 46 x 46 maps; the first scale overwrites (beta 0), the others add (beta 1).  Per scale, `iters` launches of each of

  a  rtpose_tta_accumulate                       COCO-18 (38 / 19 channels at 2 / 41 of a 64-channel pixel)
  b  rtpose_tta_accumulate_skel, COCO-18 table   the same buffer and views
  c  rtpose_tta_accumulate_skel, BODY_25 table   52 / 26 channels at 2 / 60 of a 96-channel pixel
  d  rtpose_flip_merge                           the unfused merge: dense 32 x hs x ws x 19 / 38 maps of the scale and
  e  rtpose_flip_merge_skel, COCO-18 table       their mirrored passes into dense maps of the same size

are timed one by one with device events, a and b alternating launch by launch (c, d, e after each pair), after `warmup`
untimed rounds; the medians are reported, and the whole measurement is repeated `rounds` times so that the spread of the medians
from one round to the next can be read beside the b / a ratio.  Values are random; the kernels' time does not depend on
them.  --out appends the lines to a file as well.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
B, HD, WD = 32, 46, 46
SCALES = [(0.5, 23), (1.0, 46), (1.5, 69), (2.0, 92)]     # (scale, map side of the 368 * scale pass)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta_skeleton needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    skm = importlib.import_module(PKG + ".skeleton")
    lib, ptr = capi.lib, capi.ptr
    coco, body = skm.COCO18.native_flip_table(), skm.BODY_25.native_flip_table()
    stream = capi.current_stream()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                      # microseconds

    g = torch.Generator(device=dev).manual_seed(0)
    acc = {c: torch.zeros(B, HD, WD, c, device=dev) for c in (19, 38, 26, 52)}
    for rnd in range(a.rounds):
        total = {k: 0.0 for k in "abcde"}
        for si, (scale, hs) in enumerate(SCALES):
            ws = hs
            beta = 0.0 if si == 0 else 1.0

            def views(cstride, paf_off, heat_off):
                lp, lh = capi.Layout.padded(cstride, hs, ws, 3, paf_off), capi.Layout.padded(cstride, hs, ws, 3, heat_off)
                words = lib.rtpose_layout_pixels(C.byref(lp), 2 * B, hs, ws) * cstride
                return torch.randn(words, device=dev, generator=g), lp, lh
            buf18, lp18, lh18 = views(64, 2, 41)
            buf25, lp25, lh25 = views(96, 2, 60)
            common = (B, hs, ws)
            tail = (HD, WD, float(hs), float(ws), 0.25, beta, 1)

            def old():
                capi.check(lib.rtpose_tta_accumulate(ptr(buf18), C.byref(lh18), ptr(buf18), C.byref(lp18), *common,
                                                     ptr(acc[19]), ptr(acc[38]), *tail, stream))

            def new18():
                capi.check(lib.rtpose_tta_accumulate_skel(ptr(buf18), C.byref(lh18), ptr(buf18), C.byref(lp18), *common,
                                                          ptr(acc[19]), ptr(acc[38]), *tail, C.byref(coco), stream))

            def new25():
                capi.check(lib.rtpose_tta_accumulate_skel(ptr(buf25), C.byref(lh25), ptr(buf25), C.byref(lp25), *common,
                                                          ptr(acc[26]), ptr(acc[52]), *tail, C.byref(body), stream))
            dense = [torch.randn(B, hs, ws, c, device=dev, generator=g) for c in (19, 19, 38, 38)]
            merged = [torch.empty_like(dense[0]), torch.empty_like(dense[2])]
            margs = tuple(ptr(t) for t in dense) + (B, hs, ws, ptr(merged[0]), ptr(merged[1]))

            def merge_old():
                capi.check(lib.rtpose_flip_merge(*margs, stream))

            def merge_new():
                capi.check(lib.rtpose_flip_merge_skel(*margs, C.byref(coco), stream))
            us = {k: [] for k in "abcde"}
            for i in range(a.warmup + a.iters):
                for key, fn in (("a", old), ("b", new18), ("c", new25), ("d", merge_old), ("e", merge_new)):
                    t = timed(fn)
                    if i >= a.warmup:
                        us[key].append(t)
            med = {k: statistics.median(v) for k, v in us.items()}
            for k in total:
                total[k] += med[k]
            emit({"round": rnd, "scale": scale, "src": "%dx%dx%d" % (2 * B, hs, ws), "dst": "%dx%dx%d" % (B, HD, WD),
                  "iters": a.iters,
                  "a_old_coco18_us": {"median": round(med["a"], 2), "min": round(min(us["a"]), 2), "max": round(max(us["a"]), 2)},
                  "b_skel_coco18_us": {"median": round(med["b"], 2), "min": round(min(us["b"]), 2), "max": round(max(us["b"]), 2)},
                  "c_skel_body25_us": {"median": round(med["c"], 2), "min": round(min(us["c"]), 2), "max": round(max(us["c"]), 2)},
                  "d_old_flip_merge_us": {"median": round(med["d"], 2), "min": round(min(us["d"]), 2), "max": round(max(us["d"]), 2)},
                  "e_skel_flip_merge_us": {"median": round(med["e"], 2), "min": round(min(us["e"]), 2), "max": round(max(us["e"]), 2)},
                  "b_over_a": round(med["b"] / med["a"], 3), "e_over_d": round(med["e"] / med["d"], 3)})
            del buf18, buf25, dense, merged
        emit({"round": rnd, "four_scales_sum_of_medians_us": {k: round(v, 2) for k, v in total.items()},
              "b_over_a": round(total["b"] / total["a"], 3), "c_over_a": round(total["c"] / total["a"], 3),
              "e_over_d": round(total["e"] / total["d"], 3)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
