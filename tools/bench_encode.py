"""The target encoder and the stage-loss tail on one MI355X, with the host renderer beside them for scale: JSON lines.

    timeout -k 10 300 python tools/bench_encode.py [--iters 200] [--warmup 20] [--out FILE]

  encode   rtpose_encode_targets_skel (both launches) at 32 x 368 x 368, stride 8, 8 people per image, for COCO-18 and
           BODY_25: median of `iters` calls timed one by one with device events
  tail     the twelve rtpose_stage_mse reductions of encode.stage_losses on the stage views of a 32 x 368 x 368 rtpose_vgg
           plan (after one forward with keep_intermediates): median of `iters` tails
  host     wall-clock of synth.render_skeleton (numpy, noise off) for the same 32 scenes, once

By hand only: not a test, not read by bench.py.  --out appends the lines to a file as well.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
N, SIZE, STRIDE, PEOPLE = 32, 368, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encode needs an MI355X")
    dev = torch.device("cuda", 0)
    pkg = importlib.import_module(PKG)
    capi = importlib.import_module(PKG + "._capi")
    enc = importlib.import_module(PKG + ".encode")
    skm = importlib.import_module(PKG + ".skeleton")
    synth = importlib.import_module(PKG + ".synth")
    import skeleton_restate as sr                 # the standing-figure templates of the skeleton tests
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

    def median_us(fn):
        us = [timed(fn) for _ in range(a.warmup + a.iters)][a.warmup:]
        return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    import ctypes as C
    for name, s, template in (("COCO18", skm.COCO18, sr._COCO_TEMPLATE), ("BODY_25", skm.BODY_25, sr._BODY25_TEMPLATE)):
        rng = np.random.default_rng(1)
        scenes = [synth.spaced_people(rng, template, PEOPLE, SIZE, SIZE) for _ in range(N)]
        kp = np.zeros((N, PEOPLE, s.num_parts, 3))
        for i, people in enumerate(scenes):
            for k, p in enumerate(people):
                ok = ~np.isnan(p[:, 0])
                kp[i, k, ok, :2] = p[ok]
                kp[i, k, ok, 2] = 2.0
        cfg = capi.EncodeCfg.make(SIZE, SIZE, STRIDE, 7.0, s.background)
        skel = s.native()
        g = SIZE // STRIDE
        heat = torch.empty(N, g, g, s.heat_channels, device=dev)
        paf = torch.empty(N, g, g, s.paf_channels, device=dev)
        ws = torch.empty(capi.lib.rtpose_encode_workspace_bytes(C.byref(cfg), C.byref(skel), N, PEOPLE) // 8,
                         dtype=torch.float64, device=dev)
        kp_d = torch.from_numpy(kp).to(dev)
        cnt_d = torch.full((N,), PEOPLE, dtype=torch.int32, device=dev)
        t0 = time.perf_counter()
        for people in scenes:
            synth.render_skeleton(s, people, SIZE, SIZE, STRIDE, noise=0)
        host_ms = (time.perf_counter() - t0) * 1e3
        emit({"what": "encode", "skeleton": name, "shape": "%dx%dx%d stride %d, %d people" % (N, SIZE, SIZE, STRIDE, PEOPLE),
              "iters": a.iters, "device_us": median_us(lambda: enc.encode_enqueue(kp_d, cnt_d, cfg, skel, heat, paf, ws)),
              "host_render_skeleton_ms": round(host_ms, 1)})

    m = pkg.get_model('vgg19')
    m.load_state_dict(synth.he_init_state_dict(m, seed=0))
    m = m.to(dev).float().eval()
    x = torch.rand(N, 3, SIZE, SIZE, device=dev) - 0.5
    # the reductions' time does not depend on the values: random targets
    heat = torch.rand(N, 19, SIZE // STRIDE, SIZE // STRIDE, device=dev)
    paf = torch.rand(N, 38, SIZE // STRIDE, SIZE // STRIDE, device=dev) - 0.5
    heat_nhwc, paf_nhwc = heat.permute(0, 2, 3, 1).contiguous(), paf.permute(0, 2, 3, 1).contiguous()
    plan = m.forward_native(x, keep_intermediates=True)
    g = SIZE // STRIDE
    partials = torch.empty(capi.lib.rtpose_stage_mse_partials(N, g, g, 38), dtype=torch.float64, device=dev)
    losses = torch.empty(12, device=dev)
    emit({"what": "stage_losses tail (12 x rtpose_stage_mse)", "shape": "%dx%dx%d maps, 38 / 19 channels" % (N, g, g),
          "iters": a.iters, "device_us": median_us(lambda: enc.stage_mse_enqueue(plan, heat_nhwc, paf_nhwc, losses, partials)),
          "losses": [round(v, 6) for v in losses.cpu().tolist()]})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
