"""The JPEG round trip of the training canvas on one MI355X, with Pillow's save / open beside it for scale: JSON lines.

    timeout -k 10 300 python tools/bench_jpeg.py [--steps device,batch,host] [--iters 200] [--warmup 20] [--out FILE]

The scenes of tools/bench_augment.py (32 uint8 RGB sources of 640 x 427, factors 0.5 .. 1.0, flips alternating, canvas
368, ToTensor + Normalize and the valid-area mask on), the colour params of tools/bench_jitter.py (draw_color_params
under torch.manual_seed(25)); the JPEG draw is set by hand: on all 32 images, or on images 3, 14 and 27 - 3 of 32 is
what p = 0.1 gives on average.  Quality 50.  Give each step a `timeout` of its own (--steps takes one or more).

  device   rtpose_jpeg_roundtrip_batch (the codec launch and the up-sample launch) in place on the dense
           [32, 3, 368, 368] uint8-valued canvas the geometry launches wrote: median of `iters` calls timed one by one
           with device events, all 32 images listed and 3 of 32 listed.  The split between the two launches is not
           visible to events around one call: run this step with --iters 50 under `rocprofv3 --kernel-trace --stats` and
           read jpeg_codec_kernel / jpeg_upsample_kernel off the statistics
  batch    augment.train_batch(color=...) end to end without jpeg, with jpeg=True and 3 of 32 firing, with jpeg=True
           and all 32 firing, wall clock to a synchronised device: median of `iters` runs each, from host arrays and
           from device-resident sources
  host     the same 32 canvases through Image.save(f, 'jpeg', quality=50) and Image.open(f) of PIL on one core: median
           of `iters` runs, and the elements of the whole batch in which its result differs from the device's

By hand only: not a test, not read by bench.py.  --out appends the lines to a file as well.  Nothing on bench.py's path
changes with this step; to see that, run `python bench.py --gpus 1 --steps 10 --warmup 3` in this tree and in an export of
the parent commit built the same way, alternating (profiles/r26_jpeg.txt records three rounds of it).
"""
import argparse
import ctypes as C
import importlib
import io
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_augment import EDGE, H0, N, PKG, W0, batch_params  # noqa: E402

FEW = (3, 14, 27)
QUALITY = 50


def pil_roundtrip(canvases):
    from PIL import Image
    out = np.empty((N, 3, EDGE, EDGE), np.float32)
    for k, canvas in enumerate(canvases):
        f = io.BytesIO()
        Image.fromarray(canvas).save(f, "jpeg", quality=QUALITY)
        out[k] = np.asarray(Image.open(f).convert("RGB")).transpose(2, 0, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="device,batch,host")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = set(a.steps.split(","))
    if not steps <= {"device", "batch", "host"}:
        raise SystemExit("--steps takes device, batch and host")
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg needs an MI355X")
    dev = torch.device("cuda", 0)
    importlib.import_module(PKG)
    capi = importlib.import_module(PKG + "._capi")
    aug = importlib.import_module(PKG + ".augment")
    import augment_restate as R                     # the synthetic sources of the tests
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def stats(v):
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}

    sources = [R.synthetic_source(H0, W0, k) for k in range(N)]
    params = batch_params()
    torch.manual_seed(25)
    cparams = aug.draw_color_params(N)
    rng = np.random.default_rng(2)
    anns = [[{"keypoints": np.stack([rng.uniform(0, W0, 17), rng.uniform(0, H0, 17), rng.choice([1.0, 2.0], 17)], 1)
              .reshape(-1).tolist(), "bbox": [0.0, 0.0, float(W0), float(H0)]} for _ in range(2)] for _ in range(N)]
    shape = "%d sources of %d x %d, factors 0.5 .. 1.0, flips alternating, canvas %d, quality %d" % (N, W0, H0, EDGE, QUALITY)

    ups = [torch.from_numpy(s).to(dev) for s in sources]
    canvas = aug.augment_images(ups, params, norm=0, mask_valid=False)
    canvases_u8 = canvas.cpu().numpy().astype(np.uint8).transpose(0, 2, 3, 1)
    device_result = aug.jpeg_roundtrip(canvas, quality=QUALITY).cpu().numpy()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                      # microseconds

    if "device" in steps:
        cfg = capi.JpegCfg.make(EDGE, EDGE, QUALITY)
        for which in (list(range(N)), list(FEW)):
            n = len(which)
            descs = (capi.JpegImage * n)()
            for j, k in enumerate(which):
                descs[j].n_src = descs[j].n_dst = k
            ws = torch.empty(capi.lib.rtpose_jpeg_workspace_bytes(C.byref(cfg), n) // 8, dtype=torch.int64, device=dev)
            work = canvas.clone()
            us = [timed(lambda: aug.jpeg_enqueue(descs, n, cfg, work, work, ws)) for _ in range(a.warmup + a.iters)][a.warmup:]
            emit({"what": "rtpose_jpeg_roundtrip_batch (codec launch + up-sample launch), %d of %d images, in place" % (n, N),
                  "shape": shape, "iters": a.iters, "device_us": stats(us), "images_per_s": round(n / statistics.median(us) * 1e6)})

    def wall(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    if "batch" in steps:
        few = [dict(cp, jpeg=k in FEW) for k, cp in enumerate(cparams)]
        every = [dict(cp, jpeg=True) for cp in cparams]
        for what, imgs in (("host arrays", sources), ("device-resident sources", ups)):
            for name, cps, jpeg in (("color", few, False), ("color, jpeg=True with 3 of 32 firing", few, True),
                                    ("color, jpeg=True with 32 of 32 firing", every, True)):
                ms = wall(lambda: aug.train_batch(imgs, anns, params, color=cps, jpeg=jpeg), a.iters + 5)[5:]
                emit({"what": "augment.train_batch end to end, %s, %s" % (name, what),
                      "shape": shape + ", 2 people per image", "runs": a.iters, "wall_ms": stats(ms),
                      "images_per_s": round(N / statistics.median(ms) * 1e3)})
    if "host" in steps:
        import PIL
        from PIL import features
        ms = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            host_result = pil_roundtrip(canvases_u8)
            ms.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "the same 32 canvases through Image.save(f, 'jpeg', quality=%d) and Image.open(f) of PIL %s (jpg %s, "
                      "libjpeg_turbo %s) on one core" % (QUALITY, PIL.__version__, features.version("jpg"),
                                                         bool(features.check_feature("libjpeg_turbo"))),
              "runs": len(ms), "wall_ms": stats(ms), "ms_per_image": round(statistics.median(ms) / N, 2),
              "elements_differing_from_the_device": int((host_result != device_result).sum()),
              "elements": int(host_result.size)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
