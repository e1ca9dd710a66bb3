"""The training-batch augmentation on one MI355X, with the host chain it replaces beside it for scale: JSON lines.

    timeout -k 10 300 python tools/bench_augment.py [--iters 200] [--warmup 20] [--no-host] [--out FILE]

32 uint8 RGB sources of 640 x 427 (width x height), factors spread evenly over 0.5 .. 1.0, flips alternating, the crop in
the middle of its range, canvas 368, ToTensor + Normalize and the valid-area mask on.

  device   rtpose_augment_batch (the table launch and the fused launch) into a dense [32, 3, 368, 368] tensor, sources
           resident on the device: median of `iters` calls timed one by one with device events.  The split between the
           two launches is not visible to events around one call: run this tool with --iters 50 --no-host under
           `rocprofv3 --kernel-trace --stats` and read augment_table_kernel / augment_kernel off the kernel statistics
  batch    augment.train_batch end to end (uploads of the 32 sources, annotation bookkeeping on the host, both
           augmentation launches, encode_targets of 2 people per image), wall clock to a synchronised device: median of
           `iters` / 10 runs, from host arrays and from device-resident sources
  host     where PIL imports: the same batch through PIL on one core (FLIP_LEFT_RIGHT, resize BICUBIC, crop, paste on the
           fill, then numpy for ToTensor + Normalize and the mask), wall clock, best of 3

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
N, H0, W0, EDGE = 32, 427, 640, 368


def batch_params():
    out = []
    for k in range(N):
        f = 0.5 + 0.5 * k / (N - 1)
        wr, hr = int(W0 * f), int(H0 * f)
        out.append(dict(hflip=bool(k & 1), factor=f, hr=hr, wr=wr, crop_x=max(wr - EDGE, 0) // 2,
                        crop_y=max(hr - EDGE, 0) // 2, square_edge=EDGE))
    return out


def pil_chain(sources, params, masks):
    from PIL import Image
    mean = np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]
    std = np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]
    out = np.empty((N, 3, EDGE, EDGE), np.float32)
    for k, (src, p, m) in enumerate(zip(sources, params, masks)):
        im = Image.fromarray(src)
        if p["hflip"]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        im = im.resize((p["wr"], p["hr"]), Image.BICUBIC)
        w, h = min(EDGE, p["wr"] - p["crop_x"]), min(EDGE, p["hr"] - p["crop_y"])
        im = im.crop((p["crop_x"], p["crop_y"], p["crop_x"] + w, p["crop_y"] + h))
        canvas = Image.new("RGB", (EDGE, EDGE), (124, 116, 104))
        canvas.paste(im, (int((EDGE - w) / 2.0), int((EDGE - h) / 2.0)))
        t = np.asarray(canvas).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
        t = (t - mean) / std
        keep = np.zeros((EDGE, EDGE), bool)
        keep[m[1]:m[3], m[0]:m[2]] = True
        t[:, ~keep] = 0.0
        out[k] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs an MI355X")
    dev = torch.device("cuda", 0)
    importlib.import_module(PKG)
    capi = importlib.import_module(PKG + "._capi")
    aug = importlib.import_module(PKG + ".augment")
    import augment_restate as R                     # the synthetic sources of the tests
    import ctypes as C
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def stats(v):
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}

    sources = [R.synthetic_source(H0, W0, k) for k in range(N)]
    params = batch_params()
    masks = [aug.transform_annotations([], (H0, W0), p)[3] for p in params]
    rng = np.random.default_rng(2)
    anns = [[{"keypoints": np.stack([rng.uniform(0, W0, 17), rng.uniform(0, H0, 17), rng.choice([1.0, 2.0], 17)], 1)
              .reshape(-1).tolist(), "bbox": [0.0, 0.0, float(W0), float(H0)]} for _ in range(2)] for _ in range(N)]
    shape = "%d sources of %d x %d, factors 0.5 .. 1.0, flips alternating, canvas %d" % (N, W0, H0, EDGE)

    ups = [torch.from_numpy(s).to(dev) for s in sources]
    descs = (capi.AugmentImage * N)()
    for k, (p, m) in enumerate(zip(params, masks)):
        d = descs[k]
        d.img_rgb, d.h0, d.w0, d.hr, d.wr = ups[k].data_ptr(), H0, W0, p["hr"], p["wr"]
        d.hflip, d.crop_x, d.crop_y, d.n_index = int(p["hflip"]), p["crop_x"], p["crop_y"], k
        for j in range(4):
            d.mask[j] = m[j]
    cfg = capi.AugmentCfg.make(EDGE, EDGE, 1, 1)
    dst = torch.empty(N, 3, EDGE, EDGE, device=dev)
    ws = torch.empty(capi.lib.rtpose_augment_workspace_bytes(C.byref(cfg), N) // 4, dtype=torch.int32, device=dev)

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        aug.augment_enqueue(descs, N, cfg, dst, None, ws)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                      # microseconds
    us = [timed() for _ in range(a.warmup + a.iters)][a.warmup:]
    emit({"what": "rtpose_augment_batch (table launch + fused launch)", "shape": shape, "iters": a.iters,
          "device_us": stats(us), "images_per_s": round(N / statistics.median(us) * 1e6)})
    device_result = dst.cpu().numpy()

    def wall(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    runs = max(a.iters // 10, 3)
    for what, imgs in (("host arrays", sources), ("device-resident sources", ups)):
        ms = wall(lambda: aug.train_batch(imgs, anns, params), runs + 2)[2:]
        emit({"what": "augment.train_batch end to end, " + what, "shape": shape + ", 2 people per image", "runs": runs,
              "wall_ms": stats(ms), "images_per_s": round(N / statistics.median(ms) * 1e3)})
    if not a.no_host:
        try:
            import PIL
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                host_result = pil_chain(sources, params, masks)
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            emit({"what": "the same batch through PIL " + PIL.__version__ + " + numpy on one core", "wall_ms": round(best, 1),
                  "images_per_s": round(N / best * 1e3),
                  "elements_differing_from_the_device": int((host_result.view(np.uint32) != device_result.view(np.uint32)).sum())})
        except ImportError:
            emit({"what": "PIL chain", "skipped": "PIL does not import here"})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
