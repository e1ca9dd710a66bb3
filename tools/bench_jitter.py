"""The colour jitter of the training canvas on one MI355X, with the PIL chain it replaces beside it for scale: JSON lines.

    timeout -k 10 600 python tools/bench_jitter.py [--iters 200] [--warmup 20] [--no-host] [--no-batch] [--out FILE]

The scenes of tools/bench_augment.py (32 uint8 RGB sources of 640 x 427, factors 0.5 .. 1.0, flips alternating, canvas
368, ToTensor + Normalize and the valid-area mask on), the colour params drawn by draw_color_params under
torch.manual_seed(25) with the reference's ranges (every image has all four operations, so every image takes the L-sum
pass).

  device   rtpose_jitter_batch (the L-sum launch and the apply launch) from the dense [32, 3, 368, 368] uint8-valued
           canvas the geometry launches wrote, in place: median of `iters` calls timed one by one with device events.
           The geometry launches with norm 0 and no mask are timed the same way beside it.  The split between the two
           jitter launches is not visible to events around one call: run this tool with --iters 50 --no-host --no-batch
           under `rocprofv3 --kernel-trace --stats` and read jitter_lsum_kernel / jitter_apply_kernel off the statistics
  batch    augment.train_batch end to end with and without color, wall clock to a synchronised device: median of
           `iters` runs each, from host arrays and from device-resident sources
  host     the same 32 canvases through ImageEnhance.Brightness / Contrast / Color and the HSV round trip of PIL, in
           each image's drawn order, on one core, then numpy for ToTensor + Normalize and the mask: median of `iters`
           runs, and the elements in which its result differs from the device's

By hand only: not a test, not read by bench.py.  --out appends the lines to a file as well.
"""
import argparse
import ctypes as C
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_augment import EDGE, H0, N, PKG, W0, batch_params  # noqa: E402


def pil_chain(canvases, cparams, masks):
    from PIL import Image, ImageEnhance
    mean = np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]
    std = np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]
    out = np.empty((N, 3, EDGE, EDGE), np.float32)
    for k, (canvas, cp, m) in enumerate(zip(canvases, cparams, masks)):
        im = Image.fromarray(canvas)
        for op in cp["order"]:
            if op == 0:
                im = ImageEnhance.Brightness(im).enhance(cp["brightness"])
            elif op == 1:
                im = ImageEnhance.Contrast(im).enhance(cp["contrast"])
            elif op == 2:
                im = ImageEnhance.Color(im).enhance(cp["saturation"])
            elif op == 3:
                h, s, v = im.convert("HSV").split()
                moved = Image.fromarray((np.array(h, dtype=np.uint8) + np.uint8(cp["hue_shift"])).astype(np.uint8))
                im = Image.merge("HSV", (moved, s, v)).convert("RGB")
        if cp["gray"]:
            lum = np.array(im.convert("L"), dtype=np.uint8)
            im = Image.fromarray(np.dstack([lum, lum, lum]))
        t = np.asarray(im).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
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
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jitter needs an MI355X")
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
    masks = [aug.transform_annotations([], (H0, W0), p)[3] for p in params]
    torch.manual_seed(25)
    cparams = aug.draw_color_params(N)
    rng = np.random.default_rng(2)
    anns = [[{"keypoints": np.stack([rng.uniform(0, W0, 17), rng.uniform(0, H0, 17), rng.choice([1.0, 2.0], 17)], 1)
              .reshape(-1).tolist(), "bbox": [0.0, 0.0, float(W0), float(H0)]} for _ in range(2)] for _ in range(N)]
    shape = "%d sources of %d x %d, factors 0.5 .. 1.0, flips alternating, canvas %d" % (N, W0, H0, EDGE)

    ups = [torch.from_numpy(s).to(dev) for s in sources]
    canvas = aug.augment_images(ups, params, norm=0, mask_valid=False)
    canvases_u8 = canvas.cpu().numpy().astype(np.uint8).transpose(0, 2, 3, 1)
    descs = (capi.JitterImage * N)()
    for k, (cp, m) in enumerate(zip(cparams, masks)):
        d = descs[k]
        for j in range(4):
            d.order[j] = cp["order"][j]
        d.factor[0], d.factor[1], d.factor[2] = cp["brightness"], cp["contrast"], cp["saturation"]
        d.hue_shift, d.gray, d.n_src, d.n_dst = cp["hue_shift"], int(cp["gray"]), k, k
        for j in range(4):
            d.mask[j] = m[j]
    cfg = capi.JitterCfg.make(EDGE, EDGE, 1, 1)
    dst = torch.empty_like(canvas)
    ws = torch.empty(capi.lib.rtpose_jitter_workspace_bytes(C.byref(cfg), N) // 4, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                      # microseconds
    us = [timed(lambda: aug.jitter_enqueue(descs, N, cfg, canvas, dst, None, ws)) for _ in range(a.warmup + a.iters)][a.warmup:]
    emit({"what": "rtpose_jitter_batch (L-sum launch + apply launch)", "shape": shape, "iters": a.iters,
          "device_us": stats(us), "images_per_s": round(N / statistics.median(us) * 1e6)})
    device_result = dst.cpu().numpy()

    gdescs = (capi.AugmentImage * N)()
    for k, p in enumerate(params):
        d = gdescs[k]
        d.img_rgb, d.h0, d.w0, d.hr, d.wr = ups[k].data_ptr(), H0, W0, p["hr"], p["wr"]
        d.hflip, d.crop_x, d.crop_y, d.n_index = int(p["hflip"]), p["crop_x"], p["crop_y"], k
        d.mask[0], d.mask[1], d.mask[2], d.mask[3] = 0, 0, EDGE, EDGE
    gcfg = capi.AugmentCfg.make(EDGE, EDGE, 0, 1)
    gws = torch.empty(capi.lib.rtpose_augment_workspace_bytes(C.byref(gcfg), N) // 4, dtype=torch.int32, device=dev)
    gdst = torch.empty_like(canvas)
    us = [timed(lambda: aug.augment_enqueue(gdescs, N, gcfg, gdst, None, gws)) for _ in range(a.warmup + a.iters)][a.warmup:]
    emit({"what": "rtpose_augment_batch with norm 0 and no mask (the geometry launches in front of the jitter)", "shape": shape,
          "iters": a.iters, "device_us": stats(us)})

    def wall(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    if not a.no_batch:
        for what, imgs in (("host arrays", sources), ("device-resident sources", ups)):
            for color in (False, True):
                ms = wall(lambda: aug.train_batch(imgs, anns, params, color=cparams if color else False), a.iters + 5)[5:]
                emit({"what": "augment.train_batch end to end, %s, %s" % ("color" if color else "no color", what),
                      "shape": shape + ", 2 people per image", "runs": a.iters, "wall_ms": stats(ms),
                      "images_per_s": round(N / statistics.median(ms) * 1e3)})
    if not a.no_host:
        import PIL
        ms = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            host_result = pil_chain(canvases_u8, cparams, masks)
            ms.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "the same 32 canvases through the ColorJitter chain of PIL " + PIL.__version__ + " + numpy on one core",
              "runs": a.iters, "wall_ms": stats(ms), "ms_per_image": round(statistics.median(ms) / N, 2),
              "elements_differing_from_the_device": int((host_result.view(np.uint32) != device_result.view(np.uint32)).sum())})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
