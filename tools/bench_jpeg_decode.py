"""The JPEG decoder (augment.decode_jpegs, header section 4f) on one MI355X, with Pillow's open().convert('RGB') beside
it: JSON lines.

    timeout -k 10 300 python tools/bench_jpeg_decode.py [--steps host,device,batch] [--iters 200] [--warmup 20]
                                                        [--photo FILE] [--out FILE]

The files: 32 synthetic sources of 640 x 427 (tools/bench_augment.py's scenes) saved by Pillow at quality 90, 4:2:0 -
hard-edged patches, so a photograph of the same size carries fewer coefficients per block - and one photograph:
--photo FILE, by default the upstream project's 712 x 674 readme/ski.jpg (4:4:0) as tests/golden/jpeg_decode.npz
keeps it.  Give each step a `timeout` of its own (--steps takes one or more).

  host     per file, on one core: rtpose_jpeg_probe + rtpose_jpeg_entropy_decode into a preallocated buffer, and Pillow's
           whole Image.open(f).convert('RGB') + np.asarray; the two alternate file by file within a run, median of
           `iters` runs per file, the medians of the 32 files summarised.  Then the 32 files per batch with workers=8:
           the host stage on a ThreadPoolExecutor, Pillow on a ThreadPoolExecutor (it releases the GIL while decoding)
  device   rtpose_jpeg_decode_batch on the staged coefficients of the 32 files (both launch kinds), device events around
           one call, median of `iters`; the bytes of the one host-to-device copy against the RGB upload it replaces.  The
           split between the launches is not visible to events around one call: run this step with --iters 50 under
           `rocprofv3 --kernel-trace --stats` in a run of its own and read jpeg_idct_kernel / jpeg_upsample_kernel
  batch    augment.decode_jpegs end to end (wall clock to a synchronised device); augment.train_batch from file bytes
           against train_batch from Pillow-decoded host arrays including that decode, alternating run by run

By hand only: not a test, not read by bench.py.  --out appends the lines to a file as well.
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
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_augment import H0, N, PKG, W0, batch_params  # noqa: E402


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="host,device,batch")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--photo", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = set(a.steps.split(","))
    if not steps <= {"host", "device", "batch"}:
        raise SystemExit("--steps takes host, device and batch")
    importlib.import_module(PKG)
    capi = importlib.import_module(PKG + "._capi")
    aug = importlib.import_module(PKG + ".augment")
    import augment_restate as R                     # the synthetic sources of the tests
    import jpeg_decode_restate as D
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def stats(v, nd=2):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    files = [D.pil_file(R.synthetic_source(H0, W0, k), "4:2:0", 90) for k in range(N)]
    shape = "%d synthetic files of %d x %d, quality 90, 4:2:0, %d KB on average" % (N, W0, H0, sum(map(len, files)) // N // 1024)
    if a.photo:
        photo = open(a.photo, "rb").read()
    else:                                            # the fixture of the tests carries the upstream demo picture
        photo = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))["file_ski"].tobytes()

    def host_stage_fn(data):
        info = capi.JpegInfo()
        assert capi.lib.rtpose_jpeg_probe(data, len(data), C.byref(info)) == 0
        coef = np.empty(int(info.coef_count), np.int16)
        q = np.empty((3, 64), np.uint16)

        def run():
            i2 = capi.JpegInfo()
            capi.lib.rtpose_jpeg_probe(data, len(data), C.byref(i2))
            assert capi.lib.rtpose_jpeg_entropy_decode(data, len(data), C.byref(i2), coef.ctypes.data, coef.size, q.ctypes.data) == 0
        return run

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    if "host" in steps:
        import PIL
        from PIL import features
        who = "PIL %s (jpg %s, libjpeg_turbo %s)" % (PIL.__version__, features.version("jpg"),
                                                      bool(features.check_feature("libjpeg_turbo")))
        for name, some in (("the synthetic files", files), ("the photograph", [photo] if photo else [])):
            if not some:
                continue
            runs = [host_stage_fn(f) for f in some]
            native, pil = [[] for _ in some], [[] for _ in some]
            for it in range(a.iters + 3):
                for k, f in enumerate(some):             # alternating: native, Pillow, next file
                    tn = clock(runs[k])
                    tp = clock(lambda: pil_decode(f))
                    if it >= 3:
                        native[k].append(tn)
                        pil[k].append(tp)
            emit({"what": "host stage (probe + entropy decode) per file, one core, %s" % name, "shape": shape if some is files else
                  "%d bytes" % len(photo), "runs_per_file": a.iters, "ms_median_over_files": stats([statistics.median(v) for v in native], 3)})
            emit({"what": "Image.open(f).convert('RGB') + np.asarray per file, one core, %s, %s" % (name, who),
                  "runs_per_file": a.iters, "ms_median_over_files": stats([statistics.median(v) for v in pil], 3)})
        runs = [host_stage_fn(f) for f in files]
        tn, tp = [], []
        with ThreadPoolExecutor(max_workers=8) as pool:
            for it in range(a.iters + 3):                # alternating batch by batch
                x = clock(lambda: list(pool.map(lambda r: r(), runs)))
                y = clock(lambda: list(pool.map(pil_decode, files)))
                if it >= 3:
                    tn.append(x)
                    tp.append(y)
        emit({"what": "the 32 files per batch on a ThreadPoolExecutor of 8: host stage", "runs": a.iters, "wall_ms": stats(tn),
              "ms_per_image": round(statistics.median(tn) / N, 3)})
        emit({"what": "the 32 files per batch on a ThreadPoolExecutor of 8: Pillow's whole decode", "runs": a.iters,
              "wall_ms": stats(tp), "ms_per_image": round(statistics.median(tp) / N, 3)})

    if steps & {"device", "batch"} and not torch.cuda.is_available():
        raise SystemExit("the device and batch steps need an MI355X")
    dev = torch.device("cuda", 0)

    if "device" in steps:
        infos, words = [], 0
        for f in files:
            info = capi.JpegInfo()
            capi.lib.rtpose_jpeg_probe(f, len(f), C.byref(info))
            infos.append(info)
            words += 192 + int(info.coef_count)
        host = np.zeros(words, np.int16)
        descs = (capi.JpegDecodeImage * N)()
        outs, at = [], 0
        for f, info, d in zip(files, infos, descs):
            base = host.ctypes.data + 2 * at
            assert capi.lib.rtpose_jpeg_entropy_decode(f, len(f), C.byref(info), base + 384, int(info.coef_count), base) == 0
            outs.append(torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=dev))
            d.width, d.height, d.mode, d.qtab_offset, d.coef_offset = info.width, info.height, info.mode, at, at + 192
            d.dst = outs[-1].data_ptr()
            at += 192 + int(info.coef_count)
        coef = torch.from_numpy(host).to(dev)
        wb = capi.lib.rtpose_jpeg_decode_workspace_bytes(descs, N)
        ws = torch.empty(wb // 8, dtype=torch.int64, device=dev)

        def call():
            capi.check(capi.lib.rtpose_jpeg_decode_batch(descs, N, capi.ptr(coef), coef.numel(), capi.ptr(ws), wb,
                                                         capi.current_stream()))
        us = []
        for it in range(a.warmup + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                us.append(e0.elapsed_time(e1) * 1e3)
        differing = sum(int((o.cpu().numpy() != pil_decode(f)).sum()) for o, f in zip(outs, files))
        emit({"what": "rtpose_jpeg_decode_batch (IDCT launch + up-sample launch), 32 images", "shape": shape, "iters": a.iters,
              "device_us": stats(us), "images_per_s": round(N / statistics.median(us) * 1e6),
              "h2d_bytes_coefficients_and_tables": int(host.nbytes), "h2d_bytes_rgb_upload_it_replaces": N * H0 * W0 * 3,
              "workspace_bytes": int(wb), "bytes_differing_from_pillow": differing})

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if "batch" in steps:
        ms = [wall(lambda: aug.decode_jpegs(files, device=dev)) for _ in range(a.iters + 5)][5:]
        emit({"what": "augment.decode_jpegs end to end, workers=8, pinned staging", "shape": shape, "runs": a.iters,
              "wall_ms": stats(ms), "images_per_s": round(N / statistics.median(ms) * 1e3)})
        if photo:
            ms = [wall(lambda: aug.decode_jpegs([photo], device=dev)) for _ in range(a.iters + 5)][5:]
            emit({"what": "augment.decode_jpegs end to end, the photograph alone", "runs": a.iters, "wall_ms": stats(ms)})
        params = batch_params()
        rng = np.random.default_rng(2)
        anns = [[{"keypoints": np.stack([rng.uniform(0, W0, 17), rng.uniform(0, H0, 17), rng.choice([1.0, 2.0], 17)], 1)
                  .reshape(-1).tolist(), "bbox": [0.0, 0.0, float(W0), float(H0)]} for _ in range(2)] for _ in range(N)]
        tb, tp = [], []
        for it in range(a.iters + 5):                    # alternating run by run
            x = wall(lambda: aug.train_batch(files, anns, params))
            y = wall(lambda: aug.train_batch([pil_decode(f) for f in files], anns, params))
            if it >= 5:
                tb.append(x)
                tp.append(y)
        emit({"what": "augment.train_batch end to end from file bytes (native decode, workers=8)", "shape": shape + ", 2 people per image",
              "runs": a.iters, "wall_ms": stats(tb), "images_per_s": round(N / statistics.median(tb) * 1e3)})
        emit({"what": "augment.train_batch end to end from Pillow-decoded host arrays, that decode (one core) included",
              "runs": a.iters, "wall_ms": stats(tp), "images_per_s": round(N / statistics.median(tp) * 1e3)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
