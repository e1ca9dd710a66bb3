"""Training the stacked hourglass on one MI355X: the BatchNorm passes next to torch's own, and one train_step.  JSON lines.

    timeout -k 10 900 python tools/bench_hourglass_train.py [--iters 200] [--warmup 10] [--no-step] [--batch 32] [--out FILE]

  bn       at 32 x 96 x 96 with 64, 128 and 256 channels and at 32 x 6 x 6 with 256 (the widest and the innermost maps of
           hg(8, 1, 38, 19) at 384 x 384), median of `iters` calls, timed one by one with device events, of
             fwd    rtpose_bn_stats + rtpose_bn_apply with ReLU (four launches; dense layouts, running statistics updated)
             grad   rtpose_bn_grad through the ReLU, dx in place on gy, with dweight and dbias (three launches)
           each next to torch.ops.aten.native_batch_norm (training) / native_batch_norm_backward on NCHW tensors of the same
           values on the same device - torch's pair has no ReLU in it -, with the bytes/s each achieves on the traffic the
           operation needs (fwd: read x twice, write y; grad: read x and gy twice, write dx), and the difference of the
           two weight gradients
  step     one train.train_step of hg(8, 1, 38, 19) at `batch` x 384 x 384 (SGD with momentum, masks of ones): wall clock of
           the second and third step after a first one that packs and allocates, and the peak memory

Nothing here is a pass criterion and no speed is promised: the lines say where torch is faster as well.  By hand only: not a
test, not read by bench.py.  --out appends the lines to a file as well.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
SHAPES = ((32, 64, 96, 96), (32, 128, 96, 96), (32, 256, 96, 96), (32, 256, 6, 6))
TOPO = dict(num_stacks=8, num_blocks=1, paf_classes=38, ht_classes=19)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hourglass_train needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    hourglass = importlib.import_module(PKG + ".hourglass")
    lib = capi.lib
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
        return round(statistics.median(us), 1)

    for n, ch, h, w in SHAPES:
        g = torch.Generator(device=dev).manual_seed(ch + h)
        x = torch.randn(n, ch, h, w, device=dev, generator=g) * 1.5 + 0.5
        gy = torch.randn(n, ch, h, w, device=dev, generator=g)
        wt, b = torch.rand(ch, device=dev, generator=g) + 0.5, torch.randn(ch, device=dev, generator=g) * 0.1
        rm, rv = torch.zeros(ch, device=dev), torch.ones(ch, device=dev)
        stream = capi.current_stream()
        xbuf, lx = train._to_layout(x, 0)
        gsrc, lg = train._to_layout(gy, 0)
        gbuf, ybuf = gsrc.clone(), torch.empty_like(xbuf)
        doubles = lib.rtpose_bn_workspace_doubles(ch, n, h, w)
        ws = torch.empty(doubles, dtype=torch.float64, device=dev)
        save = torch.empty(capi.BN_SAVE_ROWS * ch, device=dev)
        dw, db = torch.empty(ch, device=dev), torch.empty(ch, device=dev)

        def fwd():
            capi.check(lib.rtpose_bn_stats(capi.ptr(xbuf), C.byref(lx), capi.ptr(wt), capi.ptr(b), capi.ptr(rm), capi.ptr(rv), 0.1, 1e-5,
                                           capi.ptr(save), capi.ptr(ws), doubles, ch, n, h, w, stream), "rtpose_bn_stats")
            capi.check(lib.rtpose_bn_apply(capi.ptr(xbuf), C.byref(lx), capi.ptr(save), capi.ptr(ybuf), C.byref(lx), 1, ch, n, h, w,
                                           stream), "rtpose_bn_apply")

        def grad():
            capi.check(lib.rtpose_bn_grad(capi.ptr(xbuf), C.byref(lx), capi.ptr(gbuf), C.byref(lg), capi.ptr(save), capi.ptr(wt), 1,
                                          capi.ptr(gbuf), C.byref(lg), capi.ptr(dw), capi.ptr(db), capi.ptr(ws), doubles, ch, n, h, w,
                                          stream), "rtpose_bn_grad")
        elems = n * ch * h * w
        row = {"what": "bn", "channels": ch, "shape": "%dx%dx%d" % (n, h, w), "iters": a.iters,
               "slabs": lib.rtpose_bn_slabs(ch, n, h, w), "mbytes_fwd": round(12 * elems / 1e6, 2), "mbytes_grad": round(20 * elems / 1e6, 2)}
        # the weight gradient agrees with torch's, on the ReLU-masked gradient; taken before the in-place timing loop
        fwd()
        grad()
        y_t, mean_t, invstd_t = torch.ops.aten.native_batch_norm(x, wt, b, None, None, True, 0.1, 1e-5)
        gmask = torch.where(y_t > 0, gy, torch.zeros((), device=dev))
        _, dw_t, _ = torch.ops.aten.native_batch_norm_backward(gmask, x, wt, None, None, mean_t, invstd_t, True, 1e-5, [True, True, True])
        row["dweight_vs_torch_max_rel"] = float(((dw - dw_t).abs().max() / dw_t.abs().max()).item())
        trm, trv = torch.zeros(ch, device=dev), torch.ones(ch, device=dev)
        row["fwd_us"] = median_us(fwd)
        row["torch_fwd_us"] = median_us(lambda: torch.ops.aten.native_batch_norm(x, wt, b, trm, trv, True, 0.1, 1e-5))
        gbuf.copy_(gsrc)
        row["grad_us"] = median_us(grad)
        row["torch_grad_us"] = median_us(lambda: torch.ops.aten.native_batch_norm_backward(gy, x, wt, trm, trv, mean_t, invstd_t, True, 1e-5,
                                                                                          [True, True, True]))
        for k, nbytes in (("fwd", 12), ("torch_fwd", 12), ("grad", 20), ("torch_grad", 20)):
            row[k + "_tbytes_per_s"] = round(nbytes * elems / row[k + "_us"] / 1e6, 3)
        emit(row)
        del x, gy, xbuf, gbuf, gsrc, ybuf, ws, y_t, gmask

    if not a.no_step:
        import hourglass_train_restate as htr
        torch.manual_seed(0)
        m = htr.seed_model(hourglass.hg(**TOPO), 0).to(dev).train()
        opt = torch.optim.SGD(m.parameters(), lr=1e-5, momentum=0.9)
        n = a.batch
        x = torch.rand(n, 3, 384, 384, device=dev) - 0.5
        heat, paf = torch.rand(n, 19, 96, 96, device=dev), torch.rand(n, 38, 96, 96, device=dev) - 0.5
        ms, loss = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf)
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        emit({"what": "train_step", "model": "hg(8, 1, 38, 19)", "shape": "%dx3x384x384, SGD momentum" % n, "first_ms": ms[0],
              "steady_ms": ms[1:], "img_per_s": round(n / (min(ms[1:]) / 1e3), 1), "loss": float(loss.item()),
              "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
