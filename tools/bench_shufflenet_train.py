"""Training ShuffleNetV2 on one MI355X: the depthwise 3x3 backward passes next to torch's own, and one train_step.  JSON lines.

    timeout -k 10 900 python tools/bench_shufflenet_train.py [--iters 200] [--warmup 10] [--no-step] [--batch 32] [--out FILE]

  dwconv   the network's own depthwise shapes at batch 32 and 368 x 368: 24 and 58 channels at 92 -> 46 (stride 2), 58, 116
           and 232 channels at 46 (stride 1); median of `iters` calls, timed one by one with device events, of
             wgrad  rtpose_dwconv3x3_wgrad (two launches; x with a gap of 1, dense gy)
             dgrad  rtpose_dwconv3x3_dgrad (one launch; gy with a gap of 1, dense dx)
           each next to torch.ops.aten.convolution_backward with groups = C on NCHW tensors of the same values on the same
           device, asked for the weight gradient alone and for the data gradient alone, with the bytes/s each achieves on
           the traffic the operation needs (wgrad: read x and gy; dgrad: read gy, write dx), and the difference of the two
           weight gradients and of the two data gradients
  step     one train.train_step of shufflenet.Network(1.0) at `batch` x 368 x 368 (SGD with momentum, masks of ones): wall
           clock of the second and third step after a first one that packs and allocates, and the peak memory

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
# (channels, input size, stride)
SHAPES = ((24, 92, 2), (58, 92, 2), (58, 46, 1), (116, 46, 1), (232, 46, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shufflenet_train needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    shufflenet = importlib.import_module(PKG + ".shufflenet")
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

    n = 32
    for ch, size, stride in SHAPES:
        h = w = size
        ho = wo = (size - 1) // stride + 1
        g = torch.Generator(device=dev).manual_seed(ch + size)
        x = torch.randn(n, ch, h, w, device=dev, generator=g)
        gy = torch.randn(n, ch, ho, wo, device=dev, generator=g)
        wt = torch.randn(ch, 1, 3, 3, device=dev, generator=g) / 3
        stream = capi.current_stream()
        xbuf, lx = train._to_layout(x, 1)
        gbuf, lg = train._to_layout(gy, 1)
        gdense, lgd = train._to_layout(gy, 0)
        cp = lx.cstride
        taps, _ = train._dw_taps(wt, cp)
        ld = capi.Layout.dense(cp, h, w)
        dbuf = train._buffer(ld, n, h, w, dev, False)
        doubles = lib.rtpose_dwconv3x3_wgrad_workspace_doubles(ch, n, h, w, stride)
        ws = torch.empty(doubles, dtype=torch.float64, device=dev)
        dw = torch.empty(ch, 1, 3, 3, device=dev)

        def wgrad():
            capi.check(lib.rtpose_dwconv3x3_wgrad(capi.ptr(xbuf), C.byref(lx), capi.ptr(gdense), C.byref(lgd), capi.ptr(dw), None,
                                                  capi.ptr(ws), doubles, ch, n, h, w, stride, stream), "rtpose_dwconv3x3_wgrad")

        def dgrad():
            capi.check(lib.rtpose_dwconv3x3_dgrad(capi.ptr(gbuf), C.byref(lg), capi.ptr(taps), capi.ptr(dbuf), C.byref(ld), cp, n, h, w,
                                                  stride, stream), "rtpose_dwconv3x3_dgrad")

        def torch_bwd(mask):
            return torch.ops.aten.convolution_backward(gy, x, wt, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], ch, mask)

        in_elems, out_elems = n * ch * h * w, n * ch * ho * wo
        row = {"what": "dwconv3x3_backward", "channels": ch, "shape": "%dx%dx%d -> %dx%d" % (n, h, w, ho, wo), "stride": stride,
               "iters": a.iters, "slabs": lib.rtpose_dwconv3x3_wgrad_slabs(ch, n, h, w, stride),
               "mbytes_wgrad": round(4 * (in_elems + out_elems) / 1e6, 2), "mbytes_dgrad": round(4 * (in_elems + out_elems) / 1e6, 2)}
        wgrad()
        dgrad()
        dx_t, dw_t, _ = torch_bwd([True, True, False])
        dx = train._from_layout(dbuf, ld, n, ch, h, w)
        row["dw_vs_torch_max_rel"] = float(((dw - dw_t).abs().max() / dw_t.abs().max()).item())
        row["dx_vs_torch_max_rel"] = float(((dx - dx_t).abs().max() / dx_t.abs().max()).item())
        row["wgrad_us"] = median_us(wgrad)
        row["torch_wgrad_us"] = median_us(lambda: torch_bwd([False, True, False]))
        row["dgrad_us"] = median_us(dgrad)
        row["torch_dgrad_us"] = median_us(lambda: torch_bwd([True, False, False]))
        for k in ("wgrad", "torch_wgrad", "dgrad", "torch_dgrad"):
            row[k + "_tbytes_per_s"] = round(4 * (in_elems + out_elems) / row[k + "_us"] / 1e6, 3)
        emit(row)
        del x, gy, xbuf, gbuf, gdense, dbuf, ws, dx, dx_t

    if not a.no_step:
        import dwconv_restate as dr
        torch.manual_seed(0)
        m = dr.seed_module(shufflenet.Network(1.0), 0).to(dev).train()
        opt = torch.optim.SGD(m.parameters(), lr=1e-5, momentum=0.9)
        n = a.batch
        x = torch.rand(n, 3, 368, 368, device=dev) - 0.5
        heat, paf = torch.rand(n, 19, 46, 46, device=dev), torch.rand(n, 38, 46, 46, device=dev) - 0.5
        ms, loss = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf)
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        emit({"what": "train_step", "model": "shufflenet.Network(1.0)", "shape": "%dx3x368x368, SGD momentum" % n, "first_ms": ms[0],
              "steady_ms": ms[1:], "img_per_s": round(n / (min(ms[1:]) / 1e3), 1), "loss": float(loss.item()),
              "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
