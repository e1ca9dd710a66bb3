"""Training an OpenPose_Model on one MI355X: the PReLU passes next to torch's own, and one train_step.  JSON lines.

    timeout -k 10 900 python tools/bench_openpose_train.py [--iters 200] [--warmup 10] [--no-step] [--out FILE]

  prelu    at 32 x 46 x 46 with 96, 128, 256 and 512 channels (the widths of OpenPose_Model's PReLUs), median of `iters`
           launches, timed one by one with device events, of
             fwd    rtpose_prelu (z -> y, dense layouts)
             grad   rtpose_prelu_grad (in place on gy, with dslope: both launches)
           each next to torch.ops.aten._prelu_kernel / _prelu_kernel_backward on NCHW tensors of the same values on the same
           device, with the bytes/s each achieves on the traffic the operation needs (fwd: read z, write y; grad: read z and
           gy, write out)
  step     one train.train_step of OpenPose_Model(4, 2, 52, 26) at 32 x 368 x 368 with the trunk frozen (SGD with momentum):
           wall clock of the second and third step after a first one that packs and allocates

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
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
N, HW = 32, 46
CHANNELS = (96, 128, 256, 512)
TOPO = (4, 2, 52, 26)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_openpose_train needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    openpose = importlib.import_module(PKG + ".openpose")
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

    for ch in CHANNELS:
        g = torch.Generator(device=dev).manual_seed(ch)
        z = torch.randn(N, ch, HW, HW, device=dev, generator=g)
        gy = torch.randn(N, ch, HW, HW, device=dev, generator=g)
        slope = torch.randn(ch, device=dev, generator=g) * 0.25
        stream = capi.current_stream()
        zbuf, lz = train._to_layout(z, 0)
        gbuf, lg = train._to_layout(gy, 0)
        ybuf = torch.empty_like(zbuf)
        floats = lib.rtpose_prelu_grad_workspace_floats(ch, N, HW, HW)
        ws, ds = torch.empty(floats, device=dev), torch.empty(ch, device=dev)

        def fwd():
            capi.check(lib.rtpose_prelu(capi.ptr(zbuf), C.byref(lz), capi.ptr(slope), capi.ptr(ybuf), C.byref(lz), ch, N, HW, HW,
                                        stream), "rtpose_prelu")

        def grad():
            capi.check(lib.rtpose_prelu_grad(capi.ptr(zbuf), C.byref(lz), capi.ptr(slope), capi.ptr(gbuf), C.byref(lg),
                                             capi.ptr(gbuf), C.byref(lg), capi.ptr(ds), capi.ptr(ws), floats, ch, N, HW, HW,
                                             stream), "rtpose_prelu_grad")
        wide = slope.view(1, ch, 1, 1).expand_as(z)           # what F.prelu hands to the ATen kernels
        elems = N * ch * HW * HW
        row = {"what": "prelu", "channels": ch, "shape": "%dx%dx%d" % (N, HW, HW), "iters": a.iters,
               "slabs": lib.rtpose_prelu_grad_slabs(ch, N, HW, HW), "mbytes_fwd": round(8 * elems / 1e6, 1),
               "mbytes_grad": round(12 * elems / 1e6, 1)}
        # the slope gradient agrees with torch's (different summation orders of fp32); taken before the in-place timing loop
        zz, aa = z.clone().requires_grad_(True), slope.clone().requires_grad_(True)
        torch.nn.functional.prelu(zz, aa).backward(gy)
        grad()
        row["dslope_vs_torch_max_rel"] = float(((ds - aa.grad).abs().max() / aa.grad.abs().max()).item())
        del zz, aa
        row["fwd_us"] = median_us(fwd)
        row["torch_fwd_us"] = median_us(lambda: torch.ops.aten._prelu_kernel(z, wide))
        row["grad_us"] = median_us(grad)
        row["torch_grad_us"] = median_us(lambda: torch.ops.aten._prelu_kernel_backward(gy, z, wide))
        for k, b in (("fwd", 8), ("torch_fwd", 8), ("grad", 12), ("torch_grad", 12)):
            row[k + "_tbytes_per_s"] = round(b * elems / row[k + "_us"] / 1e6, 2)
        emit(row)
        del z, gy, zbuf, gbuf, ybuf, ws, wide

    if not a.no_step:
        torch.manual_seed(0)
        m = openpose.OpenPose_Model(*TOPO)
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, nn.Conv2d):
                    co, ci, k = mod.weight.shape[:3]
                    mod.weight.copy_(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
                    mod.bias.copy_(torch.randn(co, generator=g) * 0.1)
                elif isinstance(mod, nn.PReLU):
                    mod.weight.copy_(torch.randn(mod.weight.shape[0], generator=g) * 0.25)
        m = train.freeze_trunk(m.to(dev))
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)
        x = torch.rand(N, 3, 368, 368, device=dev) - 0.5
        heat, paf = torch.rand(N, TOPO[3], HW, HW, device=dev), torch.rand(N, TOPO[2], HW, HW, device=dev) - 0.5
        ms, loss = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf)
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        emit({"what": "train_step", "model": "OpenPose_Model%r" % (TOPO,),
              "shape": "%dx3x368x368, trunk frozen, SGD momentum" % N, "first_ms": ms[0], "steady_ms": ms[1:],
              "img_per_s": round(N / (min(ms[1:]) / 1e3), 1), "loss": float(loss.item()),
              "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
