"""The bf16 weight gradient and a mixed-precision training step on one MI355X: JSON lines.

    timeout -k 10 900 python tools/bench_conv_backward_bf16.py [--steps layers,vgg,openpose] [--iters 200] [--warmup 10] [--out FILE]

  layers    six layers at batch 32 - 3x3 512 -> 512 and 128 -> 128, 7x7 128 -> 128 and 185 -> 128, 1x1 128 -> 512 at 46 x 46,
            3x3 64 -> 64 at 368 x 368 - median of `iters` launches, timed one by one with device events, of
              wgrad_bf16   rtpose_conv2d_wgrad_bf16 (both launches, with dbias) on bf16 layout buffers
              wgrad_f32    rtpose_conv2d_wgrad on fp32 layout buffers of the same values
              torch_f32 / torch_bf16   torch.ops.aten.convolution_backward asked for the weight and bias gradient, NCHW
            with TFLOP/s, the share of the 2.5 PFLOP/s dense bf16 peak, and the difference from torch's fp32 gradient
  vgg       one train.train_step of rtpose_vgg at 32 x 368 x 368 with the trunk frozen (SGD with momentum), compute_dtype
            'fp32' then 'bf16': wall clock of the first and of two more steps, peak memory, train.bf16_fallbacks
  openpose  the same for OpenPose_Model(4, 2, 52, 26)

Nothing here is a pass criterion and no speed is promised: the lines say where another path is faster as well.  By hand only:
not a test, not read by bench.py.  --out appends the lines to a file as well.
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

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
N = 32
PEAK_BF16_TFLOPS = 2500.0
LAYERS = [(512, 512, 3, 46), (128, 128, 3, 46), (128, 128, 7, 46), (185, 128, 7, 46), (128, 512, 1, 46), (64, 64, 3, 368)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="layers,vgg,openpose")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = a.steps.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_backward_bf16 needs an MI355X")
    dev = torch.device("cuda", 0)
    pkg = importlib.import_module(PKG)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    synth = importlib.import_module(PKG + ".synth")
    lib = capi.lib
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

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

    for cin, cout, k, hw in (LAYERS if "layers" in steps else []):
        g = torch.Generator(device=dev).manual_seed(cin * 1000 + cout + k)
        # bf16 values, so that every path sees the same numbers
        x = torch.relu(torch.randn(N, cin, hw, hw, device=dev, generator=g)).bfloat16().float()
        gy = torch.randn(N, cout, hw, hw, device=dev, generator=g).bfloat16().float()
        wt = torch.randn(cout, cin, k, k, device=dev, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        stream = capi.current_stream()
        x16, lx16 = train._to_layout(x, k // 2, True)
        g16, lg16 = train._to_layout(gy, k // 2, True)
        dw, db = torch.empty_like(wt), torch.empty(cout, device=dev)
        floats = lib.rtpose_conv2d_wgrad_bf16_workspace_floats(cin, cout, k, N, hw, hw)
        ws = torch.empty(floats, device=dev)
        d16 = capi.WgradBf16Desc()
        d16.x, d16.gy, d16.dw, d16.dbias, d16.workspace = x16.data_ptr(), g16.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr()
        d16.workspace_floats, d16.lx, d16.lgy, d16.cin, d16.cout, d16.k = floats, lx16, lg16, cin, cout, k

        def wgrad_bf16():
            capi.check(lib.rtpose_conv2d_wgrad_bf16(C.byref(d16), N, hw, hw, stream), "rtpose_conv2d_wgrad_bf16")

        flops = 2.0 * N * hw * hw * cin * cout * k * k
        row = {"what": "layer", "cin": cin, "cout": cout, "k": k, "shape": "%dx%dx%d" % (N, hw, hw), "iters": a.iters,
               "slabs": lib.rtpose_conv2d_wgrad_bf16_slabs(cin, cout, k, N, hw, hw), "gflop": round(flops / 1e9, 2)}
        row["wgrad_bf16_us"] = median_us(wgrad_bf16)
        wgrad_bf16()
        mine = dw.clone()
        del x16, g16

        xbuf, lx = train._to_layout(x, k // 2)
        gbuf, lg = train._to_layout(gy, k // 2)
        floats32 = lib.rtpose_conv2d_wgrad_workspace_floats(cin, cout, k, N, hw, hw)
        ws32 = torch.empty(floats32, device=dev)
        d32 = capi.WgradDesc()
        d32.x, d32.gy, d32.dw, d32.dbias, d32.workspace = xbuf.data_ptr(), gbuf.data_ptr(), dw.data_ptr(), db.data_ptr(), ws32.data_ptr()
        d32.workspace_floats, d32.lx, d32.lgy, d32.cin, d32.cout, d32.k = floats32, lx, lg, cin, cout, k

        def wgrad_f32():
            capi.check(lib.rtpose_conv2d_wgrad(C.byref(d32), N, hw, hw, stream), "rtpose_conv2d_wgrad")

        row["wgrad_f32_us"] = median_us(wgrad_f32)
        del xbuf, gbuf, ws32

        def aten(gy_, x_, w_):
            return lambda: torch.ops.aten.convolution_backward(gy_, x_, w_, [cout], [1, 1], [k // 2, k // 2], [1, 1], False,
                                                               [0, 0], 1, [False, True, True])
        row["torch_f32_us"] = median_us(aten(gy, x, wt))
        ref = aten(gy, x, wt)()[1]
        xh, gh, wh = x.bfloat16(), gy.bfloat16(), wt.bfloat16()
        row["torch_bf16_us"] = median_us(aten(gh, xh, wh))
        for name in ("wgrad_bf16", "wgrad_f32", "torch_f32", "torch_bf16"):
            row[name + "_tflops"] = round(flops / row[name + "_us"] / 1e6, 1)
        row["wgrad_bf16_share_of_bf16_peak"] = round(row["wgrad_bf16_tflops"] / PEAK_BF16_TFLOPS, 3)
        row["wgrad_bf16_vs_torch_f32_max_rel"] = float(((mine - ref).abs().max() / ref.abs().max()).item())
        emit(row)
        del x, gy, ws, ref, xh, gh, wh

    def step(kind):
        if kind == "vgg":
            base = pkg.get_model('vgg19')
            base.load_state_dict(synth.he_init_state_dict(base, seed=0))
            heat_c, paf_c = 19, 38
        else:
            openpose = importlib.import_module(PKG + ".openpose")
            torch.manual_seed(0)
            base = openpose.OpenPose_Model(4, 2, 52, 26)
            heat_c, paf_c = 26, 52
        x = torch.rand(N, 3, 368, 368, device=dev) - 0.5
        heat, paf = torch.rand(N, heat_c, 46, 46, device=dev), torch.rand(N, paf_c, 46, 46, device=dev) - 0.5
        state = {n: t.clone() for n, t in base.state_dict().items()}
        for dt in train.COMPUTE_DTYPES:
            base.load_state_dict(state)
            m = train.freeze_trunk(base.to(dev))
            opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            train.reset_bf16_fallbacks()
            ms, loss = [], None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss, _ = train.train_step(m, opt, x, heat, paf, compute_dtype=dt)
                torch.cuda.synchronize()
                ms.append(round((time.perf_counter() - t0) * 1e3, 1))
            emit({"what": "train_step", "model": kind, "compute_dtype": dt,
                  "shape": "%dx3x368x368, trunk frozen, SGD momentum" % N, "first_ms": ms[0], "steady_ms": ms[1:],
                  "img_per_s": round(N / (min(ms[1:]) / 1e3), 1), "loss": float(loss.item()),
                  "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                  "bf16_fallbacks_over_3_steps": dict(train.bf16_fallbacks)})
            train.drop_packed_filters()

    for kind in ("vgg", "openpose"):
        if kind in steps:
            step(kind)


if __name__ == "__main__":
    main()
