"""Layout-resident dense stages of an OpenPose_Model against the per-conv bf16 path on one MI355X: JSON lines.

    timeout -k 10 900 python tools/bench_train_dense.py [--steps step,kernels] [--rounds 3] [--iters 20] [--warmup 3]
                                                        [--batch 32] [--out FILE]
    timeout -k 10 300 python tools/bench_train_dense.py --steps trace --form per_conv|dense [--iters 5]

  step     train.train_step of OpenPose_Model(4, 2, 52, 26) at batch x 3 x 368 x 368, compute_dtype='bf16', trunk frozen, SGD
           with momentum, with resident=False and resident='dense': the two forms ALTERNATE `rounds` times in one process, each
           on a model and an optimizer of its own from the same initial state; per round the median wall clock of `iters`
           steps after `warmup` ones, per form the peak memory, train.bf16_fallbacks / chain_fallbacks / dense_fallbacks over
           everything it ran, and the loss after its last step
  kernels  rtpose_prelu_bf16 and rtpose_prelu_grad_bf16 (two consumers, with the slope gradient) alone at 32 x 46 x 46 with
           96, 128, 256 and 512 channels - the destination a slice of a 3 C concat buffer gapped by 1, ga a slice of a dense
           3 C gradient - next to the passes they replace: rtpose_prelu, and rtpose_prelu_grad followed by
           rtpose_layout_f32_to_bf16; median of 200 launches by device events
  trace    `iters` steps of ONE form after one warm-up step and nothing else: the program to put behind
           `rocprofv3 --kernel-trace --stats --`, in a run of its own

The yardstick is the per-conv path in the same process.  Nothing here is a pass criterion and no speed is promised.  By hand
only: not a test, not read by bench.py.  --out appends the lines to a file as well.
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
TOPO = (4, 2, 52, 26)
HW = 46
CHANNELS = (96, 128, 256, 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="step,kernels")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--form", default="dense", choices=("per_conv", "dense"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = a.steps.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_dense needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    openpose = importlib.import_module(PKG + ".openpose")
    lib = capi.lib
    N = a.batch
    resident_of = {"per_conv": False, "dense": 'dense'}

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def fresh_model():
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
        return m, torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)

    def batch():
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.rand(N, 3, 368, 368, device=dev, generator=g) - 0.5
        return (x, torch.rand(N, TOPO[3], HW, HW, device=dev, generator=g),
                torch.rand(N, TOPO[2], HW, HW, device=dev, generator=g) - 0.5)

    def reset():
        train.reset_bf16_fallbacks()
        train.reset_chain_fallbacks()
        train.reset_dense_fallbacks()

    def run_steps(m, opt, x, heat, paf, form, count):
        ms, loss = [], None
        for _ in range(count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf, compute_dtype='bf16', resident=resident_of[form])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, float(loss.item())

    if "step" in steps:
        x, heat, paf = batch()
        forms = {}
        for name in ("per_conv", "dense"):
            m, opt = fresh_model()
            forms[name] = {"m": m, "opt": opt, "medians": [], "peak": 0, "bf16": {'fwd': 0, 'dgrad': 0}, "chain": 0, "dense": 0,
                           "first_ms": None, "loss": None}
        for r in range(a.rounds):
            for name, f in forms.items():
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                reset()
                warm, _ = run_steps(f["m"], f["opt"], x, heat, paf, name, a.warmup)
                ms, f["loss"] = run_steps(f["m"], f["opt"], x, heat, paf, name, a.iters)
                if f["first_ms"] is None:
                    f["first_ms"] = round(warm[0], 1)
                f["medians"].append(round(statistics.median(ms), 2))
                f["peak"] = max(f["peak"], torch.cuda.max_memory_allocated())
                for k in f["bf16"]:
                    f["bf16"][k] += train.bf16_fallbacks[k]
                f["chain"] += train.chain_fallbacks
                f["dense"] += train.dense_fallbacks
        for name, f in forms.items():
            emit({"what": "train_step", "model": "OpenPose_Model%r" % (TOPO,), "compute_dtype": "bf16", "form": name,
                  "shape": "%dx3x368x368, trunk frozen, SGD momentum" % N, "first_ms": f["first_ms"],
                  "median_ms_per_round": f["medians"], "steps_per_round": a.iters, "warmup_per_round": a.warmup,
                  "img_per_s": round(N / (min(f["medians"]) / 1e3), 1),
                  "peak_memory_gb": round(f["peak"] / 2 ** 30, 2), "loss_after_last_step": f["loss"],
                  "bf16_fallbacks": f["bf16"], "chain_fallbacks": f["chain"], "dense_fallbacks": f["dense"]})
        del forms
        train.drop_packed_filters()
        torch.cuda.empty_cache()

    if "kernels" in steps:
        n, iters = 32, 200

        def median_us(fn):
            for _ in range(10):
                fn()
            us = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            return round(statistics.median(us), 1)

        stream = capi.current_stream()
        for ch in CHANNELS:
            numel = lambda lay: lib.rtpose_layout_pixels(C.byref(lay), n, HW, HW) * lay.cstride      # noqa: E731
            lz = capi.Layout.dense(ch, HW, HW)                    # a conv's fp32 pre-activation, and the fp32 gradient D
            lcat = capi.Layout.padded(3 * ch, HW, HW, 1, ch)      # slice 1 of a block's bf16 concat buffer
            ldc = capi.Layout.dense(3 * ch, HW, HW, ch)           # slice 1 of the fp32 gradient of the concat
            lg = capi.Layout.padded(ch, HW, HW, 1)                # the bf16 gradient the 3x3 convs read
            g = torch.Generator(device=dev).manual_seed(ch)
            z = torch.randn(numel(lz), device=dev, generator=g)
            d = torch.randn(numel(lz), device=dev, generator=g)
            dc = torch.randn(numel(ldc), device=dev, generator=g)
            slope = torch.randn(ch, device=dev, generator=g) * 0.25
            ycat = torch.zeros(numel(lcat), device=dev, dtype=torch.bfloat16)
            gbf = torch.zeros(numel(lg), device=dev, dtype=torch.bfloat16)
            y32 = torch.empty_like(z)
            g32 = torch.randn(numel(lz), device=dev, generator=g)
            floats = lib.rtpose_prelu_grad_bf16_workspace_floats(ch, n, HW, HW)
            ws, ds = torch.empty(floats, device=dev), torch.empty(ch, device=dev)
            p = capi.ptr

            def fwd16():
                capi.check(lib.rtpose_prelu_bf16(p(z), C.byref(lz), p(slope), p(ycat), C.byref(lcat), ch, n, HW, HW, stream),
                           "rtpose_prelu_bf16")

            def fwd32():
                capi.check(lib.rtpose_prelu(p(z), C.byref(lz), p(slope), p(y32), C.byref(lz), ch, n, HW, HW, stream), "rtpose_prelu")

            def grad16():
                capi.check(lib.rtpose_prelu_grad_bf16(p(z), C.byref(lz), p(slope), p(dc), C.byref(ldc), p(d), C.byref(lz), p(gbf),
                                                      C.byref(lg), p(ds), p(ws), floats, ch, n, HW, HW, stream),
                           "rtpose_prelu_grad_bf16")

            def grad32():
                capi.check(lib.rtpose_prelu_grad(p(z), C.byref(lz), p(slope), p(g32), C.byref(lz), p(g32), C.byref(lz), p(ds),
                                                 p(ws), floats, ch, n, HW, HW, stream), "rtpose_prelu_grad")
                capi.check(lib.rtpose_layout_f32_to_bf16(p(g32), C.byref(lz), p(gbf), C.byref(lg), ch, ch, n, HW, HW, stream),
                           "rtpose_layout_f32_to_bf16")

            elems = n * HW * HW * ch
            row = {"what": "prelu_bf16", "channels": ch, "shape": "%dx%dx%d" % (n, HW, HW), "iters": iters,
                   "slabs": lib.rtpose_prelu_grad_bf16_slabs(ch, n, HW, HW),
                   "prelu_bf16_us": median_us(fwd16), "prelu_f32_us": median_us(fwd32),
                   "prelu_grad_bf16_us": median_us(grad16), "prelu_grad_f32_then_round_us": median_us(grad32)}
            row["prelu_bf16_tbytes_per_s"] = round(6 * elems / row["prelu_bf16_us"] / 1e6, 2)
            row["prelu_grad_bf16_tbytes_per_s"] = round(14 * elems / row["prelu_grad_bf16_us"] / 1e6, 2)
            emit(row)
            del z, d, dc, ycat, gbf, y32, g32, ws

    if "trace" in steps:
        x, heat, paf = batch()
        m, opt = fresh_model()
        reset()
        run_steps(m, opt, x, heat, paf, a.form, 1)
        ms, loss = run_steps(m, opt, x, heat, paf, a.form, a.iters)
        emit({"what": "trace", "form": a.form, "compute_dtype": "bf16", "steps_after_one_warmup": a.iters,
              "ms": [round(v, 1) for v in ms], "loss": loss, "bf16_fallbacks": dict(train.bf16_fallbacks),
              "chain_fallbacks": train.chain_fallbacks, "dense_fallbacks": train.dense_fallbacks})


if __name__ == "__main__":
    main()
