"""Layout-resident bf16 Bottlenecks of a HourglassNet against the default fp32 path on one MI355X: JSON lines.

    timeout -k 10 900 python tools/bench_train_bottleneck.py [--steps step,kernels] [--rounds 3] [--iters 20] [--warmup 3]
                                                             [--batch 32] [--out FILE]
    timeout -k 10 300 python tools/bench_train_bottleneck.py --steps trace --form fp32|bottleneck [--iters 3]

  step     train.train_step of hg(8, 1, 38, 19) at batch x 3 x 384 x 384, SGD with momentum, in the default form
           (compute_dtype='fp32', resident=False) and with compute_dtype='bf16', resident='bottleneck': the two forms ALTERNATE
           `rounds` times in one process, each on a model and an optimizer of its own from the same initial state, the
           allocator's cache emptied in between; per round the median wall clock of `iters` steps after `warmup` ones, per form
           the peak memory, every fallback counter over everything it ran, and the loss after its last step
  kernels  rtpose_bn_apply_bf16(relu = 1) and rtpose_bn_grad_bf16(relu = 1, dx, dweight and dbias) alone at 32 x 96 x 96 with
           128 and 256 channels - x and gy dense fp32 buffers, the destination a bf16 buffer gapped by 1 - next to the split
           pairs they replace, rtpose_bn_apply / rtpose_bn_grad followed by rtpose_layout_f32_to_bf16, next to rtpose_bn_stats,
           and next to torch's ops on NCHW fp32 tensors: relu(F.batch_norm(training)) - which includes the statistics - and
           its autograd backward; median of 200 launches by device events
  trace    `iters` steps of ONE form after one warm-up step and nothing else: the program to put behind
           `rocprofv3 --kernel-trace --stats --`, in a run of its own

The yardstick is the default path in the same process.  Nothing here is a pass criterion and no speed is promised.  By hand
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
TOPO = dict(num_stacks=8, num_blocks=1, paf_classes=38, ht_classes=19)
SIDE = 384
CHANNELS = (128, 256)
KERNEL_HW = 96
FORMS = {"fp32": dict(compute_dtype='fp32', resident=False), "bottleneck": dict(compute_dtype='bf16', resident='bottleneck')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="step,kernels")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--form", default="bottleneck", choices=tuple(FORMS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = a.steps.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_bottleneck needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    hourglass = importlib.import_module(PKG + ".hourglass")
    lib = capi.lib
    N = a.batch

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def fresh_model():
        torch.manual_seed(0)
        m = hourglass.hg(**TOPO)
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():      # He-scaled filters; the convs that write onto the residual trunk damped
            for name, mod in m.named_modules():
                if isinstance(mod, nn.Conv2d):
                    co, ci, k = mod.weight.shape[:3]
                    gain = 0.25 if name.rsplit(".", 1)[-1] == "conv3" or "_" in name.split(".")[0] else 2.0
                    mod.weight.copy_(torch.randn(co, ci, k, k, generator=g) * (gain / (ci * k * k)) ** 0.5)
                    mod.bias.copy_(torch.randn(co, generator=g) * 0.05)
        m = m.to(dev).train()
        # (the loss is a sum over every map of every stack, of the order of 1e6: a step size at which all steps stay finite)
        return m, torch.optim.SGD(m.parameters(), lr=1e-9, momentum=0.9)

    def batch():
        g = torch.Generator(device=dev).manual_seed(0)
        hw = SIDE // 4
        x = torch.rand(N, 3, SIDE, SIDE, device=dev, generator=g) - 0.5
        return (x, torch.rand(N, TOPO["ht_classes"], hw, hw, device=dev, generator=g),
                torch.rand(N, TOPO["paf_classes"], hw, hw, device=dev, generator=g) - 0.5)

    def reset():
        train.reset_bf16_fallbacks()
        train.reset_chain_fallbacks()
        train.reset_dense_fallbacks()
        train.reset_preact_fallbacks()

    def counters():
        return dict(train.bf16_fallbacks, chain=train.chain_fallbacks, dense=train.dense_fallbacks, preact=train.preact_fallbacks)

    def run_steps(m, opt, x, heat, paf, form, count):
        ms, loss = [], None
        for _ in range(count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf, **FORMS[form])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, float(loss.item())

    if "step" in steps:
        x, heat, paf = batch()
        forms = {}
        for name in FORMS:
            m, opt = fresh_model()
            forms[name] = {"m": m, "opt": opt, "medians": [], "peak": 0, "counters": {}, "first_ms": None, "loss": None}
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
                for k, v in counters().items():
                    f["counters"][k] = f["counters"].get(k, 0) + v
        for name, f in forms.items():
            emit({"what": "train_step", "model": "hg(8, 1, 38, 19)", "form": name, **{k: str(v) for k, v in FORMS[name].items()},
                  "shape": "%dx3x%dx%d, SGD momentum" % (N, SIDE, SIDE), "first_ms": f["first_ms"],
                  "median_ms_per_round": f["medians"], "steps_per_round": a.iters, "warmup_per_round": a.warmup,
                  "img_per_s": round(N / (min(f["medians"]) / 1e3), 1), "peak_memory_gb": round(f["peak"] / 2 ** 30, 2),
                  "loss_after_last_step": f["loss"], "fallbacks": f["counters"]})
        del forms
        train.drop_packed_filters()
        torch.cuda.empty_cache()

    if "kernels" in steps:
        n, hw, iters = 32, KERNEL_HW, 200

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
        p = capi.ptr
        for ch in CHANNELS:
            numel = lambda lay: lib.rtpose_layout_pixels(C.byref(lay), n, hw, hw) * lay.cstride      # noqa: E731
            lx = capi.Layout.dense(ch, hw, hw)                    # a conv's fp32 pre-activation, and the fp32 data gradient
            l16 = capi.Layout.padded(ch, hw, hw, 1)               # the bf16 buffer a 3x3 conv reads
            g = torch.Generator(device=dev).manual_seed(ch)
            x = torch.randn(numel(lx), device=dev, generator=g)
            gy = torch.randn(numel(lx), device=dev, generator=g)
            y32, d32 = torch.empty_like(x), torch.empty_like(x)
            y16 = torch.zeros(numel(l16), device=dev, dtype=torch.bfloat16)
            weight, bias = torch.rand(ch, device=dev, generator=g) + 0.5, torch.randn(ch, device=dev, generator=g) * 0.1
            rm, rv = torch.zeros(ch, device=dev), torch.ones(ch, device=dev)
            save = torch.empty(capi.BN_SAVE_ROWS * ch, device=dev)
            doubles = lib.rtpose_bn_workspace_doubles(ch, n, hw, hw)
            ws = torch.empty(doubles, device=dev, dtype=torch.float64)
            dw, db = torch.empty(ch, device=dev), torch.empty(ch, device=dev)

            def stats():
                capi.check(lib.rtpose_bn_stats(p(x), C.byref(lx), p(weight), p(bias), p(rm), p(rv), 0.1, 1e-5, p(save), p(ws), doubles,
                                               ch, n, hw, hw, stream), "rtpose_bn_stats")

            def apply16():
                capi.check(lib.rtpose_bn_apply_bf16(p(x), C.byref(lx), p(save), p(y16), C.byref(l16), 1, ch, n, hw, hw, stream),
                           "rtpose_bn_apply_bf16")

            def round_(src):
                capi.check(lib.rtpose_layout_f32_to_bf16(p(src), C.byref(lx), p(y16), C.byref(l16), ch, ch, n, hw, hw, stream),
                           "rtpose_layout_f32_to_bf16")

            def apply32():
                capi.check(lib.rtpose_bn_apply(p(x), C.byref(lx), p(save), p(y32), C.byref(lx), 1, ch, n, hw, hw, stream), "rtpose_bn_apply")
                round_(y32)

            def grad16():
                capi.check(lib.rtpose_bn_grad_bf16(p(x), C.byref(lx), p(gy), C.byref(lx), p(save), p(weight), 1, p(y16), C.byref(l16),
                                                   p(dw), p(db), p(ws), doubles, ch, n, hw, hw, stream), "rtpose_bn_grad_bf16")

            def grad32():
                capi.check(lib.rtpose_bn_grad(p(x), C.byref(lx), p(gy), C.byref(lx), p(save), p(weight), 1, p(d32), C.byref(lx),
                                              p(dw), p(db), p(ws), doubles, ch, n, hw, hw, stream), "rtpose_bn_grad")
                round_(d32)

            stats()
            xt = torch.randn(n, ch, hw, hw, device=dev, generator=g).requires_grad_(True)
            gt = torch.randn(n, ch, hw, hw, device=dev, generator=g)
            wt, bt = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)

            def torch_fwd():
                return F.relu(F.batch_norm(xt, rm, rv, wt, bt, True, 0.1, 1e-5))

            yt = torch_fwd()

            def torch_bwd():
                torch.autograd.grad(yt, (xt, wt, bt), gt, retain_graph=True)

            elems = n * hw * hw * ch
            row = {"what": "bn_bf16", "channels": ch, "shape": "%dx%dx%d" % (n, hw, hw), "iters": iters,
                   "slabs": lib.rtpose_bn_slabs(ch, n, hw, hw), "bn_stats_us": median_us(stats),
                   "bn_apply_bf16_us": median_us(apply16), "bn_apply_then_round_us": median_us(apply32),
                   "bn_grad_bf16_us": median_us(grad16), "bn_grad_then_round_us": median_us(grad32),
                   "torch_bn_relu_forward_with_statistics_us": median_us(lambda: torch_fwd()),
                   "torch_bn_relu_backward_us": median_us(torch_bwd)}
            row["bn_apply_bf16_tbytes_per_s"] = round(6 * elems / row["bn_apply_bf16_us"] / 1e6, 2)
            row["bn_grad_bf16_tbytes_per_s"] = round(18 * elems / row["bn_grad_bf16_us"] / 1e6, 2)   # x, gy twice; dx once
            emit(row)
            del x, gy, y32, d32, y16, ws, xt, gt, yt

    if "trace" in steps:
        x, heat, paf = batch()
        m, opt = fresh_model()
        reset()
        run_steps(m, opt, x, heat, paf, a.form, 1)
        ms, loss = run_steps(m, opt, x, heat, paf, a.form, a.iters)
        emit({"what": "trace", "form": a.form, "steps_after_one_warmup": a.iters, "ms": [round(v, 1) for v in ms], "loss": loss,
              "fallbacks": counters()})


if __name__ == "__main__":
    main()
