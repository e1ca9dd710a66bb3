"""Layout-resident bf16 branches of a shufflenet.Network against the default fp32 path on one MI355X: JSON lines.

    timeout -k 10 600 python tools/bench_train_branch.py [--steps step,kernels] [--rounds 3] [--iters 20] [--warmup 3]
                                                         [--batch 32] [--out FILE]
    timeout -k 10 300 python tools/bench_train_branch.py --steps trace --form fp32|branch [--iters 3]

  step     train.train_step of shufflenet.Network(1.0) at batch x 3 x 368 x 368, SGD with momentum, in the default form
           (compute_dtype='fp32', resident=False) and with compute_dtype='bf16', resident='branch': the two forms ALTERNATE
           `rounds` times in one process, each on a model and an optimizer of its own from the same initial state, the
           allocator's cache emptied in between; per round the median wall clock of `iters` steps after `warmup` ones, per form
           the peak memory, every fallback counter over everything it ran, and the loss after its last step
  kernels  rtpose_dwconv3x3_bf16_f32, rtpose_dwconv3x3_wgrad_bf16 (both launches) and rtpose_dwconv3x3_dgrad_bf16 alone next
           to their fp32 forms at the network's own depthwise shapes at this batch (C, H = W and stride of every distinct
           depthwise layer, read off the module tree), in the layouts train.unit_chain and train.dwconv3x3 give them; the two
           forms of a kernel ALTERNATE, median of 200 launches each by device events, with the bytes/s each achieves over the
           bytes it must move (every input element once, every output element once)
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
SIDE = 368
FORMS = {"fp32": dict(compute_dtype='fp32', resident=False), "branch": dict(compute_dtype='bf16', resident='branch')}


def up(c, m):
    return (c + m - 1) // m * m


def depthwise_shapes(model, side):
    """[(C, H, stride)] of every distinct depthwise layer, in the order of the forward: the stem and the pool halve the
    side (the pool in ceil mode), a stage's first block halves it again"""
    size = (side - 1) // 2 + 1
    size = (size - 3 + 1) // 2 + 1
    out = []
    net = model.network
    for stage in (net[3], net[4], net[5]):
        for blk in stage:
            convs = ([blk.conv0[0][0]] if hasattr(blk, 'conv0') else []) + [blk.conv[1][0]]
            for m in convs:
                s = (m.in_channels, size, m.stride[0])
                if s not in out:
                    out.append(s)
            size = (size - 1) // blk.conv[1][0].stride[0] + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="step,kernels")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--form", default="branch", choices=tuple(FORMS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = a.steps.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_branch needs an MI355X")
    dev = torch.device("cuda", 0)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    shufflenet = importlib.import_module(PKG + ".shufflenet")
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
        m = shufflenet.Network(1.0)
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():      # He-scaled filters, BatchNorm weights around 1: activations of unit scale at every depth
            for mod in m.modules():
                if isinstance(mod, nn.Conv2d):
                    co, ci, k = mod.weight.shape[:3]
                    mod.weight.copy_(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
                    if mod.bias is not None:
                        mod.bias.copy_(torch.randn(co, generator=g) * 0.05)
                elif isinstance(mod, nn.BatchNorm2d):
                    mod.weight.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
        m = m.to(dev).train()
        return m, torch.optim.SGD(m.parameters(), lr=1e-6, momentum=0.9)

    def batch():
        g = torch.Generator(device=dev).manual_seed(0)
        hw = (((SIDE - 1) // 2 + 1 - 3 + 1) // 2 + 1 - 1) // 2 + 1
        x = torch.rand(N, 3, SIDE, SIDE, device=dev, generator=g) - 0.5
        return (x, torch.rand(N, 19, hw, hw, device=dev, generator=g), torch.rand(N, 38, hw, hw, device=dev, generator=g) - 0.5)

    def reset():
        train.reset_bf16_fallbacks()
        train.reset_chain_fallbacks()
        train.reset_dense_fallbacks()
        train.reset_preact_fallbacks()
        train.reset_unit_fallbacks()

    def counters():
        return dict(train.bf16_fallbacks, chain=train.chain_fallbacks, dense=train.dense_fallbacks, preact=train.preact_fallbacks,
                    unit=train.unit_fallbacks)

    def run_steps(m, opt, x, heat, paf, form, count):
        ms, loss = [], None
        for _ in range(count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf, **FORMS[form])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, float(loss.item())

    if "trace" in steps:
        x, heat, paf = batch()
        m, opt = fresh_model()
        run_steps(m, opt, x, heat, paf, a.form, 1)
        ms, loss = run_steps(m, opt, x, heat, paf, a.form, a.iters)
        emit({"what": "trace", "form": a.form, "steps": a.iters, "ms": [round(v, 1) for v in ms], "loss": loss})
        return

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
            emit({"what": "train_step", "model": "shufflenet.Network(1.0)", "form": name, **{k: str(v) for k, v in FORMS[name].items()},
                  "shape": "%dx3x%dx%d, SGD momentum" % (N, SIDE, SIDE), "first_ms": f["first_ms"],
                  "median_ms_per_round": f["medians"], "steps_per_round": a.iters, "warmup_per_round": a.warmup,
                  "img_per_s": round(N / (min(f["medians"]) / 1e3), 1), "peak_memory_gb": round(f["peak"] / 2 ** 30, 2),
                  "loss_after_last_step": f["loss"], "fallbacks": f["counters"]})
        del forms
        train.drop_packed_filters()
        torch.cuda.empty_cache()

    if "kernels" in steps:
        iters = 200
        stream = capi.current_stream()
        p = capi.ptr

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3

        def alternate(fa, fb):
            """(median us of fa, of fb) over `iters` launches of each, one after the other"""
            for _ in range(10):
                fa(), fb()
            ua, ub = [], []
            for _ in range(iters):
                ua.append(timed(fa)), ub.append(timed(fb))
            return round(statistics.median(ua), 1), round(statistics.median(ub), 1)

        for ch, size, stride in depthwise_shapes(shufflenet.Network(1.0), SIDE):
            h = w = size
            ho = wo = (size - 1) // stride + 1
            cp, c16 = up(ch, 8), up(ch, 16)
            numel = lambda lay, hh, ww: lib.rtpose_layout_pixels(C.byref(lay), N, hh, ww) * lay.cstride      # noqa: E731
            g = torch.Generator(device=dev).manual_seed(ch + size)
            lx32, lx16 = capi.Layout.padded(cp, h, w, 1), capi.Layout.padded(c16, h, w, 1)
            lg32, lg16 = capi.Layout.padded(cp, ho, wo, 1), capi.Layout.padded(c16, ho, wo, 1)
            ly, ld = capi.Layout.dense(cp, ho, wo), capi.Layout.dense(cp, h, w)
            # (values everywhere, the gaps included: the timings do not depend on them)
            x32 = torch.randn(numel(lx32, h, w), device=dev, generator=g)
            g32 = torch.randn(numel(lg32, ho, wo), device=dev, generator=g)
            x16 = torch.randn(numel(lx16, h, w), device=dev, generator=g).to(torch.bfloat16)
            g16 = torch.randn(numel(lg16, ho, wo), device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(numel(ly, ho, wo), device=dev)
            d = torch.empty(numel(ld, h, w), device=dev)
            taps, zero = torch.randn(9 * cp, device=dev, generator=g), torch.zeros(cp, device=dev)
            dw = torch.empty(ch * 9, device=dev)
            doubles = lib.rtpose_dwconv3x3_wgrad_workspace_doubles(ch, N, h, w, stride)
            ws = torch.empty(doubles, device=dev, dtype=torch.float64)

            def call(name, *args):
                return lambda: capi.check(getattr(lib, name)(*args, stream), name)

            pairs = {
                "forward": (call("rtpose_dwconv3x3", p(x32), C.byref(lx32), p(taps), p(zero), p(y), C.byref(ly), cp, N, h, w, stride),
                            call("rtpose_dwconv3x3_bf16_f32", p(x16), C.byref(lx16), p(taps), p(zero), p(y), C.byref(ly), cp, N, h, w,
                                 stride),
                            (N * h * w * cp * 4 + N * ho * wo * cp * 4, N * h * w * cp * 2 + N * ho * wo * cp * 4)),
                "wgrad": (call("rtpose_dwconv3x3_wgrad", p(x32), C.byref(lx32), p(g32), C.byref(lg32), p(dw), None, p(ws), doubles, ch, N,
                               h, w, stride),
                          call("rtpose_dwconv3x3_wgrad_bf16", p(x16), C.byref(lx16), p(g16), C.byref(lg16), p(dw), None, p(ws), doubles,
                               ch, N, h, w, stride),
                          ((N * h * w + N * ho * wo) * ch * 4, (N * h * w + N * ho * wo) * ch * 2)),
                "dgrad": (call("rtpose_dwconv3x3_dgrad", p(g32), C.byref(lg32), p(taps), p(d), C.byref(ld), cp, N, h, w, stride),
                          call("rtpose_dwconv3x3_dgrad_bf16", p(g16), C.byref(lg16), p(taps), p(d), C.byref(ld), cp, N, h, w, stride),
                          (N * ho * wo * cp * 4 + N * h * w * cp * 4, N * ho * wo * cp * 2 + N * h * w * cp * 4)),
            }
            for what, (f32, f16, (b32, b16)) in pairs.items():
                us32, us16 = alternate(f32, f16)
                emit({"what": "kernel", "kernel": what, "C": ch, "H": h, "W": w, "stride": stride, "batch": N,
                      "fp32_us": us32, "bf16_us": us16, "fp32_TB_per_s": round(b32 / us32 / 1e6, 2),
                      "bf16_TB_per_s": round(b16 / us16 / 1e6, 2), "launches_each": iters})


if __name__ == "__main__":
    main()
