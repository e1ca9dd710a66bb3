"""Layout-resident training against the per-conv path on one MI355X: JSON lines.

    timeout -k 10 900 python tools/bench_train_resident.py [--steps step,relu] [--dtypes fp32,bf16] [--rounds 3] [--iters 20]
                                                           [--warmup 3] [--batch 32] [--out FILE]
    timeout -k 10 300 python tools/bench_train_resident.py --steps trace --form per_conv|resident [--iters 5]

  step    train.train_step of rtpose_vgg at batch x 3 x 368 x 368, trunk frozen, SGD with momentum, for every compute dtype
          with resident=False and resident=True: the two forms ALTERNATE `rounds` times in one process, each on a model and an
          optimizer of its own from the same initial state; per round the median wall clock of `iters` steps after `warmup`
          ones, per form the peak memory, train.bf16_fallbacks and train.chain_fallbacks over everything it ran, and the loss
          after its last step
  relu    rtpose_relu_grad_bf16 alone, in place on a gapped bf16 gradient buffer against a gapped bf16 y at 32 x 46 x 46 x 128,
          next to rtpose_relu_grad on fp32 buffers of the same shape: median of 200 launches by device events, and the
          bytes/s each moves (two reads and one write per element)
  trace   `iters` bf16 steps of ONE form after one warm-up step and nothing else: the program to put behind
          `rocprofv3 --kernel-trace --stats --`, in a run of its own, for the conversion kernels' share of a step

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="step,relu")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--form", default="resident", choices=("per_conv", "resident"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    steps = a.steps.split(",")
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_resident needs an MI355X")
    dev = torch.device("cuda", 0)
    pkg = importlib.import_module(PKG)
    capi = importlib.import_module(PKG + "._capi")
    train = importlib.import_module(PKG + ".train")
    synth = importlib.import_module(PKG + ".synth")
    lib = capi.lib
    N = a.batch

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")

    def fresh_model():
        base = pkg.get_model('vgg19')
        base.load_state_dict(synth.he_init_state_dict(base, seed=0))
        m = train.freeze_trunk(base.to(dev))
        return m, torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)

    def batch():
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.rand(N, 3, 368, 368, device=dev, generator=g) - 0.5
        return x, torch.rand(N, 19, 46, 46, device=dev, generator=g), torch.rand(N, 38, 46, 46, device=dev, generator=g) - 0.5

    def run_steps(m, opt, x, heat, paf, dt, resident, count):
        ms, loss = [], None
        for _ in range(count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf, compute_dtype=dt, resident=resident)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, float(loss.item())

    if "step" in steps:
        x, heat, paf = batch()
        for dt in a.dtypes.split(","):
            forms = {}
            for name in ("per_conv", "resident"):
                m, opt = fresh_model()
                forms[name] = {"m": m, "opt": opt, "medians": [], "peak": 0, "bf16": {'fwd': 0, 'dgrad': 0}, "chain": 0,
                               "first_ms": None, "loss": None}
            for r in range(a.rounds):
                for name, f in forms.items():
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    train.reset_bf16_fallbacks()
                    train.reset_chain_fallbacks()
                    warm, _ = run_steps(f["m"], f["opt"], x, heat, paf, dt, name == "resident", a.warmup)
                    ms, f["loss"] = run_steps(f["m"], f["opt"], x, heat, paf, dt, name == "resident", a.iters)
                    if f["first_ms"] is None:
                        f["first_ms"] = round(warm[0], 1)
                    f["medians"].append(round(statistics.median(ms), 2))
                    f["peak"] = max(f["peak"], torch.cuda.max_memory_allocated())
                    for k in f["bf16"]:
                        f["bf16"][k] += train.bf16_fallbacks[k]
                    f["chain"] += train.chain_fallbacks
            for name, f in forms.items():
                emit({"what": "train_step", "model": "rtpose_vgg", "compute_dtype": dt, "form": name,
                      "shape": "%dx3x368x368, trunk frozen, SGD momentum" % N, "first_ms": f["first_ms"],
                      "median_ms_per_round": f["medians"], "steps_per_round": a.iters, "warmup_per_round": a.warmup,
                      "img_per_s": round(N / (min(f["medians"]) / 1e3), 1),
                      "peak_memory_gb": round(f["peak"] / 2 ** 30, 2), "loss_after_last_step": f["loss"],
                      "bf16_fallbacks": f["bf16"], "chain_fallbacks": f["chain"]})
            del forms
            train.drop_packed_filters()
            torch.cuda.empty_cache()

    if "relu" in steps:
        n, hw, ch, iters = 32, 46, 128, 200

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
            return statistics.median(us)

        ly, lg = capi.Layout.padded(ch, hw, hw, 1), capi.Layout.padded(ch, hw, hw, 3)
        elems = n * hw * hw * ch
        row = {"what": "relu_grad", "shape": "%dx%dx%dx%d, y gapped by 1, gy by 3, in place" % (n, hw, hw, ch), "iters": iters}
        stream = capi.current_stream()
        for name, dtype, size, fn in (("relu_grad_bf16", torch.bfloat16, 2, lib.rtpose_relu_grad_bf16),
                                      ("relu_grad_f32", torch.float32, 4, lib.rtpose_relu_grad)):
            numel = lambda lay: lib.rtpose_layout_pixels(C.byref(lay), n, hw, hw) * lay.cstride      # noqa: E731
            y = torch.randn(numel(ly), device=dev).to(dtype)
            gy = torch.randn(numel(lg), device=dev).to(dtype)

            def launch():
                capi.check(fn(capi.ptr(y), C.byref(ly), capi.ptr(gy), C.byref(lg), capi.ptr(gy), C.byref(lg), ch, n, hw, hw,
                              stream), name)
            us = median_us(launch)
            row[name + "_us"] = round(us, 1)
            row[name + "_mbytes"] = round(3 * size * elems / 1e6, 1)
            row[name + "_tbytes_per_s"] = round(3 * size * elems / us / 1e6, 2)
            del y, gy
        emit(row)

    if "trace" in steps:
        x, heat, paf = batch()
        m, opt = fresh_model()
        train.reset_bf16_fallbacks()
        train.reset_chain_fallbacks()
        run_steps(m, opt, x, heat, paf, 'bf16', a.form == "resident", 1)
        ms, loss = run_steps(m, opt, x, heat, paf, 'bf16', a.form == "resident", a.iters)
        emit({"what": "trace", "form": a.form, "compute_dtype": "bf16", "steps_after_one_warmup": a.iters,
              "ms": [round(v, 1) for v in ms], "loss": loss, "bf16_fallbacks": dict(train.bf16_fallbacks),
              "chain_fallbacks": train.chain_fallbacks})


if __name__ == "__main__":
    main()
