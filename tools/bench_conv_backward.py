"""The conv backward pass on one MI355X next to torch's own on the same tensors: JSON lines.

    timeout -k 10 900 python tools/bench_conv_backward.py [--iters 200] [--warmup 10] [--no-step] [--out FILE]

  layer    per distinct (cin, cout, k) of rtpose_vgg - the stage convs at 32 x 46 x 46, the trunk's at their own resolutions -
           median of `iters` launches, timed one by one with device events, of
             wgrad   rtpose_conv2d_wgrad (both launches, with dbias)
             dgrad   rtpose_conv2d on the flipped, transposed filter
           each next to torch.ops.aten.convolution_backward asked for that one gradient, on the same values in NCHW
  step     one train.train_step at 32 x 368 x 368 with the trunk frozen (SGD with momentum): wall clock of the second and
           third step after a first one that packs and allocates

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

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
N = 32
# (cin, cout, k, H = W): the trunk at its own resolutions, then the stages at 46 x 46
TRUNK = [(3, 64, 3, 368), (64, 64, 3, 368), (64, 128, 3, 184), (128, 128, 3, 184), (128, 256, 3, 92), (256, 256, 3, 92),
         (256, 512, 3, 46), (512, 512, 3, 46), (512, 256, 3, 46), (256, 128, 3, 46)]
STAGES = [(128, 128, 3, 46), (128, 512, 1, 46), (512, 38, 1, 46), (512, 19, 1, 46), (185, 128, 7, 46), (128, 128, 7, 46),
          (128, 128, 1, 46), (128, 38, 1, 46), (128, 19, 1, 46)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_backward needs an MI355X")
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

    for cin, cout, k, hw in TRUNK + STAGES:
        g = torch.Generator(device=dev).manual_seed(cin * 1000 + cout + k)
        x = torch.relu(torch.randn(N, cin, hw, hw, device=dev, generator=g))
        gy = torch.randn(N, cout, hw, hw, device=dev, generator=g)
        wt = torch.randn(cout, cin, k, k, device=dev, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        stream = capi.current_stream()
        xbuf, lx = train._to_layout(x, k // 2)
        gbuf, lg = train._to_layout(gy, k // 2)
        dw, db = torch.empty_like(wt), torch.empty(cout, device=dev)
        floats = lib.rtpose_conv2d_wgrad_workspace_floats(cin, cout, k, N, hw, hw)
        ws = torch.empty(floats, device=dev)
        d = capi.WgradDesc()
        d.x, d.gy, d.dw, d.dbias, d.workspace = xbuf.data_ptr(), gbuf.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr()
        d.workspace_floats, d.lx, d.lgy, d.cin, d.cout, d.k = floats, lx, lg, cin, cout, k
        wp, bp = train._pack(train.dgrad_weights(wt), torch.zeros(cin, device=dev), lg.cstride)
        lout = capi.Layout.dense(train._up8(cin), hw, hw)
        obuf = train._buffer(lout, N, hw, hw, dev, False)
        cdesc = capi.ConvDesc()
        cdesc.inp, cdesc.w_packed, cdesc.bias_packed, cdesc.out = gbuf.data_ptr(), wp.data_ptr(), bp.data_ptr(), obuf.data_ptr()
        cdesc.lin, cdesc.lout, cdesc.cin, cdesc.cout, cdesc.k = lg, lout, lg.cstride, cin, k

        def wgrad():
            capi.check(lib.rtpose_conv2d_wgrad(C.byref(d), N, hw, hw, stream), "rtpose_conv2d_wgrad")

        def dgrad():
            capi.check(lib.rtpose_conv2d(C.byref(cdesc), 1, N, hw, hw, stream), "rtpose_conv2d")

        def aten(mask):
            return lambda: torch.ops.aten.convolution_backward(gy, x, wt, [cout], [1, 1], [k // 2, k // 2], [1, 1], False,
                                                               [0, 0], 1, mask)
        flops = 2.0 * N * hw * hw * cin * cout * k * k
        row = {"what": "layer", "cin": cin, "cout": cout, "k": k, "shape": "%dx%dx%d" % (N, hw, hw), "iters": a.iters,
               "slabs": lib.rtpose_conv2d_wgrad_slabs(cin, cout, k, N, hw, hw), "gflop": round(flops / 1e9, 2)}
        row["wgrad_us"] = median_us(wgrad)
        row["torch_wgrad_us"] = median_us(aten([False, True, True]))
        row["dgrad_us"] = median_us(dgrad)
        row["torch_dgrad_us"] = median_us(aten([True, False, False]))
        row["wgrad_tflops"] = round(flops / row["wgrad_us"] / 1e6, 2)
        row["dgrad_tflops"] = round(flops / row["dgrad_us"] / 1e6, 2)
        # the two weight gradients agree (different summation orders of fp32)
        ref = aten([False, True, True])()[1]
        wgrad()
        row["wgrad_vs_torch_max_rel"] = float(((dw - ref).abs().max() / ref.abs().max()).item())
        emit(row)
        del x, gy, xbuf, gbuf, ws, obuf, ref

    if not a.no_step:
        m = pkg.get_model('vgg19')
        m.load_state_dict(synth.he_init_state_dict(m, seed=0))
        m = train.freeze_trunk(m.to(dev))
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)
        x = torch.rand(N, 3, 368, 368, device=dev) - 0.5
        heat, paf = torch.rand(N, 19, 46, 46, device=dev), torch.rand(N, 38, 46, 46, device=dev) - 0.5
        ms, loss = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = train.train_step(m, opt, x, heat, paf)
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        emit({"what": "train_step", "shape": "%dx3x368x368, trunk frozen, SGD momentum" % N, "first_ms": ms[0],
              "steady_ms": ms[1:], "img_per_s": round(N / (min(ms[1:]) / 1e3), 1), "loss": float(loss.item()),
              "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
