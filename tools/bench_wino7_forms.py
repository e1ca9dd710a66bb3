"""Per-launch device time of the 7x7 stage convolutions in F(6,7) and F(8,7) (developer tool; bench.py keeps the contract):
the two stage geometries of the headline configuration - Mconv1_stageN (185 -> 128, packed to 192 input channels) and
Mconv2..5_stageN (128 -> 128), each as the grouped two-branch launch the executor issues, at 32 x 46 x 46 - through
rtpose_conv2d_winograd_ex with the caller's hand-over scratch (persistent blocks with split tiles, as in the network).

Both forms run in ONE process, alternating: round r times `--launches` back-to-back launches of form 6, then of form 8, between
two events on the launch stream; nothing is recorded or queried inside a timed loop.  One JSON line: per geometry and form
the median, minimum and maximum over the rounds of the mean launch time, the MFMA flops a launch issues (whole 32-position
strips, padded channels; = SQ_INSTS_MFMA x 4096) and the issued-MFMA fraction of the fp32 matrix peak at the median.

  python tools/bench_wino7_forms.py [--rounds 8] [--launches 20]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
FP32_MFMA_PEAK_TFLOPS = 157.3      # v_mfma_f32_32x32x2_f32 peak of an MI355X (the figure bench.py uses)
N, H, W = 32, 46, 46


def issued_flops(cin_packed, cout, m, groups):
    """conv2d_wino7_issued_flops restated: strips of 32 positions per image, 7 rows x (m + 6) frequencies."""
    gx = -(-W // m)
    mtiles = N * -(-(H * gx) // 32)
    return 2.0 * mtiles * 32 * 7 * (m + 6) * cin_packed * ((cout + 63) // 64 * 64) * groups


class Launch(object):
    """One grouped two-branch 7x7 launch in F(m,7): descriptors, packed filters, buffers."""

    def __init__(self, capi, dev, cin, m, seed):
        lib, Layout = capi.lib, capi.Layout
        self.lib, self.capi, self.m = lib, capi, m
        cin_p, cout = (cin + 7) // 8 * 8, 128
        g = torch.Generator().manual_seed(seed)
        stream = capi.current_stream()
        lin = Layout.padded(cin_p, H, W, 3)
        self.xin = torch.zeros(lib.rtpose_layout_pixels(C.byref(lin), N, H, W) * cin_p, device=dev)
        x = torch.rand(N, cin, H, W, generator=g).to(dev)
        capi.check(lib.rtpose_nchw_to_layout(capi.ptr(x), capi.ptr(self.xin), C.byref(lin), cin, cin_p, N, H, W, stream))
        self.descs = (capi.ConvDesc * 2)()
        self.keep = []
        for b in range(2):
            wt = (torch.randn(cout, cin, 7, 7, generator=g) * (2.0 / (cin * 49)) ** 0.5).to(dev)
            bias = (torch.randn(cout, generator=g) * 0.1).to(dev)
            wp = torch.zeros(lib.rtpose_packed_weight_floats_winograd7(cout, cin_p, m), device=dev)
            bp = torch.zeros(lib.rtpose_packed_bias_floats(cout), device=dev)
            capi.check(lib.rtpose_pack_conv_weights_winograd7(capi.ptr(wt), capi.ptr(bias), cout, cin, m, None, cin_p,
                                                              capi.ptr(wp), capi.ptr(bp), stream))
            lout = Layout.padded(cout, H, W, 3)
            out = torch.zeros(lib.rtpose_layout_pixels(C.byref(lout), N, H, W) * cout, device=dev)
            d = self.descs[b]
            d.inp, d.w_packed, d.bias_packed, d.out = self.xin.data_ptr(), wp.data_ptr(), bp.data_ptr(), out.data_ptr()
            d.lin, d.lout = lin, lout
            d.cin, d.cout, d.k, d.relu, d.pool, d.wino_m = cin_p, cout, 7, 1, 0, m
            self.keep += [wp, bp, out]
        assert lib.rtpose_conv2d_winograd_fits(self.descs, N, H, W) == 1
        self.scratch = torch.zeros(lib.rtpose_conv2d_winograd_scratch_bytes() // 4, dtype=torch.int32, device=dev)
        self.flops = issued_flops(cin_p, cout, m, 2)
        torch.cuda.synchronize()

    def run(self, count):
        stream = self.capi.current_stream()
        for _ in range(count):
            self.capi.check(self.lib.rtpose_conv2d_winograd_ex(self.descs, 2, N, H, W, self.capi.ptr(self.scratch),
                                                               self.scratch.numel() * 4, stream), "rtpose_conv2d_winograd_ex")

    def error_word(self):
        word = C.c_int(-1)
        self.capi.check(self.lib.rtpose_conv2d_winograd_scratch_error(self.capi.ptr(self.scratch), C.byref(word),
                                                                      self.capi.current_stream()))
        return word.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8, help="alternations of the two forms (>= 8)")
    ap.add_argument("--launches", type=int, default=20, help="back-to-back launches per timed loop")
    args = ap.parse_args()
    if args.rounds < 8:
        raise SystemExit("bench_wino7_forms.py: at least 8 alternations")
    if not torch.cuda.is_available():
        raise SystemExit("bench_wino7_forms.py needs an MI355X")
    capi = importlib.import_module(PKG + "._capi")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"tool": "bench_wino7_forms", "geometry": "grouped two-branch launch, %d x %d x %d, cout 128" % (N, H, W),
           "rounds": args.rounds, "launches_per_timed_loop": args.launches, "unit": "ms per launch", "layers": {}}
    for name, cin in (("185->128 (Mconv1_stageN)", 185), ("128->128 (Mconv2..5_stageN)", 128)):
        forms = {m: Launch(capi, dev, cin, m, seed=cin) for m in (6, 8)}
        times = {6: [], 8: []}
        for m in (6, 8):
            forms[m].run(3)                      # untimed: lazy statics, clocks
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for m in (6, 8):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                forms[m].run(args.launches)
                e1.record()
                e1.synchronize()
                times[m].append(e0.elapsed_time(e1) / args.launches)
        layer = {}
        for m in (6, 8):
            if forms[m].error_word():
                raise SystemExit("device error word set after the F(%d,7) launches" % m)
            med = statistics.median(times[m])
            layer["F(%d,7)" % m] = {"median": round(med, 4), "min": round(min(times[m]), 4), "max": round(max(times[m]), 4),
                                    "issued_mfma_gflop": round(forms[m].flops / 1e9, 2),
                                    "issued_mfma_fraction": round(forms[m].flops / (med * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4)}
        layer["F(8,7) / F(6,7) median time"] = round(layer["F(8,7)"]["median"] / layer["F(6,7)"]["median"], 4)
        out["layers"][name] = layer
        del forms
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
