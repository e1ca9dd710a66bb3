"""OpenPose_Model (4, 2, 38, 19) fp32 on one MI355X: one JSON line.

    python tools/bench_openpose.py [N=32] [iters=20]

* images/s of forward + scene blend + decode + record D2H through PoseEstimator.submit / collect at N x 368 x 368 (two
  tickets in flight, as bench.py runs rtpose_vgg), and ms per forward alone (device events around `iters` forwards);
* per-kind launch times of one profiled forward (rtpose_net_set_profiling): trunk, stage 3x3 by (cin, cout), heads;
* algorithmic TFLOP/s at 160.7 GFLOP per 368 x 368 image, and for the stage 3x3 launches the matrix-core flops they
  issue (rtpose_net_launch_executed_flops) per second as a fraction of the 157.3 TFLOP/s fp32 MFMA peak.
Seeded weights (tests/openpose_restate.py); synthetic scenes so that the decoder has people to assemble.
"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import openpose_restate as R  # noqa: E402

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
GFLOP_PER_IMAGE = 160.7  # 80.33 GMAC at 368 x 368 (trunk 3x3 40.80, stage 3x3 37.38, stage 1x1 2.15)
PEAK_F32_MFMA_TFLOPS = 157.3


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    if not torch.cuda.is_available():
        raise SystemExit("bench_openpose needs an MI355X")
    op = importlib.import_module(PKG + ".openpose")
    pipeline = importlib.import_module(PKG + ".pipeline")
    synth = importlib.import_module(PKG + ".synth")
    capi = importlib.import_module(PKG + "._capi")
    lib = capi.lib
    dev = torch.device("cuda", 0)
    cfg = (4, 2, 38, 19)
    m = op.OpenPose_Model(*cfg)
    m.load_state_dict(R.seeded_state_dict(R.state_dict_spec(*cfg), 3))
    m = m.cuda().eval()
    S = 368
    x = (torch.rand(n, 3, S, S, generator=torch.Generator().manual_seed(0)) - 0.5).to(dev)
    h, p, _ = synth.make_batch(n, S, S, seed=1)
    scene = (torch.from_numpy(h).to(dev), torch.from_numpy(p).to(dev))
    est = pipeline.PoseEstimator(m)
    with torch.no_grad():
        est(x, scene, scene_alpha=2e-2)  # plan, weights, forms, decoder capacities
        for _ in range(3):
            m.forward_native(x)
        torch.cuda.synchronize()
        # forward alone
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            m.forward_native(x)
        e1.record()
        torch.cuda.synchronize()
        fwd_ms = e0.elapsed_time(e1) / iters
        # forward + blend + decode + record D2H, pipelined
        prev = est.submit(x, scene, scene_alpha=2e-2)
        est.collect(prev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prev = None
        for _ in range(iters):
            t = est.submit(x, scene, scene_alpha=2e-2)
            if prev is not None:
                est.collect(prev)
            prev = t
        est.collect(prev)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        # one profiled forward
        plan = m.plan_for(x)
        lib.rtpose_net_set_profiling(plan.handle, 1)
        m.forward_native(x)
        torch.cuda.synchronize()
        kinds = {}
        name = C.create_string_buffer(96)
        ms, k, fl, ex, wf = C.c_float(), C.c_int(), C.c_double(), C.c_double(), C.c_int()
        st_ex = st_ms = 0.0
        total_ms = 0.0
        ncin = {}
        for i in range(lib.rtpose_net_num_convs(plan.handle)):
            co, ci, kk = C.c_int(), C.c_int(), C.c_int()
            lib.rtpose_net_conv_info(plan.handle, i, name, 96, C.byref(co), C.byref(ci), C.byref(kk))
            ncin[name.value.decode()] = (ci.value, co.value)
        for i in range(lib.rtpose_net_num_launches(plan.handle)):
            lib.rtpose_net_launch_info(plan.handle, i, C.byref(ms), C.byref(k), C.byref(fl), name, 96)
            lib.rtpose_net_launch_executed_flops(plan.handle, i, C.byref(ex), C.byref(wf))
            nm = name.value.decode()
            total_ms += ms.value
            if nm.startswith("feature_extractor"):
                kind = "trunk"
            elif nm.endswith("Mconv6.Mconv") or nm.endswith("Mconv7"):
                kind = "head 1x1"
            elif k.value == 3:
                kind = "stage 3x3 %d->%d" % ncin[nm]
                st_ex += ex.value
                st_ms += ms.value
            else:
                kind = "other"
            kinds[kind] = kinds.get(kind, 0.0) + ms.value
        lib.rtpose_net_set_profiling(plan.handle, 0)
    print(json.dumps({
        "workload": "OpenPose_Model(4, 2, 38, 19) fp32, %d x 3 x %d x %d" % (n, S, S),
        "images_per_s_submit_collect": round(n * iters / wall, 1),
        "ms_per_forward": round(fwd_ms, 3),
        "algorithmic_tflops_forward": round(GFLOP_PER_IMAGE * n / fwd_ms, 1),
        "profiled_forward_ms": round(total_ms, 3),
        "launch_ms_by_kind": {k: round(v, 3) for k, v in sorted(kinds.items())},
        "stage3x3_issued_mfma_fraction_of_peak": round(st_ex / (st_ms * 1e9) / PEAK_F32_MFMA_TFLOPS, 3) if st_ms else None,
    }))


if __name__ == "__main__":
    main()
