"""hg(8, 1, 38, 19) fp32 on one MI355X: one JSON line.

    python tools/bench_hourglass.py [N=32] [iters=20] [--layers] [--torch]

* images/s of forward + scene blend + decode + record D2H through PoseEstimator.submit / collect at N x 384 x 384 (two
  tickets in flight, as bench.py runs rtpose_vgg; config with MODEL.DOWNSAMPLE = 4), and ms per forward alone (device
  events around `iters` forwards; with RTPOSE_GRAPH=1 in the environment that is the replayed launch list);
* algorithmic TFLOP/s at 129.33 GFLOP per 384 x 384 image, and the matrix-core flops the forward issues
  (rtpose_net_launch_executed_flops) per second as a fraction of the 157.3 TFLOP/s fp32 MFMA peak;
* --layers: the launch list of one profiled forward (rtpose_net_set_profiling) grouped by map size and kind;
* --torch: beside it, ms per forward of the CPU restatement (tests/hourglass_restate.py: F.conv2d, F.batch_norm, ...)
  run on the same device and batch through PyTorch-ROCm, i.e. through MIOpen - the only other implementation there is.
Seeded weights (tests/hourglass_restate.py); synthetic stride-4 scenes so that the decoder has people to assemble.
"""
import ctypes as C
import importlib
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hourglass_restate as R  # noqa: E402

PKG = "pytorch_realtime_multi-person_pose_estimation_amd"
GFLOP_PER_IMAGE = 129.33  # 64.664 GMAC at 384 x 384 (1x1 27.667, 3x3 36.649, 7x7 0.347)
PEAK_F32_MFMA_TFLOPS = 157.3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = set(a for a in sys.argv[1:] if a.startswith("--"))
    n = int(args[0]) if len(args) > 0 else 32
    iters = int(args[1]) if len(args) > 1 else 20
    if not torch.cuda.is_available():
        raise SystemExit("bench_hourglass needs an MI355X")
    hgm = importlib.import_module(PKG + ".hourglass")
    pipeline = importlib.import_module(PKG + ".pipeline")
    dec = importlib.import_module(PKG + ".decode")
    synth = importlib.import_module(PKG + ".synth")
    capi = importlib.import_module(PKG + "._capi")
    lib = capi.lib
    dev = torch.device("cuda", 0)
    m = hgm.hg(num_stacks=8, num_blocks=1, paf_classes=38, ht_classes=19)
    sd = R.seeded_state_dict(R.state_dict_spec(8, 1, 38, 19), 3)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    S = 384
    x = (torch.rand(n, 3, S, S, generator=torch.Generator().manual_seed(0)) - 0.5).to(dev)
    rng = np.random.default_rng(1)
    hs, ps = [], []
    for _ in range(n):
        people = synth.random_people(rng, int(rng.integers(1, 9)), S, S)
        hm, pf = synth.render(people, S, S, stride=4, rng=rng)
        hs.append(hm)
        ps.append(pf)
    scene = (torch.from_numpy(np.stack(hs)).to(dev), torch.from_numpy(np.stack(ps)).to(dev))
    cfg = dec.default_config()
    cfg.MODEL.DOWNSAMPLE = 4
    est = pipeline.PoseEstimator(m, cfg)
    out = {"workload": "hg(8, 1, 38, 19) fp32, %d x 3 x %d x %d" % (n, S, S),
           "graph_replay": os.environ.get("RTPOSE_GRAPH") == "1"}
    with torch.no_grad():
        est(x, scene, scene_alpha=2e-3)  # plan, weights, forms, decoder capacities
        for _ in range(3):
            m.forward_native(x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            m.forward_native(x)
        e1.record()
        torch.cuda.synchronize()
        fwd_ms = e0.elapsed_time(e1) / iters
        prev = est.submit(x, scene, scene_alpha=2e-3)
        est.collect(prev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prev = None
        for _ in range(iters):
            t = est.submit(x, scene, scene_alpha=2e-3)
            if prev is not None:
                est.collect(prev)
            prev = t
        est.collect(prev)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        plan = m.plan_for(x)
        name = C.create_string_buffer(96)
        ms, k, fl, ex, wf = C.c_float(), C.c_int(), C.c_double(), C.c_double(), C.c_int()
        issued = 0.0
        for i in range(lib.rtpose_net_num_launches(plan.handle)):
            lib.rtpose_net_launch_executed_flops(plan.handle, i, C.byref(ex), C.byref(wf))
            issued += ex.value
        out.update({
            "images_per_s_submit_collect": round(n * iters / wall, 1),
            "ms_per_forward": round(fwd_ms, 3),
            "algorithmic_tflops_forward": round(GFLOP_PER_IMAGE * n / fwd_ms, 1),
            "issued_mfma_fraction_of_peak": round(issued / (fwd_ms * 1e9) / PEAK_F32_MFMA_TFLOPS, 3),
            "launches": lib.rtpose_net_num_launches(plan.handle),
        })
        if "--layers" in flags:
            lib.rtpose_net_set_profiling(plan.handle, 1)
            m.forward_native(x)
            torch.cuda.synchronize()
            groups, total = {}, 0.0
            for i in range(lib.rtpose_net_num_launches(plan.handle)):
                lib.rtpose_net_launch_info(plan.handle, i, C.byref(ms), C.byref(k), C.byref(fl), name, 96)
                nm = name.value.decode()
                total += ms.value
                side = _map_side(nm, S)
                kind = "%dx%d conv" % (k.value, k.value) if k.value else \
                    ("pool" if "pool" in nm else "upsample-add" if ".up" in nm else "other")
                key = "%s @%d" % (kind, side)
                g = groups.setdefault(key, [0, 0.0])
                g[0] += 1
                g[1] += ms.value
            lib.rtpose_net_set_profiling(plan.handle, 0)
            out["profiled_forward_ms"] = round(total, 3)
            out["launches_ms_by_kind_and_map_side"] = {k_: [v[0], round(v[1], 3)] for k_, v in sorted(groups.items())}
        if "--torch" in flags:
            sdd = {k_: v.to(dev) for k_, v in sd.items()}
            for _ in range(2):
                R.forward(sdd, x, 8, 1)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(max(1, iters // 4)):
                R.forward(sdd, x, 8, 1)
            e1.record()
            torch.cuda.synchronize()
            out["torch_rocm_restatement_ms_per_forward"] = round(e0.elapsed_time(e1) / max(1, iters // 4), 3)
    print(json.dumps(out))


def _map_side(launch, size):
    """Side of the map a launch of the plan writes, from its name (csrc/net.hip, build_plan_hourglass): the stem and
    layer1 at size / 2; chain j of level i of an hourglass (`hg.S.hg.i.j...`) at size >> (5 - i) for up1 (j = 0) and
    size >> (6 - i) for the others; `hg.S.poolN` writes the level below N, `hg.S.upN` level N; the rest at size / 4."""
    m = re.match(r"hg\.\d+\.hg\.(\d)\.(\d)\.", launch)
    if m:
        return size >> ((5 if m.group(2) == "0" else 6) - int(m.group(1)))
    m = re.match(r"hg\.\d+\.(pool|up)(\d)$", launch)
    if m:
        return size >> ((7 if m.group(1) == "pool" else 6) - int(m.group(2)))
    if launch == "conv1" or launch.startswith("layer1."):
        return size // 2
    if launch in ("nchw_to_nhwc8",):
        return size
    return size // 4


if __name__ == "__main__":
    main()
