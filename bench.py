#!/usr/bin/env python
"""bench.py — end-to-end persons-posed FPS at 368x368 (net + pafprocess), the
metric BASELINE.json names, on the configuration it is quoted on:

    rtpose VGG19 368x368 batch=32 synthetic images, single MI355X, fp32

One "step" = one pass of the whole hot path over one batch that is already
resident in HBM:  rtpose_vgg forward (92 convs, fp32 MFMA)  ->  scene blend (see
below)  ->  NMS + bicubic refine  ->  PAF scoring + greedy assignment  ->
person grouping  ->  [N>1: RCCL all_gather of the result records]  ->  D2H of the
compact records + stream sync.  Nothing is cached between steps.

Data: synthetic.  Weights: seeded He-init of the reference architecture (no
checkpoint exists offline).  Because random weights produce no meaningful peaks,
the maps the decoder consumes are  scene + 1e-3 * net_output  where `scene` is a
rasterised multi-person stick-figure batch resident in HBM (pkg.synth, 1-8 people
per image); the blend is an extra elementwise kernel INSIDE the timed region, so
no work is skipped and the decoder still depends on what the network wrote.

Launch:  python bench.py --gpus 1 --steps K --warmup W
         python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
         python bench.py --gpus N ...      (N > 1 started plain: re-executes itself through
                                            torch.distributed.run with N ranks and relays rank 0's line)
One process per GPU, weak scaling (32 images per GPU), one RCCL all_gather of the
result records per step.  Rank 0 prints ONE JSON line; `ranks_seen` in it is the size of
the process group the timed region really ran in, and a WORLD_SIZE that is not --gpus is an
error, never a one-GPU measurement labelled N.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds what the
headline does not need: every timed step's records checked bit for bit against the serial
one-stream flow, the per-launch roofline leg (HIP events), the conv numerics of the plan, the
gather on its own (N > 1), the rocprofv3 traffic passes (--no-traffic drops them) and the CPU
baseline (--no-cpu-baseline drops it).
--dump-outputs DIR writes what the last timed step computed as .npy files (see dump_outputs);
the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "pytorch_realtime_multi-person_pose_estimation_amd"

BATCH = 32
SIZE = 368
GFLOP_PER_IMAGE = 271.868          # 2 x 135.934 GMAC over the 92 convs
FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
BF16_MFMA_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense bf16 MFMA peak (--dtype bf16 only)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sample_scenes):
    """the reference's arithmetic on the host cores of THIS box, bounded sample.
      net  = the oracle port (oracle/net_oracle.py: the ATen CPU conv2d / max_pool2d / cat calls the
             reference module makes, fp32), bs=1 (the reference's own usage, coco_eval.py:105) and bs=32;
      post = restated NMS (C) + the reference's pafprocess.cpp compiled UNMODIFIED
             (oracle/_ref/libpafprocess_ref.so, fed x8 INTER_NEAREST maps exactly like
             paf_to_pose.py:381-386) when that binary travelled with the snapshot, else the C restatement.
    `value` = the better of the reference's serial per-image flow, 1 / (net bs=1 s/img + post s/img), and the
    batched one, 1 / (net bs=32 s/img + post s/img), each at its own best torch thread count (`value_flow`
    says which; `cores` = the threads of that flow)."""
    from oracle import net_oracle, post_oracle
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    logical = os.cpu_count() or 1
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = logical
    m = pkg.get_model('vgg19')
    sd = synth.he_init_state_dict(m, seed=0)
    g = torch.Generator().manual_seed(0)
    # torch's intra-op pool: os.cpu_count() can exceed what this process may use (cgroup quota /
    # affinity), so the candidates stop at the affinity; EVERY candidate is timed on the real input -
    # 1 x 3 x 368 x 368 for the reference's serial flow, 8 x 3 x 368 x 368 for the batched pass (round 4
    # probed a quarter-size image, stopped at the first slow size and never tried more than 32 of 256
    # logical CPUs) - the fastest is kept for each, all times are reported
    cands = sorted({t for t in (avail, 256, 192, 128, 96, 64, 32, 16, 8, 4) if t <= avail})

    def probe(x, reps):
        # ascending; stops after two consecutive candidates slower than the best so far (round 5 spent 115 s of the
        # driver's run on two 256-thread passes 40x slower than the 16-thread one)
        tried, best, worse = {}, None, 0
        for t in cands:
            if worse >= 2:
                break
            torch.set_num_threads(t)
            net_oracle.forward(sd, torch.rand(1, 3, 64, 64, generator=g) - 0.5)   # warm the pool
            t0 = time.perf_counter()
            for _ in range(reps):
                net_oracle.forward(sd, x)
            dt = (time.perf_counter() - t0) / reps
            tried[t] = round(dt, 4)
            if best is None or dt < best[0]:
                best = (dt, t)
                worse = 0
            else:
                worse += 1
        return best[1], tried
    threads, tried = probe(torch.rand(1, 3, SIZE, SIZE, generator=g) - 0.5, 2)
    threads_b, tried_b = probe(torch.rand(8, 3, SIZE, SIZE, generator=g) - 0.5, 1)
    torch.set_num_threads(threads)
    t_net, n_net = 0.0, 0
    while n_net < 8 and t_net < 8.0:
        x = torch.rand(1, 3, SIZE, SIZE, generator=g) - 0.5               # bs=1 like coco_eval.py:105
        t0 = time.perf_counter()
        net_oracle.forward(sd, x)
        t_net += time.perf_counter() - t0
        n_net += 1
    torch.set_num_threads(threads_b)
    xb = torch.rand(BATCH, 3, SIZE, SIZE, generator=g) - 0.5              # one bs=32 pass
    t0 = time.perf_counter()
    net_oracle.forward(sd, xb)
    t_b32 = (time.perf_counter() - t0) / BATCH
    torch.set_num_threads(threads)
    heat, paf = sample_scenes
    use_ref = post_oracle.have_ref()
    t_nms = t_pp = 0.0
    for i in range(heat.shape[0]):
        t0 = time.perf_counter()
        jl = post_oracle.nms(heat[i])
        t1 = time.perf_counter()
        if use_ref:                      # paf_to_pose.py:382-386: x8 nearest maps, then process_paf
            post_oracle.ref_process_paf(jl, post_oracle.upsample_nearest(heat[i], 8),
                                        post_oracle.upsample_nearest(paf[i], 8))
        else:
            post_oracle.process_paf(jl, paf[i], 8)
        t2 = time.perf_counter()
        t_nms += t1 - t0
        t_pp += t2 - t1
    n_post = heat.shape[0]
    t_post = (t_nms + t_pp) / n_post
    per_img = t_net / n_net + t_post
    # BASELINE.json configs[0] on THIS box: the picture_demo.py flow on readme/ski.jpg (674 x 712 -> net input
    # 1 x 3 x 368 x 392, maps 46 x 49).  /root/reference does not exist here, so the pixels are synthetic and the
    # arithmetic is the port's; with random weights the maps are junk, so the post step is timed on a synthetic
    # 46 x 49 scene of the same geometry instead of on them (with real weights it is ~1-10 ms either way).
    c1 = None
    try:
        x1 = torch.rand(1, 3, 368, 392, generator=g) - 0.5
        net_oracle.forward(sd, x1)
        t0 = time.perf_counter()
        for _ in range(3):
            net_oracle.forward(sd, x1)
        t_c1 = (time.perf_counter() - t0) / 3
        h1, p1, _ = synth.make_batch(1, 368, 392, seed=7)
        t0 = time.perf_counter()
        jl1 = post_oracle.nms(h1[0])
        if use_ref:
            post_oracle.ref_process_paf(jl1, post_oracle.upsample_nearest(h1[0], 8), post_oracle.upsample_nearest(p1[0], 8))
        else:
            post_oracle.process_paf(jl1, p1[0], 8)
        t_c1p = time.perf_counter() - t0
        c1 = {"net_s": round(t_c1, 4), "post_s": round(t_c1p, 4), "images_per_s": round(1.0 / (t_c1 + t_c1p), 3),
              "what": "configs[0] geometry (1 x 3 x 368 x 392, maps 46 x 49): oracle-port forward + NMS + process_paf"}
    except Exception as e:   # noqa: BLE001
        c1 = {"error": str(e)[:200]}
    per_img_b = t_b32 + t_post
    batched_wins = per_img_b < per_img
    return {"value": round(1.0 / min(per_img, per_img_b), 3), "unit": "images/s",
            "cores": threads_b if batched_wins else threads, "kind": "port",
            "value_flow": "bs=32 batched forward" if batched_wins else "bs=1 serial forward (the reference's usage)",
            "serial_bs1_img_s": round(1.0 / per_img, 3), "torch_threads_bs32": threads_b,
            "thread_probe_bs8_s_per_pass": tried_b,
            "post_kind": "reference" if use_ref else "port",
            "cpu_model": _cpu_model(), "os_cpu_count": logical, "sched_affinity": avail,
            "torch_threads": threads, "thread_probe_s": tried,
            "net_bs1_img_s": round(n_net / t_net, 3), "net_bs32_img_s": round(1.0 / t_b32, 3),
            "post_img_s": round(1.0 / t_post, 1),
            "end_to_end_bs32_img_s": round(1.0 / (t_b32 + t_post), 3),
            "config1_picture_demo": c1,
            "sample": "net: %d images 368x368 at bs=1 (%.3f s/img, %d threads) + one bs=32 pass (%.3f s/img, %d threads) "
                      "through the torch-CPU fp32 oracle port, thread counts probed on the real shapes up to the "
                      "affinity; post: %d synthetic scenes, restated C NMS (%.2f ms/img) + %s (%.2f ms/img), 1 thread"
                      % (n_net, t_net / n_net, threads, t_b32, threads_b, n_post, t_nms / n_post * 1e3,
                         "the reference's pafprocess.cpp compiled unmodified (oracle/_ref) on x8 nearest maps"
                         if use_ref else "the C restatement of process_paf (oracle/_ref absent)",
                         t_pp / n_post * 1e3)}


def algorithmic_bytes_7x7(two_byte):
    """HBM bytes one grouped (PAF + heat-map branch) 7x7 launch must move at least: its input read
    once, both branches' weights and biases, both outputs - averaged over the 25 such launches of a
    forward (5 stages x [one 185 -> 128 layer whose 185-channel input the two branches share + four
    128 -> 128 layers with one input per branch]); rtpose_vgg.py:108-127."""
    e = 2 if two_byte else 4
    npix = BATCH * (SIZE // 8) * (SIZE // 8)
    first = npix * 185 * e + 2 * (185 * 49 * 128 * e + 128 * 4) + 2 * npix * 128 * e
    other = 2 * npix * 128 * e + 2 * (128 * 49 * 128 * e + 128 * 4) + 2 * npix * 128 * e
    return int(round((5 * first + 20 * other) / 25.0))


def measure_traffic(timeout_s=150, dtype="fp32"):
    """HBM/fabric bytes per launch of the dominant (7x7) kernel from the rocprofv3 PMC counters,
    collected as MI355X_MICROARCH.md §HBM prescribes: FETCH_SIZE and WRITE_SIZE in SEPARATE
    `--pmc` passes (they do not fit one pass), with `--kernel-trace` only, FETCH_SIZE doubled
    (gfx950 counts the 128-B requests of wide coalesced reads as 64 B).  Each pass profiles one
    warm + one measured forward of the same 32 x 368 x 368 workload in a child process.  Any
    failure -> None (the FPS line never depends on the profiler)."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    tool = os.path.join(ROOT, "tools", "profile_layers.py")
    out = {}
    tmp = tempfile.mkdtemp(prefix="rtpose_pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            env = dict(os.environ, TMPDIR="/tmp")
            p = subprocess.run([exe, "--pmc", counter, "--kernel-trace", "-d", d, "-o", "t", "--", sys.executable, tool,
                                str(BATCH), str(SIZE), str(SIZE), "1", dtype], cwd="/tmp", env=env, timeout=timeout_s,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            if p.returncode != 0:
                return None
            db = None
            for r, _, files in os.walk(d):
                for f in files:
                    if f.endswith(".db"):
                        db = os.path.join(r, f)
            if not db:
                return None
            cur = sqlite3.connect(db).cursor()
            row = cur.execute("select sum(value), count(distinct dispatch_id) from counters_collection "
                              "where counter_name = ? and kernel_name like ?",
                              (counter, "%conv_mfma_bf16<7, 16, 0%" if dtype == "bf16x3" else
                               "%conv_mfma_bf16<7, 32, 0%" if dtype == "bf16" else
                               "%wino7_f32%" if os.environ.get("RTPOSE_WINOGRAD", "1")[:1] in ("1", "7") else
                               "%conv_mfma_f32<7, 16, 0%")).fetchone()
            if not row or not row[1]:
                return None
            out[counter] = float(row[0]) / float(row[1]) * 1024.0      # KiB per launch -> bytes
        return {"fetch_bytes": 2.0 * out["FETCH_SIZE"], "write_bytes": out["WRITE_SIZE"],
                "note": "per launch; FETCH_SIZE x2 (gfx950 wide-read correction), WRITE_SIZE uncalibrated"}
    except Exception:   # noqa: BLE001  (profiler trouble must never take the bench down)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dump_outputs(path, block, dec, cfg, maps):
    """--dump-outputs: what the last timed step handed out, as float32 / float64 .npy files in ``path``.
      records_peaks.npy   float32 [P, 6]  image index + the joint_list row of decode.parse_image (x, y, score, id, part)
      records_humans.npy  float64 [H, 20] image index, the 18 part assignments (-1 = none), the human score
      records_counts.npy  float64 [N, 3]  peaks, humans and overflow flags of each image
      paf.npy, heatmap.npy float32 NCHW   the maps the decoder read (scene + 1e-3 * net output) of this rank's images
    ``block``: the int32 record block [N, words] the step returned (every rank's images under a collective)."""
    os.makedirs(path, exist_ok=True)
    recs = [dec.parse_image(r, cfg) for r in np.asarray(block)]
    peaks = [np.column_stack([np.full(len(r["peaks"]), i, np.float32), r["peaks"]]) for i, r in enumerate(recs)]
    humans = [np.column_stack([np.full(len(r["score"]), i, np.float64), r["parts"].astype(np.float64),
                               r["score"].astype(np.float64)]) for i, r in enumerate(recs)]
    counts = [(r["n_peaks"], len(r["score"]), r["flags"]) for r in recs]
    np.save(os.path.join(path, "records_peaks.npy"), np.concatenate(peaks, 0).astype(np.float32))
    np.save(os.path.join(path, "records_humans.npy"), np.concatenate(humans, 0).astype(np.float64))
    np.save(os.path.join(path, "records_counts.npy"), np.asarray(counts, dtype=np.float64).reshape(-1, 3))
    for name, t in maps.items():
        np.save(os.path.join(path, name + ".npy"), t.detach().cpu().numpy().astype(np.float32))


def stub_main(args, par):
    """TEST INFRASTRUCTURE: the contract's skeleton - one process per rank, barrier + timing of exactly --steps steps,
    max over ranks, one all_gather of the result records per step, rank 0 prints ONE line - on CPU ranks over gloo with a
    stand-in step (a record block filled with the rank's number).  Proves that `bench.py --gpus N` started plain really
    runs N ranks and says so; it measures nothing."""
    rank, _, world = par.init_from_env("gloo", always=True)
    dev = torch.device("cpu")
    words = 64
    blk = torch.full((BATCH, words), rank, dtype=torch.int32)
    seen = set()

    def step():
        allrec = par.gather_records(blk, world, force=torch.distributed.is_initialized())
        seen.update(int(v) for v in allrec[:, 0].unique())
        return allrec

    for _ in range(max(args.warmup, 1)):
        step()
    par.barrier(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        allrec = step()
    par.barrier(dev)
    local = time.perf_counter() - t0
    elapsed = par.max_over_ranks(local, dev)
    per_rank = par.all_gather_floats(local, dev)
    ranks_seen = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    ok = sorted(seen) == list(range(world)) and tuple(allrec.shape) == (world * BATCH, words)
    if rank == 0:
        print(json.dumps({"metric": "STUB - launcher / gather skeleton only, not a measurement", "value": None,
                          "unit": "images/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int32",
                          "data": "stub", "config": {"workload": "stub step on CPU ranks (gloo)", "global_batch": BATCH * world},
                          "records_from_ranks": sorted(seen), "gathered_block_ok": ok,
                          "per_rank_s": [round(v, 6) for v in per_rank]}), flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also the checks and secondary figures a plain run skips: records of every timed step against the "
                         "serial flow, roofline leg, conv numerics, gather timing, rocprofv3 traffic, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-traffic", action="store_true", help="--full without the two rocprofv3 PMC passes")
    ap.add_argument("--dtype", choices=("fp32", "bf16", "bf16x3"), default="fp32",
                    help="fp32 = BASELINE.json configs[1] (the contract, default); bf16 = the configs[2] "
                         "arithmetic (bf16 operands, fp32 accumulate); bf16x3 = split bf16 operands, 3 MFMAs per "
                         "product (fp32-grade maps from the bf16 pipe) - both on the same workload, for reference")
    # test infrastructure (tests/test_host_cpu.py): the launcher / barrier / timing / gather skeleton on CPU ranks
    # over gloo with a stand-in for the GPU step.  Its line says so and is not a measurement.
    ap.add_argument("--decode-overlap", type=int, choices=(0, 1), default=1,
                    help="1 (default): the decoder and the record D2H of step k run on a second stream under the forward "
                         "of step k + 1 (PoseEstimator.submit / collect); 0: everything on one stream, step by step")
    ap.add_argument("--stub-step", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    par = importlib.import_module(PKG + ".parallel")
    if not args.stub_step:
        par.require_devices(args.gpus, "bench.py")      # before any rank is spawned
    if args.gpus > 1 and not par.launched_by_torchrun():
        # started plain: run the N ranks ourselves (the driver's own launch line), relay their output
        raise SystemExit(par.relaunch_under_torchrun(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    if par.env_world()[2] != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d - refusing to label a %d-rank run as %d GPUs"
                         % (args.gpus, par.env_world()[2], par.env_world()[2], args.gpus))
    if args.stub_step:
        return stub_main(args, par)

    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    dec = importlib.import_module(PKG + ".decode")
    pipeline = importlib.import_module(PKG + ".pipeline")
    lib = pkg._capi.lib

    # (under torchrun even a world of one joins an RCCL process group and gathers through it)
    rank, local_rank, world = par.init_from_env("nccl", always=True)
    collective = torch.distributed.is_initialized()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path for the product)")
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    model = pkg.get_model('vgg19')
    model.load_state_dict(synth.he_init_state_dict(model, seed=0))   # no checkpoint exists offline
    model = model.cuda().float().eval()
    model.set_compute_dtype(args.dtype)
    bf16 = args.dtype != "fp32"
    x3 = args.dtype == "bf16x3"
    # bf16x3 spends three bf16 MFMAs per algorithmic multiply-add
    peak = (BF16_MFMA_PEAK_TFLOPS / 3.0 if x3 else BF16_MFMA_PEAK_TFLOPS) if bf16 else FP32_MFMA_PEAK_TFLOPS
    est = pipeline.PoseEstimator(model)

    g = torch.Generator().manual_seed(rank)
    x = (torch.rand(BATCH, 3, SIZE, SIZE, generator=g) - 0.5).to(dev)
    heat_np, paf_np, _ = synth.make_batch(BATCH, SIZE, SIZE, seed=100 + rank)
    scene = (torch.from_numpy(heat_np).to(dev), torch.from_numpy(paf_np).to(dev))

    def step():
        bufs = est.enqueue(x, scene)
        n_local, words = bufs.n, bufs.words
        if collective:
            allrec = par.gather_records(bufs.result.view(n_local, words), world, force=True)
            host = allrec.cpu()                      # D2H + sync
        else:
            host = dec.fetch(bufs)                   # pinned D2H + stream sync
        return bufs, host

    post = (lambda blk: par.gather_records(blk, world, force=True)) if collective else None

    def run_steps(k, keep=None):
        """k steps of the production configuration -> (buffers, records) of the last one.  With --decode-overlap 1
        step i's decoder, gather and record D2H run on the side stream while step i + 1's forward is already on the
        compute stream; the host takes step i's records after it has submitted step i + 1, and the last step's before
        it returns - all k steps are complete when this returns.  ``keep``: a list that receives a copy of THIS rank's
        record block of every step (0.3 MB memcpy per step; the pinned block is reused two steps later)."""
        def take(out):
            if keep is not None:
                keep.append(np.array(np.asarray(out[1]).reshape(-1, out[0].words)[rank * BATCH:(rank + 1) * BATCH]
                                     if collective else np.asarray(out[1]).reshape(-1, out[0].words)))
            return out
        if not args.decode_overlap:
            for _ in range(k):
                out = take(step())
            return out
        prev = None
        for _ in range(k):
            t = est.submit(x, scene, post=post)
            if prev is not None:
                take(est.collect(prev))
            prev = t
        return take(est.collect(prev))

    # capacity check + warm-up (untimed)
    recs0 = est(x, scene)
    humans_per_batch = sum(r["parts"].shape[0] for r in recs0)
    peaks_per_batch = sum(r["n_peaks"] for r in recs0)
    if args.full:
        # what every step has to return: the records of the SERIAL flow (one stream, forward -> blend -> decode -> D2H,
        # nothing beside the decoder) over the same batch, taken before the timed region
        ref_bufs = est.enqueue(x, scene)
        ref_block = dec.fetch(ref_bufs).copy()
        ref_mask = dec.result_mask(ref_block)
    run_steps(max(args.warmup, 1))              # >= 1 untimed step: also warms the RCCL gather

    plan = model.plan_for(x)
    nl = lib.rtpose_net_num_launches(plan.handle)
    # arithmetic of the plan as rtpose_net_conv_numerics reports it (fp32: the guarded per-layer AUTO choice is the
    # library default; the estimates are those of the filters loaded above)
    numerics = None
    if args.full and not bf16:
        names = {0: "direct", 3: "F(2x2,3x3)", 43: "F(4x4,3x3)", 4: "F(4,7)", 6: "F(6,7)"}
        forms, worst = {}, {}
        for _, form, amp in model.conv_numerics(plan):
            forms[names[form]] = forms.get(names[form], 0) + 1
            for nm, a in zip(("F(2x2,3x3)", "F(4,7)", "F(6,7)", "F(4x4,3x3)"), amp):
                worst[nm] = round(max(worst.get(nm, 0.0), a), 1)
        numerics = {"mode": "library default: per-layer AUTO, the fastest form whose amplification estimate <= amp_limit",
                    "amp_limit": 256.0, "convs_by_form": forms, "worst_amplification_estimate": worst}

    # ---- the timed region: EXACTLY --steps steps of the production configuration (no per-launch events, no
    # library queries), bracketed by barrier + synchronize on both sides -------------------------------------
    torch.cuda.synchronize()
    par.barrier(dev)
    t0 = time.perf_counter()
    kept = [] if args.full else None
    bufs, host = run_steps(args.steps, kept)
    torch.cuda.synchronize()
    par.barrier(dev)
    elapsed_local = time.perf_counter() - t0
    if args.full:
        # every block the timed steps handed out (copied inside the region, compared here, outside it) against the
        # serial flow's: all result words bit for bit - peak coordinates, scores, ids, part assignments, human scores
        differing = [i for i, blk in enumerate(kept)
                     if blk.shape != ref_block.shape or not np.array_equal(blk[ref_mask], ref_block[ref_mask])]
        if len(kept) != args.steps or differing:
            raise SystemExit("bench.py: rank %d: the records of %d of %d timed steps differ from the serial flow's "
                             "(steps %s) - the measurement is void" % (rank, len(differing), len(kept), differing[:8]))
    flags = int(np.bitwise_or.reduce(np.asarray(host).reshape(-1, bufs.words)[:, dec.RES_HEADER + 2]))
    if flags:
        raise SystemExit("decode tables overflowed inside the timed region (flags=%d)" % flags)
    if args.dump_outputs and rank == 0:
        # the last timed step's records and the maps its decoder read (no step has run on this plan since)
        dump_outputs(args.dump_outputs, np.asarray(host).reshape(-1, bufs.words), dec, bufs.cfg,
                     {"paf": model.read_output(plan, 10), "heatmap": model.read_output(plan, 11)})
    elapsed = par.max_over_ranks(elapsed_local, dev)
    per_rank_s = par.all_gather_floats(elapsed_local, dev)
    ranks_seen = torch.distributed.get_world_size() if collective else 1
    gather_us = None
    if args.full and collective:    # the exchange step on its own, after the timed region: all_gather of one step's block
        blk = bufs.result.view(bufs.n, bufs.words)
        torch.cuda.synchronize()
        par.barrier(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            par.gather_records(blk, world, force=True)
        torch.cuda.synchronize()
        gather_us = par.max_over_ranks((time.perf_counter() - t0) / 20 * 1e6, dev)

    # ---- roofline leg, AFTER the timed region: the same step with per-launch HIP events recorded on the launch
    # stream (rtpose_net_set_profiling), for the average duration of the dominant kernel ------------------------
    k7_ms, k7_flops, k7_exec, k7_n, k7_wino, net_ms, k7_form = 0.0, 0.0, 0.0, 0, 0, 0.0, 0
    k3_ms, k3_flops, k3_exec, k3_n, k3_form = 0.0, 0.0, 0.0, 0, 0   # the second kernel family: the 3x3 convs
    prof_steps = max(3, min(args.steps, 8))
    if args.full:
        lib.rtpose_net_set_profiling(plan.handle, 1)
        step()                                      # (the first profiled forward creates the events)
        for _ in range(prof_steps):
            step()
            ms, k, fl, fx, wf = C.c_float(), C.c_int(), C.c_double(), C.c_double(), C.c_int()
            for i in range(nl):
                lib.rtpose_net_launch_info(plan.handle, i, C.byref(ms), C.byref(k), C.byref(fl), None, 0)
                if ms.value > 0:
                    net_ms += ms.value
                    if k.value == 7:
                        lib.rtpose_net_launch_executed_flops(plan.handle, i, C.byref(fx), C.byref(wf))
                        k7_ms += ms.value
                        k7_flops += fl.value
                        k7_exec += fx.value
                        k7_wino += 1 if wf.value else 0
                        k7_form = wf.value
                        k7_n += 1
                    elif k.value == 3:
                        lib.rtpose_net_launch_executed_flops(plan.handle, i, C.byref(fx), C.byref(wf))
                        k3_ms += ms.value
                        k3_flops += fl.value
                        k3_exec += fx.value
                        k3_form = max(k3_form, wf.value)
                        k3_n += 1
        lib.rtpose_net_set_profiling(plan.handle, 0)
    status = model.device_status(plan) if not bf16 else 0
    if status:
        raise SystemExit("device error word %d after the run (split-tile hand-over timed out)" % status)

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        fps = BATCH * world * args.steps / elapsed
        achieved = k7_flops / (k7_ms * 1e-3) / 1e12 if k7_ms > 0 else 0.0
        executed = k7_exec / (k7_ms * 1e-3) / 1e12 if k7_ms > 0 else 0.0
        wino7 = k7_wino == k7_n and k7_n > 0
        out = {
            "metric": "end-to-end persons-posed FPS at 368x368 (net+pafprocess)",
            "value": round(fps, 2), "unit": "images/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("rtpose VGG19 368x368 batch=32 synthetic images, single MI355X, %s "
                                    "(NOT the contract config: BASELINE.json configs[1] is fp32)" % (
                                        "split bf16 operands hi+lo, 3 bf16 MFMAs per product, fp32 accumulate"
                                        if x3 else "bf16 operands / fp32 accumulate")
                                    if bf16 else
                                    "rtpose VGG19 368x368 batch=32 synthetic images, single MI355X, fp32 "
                                    "(BASELINE.json configs[1]); per-GPU batch 32, one process per GPU"),
                       "global_batch": BATCH * world, "image": [SIZE, SIZE],
                       "weights": "seeded He init (no checkpoint offline)",
                       "decoder_input": "synthetic scene + 1e-3 * net output (blend kernel timed)",
                       "pipeline": ("one stream, step by step" if not args.decode_overlap else
                                    "decoder + record D2H of step k on a second stream; the forward of step k + 1 is queued "
                                    "at once but starts when that decoder has read the maps (RTPOSE_GUARD_WHOLE_FORWARD=1)"
                                    if os.environ.get("RTPOSE_GUARD_WHOLE_FORWARD") == "1" or os.environ.get("RTPOSE_GUARD_FINE") == "0" else
                                    "decoder + record D2H of step k on a second stream under the forward of step k + 1 (the "
                                    "forward waits for that decoder only in front of its first launch that rewrites the maps' "
                                    "buffer; library default, DESIGN.md 3.3)"),
                       "humans_per_batch": humans_per_batch, "peaks_per_batch": peaks_per_batch,
                       "conv_numerics": numerics,
                       "parallelism": ("image-sharded, all_gather of result records only" if world > 1 else
                                       "single GPU, RCCL all_gather of a world of one" if collective else "single GPU")},
            "per_rank_images_per_s": {"min": round(BATCH * args.steps / max(per_rank_s), 2),
                                      "max": round(BATCH * args.steps / min(per_rank_s), 2)},
            "multi_gpu_note": ("N > 1 has never run on hardware from this code (1-GPU leases only): unmeasured"
                               if world == 1 else "measured on %d ranks" % ranks_seen),
            "net_tflops_end_to_end": round(fps / world * GFLOP_PER_IMAGE / 1e3, 2),
        }
        if args.full:
            out.update({
                "records_verified": len(kept),
                "records_verified_note": "every timed step's record block (this rank's %d images: peaks, scores, ids, part "
                                         "assignments, human scores) equals the serial one-stream flow's bit for bit; blocks "
                                         "copied inside the timed region, compared after it; a difference exits non-zero" % BATCH,
                "gather_us_per_step": None if gather_us is None else round(gather_us, 1),
                "net_ms_per_step_events": round(net_ms / prof_steps, 3),
                "roofline": {"bound": "mfma",
                             "kernel": ("conv_mfma_bf16<7,16,0,..,SP=2>" if x3 else
                                        "conv_mfma_bf16<7,32,0>" if bf16 else
                                        "wino7_f32 (F(%d,7) Winograd along x)" % k7_form if wino7 else "conv_mfma_f32<7,16,0>") +
                                       " (7x7 stage convs, 68% of the network's direct-convolution FLOPs)",
                             "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                             "frac": round(achieved / peak, 4), "traffic": None,
                             # `achieved` counts the ALGORITHMIC flops of the direct 7x7 sum.  In
                             # Winograd form the kernel issues 84/294 of them (F(6,7); + group / channel padding), so
                             # frac may exceed 1; executed_frac = issued MFMA flops / time / peak is the
                             # matrix-pipe utilisation and cannot.
                             "executed": round(executed, 2), "executed_frac": round(executed / peak, 4),
                             "note": "achieved = SURVEY 8(d) direct-convolution flops / event time (the contract's "
                                     "definition; > peak in Winograd form). executed = MFMA flops the launch issues "
                                     "(= SQ_INSTS_MFMA x 4096, profiles/) / event time: the matrix-pipe roofline fraction. "
                                     "Events are taken in %d extra steps after the timed region." % prof_steps,
                             "launches_timed": k7_n,
                             "flops_per_launch": round(k7_flops / max(k7_n, 1)),
                             "avg_launch_ms": round(k7_ms / max(k7_n, 1), 4)},
            })
        if k3_ms > 0:
            # not part of the contract's roofline object: the same accounting for the 3x3 convs (conv1_1 .. conv4_4_CPM
            # and the stage-1 convs), the second-largest share of the step
            out["roofline_3x3"] = {
                "kernel": ("wino4_f32 / wino4s_f32 (F(4x4,3x3))" if k3_form == 43 else
                           "wino_f32 (F(2x2,3x3))" if k3_form == 3 else "direct / bf16 kernels") +
                          " + conv_first_kernel (conv1_1)",
                "ms_per_forward": round(k3_ms / prof_steps, 3), "launches_per_forward": k3_n // prof_steps,
                "achieved": round(k3_flops / (k3_ms * 1e-3) / 1e12, 2), "executed": round(k3_exec / (k3_ms * 1e-3) / 1e12, 2),
                "executed_frac": round(k3_exec / (k3_ms * 1e-3) / 1e12 / peak, 4), "peak": peak, "unit": "TFLOP/s",
                "note": "achieved = direct-convolution flops / event time; executed = MFMA flops issued (whole tiles, "
                        "36 frequencies per 4 x 4 outputs in F(4x4,3x3)) / event time"}
        if args.full and world == 1 and not args.no_traffic and "ROCPROF" not in "".join(os.environ.keys()).upper():
            # free this process's GPU memory pressure is irrelevant (288 GB); the child runs its own plan
            tr = measure_traffic(dtype=args.dtype)
            if tr:
                out["roofline"]["traffic"] = round(tr["fetch_bytes"] + tr["write_bytes"])
                out["roofline"]["traffic_detail"] = tr
                out["roofline"]["algorithmic_bytes_per_launch"] = algorithmic_bytes_7x7(bf16 and not x3)
        if args.full:
            out["cpu_baseline"] = cpu_baseline((heat_np, paf_np)) if world == 1 and not args.no_cpu_baseline else None
        print(json.dumps(out), flush=True)
    if collective:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
