"""Developer probe: how often do the records of PoseEstimator.submit / collect (decoder on the side stream) differ from the
serial path's, per dtype, and in what?   python tools/exp/overlap_flake.py [rounds] [dtype ...]"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = "pytorch_realtime_multi-person_pose_estimation_amd"


def main(rounds=10, dtypes=("bf16", "fp32")):
    pkg = importlib.import_module(PKG)
    dec = importlib.import_module(PKG + ".decode")
    synth = importlib.import_module(PKG + ".synth")
    pipeline = importlib.import_module(PKG + ".pipeline")
    dev = torch.device("cuda", 0)
    m = pkg.get_model('vgg19')
    m.load_state_dict(synth.he_init_state_dict(m, seed=0))
    m = m.cuda().float().eval()
    B, S = 16, 368

    def batch(r):
        g = torch.Generator().manual_seed(300 + r)
        h, p, _ = synth.make_batch(B, S, S, seed=400 + r)
        return (torch.rand(B, 3, S, S, generator=g) - 0.5).to(dev), (torch.from_numpy(h).to(dev), torch.from_numpy(p).to(dev))

    data = [batch(r) for r in range(3)]
    # what the decoder is given: a copy of the maps' buffer taken on the decoder's stream right in front of its launches
    seen = []
    seen_ws = []
    orig = dec.decode_enqueue

    mode = os.environ.get("SPY", "pre")

    def spy(hbase, lheat, pbase, lpaf, n, h, w, bufs, **kw):
        if mode == "post":
            orig(hbase, lheat, pbase, lpaf, n, h, w, bufs, **kw)
        npix = pkg._capi.lib.rtpose_layout_pixels(C.byref(lheat), n, h, w)
        words = npix * lheat.cstride
        base = min(hbase.value, pbase.value)
        t = None
        for plan in m._plans.values():
            ws = plan.workspace.view(-1)
            off = (base - ws.data_ptr()) // ws.element_size()
            if 0 <= off and off + words <= ws.numel():
                t = ws[off:off + words].clone() if mode != "none" else ws[:1]
        assert t is not None
        seen.append(t)
        if mode == "post":
            seen_ws.append(bufs.workspace.clone())
        if mode != "post":
            orig(hbase, lheat, pbase, lpaf, n, h, w, bufs, **kw)
    dec.decode_enqueue = spy
    pipeline.dec.decode_enqueue = spy
    order = [0, 1, 2, 2, 1, 0, 0, 1, 2, 1]
    est = None
    all_rounds = rounds
    for dt in dtypes:
        rounds = all_rounds
        if ":" in dt:
            dt, rr = dt.split(":")
            rounds = int(rr)
        m.set_compute_dtype(dt)
        if est is None or not os.environ.get("SHARED_ESTIMATOR"):
            est = pipeline.PoseEstimator(m)
        for x, scene in data:
            est(x, scene)
        del seen[:]
        del seen_ws[:]
        want = [dec.fetch(est.enqueue(x, scene)).copy() for x, scene in data]
        want_maps = [t.clone() for t in seen]
        want_ws = [t.clone() for t in seen_ws]
        again = [dec.fetch(est.enqueue(x, scene)).copy() for x, scene in data]
        print(dt, "serial path repeatable:", all(np.array_equal(a, b) for a, b in zip(want, again)))
        bad = 0
        maps_bad = 0
        for rd in range(rounds):
            prev, got = None, []
            del seen[:]
            del seen_ws[:]
            for r in order:
                t = est.submit(*data[r])
                if prev is not None:
                    got.append(est.collect(prev)[1].reshape(B, -1).copy())
                prev = t
            got.append(est.collect(prev)[1].reshape(B, -1).copy())
            if mode != "none":
                for k, r in enumerate(order):
                    d = (seen[k].view(torch.int32) != want_maps[r].view(torch.int32)).nonzero().flatten()
                    if len(d):
                        maps_bad += 1
                        ch = torch.bincount(d % 57, minlength=57)
                        print("%s round %d step %d (batch %d): the %s-decode copy of the maps differs from the serial path's in "
                              "%d words (paf %d, heat %d); first at %d: %r vs %r" % (
                                  dt, rd, k, r, mode, len(d), int(ch[:38].sum()), int(ch[38:].sum()), int(d[0]),
                                  float(seen[k][d[0]]), float(want_maps[r][d[0]])))
            for k, r in enumerate(order):
                for b in range(B):
                    a, w = dec.parse_image(got[k][b]), dec.parse_image(want[r][b])
                    same = all(np.array_equal(a[f].view(np.uint32) if a[f].dtype == np.float32 else a[f],
                                              w[f].view(np.uint32) if w[f].dtype == np.float32 else w[f])
                               for f in ("peaks", "parts", "score"))
                    if not same:
                        bad += 1
                        what = []
                        if a["peaks"].shape != w["peaks"].shape:
                            what.append("peak count %d vs %d" % (len(a["peaks"]), len(w["peaks"])))
                        else:
                            d = np.argwhere(a["peaks"].view(np.uint32) != w["peaks"].view(np.uint32))
                            if len(d):
                                i = d[0][0]
                                what.append("%d peak words, first peak %d: %s vs %s" % (len(d), i, a["peaks"][i], w["peaks"][i]))
                        if a["parts"].shape != w["parts"].shape:
                            what.append("humans %d vs %d" % (len(a["parts"]), len(w["parts"])))
                        elif not np.array_equal(a["parts"], w["parts"]):
                            what.append("parts differ")
                        if mode == "none":
                            print("%s round %d step %d (batch %d) image %d: %s" % (dt, rd, k, r, b, "; ".join(what)))
                            continue
                        d = (seen[k].view(torch.int32) != want_maps[r].view(torch.int32)).nonzero().flatten()
                        what.append("maps given to the decoder: %d words differ%s" % (
                            len(d), "" if not len(d) else " (first at %d: %r vs %r; channel %d)" % (
                                int(d[0]), float(seen[k][d[0]]), float(want_maps[r][d[0]]), int(d[0]) % 57)))
                        ds = np.argwhere(a["score"].view(np.uint32) != w["score"].view(np.uint32)).flatten()
                        what.append("human scores: %s" % ", ".join("%d: %.9g vs %.9g" % (i, a["score"][i], w["score"][i]) for i in ds[:4]))
                        if mode == "post":
                            pcap = int(got[k][b][dec.RES_HEADER + 3])
                            cw = 19 * (1 + 3 * pcap)
                            ca = seen_ws[k][b * cw:(b + 1) * cw].cpu().numpy()
                            cb = want_ws[r][b * cw:(b + 1) * cw].cpu().numpy()
                            for limb in range(19):
                                la, lb = ca[limb * (1 + 3 * pcap):][:1 + 3 * pcap], cb[limb * (1 + 3 * pcap):][:1 + 3 * pcap]
                                na, nb = int(la[0]), int(lb[0])
                                if na != nb or not np.array_equal(la[1:1 + 3 * na], lb[1:1 + 3 * nb]):
                                    cnts = got[k][b][dec.RES_PART_COUNT:dec.RES_PART_COUNT + 18]
                                    what.append("part counts %s" % list(map(int, cnts)))
                                    fa = la[1:1 + 3 * na].reshape(-1, 3)
                                    fb = lb[1:1 + 3 * nb].reshape(-1, 3)
                                    what.append("limb %d: got %s | want %s" % (
                                        limb, [(int(x[0]), int(x[1]), float(x[2:3].view(np.float32)[0])) for x in fa],
                                        [(int(x[0]), int(x[1]), float(x[2:3].view(np.float32)[0])) for x in fb]))
                        print("%s round %d step %d (batch %d) image %d: %s" % (dt, rd, k, r, b, "; ".join(what)))
        print("%s: %d differing records in %d rounds x %d steps x %d images; %d map copies differ" % (dt, bad, rounds, len(order), B, maps_bad))


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 10, tuple(a[1:]) or ("bf16", "fp32"))
