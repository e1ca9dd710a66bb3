"""The table-driven decoder (csrc/decode.hip) on the MI355X.  Everything a record holds is integers and float bit
patterns: every comparison here is bit for bit, inside decode.result_mask (the words a record defines).

  * the COCO-18 preset through rtpose_decode_batch_skel against rtpose_decode_batch_ex, word for word, and both against
    tests/golden/decode_coco18_records.npz: what the fixed COCO-18 kernels wrote before the two doors came to share one
    kernel set (tools/make_golden_decode_records.py) - also at the capacities on both sides of every launcher switch and
    for rtpose_nms_batch_ex;
  * BODY_25, a 2-part / 1-limb table, a 32-part / 32-limb table with scattered PAF channels and COCO-18 walked backwards
    under seed mask 0x15555 against the host restatement (tests/skeleton_restate.py), at capacities on both sides of every
    switch of the launcher, into sentinel-filled buffers of exactly the queried sizes with a guard region behind them;
  * rtpose_nms_batch_skel against the oracle's NMS with num_keypoints below P;
  * PoseEstimator(skeleton=BODY_25) over OpenPose_Model(4, 2, 52, 26) and a stride-4 hourglass, serial and pipelined.

tests/test_skeleton_cpu.py checks on the CPU that the scene sets used here hold people, merges, refused seeds and
overflows (and says which of the issue's conditions two of the tables cannot meet, and why).
"""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skeleton_restate as sr  # noqa: E402
from decode_run import GUARD, SENTINEL, run_decode as _run  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "post_scenes.npz")


@pytest.fixture(scope="module")
def dec(pkg):
    return importlib.import_module(pkg.__name__ + ".decode")


@pytest.fixture(scope="module")
def skm(pkg):
    return importlib.import_module(pkg.__name__ + ".skeleton")


# ---- 5. the same records through both doors, and the records of the fixed COCO-18 kernels they replaced ----------------
GOLD_RECORDS = os.path.join(os.path.dirname(__file__), "golden", "decode_coco18_records.npz")
DOOR_FLAGS = [0, 1, 2]                                  # refine, RTPOSE_NMS_NO_REFINE, RTPOSE_NMS_GAUSSIAN
DOOR_CAPS = [(32, 64), (111, 64)]                       # (max_peaks_per_part, max_humans), at every flag
SWITCH_CAPS = [(4, 4), (65, 64), (128, 64), (32, 400)]  # both sides of every launcher switch, at flags 0 (CAPS below)


def _door_scenes(synth):
    z = np.load(GOLD)
    scenes = [("golden%d" % i, z["heat%d" % i][None], z["paf%d" % i][None]) for i in range(int(z["n"]))]
    heat, paf, _ = synth.make_batch(4, 368, 368, seed=5)            # crowded figures: exact score ties among them
    scenes.append(("synth368", heat, paf))
    heat, paf, _ = synth.make_batch(3, 184, 248, seed=9)
    scenes.append(("synth23x31", heat, paf))
    rng = np.random.default_rng(0)                                  # junk: many peaks, no structure
    scenes.append(("noise", rng.uniform(0, 0.3, (2, 13, 29, 19)).astype(np.float32),
                   rng.uniform(-1, 1, (2, 13, 29, 38)).astype(np.float32)))
    return scenes


def _gold_key(kind, flags, pcap, hcap, scene):
    """Name of one (case, scene batch) entry of decode_coco18_records.npz; kind 'decode' or 'nms'."""
    return "%s_f%d_p%d_h%d_%s" % (kind, flags, pcap, hcap, scene)


def _maps_digest(heat, paf):
    return hashlib.sha256(np.ascontiguousarray(heat).tobytes() + np.ascontiguousarray(paf).tobytes()).hexdigest()


def _record_digest(block, mask):
    """SHA-256 of the int32 words of a record block inside `mask`, in record order."""
    return hashlib.sha256(np.ascontiguousarray(block[mask], dtype="<i4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def gold_records():
    return np.load(GOLD_RECORDS)


def _assert_parent_records(dec, gold, key, name, heat, paf, got, header_words):
    """`got` against what the fixed COCO-18 kernels wrote for this case (tools/make_golden_decode_records.py): the header
    words, the digest of the words inside the parent's result mask, and - to name the word on a failure - the records."""
    assert str(gold["maps_" + name]) == _maps_digest(heat, paf), "%s: not the maps the fixture was recorded on" % name
    want = gold[key + "_records"]
    assert got.shape == want.shape, key
    assert np.array_equal(got[:, header_words], gold[key + "_header"][:, header_words]), key
    m = dec.result_mask(want)
    diff = np.argwhere(got[m] != want[m])
    assert diff.size == 0, "%s: %d words differ from the parent's record, the first at masked index %d" % (
        key, len(diff), int(diff[0, 0]))
    assert _record_digest(got, m) == str(gold[key + "_sha256"]), key


@pytest.mark.parametrize("pcap", [c[0] for c in DOOR_CAPS])
@pytest.mark.parametrize("flags", DOOR_FLAGS, ids=["refine", "no_refine", "gaussian"])
def test_coco18_preset_writes_the_records_of_the_old_entry_point(capi, dec, skm, pkg, cuda, gold_records, flags, pcap):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    coco = skm.COCO18.native()
    humans = 0
    for name, heat, paf in _door_scenes(synth):
        heat_d, paf_d = torch.from_numpy(heat).to(cuda), torch.from_numpy(paf).to(cuda)
        cfg = capi.DecodeCfg(18, 8, 0.1, pcap, 64)
        old = _run(capi, cuda, heat_d, paf_d, cfg, None, flags)
        new = _run(capi, cuda, heat_d, paf_d, cfg, coco, flags)
        assert old.shape == new.shape, name
        m = dec.result_mask(old)
        assert np.array_equal(m, dec.result_mask(new)), name
        assert np.array_equal(new[m], old[m]), "%s: the two entry points' records differ" % name
        assert (old[:, 5:7] == 0).all() and (new[:, 5] == 18).all() and (new[:, 6] == 19).all(), name
        # both doors run one kernel set now: what pins it is the record of the fixed kernels
        key = _gold_key("decode", flags, pcap, 64, name)
        _assert_parent_records(dec, gold_records, key, name, heat, paf, old, slice(0, 8))
        _assert_parent_records(dec, gold_records, key, name, heat, paf, new, [0, 1, 2, 3, 4, 7])
        humans += int(old[:, 1].sum())
    assert humans > 12


@pytest.mark.parametrize("caps", SWITCH_CAPS, ids=["%dx%d" % c for c in SWITCH_CAPS])
def test_old_entry_point_at_the_launcher_switches_writes_the_parent_records(capi, dec, pkg, cuda, gold_records, caps):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    for name, heat, paf in _door_scenes(synth):
        cfg = capi.DecodeCfg(18, 8, 0.1, caps[0], caps[1])
        got = _run(capi, cuda, torch.from_numpy(heat).to(cuda), torch.from_numpy(paf).to(cuda), cfg, None, 0)
        _assert_parent_records(dec, gold_records, _gold_key("decode", 0, caps[0], caps[1], name), name, heat, paf, got,
                               slice(0, 8))


@pytest.mark.parametrize("flags", DOOR_FLAGS, ids=["refine", "no_refine", "gaussian"])
def test_old_nms_entry_point_writes_the_parent_records(capi, dec, pkg, cuda, gold_records, flags):
    synth = importlib.import_module(pkg.__name__ + ".synth")
    for name, heat, paf in _door_scenes(synth):
        cfg = capi.DecodeCfg(18, 8, 0.1, 32, 64)
        got = _run(capi, cuda, torch.from_numpy(heat).to(cuda), torch.from_numpy(paf).to(cuda), cfg, None, flags,
                   nms_only=True)
        _assert_parent_records(dec, gold_records, _gold_key("nms", flags, 32, 64, name), name, heat, paf, got, slice(0, 8))


# ---- 6. other skeletons against the restatement -----------------------------------------------------------------------
CAPS = [(4, 4), (32, 64), (65, 64), (111, 64), (128, 64), (32, 400)]
CASES = [(n, c) for n in sorted(sr.SCENE_SETS) for c in CAPS] + [("coco18rev", (4, 1))]


@pytest.mark.parametrize("name,caps", CASES, ids=["%s-%dx%d" % (n, c[0], c[1]) for n, c in CASES])
def test_other_skeletons_match_the_restatement(capi, dec, skm, cuda, name, caps):
    table, heat, paf, up = sr.scene_set(name)
    want, _ = sr.expected_block(name, *caps)
    skel = table.skeleton(skm).native()
    cfg = capi.DecodeCfg(table.P, up, 0.1, caps[0], caps[1])
    got = _run(capi, cuda, torch.tensor(heat, device=cuda), torch.tensor(paf, device=cuda), cfg, skel)
    assert got.shape == want.shape
    assert np.array_equal(got[:, :8], want[:, :8]), (got[:, :8], want[:, :8])       # counts, flags, capacities, P, L
    m = dec.result_mask(want)
    assert np.array_equal(got[m], want[m])
    for i in range(len(got)):                                                      # and as the consumer reads it
        d = dec.parse_image(got[i])
        assert d["num_parts"] == table.P and d["parts"].shape == (want[i, 1], table.P)


# ---- 7. NMS only -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nk", [("body25", 20), ("full32", 29)])
def test_nms_only_with_fewer_keypoints_than_parts(capi, dec, skm, cuda, name, nk):
    table, heat, paf, up = sr.scene_set(name)
    want, _ = sr.expected_block(name, 32, 64, nms_only=True, num_keypoints=nk)
    assert (want[:, 8 + nk:8 + table.P] == 0).all() and int(want[:, 8:8 + nk].sum()) > nk * len(want)
    cfg = capi.DecodeCfg(nk, up, 0.1, 32, 64)
    got = _run(capi, cuda, torch.tensor(heat, device=cuda), torch.tensor(paf, device=cuda), cfg,
               table.skeleton(skm).native(), nms_only=True)
    assert np.array_equal(got[:, :8], want[:, :8])
    m = dec.result_mask(want)
    assert np.array_equal(got[m], want[m])


# ---- 8. pipeline -----------------------------------------------------------------------------------------------------
def _openpose_body25(pkg):
    import openpose_restate as R
    op = importlib.import_module(pkg.__name__ + ".openpose")
    m = op.OpenPose_Model(4, 2, 52, 26)
    m.load_state_dict(R.seeded_state_dict(R.state_dict_spec(4, 2, 52, 26), 3))
    return m.cuda().eval(), 4, 368, 8, 2e-2, (3, 5)


def _hourglass_body25(pkg):
    import hourglass_restate as R
    hgm = importlib.import_module(pkg.__name__ + ".hourglass")
    m = hgm.hg(num_stacks=1, num_blocks=1, paf_classes=52, ht_classes=26)
    m.load_state_dict(R.seeded_state_dict(R.state_dict_spec(1, 1, 52, 26), 3, R.BRANCH_GAIN))
    return m.cuda().eval(), 2, 384, 4, 2e-3, (0, 1)


@pytest.mark.parametrize("make", [_openpose_body25, _hourglass_body25], ids=["openpose_4x368", "hourglass_2x384_stride4"])
def test_pose_estimator_with_body25(pkg, dec, skm, cuda, make):
    from oracle import post_oracle
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    m, B, S, stride, alpha, outs = make(pkg)
    table = sr.TABLES["body25"]
    cfg = dec.default_config(skm.BODY_25)
    cfg.MODEL.DOWNSAMPLE = stride

    def batch(r):
        g = torch.Generator().manual_seed(500 + r)
        h, p = sr.make_scenes(table, [3 + (r + i) % 3 for i in range(B)], S // stride, S // stride, stride, 600 + r)
        return (torch.rand(B, 3, S, S, generator=g) - 0.5).to(cuda), (torch.from_numpy(h).to(cuda), torch.from_numpy(p).to(cuda))

    data = [batch(r) for r in range(2)]
    est = pipeline.PoseEstimator(m, cfg, skeleton=skm.BODY_25)
    want = []
    for x, scene in data:
        est(x, scene, scene_alpha=alpha)                      # capacities settle
        bufs = est.enqueue(x, scene, scene_alpha=alpha)
        recs = dec.fetch(bufs).copy()
        assert bufs.map_hw == (S // stride, S // stride) and (recs[:, 5] == 25).all() and (recs[:, 6] == 26).all()
        # the maps the decoder read: the blended last PAF / heat maps, where the plan keeps them
        paf = m.read_output(bufs.plan, outs[0]).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        heat = m.read_output(bufs.plan, outs[1]).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        assert paf.shape[3] == 52 and heat.shape[3] == 26
        pcap, hcap = bufs.cfg.max_peaks_per_part, bufs.cfg.max_humans
        exp = []
        for i in range(B):
            jl, over = sr.truncate_peaks(post_oracle.nms(heat[i], num_keypoints=25, thr=0.1, up=stride), 25, pcap)
            exp.append(sr.pack_record(jl, sr.process(jl, paf[i], table, stride, hcap), table, pcap, hcap, over))
        exp = np.stack(exp)
        mask = dec.result_mask(exp)
        assert np.array_equal(recs[:, :8], exp[:, :8]) and np.array_equal(recs[mask], exp[mask])
        assert int(exp[:, 1].sum()) > B and not exp[:, 2].any()
        want.append(recs[mask].tobytes())
    order = [0, 1, 1, 0]
    prev, got = None, []

    def content(block):
        block = block.reshape(B, -1)
        return block[dec.result_mask(block)].tobytes()
    for r in order:
        t = est.submit(*data[r], scene_alpha=alpha)
        if prev is not None:
            got.append(content(est.collect(prev)[1]))
        prev = t
    got.append(content(est.collect(prev)[1]))
    torch.cuda.synchronize()
    for k, r in enumerate(order):
        assert got[k] == want[r], "step %d: the pipelined records differ from the serial path's" % k
    # Human objects with BODY_25 part ids and names
    humans = est.humans(data[0][0], scene=data[0][1], scene_alpha=alpha)
    ids = set(k for img in humans for h in img for k in h.body_parts)
    assert max(ids) > 18 and max(ids) <= 24 and sum(len(img) for img in humans) > B
    assert all(bp.get_part_name() == skm.BODY_25.part_names[k] for img in humans for h in img for k, bp in h.body_parts.items())
