"""The table-driven decoder without a GPU: the host restatement (tests/skeleton_restate.py) against the C oracle, the
conditions its scene sets must meet for the GPU tests to mean something, skeleton validation and record / workspace sizes
through the C ABI, and PoseEstimator's channel check with and without a skeleton.

Two things the scenes could not be made to do, with the reasons:

* synth.make_batch scenes are NOT tie-free.  Two figures whose peaks of one part refine to the same pixel give candidates
  of exactly equal score whatever noise is on the maps; of the seeds 1..59 every 8-image batch at 368 x 368 had between 2
  and 8 images with such a tie (counted with post_oracle.process_paf's had_ties).  The restatement keeps raising on a tie
  (the GPU tests depend on that), so test 1 compares it with the oracle's libstdc++ order on every tie-free image of three
  batches, and its `ties="keep"` mode (equal scores stay in (a, b) order) with the oracle's sort mode of the same rule on
  all 24 images.  The restatement's own scene sets put the figures side by side and ARE tie-free, which is asserted.
* "both overflow flags at (4, 4)" cannot hold for two of the four tables.  The 2-part table can never emit a person (a
  person needs 4 parts) nor exceed max(64, 2 hcap) rows with the at most 4 connections its limb has at pcap 4.  COCO-18
  walked backwards with seed mask 0x15555 starts at most 10 limbs x 4 connections = 40 rows at pcap 4 (below the 64-row
  table), and no figure scene tried (seeds 1..80, up to 8 figures per image, whole figures and fragments) gave more than 4
  people from 4 peaks per part.  Their (4, 4) case must show the peak flag; the human flag of that table is exercised at
  (4, 1) instead, an extra case, where it must be set together with the peak flag.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skeleton_restate as sr  # noqa: E402


@pytest.fixture(scope="module")
def skm(pkg):
    return importlib.import_module(pkg.__name__ + ".skeleton")


@pytest.fixture(scope="module")
def synth(pkg):
    return importlib.import_module(pkg.__name__ + ".synth")


# ---- 1. the restatement against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [38, 49, 7])
def test_restatement_with_the_coco18_tables_equals_the_oracle(synth, seed):
    from oracle import post_oracle
    heat, paf, _ = synth.make_batch(8, 368, 368, seed=seed)
    table = sr.TABLES["coco18"]
    free = humans = 0
    for i in range(8):
        jl = post_oracle.nms(heat[i])
        ref = post_oracle.process_paf(jl, paf[i], 8)
        keep = post_oracle.process_paf(jl, paf[i], 8, libstdcxx_sort=False)
        got = sr.process(jl, paf[i], table, 8, ties="keep")
        assert np.array_equal(got["parts"], keep["parts"])
        assert np.array_equal(got["score"].view(np.uint32), keep["score"].view(np.uint32))
        if keep["had_ties"]:
            with pytest.raises(sr.TieError):
                sr.process(jl, paf[i], table, 8)
            continue
        got = sr.process(jl, paf[i], table, 8)
        assert np.array_equal(got["parts"], ref["parts"])
        assert np.array_equal(got["score"].view(np.uint32), ref["score"].view(np.uint32))
        free += 1
        humans += len(got["parts"])
    assert free >= 1 and humans >= 1       # the raising mode was compared on something


def test_the_generic_renderer_draws_what_synth_draws(synth):
    """skeleton_restate.render with the COCO-18 table = synth.render, bit for bit (same formulas, same noise draws)."""
    rng = np.random.default_rng(5)
    people = synth.random_people(rng, 4, 184, 200)
    h1, p1 = synth.render(people, 184, 200, rng=np.random.default_rng(9))
    h2, p2 = sr.render(sr.TABLES["coco18"], people, 184, 200, rng=np.random.default_rng(9))
    assert np.array_equal(h1, h2) and np.array_equal(p1, p2)


# ---- 2. conditions on the scene sets --------------------------------------------------------------------------------
# name -> (humans possible, flags the (4, 4) block must show, extra (pcap, hcap) case that must show both flags or None)
CONDITIONS = {"body25": (True, 3, None), "full32": (True, 3, None), "coco18rev": (True, 1, (4, 1)), "pair2": (False, 1, None)}


@pytest.mark.parametrize("name", sorted(sr.SCENE_SETS))
def test_scene_sets_have_something_to_get_wrong(name):
    """By the restatement alone (no device): no tie in any scene (sr.process would raise), more humans than images, row
    merges, refused seeds where the mask refuses some, no overflow at (32, 64), overflow at (4, 4)."""
    table, heat, paf, up = sr.scene_set(name)
    n = len(heat)
    assert n <= 4 and heat.shape[1:3] in ((46, 46), (23, 31)) and up in (8, 4, 6)
    assert heat.shape[3] == table.heat_channels and paf.shape[3] == table.paf_channels
    humans_possible, flags44, extra = CONDITIONS[name]
    blk, res = sr.expected_block(name, 32, 64)
    assert int(np.bitwise_or.reduce(blk[:, 2])) == 0
    assert int(blk[:, 0].sum()) > n and sum(r["connections"] for r in res) > n
    if humans_possible:
        assert int(blk[:, 1].sum()) > n
        assert sum(r["merges"] for r in res) >= 1
    else:
        assert table.P < 4 and int(blk[:, 1].sum()) == 0       # a person needs 4 parts
    if table.seed_mask != (1 << table.L) - 1:
        assert sum(r["refused_seeds"] for r in res) >= 1
    for caps in ((65, 64), (111, 64), (128, 64), (32, 400)):      # the other side of each launcher switch: same content
        b, _ = sr.expected_block(name, *caps)
        assert int(np.bitwise_or.reduce(b[:, 2])) == 0 and np.array_equal(b[:, :3], blk[:, :3])
    b44, _ = sr.expected_block(name, 4, 4)
    assert int(np.bitwise_or.reduce(b44[:, 2])) == flags44
    if extra:
        bx, _ = sr.expected_block(name, *extra)
        assert int(np.bitwise_or.reduce(bx[:, 2])) == 3


# ---- 3. validation and sizes ------------------------------------------------------------------------------------------
def _native(capi, P, limbs, seed_mask, struct_bytes=None):
    s = capi.SkeletonStruct()
    s.struct_bytes = C.sizeof(capi.SkeletonStruct) if struct_bytes is None else struct_bytes
    s.num_parts, s.num_limbs, s.seed_mask = P, len(limbs), seed_mask
    for i, (a, b, cx, cy) in enumerate(limbs[:32]):
        s.limb_part[i][0], s.limb_part[i][1], s.limb_paf[i][0], s.limb_paf[i][1] = a, b, cx, cy
    return s


GOOD = [(0, 1, 0, 1), (1, 2, 2, 3), (2, 3, 5, 4)]
BAD_TABLES = [      # (what, P, limbs, seed mask, heat channels, PAF channels, limb named by the message or None)
    ("part out of range", 4, [(0, 1, 0, 1), (1, 4, 2, 3)], 3, 5, 6, 1),
    ("negative part", 4, [(0, 1, 0, 1), (1, 2, 2, 3), (-1, 3, 4, 5)], 7, 5, 6, 2),
    ("channel out of range", 4, [(0, 1, 0, 1), (1, 2, 2, 6)], 3, 5, 6, 1),
    ("A == B", 4, [(2, 2, 0, 1)], 1, 5, 6, 0),
    ("the same limb twice", 4, [(0, 1, 0, 1), (1, 2, 2, 3), (0, 1, 4, 5)], 7, 5, 6, 2),
    ("x == y", 4, [(0, 1, 0, 1), (1, 2, 3, 3)], 3, 5, 6, 1),
    ("no parts", 0, [(0, 1, 0, 1)], 1, 5, 6, None),
    ("too many parts", 33, [(0, 1, 0, 1)], 1, 40, 6, None),
    ("no limbs", 4, [], 0, 5, 6, None),
    ("seed bit above the limbs", 4, GOOD, 0x8 | 1, 5, 6, None),
    ("more parts than heat-map channels", 4, GOOD, 7, 3, 6, None),
]


@pytest.mark.parametrize("case", BAD_TABLES, ids=[c[0] for c in BAD_TABLES])
def test_malformed_tables_are_refused_by_the_library_and_by_skeleton(capi, skm, case):
    what, P, limbs, mask, hc, pc, limb = case
    lib = capi.lib
    good = _native(capi, 4, GOOD, 7)
    assert lib.rtpose_skeleton_check(C.byref(good), 5, 6) == 0
    bad = _native(capi, P, limbs, mask)
    assert lib.rtpose_skeleton_check(C.byref(bad), hc, pc) != 0, what
    msg = capi.last_error()
    if limb is not None:
        assert "limb %d" % limb in msg, msg
    cfg = capi.DecodeCfg(1, 8, 0.1, 32, 64)
    if what not in ("channel out of range", "more parts than heat-map channels"):     # the maps are not known to these
        assert lib.rtpose_decode_result_bytes_skel(C.byref(cfg), C.byref(bad), 2) == 0
        assert lib.rtpose_decode_workspace_bytes_skel(C.byref(cfg), C.byref(bad), 2) == 0
        with pytest.raises(ValueError):
            skm.Skeleton.from_mask("bad", ["p%d" % i for i in range(P)], limbs, mask)


def test_more_refusals(capi, skm):
    lib = capi.lib
    assert lib.rtpose_skeleton_check(C.byref(_native(capi, 4, GOOD, 7, struct_bytes=64)), 5, 6) != 0
    assert "struct_bytes" in capi.last_error()
    assert lib.rtpose_skeleton_check(None, 5, 6) != 0
    with pytest.raises(ValueError):
        skm.Skeleton("bad", ["a", "b"], [(0, 1, 0, 1)], seed=[1])
    with pytest.raises(ValueError):
        skm.Skeleton("bad", ["p%d" % i for i in range(4)], [(i % 3, 3, 2 * i, 2 * i + 1) for i in range(33)])
    # a skeleton whose channels the maps do not have is refused by the library when native() checks it
    s = skm.Skeleton("wide", ["a", "b"], [(0, 1, 0, 70)])
    assert s.paf_channels == 71 and s.native().limb_paf[0][1] == 70
    # num_keypoints must lie inside the skeleton's parts
    sk = skm.BODY_25.native()
    assert lib.rtpose_decode_result_bytes_skel(C.byref(capi.DecodeCfg(26, 8, 0.1, 32, 64)), C.byref(sk), 1) == 0
    assert lib.rtpose_decode_result_bytes_skel(C.byref(capi.DecodeCfg(25, 8, 0.1, 32, 64)), C.byref(sk), 1) > 0
    assert lib.rtpose_decode_result_bytes_skel(C.byref(capi.DecodeCfg(19, 8, 0.1, 32, 64)),
                                               C.byref(skm.COCO18.native()), 1) == 0


def test_presets_round_trip_through_the_ctypes_mirror(capi, skm):
    lib = capi.lib
    for fill, sk, P, L, pafc, heatc, mask in ((lib.rtpose_skeleton_coco18, skm.COCO18, 18, 19, 38, 19, 0x3FFFF),
                                              (lib.rtpose_skeleton_body25, skm.BODY_25, 25, 26, 52, 26, (1 << 26) - 1)):
        s = capi.SkeletonStruct()
        assert fill(C.byref(s)) == 0
        mine = sk.native()
        assert bytes(s) == bytes(mine) and s.struct_bytes == C.sizeof(capi.SkeletonStruct) == 528
        assert (s.num_parts, s.num_limbs, s.seed_mask) == (P, L, mask)
        assert (sk.num_parts, sk.num_limbs, sk.paf_channels, sk.heat_channels) == (P, L, pafc, heatc)
        assert lib.rtpose_skeleton_check(C.byref(s), heatc, pafc) == 0
        assert lib.rtpose_skeleton_check(C.byref(s), heatc, pafc - 1) != 0
        assert [tuple(l) for l in sk.limbs] == [(s.limb_part[i][0], s.limb_part[i][1], s.limb_paf[i][0], s.limb_paf[i][1])
                                                for i in range(L)]
        # every PAF channel is read by exactly one limb
        assert sorted(c for l in sk.limbs for c in l[2:]) == list(range(pafc))
    assert [tuple(l) for l in skm.COCO18.limbs] == sr.COCO18_LIMBS and [tuple(l) for l in skm.BODY_25.limbs] == sr.BODY25_LIMBS
    assert "NOT VERIFIED" in skm.BODY_25.__doc__
    for t in sr.TABLES.values():                      # the test tables are valid skeletons with the channel counts said
        s = t.skeleton(skm)
        assert (s.paf_channels, s.heat_channels, s.seed_mask) == (t.paf_channels, t.heat_channels, t.seed_mask)
        s.native()


def test_sizes_with_the_coco18_preset_equal_the_old_ones_and_grow_with_the_table(capi, skm):
    lib = capi.lib
    coco = skm.COCO18.native()
    tables = [sr.TABLES[k].skeleton(skm).native() for k in ("pair2", "coco18", "body25", "full32")]
    for pcap in (4, 32, 111, 128):
        for hcap in (4, 64, 400):
            cfg = capi.DecodeCfg(1, 8, 0.1, pcap, hcap)
            for n in (1, 3):
                assert (lib.rtpose_decode_result_bytes_skel(C.byref(cfg), C.byref(coco), n)
                        == lib.rtpose_decode_result_bytes(C.byref(cfg), n) > 0)
                assert (lib.rtpose_decode_workspace_bytes_skel(C.byref(cfg), C.byref(coco), n)
                        == lib.rtpose_decode_workspace_bytes(C.byref(cfg), n) > 0)
            rb = [lib.rtpose_decode_result_bytes_skel(C.byref(cfg), C.byref(t), 2) for t in tables]
            ws = [lib.rtpose_decode_workspace_bytes_skel(C.byref(cfg), C.byref(t), 2) for t in tables]
            assert rb == sorted(rb) and len(set(rb)) == 4 and ws == sorted(ws) and len(set(ws)) == 4
            for t, b in zip(tables, rb):
                assert b == 2 * 4 * sr.result_words(t.num_parts, pcap, hcap)
    # the record layout rule: any P up to 24 keeps the peaks at word 32, 25 parts move them to 36, 32 parts to 40
    assert [sr.peaks_word(p) for p in (1, 18, 24, 25, 28, 29, 32)] == [32, 32, 32, 36, 36, 40, 40]
    # workspace sections, in bytes, for the 32-part table at the capacities where the launcher switches
    t32 = tables[3]
    conn = lambda pcap, n: -(-n * 32 * (1 + 3 * pcap) * 4 // 256) * 256      # noqa: E731

    def ws(pcap, hcap, n=2):
        return lib.rtpose_decode_workspace_bytes_skel(C.byref(capi.DecodeCfg(1, 8, 0.1, pcap, hcap)), C.byref(t32), n)
    assert ws(32, 64) == conn(32, 2)                                                   # everything else in LDS
    assert ws(65, 64) == conn(65, 2) + 2 * 32 * 65 * 65 * 8                            # tie lists past 4096 candidates
    assert ws(111, 64) == conn(111, 2) + 2 * 32 * 111 * 111 * 4 + 2 * 32 * 111 * 111 * 8    # + scores past 110 x 110
    assert ws(32, 400) == conn(32, 2) + 2 * 800 * 35 * 4                               # 800 rows of 35 floats > 60480 bytes
    assert ws(32, 216) == conn(32, 2) and ws(32, 217) > conn(32, 2)                    # 432 x 35 x 4 = 60480 bytes: the last fit


def test_parse_image_and_result_mask_read_the_part_count_from_the_record(pkg):
    dec = importlib.import_module(pkg.__name__ + ".decode")
    blk, res = sr.expected_block("body25", 32, 64)
    assert dec.peaks_word(25) == sr.peaks_word(25) == 36
    m = dec.result_mask(blk)
    for i, r in enumerate(res):
        d = dec.parse_image(blk[i])
        assert d["num_parts"] == 25 and np.array_equal(d["parts"], r["parts"])
        assert np.array_equal(d["score"].view(np.uint32), r["score"].view(np.uint32))
        assert len(d["peaks"]) == blk[i, 0] and m[i].sum() == 5 + 25 + 4 * blk[i, 0] + 26 * blk[i, 1]
    assert not m[:, 5:8].any() and np.array_equal(np.flatnonzero(blk[0] * ~m[0]), [5, 6])    # only P and L outside the mask
    names = importlib.import_module(pkg.__name__ + ".skeleton").BODY_25
    humans = dec.humans_from_record(dec.parse_image(blk[0]), 368, 368, skeleton=names)
    assert len(humans) == blk[0, 1] and max(max(h.body_parts) for h in humans) > 18
    assert all(bp.get_part_name() == names.part_names[k] for h in humans for k, bp in h.body_parts.items())
    img = importlib.import_module(pkg.__name__ + ".common").draw_humans(np.zeros((64, 64, 3), np.uint8), humans, skeleton=names)
    assert img.any()


# ---- 4. PoseEstimator with and without a skeleton --------------------------------------------------------------------
def test_pose_estimator_checks_the_models_channels_against_the_skeleton(pkg, skm):
    op = importlib.import_module(pkg.__name__ + ".openpose")
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    small = skm.Skeleton("small", ["p%d" % i for i in range(8)], [(i, i + 1, 2 * i, 2 * i + 1) for i in range(7)])
    assert (small.paf_channels, small.heat_channels) == (14, 9)
    est = pipeline.PoseEstimator(op.OpenPose_Model(), skeleton=small)
    assert est.config.MODEL.NUM_KEYPOINTS == 8 and (est.paf_channels, est.heat_channels) == (14, 9)
    est = pipeline.PoseEstimator(op.OpenPose_Model(4, 2, 52, 26), skeleton=skm.BODY_25)
    assert est.config.MODEL.NUM_KEYPOINTS == 25
    with pytest.raises(ValueError) as e:
        pipeline.PoseEstimator(op.OpenPose_Model(4, 2, 38, 19), skeleton=skm.BODY_25)
    assert "52 PAF / 26 heat-map" in str(e.value) and "38 / 19" in str(e.value)
    # without a skeleton: as before
    with pytest.raises(ValueError) as e:
        pipeline.PoseEstimator(op.OpenPose_Model())
    assert "COCO-18" in str(e.value) and "14 / 9" in str(e.value)
    est = pipeline.PoseEstimator(op.OpenPose_Model(4, 2, 38, 19))
    assert est.skeleton is None and est.config.MODEL.NUM_KEYPOINTS == 18
    pipeline.PoseEstimator(op.OpenPose_Model(4, 2, 38, 19), skeleton=skm.COCO18)
