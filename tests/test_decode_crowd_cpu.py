"""The scenes and cases of tests/test_decode_crowd_gpu.py, checked without a GPU: every scene is what its GPU case needs
(through the oracle alone), and the cases together reach every group_kernel instance and the four limb_assign_kernel
instances with 64-bit map offsets (through tests/crowd_scenes.py's restatement of assign_group_launch's switches, whose
constants are read out of csrc/).  Where the compiled reference is at hand the oracle is pinned to it on the caller-order
joint lists and on the tied field."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crowd_scenes as cs  # noqa: E402
from conftest import PKG_NAME  # noqa: E402
from oracle import post_oracle as po  # noqa: E402

CROWDS = [n for n in cs.SCENES if cs.SCENES[n][0] == "crowd"]
KEYS = ("parts", "score", "line_x", "line_y", "line_score")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, keys=KEYS):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _had_ties(jl, paf):
    """(the oracle reports equal candidate scores of a limb only in its stable mode)"""
    return po.process_paf(jl, paf, 1, libstdcxx_sort=False)["had_ties"]


def test_constants_are_read_from_the_sources():
    k = cs.launcher_constants()
    assert set(k) == {"kLdsPairs", "kLdsRowBytes", "kTieLdsCands", "kStageWords", "stage_budget"}
    assert all(isinstance(v, int) and v > 0 for v in k.values())
    assert cs._int_expr("720 * 21 * (int)sizeof(float)") == 720 * 21 * 4 and cs._int_expr("96 * 1024") == 98304
    with pytest.raises(AssertionError):
        cs._int_expr("kOther + 1")


@pytest.mark.parametrize("name", CROWDS)
def test_crowd_scene_is_what_its_cases_need(name):
    _, persons, junk = cs.SCENES[name]
    heat, paf = cs.scene(name)
    want = cs.crowd_counts(persons, junk)
    jl, r = po.paf_to_pose(heat, paf, 18, 0.1, 1)
    assert np.array_equal(np.bincount(jl[:, 4].astype(int), minlength=18), want["per_part"])
    assert np.array_equal(jl, cs.part_sorted(jl)), "the oracle's NMS list is part-sorted with running ids"
    parts = r["parts"]
    assert len(parts) == want["humans"] and ((parts >= 0).sum(1) == 4).all()
    type_a = (parts[:, [1, 2, 3, 4]] >= 0).all(1)
    type_b = (parts[:, [1, 2, 14, 16]] >= 0).all(1)                 # two rows, merged by limb (2, 16)
    assert int(type_b.sum()) == want["merged"] and int(type_a.sum()) == want["humans"] - want["merged"]
    # a type-B person seeds twice - limbs (1, 2) and (14, 16) may both seed and both come before (2, 16), which joins them
    limbs = [l[:2] for l in importlib.import_module(PKG_NAME + ".skeleton").COCO18.limbs]
    assert limbs.index((1, 2)) < limbs.index((14, 16)) < limbs.index((2, 16)) < 18
    assert int(type_a.sum()) + 2 * int(type_b.sum()) == want["seeded_rows"]
    assert not _had_ties(jl, paf)
    # caller order: ids differ from positions in peak_infos_line, and the human scores show it
    jp = cs.permuted(jl)
    assert not np.array_equal(jp[:, 4], jl[:, 4])
    rp = po.process_paf(jp, paf, 1)
    assert not _had_ties(jp, paf) and len(rp["parts"]) == want["humans"]
    assert not np.array_equal(np.sort(rp["score"]), np.sort(r["score"]))


def test_crowd_decodes_at_other_upsampling_factors():
    for kind, persons, junk, seed in cs.FAR_SCENES:
        heat, paf = cs.crowd(persons, junk, seed)
        for up in (1, 3, 8):
            jl, r = po.paf_to_pose(heat, paf, 18, 0.1, up)
            assert len(r["parts"]) == persons and ((r["parts"] >= 0).sum(1) == 4).all(), (seed, up)
            assert max(np.bincount(jl[:, 4].astype(int))) <= min(c[1] for c in cs.FAR_CASES)
    a, b = (cs.crowd(*s[1:]) for s in cs.FAR_SCENES)
    assert a[0].shape == b[0].shape and not np.array_equal(a[1], b[1])


def _limb0_candidates(jl, paf):
    """Candidates of limb (1, 2) - PAF channels 12 / 13 - at upsample 1, restated in numpy.  Good for scenes whose sample
    scores lie far from the 0.05 threshold (the tied field: every sample scores dx / norm >= 0.28)."""
    A, B = jl[jl[:, 4] == 1][:, :2].astype(int), jl[jl[:, 4] == 2][:, :2].astype(int)
    n = 0
    for a in A:
        d = (B - a).astype(np.float64)
        norm = np.sqrt((d ** 2).sum(1))
        ok = norm > 0
        t = np.arange(10)[None, :, None] / 10.0
        pts = np.floor(a[None, None, :] + t * d[:, None, :] + 0.5).astype(int)
        px = paf[pts[..., 1], pts[..., 0], 12]
        py = paf[pts[..., 1], pts[..., 0], 13]
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (d[:, None, 0] * px + d[:, None, 1] * py) / norm[:, None]
        assert (2 * norm <= paf.shape[0]).all()                    # no length penalty
        n += int((ok & ((s > 0.05).sum(1) > 6) & (s.sum(1) > 0)).sum())
    return n


def test_tied_field_is_what_its_cases_need():
    _, K, _ = cs.SCENES["tied65"]
    heat, paf = cs.scene("tied65")
    jl, r = po.paf_to_pose(heat, paf, 18, 0.1, 1)
    cnt = np.bincount(jl[:, 4].astype(int), minlength=18)
    assert (cnt[1:5] == K).all() and cnt.sum() == 4 * K
    ncand = _limb0_candidates(jl, paf)
    assert ncand == K * K and cs.tie_list_in_workspace(ncand) and not cs.tie_list_in_workspace(64 * 64)
    assert cs.instance(K, 64)["tie_ws_reserved"] and cs.instance(K, 64)["scores_in_lds"]
    assert _had_ties(jl, paf)
    stable = po.process_paf(jl, paf, 1, libstdcxx_sort=False)
    assert len(r["parts"]) > 0 and ((r["parts"] >= 0).sum(1) == 4).all()
    assert not _same(stable, r, ("parts", "score")), "std::sort's order must give other people than the stable order"
    jp = cs.permuted(jl)
    assert not np.array_equal(np.sort(po.process_paf(jp, paf, 1)["score"]), np.sort(r["score"]))


def test_overflow_cases_overflow():
    for name, pcap, hcap, bit in cs.OVERFLOW_CASES:
        _, persons, junk = cs.SCENES[name]
        want = cs.crowd_counts(persons, junk)
        if bit == 1:
            assert want["per_part"].max() > pcap and hcap >= want["humans"] and cs.row_cap(hcap) >= want["seeded_rows"]
        else:
            assert want["per_part"].max() <= pcap and (want["humans"] > hcap or want["seeded_rows"] > cs.row_cap(hcap))


def _rows_and_humans(name):
    kind, n, junk = cs.SCENES[name]
    if kind == "crowd":
        c = cs.crowd_counts(n, junk)
        return int(c["per_part"].max()), c["seeded_rows"], c["humans"]
    heat, paf = cs.scene(name)
    jl, r = po.paf_to_pose(heat, paf, 18, 0.1, 1)
    return n, n, len(r["parts"])          # at most one row per connection of limb (1, 2): min(K, K)


def test_cases_reach_every_grouping_instance():
    reached = {}
    for name, pcap, hcap, inst in cs.BATCHED_CASES:
        peaks, rows, humans = _rows_and_humans(name)
        assert peaks <= pcap and rows <= cs.row_cap(hcap) and humans <= hcap, name      # nothing overflows
        assert cs.group_instance(True, pcap, hcap) == inst, (name, cs.group_instance(True, pcap, hcap))
        reached.setdefault(inst, []).append(name)
    assert not cs.instance(20 + cs.JUNK, 64)["scores_in_lds"] and not cs.instance(300, 512)["scores_in_lds"]
    assert cs.instance(128, 128)["scores_in_lds"] is False and cs.crowd_counts(70)["seeded_rows"] > 64
    finals = set()
    for name, passes, inst in cs.LEGACY_CASES:
        peaks, rows, humans = _rows_and_humans(name)
        got = cs.legacy_schedule(peaks, rows, humans)                # process_paf sizes its tables to the fullest part
        assert got == (passes, inst), (name, got)
        reached.setdefault(inst, []).append(name)
        finals.add(inst)
    every = set(itertools.product((True, False), repeat=3))
    assert set(reached) == every, "group_kernel instances never launched: %s" % sorted(every - set(reached))
    assert finals == {i for i in every if not i[0]}, "each process_paf instance must be the last pass of a case"
    # the thresholds the issue names for COCO-18: STAGE_ALL up to 230 peaks with the rows in LDS, up to 258 without
    assert cs.group_instance(True, 230, 64)[1] and not cs.group_instance(True, 231, 64)[1]
    assert cs.group_instance(True, 258, 512)[1:] == (True, False) and not cs.group_instance(True, 259, 512)[1]


def test_far_cases_reach_every_limb_assign_instance_with_64_bit_offsets():
    cstride, choff, ws, hs, lead = cs.FAR_LAYOUT
    assert hs * ws * cstride * 4 == 1 << 31 and lead == 0 and choff + cs.PAF_CHANNELS <= cstride
    heat, _ = cs.crowd(*cs.FAR_SCENES[0][1:])
    assert heat.shape[0] <= hs and heat.shape[1] <= ws
    got = {cs.limb_instance(pcap, up, cstride, ws, hs) for up, pcap, _ in cs.FAR_CASES}
    assert [cs.limb_instance(pcap, up, cstride, ws, hs) for up, pcap, _ in cs.FAR_CASES] == [c[2] for c in cs.FAR_CASES]
    assert got == {(a, b, False) for a in (True, False) for b in (True, False)}
    assert cs.limb_instance(32, 1, cstride, ws, hs - 1)[2], "one row less and the offsets fit 31 bits"


@pytest.mark.parametrize("name", sorted(cs.SCENES))
def test_oracle_equals_the_compiled_reference_on_caller_order_lists(name):
    if not po.have_ref():
        pytest.skip("oracle/_ref/libpafprocess_ref.so not built (needs the reference sources)")
    heat, paf = cs.scene(name)
    jl = po.nms(heat, 18, 0.1, 1)
    for lst in (jl, cs.permuted(jl)):
        assert _same(po.process_paf(lst, paf, 1), po.ref_process_paf(lst, heat, paf))
