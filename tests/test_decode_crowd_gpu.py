"""The decoder (csrc/decode.hip) on crowds, through both doors - the batched rtpose_decode_batch_ex and the legacy
process_paf (csrc/legacy_pafprocess.hip) - at capacities that launch every group_kernel instance and the four
limb_assign_kernel instances with 64-bit map offsets: more than 64 rows, connections and people, rows merged across
64-row chunks, score matrices and rows in the workspace, std::sort replayed on a workspace list, the max_humans doubling
of process_paf, and joint lists in caller order (a peak's id is not its position in peak_infos_line).

Everything is compared bit for bit - integers and float bit patterns - with the oracle (oracle/post_oracle.py), with the
compiled reference where oracle/_ref is at hand, and with tests/golden/legacy_order.npz (the reference's own output).
tests/test_decode_crowd_cpu.py proves on the CPU that each scene is what its case needs and which instance a case runs.
"""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crowd_scenes as cs  # noqa: E402
from conftest import PKG_NAME  # noqa: E402
from decode_run import run_decode  # noqa: E402
from oracle import make_golden_legacy_order as glo, post_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec(pkg):
    return importlib.import_module(PKG_NAME + ".decode")


@pytest.fixture(scope="module")
def pafprocess(pkg):
    return importlib.import_module(PKG_NAME + ".pafprocess")


@functools.lru_cache(maxsize=None)
def _oracle(name, up=1):
    """-> (joint list, result dict) of a scene of crowd_scenes.SCENES, computed once."""
    heat, paf = cs.scene(name)
    jl, r = po.paf_to_pose(heat, paf, 18, 0.1, up)
    for a in [jl] + [v for v in r.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return jl, r


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_record(dec, rec, jl, r, pcap, hcap):
    """One image's record against the oracle: header, peaks (ids, parts, truncated coordinates, score bits), humans."""
    assert list(rec[:5]) == [len(jl), len(r["parts"]), 0, pcap, hcap], list(rec[:8])
    d = dec.parse_image(rec)
    assert d["peaks"].shape == jl.shape
    assert np.array_equal(d["peaks"][:, [0, 1, 3, 4]], jl[:, [0, 1, 3, 4]])
    assert np.array_equal(_u32(d["peaks"][:, 2]), _u32(jl[:, 2])), "peak scores differ"
    assert np.array_equal(d["parts"], r["parts"]), "person assignments differ"
    assert np.array_equal(_u32(d["score"]), _u32(r["score"])), "human scores differ"


# ---- the batched door -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pcap,hcap,inst", cs.BATCHED_CASES,
                         ids=["%s-%dx%d" % c[:3] for c in cs.BATCHED_CASES])
def test_batched_door_on_crowds(capi, dec, cuda, name, pcap, hcap, inst):
    heat, paf = cs.scene(name)
    jl, r = _oracle(name)
    cfg = capi.DecodeCfg(18, 1, 0.1, pcap, hcap)
    got = run_decode(capi, cuda, torch.from_numpy(heat)[None].to(cuda), torch.from_numpy(paf)[None].to(cuda), cfg)
    _check_record(dec, got[0], jl, r, pcap, hcap)


@pytest.mark.parametrize("name,pcap,hcap,bit", cs.OVERFLOW_CASES, ids=["humans", "peaks"])
def test_batched_door_reports_overflow_and_stays_inside_its_buffers(capi, cuda, name, pcap, hcap, bit):
    heat, paf = cs.scene(name)
    cfg = capi.DecodeCfg(18, 1, 0.1, pcap, hcap)
    got = run_decode(capi, cuda, torch.from_numpy(heat)[None].to(cuda), torch.from_numpy(paf)[None].to(cuda), cfg)
    assert int(got[0, 2]) & bit, "header word 2 is %d" % int(got[0, 2])     # (run_decode checked the guard regions)


# ---- the legacy door --------------------------------------------------------------------------------------------------
def _as_call_shape(lst, shape):
    """The joint list as process_paf may be handed it: [1, n, 5]; [2, n/2, 5] (p1 > 1); [1, n, 6] (p3 > 5)."""
    if shape == "two_blocks":
        assert len(lst) % 2 == 0
        return lst.reshape(2, len(lst) // 2, 5)
    if shape == "six_columns":
        return np.concatenate([lst, np.full((len(lst), 1), 77.0, np.float32)], 1)[None]
    return lst[None]


def _check_getters(pafprocess, want, n_peaks, tag):
    nh = len(want["parts"])
    assert pafprocess.get_num_humans() == nh, tag
    got_parts = np.array([[pafprocess.get_part_cid(h, p) for p in range(18)] for h in range(nh)], np.int32).reshape(nh, 18)
    assert np.array_equal(got_parts, want["parts"]), tag
    got_score = np.array([pafprocess.get_score(h) for h in range(nh)], np.float32)
    assert np.array_equal(_u32(got_score), _u32(want["score"])), tag
    assert [pafprocess.get_part_x(c) for c in range(n_peaks)] == list(want["line_x"]), tag
    assert [pafprocess.get_part_y(c) for c in range(n_peaks)] == list(want["line_y"]), tag
    got_ls = np.array([pafprocess.get_part_score(c) for c in range(n_peaks)], np.float32)
    assert np.array_equal(_u32(got_ls), _u32(want["line_score"])), tag
    # bounds-checked getters behind the last human / peak
    assert pafprocess.get_part_cid(nh, 0) == -1 and pafprocess.get_part_x(n_peaks) == -1
    assert pafprocess.get_part_y(n_peaks) == -1 and np.isnan(pafprocess.get_score(nh))


def _legacy(pafprocess, name, order, shape="plain"):
    heat, paf = cs.scene(name)
    jl, _ = _oracle(name)
    lst = jl.copy() if order == "sorted" else cs.permuted(jl)
    assert pafprocess.process_paf(_as_call_shape(lst, shape), heat, paf) == 0
    _check_getters(pafprocess, po.process_paf(lst, paf, 1), len(lst), "oracle")
    if po.have_ref():
        _check_getters(pafprocess, po.ref_process_paf(lst, heat, paf), len(lst), "compiled reference")
    return lst


# every scene part-sorted and in caller order; one list handed over as [2, n/2, 5], one with a sixth column
SHAPES = {("crowd20", "permuted"): "two_blocks", ("crowd70", "sorted"): "six_columns"}
LEGACY = [(c[0], order, SHAPES.get((c[0], order), "plain")) for c in cs.LEGACY_CASES for order in ("sorted", "permuted")]


@pytest.mark.parametrize("name,order,shape", LEGACY, ids=["%s-%s-%s" % c for c in LEGACY])
def test_legacy_door_on_crowds(pafprocess, cuda, name, order, shape):
    _legacy(pafprocess, name, order, shape)


@pytest.mark.parametrize("name", glo.SCENES)
def test_legacy_door_equals_the_recorded_reference_on_caller_order_lists(pafprocess, cuda, name):
    z = np.load(glo.PATH)
    jl, heat, paf = glo.caller_order_list(name)
    assert str(z[name + "_digest"]) == glo.digest(jl, heat, paf), "not the scene the fixture was recorded on"
    assert pafprocess.process_paf(jl[None], heat, paf) == 0
    _check_getters(pafprocess, {k: z[name + "_" + k] for k in glo.FIELDS}, len(jl), "recorded reference")


def test_legacy_door_small_scene_after_the_largest(pafprocess, cuda):
    """The scratch process_paf grew for 300 people (512 humans, 300 peaks per part, rows and scores in the workspace) must
    not leak into the next, small, result."""
    _legacy(pafprocess, "crowd300", "permuted")
    _legacy(pafprocess, "crowd20", "permuted")
    _legacy(pafprocess, "crowd20", "sorted")


# ---- map offsets past 2^31 ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_maps(capi, cuda):
    """Two 20-person scenes: dense heat and PAF batches, and the same PAFs inside one 4 GiB buffer whose images are 2^31
    bytes apart (only the two h x w windows are written).  The buffer is freed when the module's tests are done."""
    scenes = [cs.crowd(*s[1:]) for s in cs.FAR_SCENES]
    heat = np.stack([s[0] for s in scenes])
    paf = np.stack([s[1] for s in scenes])
    cstride, choff, ws, hs, lead = cs.FAR_LAYOUT
    n, h, w, ch = paf.shape
    far = torch.empty((n, hs, ws, cstride), dtype=torch.float32, device=cuda)
    assert far.numel() * 4 == n << 31
    paf_d = torch.from_numpy(paf).to(cuda)
    far[:, :h, :w, choff:choff + ch] = paf_d
    torch.cuda.synchronize()
    yield heat, paf, torch.from_numpy(heat).to(cuda), paf_d, far, capi.Layout(cstride, choff, ws, hs, lead)
    del far
    torch.cuda.empty_cache()


@pytest.mark.parametrize("up,pcap,inst", cs.FAR_CASES, ids=["up%d-p%d" % c[:2] for c in cs.FAR_CASES])
def test_paf_image_starting_2_to_the_31_bytes_into_its_buffer(capi, dec, cuda, far_maps, up, pcap, inst):
    heat, paf, heat_d, paf_d, far, lfar = far_maps
    cfg = capi.DecodeCfg(18, up, 0.1, pcap, 64)
    dense = run_decode(capi, cuda, heat_d, paf_d, cfg)
    got = run_decode(capi, cuda, heat_d, far, cfg, lpaf=lfar)
    m = dec.result_mask(dense)
    assert np.array_equal(m, dec.result_mask(got)) and np.array_equal(got[m], dense[m]), "far and dense records differ"
    for i in range(len(heat)):
        jl, r = po.paf_to_pose(heat[i], paf[i], 18, 0.1, up)
        assert len(r["parts"]) == cs.FAR_SCENES[i][1]
        _check_record(dec, got[i], jl, r, pcap, 64)
