"""Crowd scenes for the decoder's grouping kernels, and a restatement of the switches of assign_group_launch
(csrc/decode.hip) that pick the kernel instance.  numpy only: tests/test_decode_crowd_cpu.py proves on the CPU that every
scene is what its GPU case in tests/test_decode_crowd_gpu.py needs, and that the cases reach the instances they name.

Scenes are full-resolution COCO-18 maps (heat HWC 19 channels, PAF HWC 38 channels) meant for upsample = 1.

The launcher's constants are READ out of the C++ sources with regular expressions, never copied: a changed constant moves
a case onto another instance, and then the coverage assertion of the CPU test fails instead of the case quietly running
a kernel that is covered already.
"""
import math
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "pytorch_realtime_multi-person_pose_estimation_amd", "csrc")
CELL = 16

# ---- scenes -----------------------------------------------------------------------------------------------------------
# (part at x offset 1, 5, 9, 13), [(part A, part B, PAF x channel, sign)]: CocoPairs / CocoPairsNetwork of decode.hip
TYPE_A = ((1, 2, 3, 4), ((1, 2, 12, 1.0), (2, 3, 14, 1.0), (3, 4, 16, 1.0)))
TYPE_B = ((1, 2, 16, 14), ((1, 2, 12, 1.0), (2, 16, 18, 1.0), (14, 16, 34, -1.0)))
JOINT_X = (1, 5, 9, 13)
JUNK_ROWS = (1, 3, 13)      # rows of a cell no person reaches (persons sit on rows 6 .. 10): at least 3 rows away


def crowd(persons, junk, seed):
    """`persons` four-joint stick figures, one per 16 x 16 cell on a ceil(sqrt(persons))-wide grid, every one a human of
    4 parts.  Even persons are type A (parts 1, 2, 3, 4: one subset row), odd ones type B (parts 1, 2, 16, 14; the ear
    lies left of the eye, so limb (14, 16) points -x): limb 0 seeds the row {1, 2}, limb 14 the row {14, 16}, and limb 17
    (2, 16) merges the two - rows seeded persons/2 .. 3 persons/2 apart, in different 64-row chunks of the row search once
    the crowd is large.  `junk` further single-pixel peaks of part 2, two pixels apart on rows without PAF (no candidate
    reaches crit1 > 6 from there: a segment to a row 3 away leaves the person's row after two samples).
    -> heat [H, W, 19], paf [H, W, 38] float32."""
    rng = np.random.default_rng(seed)
    cols = int(math.ceil(math.sqrt(persons)))
    rows = (persons + cols - 1) // cols
    H, W = rows * CELL, cols * CELL
    heat = np.zeros((H, W, 19), np.float32)
    paf = np.zeros((H, W, 38), np.float32)
    for k in range(persons):
        cy, cx = (k // cols) * CELL, (k % cols) * CELL
        y = cy + 8 + int(rng.integers(-2, 3))
        parts, limbs = TYPE_B if k % 2 else TYPE_A
        for part, dx in zip(parts, JOINT_X):
            heat[y, cx + dx, part] = rng.uniform(0.3, 1.0)
        mag = np.float32(rng.uniform(0.55, 1.0))
        where = dict(zip(parts, JOINT_X))
        for a, b, ch, sign in limbs:
            x0, x1 = sorted((where[a], where[b]))
            paf[y, cx + x0:cx + x1 + 1, ch] = sign * mag
    placed = 0
    for cy in range(0, H, CELL):
        for dy in JUNK_ROWS:
            for x in range(0, W, 2):
                if placed < junk:
                    heat[cy + dy, x, 2] = rng.uniform(0.3, 1.0)
                    placed += 1
    assert placed == junk, "crowd: the map has room for %d junk peaks, not %d" % (placed, junk)
    return heat, paf


def crowd_counts(persons, junk=0):
    """What crowd(persons, junk, .) must decode to: peaks per part, humans, merged type-B humans, seeded rows."""
    b = persons // 2
    a = persons - b
    per_part = np.zeros(18, np.int64)
    per_part[[1, 2]] = persons
    per_part[[3, 4]] = a
    per_part[[14, 16]] = b
    per_part[2] += junk
    return {"per_part": per_part, "humans": persons, "merged": b, "seeded_rows": a + 2 * b}


def tied_field(K, seed=1):
    """K necks at x = 2 and K right shoulders at x = 40 on rows 2 + 2i over a PAF that is 1 on channel 12 for x <= 40
    everywhere: every (neck, shoulder) pair is a candidate of limb (1, 2) - K * K of them - and pairs with the same
    |row difference| score exactly the same.  Each shoulder goes on into private (2, 3) and (3, 4) limbs to x = 46 and
    52.  The map is 2K + 240 rows high so that no limb is longer than half of it (no length penalty).
    -> heat [2K + 240, 64, 19], paf [2K + 240, 64, 38] float32."""
    rng = np.random.default_rng(seed)
    H, W = 2 * K + 240, 64
    heat = np.zeros((H, W, 19), np.float32)
    paf = np.zeros((H, W, 38), np.float32)
    paf[:, :41, 12] = 1.0
    for i in range(K):
        y = 2 + 2 * i
        for part, x in ((1, 2), (2, 40), (3, 46), (4, 52)):
            heat[y, x, part] = rng.uniform(0.3, 1.0)
        paf[y, 40:47, 14] = np.float32(rng.uniform(0.6, 1.0))
        paf[y, 46:53, 16] = np.float32(rng.uniform(0.6, 1.0))
    return heat, paf


def permuted(jl, seed=0):
    """The joint list in a random caller order, ids renumbered in arrival order (what pafprocess.cpp:24-43 assigns): a
    peak's id is then no longer its position in the part-major peak_infos_line."""
    out = np.ascontiguousarray(jl[np.random.default_rng(seed).permutation(len(jl))], dtype=np.float32)
    out[:, 3] = np.arange(len(out), dtype=np.float32)
    return out


def part_sorted(jl):
    """The joint list sorted by part (stable), ids renumbered: id == position in peak_infos_line."""
    out = np.ascontiguousarray(jl[np.argsort(jl[:, 4], kind="stable")], dtype=np.float32)
    out[:, 3] = np.arange(len(out), dtype=np.float32)
    return out


# ---- the launcher's switches ------------------------------------------------------------------------------------------
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int_expr(text):
    """'110 * 110', '720 * 21 * (int)sizeof(float)', '96 * 1024' -> int; anything else is an error."""
    text = re.sub(r"\(\s*int\s*\)\s*sizeof\s*\(\s*float\s*\)|sizeof\s*\(\s*float\s*\)", "4", text)
    factors = [f.strip() for f in text.split("*")]
    assert factors and all(re.fullmatch(r"\d+", f) for f in factors), "not a product of integers: %r" % text
    return int(np.prod([int(f) for f in factors], dtype=np.int64))


def _constant(source, pattern):
    m = re.findall(pattern, _read(source))
    assert len(m) == 1, "%s: %d matches for %r" % (source, len(m), pattern)
    return _int_expr(m[0])


def launcher_constants():
    return {
        "kLdsPairs": _constant("decode.h", r"constexpr\s+int\s+kLdsPairs\s*=\s*([^;]+);"),
        "kLdsRowBytes": _constant("decode.h", r"constexpr\s+int\s+kLdsRowBytes\s*=\s*([^;]+);"),
        "kTieLdsCands": _constant("decode.h", r"constexpr\s+int\s+kTieLdsCands\s*=\s*([^;]+);"),
        "kStageWords": _constant("decode_dev.h", r"constexpr\s+int\s+kStageWords\s*=\s*([^;]+);"),
        "stage_budget": _constant("decode.hip", r"stage_all\s*=\s*rows_bytes\s*\+\s*all_bytes\s*<=\s*([^;]+);"),
    }


def row_cap(hcap):
    return max(2 * hcap, 64)                                    # decode_row_cap


def instance(pcap, hcap, P=18, L=19):
    """The switches assign_group_launch takes on (max_peaks_per_part, max_humans) for a skeleton of P parts and L limbs."""
    k = launcher_constants()
    scores_in_lds = pcap * pcap * 4 <= k["kLdsPairs"] * 4       # decode_scores_in_lds
    rows_bytes = row_cap(hcap) * (P + 3) * 4                    # decode_rows_bytes
    rows_in_lds = rows_bytes <= k["kLdsRowBytes"]               # decode_rows_in_lds
    all_bytes = L * pcap * k["kStageWords"] * 4
    stage_all = (rows_bytes if rows_in_lds else 0) + all_bytes <= k["stage_budget"]
    return {"scores_in_lds": scores_in_lds, "stage_all": stage_all, "rows_in_lds": rows_in_lds,
            "tie_ws_reserved": pcap * pcap > k["kTieLdsCands"]}  # decode_ws_tie_bytes


def tie_list_in_workspace(candidates):
    """Whether a tied limb with this many candidates replays std::sort on the workspace list (else in LDS)."""
    return candidates > launcher_constants()["kTieLdsCands"]


def group_instance(write_ids, pcap, hcap, P=18, L=19):
    """group_kernel<WRITE_IDS, STAGE_ALL, ROWS_IN_LDS> as a tuple of bools."""
    i = instance(pcap, hcap, P, L)
    return (bool(write_ids), i["stage_all"], i["rows_in_lds"])


def limb_instance(pcap, up, cstride, ws, hs):
    """limb_assign_kernel<SCORES_IN_LDS, UP_POW2, A32> for a PAF view of that layout."""
    a32 = hs * ws < (1 << 24) and cstride * 4 < (1 << 24) and hs * ws * cstride * 4 < (1 << 31)
    return (instance(pcap, 64)["scores_in_lds"], up in (1, 2, 4, 8, 16, 32, 64, 128), a32)


def legacy_schedule(pcap, seeded_rows, humans):
    """process_paf (csrc/legacy_pafprocess.hip): max_humans starts at 64 and doubles while a pass reports
    kOverflowHumans - more rows seeded than 2 * max_humans (64 at least), or more humans than max_humans.
    -> ([max_humans of every pass], group_kernel instance of the last pass)."""
    hcap, passes = 64, [64]
    while seeded_rows > row_cap(hcap) or humans > hcap:
        assert hcap < 16384, "process_paf refuses with RTPOSE_E_CAPACITY here"
        hcap *= 2
        passes.append(hcap)
    return passes, group_instance(False, pcap, hcap)


# ---- the cases of tests/test_decode_crowd_gpu.py (tests/test_decode_crowd_cpu.py proves what is said about them) -------
JUNK = 215                                                       # crowd(20, JUNK, 1): 235 peaks of part 2, above 230
PAF_CHANNELS = 38
SCENES = {
    "crowd20": ("crowd", 20, 0), "crowd20junk": ("crowd", 20, JUNK), "crowd70": ("crowd", 70, 0),
    "crowd257": ("crowd", 257, 0), "crowd300": ("crowd", 300, 0), "tied65": ("tied", 65, 0),
}
_cache = {}


def scene(name):
    """-> (heat, paf) of SCENES[name], read-only, built once."""
    if name not in _cache:
        kind, n, junk = SCENES[name]
        heat, paf = crowd(n, junk, 1) if kind == "crowd" else tied_field(n)
        heat.setflags(write=False)
        paf.setflags(write=False)
        _cache[name] = (heat, paf)
    return _cache[name]


# batched door: (scene, max_peaks_per_part, max_humans, group_kernel<WRITE_IDS, STAGE_ALL, ROWS_IN_LDS>)
BATCHED_CASES = [
    ("crowd20junk", 20 + JUNK, 64, (True, False, True)),          # and the score matrices in the workspace
    ("crowd257", 258, 512, (True, True, False)),                  # 385 rows
    ("crowd300", 300, 512, (True, False, False)),                 # 450 rows, 300 x 300 score matrices in the workspace
    ("crowd70", 128, 128, (True, True, True)),                    # past 64 rows
    ("tied65", 65, 64, (True, True, True)),                       # std::sort replayed on the workspace list
]
# (scene, max_peaks_per_part, max_humans, bit of header word 2 that must be set)
OVERFLOW_CASES = [("crowd300", 300, 64, 2), ("crowd300", 256, 512, 1)]
# legacy door: (scene, the max_humans of every pass, group_kernel instance of the last pass)
LEGACY_CASES = [
    ("crowd20", [64], (False, True, True)),
    ("crowd70", [64, 128], (False, True, True)),
    ("crowd20junk", [64], (False, False, True)),
    ("crowd257", [64, 128, 256, 512], (False, True, False)),
    ("crowd300", [64, 128, 256, 512], (False, False, False)),
    ("tied65", [64], (False, True, True)),
]
# a PAF view whose image spans exactly 2^31 bytes: (cstride, choff, ws, hs, lead); image 1 starts 2^31 bytes in
FAR_LAYOUT = (64, 8, 2048, 4096, 0)
# (upsample, max_peaks_per_part, limb_assign_kernel<SCORES_IN_LDS, UP_POW2, A32>)
FAR_CASES = [(1, 32, (True, True, False)), (3, 32, (True, False, False)), (1, 128, (False, True, False)),
             (3, 128, (False, False, False))]
FAR_SCENES = [("crowd", 20, 0, 1), ("crowd", 20, 0, 2)]          # crowd(20, 0, 1) and crowd(20, 0, 2): same map size
