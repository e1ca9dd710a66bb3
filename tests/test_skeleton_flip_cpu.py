"""CPU suite: the flip tables a skeleton gives (skeleton.Skeleton.flip_tables, rtpose_flip_table_from_skeleton) and the
host-side check of a hand-filled table (rtpose_flip_table_check).  No GPU: the library's table functions are host only.

The COCO-18 tables are compared with the reference's own constants (SWAP_HEAT / SWAP_PAF as tests/layout_restate.py
carries them); BODY_25's heat map with the list written out in tests/tta_skel_restate.py; a 3-part table exercises the
limb whose mirror exists only walked backwards.
"""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_restate as lr  # noqa: E402
import tta_skel_restate as tr  # noqa: E402

from conftest import ROOT  # noqa: E402


@pytest.fixture(scope="module")
def skm(pkg):
    return importlib.import_module(pkg.__name__ + ".skeleton")


def _twice_is_identity(heat_src, paf_src, paf_sign):
    return (all(heat_src[heat_src[c]] == c for c in range(len(heat_src)))
            and all(paf_src[paf_src[c]] == c and paf_sign[c] * paf_sign[paf_src[c]] == 1 for c in range(len(paf_src))))


def test_coco18_tables_are_the_reference_constants(skm):
    heat_src, paf_src, paf_sign = skm.COCO18.flip_tables()
    assert heat_src == list(lr.SWAP_HEAT) and len(heat_src) == skm.COCO18.heat_channels == 19
    assert paf_src == list(lr.SWAP_PAF) and len(paf_src) == skm.COCO18.paf_channels == 38
    assert paf_sign == [-1 if s % 2 == 0 else 1 for s in lr.SWAP_PAF]          # "negate iff the gathered channel is even"
    assert _twice_is_identity(heat_src, paf_src, paf_sign)


def test_body25_tables(skm):
    heat_src, paf_src, paf_sign = skm.BODY_25.flip_tables()
    assert heat_src == tr.BODY_25_HEAT and len(heat_src) == 26
    assert sorted(paf_src) == list(range(52))
    assert paf_sign == [-1 if c % 2 == 0 else 1 for c in range(52)]            # every limb's mirror is in the same direction
    assert _twice_is_identity(heat_src, paf_src, paf_sign)
    assert paf_src != list(range(52))


def test_a_limb_whose_mirror_exists_only_reversed(skm):
    s = tr.make(skm, "reversed3")
    assert s.mirror == (0, 2, 1)
    heat_src, paf_src, paf_sign = s.flip_tables()
    assert heat_src == [0, 2, 1, 3] and paf_src == [2, 3, 0, 1] and paf_sign == [1, -1, 1, -1]


def test_the_other_tables_of_the_gpu_suite(skm):
    s = tr.make(skm, "pair2")
    assert s.flip_tables() == ([1, 0], [0, 1], [-1, 1])                        # x channel is 1, y channel is 0, limb reversed
    s = tr.make(skm, "full32")
    heat_src, paf_src, paf_sign = s.flip_tables()
    assert len(heat_src) == 33 and len(paf_src) == 64 and sorted(paf_src) == list(range(64))
    assert all(heat_src[i] != i for i in range(32)) and heat_src[32] == 32
    assert _twice_is_identity(heat_src, paf_src, paf_sign)
    assert sum(1 for c in range(64) if paf_src[c] == c) == 4                   # limbs 2 and 18 mirror onto themselves
    assert sorted(set(paf_sign)) == [-1, 1]
    # an unused PAF channel maps to itself with sign +
    s = skm.Skeleton("gap", ["LHip", "RHip", "Neck"], [(2, 0, 0, 1), (2, 1, 4, 5)])
    assert s.paf_channels == 6 and s.flip_tables()[1:] == ([4, 5, 2, 3, 0, 1], [-1, 1, 1, 1, -1, 1])


def test_errors_name_what_is_wrong(skm):
    with pytest.raises(ValueError, match=r"limb 1 \(Neck -> LHand\) has no mirror.*Neck and RHand"):
        skm.Skeleton("lonely", ["Neck", "LHand", "RHand", "LFoot", "RFoot"], [(3, 4, 0, 1), (0, 1, 2, 3)]).flip_tables()
    with pytest.raises(ValueError, match=r"part 0 mirrors to 1 but 1 mirrors to 2.*not an involution"):
        skm.Skeleton("cycle", ["a", "b", "c"], [(0, 1, 0, 1)], mirror=[1, 2, 0])
    with pytest.raises(ValueError, match=r"outside \[0,3\)"):
        skm.Skeleton("range", ["a", "b", "c"], [(0, 1, 0, 1)], mirror=[0, 1, 3])
    with pytest.raises(ValueError, match=r"mirror has 2 entries for 3 parts"):
        skm.Skeleton("short", ["a", "b", "c"], [(0, 1, 0, 1)], mirror=[0, 1])
    # the names are read on first use: the skeleton itself is still built (and decodes)
    s = skm.Skeleton("halved", ["Neck", "LHand"], [(0, 1, 0, 1)])
    with pytest.raises(ValueError, match=r"part LHand has no counterpart RHand"):
        s.flip_tables()
    # Neck -> LHand reads Neck -> RHand: channel 1 (its y) reads +channel 2; Neck -> RHand's x is channel 1 too and reads -channel 0
    with pytest.raises(ValueError, match=r"limb 1 gives PAF channel 1 .* another limb gave it"):
        skm.Skeleton("shared", ["Neck", "LHand", "RHand"], [(0, 1, 0, 1), (0, 2, 1, 2)]).flip_tables()
    # ... while limbs that share a channel and agree about it are accepted
    assert skm.Skeleton("agree", ["Neck", "LHand", "RHand"], [(0, 1, 0, 1), (0, 2, 0, 3)]).flip_tables()[1:] == (
        [0, 3, 2, 1], [-1, 1, 1, 1])
    # more PAF channels than a flip table holds: the tables exist, the struct is refused
    wide = skm.Skeleton("wide", ["a", "b"], [(0, 1, 0, 70)])
    assert len(wide.flip_tables()[1]) == 71
    with pytest.raises(ValueError, match=r"at most 33 / 64"):
        wide.native_flip_table()
    # lower-case names carry no side: they mirror to themselves
    assert skm.Skeleton("plain", ["left", "right", "Rx"], [(0, 1, 0, 1)]).mirror == (0, 1, 2)


def _native_tables(capi, t):
    mask = int(t.paf_neg_mask)
    return (list(t.heat_src[:t.heat_channels]), list(t.paf_src[:t.paf_channels]),
            [-1 if (mask >> c) & 1 else 1 for c in range(t.paf_channels)])


@pytest.mark.parametrize("name", tr.TABLE_NAMES)
def test_library_derivation_agrees_with_python(capi, skm, name):
    s = tr.make(skm, name)
    mirror = (C.c_int32 * s.num_parts)(*s.mirror)
    out = capi.FlipTable()
    capi.check(capi.lib.rtpose_flip_table_from_skeleton(C.byref(s.native()), mirror, int(s.background), s.paf_channels,
                                                        C.byref(out)), "rtpose_flip_table_from_skeleton")
    assert out.struct_bytes == C.sizeof(capi.FlipTable) and out.reserved == 0
    assert _native_tables(capi, out) == s.flip_tables()
    packed = s.native_flip_table()
    assert bytes(packed) == bytes(out)
    assert capi.lib.rtpose_flip_table_check(C.byref(out)) == 0


def test_library_coco18_table_is_the_reference_lists_and_the_even_source_rule(capi, skm):
    """What the COCO-18 doors (rtpose_flip_merge, rtpose_tta_accumulate) derive their table from - the library's own
    rtpose_skeleton_coco18 and COCO-18's part mirror - gives the reference's swap lists, and negates exactly the PAF
    channels k whose source SWAP_PAF[k] is even: the rule the fixed COCO-18 kernels applied, as data."""
    from oracle.host_oracle import SWAP_HEAT, SWAP_PAF
    sk, out = capi.SkeletonStruct(), capi.FlipTable()
    capi.check(capi.lib.rtpose_skeleton_coco18(C.byref(sk)), "rtpose_skeleton_coco18")
    mirror = (C.c_int32 * 18)(*skm.COCO18.mirror)
    capi.check(capi.lib.rtpose_flip_table_from_skeleton(C.byref(sk), mirror, 1, 38, C.byref(out)),
               "rtpose_flip_table_from_skeleton")
    assert (out.heat_channels, out.paf_channels) == (19, 38)
    assert list(out.heat_src[:19]) == list(SWAP_HEAT) and list(mirror) == list(SWAP_HEAT[:18])
    assert list(out.paf_src[:38]) == list(SWAP_PAF)
    assert int(out.paf_neg_mask) == sum(1 << k for k in range(38) if SWAP_PAF[k] % 2 == 0)


def test_library_refuses_what_python_refuses(capi, skm):
    lib = capi.lib
    out = capi.FlipTable()

    def derive(names, limbs, mirror, paf_channels=None, background=1):
        s = skm.Skeleton("t", names, limbs)
        m = (C.c_int32 * len(names))(*mirror)
        return lib.rtpose_flip_table_from_skeleton(C.byref(s.native()), m, background, paf_channels or s.paf_channels,
                                                   C.byref(out))
    five = ["Neck", "LHand", "RHand", "LFoot", "RFoot"]
    assert derive(five, [(3, 4, 0, 1), (0, 1, 2, 3)], [0, 2, 1, 4, 3]) == -1
    assert "limb 1" in capi.last_error() and "no mirror" in capi.last_error()
    assert derive(["a", "b", "c"], [(0, 1, 0, 1)], [1, 2, 0]) == -1 and "not an involution" in capi.last_error()
    assert derive(["a", "b", "c"], [(0, 1, 0, 1)], [0, 1, 3]) == -1 and "outside [0,3)" in capi.last_error()
    assert derive(["Neck", "LHand", "RHand"], [(0, 1, 0, 1), (0, 2, 1, 2)], [0, 2, 1]) == -1
    assert "limb 1 gives PAF channel 1" in capi.last_error()
    assert derive(["a", "b"], [(0, 1, 0, 1)], [0, 1], paf_channels=65) == -1
    assert derive(["a", "b"], [(0, 1, 0, 1)], [0, 1], paf_channels=1) == -1         # the skeleton reads channel 1
    s = skm.COCO18
    assert lib.rtpose_flip_table_from_skeleton(C.byref(s.native()), None, 1, 38, C.byref(out)) == -1
    assert lib.rtpose_flip_table_from_skeleton(None, (C.c_int32 * 18)(*s.mirror), 1, 38, C.byref(out)) == -1


def test_check_refuses_hand_broken_tables(capi, skm):
    lib = capi.lib

    def broken(edit):
        t = skm.BODY_25.native_flip_table()
        edit(t)
        rc = lib.rtpose_flip_table_check(C.byref(t))
        return rc, capi.last_error()

    def setf(field, value):
        return lambda t: setattr(t, field, value)

    def seti(field, i, value):
        return lambda t: getattr(t, field).__setitem__(i, value)
    assert lib.rtpose_flip_table_check(C.byref(skm.BODY_25.native_flip_table())) == 0
    assert lib.rtpose_flip_table_check(None) == -1
    for what, edit, word in (
            ("struct_bytes", setf("struct_bytes", C.sizeof(capi.FlipTable) - 8), "struct_bytes"),
            ("heat 0", setf("heat_channels", 0), "heat_channels"),
            ("heat 34", setf("heat_channels", 34), "heat_channels"),
            ("paf 65", setf("paf_channels", 65), "paf_channels"),
            ("paf 0", setf("paf_channels", 0), "paf_channels"),
            ("heat source out of range", seti("heat_src", 25, 26), "outside [0,26)"),
            ("paf source out of range", seti("paf_src", 0, 52), "outside [0,52)"),
            ("heat not an involution", seti("heat_src", 2, 6), "not the identity"),
            ("paf not an involution", seti("paf_src", 0, 2), "not the identity"),
            ("signs disagree", setf("paf_neg_mask", int(skm.BODY_25.native_flip_table().paf_neg_mask) ^ 4), "different signs"),
            ("mask above the channels", setf("paf_neg_mask", int(skm.BODY_25.native_flip_table().paf_neg_mask) | 1 << 60),
             "at or above paf_channels")):
        rc, msg = broken(edit)
        assert rc == -1 and word in msg, (what, rc, msg)


def test_ctypes_mirror_of_the_flip_table_matches_the_header(capi, tmp_path):
    """Size and field offsets of rtpose_flip_table as gcc lays the header's struct out, against capi.FlipTable; the struct
    is small enough to travel as a kernel argument beside the other launch arguments."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    cls = capi.FlipTable
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(rtpose_flip_table));',
             '  printf("limits %d %d\\n", RTPOSE_FLIP_MAX_HEAT, RTPOSE_FLIP_MAX_PAF);']
    for f, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rtpose_flip_table, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "flip_layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "flip_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE,
                                                          text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) <= 256
    assert got["limits"].split() == [str(capi.FLIP_MAX_HEAT), str(capi.FLIP_MAX_PAF)]
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_restated_flip_merge_is_the_old_one_for_coco18(skm):
    """tta_skel_restate.flip_merge over COCO-18's tables == layout_restate.flip_merge (value and magnitude sum), and the
    fp32 form rounds the float64 value once."""
    rng = np.random.default_rng(5)
    heat_src, paf_src, paf_sign = skm.COCO18.flip_tables()
    for c, src, sign, swap, neg in ((19, heat_src, [1] * 19, lr.SWAP_HEAT, False), (38, paf_src, paf_sign, lr.SWAP_PAF, True)):
        a = rng.standard_normal((2, 3, 5, c)).astype(np.float32)
        f = rng.standard_normal((2, 3, 5, c)).astype(np.float32)
        v, s = tr.flip_merge(a, f, src, sign)
        v0, s0 = lr.flip_merge(a, f, swap, neg)
        assert np.array_equal(v.numpy(), v0.numpy()) and np.array_equal(s.numpy(), s0.numpy())
        got = tr.flip_merge_f32(a, f, src, sign).view(np.float32).astype(np.float64)
        assert np.all(np.abs(got - v.numpy()) <= 2.0 ** -24 * s.numpy())
        assert got[0, 1, 2, 0] == (np.float32(a[0, 1, 2, 0]) + np.float32(sign[0]) * f[0, 1, 2, src[0]]) / np.float32(2)
