"""CPU suite of the target encoder (encode.py, header section 4b): the float64 restatement the kernel mirrors
(tests/encode_restate.py) against the fixture made by the reference's own get_ground_truth
(tools/make_golden_encode.py -> tests/golden/encode_ref.npz), the host helpers, and the argument refusals of the two
entry points, which run before any launch and need no device."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

import encode_restate as R

GOLD = os.path.join(ROOT, "tests", "golden", "encode_ref.npz")
SCENES = ("s0", "s1", "s2", "s3", "s4")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def enc(pkg):
    return importlib.import_module(PKG_NAME + ".encode")


def scene(gold, name):
    import json
    size = json.loads(str(gold["meta"]))["sizes"][name]
    heat, paf = gold["heat_" + name], gold["paf_" + name]
    hz = np.unpackbits(gold["heat_zero_" + name])[:heat.size].reshape(heat.shape).astype(bool)
    pz = np.unpackbits(gold["paf_zero_" + name])[:paf.size].reshape(paf.shape).astype(bool)
    return size, gold["kp18_" + name], heat, paf, hz, pz


@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_the_reference(gold, enc, name):
    """Zero pattern identical in float64; after the cast to fp32 within 1 ulp (what a different exp, or a fused
    multiply-add inside np.linalg.norm's dot, can leave after rounding).  0 differing elements are expected."""
    size, kp18, heat, paf, hz, pz = scene(gold, name)
    h64, p64 = R.encode(kp18, enc.COCO18_TRAIN, size, size, stride=8, sigma=7.0)
    assert h64.shape == heat.shape and p64.shape == paf.shape
    assert np.array_equal(h64 == 0, hz), "heat zero pattern differs in %d cells" % int(((h64 == 0) != hz).sum())
    assert np.array_equal(p64 == 0, pz), "PAF zero pattern differs in %d cells" % int(((p64 == 0) != pz).sum())
    dh, dp = R.ulp_distance(h64.astype(np.float32), heat), R.ulp_distance(p64.astype(np.float32), paf)
    print("%s: %d heat / %d PAF elements differ from the reference (max %d / %d ulp)"
          % (name, int((dh > 0).sum()), int((dp > 0).sum()), int(dh.max()), int(dp.max())))
    assert dh.max() <= 1 and dp.max() <= 1


def test_the_fixture_holds_the_cases_it_promises(gold, enc):
    """s2: the heat sum clips at 1, a limb's count reaches 3, a zero-length limb of two present parts is skipped (the
    fixture's channels of that limb are what the other five people alone give), illegal and unlabelled joints; s3:
    half-even rounding of the box changes cells (a restatement that rounds half up differs from the fixture)."""
    size, kp18, heat, paf, hz, pz = scene(gold, "s2")
    table = enc.COCO18_TRAIN
    assert (heat[:, :, :18] == 1.0).sum() > 0
    _, _, counts = R.encode(kp18, table, size, size, return_counts=True)
    assert counts.max() >= 3
    assert np.array_equal(kp18[3, 4, :2], kp18[3, 3, :2])            # RWrist on RElbow
    assert R.present(kp18[3, 3:5], size, size).all()                 # skipped for its norm, not for an absent part
    l = [(a, b) for a, b, _, _ in table.limbs].index((3, 4))
    chans = list(table.limbs[l][2:])
    _, p_others = R.encode(np.delete(kp18, 3, axis=0), table, size, size)
    assert (p_others[:, :, chans] != 0).any()
    assert np.array_equal(p_others[:, :, chans] == 0, pz[:, :, chans])
    assert R.ulp_distance(p_others[:, :, chans].astype(np.float32), paf[:, :, chans]).max() <= 1
    assert (kp18[:, :, 0] == 184).any() and (kp18[:, :, 0] == -1).any()
    assert set(np.unique(kp18[:, :, 2])) >= {0.0, 1.0, 2.0}
    size, kp18, heat, paf, hz, pz = scene(gold, "s3")
    saved = np.rint
    try:
        R.np.rint = lambda v: np.floor(v + 0.5)
        _, p_up = R.encode(kp18, enc.COCO18_TRAIN, size, size)
    finally:
        R.np.rint = saved
    assert ((p_up == 0) != pz).sum() > 0, "s3 does not tell half-even from half-up rounding"


def test_add_neck_against_the_annotations(gold, enc):
    for name in SCENES:
        kp17, kp18 = gold["kp17_" + name], gold["kp18_" + name]
        for a, b in zip(kp17, kp18):
            got = enc.add_neck(a.copy())
            assert got.shape == (18, 3) and np.array_equal(got, b)
    # the visibility rule: 2 only if both shoulders have 2, else the product
    kp = np.zeros((17, 3))
    kp[5], kp[6] = (11, 20, 2), (20, 31, 1)
    assert enc.add_neck(kp)[1].tolist() == [16.0, 26.0, 2.0]      # np.round: half to even on 15.5 and 25.5
    kp[6, 2] = 2
    assert enc.add_neck(kp)[1, 2] == 2
    kp[5, 2] = 0
    assert enc.add_neck(kp)[1, 2] == 0


def test_training_table_equals_kp_connections(gold, enc):
    s = enc.COCO18_TRAIN
    conn = gold["kp_connections"]
    assert s.num_parts == 18 and s.num_limbs == len(conn) == 19 and s.heat_channels == 19 and s.paf_channels == 38
    for i, (l, c) in enumerate(zip(s.limbs, conn)):
        assert l == (int(c[0]), int(c[1]), 2 * i, 2 * i + 1)
    names = [n.lower() for n in s.part_names]
    ref = [n.replace("right_", "r").replace("left_", "l") for n in gold["keypoint_names"].tolist()]
    assert names == ref
    # the two limbs in which it differs from the decoder's preset, on the same channels
    skel = importlib.import_module(PKG_NAME + ".skeleton")
    diff = sorted(set(s.limbs) ^ set(skel.COCO18.limbs))
    assert diff == [(2, 14, 18, 19), (2, 16, 18, 19), (5, 15, 26, 27), (5, 17, 26, 27)]
    assert "eye" in s.__doc__.lower() and "ear" in s.__doc__.lower()
    s.native()                                                       # passes rtpose_skeleton_check


def test_get_loss_names_and_values(enc):
    import torch
    g = torch.Generator().manual_seed(0)
    saved = [torch.rand(2, 38 if i % 2 == 0 else 19, 6, 8, generator=g) for i in range(12)]
    heat, paf = torch.rand(2, 19, 6, 8, generator=g), torch.rand(2, 38, 6, 8, generator=g)
    total, log = enc.get_loss(saved, heat, paf)
    names = ['loss_stage%d_L%d' % (j, k) for j in range(1, 7) for k in range(1, 3)]
    assert enc.build_names() == names
    assert list(log) == names + ['max_ht', 'min_ht', 'max_paf', 'min_paf']
    for i, nm in enumerate(names):
        want = R.stage_mse(saved[i].numpy(), (paf if i % 2 == 0 else heat).numpy())
        assert abs(log[nm] - want) <= 1e-6 * want
    assert abs(float(total) - sum(log[nm] for nm in names)) <= 1e-5 * float(total)
    assert log['max_ht'] == saved[-1][:, :-1].max().item() and log['min_paf'] == saved[-2].min().item()


def _encode_args(capi, enc, skeleton=None, **over):
    s = skeleton or enc.COCO18_TRAIN
    a = dict(kp=C.c_void_p(64), np=None, N=1, K=1, cfg=capi.EncodeCfg.make(64, 48, 8, 7.0, 1), skel=s.native(),
             ch=s.heat_channels, cp=s.paf_channels, heat=C.c_void_p(64), paf=C.c_void_p(64), ws=C.c_void_p(64),
             wsb=1 << 20)
    a.update(over)
    return a


def _encode(capi, a):
    return capi.lib.rtpose_encode_targets_skel(a["kp"], a["np"], a["N"], a["K"], C.byref(a["cfg"]) if a["cfg"] else None,
                                               C.byref(a["skel"]) if a["skel"] else None, a["ch"], a["cp"], a["heat"],
                                               a["paf"], a["ws"], a["wsb"], None)


def test_encode_refusals_name_the_argument(capi, enc):
    """Every refusal comes before any launch (and before the pointers are looked at): no device needed."""
    def refused(text, **over):
        rc = _encode(capi, _encode_args(capi, enc, **over))
        assert rc == -1, (over, rc)
        assert text in capi.last_error(), (text, capi.last_error())
    refused("NULL keypoints", kp=None)
    refused("NULL heat", heat=None)
    refused("NULL paf", paf=None)
    refused("NULL workspace", ws=None)
    refused("NULL cfg", cfg=None)
    refused("NULL skeleton", skel=None)
    cfg = capi.EncodeCfg.make(64, 48)
    cfg.struct_bytes = 8
    refused("struct_bytes", cfg=cfg)
    refused("stride", cfg=capi.EncodeCfg.make(64, 48, 0))
    refused("sigma", cfg=capi.EncodeCfg.make(64, 48, 8, 0.0))
    refused("sigma", cfg=capi.EncodeCfg.make(64, 48, 8, float("nan")))
    refused("background", ch=18)                                     # background wants channel 18 of 18
    refused("limb", cp=37)                                           # the skeleton check: a limb reads channel 37
    refused("heat_channels", ch=34)
    refused("empty grid", cfg=capi.EncodeCfg.make(4, 48, 8))
    refused("launch limit", cfg=capi.EncodeCfg.make(65536 * 8, 48, 8))
    refused("N ", N=65536)
    refused("N ", N=-1)
    refused("max_people", K=-1)
    refused("launch limit", N=65535, K=65535)
    refused("workspace_bytes", wsb=8)
    # N == 0 is a no-op, whatever the pointers are
    assert _encode(capi, _encode_args(capi, enc, N=0)) == 0
    # the size query: records of 3 words per part and 7 per limb, 8 bytes each, rounded up to 256; 0 on bad arguments
    s = enc.COCO18_TRAIN.native()
    cfg = capi.EncodeCfg.make(64, 48)
    q = capi.lib.rtpose_encode_workspace_bytes
    assert q(C.byref(cfg), C.byref(s), 3, 5) == (3 * 5 * (3 * 18 + 7 * 19) * 8 + 255) // 256 * 256
    assert q(C.byref(cfg), C.byref(s), 0, 5) == 256 and q(C.byref(cfg), C.byref(s), 3, 0) == 256
    assert q(C.byref(cfg), C.byref(s), -1, 5) == 0 and q(None, C.byref(s), 1, 1) == 0 and q(C.byref(cfg), None, 1, 1) == 0
    assert capi.ENCODE_CHUNK == 16


def test_stage_mse_refusals_and_size_query(capi):
    lib = capi.lib
    lay = capi.Layout.padded(64, 6, 8, 3, choff=38)
    p = C.c_void_p(64)

    def call(pred=p, lp=lay, tgt=p, n=2, h=6, w=8, c=19, part=p, pc=4096, loss=p):
        return lib.rtpose_stage_mse(pred, C.byref(lp) if lp is not None else None, tgt, n, h, w, c, part, pc, loss, None)

    def refused(text, **kw):
        assert call(**kw) == -1
        assert text in capi.last_error(), (text, capi.last_error())
    refused("NULL pred", pred=None)
    refused("NULL lpred", lp=None)
    refused("NULL target", tgt=None)
    refused("NULL partials", part=None)
    refused("NULL loss_out", loss=None)
    refused("channels 27", c=27)                                     # cstride 64 - choff 38 = 26
    refused("partial_count", pc=0)
    refused("bad sizes", n=0)
    refused("view", h=10)                                            # a map taller than the view's image stride
    q = lib.rtpose_stage_mse_partials
    assert q(2, 6, 8, 19) == 2 and q(2, 6, 8, 38) == 4               # 1024 elements per partial
    assert q(2, 46, 46, 38) == 158 and q(1, 1, 1, 1) == 1
    assert q(32, 46, 46, 38) == 2513 and q(64, 184, 184, 38) == 4096  # capped
    assert q(0, 6, 8, 19) == 0 and q(65535, 65535, 1, 1) == 0


def test_new_structs_mirror_the_header(capi, tmp_path):
    """rtpose_encode_cfg against its ctypes mirror (sizes and offsets from gcc), as test_capi_cpu.py does for the others."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    cls = capi.EncodeCfg
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(rtpose_encode_cfg));', '  printf("chunk %d\\n", RTPOSE_ENCODE_CHUNK);']
    lines += ['  printf("%s %%zu\\n", offsetof(rtpose_encode_cfg, %s));' % (f, f) for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "enc_layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "enc_layout")],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "enc_layout")], check=True, stdout=subprocess.PIPE,
                                                   text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["chunk"]) == capi.ENCODE_CHUNK
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_encode_is_built_with_the_decoder_flags():
    """csrc/encode.hip is built with the decoder's flags (it may run beside a forward): the Makefile says so."""
    import re
    mk = open(os.path.join(ROOT, PKG_NAME, "csrc", "Makefile")).read()
    assert re.search(r"build/encode\.o: CXXFLAGS \+= -fno-slp-vectorize -fno-vectorize", mk)
    assert re.search(r"^SRCS := .*\bencode\.hip\b", mk, flags=re.M)


def test_pack_people_forms(enc):
    a = np.arange(2 * 18 * 3, dtype=np.float64).reshape(2, 18, 3)
    kp, cnt = enc.pack_people([a, np.zeros((0, 18, 3)), a[:1]], 18)
    assert kp.shape == (3, 2, 18, 3) and cnt.tolist() == [2, 0, 1] and np.array_equal(kp[2, 0], a[0])
    kp, cnt = enc.pack_people(np.zeros((2, 5, 18, 3)), 18, counts=[5, 3])
    assert kp.shape == (2, 5, 18, 3) and cnt.tolist() == [5, 3]
    kp, cnt = enc.pack_people([np.zeros((0, 18, 3))], 18)
    assert kp.shape == (1, 1, 18, 3) and cnt.tolist() == [0]
    with pytest.raises(ValueError):
        enc.pack_people(np.zeros((2, 5, 17, 3)), 18)
    with pytest.raises(_capi_error(enc)):
        enc.encode_targets([a], device="cpu")


def _capi_error(enc):
    return importlib.import_module(PKG_NAME + "._capi").RtposeError
