"""OpenPose_Model on the host: module tree vs the reference's state_dict (tests/golden/openpose_small.npz), the CPU
restatement vs the reference outputs, the native plan's conv / PReLU / launch lists (host-only introspection of
rtpose_openpose_create), the CMU weight loader and the refusals."""
import ctypes as C
import importlib
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import openpose_restate as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "openpose_small.npz")
CONFIGS = ((4, 2, 38, 19), (4, 2, 14, 9))


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(pkg.__name__ + ".openpose")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_state_dict_matches_the_reference_keys_and_shapes(op, gold, cfg):
    tag = "c%d_%d_%d_%d" % cfg
    m = op.OpenPose_Model(*cfg)
    sd = m.state_dict()
    assert list(sd) == list(gold[tag + "_keys"])
    assert ["x".join(map(str, v.shape)) for v in sd.values()] == list(gold[tag + "_shapes"])
    if cfg == (4, 2, 38, 19):  # the figures of the issue
        assert len(sd) == 327 and sum(v.numel() for v in sd.values()) == 26050878
    # a checkpoint of the reference layout loads strictly
    m.load_state_dict(R.seeded_state_dict(R.state_dict_spec(*cfg), int(gold["seed"])), strict=True)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_restatement_reproduces_the_reference_outputs(gold, cfg):
    tag = "c%d_%d_%d_%d" % cfg
    sd = R.seeded_state_dict(R.state_dict_spec(*cfg), int(gold["seed"]))
    with torch.no_grad():
        paf, heat = R.forward(sd, torch.from_numpy(gold["x"]), cfg[0], cfg[1])
    outs = paf + heat
    assert len(outs) == cfg[0] + cfg[1]
    for i, t in enumerate(outs):
        ref = gold["%s_out%d" % (tag, i)]
        assert t.shape == ref.shape
        assert np.abs(t.numpy() - ref).max() <= 1e-6, i
        assert 0.1 <= np.abs(ref).max() <= 100.0  # not vanishing, not exploding


def _plan(capi, cfg, n=2, h=64, w=72):
    h_ = C.c_void_p()
    o = capi.OpenPoseOptions.make(*cfg)
    assert capi.lib.rtpose_openpose_create(n, h, w, C.byref(o), C.byref(h_)) == 0
    return h_


@pytest.mark.parametrize("cfg", CONFIGS)
def test_plan_introspection_matches_reference_state_dict(capi, gold, cfg):
    tag = "c%d_%d_%d_%d" % cfg
    lib = capi.lib
    h = _plan(capi, cfg)
    try:
        keys = list(gold[tag + "_keys"])
        shapes = dict(zip(keys, [tuple(int(v) for v in s.split("x")) for s in gold[tag + "_shapes"]]))
        conv_keys = [k[:-len(".weight")] for k in keys if k.endswith(".weight") and len(shapes[k]) == 4]
        prelu_keys = [k[:-len(".weight")] for k in keys if k.endswith(".weight") and len(shapes[k]) == 1]
        assert lib.rtpose_net_num_convs(h) == len(conv_keys) == 114
        name = C.create_string_buffer(96)
        co, ci, k = C.c_int(), C.c_int(), C.c_int()
        got_prelu = []
        for i, ck in enumerate(conv_keys):
            assert lib.rtpose_net_conv_info(h, i, name, 96, C.byref(co), C.byref(ci), C.byref(k)) == 0
            assert name.value.decode() == ck
            assert shapes[ck + ".weight"] == (co.value, ci.value, k.value, k.value)
            r = lib.rtpose_net_prelu_info(h, i, name, 96)
            assert r in (0, 1)
            if r:
                got_prelu.append(name.value.decode())
                assert shapes[name.value.decode() + ".weight"] == (co.value,)
            else:
                assert ck.endswith("Mconv7") or (ck.startswith("feature_extractor") and int(ck.split(".")[1]) < 21)
        assert got_prelu == prelu_keys and len(got_prelu) == 99
        assert lib.rtpose_net_prelu_info(h, 114, name, 96) < 0
        # launches: the trunk, then per stage 15 dense-block convs + Mconv6 + Mconv7 + a record copy; no concat copies
        names = []
        for i in range(lib.rtpose_net_num_launches(h)):
            assert lib.rtpose_net_launch_info(h, i, None, None, None, name, 96) == 0
            names.append(name.value.decode())
        assert names[0] == "nchw_to_nhwc8"
        trunk = [n for n in names if n.startswith("feature_extractor")]
        assert len(trunk) == 12
        stages = cfg[0] + cfg[1]
        assert len(names) == 1 + 12 + stages * 18
        copies = [n for n in names if not n.startswith(("feature_extractor", "l2_stages", "l1_stages", "nchw"))]
        assert copies == ["save%d" % s for s in range(stages)]
        body = names[13:]
        for s in range(stages):
            st = body[18 * s:18 * s + 18]
            pre = ("l2_stages.%d." % s) if s < cfg[0] else ("l1_stages.%d." % (s - cfg[0]))
            assert st[:17] == [pre + "Mconv%d_%d.Mconv" % (b, j) for b in range(1, 6) for j in range(3)] + \
                [pre + "Mconv6.Mconv", pre + "Mconv7"]
    finally:
        lib.rtpose_net_destroy(h)


def test_plan_creation_refuses_unsupported_topologies(capi):
    lib = capi.lib
    for cfg in ((1, 2, 38, 19), (4, 1, 38, 19), (4, 2, 0, 19), (4, 2, 38, 65), (4, 2, 65, 19)):
        h = C.c_void_p()
        o = capi.OpenPoseOptions.make(*cfg)
        assert lib.rtpose_openpose_create(1, 64, 64, C.byref(o), C.byref(h)) == -1  # RTPOSE_E_INVAL
    o = capi.OpenPoseOptions.make(4, 2, 38, 19)
    o.struct_bytes = 4
    h = C.c_void_p()
    assert lib.rtpose_openpose_create(1, 64, 64, C.byref(o), C.byref(h)) == -1


def test_unsupported_arguments_raise(op):
    for args in ((1, 2, 38, 19), (4, 1, 38, 19), (4, 2, 0, 19), (4, 2, 38, 65), (4, 2, 65, 19), (4.0, 2, 38, 19)):
        with pytest.raises(ValueError):
            op.OpenPose_Model(*args)
    m = op.OpenPose_Model(2, 2, 38, 19)
    assert m.set_compute_dtype('fp32') is m
    for dt in ('bf16', 'bf16x3', 'fp16'):
        with pytest.raises(ValueError, match="fp32 only"):
            m.set_compute_dtype(dt)
    with pytest.raises(ValueError):
        m.set_winograd(winograd3=3)
    with pytest.raises(RuntimeError):
        op.use_vgg(m)


def test_pose_estimator_refuses_non_coco_channel_counts(op, pkg):
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    with pytest.raises(ValueError, match="COCO-18"):
        pipeline.PoseEstimator(op.OpenPose_Model())  # the reference defaults: 14 / 9
    pipeline.PoseEstimator(op.OpenPose_Model(4, 2, 38, 19))


def test_forward_refuses_host_tensors(op, pkg):
    m = op.OpenPose_Model(2, 2, 38, 19)
    with pytest.raises(pkg._capi.RtposeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 64, 64))


def test_init_w_pretrained_weights_loads_convs_and_prelus_in_module_order(op, tmp_path):
    m = op.OpenPose_Model(2, 2, 38, 19)
    convs = [mm for mm in m.modules() if isinstance(mm, torch.nn.Conv2d)]
    prelus = [mm for mm in m.modules() if isinstance(mm, torch.nn.PReLU)]
    rng = np.random.Generator(np.random.PCG64(5))
    entries, want_c, want_p = [], [], []
    ci = pi = 0
    # caffe-style list: convs and prelus interleaved, with split / concat / data layers that must be skipped
    entries.append({'name': 'data_split', 'weights': []})
    for mm in m.modules():
        if isinstance(mm, torch.nn.Conv2d):
            w = rng.standard_normal(tuple(mm.weight.shape)).astype(np.float32)
            b = rng.standard_normal(tuple(mm.bias.shape)).astype(np.float32)
            entries.append({'name': 'conv_%d' % ci, 'weights': [w, b]})
            want_c.append((w, b))
            ci += 1
        elif isinstance(mm, torch.nn.PReLU):
            a = rng.standard_normal(tuple(mm.weight.shape)).astype(np.float32)
            entries.append({'name': 'prelu_%d' % pi, 'weights': [a]})
            want_p.append(a)
            pi += 1
            if pi == 3:
                entries.append({'name': 'concat_stage2', 'weights': []})
    path = tmp_path / "openpose.pkl"
    with open(path, 'wb') as f:
        pickle.dump(entries, f)
    m.init_w_pretrained_weights(str(path))
    convs = [mm for mm in m.modules() if isinstance(mm, torch.nn.Conv2d)]
    prelus = [mm for mm in m.modules() if isinstance(mm, torch.nn.PReLU)]
    assert len(convs) == len(want_c) == 12 + 4 * 17 and len(prelus) == len(want_p) == 3 + 4 * 16
    for mm, (w, b) in zip(convs, want_c):
        assert np.array_equal(mm.weight.detach().numpy(), w) and np.array_equal(mm.bias.detach().numpy(), b)
    for mm, a in zip(prelus, want_p):
        assert np.array_equal(mm.weight.detach().numpy(), a)
    # the state_dict keeps the reference layout
    assert list(m.state_dict()) == [k for k, _ in R.state_dict_spec(2, 2, 38, 19)]
