"""CPU suite of the stacked hourglass: the module tree against the reference's state_dict layout, the plan's introspection
and refusals (host-only), the host's BatchNorm folding, and the CPU restatement against the reference's golden maps."""
import ctypes as C
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hourglass_restate as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "hourglass_small.npz")


@pytest.fixture(scope="module")
def hgm(pkg):
    return importlib.import_module(pkg.__name__ + ".hourglass")


@pytest.mark.parametrize("stacks,blocks", [(8, 1), (2, 1), (2, 2)])
def test_state_dict_layout_is_the_references(hgm, stacks, blocks):
    m = hgm.hg(num_stacks=stacks, num_blocks=blocks, paf_classes=38, ht_classes=19)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    spec = R.state_dict_spec(stacks, blocks, 38, 19)
    assert got == [(k, tuple(s)) for k, s in spec]
    gold = np.load(GOLD)
    tag = "s%d_b%d" % (stacks, blocks)
    assert [k for k, _ in got] == list(gold[tag + "_keys"])             # what the reference module itself listed
    assert ["x".join(map(str, s)) for _, s in got] == list(gold[tag + "_shapes"])
    if (stacks, blocks) == (8, 1):
        assert len(got) == 2 * 393 + 5 * 354                       # 393 nn.Conv2d, 354 nn.BatchNorm2d
        assert sum(int(np.prod(s)) for k, s in got if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))) \
            == sum(p.numel() for p in m.parameters())
    # the reference's init: N(0, 0.01) filters, zero bias, BatchNorm weight 1 / bias 0
    assert float(m.conv1.bias.detach().abs().max()) == 0.0 and 0.005 < float(m.layer1[0].conv2.weight.detach().std()) < 0.02
    assert float(m.bn1.weight.detach().min()) == 1.0 and float(m.fc[0][1].bias.detach().abs().max()) == 0.0
    m.load_state_dict(R.seeded_state_dict(spec, 1))


def test_compat_module_is_the_package_module(pkg, hgm):
    compat = os.path.join(os.path.dirname(pkg.__file__), "compat", "lib")
    sys.path.insert(0, compat)
    try:
        mod = importlib.import_module("network.rtpose_hourglass")
    finally:
        sys.path.remove(compat)
    assert mod.hg is hgm.hg and mod.HourglassNet is hgm.HourglassNet and mod.Bottleneck is hgm.Bottleneck


def test_plan_introspection_matches_the_module(capi, hgm):
    lib = capi.lib
    h = C.c_void_p()
    opts = capi.HourglassOptions.make(8, 1, 38, 19)
    capi.check(lib.rtpose_hourglass_create(2, 384, 384, C.byref(opts), C.byref(h)))
    try:
        m = hgm.hg(num_stacks=8, num_blocks=1, paf_classes=38, ht_classes=19)
        convs = m._convs()
        assert lib.rtpose_net_num_convs(h) == 393 == len(convs)
        assert [c[0] for c in convs] == [k[:-len(".weight")] for k, v in m.state_dict().items() if v.dim() == 4]
        name = C.create_string_buffer(96)
        co, ci, k = C.c_int(), C.c_int(), C.c_int()
        pre = 0
        for i, (nm, mod, bn, pnm, pbn) in enumerate(convs):
            capi.check(lib.rtpose_net_conv_info(h, i, name, 96, C.byref(co), C.byref(ci), C.byref(k)))
            assert name.value.decode() == nm
            assert tuple(mod.weight.shape) == (co.value, ci.value, k.value, k.value)
            has = lib.rtpose_net_preact_info(h, i, name, 96)
            assert has == (1 if pbn is not None else 0) and (not has or name.value.decode() == pnm)
            assert lib.rtpose_net_prelu_info(h, i, name, 96) == 0
            pre += has
        assert pre == 115                                           # one bn1 per Bottleneck
        names = [c[0] for c in convs]
        for nm in ("conv1", "layer1.0.conv1", "layer1.0.downsample.0", "hg.3.hg.2.1.0.conv3", "fc.0.0", "score_paf.7",
                   "paf_score_.0", "ht_score_.6"):
            assert nm in names
        assert names.index("score_ht.0") < names.index("score_paf.0")      # the reference's registration order
        # algorithmic flops of the launch list: 129.33 GFLOP per image at 384 x 384
        fl, f = 0.0, C.c_double()
        kinds = {}
        for i in range(lib.rtpose_net_num_launches(h)):
            capi.check(lib.rtpose_net_launch_info(h, i, None, C.byref(k), C.byref(f), name, 96))
            fl += f.value
            nm = name.value.decode()
            key = "pool" if "pool" in nm else "up" if ".up" in nm else "save" if nm.startswith("save") else "other"
            kinds[key] = kinds.get(key, 0) + 1
        assert abs(fl / 2 / 1e9 - 129.33) < 0.01, fl / 2 / 1e9
        assert kinds["pool"] == 33 and kinds["up"] == 32 and kinds["save"] == 8
        assert lib.rtpose_net_num_launches(h) == 393 - 8 + 33 + 32 + 8 + 1      # the two score heads of a stack share a launch
        assert lib.rtpose_net_dtype(h) == capi.DTYPE_F32
        assert lib.rtpose_net_workspace_bytes(h) > 0 and lib.rtpose_net_weight_bytes(h) > 25.8e6 * 4
        assert lib.rtpose_net_forward(h, C.c_void_p(16), None) != 0 and "not bound" in capi.last_error()
        g = lib.rtpose_net_output_guard_launch(h)
        capi.check(lib.rtpose_net_launch_info(h, g, None, None, None, name, 96))
        assert name.value.decode() == "score_paf.0+score_ht.0"     # the first launch that writes the score buffer
    finally:
        lib.rtpose_net_destroy(h)


def test_plan_creation_refusals(capi):
    lib = capi.lib
    h = C.c_void_p()
    ok = capi.HourglassOptions.make(2, 1, 38, 19)

    def refused(n, hh, ww, opts, phrase):
        assert lib.rtpose_hourglass_create(n, hh, ww, C.byref(opts) if opts is not None else None, C.byref(h)) == -1
        assert phrase in capi.last_error(), capi.last_error()
    refused(1, 368, 368, ok, "multiple of 64")
    assert "rtpose_hourglass.py:85" in capi.last_error()
    refused(1, 384, 392, ok, "multiple of 64")
    refused(1, 0, 64, ok, "multiple of 64")
    refused(0, 384, 384, ok, "N>=1")
    refused(1, 384, 384, capi.HourglassOptions.make(0, 1, 38, 19), "num_stacks")
    refused(1, 384, 384, capi.HourglassOptions.make(2, 0, 38, 19), "num_blocks")
    refused(1, 384, 384, capi.HourglassOptions.make(2, 1, 0, 19), "paf_classes")
    refused(1, 384, 384, capi.HourglassOptions.make(2, 1, 38, 65), "ht_classes")
    refused(1, 384, 384, capi.HourglassOptions.make(2, 1, 38, 19, winograd3=2), "winograd3")
    short = capi.HourglassOptions.make(2, 1, 38, 19)
    short.struct_bytes = C.sizeof(short) - 4
    refused(1, 384, 384, short, "struct_bytes")
    refused(1, 384, 384, None, "options missing")
    for size in ((384, 384), (64, 128), (128, 192)):                # the sizes the reference accepts
        capi.check(lib.rtpose_hourglass_create(1, size[0], size[1], C.byref(ok), C.byref(h)))
        assert lib.rtpose_net_load_preact(h, 1, None, None, None) != 0 and "not bound" in capi.last_error()
        lib.rtpose_net_destroy(h)


def test_abi_mirror_of_the_options_struct(capi, tmp_path):
    import subprocess
    from conftest import ROOT
    cls = capi.HourglassOptions
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtpose_mi355x.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(rtpose_hourglass_options));']
    for f, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rtpose_hourglass_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "abi")], check=True, stdout=subprocess.PIPE,
                                                   text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_module_refusals(pkg, hgm):
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    dec = importlib.import_module(pkg.__name__ + ".decode")
    capi = importlib.import_module(pkg.__name__ + "._capi")
    m = hgm.hg(num_stacks=2, num_blocks=1, paf_classes=38, ht_classes=19)
    with pytest.raises(ValueError, match="fp32 only"):
        m.set_compute_dtype('bf16')
    assert m.set_compute_dtype('fp32').compute_dtype == 'fp32'
    with pytest.raises(ValueError):
        m.set_winograd(3)
    assert m.set_winograd('auto', amp_limit=100.0)._wino == (capi.WINO3_AUTO, 100.0)
    x = torch.zeros(1, 3, 64, 64)
    assert m.training
    with pytest.raises(capi.RtposeError, match=r"\.eval\(\)"):       # a fresh module is in training mode
        m(x)
    m.eval()
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):   # host tensors
        m(x)
    for bad in (dict(num_stacks=0, num_blocks=1, paf_classes=38, ht_classes=19),
                dict(num_stacks=2, num_blocks=0, paf_classes=38, ht_classes=19),
                dict(num_stacks=2, num_blocks=1, paf_classes=65, ht_classes=19)):
        with pytest.raises(ValueError):
            hgm.hg(**bad)
    # PoseEstimator: the model's stride against the config's DOWNSAMPLE, and the COCO-18 channel counts
    assert m.output_stride == 4 and (m.paf_out_channels, m.heat_out_channels) == (38, 19)
    with pytest.raises(ValueError, match="DOWNSAMPLE"):
        pipeline.PoseEstimator(m)                                    # the default config has DOWNSAMPLE = 8
    cfg = dec.default_config()
    cfg.MODEL.DOWNSAMPLE = 4
    assert pipeline.PoseEstimator(m, cfg).stride == 4
    with pytest.raises(ValueError, match="COCO-18"):
        pipeline.PoseEstimator(hgm.hg(num_stacks=1, num_blocks=1, paf_classes=14, ht_classes=9), cfg)
    # a model without the attribute behaves as before, whatever DOWNSAMPLE says
    plain = types.SimpleNamespace()
    assert pipeline.PoseEstimator(plain).stride is None and pipeline.PoseEstimator(plain, cfg).stride is None


def test_host_folding_arithmetic(hgm):
    """fold, then conv == conv, then batch_norm; and (scale, shift) == batch_norm, on random data with the module's eps"""
    g = torch.Generator().manual_seed(0)
    for k, pad, eps in ((1, 0, 1e-5), (3, 1, 1e-5), (7, 3, 1e-3)):
        conv = torch.nn.Conv2d(12, 20, k, padding=pad)
        bn = torch.nn.BatchNorm2d(20, eps=eps)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
            conv.bias.copy_(torch.randn(20, generator=g))
            bn.weight.copy_(torch.rand(20, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(20, generator=g))
            bn.running_mean.copy_(torch.randn(20, generator=g))
            bn.running_var.copy_(torch.rand(20, generator=g) + 0.5)
        bn.eval()
        x = torch.randn(2, 12, 9, 11, generator=g)
        with torch.no_grad():
            want = bn(conv(x))
            w, b = hgm.fold_bn(conv.weight, conv.bias, bn)
            got = F.conv2d(x, w, b, padding=pad)
            assert (got - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
            y = torch.randn(2, 20, 5, 5, generator=g)
            sc, sh = hgm.bn_scale_shift(bn)
            assert (y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) - bn(y)).abs().max().item() <= 1e-5
            assert sc.dtype == torch.float32 and w.dtype == torch.float32


def test_restatement_reproduces_the_golden_maps():
    gold = np.load(GOLD)
    x = torch.from_numpy(gold["x"])
    assert np.array_equal(gold["x"], np.random.Generator(np.random.PCG64(int(gold["input_seed"])))
                          .uniform(-0.5, 0.5, x.shape).astype(np.float32))
    for stacks, blocks in ((8, 1), (2, 1), (2, 2), (1, 1)):
        tag = "s%d_b%d" % (stacks, blocks)
        sd = R.seeded_state_dict(R.state_dict_spec(stacks, blocks, 38, 19), int(gold["seed"]), float(gold[tag + "_gain"]))
        with torch.no_grad():
            paf, heat = R.forward(sd, x, stacks, blocks)
        for got, want in ((paf, gold[tag + "_paf"]), (heat, gold[tag + "_heat"])):
            want = torch.from_numpy(want)
            assert 0.1 <= want.abs().max().item() <= 100.0
            assert (got - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item())
