"""F(8,7), the opt-in 14-frequency form of the 7x7 stage convolutions (csrc/conv_wino7.hip: WT<8>), on the host: the
exact transform identity of its point set, the sizes and validity rules of the C ABI, host-only plan creation with
rtpose_net_options.winograd7 = 8 (the arena grows BEHIND the standard layout, which every other plan keeps), the Python
switch, and the fp32 restatement of the form (tests/wino7_f8_restate.py) against a float64 direct sum under the limit the
GPU test uses."""
import ctypes as C
import random
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import conv_driver as cd          # the suite's input / filter statistics, its float64 reference and the F(8,7) limit
import wino7_f8_restate as f87


def test_toom_cook_identity_of_the_point_set():
    """AT [(G g) o (BT d)] == the 8-output correlation, in exact rational arithmetic."""
    from oracle.winograd_tables import toom_cook
    assert len(f87.POINTS_F8_7) == 13 and f87.POINTS_F8_7[-2:] == [Fr(5, 4), Fr(-5, 4)]
    AT, G, BT = toom_cook(8, 7, f87.POINTS_F8_7)
    assert len(AT) == 8 and len(G) == 14 and len(BT) == 14 and len(BT[0]) == 14
    rng = random.Random(87)
    for _ in range(4):
        d = [Fr(rng.randint(-50, 50)) for _ in range(14)]
        g = [Fr(rng.randint(-50, 50)) for _ in range(7)]
        U = [sum(G[f][k] * g[k] for k in range(7)) for f in range(14)]
        V = [sum(BT[f][n] * d[n] for n in range(14)) for f in range(14)]
        y = [sum(AT[i][f] * U[f] * V[f] for f in range(14)) for i in range(8)]
        assert y == [sum(d[i + k] * g[k] for k in range(7)) for i in range(8)]
    # what the kernel's even / odd pairing relies on: rows 2p+1 / 2p+2 agree on even and differ in sign on odd columns,
    # column 0 of the paired rows is zero, row 0 has only even and the last row only odd columns
    for p in range(6):
        a, b = BT[2 * p + 1], BT[2 * p + 2]
        assert a[0] == 0 and b[0] == 0 and a[13] == 0 and b[13] == 0
        assert all(a[n] == (b[n] if n % 2 == 0 else -b[n]) for n in range(14))
    assert all(BT[0][n] == 0 for n in range(1, 14, 2)) and all(BT[13][n] == 0 for n in range(0, 14, 2))
    assert all(AT[i][1] == 1 for i in range(8))          # the bias rides in the point 1


def test_packed_size_and_descriptor_validity(capi):
    lib = capi.lib
    assert lib.rtpose_packed_weight_floats_winograd7(128, 128, 8) == (98 * 128 + 96) * 128
    assert lib.rtpose_packed_weight_floats_winograd7(128, 128, 6) == (84 * 128 + 96) * 128
    d = (capi.ConvDesc * 1)()
    d[0].k, d[0].cin, d[0].cout = 7, 128, 128
    d[0].lin = capi.Layout.padded(128, 46, 46, 3)
    d[0].wino_m = 8
    assert lib.rtpose_conv2d_winograd_fits(d, 32, 46, 46) == 1
    assert lib.rtpose_conv2d_winograd_fits(d, 1, 46, 46) == 1
    d[0].wino_m = 5
    assert lib.rtpose_conv2d_winograd_fits(d, 32, 46, 46) == 0
    d[0].wino_m = 8
    d[0].pool = 1
    assert lib.rtpose_conv2d_winograd_fits(d, 32, 46, 46) == 0
    d[0].pool = 0
    d[0].k, d[0].cin, d[0].cout = 3, 32, 64        # the 3x3 forms know no m = 8
    assert lib.rtpose_conv2d_winograd_fits(d, 1, 16, 16) == 0
    # the hand-over scratch a caller sizes covers 14 accumulators per wave: [flags][4 waves x 14 x 16 x 64 floats per block]
    sb = lib.rtpose_conv2d_winograd_scratch_bytes()
    assert any(sb == (4 * (cu + 2) + 255) // 256 * 256 + cu * (4 * 14 * 16 * 64 * 4) for cu in range(1, 1025)), sb


def _plan_sizes(capi, w7):
    lib = capi.lib
    h = C.c_void_p()
    opts = capi.NetOptions.make(capi.DTYPE_F32, capi.WINO_DEFAULT, w7, 0.0)
    capi.check(lib.rtpose_net_create_opts(2, 368, 368, C.byref(opts), C.byref(h)))
    try:
        return (lib.rtpose_net_num_convs(h), lib.rtpose_net_num_launches(h), lib.rtpose_net_weight_bytes(h),
                lib.rtpose_net_workspace_bytes(h))
    finally:
        lib.rtpose_net_destroy(h)


def test_host_only_plan_with_the_form_forced(pkg, capi, monkeypatch):
    """Same 92 convs and launch list; the arena of a winograd7 = 8 plan is the standard one plus the F(8,7) packings of
    the fifty 7x7 convs; the default plan's byte count is what it is without the option in the same process; the module
    sizes the arena of a key alike for every option set that maps to the key."""
    monkeypatch.delenv("RTPOSE_WINOGRAD7_M", raising=False)
    before = _plan_sizes(capi, capi.WINO_DEFAULT)
    forced = _plan_sizes(capi, 8)
    after = _plan_sizes(capi, capi.WINO_DEFAULT)
    assert before == after                                         # layout-unchanged guard
    assert forced[0] == before[0] == 92 and forced[1] == before[1]
    assert forced[2] > before[2]
    ru = lambda v: (v + 63) // 64 * 64   # noqa: E731
    extra = sum(ru((98 * cin + 96) * 128) for cin in [192] * 10 + [128] * 40)
    assert forced[2] == before[2] + 4 * extra
    # F(6,7) and F(4,7) plans read the standard arena
    assert _plan_sizes(capi, 6)[2] == before[2] and _plan_sizes(capi, 4)[2] == before[2]
    # RtposeVGG allocates an arena at the size its probe plan reports: one size per arena key over every set_winograd
    # that maps to the key, which is what a real plan with those options asks rtpose_net_bind for; F(8,7)'s is larger
    m = pkg.get_model('vgg19')
    sizes = {}
    for w3 in (None, 0, 1, 4, 'auto'):
        for w7 in (None, 0, 4, 6, 'auto', 8):
            dtype, wino = m.set_winograd(winograd3=w3, winograd7=w7)._plan_options()
            key, probe_wino = m._arena(0, dtype, wino)
            assert key == ((0, capi.DTYPE_F32, 'f87') if w7 == 8 else (0, capi.DTYPE_F32))
            sizes.setdefault(key, set()).add(m._arena_bytes(dtype, probe_wino))
            h = m._create(2, 64, 72, dtype, wino)
            try:
                assert capi.lib.rtpose_net_weight_bytes(h) == m._arena_bytes(dtype, probe_wino), (w3, w7)
            finally:
                capi.lib.rtpose_net_destroy(h)
    assert sizes == {(0, capi.DTYPE_F32): {before[2]}, (0, capi.DTYPE_F32, 'f87'): {forced[2]}}
    # the environment's switch forces the form for default-option plans (what lets bench.py run it unchanged)
    monkeypatch.setenv("RTPOSE_WINOGRAD7_M", "8")
    assert _plan_sizes(capi, capi.WINO_DEFAULT) == forced
    assert _plan_sizes(capi, 6)[2] == before[2]
    monkeypatch.delenv("RTPOSE_WINOGRAD7_M")
    bad = capi.NetOptions.make(capi.DTYPE_F32, capi.WINO_DEFAULT, 5, 0.0)
    h = C.c_void_p()
    assert capi.lib.rtpose_net_create_opts(1, 64, 64, C.byref(bad), C.byref(h)) != 0


def test_set_winograd_accepts_the_form(pkg):
    m = pkg.get_model('vgg19')
    assert m.set_winograd(winograd7=8) is m
    assert m._wino[1] == 8
    with pytest.raises(ValueError):
        m.set_winograd(winograd7=5)
    with pytest.raises(ValueError):
        m.set_winograd(winograd7=10)
    assert m.set_winograd() is m


@pytest.mark.parametrize("kw", ("he", "pos", "smooth", "ref_init_x30"))
def test_fp32_restatement_stays_under_the_gamma_limit(kw):
    """The fp32 numpy restatement of the form (64 -> 16 channels on a 12 x 46 map: 6 position groups per row, the last one
    reaching past the row) against the float64 direct sum, for the suite's seven input and four filter statistics, under
    the limit tests/test_wino7_f8_gpu.py holds the kernel to: 1000 x amp_exact(w, 7, 8) / amp_exact(w, 7, 6) (about 8 k).
    Keeps that limit honest: the arithmetic of the form alone is inside it."""
    g = torch.Generator().manual_seed(8700 + len(kw))
    c, h, w, cout = 64, 12, 46, 16
    wts = cd.weights(kw, cout, c, 7, g)
    bias = torch.randn(cout, generator=g) * 0.1
    limit = cd.gamma_limit_f87(wts)
    assert 6000.0 < limit < 10000.0, limit
    worst = {}
    for kx in cd.INPUT_KINDS:
        x = cd.inputs(kx, 1, c, h, w, g)
        y = torch.from_numpy(f87.conv_rows_f87(x[0].numpy(), wts.numpy(), bias.numpy()))[None]
        y64, s = cd.ref64(x, wts, bias, 7, (0, 13) if kx in cd.HETEROGENEOUS else None)
        worst[kx] = ((y.double() - y64).abs() / (cd.U * s)).max().item()
    print("F(8,7) restatement, %s filters: limit %.0f, gamma %s" % (kw, limit, {k: round(v, 1) for k, v in worst.items()}))
    assert all(v <= limit for v in worst.values()), (limit, worst)
    assert max(worst.values()) > 10.0           # (it IS the minimal-filtering form, not a direct sum in disguise)
