"""CPU suite of the PReLU passes of training (header section 2b continued, csrc/prelu_backward.hip, train.py, encode.py): the
restatements of tests/prelu_restate.py against torch's float64 F.prelu autograd, the exact operand sets held to their
condition on torch alone, the host side of rtpose_prelu / rtpose_prelu_grad (geometry queries, every refusal with its text,
before any HIP call) and what train.py / encode.py do for an OpenPose_Model without a launch."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prelu_restate as pr
from conftest import PKG_NAME

FAKE = 1 << 20          # a 16-byte aligned "device pointer" no refused launch touches
N, H, W = pr.FAULT_N, pr.FAULT_H, pr.FAULT_W


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(PKG_NAME + ".encode")


@pytest.fixture(scope="module")
def openpose(pkg):
    return importlib.import_module(PKG_NAME + ".openpose")


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def test_restatements_against_float64_autograd_at_zero_and_nan():
    """z in {+0, -0, NaN, +-1} under slopes < 0, == 0 and > 0 (channels), gy = 3: the forward bits are prelu1's, sign of zero
    included; the backward is torch's."""
    zs = np.array([0.0, -0.0, np.nan, 2.0, -2.0], dtype=np.float32)
    slope = torch.tensor([-0.5, 0.0, 0.25])
    z = torch.from_numpy(np.tile(zs.reshape(1, 1, 1, 5), (1, 3, 1, 1)).copy())
    gy = torch.full_like(z, 3.0)
    y64, dz64, da64, s = pr.prelu64(z, gy, slope)
    # torch itself (confirmed here, not assumed): at z = +-0 the input gradient is slope * gy and the slope term is 0
    assert dz64[0, :, 0, 0].tolist() == [-1.5, 0.0, 0.75] and dz64[0, :, 0, 1].tolist() == [-1.5, 0.0, 0.75]
    assert dz64[0, :, 0, 2].tolist() == [-1.5, 0.0, 0.75]              # NaN z compares false: the slope path
    assert dz64[0, :, 0, 3].tolist() == [3.0, 3.0, 3.0] and torch.isnan(da64).all()
    ybits = pr.prelu_bits(z.numpy(), slope.numpy())
    y = ybits.view(np.float32)
    # prelu1 keeps z's own zero (z >= 0 holds for -0 as well); F.prelu multiplies it by the slope
    assert ybits[0, :, 0, 0].tolist() == [0, 0, 0] and ybits[0, :, 0, 1].tolist() == [0x80000000] * 3
    assert np.signbit(F.prelu(z, slope).numpy()[0, 0, 0, 0]) and not np.signbit(y[0, 0, 0, 0])
    assert np.isnan(y[0, :, 0, 2]).all() and y[0, :, 0, 3].tolist() == [2.0] * 3 and y[0, :, 0, 4].tolist() == [1.0, -0.0, -0.5]
    fin = [0, 1, 3, 4]
    assert np.array_equal(y[..., fin].astype(np.float64), y64.numpy()[..., fin])       # == : +0 equals -0
    obits = pr.prelu_grad_bits(z.numpy(), gy.numpy().view(np.uint32), slope.numpy())
    assert np.array_equal(obits.view(np.float32).astype(np.float64), dz64.numpy())
    # without the NaN column the slope gradient is the sum over z <= 0 of z * gy, and S its absolute counterpart
    _, _, da, s = pr.prelu64(z[..., fin], gy[..., fin], slope)
    assert da.tolist() == [-6.0] * 3 and s.tolist() == [6.0] * 3


def test_gradient_bits_travel_where_z_is_positive():
    z = np.array([1.0, 0.0, -0.0, -2.0, np.nan, 3.0], dtype=np.float32).reshape(1, 1, 1, 6)
    g = np.array([0x3F800000, 0x3F800000, 0x3F800000, 0x40000000, 0x3F800000, 0x7FC12345], dtype=np.uint32).reshape(1, 1, 1, 6)
    out = pr.prelu_grad_bits(z, g, np.array([0.25], dtype=np.float32))
    assert out.reshape(-1).tolist() == [0x3F800000, 0x3E800000, 0x3E800000, 0x3F000000, 0x3E800000, 0x7FC12345]


# ---- the exact operand sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(pr.EXACT_SETS))
@pytest.mark.parametrize("c", pr.CASES, ids=pr.case_id)
def test_exact_set_is_exact_in_fp32(c, kind):
    """S < 2^24 (the condition, not a measurement), and torch's own fp32 CPU F.prelu, forward and backward, equals the float64
    one: the reference alone meets the condition.  The fp32 restatements are those values."""
    z, gy, slope = pr.EXACT_SETS[kind](c)
    assert pr.exact_margin(z, gy) < 2 ** 24
    for t in (z, gy):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max().item() <= 3
    assert (gy != 0).all() and torch.equal(slope * 4, (slope * 4).round()) and set(slope.tolist()) <= set(pr.SLOPES)
    if kind == "mixed":
        assert z.numel() < 32 or ((z == 0).any() and (z > 0).any() and (z < 0).any())
    else:
        assert (z < 0).all() and (gy > 0).all()
    got = {}
    for dt in (torch.float32, torch.float64):
        zz, aa = z.to(dt).clone().requires_grad_(True), slope.to(dt).clone().requires_grad_(True)
        y = F.prelu(zz, aa)
        got[dt] = (y.detach(),) + torch.autograd.grad(y, (zz, aa), gy.to(dt))
    for a, b, name in zip(got[torch.float32], got[torch.float64], ("y", "dz", "dslope")):
        assert torch.equal(a.double(), b), name
    y64, dz64, da64, s = pr.prelu64(z, gy, slope)
    assert torch.equal(y64, got[torch.float64][0]) and torch.equal(dz64, got[torch.float64][1])
    assert torch.equal(da64, got[torch.float64][2]) and s.max().item() <= pr.exact_margin(z, gy)
    assert np.array_equal(pr.prelu_bits(z.numpy(), slope.numpy()).view(np.float32).astype(np.float64), y64.numpy())
    assert np.array_equal(pr.prelu_grad_bits(z.numpy(), gy.numpy().view(np.uint32), slope.numpy()).view(np.float32)
                          .astype(np.float64), dz64.numpy())


@pytest.mark.parametrize("c", [pr.CASES[i] for i in (2, 7, 8)], ids=pr.case_id)
def test_a_single_missing_pixel_changes_the_slope_gradient(c):
    z, gy, slope = pr.exact_negative(c)
    da = pr.prelu64(z, gy, slope)[2]
    assert (da < 0).all()
    for n, yy, xx in ((0, 0, 0), (c.n - 1, c.h - 1, c.w - 1), (c.n // 2, c.h // 2, c.w // 2)):
        g2 = gy.clone()
        g2[n, :, yy, xx] = 0
        assert (pr.prelu64(z, g2, slope)[2] != da).all()


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def test_slabs_and_workspace_depend_on_the_shape_only(capi):
    lib = capi.lib
    several = partial = 0
    for c in pr.CASES:
        p = c.n * c.h * c.w
        slabs = lib.rtpose_prelu_grad_slabs(c.channels, c.n, c.h, c.w)
        floats = lib.rtpose_prelu_grad_workspace_floats(c.channels, c.n, c.h, c.w)
        assert slabs >= 1 and floats >= slabs * c.channels, c
        assert slabs == lib.rtpose_prelu_grad_slabs(c.channels, c.n, c.h, c.w)
        assert slabs == lib.rtpose_prelu_grad_slabs(c.channels, 1, 1, p), "the slabs follow from the pixel count"
        assert ("several slabs" in c.tags) == (slabs >= 2), (c, slabs)
        # at these sizes a slab is SLAB_UNIT pixels: the count says so, and the last slab is partial iff the unit does not divide P
        assert slabs == (p + pr.SLAB_UNIT - 1) // pr.SLAB_UNIT, c
        assert ("partial last slab" in c.tags) == (p % pr.SLAB_UNIT != 0), c
        assert ("vector" in c.tags) == pr.is_vector(c) and ("scalar" in c.tags) != ("vector" in c.tags), c
        for cs, off in (c.z, c.gy, c.out):
            assert off + c.channels <= cs, c
        several += slabs >= 2
        partial += slabs >= 2 and p % pr.SLAB_UNIT != 0
    assert several >= 3 and partial >= 1
    assert sum(len({c.z, c.gy, c.out}) > 1 for c in pr.CASES) >= 3          # z, gy and out in different layouts
    assert {pr.is_vector(c) for c in pr.CASES if "several slabs" in c.tags} == {True, False}
    assert len({pr.case_id(c) for c in pr.CASES}) == len(pr.CASES)
    # the slab size off the query: the smallest P with two slabs is slab + 1
    assert [lib.rtpose_prelu_grad_slabs(8, 1, 1, p) for p in (63, 64, 65)] == [1, 1, 2]
    # slabs grow in multiples of the unit once there would be more than 1024 of them
    assert lib.rtpose_prelu_grad_slabs(512, 32, 46, 46) == (32 * 46 * 46 + 127) // 128
    # unsupported shapes have no geometry
    for bad in ((0, 1, 4, 4), (-1, 1, 4, 4), (8, 0, 4, 4), (8, 1, 1 << 16, 1 << 15), (8, 1 << 15, 1 << 15, 1 << 15)):
        assert lib.rtpose_prelu_grad_slabs(*bad) == 0 and lib.rtpose_prelu_grad_workspace_floats(*bad) == 0, bad
    assert lib.rtpose_prelu_grad_slabs(1, 1, 1 << 15, (1 << 16) - 1) > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
CH = pr.FAULT_CH


def grad_args(capi):
    """valid arguments of rtpose_prelu_grad but for the pointers: [z, lz, slope, gy, lgy, out, lout, dslope, workspace,
    workspace_floats, channels, N, H, W, stream]; the layouts are kept alive by the caller's list"""
    lays = [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(24, H, W, 2, 5), capi.Layout.padded(20, H, W, 0, 1)]
    floats = capi.lib.rtpose_prelu_grad_workspace_floats(CH, N, H, W)
    return lays, [FAKE, C.byref(lays[0]), FAKE, FAKE, C.byref(lays[1]), FAKE, C.byref(lays[2]), FAKE, FAKE, floats, CH, N, H, W, None]


# the rows all four PReLU entry points share (tests/prelu_restate.py) on this entry point's arguments, and the rows that are
# only here
GRAD_FAULTS = pr.shared_faults([("z", 0, 1, 0, False), ("gy", 3, 4, 1, False), ("out", 5, 6, 2, False)], slope=2, channels=10,
                               workspace=8) + [
    ("cstride 0", pr.layout_fault(0, "cstride", 0), "bad layout"),
    ("negative choff", pr.layout_fault(1, "choff", -1), "bad layout"),
    ("negative lead", pr.layout_fault(2, "lead", -1), "bad layout"),
    ("gy images shorter than the map", pr.layout_fault(1, "hs", H - 1), "layout smaller than the map"),
]


@pytest.mark.parametrize("name,fault,text", GRAD_FAULTS, ids=[f[0] for f in GRAD_FAULTS])
def test_prelu_grad_refuses_on_the_host(capi, name, fault, text):
    lays, a = grad_args(capi)
    fault(a, lays)
    pr.refused(capi, capi.lib.rtpose_prelu_grad, "prelu_grad", a, text)


def test_prelu_grad_host_checks_pass_valid_arguments_and_frozen_slopes(capi):
    """with every host check passed the refusal is the pointer's (fake: no device owns it); dslope = NULL needs no workspace"""
    lays, a = grad_args(capi)
    assert capi.lib.rtpose_prelu_grad_slabs(CH, N, H, W) == 2 and a[9] >= 2 * CH
    assert capi.lib.rtpose_prelu_grad(*a) != 0 and "device memory" in capi.last_error()
    a[7] = a[8] = None
    a[9] = 0
    assert capi.lib.rtpose_prelu_grad(*a) != 0 and "device memory" in capi.last_error()
    # a map above the launch limit, in layouts that hold it
    lays, a = grad_args(capi)
    for lay in lays:
        lay.ws, lay.hs, lay.lead = 1 << 15, 1 << 16, 0
    a[11:14] = [1, 1 << 16, 1 << 15]
    assert capi.lib.rtpose_prelu_grad(*a) == -1 and "above the launch limit" in capi.last_error()


def fwd_args(capi):
    """valid arguments of rtpose_prelu but for the pointers: [z, lz, slope, y, ly, channels, N, H, W, stream]"""
    lays = [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(20, H, W, 0, 1)]
    return lays, [FAKE, C.byref(lays[0]), FAKE, FAKE, C.byref(lays[1]), CH, N, H, W, None]


FWD_FAULTS = pr.shared_faults([("z", 0, 1, 0, False), ("y", 3, 4, 1, False)], slope=2, channels=5)


@pytest.mark.parametrize("name,fault,text", FWD_FAULTS, ids=[f[0] for f in FWD_FAULTS])
def test_prelu_refuses_the_shared_rows(capi, name, fault, text):
    lays, a = fwd_args(capi)
    fault(a, lays)
    pr.refused(capi, capi.lib.rtpose_prelu, "prelu", a, text)


def test_prelu_refuses_on_the_host(capi):
    lib = capi.lib
    lz, ly = capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(20, H, W, 0, 1)
    ok = [FAKE, C.byref(lz), FAKE, FAKE, C.byref(ly), CH, N, H, W, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        rc = lib.rtpose_prelu(*a)
        assert rc != 0 and capi.last_error().startswith("prelu:")
        return rc
    assert call(a0=None) == -1 and "NULL buffer" in capi.last_error()
    assert call(a2=None) == -1 and "NULL buffer" in capi.last_error()
    assert call(a3=None) == -1 and "NULL buffer" in capi.last_error()
    assert call(a1=None) == -1 and "NULL layout" in capi.last_error()
    assert call(a4=None) == -1 and "NULL layout" in capi.last_error()
    assert call(a5=21) == -1 and "z slice exceeds cstride" in capi.last_error()
    assert call(a5=20) == -1 and "y slice exceeds cstride" in capi.last_error()
    assert call(a5=0) == -1 and "empty tensor" in capi.last_error()
    assert call(a8=W + 2) == -1 and "smaller than the map" in capi.last_error()
    bad = capi.Layout.padded(24, H, W, 1, 4)
    bad.hs = 0
    assert call(a1=C.byref(bad)) == -1 and "bad layout" in capi.last_error()
    assert call() != 0 and "device memory" in capi.last_error()


# ---- the specs of the exact train.conv2d(prelu=) test hold their condition on torch alone -----------------------------------------
@pytest.mark.parametrize("s", pr.SPECS, ids=pr.spec_id)
def test_conv_prelu_spec_is_exact_in_fp32(s):
    """Four times the largest sum of absolute terms (quarter units) stays below 2^24 - doubled once more for the variants whose
    gradients accumulate twice - and torch's fp32 CPU autograd of F.prelu(F.conv2d) equals the float64 one."""
    assert 8 * pr.spec_margin(s) < 2 ** 24
    x, G, wt, b, a = pr.spec_tensors(s)
    assert set(a.tolist()) <= set(pr.SLOPES) and (a < 0).any() and (a > 0).any() and (a == 0).any()
    got = {}
    for dt in (torch.float32, torch.float64):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in (x, wt, b, a)]
        y = F.prelu(F.conv2d(leaves[0], leaves[1], leaves[2], padding=s.k // 2), leaves[3])
        got[dt] = (y.detach(),) + torch.autograd.grad(y, leaves, G.to(dt))
    for u, v, name in zip(got[torch.float32], got[torch.float64], ("y", "dx", "dw", "db", "da")):
        assert torch.equal(u.double(), v), name
    z = F.conv2d(x, wt, b, padding=s.k // 2)
    assert s.n * s.h * s.w < 8 or ((z == 0).any() and (z > 0).any() and (z < 0).any())


# ---- train.py / encode.py without a launch --------------------------------------------------------------------------------------
def test_python_side_refuses_without_a_launch(pkg, capi, train, openpose):
    model = openpose.OpenPose_Model(2, 2, 6, 4)
    keys = list(model.state_dict().keys())
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.forward_train(model, torch.zeros(1, 3, 16, 16))
    w, b, a = torch.zeros(5, 3, 3, 3), torch.zeros(5), torch.zeros(5)
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.conv2d(torch.zeros(1, 3, 8, 8), w, b, prelu=a)
    with pytest.raises(capi.RtposeError, match="relu and prelu are exclusive"):
        train.conv2d(torch.zeros(1, 3, 8, 8), w, b, relu=True, prelu=a)
    for wrong in (torch.zeros(4), torch.zeros(1), torch.zeros(5, 1), torch.zeros(5, dtype=torch.float64), 0.25):
        with pytest.raises(capi.RtposeError, match=r"fp32 \[cout\] weight of an nn.PReLU"):
            train.conv2d(torch.zeros(1, 3, 8, 8), w, b, prelu=wrong)
    # a PReLU with one shared slope cannot fuse: refused before the conv is looked at
    seq = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, 1, 1), torch.nn.PReLU())
    with pytest.raises(capi.RtposeError, match="one slope per output channel"):
        train.run_sequential(seq, torch.zeros(1, 3, 8, 8))
    with pytest.raises(capi.RtposeError, match="no backward for PReLU"):
        train.run_sequential(torch.nn.Sequential(torch.nn.PReLU(3)), torch.zeros(1, 3, 8, 8))
    for fn in (train.forward_train, train.freeze_trunk):
        with pytest.raises(TypeError, match="RtposeVGG.*OpenPose_Model"):
            fn(torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, 1, 1)), *([torch.zeros(1, 3, 8, 8)] if fn is train.forward_train else []))
    with pytest.raises(TypeError, match="RtposeVGG.*OpenPose_Model"):
        train.train_step(torch.nn.Identity(), None, None, None, None)
    assert list(model.state_dict().keys()) == keys


def test_freeze_trunk_of_an_openpose_model(train, openpose):
    model = openpose.OpenPose_Model(2, 2, 6, 4)
    assert train.freeze_trunk(model) is model
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    # modules 0 .. 19 of feature_extractor hold conv1_1 .. conv4_1: nine convs, as in rtpose_vgg's model0
    assert frozen == ["feature_extractor.%d.%s" % (i, s) for i in (0, 2, 5, 7, 10, 12, 14, 16, 19) for s in ("weight", "bias")]
    assert len(frozen) == 18 and all(p.requires_grad for n, p in model.named_parameters() if n not in frozen)
    assert sum(1 for _ in model.parameters()) == 227


def test_get_loss_openpose_is_the_stated_sum(encode):
    g = torch.Generator().manual_seed(3)
    pafs = [torch.randn(2, 6, 4, 5, generator=g) for _ in range(3)]
    heats = [torch.randn(2, 4, 4, 5, generator=g) for _ in range(2)]
    heat_t, paf_t = torch.rand(2, 4, 4, 5, generator=g), torch.randn(2, 6, 4, 5, generator=g)
    total, log = encode.get_loss_openpose([pafs, heats], heat_t, paf_t)
    terms = [((p - paf_t) ** 2).mean() for p in pafs] + [((h - heat_t) ** 2).mean() for h in heats]
    names = ["loss_paf_stage1", "loss_paf_stage2", "loss_paf_stage3", "loss_heat_stage1", "loss_heat_stage2"]
    assert list(log)[:5] == names and list(log)[5:] == ["max_ht", "min_ht", "max_paf", "min_paf"]
    for nm, t in zip(names, terms):
        assert log[nm] == pytest.approx(t.item(), rel=1e-6), nm
    by_hand = F.mse_loss(pafs[0], paf_t)
    for t in [F.mse_loss(p, paf_t) for p in pafs[1:]] + [F.mse_loss(h, heat_t) for h in heats]:
        by_hand = by_hand + t
    assert torch.equal(total, by_hand)                       # the same terms, added in the stated order
    assert [log[n] for n in names] == [F.mse_loss(p, paf_t).item() for p in pafs] + [F.mse_loss(h, heat_t).item() for h in heats]
    assert log["max_ht"] == heats[-1][:, :3].max().item() and log["min_paf"] == pafs[-1].min().item()
    for bad in ([pafs], [pafs, heats, heats], [pafs, []], [[], heats], pafs[0], [pafs[0], heats[0]]):
        with pytest.raises(ValueError, match="two non-empty lists"):
            encode.get_loss_openpose(bad, heat_t, paf_t)
    # get_loss is as it was
    for bad in ([pafs, heats], pafs + heats):
        with pytest.raises(ValueError, match="12 stage outputs"):
            encode.get_loss(bad, heat_t, paf_t)
