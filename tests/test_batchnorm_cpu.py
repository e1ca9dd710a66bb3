"""CPU suite of the training-mode BatchNorm passes and of hourglass training (header section 2b continued,
csrc/batchnorm.hip, train.py, encode.py): the restatements of tests/bn_restate.py against float64 F.batch_norm autograd, the
conditions of the exact and of the ReLU cases the GPU tests rely on, the host side of rtpose_bn_stats / _apply / _grad
(geometry queries, every refusal with its text, before any HIP call), the zero-stuffing identity behind the stem's weight
gradient, get_loss_hourglass, and train.hourglass_forward with torch's float64 operations against the independent
restatement of tests/hourglass_train_restate.py: outputs, every parameter gradient and every running statistic, with
torch.equal - the proof of the wiring, without any rounding."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_restate as br
import hourglass_train_restate as htr
from conftest import PKG_NAME

FAKE = 1 << 20          # a 16-byte aligned "device pointer" no refused launch touches
N, H, W = 2, 9, 7
CH = 19
REFERENCE = os.environ.get("RTPOSE_REFERENCE", "/root/reference")   # the reference tree, as tools/make_golden_encode.py finds it


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


@pytest.fixture(scope="module")
def encode(pkg):
    return importlib.import_module(PKG_NAME + ".encode")


@pytest.fixture(scope="module")
def hgm(pkg):
    return importlib.import_module(PKG_NAME + ".hourglass")


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


SMALL = [c for c in br.CASES if c.n * c.h * c.w * c.channels <= 20000]


# ---- the restatements against float64 autograd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("c", SMALL, ids=br.case_id)
def test_exact_sets_restate_float64_autograd(c, relu):
    """integer operands: the sums are exact (margin < 2^53), so the restated vectors are float64's rounded once - within
    the stated bounds with room to spare - and dbias, an integer, is float64's own"""
    x, gy = br.exact_operands(c)
    w, b, rm, rv = br.affine(c.channels, True)
    assert br.exact_margin(x, gy) < 2 ** 53
    assert torch.equal(x, x.round()) and torch.equal(gy, gy.round())
    save, rm1, rv1 = br.stats_restate(x.numpy(), w.numpy(), b.numpy(), rm.numpy(), rv.numpy())
    # the ReLU mask of the truth must be the restated fp32 one: gy is masked by the restatement's y for the truth
    g = torch.from_numpy(br.masked(x.numpy(), gy.numpy(), save, relu))
    t = br.bn64(x, g, w, b, rm, rv, relu=False)
    bd = br.bounds(x.numpy(), g.numpy(), w.numpy(), b.numpy(), t, rm.numpy(), rv.numpy())
    for row, name in enumerate(("mean", "var", "invstd", "scale", "shift")):
        assert (np.abs(f64(save[row]) - t[name].numpy()) <= bd[name]).all(), name
    assert (np.abs(f64(rm1) - t["running_mean"].numpy()) <= bd["running_mean"]).all()
    assert (np.abs(f64(rv1) - t["running_var"].numpy()) <= bd["running_var"]).all()
    assert np.abs(f64(save[0]) + f64(save[5]) - t["mean"].numpy()).max() <= 2.0 ** -40 * max(1.0, np.abs(t["mean"].numpy()).max())
    db, dw, coef = br.grad_vectors_restate(x.numpy(), gy.numpy(), save, w.numpy(), relu)
    assert np.array_equal(f64(db), t["dbias"].numpy())
    assert (np.abs(f64(dw) - t["dweight"].numpy()) <= bd["dweight"]).all()
    dx = br.dx_restate(x.numpy(), gy.numpy(), save, coef, relu)
    assert (np.abs(f64(dx) - t["dx"].numpy()) <= br.dx_bound(x.numpy(), g.numpy(), w.numpy(), t, bd, False)).all()
    y = br.apply_restate(x.numpy(), save, False)
    assert (np.abs(f64(y) - t["y"].numpy()) <= br.y_bound(x.numpy(), t, bd)).all()


@pytest.mark.parametrize("big", [False, True], ids=["unit", "mean1000std"])
@pytest.mark.parametrize("c", SMALL, ids=br.case_id)
def test_random_operands_restate_within_the_bounds(c, big):
    """the same on random operands, |mean| = 1000 std included: numpy's float64 sums are one more order of summation, which
    the bounds cover like the kernel's"""
    x, gy = br.random_operands(c, big_mean=big)
    w, b, rm, rv = br.affine(c.channels, False)
    t = br.bn64(x, gy, w, b, rm, rv)
    bd = br.bounds(x.numpy(), gy.numpy(), w.numpy(), b.numpy(), t, rm.numpy(), rv.numpy())
    save, rm1, rv1 = br.stats_restate(x.numpy(), w.numpy(), b.numpy(), rm.numpy(), rv.numpy())
    for row, name in enumerate(("mean", "var", "invstd", "scale", "shift")):
        err = np.abs(f64(save[row]) - t[name].numpy())
        assert (err <= bd[name]).all(), (name, float((err / bd[name]).max()))
        # "about one fp32 ulp": the fp64 dust is far below the rounding
        if name in ("mean", "var") and c.n * c.h * c.w > 2:
            assert (bd[name] <= 1.01 * br.U32 * np.abs(t[name].numpy()) + 1e-300).all(), name
    assert (np.abs(f64(rm1) - t["running_mean"].numpy()) <= bd["running_mean"]).all()
    assert (np.abs(f64(rv1) - t["running_var"].numpy()) <= bd["running_var"]).all()
    db, dw, coef = br.grad_vectors_restate(x.numpy(), gy.numpy(), save, w.numpy(), False)
    assert (np.abs(f64(db) - t["dbias"].numpy()) <= bd["dbias"]).all()
    err = np.abs(f64(dw) - t["dweight"].numpy())
    assert (err <= bd["dweight"]).all(), float((err / bd["dweight"]).max())
    dx = br.dx_restate(x.numpy(), gy.numpy(), save, coef, False)
    err, bound = np.abs(f64(dx) - t["dx"].numpy()), br.dx_bound(x.numpy(), gy.numpy(), w.numpy(), t, bd, False)
    assert (err <= bound).all(), float((err / bound).max())
    y = br.apply_restate(x.numpy(), save, False)
    assert (np.abs(f64(y) - t["y"].numpy()) <= br.y_bound(x.numpy(), t, bd)).all()


@pytest.mark.parametrize("c", br.CASES, ids=br.case_id)
def test_exact_operands_keep_every_sum_below_2_to_53(c):
    """the condition of the GPU suite's bit-for-bit comparison, for every case (the largest included)"""
    x, gy = br.exact_operands(c)
    assert br.exact_margin(x, gy) < 2 ** 53 and x.abs().max() <= 44 and gy.abs().max() <= 3
    assert torch.equal(x, x.round()) and torch.equal(gy, gy.round()) and x.dtype == gy.dtype == torch.float32


def test_torch_updates_its_running_statistics_by_the_stated_rule():
    """(1 - m) r + m v with the UNBIASED variance, and P = 2 is accepted, P = 1 refused - torch itself, confirmed here"""
    x = torch.tensor([1.0, 4.0], dtype=torch.float64).view(2, 1, 1, 1)
    rm, rv = torch.tensor([10.0], dtype=torch.float64), torch.tensor([20.0], dtype=torch.float64)
    F.batch_norm(x, rm, rv, None, None, True, 0.1, 1e-5)
    assert rm.item() == 0.9 * 10.0 + 0.1 * 2.5 and abs(rv.item() - (0.9 * 20.0 + 0.1 * 4.5)) < 1e-12
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        F.batch_norm(x[:1], rm, rv, None, None, True, 0.1, 1e-5)


@pytest.mark.parametrize("c", SMALL, ids=br.case_id)
def test_relu_cases_have_a_mask_margin(c):
    """the condition of the GPU suite's ReLU comparison against float64: a seed whose pre-activations all stay further
    from zero than y's bound"""
    r = br.relu_operands(c)
    assert r is not None, "no seed among RELU_SEEDS clears the bound"
    x, gy, w, b, rm, rv, t, bd, margin = r
    assert margin > 0
    pre = t["scale"].view(1, -1, 1, 1) * x.double() + t["shift"].view(1, -1, 1, 1)
    assert ((pre > 0) == (t["y"] > 0)).all()


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def test_slabs_and_workspace_depend_on_the_shape_only(capi):
    lib = capi.lib
    assert capi.BN_SAVE_ROWS == br.SAVE_ROWS
    for c in br.CASES:
        p = c.n * c.h * c.w
        slab, slabs = br.slab_geometry(c.n, c.h, c.w)
        assert lib.rtpose_bn_slabs(c.channels, c.n, c.h, c.w) == slabs == lib.rtpose_bn_slabs(c.channels, 1, 1, p), c
        assert lib.rtpose_bn_workspace_doubles(c.channels, c.n, c.h, c.w) == br.workspace_doubles(c.channels, c.n, c.h, c.w)
        assert ("several slabs" in c.tags) == (slabs >= 2), (c, slabs)
        assert ("partial last slab" in c.tags) <= (p % slab != 0), c
        assert ("vector" in c.tags) == br.is_vector(c) and ("scalar" in c.tags) != ("vector" in c.tags), c
        for cs, off in (c.x, c.gy, c.out):
            assert off + c.channels <= cs, c
    ps = {c.n * c.h * c.w for c in br.CASES}
    assert {2, 63, 64, 65} <= ps and {1, 3, 4, 5, 64, 255, 256, 257} <= {c.channels for c in br.CASES}
    assert any("across" in c.tags and (c.h * c.w) % br.slab_geometry(c.n, c.h, c.w)[0] for c in br.CASES)
    assert any(br.slab_geometry(c.n, c.h, c.w)[0] > br.SLAB_UNIT for c in br.CASES)
    assert {br.is_vector(c) for c in br.CASES if "several slabs" in c.tags} == {True, False}
    assert len({br.case_id(c) for c in br.CASES}) == len(br.CASES)
    assert [lib.rtpose_bn_slabs(8, 1, 1, p) for p in (2, 63, 64, 65)] == [1, 1, 1, 2]
    assert lib.rtpose_bn_slabs(256, 32, 96, 96) == (32 * 96 * 96 + 319) // 320
    for bad in ((0, 1, 4, 4), (-1, 1, 4, 4), (8, 0, 4, 4), (8, 1, 1, 1), (8, 1, 1 << 16, 1 << 15), (8, 1 << 15, 1 << 15, 1 << 15)):
        assert lib.rtpose_bn_slabs(*bad) == 0 and lib.rtpose_bn_workspace_doubles(*bad) == 0, bad
    assert lib.rtpose_bn_slabs(1, 1, 1 << 15, (1 << 16) - 1) > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _lays(capi):
    return [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(24, H, W, 2, 5), capi.Layout.padded(20, H, W, 0, 1)]


def stats_args(capi):
    """[x, lx, weight, bias, running_mean, running_var, momentum, eps, save, workspace, doubles, channels, N, H, W, stream]"""
    lays = _lays(capi)
    return lays, [FAKE, C.byref(lays[0]), FAKE, FAKE, FAKE, FAKE, 0.1, 1e-5, FAKE, FAKE,
                  capi.lib.rtpose_bn_workspace_doubles(CH, N, H, W), CH, N, H, W, None]


def apply_args(capi):
    """[x, lx, save, y, ly, relu, channels, N, H, W, stream]"""
    lays = _lays(capi)
    return lays, [FAKE, C.byref(lays[0]), FAKE, FAKE, C.byref(lays[2]), 1, CH, N, H, W, None]


def grad_args(capi):
    """[x, lx, gy, lgy, save, weight, relu, dx, ldx, dweight, dbias, workspace, doubles, channels, N, H, W, stream]"""
    lays = _lays(capi)
    return lays, [FAKE, C.byref(lays[0]), FAKE, C.byref(lays[1]), FAKE, FAKE, 1, FAKE, C.byref(lays[2]), FAKE, FAKE, FAKE,
                  capi.lib.rtpose_bn_workspace_doubles(CH, N, H, W), CH, N, H, W, None]


def _arg(i, v):
    def f(a, lays):
        a[i] = v
    return f


def _args(*pairs):
    def f(a, lays):
        for i, v in pairs:
            a[i] = v
    return f


def _lay(j, field, v):
    def f(a, lays):
        setattr(lays[j], field, v)
    return f


STATS_FAULTS = [
    ("null x", _arg(0, None), "NULL buffer (x)"),
    ("null lx", _arg(1, None), "NULL layout (x)"),
    ("null weight", _arg(2, None), "NULL buffer (weight, bias or save)"),
    ("null bias", _arg(3, None), "NULL buffer (weight, bias or save)"),
    ("null save", _arg(8, None), "NULL buffer (weight, bias or save)"),
    ("running_mean alone", _arg(5, None), "given together or not at all"),
    ("running_var alone", _arg(4, None), "given together or not at all"),
    ("momentum above 1", _arg(6, 1.5), "momentum must lie in [0, 1]"),
    ("eps 0", _arg(7, 0.0), "eps must be a positive finite number"),
    ("eps nan", _arg(7, float("nan")), "eps must be a positive finite number"),
    ("cstride 0", _lay(0, "cstride", 0), "bad layout (x)"),
    ("negative choff", _lay(0, "choff", -1), "bad layout (x)"),
    ("x slice past cstride", _lay(0, "choff", 6), "x slice exceeds cstride"),
    ("rows shorter than the map", _lay(0, "ws", W - 1), "layout smaller than the map (x)"),
    ("null workspace", _arg(9, None), "NULL workspace"),
    ("odd workspace", _arg(9, FAKE + 4), "workspace must be 8-byte aligned"),
    ("workspace too small", _arg(10, 4 * CH - 1), "workspace of"),
    ("no channels", _arg(11, 0), "empty tensor"),
    ("no images", _arg(12, 0), "empty tensor"),
    ("one value per channel", _args((12, 1), (13, 1), (14, 1)), "N * H * W = 1"),
    ("above the launch limit", _args((12, 1 << 15), (13, 1 << 15), (14, 1 << 15)), "above the launch limit"),
]
APPLY_FAULTS = [
    ("null x", _arg(0, None), "NULL buffer (x)"),
    ("null y", _arg(3, None), "NULL buffer (y)"),
    ("null save", _arg(2, None), "NULL buffer (save)"),
    ("null lx", _arg(1, None), "NULL layout (x)"),
    ("null ly", _arg(4, None), "NULL layout (y)"),
    ("negative lead", _lay(2, "lead", -1), "bad layout (y)"),
    ("x slice past cstride", _lay(0, "choff", 6), "x slice exceeds cstride"),
    ("y slice past cstride", _lay(2, "choff", 2), "y slice exceeds cstride"),
    ("y images shorter than the map", _lay(2, "hs", H - 1), "layout smaller than the map (y)"),
    ("no rows", _arg(8, 0), "empty tensor"),
    ("one value per channel", _args((7, 1), (8, 1), (9, 1)), "N * H * W = 1"),
]
GRAD_FAULTS = [
    ("null x", _arg(0, None), "NULL buffer (x)"),
    ("null gy", _arg(2, None), "NULL buffer (gy)"),
    ("null lgy", _arg(3, None), "NULL layout (gy)"),
    ("null save", _arg(4, None), "NULL buffer (save or weight)"),
    ("null weight", _arg(5, None), "NULL buffer (save or weight)"),
    ("dx without a layout", _arg(8, None), "NULL layout (dx)"),
    ("nothing to compute", _args((7, None), (9, None), (10, None)), "nothing to compute"),
    ("gy slice past cstride", _lay(1, "choff", 6), "gy slice exceeds cstride"),
    ("dx slice past cstride", _lay(2, "choff", 2), "dx slice exceeds cstride"),
    ("dx rows shorter than the map", _lay(2, "ws", W - 1), "layout smaller than the map (dx)"),
    ("null workspace", _arg(11, None), "NULL workspace"),
    ("workspace too small", _arg(12, 4 * CH - 1), "workspace of"),
    ("no columns", _arg(16, 0), "empty tensor"),
    ("one value per channel", _args((14, 1), (15, 1), (16, 1)), "N * H * W = 1"),
]


def _refused(capi, fn, make, fault, text, who):
    lays, a = make(capi)
    fault(a, lays)
    rc = getattr(capi.lib, fn)(*a)
    assert rc == -1, (rc, capi.last_error())            # RTPOSE_E_INVAL, not a HIP error
    assert text in capi.last_error() and capi.last_error().startswith(who + ":"), capi.last_error()
    assert "device memory" not in capi.last_error()     # returned before the pointers were looked at


@pytest.mark.parametrize("name,fault,text", STATS_FAULTS, ids=[f[0] for f in STATS_FAULTS])
def test_bn_stats_refuses_on_the_host(capi, name, fault, text):
    _refused(capi, "rtpose_bn_stats", stats_args, fault, text, "bn_stats")


@pytest.mark.parametrize("name,fault,text", APPLY_FAULTS, ids=[f[0] for f in APPLY_FAULTS])
def test_bn_apply_refuses_on_the_host(capi, name, fault, text):
    _refused(capi, "rtpose_bn_apply", apply_args, fault, text, "bn_apply")


@pytest.mark.parametrize("name,fault,text", GRAD_FAULTS, ids=[f[0] for f in GRAD_FAULTS])
def test_bn_grad_refuses_on_the_host(capi, name, fault, text):
    _refused(capi, "rtpose_bn_grad", grad_args, fault, text, "bn_grad")


def test_a_dx_less_gradient_needs_no_dx_layout(capi):
    """dx = NULL takes ldx = NULL: the call gets past the host checks (and fails at the fake pointers, or launches)"""
    lays, a = grad_args(capi)
    a[7] = a[8] = None
    a[0] = None                      # ... so stop it at the next host check instead
    assert capi.lib.rtpose_bn_grad(*a) == -1 and "NULL buffer (x)" in capi.last_error()


# ---- train.py / encode.py without a launch --------------------------------------------------------------------------------------------------
def test_train_refusals_without_a_device(train, hgm):
    import torch.nn as nn
    bn = nn.BatchNorm2d(4)
    x = torch.zeros(2, 4, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.batch_norm(x, bn)
    with pytest.raises(RuntimeError, match="training mode"):
        train.batch_norm(x, bn.eval())
    with pytest.raises(RuntimeError, match="momentum=None"):
        train.batch_norm(x, nn.BatchNorm2d(4, momentum=None))
    with pytest.raises(RuntimeError, match="affine=True and track_running_stats=True"):
        train.batch_norm(x, nn.BatchNorm2d(4, affine=False))
    with pytest.raises(RuntimeError, match="affine=True and track_running_stats=True"):
        train.batch_norm(x, nn.BatchNorm2d(4, track_running_stats=False))
    with pytest.raises(RuntimeError, match="takes an nn.BatchNorm2d"):
        train.batch_norm(x, nn.BatchNorm1d(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.conv7x7_s2(torch.zeros(1, 3, 8, 8), torch.zeros(64, 3, 7, 7))
    m = hgm.hg(num_stacks=1, num_blocks=1, paf_classes=5, ht_classes=3)
    assert train._model_kind(m, "t") == "hourglass"
    with pytest.raises(TypeError, match="freezes nothing of a HourglassNet"):
        train.freeze_trunk(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.forward_train(m, torch.zeros(1, 3, 64, 64))
    conv, bnop, stem = htr.torch_ops()
    with pytest.raises(RuntimeError, match=r"call \.train\(\) first"):
        train.hourglass_forward(m.eval(), torch.zeros(1, 3, 64, 64), conv, bnop, stem)
    with pytest.raises(TypeError, match="takes an hourglass.HourglassNet"):
        train.hourglass_forward(nn.Conv2d(1, 1, 1), torch.zeros(1, 3, 64, 64), conv, bnop, stem)
    with pytest.raises(TypeError, match="HourglassNet"):
        train._model_kind(nn.Conv2d(1, 1, 1), "t")


@pytest.mark.parametrize("n,h,w", [(1, 2, 2), (2, 5, 7), (1, 8, 6)])
def test_zero_stuffing_identity_of_the_stem(n, h, w):
    """dW and dbias of Conv2d(3, 64, 7, stride 2, padding 3) from F.conv2d's float64 autograd equal the stride-1 k = 7
    weight gradient of the zero-stuffed output gradient, on integers (every sum exact): =="""
    g = torch.Generator().manual_seed(n * 100 + h * 10 + w)
    x = torch.randint(-3, 4, (n, 3, h, w), generator=g).double()
    wt = torch.randint(-2, 3, (64, 3, 7, 7), generator=g).double().requires_grad_(True)
    b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wt, b, stride=2, padding=3)
    assert tuple(y.shape[2:]) == ((h + 1) // 2, (w + 1) // 2)
    gy = torch.randint(-3, 4, y.shape, generator=g).double()
    dw, db = torch.autograd.grad(y, (wt, b), gy)
    gyz = torch.zeros(n, 64, h, w, dtype=torch.float64)
    gyz[:, :, ::2, ::2] = gy
    w1 = wt.detach().clone().requires_grad_(True)
    b1 = b.detach().clone().requires_grad_(True)
    dw1, db1 = torch.autograd.grad(F.conv2d(x, w1, b1, stride=1, padding=3), (w1, b1), gyz)
    assert torch.equal(dw, dw1) and torch.equal(db, db1) and dw.abs().max() > 0


@pytest.mark.parametrize("masks", [False, True], ids=["no_masks", "masks"])
def test_get_loss_hourglass_is_the_references_expression(encode, masks):
    g = torch.Generator().manual_seed(3)
    paf, ht = torch.randn(3, 8, 5, 6, generator=g), torch.randn(3, 4, 5, 6, generator=g)
    vec, heat = torch.randn(3, 8, 5, 6, generator=g), torch.randn(3, 4, 5, 6, generator=g)
    vw = (torch.rand(3, 8, 5, 6, generator=g) > 0.3).float()
    hw = (torch.rand(3, 4, 5, 6, generator=g) > 0.3).float()
    total, log = encode.get_loss_hourglass([paf, ht], heat, hw if masks else None, vec, vw if masks else None)
    if not masks:
        vw, hw = torch.ones_like(vw), torch.ones_like(hw)
    crit = torch.nn.MSELoss(reduction='sum')           # size_average=False
    loss1 = crit(paf * vw, vec * vw) / (2 * 3)
    loss2 = crit(ht * hw, hw * heat) / (2 * 3)
    want = 0 + loss1
    want = want + loss2
    assert torch.equal(total, want)
    assert list(log) == ['paf', 'heatmap', 'max_ht', 'min_ht', 'max_paf', 'min_paf']
    assert log['paf'] == loss1.item() and log['heatmap'] == loss2.item()
    assert log['max_ht'] == ht[:, 0:-1].max().item() and log['min_ht'] == ht[:, 0:-1].min().item()
    assert log['max_paf'] == paf.max().item() and log['min_paf'] == paf.min().item()
    with pytest.raises(ValueError):
        encode.get_loss_hourglass([paf], heat, None, vec, None)


# ---- the wiring, exactly ----------------------------------------------------------------------------------------------------------------
def _loss(paf, ht, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (paf * torch.randn(paf.shape, generator=g, dtype=paf.dtype)).sum() + (ht * torch.randn(ht.shape, generator=g, dtype=ht.dtype)).sum()


@pytest.fixture(scope="module")
def wired(train, hgm):
    """hg(2, 2, 5, 3) at 2 x 3 x 64 x 64 in float64 through train.hourglass_forward with torch's operations, once"""
    torch.manual_seed(0)
    m = htr.seed_model(hgm.hg(num_stacks=2, num_blocks=2, paf_classes=5, ht_classes=3), 3).double().train()
    sd = htr.tensors_of(m)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (paf, ht), saved = train.hourglass_forward(m, x, *htr.torch_ops())
    assert saved[0] is paf and saved[1] is ht
    _loss(paf, ht).backward()
    return m, sd, x, paf.detach(), ht.detach()


def test_hourglass_forward_equals_the_restatement_exactly(wired):
    m, sd, x, paf, ht = wired
    rpaf, rht = htr.forward(sd, x, 2, 2)
    assert torch.equal(paf, rpaf) and torch.equal(ht, rht) and paf.abs().max() > 0
    _loss(rpaf, rht).backward()
    params = dict(m.named_parameters())
    for k, v in m.state_dict().items():
        if k in params:
            assert params[k].grad is not None and torch.equal(params[k].grad, sd[k].grad), k
            assert params[k].grad.abs().max() > 0 or k.endswith("bias"), k
        else:
            assert torch.equal(v, sd[k]), k
    assert all(int(v) == 1 for k, v in m.state_dict().items() if k.endswith("num_batches_tracked"))
    assert sum(1 for k in sd if k.endswith("running_mean")) == len([1 for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "lib", "network")), reason="the reference tree is not present")
def test_hourglass_forward_equals_the_reference_module(wired, hgm):
    m, sd, x, paf, ht = wired
    sys.path.insert(0, os.path.join(REFERENCE, "lib", "network"))
    try:
        ref_mod = importlib.import_module("rtpose_hourglass")
    finally:
        sys.path.pop(0)
    ref = ref_mod.hg(num_stacks=2, num_blocks=2, paf_classes=5, ht_classes=3).double().train()
    fresh = htr.seed_model(hgm.hg(num_stacks=2, num_blocks=2, paf_classes=5, ht_classes=3), 3).double()
    ref.load_state_dict(fresh.state_dict())
    (rpaf, rht), _ = ref(x)
    assert torch.equal(paf, rpaf) and torch.equal(ht, rht)
    _loss(rpaf, rht).backward()
    params, rparams = dict(m.named_parameters()), dict(ref.named_parameters())
    for k, v in ref.state_dict().items():
        if k in rparams:
            assert torch.equal(params[k].grad, rparams[k].grad), k
        else:
            assert torch.equal(m.state_dict()[k], v), k
