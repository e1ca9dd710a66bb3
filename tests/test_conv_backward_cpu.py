"""CPU suite of the conv backward pass (header section 2b, csrc/conv_backward.hip, train.py): the flipped, transposed filter
of the data gradient and the float64 restatements of tests/conv_backward_restate.py against torch's CPU autograd, the host
side of rtpose_conv2d_wgrad / rtpose_relu_grad (geometry queries, every refusal with its text, before any HIP call), and
what train.freeze_trunk / train.forward_train do to a CPU-constructed model without a launch."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

import conv_backward_restate as cb
from conftest import PKG_NAME

FAKE = cb.FAKE          # a 16-byte aligned "device pointer" no refused launch touches
N, H, W = cb.FAULT_N, cb.FAULT_H, cb.FAULT_W


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


# ---- the data gradient's filter and the restatements -------------------------------------------------------------------------
@pytest.mark.parametrize("k,cin,cout", [(1, 5, 3), (3, 3, 7), (7, 6, 2)])
def test_dgrad_weights_give_the_input_gradient(train, k, cin, cout):
    g = torch.Generator().manual_seed(k)
    x = torch.randn(2, cin, 6, 9, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    gy = torch.randn(2, cout, 6, 9, generator=g, dtype=torch.float64)
    F.conv2d(x, w, None, padding=k // 2).backward(gy)
    wt = train.dgrad_weights(w)
    assert tuple(wt.shape) == (cin, cout, k, k) and wt.is_contiguous()
    got = F.conv2d(gy, wt, None, padding=k // 2)
    assert (got - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item()
    dx, s = cb.dgrad64(gy, w)
    assert torch.equal(dx, x.grad) and (s >= dx.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("k", [1, 3, 7])
def test_wgrad_restatement_is_the_defining_sum(k):
    """wgrad64 (autograd of F.conv2d) against the formula of the header, tap by tap, on a zero-padded input"""
    g = torch.Generator().manual_seed(10 + k)
    n, cin, cout, h, w = 2, 3, 4, 5, 6
    x = torch.randn(n, cin, h, w, generator=g)
    gy = torch.randn(n, cout, h, w, generator=g)
    dw, s = cb.wgrad64(x, gy, k)
    p = k // 2
    xp = F.pad(x.double(), (p, p, p, p))
    for dy in range(k):
        for dx in range(k):
            ref = torch.einsum("nohw,nchw->oc", gy.double(), xp[:, :, dy:dy + h, dx:dx + w])
            sref = torch.einsum("nohw,nchw->oc", gy.double().abs(), xp[:, :, dy:dy + h, dx:dx + w].abs())
            assert (dw[:, :, dy, dx] - ref).abs().max().item() <= 1e-12
            assert (s[:, :, dy, dx] - sref).abs().max().item() <= 1e-12
    db, sb = cb.dbias64(gy)
    assert torch.allclose(db, gy.double().sum((0, 2, 3))) and (sb >= db.abs()).all()
    assert cb.gamma(1) > cb.U and cb.gamma(1 << 20) < 0.07


def test_relu_grad_restatement_on_bits():
    import numpy as np
    y = np.array([1.0, 0.0, -0.0, -2.0, np.nan, 3.0], dtype=np.float32)
    g = np.array([0x3F800000, 0x3F800000, 0x3F800000, 0x3F800000, 0x3F800000, 0x7FC12345], dtype=np.uint32)
    assert cb.relu_grad_bits(y, g).tolist() == [0x3F800000, 0, 0, 0, 0, 0x7FC12345]


# ---- geometry queries ---------------------------------------------------------------------------------------------------------
def test_slabs_and_workspace_depend_on_the_shape_only(capi):
    lib = capi.lib
    for c in cb.CASES:
        slabs = lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
        floats = lib.rtpose_conv2d_wgrad_workspace_floats(c.cin, c.cout, c.k, c.n, c.h, c.w)
        assert slabs >= 1
        # every slab holds a [tap][cout][cin] partial tile and a [cout] bias partial
        assert floats >= slabs * (c.k * c.k * c.cin * c.cout + c.cout) and floats % 4 == 0
        assert slabs == lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
    big = cb.CASES[-1]
    assert lib.rtpose_conv2d_wgrad_slabs(big.cin, big.cout, big.k, big.n, big.h, big.w) >= 3
    # unsupported shapes have no geometry
    assert lib.rtpose_conv2d_wgrad_slabs(8, 8, 5, 1, 4, 4) == 0
    assert lib.rtpose_conv2d_wgrad_workspace_floats(0, 8, 3, 1, 4, 4) == 0


# ---- the exact cases do what they claim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cb.EXACT_CASES, ids=cb.case_id)
def test_exact_case_is_exact_in_fp32_and_detects_a_missing_term(c):
    """S < 2^24 (the condition, not a measurement), torch's own fp32 CPU autograd of F.conv2d on the integer tensors equals the
    float64 one bit for bit - the reference meets the condition by itself - and no operand hides a dropped term."""
    assert cb.exact_margin(c) < 2 ** 24
    x, gy, wt, bias = cb.exact_tensors(c)
    for t, lo, hi in ((x, 0, 3), (gy, -3, 3), (wt, -2, 2), (bias, -3, 3)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and lo <= t.min().item() and t.max().item() <= hi
    assert (gy != 0).all() and (x[:, 0] >= 1).all()
    assert (c.cin - 1) * c.n * c.h * c.w < 32 or (x == 0).any()          # zeros as a ReLU leaves them
    got = {}
    for dt in (torch.float32, torch.float64):
        xx, ww, bb = (t.to(dt).requires_grad_(True) for t in (x, wt, bias))
        y = F.conv2d(xx, ww, bb, padding=c.k // 2)
        got[dt] = (y.detach(),) + torch.autograd.grad(y, (xx, ww, bb), gy.to(dt))
    for a, b, name in zip(got[torch.float32], got[torch.float64], ("y", "dx", "dw", "db")):
        assert torch.equal(a.double(), b), name
    # the restatements the GPU tests compare with are those gradients
    assert torch.equal(cb.wgrad64(x, gy, c.k)[0], got[torch.float64][2])
    assert torch.equal(cb.dbias64(gy)[0], got[torch.float64][3])
    assert torch.equal(cb.dgrad64(gy, wt)[0], got[torch.float64][1])


@pytest.mark.parametrize("c", [cb.EXACT_CASES[i] for i in (4, 11, 17)], ids=cb.case_id)
def test_a_single_missing_pixel_changes_the_exact_gradients(c):
    """zeroing one pixel of gy changes dbias of every channel, and dW[:, 0] at every tap whose shifted pixel lies in the map"""
    x, gy, _, _ = cb.exact_tensors(c)
    dw, db = cb.wgrad64(x, gy, c.k)[0], cb.dbias64(gy)[0]
    half = c.k // 2
    for n, yy, xx in ((0, 0, 0), (c.n - 1, c.h - 1, c.w - 1), (c.n // 2, c.h // 2, c.w // 2)):
        g2 = gy.clone()
        g2[n, :, yy, xx] = 0
        assert (cb.dbias64(g2)[0] != db).all()
        changed = cb.wgrad64(x, g2, c.k)[0][:, 0] != dw[:, 0]
        for dy in range(c.k):
            for dx in range(c.k):
                inside = 0 <= yy + dy - half < c.h and 0 <= xx + dx - half < c.w
                assert bool(changed[:, dy, dx].all()) == inside and bool(changed[:, dy, dx].any()) == inside, (dy, dx)


def test_exact_case_tags_hold_in_the_library_geometry(capi):
    """A tag that no longer holds fails here: a later change of the slab rule cannot quietly empty the sweep."""
    lib = capi.lib
    several = 0
    for c in cb.EXACT_CASES:
        p = c.n * c.h * c.w
        slabs = lib.rtpose_conv2d_wgrad_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
        floats = lib.rtpose_conv2d_wgrad_workspace_floats(c.cin, c.cout, c.k, c.n, c.h, c.w)
        assert slabs >= 1 and floats >= slabs * (c.k * c.k * c.cin * c.cout + c.cout) and floats % 4 == 0, c
        assert ("several slabs" in c.tags) == (slabs >= 2), (c, slabs)
        assert ("partial last chunk" in c.tags) == (p % 32 != 0) and ("full" in c.tags) == (p % 32 == 0), c
        assert c.gap in (0, 2) and ("wide gap" in c.tags) == (c.gap == 2), c        # the gap is k // 2 + c.gap
        assert "ends at cstride" not in c.tags or (c.x_off > 0 and c.x_off + c.cin == c.x_cs), c
        assert ("odd choff, odd cstride" in c.tags) == (c.x_off % 2 == 1 and c.x_cs % 2 == 1), c
        assert c.x_off + c.cin <= c.x_cs
        several += slabs >= 2
    assert several >= 9
    # the layouts the issue of the exact tests asks for are all there
    assert any(c.x_off == 0 for c in cb.EXACT_CASES) and any(c.x_off and c.x_off % 4 == 0 for c in cb.EXACT_CASES)
    assert sum("wide gap" in c.tags for c in cb.EXACT_CASES) >= 4
    assert {1, 3, 7} == {c.k for c in cb.EXACT_CASES if "several slabs" in c.tags}
    assert len({cb.case_id(c) for c in cb.EXACT_CASES}) == len(cb.EXACT_CASES)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def base(capi, k=3, cin=24, cout=38):
    d = capi.WgradDesc()
    d.x = d.gy = d.dw = d.dbias = d.workspace = FAKE
    d.workspace_floats = capi.lib.rtpose_conv2d_wgrad_workspace_floats(cin, cout, k, N, H, W)
    d.lx = capi.Layout.padded(40, H, W, k // 2, 8)
    d.lgy = capi.Layout.padded(48, H, W, 0, 4)
    d.cin, d.cout, d.k = cin, cout, k
    return d


@pytest.mark.parametrize("name,fault,text", cb.WGRAD_FAULTS, ids=[f[0] for f in cb.WGRAD_FAULTS])
def test_wgrad_refuses_on_the_host(capi, name, fault, text):
    """the table rtpose_conv2d_wgrad_bf16 runs too (tests/conv_backward_restate.py): one host path serves both"""
    d = base(capi)
    fault(d)
    cb.wgrad_refused(capi, capi.lib.rtpose_conv2d_wgrad, "conv2d_wgrad", d, (N, H, W), text)


def test_wgrad_refuses_null_descriptor_and_empty_tensor(capi):
    """and each of the three empty shapes and the two shapes above the launch limit, rtpose_conv2d_wgrad_slabs == 0 included"""
    cb.wgrad_null_empty_and_launch_limits(capi, capi.lib.rtpose_conv2d_wgrad, capi.lib.rtpose_conv2d_wgrad_slabs,
                                          "conv2d_wgrad", base)


def test_wgrad_takes_a_gap_of_exactly_half_the_filter(capi):
    """k = 7 with a gap of 3 passes every host check, with dbias and with dbias = NULL: the refusal is then the pointer's"""
    cb.wgrad_passes_the_host_checks(capi, capi.lib.rtpose_conv2d_wgrad, base)


def test_relu_grad_refuses_on_the_host(capi):
    lib = capi.lib
    lay = capi.Layout.padded(24, H, W, 1, 4)
    ok = [FAKE, C.byref(lay), FAKE, C.byref(lay), FAKE, C.byref(lay), 19, N, H, W, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.rtpose_relu_grad(*a)
    assert call(a0=None) == -1 and "NULL buffer" in capi.last_error()
    assert call(a2=None) == -1 and "NULL buffer" in capi.last_error()
    assert call(a4=None) == -1 and "NULL buffer" in capi.last_error()
    assert call(a3=None) == -1 and "NULL layout" in capi.last_error()
    assert call(a6=21) == -1 and "slice exceeds cstride" in capi.last_error()
    assert call(a6=0) == -1 and "empty tensor" in capi.last_error()
    assert call(a9=W + 2) == -1 and "smaller than the map" in capi.last_error()


# ---- train.py on a CPU-constructed model ---------------------------------------------------------------------------------------
def test_freeze_trunk_and_forward_train_leave_the_module_tree_alone(pkg, capi, train):
    model = pkg.get_model('vgg19')
    keys = list(model.state_dict().keys())
    tree = [n for n, _ in model.named_modules()]
    assert train.freeze_trunk(model) is model
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    # train/train_VGG19.py:305-307: modules 0 .. 19 of model0 hold conv1_1 .. conv4_1, nine convs
    assert frozen == ["model0.%d.%s" % (i, s) for i in (0, 2, 5, 7, 10, 12, 14, 16, 19) for s in ("weight", "bias")]
    assert sum(1 for p in model.parameters() if p.requires_grad) == 184 - len(frozen)
    # no CPU fallback, and the refusal comes before anything is changed
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.forward_train(model, torch.zeros(1, 3, 16, 16))
    with pytest.raises(capi.RtposeError, match="no CPU fallback"):
        train.conv2d(torch.zeros(1, 3, 8, 8), model.model0[0].weight, model.model0[0].bias, relu=True)
    assert list(model.state_dict().keys()) == keys and [n for n, _ in model.named_modules()] == tree
    assert len(keys) == 184 and model.training
    assert all(isinstance(m, torch.nn.Conv2d) for _, m in model._convs())
