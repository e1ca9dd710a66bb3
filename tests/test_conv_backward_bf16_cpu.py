"""CPU suite of mixed-precision training (header section 2b, continued; csrc/conv_backward.hip; train.py's
compute_dtype): the host side of rtpose_conv2d_wgrad_bf16 - geometry queries, every refusal with its text, before any HIP
call -, the exact cases' condition, the float64 emulation of tests/conv_backward_bf16_restate.py against torch's own autograd,
and what train.py refuses without a launch."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

import conv_backward_bf16_restate as cb
from conftest import PKG_NAME

FAKE = cb.FAKE          # a 16-byte aligned "device pointer" no refused launch touches
N, H, W = cb.FAULT_N, cb.FAULT_H, cb.FAULT_W


@pytest.fixture(scope="module")
def train(pkg):
    return importlib.import_module(PKG_NAME + ".train")


# ---- geometry queries ---------------------------------------------------------------------------------------------------------
def test_slabs_and_workspace_follow_the_stated_rule(capi):
    """slabs >= 1, equal multiples of the 64-pixel chunk but for the last one, the workspace slabs * (taps cout cin + cout)
    floats rounded up to 4 as the fp32 kernel's is: the library against the restated rule, shape by shape"""
    lib = capi.lib
    shapes = [(c.cin, c.cout, c.k, c.n, c.h, c.w) for c in cb.CASES + cb.EXACT_CASES]
    shapes += [(512, 512, 3, 32, 46, 46), (128, 128, 7, 32, 46, 46), (64, 64, 3, 32, 368, 368), (128, 512, 1, 32, 46, 46)]
    for s in shapes:
        slab, slabs, floats = cb.geometry(*s)
        p = s[3] * s[4] * s[5]
        assert slabs >= 1 and slab % cb.CHUNK == 0 and (slabs - 1) * slab < p <= slabs * slab, s
        assert lib.rtpose_conv2d_wgrad_bf16_slabs(*s) == slabs, s
        assert lib.rtpose_conv2d_wgrad_bf16_workspace_floats(*s) == floats, s
        assert floats % 4 == 0 and 0 <= floats - slabs * (s[2] * s[2] * s[0] * s[1] + s[1]) < 4, s
    big = cb.CASES[-1]
    assert lib.rtpose_conv2d_wgrad_bf16_slabs(big.cin, big.cout, big.k, big.n, big.h, big.w) >= 3
    # unsupported shapes have no geometry
    assert lib.rtpose_conv2d_wgrad_bf16_slabs(8, 8, 5, 1, 4, 4) == 0
    assert lib.rtpose_conv2d_wgrad_bf16_workspace_floats(0, 8, 3, 1, 4, 4) == 0
    assert lib.rtpose_conv2d_wgrad_bf16_slabs(8, 8, 3, 1, 0, 4) == 0


def test_exact_case_tags_hold_in_the_library_geometry(capi):
    """A tag that no longer holds fails here: a later change of the slab rule cannot quietly empty the sweep."""
    lib = capi.lib
    several = 0
    for c in cb.EXACT_CASES:
        p = c.n * c.h * c.w
        slabs = lib.rtpose_conv2d_wgrad_bf16_slabs(c.cin, c.cout, c.k, c.n, c.h, c.w)
        tags = c.tags.split("; ")
        assert ("several slabs" in tags) == (slabs >= 2), (c, slabs)
        assert ("partial last chunk" in tags) == (p % cb.CHUNK != 0) and ("full" in tags) == (p % cb.CHUNK == 0), c
        assert c.gap in (0, 2) and ("wide gap" in tags) == (c.gap == 2), c        # the gap is k // 2 + c.gap
        assert "ends at cstride" not in tags or (c.x_off > 0 and c.x_off + c.cin == c.x_cs), c
        assert c.x_cs % 8 == 0 and c.x_off % 8 == 0 and c.x_off + c.cin <= c.x_cs, c
        several += slabs >= 2
    assert several >= 9
    assert {1, 3, 7} == {c.k for c in cb.EXACT_CASES if "several slabs" in c.tags}
    assert any(c.n * c.h * c.w == cb.CHUNK for c in cb.EXACT_CASES) and any(c.n * c.h * c.w == cb.CHUNK + 1 for c in cb.EXACT_CASES)
    assert len({cb.case_id(c) for c in cb.EXACT_CASES}) == len(cb.EXACT_CASES)
    assert sum(c.wide for c in cb.EXACT_CASES) == 1


# ---- the exact cases do what they claim ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cb.EXACT_CASES, ids=cb.case_id)
def test_exact_case_is_exact_in_bf16_operands_and_fp32_sums(c):
    """S < 2^24 (the condition, not a measurement), every operand an integer bf16 holds, no operand hides a dropped term, and
    torch's fp32 CPU autograd on them equals the float64 one: the reference meets the condition by itself."""
    s = cb.exact_margin(c)
    assert s < 2 ** 24
    assert c.wide or s <= 8783
    x, gy, wt, bias = cb.exact_operands(c)
    top = 255 if c.wide else 3
    for t, lo, hi in ((x, 0, top), (gy, -top, top), (wt, -2, 2), (bias, -3, 3)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and lo <= t.min().item() and t.max().item() <= hi
        assert torch.equal(cb.rb(t), t)
    assert (gy != 0).all() and (x[:, 0] >= 1).all()
    if c.wide:
        assert x.max().item() > 128 and gy.abs().max().item() > 128       # 8 significant bits are used
    got = {}
    for dt in (torch.float32, torch.float64):
        xx, ww, bb = (t.to(dt).requires_grad_(True) for t in (x, wt, bias))
        y = F.conv2d(xx, ww, bb, padding=c.k // 2)
        got[dt] = (y.detach(),) + torch.autograd.grad(y, (xx, ww, bb), gy.to(dt))
    for a, b, name in zip(got[torch.float32], got[torch.float64], ("y", "dx", "dw", "db")):
        assert torch.equal(a.double(), b), name
    assert torch.equal(cb.wgrad64(x, gy, c.k)[0], got[torch.float64][2])
    assert torch.equal(cb.dbias64(gy)[0], got[torch.float64][3])


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,relu,bias", [(1, True, True), (3, True, False), (7, False, True)])
def test_emulation_without_rounding_is_float64_autograd(k, relu, bias):
    g = torch.Generator().manual_seed(50 + k)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    x, w, b, gy = mk(2, 5, 6, 7), mk(4, 5, k, k), (mk(4) if bias else None), mk(2, 4, 6, 7)
    outs = []
    for emul in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in (x, w) + ((b,) if bias else ())]
        bb = leaves[2] if bias else None
        if emul:
            y = cb.emul_conv(leaves[0], leaves[1], bb, relu, rounding=False)
        else:
            y = F.conv2d(leaves[0], leaves[1], bb, padding=k // 2)
            y = F.relu(y) if relu else y
        outs.append((y.detach(),) + torch.autograd.grad(y, leaves, gy))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_emulation_rounds_where_the_contract_says():
    """an input of 257 is 256 to the conv, a filter of 1 + 2^-8 is 1, a gradient of 1 + 2^-9 is 1: in y, dw and dx"""
    x = torch.full((1, 1, 1, 1), 257.0, dtype=torch.float64, requires_grad=True)
    w = torch.full((1, 1, 1, 1), 1.0 + 2.0 ** -8, dtype=torch.float64, requires_grad=True)
    y = cb.emul_conv(x, w, None, True)
    assert y.item() == 256.0
    dx, dw = torch.autograd.grad(y, (x, w), torch.full_like(y, 1.0 + 2.0 ** -9))
    assert dx.item() == 1.0 and dw.item() == 256.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def base(capi, k=3, cin=24, cout=38):
    d = capi.WgradBf16Desc()
    d.x = d.gy = d.dw = d.dbias = d.workspace = FAKE
    d.workspace_floats = capi.lib.rtpose_conv2d_wgrad_bf16_workspace_floats(cin, cout, k, N, H, W)
    d.lx = capi.Layout.padded(40, H, W, k // 2, 8)
    d.lgy = capi.Layout.padded(48, H, W, 0, 8)
    d.cin, d.cout, d.k = cin, cout, k
    return d


# the rows both entry points share (tests/conv_backward_restate.py) and the alignment rows only the bf16 kernel's 16-byte
# operand loads ask for
BF16_FAULTS = [
    ("x base not 16-byte aligned", cb.set_field("x", FAKE + 8), "input slice must be 16-byte aligned"),
    ("gy base not 16-byte aligned", cb.set_field("gy", FAKE + 2), "output-gradient slice must be 16-byte aligned"),
    ("x choff not a multiple of 8", cb.set_layout("lx", "choff", 4), "input slice must be 16-byte aligned"),
    ("x cstride not a multiple of 8", cb.set_layout("lx", "cstride", 36), "input slice must be 16-byte aligned"),
    ("gy choff not a multiple of 8", cb.set_layout("lgy", "choff", 4), "output-gradient slice must be 16-byte aligned"),
    ("gy cstride not a multiple of 8", cb.set_layout("lgy", "cstride", 52), "output-gradient slice must be 16-byte aligned"),
]
WGRAD_FAULTS = cb.WGRAD_FAULTS + BF16_FAULTS


@pytest.mark.parametrize("name,fault,text", WGRAD_FAULTS, ids=[f[0] for f in WGRAD_FAULTS])
def test_wgrad_bf16_refuses_on_the_host(capi, name, fault, text):
    d = base(capi)
    fault(d)
    cb.wgrad_refused(capi, capi.lib.rtpose_conv2d_wgrad_bf16, "conv2d_wgrad_bf16", d, (N, H, W), text)


def test_wgrad_bf16_refuses_null_descriptor_empty_tensor_and_launch_limits(capi):
    # (the restated slab rule agrees that neither shape of the launch-limit cases could outgrow the grid along z)
    assert cb.geometry(46344, 46344, 1, N, H, W)[1] <= 1024 and cb.geometry(8, 8, 1, 1, 1 << 15, 1 << 15)[1] <= 1024
    cb.wgrad_null_empty_and_launch_limits(capi, capi.lib.rtpose_conv2d_wgrad_bf16, capi.lib.rtpose_conv2d_wgrad_bf16_slabs,
                                          "conv2d_wgrad_bf16", base)


def test_wgrad_bf16_takes_a_gap_of_exactly_half_the_filter_and_no_dbias(capi):
    """k = 7 with a gap of 3 and dbias = NULL pass every host check: the refusal is then the pointer's (fake: no device owns it)"""
    cb.wgrad_passes_the_host_checks(capi, capi.lib.rtpose_conv2d_wgrad_bf16, base)


# ---- train.py's compute_dtype on CPU-constructed models ----------------------------------------------------------------------------
def test_compute_dtype_refusals_come_before_the_device_check(pkg, capi, train):
    model = pkg.get_model('vgg19')
    x = torch.zeros(1, 3, 16, 16)
    wt, b = model.model0[0].weight, model.model0[0].bias
    for bad in ('fp16', 'BF16', None, 16):
        with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
            train.conv2d(x, wt, b, relu=True, compute_dtype=bad)
        with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
            train.run_sequential(model.model0, x, compute_dtype=bad)
        with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
            train.forward_train(model, x, compute_dtype=bad)
        with pytest.raises(capi.RtposeError, match="compute_dtype is 'fp32' or 'bf16'"):
            train.train_step(model, None, x, None, None, compute_dtype=bad)
    # a good one reaches the device check, in both spellings: there is no CPU fallback in either arithmetic
    for good in train.COMPUTE_DTYPES:
        with pytest.raises(capi.RtposeError, match="no CPU fallback"):
            train.conv2d(x, wt, b, relu=True, compute_dtype=good)
        with pytest.raises(capi.RtposeError, match="no CPU fallback"):
            train.forward_train(model, x, compute_dtype=good)
    assert train.bf16_fallbacks == {'fwd': 0, 'dgrad': 0}
    train.bf16_fallbacks['fwd'] = 3
    train.reset_bf16_fallbacks()
    assert train.bf16_fallbacks == {'fwd': 0, 'dgrad': 0}


def test_bf16_is_refused_for_the_batchnorm_networks(pkg, capi, train):
    hourglass = importlib.import_module(PKG_NAME + ".hourglass")
    shufflenet = importlib.import_module(PKG_NAME + ".shufflenet")
    x = torch.zeros(1, 3, 32, 32)
    for model, text in ((hourglass.HourglassNet(num_stacks=1, num_blocks=1, paf_classes=4, ht_classes=3), "BatchNorm kernels"),
                        (shufflenet.Network(), "BatchNorm and depthwise kernels")):
        with pytest.raises(capi.RtposeError, match=text):
            train.forward_train(model, x, compute_dtype='bf16')
        with pytest.raises(capi.RtposeError, match=text):
            train.train_step(model, None, x, None, None, compute_dtype='bf16')
        # 'fp32' is not refused for its dtype: the refusal that follows is the device's
        with pytest.raises(capi.RtposeError, match="no CPU fallback"):
            train.forward_train(model, x, compute_dtype='fp32')
