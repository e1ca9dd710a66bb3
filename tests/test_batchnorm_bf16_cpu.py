"""CPU suite of the bf16 BatchNorm passes (header section 2b continued, csrc/batchnorm.hip): the host side of
rtpose_bn_apply_bf16 / rtpose_bn_grad_bf16 - the symbols, the geometry they share with rtpose_bn_grad (there are no queries
of their own), every refusal with its text, before any HIP call - and the restatements of tests/bn_bf16_restate.py: the
rounding against torch's own fp32 -> bf16 conversion over every upper half, the cases held to what their tags say, the exact
sets held to their condition."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_bf16_restate as bb
import bn_restate as br
import prelu_restate as pr

N, H, W = pr.FAULT_N, pr.FAULT_H, pr.FAULT_W
CH = pr.FAULT_CH
# 16-byte aligned "device pointers" no refused launch touches, far enough apart that no two slices meet
X, GY, SAVE, WEIGHT, OUT, DW, DB, WS = ((i + 1) << 24 for i in range(8))


# ---- the rounding -------------------------------------------------------------------------------------------------------------------
def test_rounding_equals_torch_over_every_upper_half():
    """all 65,536 upper halves under the lower halves 0x0000, 0x7fff, 0x8000, 0x8001 and 0xffff: the restatement's rounding is
    torch.Tensor.to(torch.bfloat16) on the CPU - nearest even, the largest finite values to Inf, Inf as Inf -, a NaN a NaN of
    its sign"""
    bits = bb.sweep_bits()
    assert bits.size == 5 * 65536 and len(np.unique(bits)) == bits.size
    got = bb.round_bits(bits)
    want = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = bb.is_nan32(bits)
    assert nan.sum() == 5 * 2 * 127 + 4 * 2 and np.array_equal(got[~nan], want[~nan])
    assert bb.is_nan16(got[nan]).all() and bb.is_nan16(want[nan]).all()
    assert np.array_equal(got[nan] >> 15, (bits[nan] >> 31).astype(np.uint16)), "a NaN keeps its sign"
    assert bb.same_bf16(got, want).all()
    inf = (bits & 0x7FFFFFFF) == 0x7F800000
    assert np.array_equal(got[inf], (bits[inf] >> 16).astype(np.uint16))
    # ties: an even upper half stays, an odd one goes up; the largest finite fp32 rounds to Inf
    assert bb.round_bits(np.array([0x3F808000, 0x3F818000, 0x7F7FFFFF, 0xFF7F8000], dtype=np.uint32)).tolist() == \
        [0x3F80, 0x3F82, 0x7F80, 0xFF80]


def test_apply_restatement_keeps_a_nan_through_the_relu():
    x = np.array([np.nan, -1.0, 0.0, -0.0, 2.0, np.inf, -np.inf], dtype=np.float32).reshape(1, 1, 1, 7)
    save = np.zeros((6, 1), dtype=np.float32)
    save[3] = 1.0
    y = bb.apply_bf16_restate(x, save, True).reshape(-1)
    assert bb.is_nan16(y[0]) and y[1:].tolist() == [0, 0, 0, 0x4000, 0x7F80, 0]
    y = bb.apply_bf16_restate(x, save, False).reshape(-1)
    assert bb.is_nan16(y[0]) and y[1:].tolist() == [0xBF80, 0, 0, 0x4000, 0x7F80, 0xFF80]      # (-0 + (+0) = +0)


# ---- the cases and the exact sets ---------------------------------------------------------------------------------------------------
def test_cases_are_what_their_tags_say(capi):
    lib = capi.lib
    assert [(c.channels, c.n, c.h, c.w, c.x, c.gy) for c in bb.CASES] == [(c.channels, c.n, c.h, c.w, c.x, c.gy) for c in br.CASES]
    for c in bb.CASES:
        slabs = lib.rtpose_bn_slabs(c.channels, c.n, c.h, c.w)
        assert ("several slabs" in c.tags) == (slabs >= 2), c
        assert c.tags.startswith("vector") == bb.is_vector(c) and c.tags.startswith("scalar") != bb.is_vector(c), c
        assert c.out[1] + c.channels <= c.out[0], c
        assert lib.rtpose_bn_workspace_doubles(c.channels, c.n, c.h, c.w) == br.workspace_doubles(c.channels, c.n, c.h, c.w)
    assert {c.n * c.h * c.w for c in bb.CASES} >= {2, 63, 64, 65, 128, 3 * 19 * 18, 129 * 511}
    assert {c.gap for c in bb.CASES} == {0, 1, 3} and len({bb.case_id(c) for c in bb.CASES}) == len(bb.CASES)
    reasons = {c.tags.split(";")[0] for c in bb.CASES}
    assert reasons == {"vector", "scalar (both)", "scalar (the fp32 slices alone)", "scalar (the bf16 slice alone)"}
    assert {bb.is_vector(c) for c in bb.CASES if "several slabs" in c.tags} == {True, False}
    assert any(c.channels > 256 for c in bb.CASES) and any(c.channels < 64 for c in bb.CASES)
    assert any(c.shift for c in bb.CASES) and bb.BIG not in bb.SMALL and len(bb.SMALL) == len(bb.CASES) - 1
    assert sum(bb.is_pow2(c.n * c.h * c.w) for c in bb.SMALL) >= 4


@pytest.mark.parametrize("c", bb.SMALL, ids=bb.case_id)
def test_exact_sets_are_exact(c):
    """the condition, not a measurement: every float64 result of the header's expressions on the dyadic set is an fp32 number,
    so no fp32 operation of the kernel rounds, and y and dx are the float64 values rounded to bf16 once"""
    x, gy, save, weight = bb.exact_set(c)
    assert torch.equal(x, x.round()) and torch.equal(gy, gy.round()) and gy.abs().max() <= 3
    for relu in (False, True):
        y, dx, db, dw, coef = bb.exact64(x, gy, save, weight, relu)
        assert bb.exact_in_fp32(y)
        want = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(bb.bf16_f64(bb.apply_bf16_restate(x.numpy(), save, relu)), bb.bf16_f64(want))
        if not bb.is_pow2(c.n * c.h * c.w):
            continue
        assert all(bb.exact_in_fp32(v) for v in (dx, db, dw, coef))
        t = (gy.double().numpy() if not relu else np.where(y > 0, gy.double().numpy(), 0.0)) * coef[0].reshape(1, -1, 1, 1)
        u = (x.double().numpy() - save[0].astype(np.float64).reshape(1, -1, 1, 1)) * coef[2].reshape(1, -1, 1, 1)
        assert bb.exact_in_fp32(t) and bb.exact_in_fp32(t - coef[1].reshape(1, -1, 1, 1)) and bb.exact_in_fp32(u)
        got = bb.dx_bf16_restate(x.numpy(), gy.numpy(), save, coef.astype(np.float32), relu)
        want = torch.from_numpy(dx).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(bb.bf16_f64(got), bb.bf16_f64(want))


# ---- symbols and geometry -----------------------------------------------------------------------------------------------------------
def test_symbols(capi):
    for name in ("rtpose_bn_apply_bf16", "rtpose_bn_grad_bf16"):
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
    # no queries of their own: rtpose_bn_workspace_doubles / rtpose_bn_slabs serve both gradients
    assert not any(n.startswith(("rtpose_bn_grad_bf16_", "rtpose_bn_apply_bf16_")) for n in capi.EXPORTED)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _lays(capi):
    return [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(24, H, W, 2, 5), capi.Layout.padded(24, H, W, 1, 3)]


def apply_args(capi, ptrs=(X, SAVE, OUT)):
    """valid arguments of rtpose_bn_apply_bf16: [x, lx, save, y, ly, relu, channels, N, H, W, stream]"""
    x, save, y = ptrs
    lays = _lays(capi)
    return lays, [x, C.byref(lays[0]), save, y, C.byref(lays[2]), 1, CH, N, H, W, None]


def grad_args(capi, ptrs=(X, GY, SAVE, WEIGHT, OUT, DW, DB, WS)):
    """valid arguments of rtpose_bn_grad_bf16: [x, lx, gy, lgy, save, weight, relu, dx, ldx, dweight, dbias, workspace,
    workspace_doubles, channels, N, H, W, stream]"""
    x, gy, save, weight, dx, dw, db, ws = ptrs
    lays = _lays(capi)
    doubles = capi.lib.rtpose_bn_workspace_doubles(CH, N, H, W)
    return lays, [x, C.byref(lays[0]), gy, C.byref(lays[1]), save, weight, 1, dx, C.byref(lays[2]), dw, db, ws, doubles,
                  CH, N, H, W, None]


_arg, _lay = pr.arg_fault, pr.layout_fault


def _args(*pairs):
    def f(a, lays):
        for i, v in pairs:
            a[i] = v
    return f


def _past_cstride(j):
    def f(a, lays):
        lays[j].choff = lays[j].cstride - CH + 1
    return f


def _one_value(first):
    """N = H = W = 1 (the three follow `channels` at index first - 1)"""
    return _args((first, 1), (first + 1, 1), (first + 2, 1))


# (the destination's first valid element lies (9 * 24 + 3) * 2 = 438 bytes past its base: 430 bytes before a per-channel
# vector puts it 8 bytes into it)
APPLY_FAULTS = [
    ("null x", _arg(0, None), "NULL buffer (x)"),
    ("null lx", _arg(1, None), "NULL layout (x)"),
    ("null save", _arg(2, None), "NULL buffer (save)"),
    ("null y", _arg(3, None), "NULL buffer (y)"),
    ("null ly", _arg(4, None), "NULL layout (y)"),
    ("no channels", _arg(6, 0), "empty tensor"),
    ("no images", _arg(7, 0), "empty tensor"),
    ("no rows", _arg(8, -1), "empty tensor"),
    ("no columns", _arg(9, 0), "empty tensor"),
    ("one value per channel", _one_value(7), "N * H * W = 1"),
    ("x slice past cstride", _past_cstride(0), "x slice exceeds cstride"),
    ("y slice past cstride", _past_cstride(2), "y slice exceeds cstride"),
    ("x rows shorter than the map", _lay(0, "ws", W - 1), "layout smaller than the map (x)"),
    ("y images shorter than the map", _lay(2, "hs", H - 1), "layout smaller than the map (y)"),
    ("x bad layout", _lay(0, "cstride", 0), "bad layout (x)"),
    ("y bad layout", _lay(2, "lead", -1), "bad layout (y)"),
    ("above the launch limit", pr.above_launch_limit, "above the launch limit"),
    ("an odd bf16 base", _arg(3, OUT + 1), "y must be 2-byte aligned"),
    ("y inside x", _arg(3, X + 64), "overlap those of x"),
    ("y inside save", _arg(3, SAVE - 430), "overlap those of save"),
]

GRAD_FAULTS = [
    ("null x", _arg(0, None), "NULL buffer (x)"),
    ("null lx", _arg(1, None), "NULL layout (x)"),
    ("null gy", _arg(2, None), "NULL buffer (gy)"),
    ("null lgy", _arg(3, None), "NULL layout (gy)"),
    ("null save", _arg(4, None), "NULL buffer (save or weight)"),
    ("null weight", _arg(5, None), "NULL buffer (save or weight)"),
    ("dx without a layout", _arg(8, None), "NULL layout (dx)"),
    ("nothing to compute", _args((7, None), (9, None), (10, None)), "nothing to compute"),
    ("no channels", _arg(13, 0), "empty tensor"),
    ("no images", _arg(14, -2), "empty tensor"),
    ("no rows", _arg(15, 0), "empty tensor"),
    ("no columns", _arg(16, 0), "empty tensor"),
    ("one value per channel", _one_value(14), "N * H * W = 1"),
    ("x slice past cstride", _past_cstride(0), "x slice exceeds cstride"),
    ("gy slice past cstride", _past_cstride(1), "gy slice exceeds cstride"),
    ("dx slice past cstride", _past_cstride(2), "dx slice exceeds cstride"),
    ("x rows shorter than the map", _lay(0, "ws", W - 1), "layout smaller than the map (x)"),
    ("gy images shorter than the map", _lay(1, "hs", H - 1), "layout smaller than the map (gy)"),
    ("dx rows shorter than the map", _lay(2, "ws", W - 1), "layout smaller than the map (dx)"),
    ("dx bad layout", _lay(2, "cstride", 0), "bad layout (dx)"),
    ("gy negative choff", _lay(1, "choff", -1), "bad layout (gy)"),
    ("above the launch limit", pr.above_launch_limit, "above the launch limit"),
    ("an odd bf16 base", _arg(7, OUT + 1), "dx must be 2-byte aligned"),
    ("dx inside x", _arg(7, X + 64), "overlap those of x"),
    ("dx inside gy", _arg(7, GY + 64), "overlap those of gy"),
    ("dx inside save", _arg(7, SAVE - 430), "overlap those of save"),
    ("dx inside weight", _arg(7, WEIGHT - 430), "overlap those of weight"),
    ("no workspace", _arg(11, None), "NULL workspace"),
    ("workspace off 8 bytes", _arg(11, WS + 4), "8-byte aligned"),
    ("workspace one double short", lambda a, lays: a.__setitem__(12, a[12] - 1), "rtpose_bn_workspace_doubles"),
]


@pytest.mark.parametrize("name,fault,text", APPLY_FAULTS, ids=[f[0] for f in APPLY_FAULTS])
def test_bn_apply_bf16_refuses_on_the_host(capi, name, fault, text):
    lays, a = apply_args(capi)
    fault(a, lays)
    pr.refused(capi, capi.lib.rtpose_bn_apply_bf16, "bn_apply_bf16", a, text)


@pytest.mark.parametrize("name,fault,text", GRAD_FAULTS, ids=[f[0] for f in GRAD_FAULTS])
def test_bn_grad_bf16_refuses_on_the_host(capi, name, fault, text):
    lays, a = grad_args(capi)
    fault(a, lays)
    pr.refused(capi, capi.lib.rtpose_bn_grad_bf16, "bn_grad_bf16", a, text)


def test_host_checks_pass_valid_arguments(capi):
    """with every host check passed the refusal is the pointer's (fake: no device owns it); the workspace both gradients ask
    for is rtpose_bn_workspace_doubles(); dx = NULL needs no layout and no destination checks; a frozen weight or bias is NULL"""
    lib = capi.lib
    lays, a = grad_args(capi)
    assert a[12] == lib.rtpose_bn_workspace_doubles(CH, N, H, W) == lib.rtpose_bn_slabs(CH, N, H, W) * 2 * CH + 2 * CH
    assert lib.rtpose_bn_slabs(CH, N, H, W) == 2
    assert lib.rtpose_bn_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    f32 = list(a)
    assert lib.rtpose_bn_grad(*f32) != 0 and "device memory" in capi.last_error()      # the same workspace serves the fp32 one
    a[7] = a[8] = None
    assert lib.rtpose_bn_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    lays, a = grad_args(capi)
    a[9] = a[10] = None
    assert lib.rtpose_bn_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    lays, a = apply_args(capi)
    assert lib.rtpose_bn_apply_bf16(*a) != 0 and "device memory" in capi.last_error()
    # the bf16 passes never run in place, the fp32 ones may: the same pointer for x and y
    lays, a = apply_args(capi, (X, SAVE, X))
    pr.refused(capi, lib.rtpose_bn_apply_bf16, "bn_apply_bf16", a, "overlap those of x")
