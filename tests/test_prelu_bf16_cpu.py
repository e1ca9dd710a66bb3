"""CPU suite of the bf16 PReLU passes (header section 2b continued, csrc/prelu_backward.hip): the restatements of
tests/prelu_bf16_restate.py against torch's float64 F.prelu autograd, the exact operand sets held to their condition on torch
alone, and the host side of rtpose_prelu_bf16 / rtpose_prelu_grad_bf16 - the symbols, the geometry queries against
rtpose_prelu_grad's own, every refusal with its text, before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

import prelu_bf16_restate as pb
import prelu_restate as pr

N, H, W = pr.FAULT_N, pr.FAULT_H, pr.FAULT_W
CH = pr.FAULT_CH
# 16-byte aligned "device pointers" no refused launch touches, far enough apart that no two slices meet
Z, SLOPE, GA, GB, OUT, DS, WS = ((i + 1) << 24 for i in range(7))


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def test_rounding_restated():
    f = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.4e38, np.inf, -np.inf, 0.0, -0.0, 1e-40], dtype=np.float32)
    got = pb.round_bits(f.view(np.uint32))
    # ties go to the even upper half; the largest finite values round to Inf; a subnormal keeps its upper half
    assert got.tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBF80, 0x7F80, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001]
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    nans = np.array([0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFFBFFFFF], dtype=np.uint32)
    assert pb.round_bits(nans).tolist() == [0x7FC0, 0x7FC0, 0xFFC0, 0xFFC0] and pb.is_nan16(pb.round_bits(nans)).all()
    assert pb.same_bf16([0x7FC1, 0x3F80, 0x3F80], [0xFFFF, 0x3F80, 0x3F81]).tolist() == [True, True, False]


def test_restatements_against_float64_autograd_at_zero_and_nan():
    """z in {+0, -0, NaN, +-2} under slopes < 0, == 0 and > 0 (channels), ga = 2 and gb = 1 or None: the forward is prelu1
    rounded, sign of zero included; the backward is torch's on the sum"""
    zs = np.array([0.0, -0.0, np.nan, 2.0, -2.0], dtype=np.float32)
    slope = torch.tensor([-0.5, 0.0, 0.25])
    z = torch.from_numpy(np.tile(zs.reshape(1, 1, 1, 5), (1, 3, 1, 1)).copy())
    ga, gb = torch.full_like(z, 2.0), torch.full_like(z, 1.0)
    y = pb.prelu_bf16_bits(z.numpy(), slope.numpy())
    assert y[0, :, 0, 0].tolist() == [0, 0, 0] and y[0, :, 0, 1].tolist() == [0x8000] * 3      # prelu1 keeps z's own zero
    assert pb.is_nan16(y[0, :, 0, 2]).all()
    assert pb.bf16_f64(y[0, :, 0, 3]).tolist() == [2.0] * 3 and pb.bf16_f64(y[0, :, 0, 4]).tolist() == [1.0, -0.0, -0.5]
    for two in (True, False):
        dz64, da64, _ = pb.grad64(z, ga, gb if two else None, slope)
        g = 3.0 if two else 2.0
        # torch itself: z = +-0 and a NaN z take the slope path
        for col in (0, 1, 2, 4):
            assert dz64[0, :, 0, col].tolist() == [-0.5 * g, 0.0, 0.25 * g]
        assert dz64[0, :, 0, 3].tolist() == [g] * 3 and torch.isnan(da64).all()
        out = pb.prelu_grad_bf16_bits(z.numpy(), ga.numpy().view(np.uint32), gb.numpy().view(np.uint32) if two else None,
                                      slope.numpy())
        assert np.array_equal(pb.bf16_f64(out), dz64.numpy())
        fin = [0, 1, 3, 4]
        _, da, s = pb.grad64(z[..., fin], ga[..., fin], gb[..., fin] if two else None, slope)
        assert da.tolist() == [-2.0 * g] * 3 and s.tolist() == [2.0 * g] * 3


def test_a_single_consumer_keeps_minus_zero_and_nan_bits_travel():
    z = np.array([1.0, 1.0, 1.0, 1.0, -1.0], dtype=np.float32).reshape(1, 1, 1, 5)
    ga = np.array([0x80000000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0x80000000], dtype=np.uint32).reshape(1, 1, 1, 5)
    zero = np.zeros_like(ga)
    sl = np.array([0.25], dtype=np.float32)
    assert pb.prelu_grad_bf16_bits(z, ga, None, sl).reshape(-1).tolist() == [0x8000, 0x7FC0, 0xFFC0, 0x7F80, 0x8000]
    # ga + (+0): the sum of -0 and +0 is +0 (and -0 under the slope stays a zero of the product's sign)
    assert pb.prelu_grad_bf16_bits(z, ga, zero, sl).reshape(-1).tolist()[:1] == [0x0000]
    assert pb.prelu_grad_bf16_bits(z, ga, zero, sl).reshape(-1).tolist()[3:] == [0x7F80, 0x0000]
    assert pb.sum_bits(ga, ga.copy()).reshape(-1).tolist()[0] == 0x80000000                      # -0 + -0 = -0


@pytest.mark.parametrize("kind", sorted(pb.EXACT_SETS))
@pytest.mark.parametrize("c", pb.CASES, ids=pb.case_id)
def test_exact_set_is_exact_in_bf16_and_fp32(c, kind):
    """S < 2^24 (the condition, not a measurement); y and out of the float64 reference are values bf16 holds; the restatements
    are those values"""
    z, ga, gb, slope = pb.EXACT_SETS[kind](c)
    assert pb.exact_margin(z, ga, gb) < 2 ** 24
    for t in (z, ga, gb):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max().item() <= 3
    assert (ga != 0).all() and (gb != 0).all() and set(slope.tolist()) <= set(pr.SLOPES)
    if kind == "mixed":
        assert z.numel() < 32 or ((z == 0).any() and (z > 0).any() and (z < 0).any())
        assert z.numel() < 500 or (((ga + gb) == 0).any() and ((ga + gb).abs() == 6).any())
    y64 = pr.prelu64(z, ga, slope)[0]
    for two in (True, False):
        dz64, da64, s = pb.grad64(z, ga, gb if two else None, slope)
        for v in (y64, dz64):
            assert torch.equal(v.float().to(torch.bfloat16).double(), v)
        out = pb.prelu_grad_bf16_bits(z.numpy(), ga.numpy().view(np.uint32), gb.numpy().view(np.uint32) if two else None,
                                      slope.numpy())
        assert np.array_equal(pb.bf16_f64(out), dz64.numpy())
        assert s.max().item() <= pb.exact_margin(z, ga, gb)
    assert np.array_equal(pb.bf16_f64(pb.prelu_bf16_bits(z.numpy(), slope.numpy())), y64.numpy())


def test_random_operands_hold_what_they_promise():
    c = pb.CASES[4]
    z, ga_bits, gb_bits, slope = pb.random_operands(c)
    zn = z.numpy()
    assert (slope < 0).any() and (slope > 0).any() and (zn == 0).any() and np.signbit(zn[zn == 0]).any()
    for s in pb.SPECIALS:
        assert (ga_bits == s).any(), hex(s)
    g = pb.sum_bits(ga_bits, gb_bits)
    assert (g[(ga_bits == 0x80000000) & (gb_bits == 0x80000000)] == 0x80000000).all()
    assert pb.is_nan32(g[(ga_bits == 0x7F800000) & (gb_bits == 0xFF800000)]).all()
    low = zn <= 0
    assert np.isfinite(ga_bits.view(np.float32)[low]).all() and np.isfinite(gb_bits.view(np.float32)[low]).all()
    assert (gb_bits[low] == 3).any()
    zs, sl = pb.sweep_operands()
    assert zs.shape == (1, 4, 512, 512) and len(np.unique(zs[0, 0])) == 1 << 18 and (sl > 0).any() and (sl < 0).any()


# ---- symbols and geometry -----------------------------------------------------------------------------------------------------------
def test_symbols_and_geometry(capi):
    lib = capi.lib
    for name in ("rtpose_prelu_bf16", "rtpose_prelu_grad_bf16", "rtpose_prelu_grad_bf16_workspace_floats",
                 "rtpose_prelu_grad_bf16_slabs"):
        assert name in capi.EXPORTED and hasattr(lib, name)
    several = 0
    for c in pb.CASES:
        shape = (c.channels, c.n, c.h, c.w)
        slabs = lib.rtpose_prelu_grad_bf16_slabs(*shape)
        assert slabs == lib.rtpose_prelu_grad_slabs(*shape) >= 1, c
        assert lib.rtpose_prelu_grad_bf16_workspace_floats(*shape) == lib.rtpose_prelu_grad_workspace_floats(*shape) \
            >= slabs * c.channels, c
        assert ("several slabs" in c.tags) == (slabs >= 2), c
        assert ("vector" in c.tags) == pb.is_vector(c) and ("scalar" in c.tags) != ("vector" in c.tags), c
        for cs, off in (c.z, c.ga, c.gb, c.out):
            assert off + c.channels <= cs, c
        several += slabs >= 2
    assert several >= 5 and len({pb.case_id(c) for c in pb.CASES}) == len(pb.CASES)
    assert {c.n * c.h * c.w for c in pb.CASES} >= {1, 63, 64, 65, 1537, 128, 3 * 19 * 18}
    assert {c.channels for c in pb.CASES} == {1, 3, 19, 52, 96, 130, 8, 512, 128}
    assert {pb.is_vector(c) for c in pb.CASES if "several slabs" in c.tags} == {True, False}
    assert lib.rtpose_prelu_grad_bf16_slabs(512, 32, 46, 46) == (32 * 46 * 46 + 127) // 128
    for bad in ((0, 1, 4, 4), (-1, 1, 4, 4), (8, 0, 4, 4), (8, 1, 1 << 16, 1 << 15), (8, 1 << 15, 1 << 15, 1 << 15)):
        assert lib.rtpose_prelu_grad_bf16_slabs(*bad) == 0 and lib.rtpose_prelu_grad_bf16_workspace_floats(*bad) == 0, bad


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def grad_args(capi, ptrs=(Z, SLOPE, GA, GB, OUT, DS, WS)):
    """valid arguments of rtpose_prelu_grad_bf16: [z, lz, slope, ga, lga, gb, lgb, out, lout, dslope, workspace,
    workspace_floats, channels, N, H, W, stream]; the layouts are kept alive by the caller's list"""
    z, slope, ga, gb, out, ds, ws = ptrs
    lays = [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(24, H, W, 2, 5), capi.Layout.padded(20, H, W, 0, 1),
            capi.Layout.padded(24, H, W, 1, 3)]
    floats = capi.lib.rtpose_prelu_grad_bf16_workspace_floats(CH, N, H, W)
    return lays, [z, C.byref(lays[0]), slope, ga, C.byref(lays[1]), gb, C.byref(lays[2]), out, C.byref(lays[3]), ds, ws, floats,
                  CH, N, H, W, None]


def fwd_args(capi, ptrs=(Z, SLOPE, OUT)):
    """valid arguments of rtpose_prelu_bf16: [z, lz, slope, y, ly, channels, N, H, W, stream]"""
    z, slope, y = ptrs
    lays = [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(24, H, W, 1, 3)]
    return lays, [z, C.byref(lays[0]), slope, y, C.byref(lays[1]), CH, N, H, W, None]


def _onto(i, j, delta=64):
    """argument i (the bf16 destination) moved to `delta` bytes past argument j: inside its bytes"""
    def f(a, lays):
        a[i] = a[j] + delta
    return f


_arg, _lay = pr.arg_fault, pr.layout_fault

# The rows all four PReLU entry points share (tests/prelu_restate.py) on these entry points' arguments, and the rows that are
# only the bf16 passes': the 2-byte alignment and every overlap of the destination.
# (the destination's first valid element lies (9 * 24 + 3) * 2 = 438 bytes past its base: 430 bytes before the slopes puts
# it 8 bytes into them)
GRAD_FAULTS = pr.shared_faults([("z", 0, 1, 0, False), ("ga", 3, 4, 1, False), ("gb", 5, 6, 2, True), ("out", 7, 8, 3, False)],
                               slope=2, channels=12, workspace=10) + [
    ("gb without a layout", _arg(6, None), "NULL layout (gb)"),
    ("cstride 0", _lay(0, "cstride", 0), "bad layout"),
    ("negative choff", _lay(2, "choff", -1), "bad layout"),
    ("negative lead", _lay(3, "lead", -1), "bad layout"),
    ("ga images shorter than the map", _lay(1, "hs", H - 1), "layout smaller than the map (ga)"),
    ("an odd bf16 base", _arg(7, OUT + 1), "out must be 2-byte aligned"),
    ("out inside z", _onto(7, 0), "overlap those of z"),
    ("out inside ga", _onto(7, 3), "overlap those of ga"),
    ("out inside gb", _onto(7, 5), "overlap those of gb"),
    ("out inside slope", _onto(7, 2, -430), "overlap those of slope"),
    ("no rows", _arg(14, -1), "empty tensor"),
    ("no columns", _arg(15, 0), "empty tensor"),
]

FWD_FAULTS = pr.shared_faults([("z", 0, 1, 0, False), ("y", 3, 4, 1, False)], slope=2, channels=5) + [
    ("bad layout", _lay(1, "hs", 0), "bad layout"),
    ("y images shorter than the map", _lay(1, "hs", H - 1), "layout smaller than the map (y)"),
    ("an odd bf16 base", _arg(3, OUT + 1), "y must be 2-byte aligned"),
    ("y inside z", _onto(3, 0), "overlap those of z"),
    ("y inside slope", _onto(3, 2, -430), "overlap those of slope"),
    ("no rows", _arg(7, 0), "empty tensor"),
    ("no columns", _arg(8, -3), "empty tensor"),
]

refused = pr.refused


@pytest.mark.parametrize("name,fault,text", GRAD_FAULTS, ids=[f[0] for f in GRAD_FAULTS])
def test_prelu_grad_bf16_refuses_on_the_host(capi, name, fault, text):
    lays, a = grad_args(capi)
    fault(a, lays)
    refused(capi, capi.lib.rtpose_prelu_grad_bf16, "prelu_grad_bf16", a, text)


@pytest.mark.parametrize("name,fault,text", FWD_FAULTS, ids=[f[0] for f in FWD_FAULTS])
def test_prelu_bf16_refuses_on_the_host(capi, name, fault, text):
    lays, a = fwd_args(capi)
    fault(a, lays)
    refused(capi, capi.lib.rtpose_prelu_bf16, "prelu_bf16", a, text)


def test_host_checks_pass_valid_arguments(capi):
    """with every host check passed the refusal is the pointer's (fake: no device owns it); gb = NULL needs no layout,
    dslope = NULL no workspace"""
    lib = capi.lib
    lays, a = grad_args(capi)
    assert lib.rtpose_prelu_grad_bf16_slabs(CH, N, H, W) == 2 and a[11] >= 2 * CH
    assert lib.rtpose_prelu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    a[5] = a[6] = None
    assert lib.rtpose_prelu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    a[9] = a[10] = None
    a[11] = 0
    assert lib.rtpose_prelu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    lays, a = fwd_args(capi)
    assert lib.rtpose_prelu_bf16(*a) != 0 and "device memory" in capi.last_error()
    # disjoint channel slices of one fp32 and one bf16 buffer are what a dense block launches: bytes apart, so fine
    lays, a = grad_args(capi)
    a[3] = a[5] = GA
    assert lib.rtpose_prelu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
