"""CPU suite of rtpose_relu_grad_bf16 (header section 2b, csrc/act_grad_bf16.hip): the restatement of
tests/act_grad_bf16_restate.py against torch.where on bfloat16 tensors over every bit pattern of y, and every refusal of the
launcher, reached through the library without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import act_grad_bf16_restate as ar


def as_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def bits_of(t):
    return t.view(torch.int16).numpy().view(np.uint16)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_is_torch_where_on_every_pattern_of_y():
    y = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    for gy in (np.full(1 << 16, 0x3FC0, dtype=np.uint16),                      # 1.5 everywhere
               np.full(1 << 16, 0x7FC7, dtype=np.uint16),                      # a NaN with a payload
               np.full(1 << 16, 0xFF80, dtype=np.uint16),                      # -Inf
               ((y.astype(np.uint32) * 40503 + 12345) & 0xFFFF).astype(np.uint16)):    # every pattern of gy once, permuted
        want = torch.where(as_bf16(y) > 0, as_bf16(gy), torch.zeros((), dtype=torch.bfloat16))
        got = ar.relu_grad_bf16_bits(y, gy)
        assert np.array_equal(got, bits_of(want))
    assert len(set(((y.astype(np.uint32) * 40503 + 12345) & 0xFFFF).tolist())) == 1 << 16


def test_the_classes_of_y():
    g = np.full(ar.Y_SPECIAL.size, 0x7FC7, dtype=np.uint16)
    out = ar.relu_grad_bf16_bits(ar.Y_SPECIAL, g)
    passes = {0x7F80, 0x0001, 0x007F, 0x0080, 0x7F7F, 0x3F80}      # +Inf, the subnormals, the normals, 1
    for yb, ob in zip(ar.Y_SPECIAL.tolist(), out.tolist()):
        assert ob == (0x7FC7 if yb in passes else 0x0000), hex(yb)
    # 2^-134, the largest fp32 a conv's store rounds to a bf16 +0 (round to nearest even: the tie goes to the even 0x0000)
    tie = torch.tensor([2.0 ** -134, 2.0 ** -134 + 2.0 ** -149], dtype=torch.float32)     # (the next fp32 subnormal)
    assert bits_of(tie.to(torch.bfloat16)).tolist() == [0x0000, 0x0001]


def test_the_grid_of_the_gpu_suite_has_both_paths():
    grid = [c for ch in ar.CHANNELS for off in ar.CHOFFS for c in ar.cases(ch, off)]
    assert len(grid) == 5 * 3 * 18
    assert {ar.is_vector(c) for c in grid} == {True, False}
    assert any(ar.is_vector(c) and c.channels % 8 for c in grid), "a vector launch with a partial last unit"
    for c in grid:
        assert c.choff + c.channels <= ar.CSTRIDE
        assert c.gaps[0] != c.gaps[1]
        y, gy = ar.operands(c)
        assert set(ar.Y_SPECIAL.tolist()) <= set(y.reshape(-1).tolist())
        assert set(ar.GY_SPECIAL.tolist()) <= set(gy.reshape(-1).tolist())
        assert not (gy == ar.SENTINEL16).any()
        out = ar.relu_grad_bf16_bits(y, gy)
        assert set(ar.GY_SPECIAL.tolist()) <= set(out.reshape(-1).tolist()), "every special gy passes somewhere"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
Y, GY, OUT = 1 << 20, 2 << 20, 3 << 20          # 16-byte aligned "device pointers" a megabyte apart that no refused launch touches
CH = 19
N, H, W = 2, 9, 7


def args(capi):
    """valid arguments but for the pointers: [y, ly, gy, lgy, out, lout, channels, N, H, W, stream]; the caller keeps the layouts"""
    lays = [capi.Layout.padded(24, H, W, 1, 4), capi.Layout.padded(24, H, W, 3, 5), capi.Layout.padded(20, H, W, 0, 1)]
    return lays, [Y, C.byref(lays[0]), GY, C.byref(lays[1]), OUT, C.byref(lays[2]), CH, N, H, W, None]


def _arg(i, v):
    def f(a, lays):
        a[i] = v
    return f


def _lay(j, field, v):
    def f(a, lays):
        setattr(lays[j], field, v)
    return f


def _out_into_gy(shift_elems, **fields):
    """out in gy's buffer, `shift_elems` elements on, in gy's layout but for `fields`"""
    def f(a, lays):
        lays[2].cstride, lays[2].choff, lays[2].ws, lays[2].hs, lays[2].lead = (lays[1].cstride, lays[1].choff, lays[1].ws,
                                                                                lays[1].hs, lays[1].lead)
        for k, v in fields.items():
            setattr(lays[2], k, v)
        a[4] = GY + 2 * shift_elems
    return f


FAULTS = [
    ("null y", _arg(0, None), "NULL buffer (y)"),
    ("null gy", _arg(2, None), "NULL buffer (gy)"),
    ("null out", _arg(4, None), "NULL buffer (out)"),
    ("null ly", _arg(1, None), "NULL layout (y)"),
    ("null lgy", _arg(3, None), "NULL layout (gy)"),
    ("null lout", _arg(5, None), "NULL layout (out)"),
    ("no channels", _arg(6, 0), "empty tensor"),
    ("negative channels", _arg(6, -3), "empty tensor"),
    ("no images", _arg(7, 0), "empty tensor"),
    ("no rows", _arg(8, 0), "empty tensor"),
    ("no columns", _arg(9, -1), "empty tensor"),
    ("cstride 0", _lay(0, "cstride", 0), "bad layout"),
    ("negative choff", _lay(1, "choff", -1), "bad layout"),
    ("negative lead", _lay(2, "lead", -1), "bad layout"),
    ("y slice past cstride", _lay(0, "choff", 6), "y slice exceeds cstride"),
    ("gy slice past cstride", _lay(1, "choff", 6), "gy slice exceeds cstride"),
    ("out slice past cstride", _lay(2, "choff", 2), "out slice exceeds cstride"),
    ("y rows shorter than the map", _lay(0, "ws", W - 1), "layout smaller than the map"),
    ("gy images shorter than the map", _lay(1, "hs", H - 1), "layout smaller than the map"),
    ("out rows shorter than the map", _lay(2, "ws", W - 1), "layout smaller than the map"),
    ("odd y", _arg(0, Y + 1), "2-byte aligned"),
    ("odd gy", _arg(2, GY + 1), "2-byte aligned"),
    ("odd out", _arg(4, OUT + 1), "2-byte aligned"),
    ("out one element into gy", _out_into_gy(1), "out overlaps gy"),
    ("out one pixel into gy", _out_into_gy(24), "out overlaps gy"),
    ("out on gy's base, channels overlapping", _out_into_gy(0, choff=4), "out overlaps gy"),
    ("out on gy's base, another row stride", _out_into_gy(0, ws=W + 4), "out overlaps gy"),
    ("out into y", lambda a, lays: a.__setitem__(4, Y + 2 * 24 * 40), "out overlaps y"),
]


@pytest.mark.parametrize("name,fault,text", FAULTS, ids=[f[0] for f in FAULTS])
def test_relu_grad_bf16_refuses_on_the_host(capi, name, fault, text):
    lays, a = args(capi)
    fault(a, lays)
    rc = capi.lib.rtpose_relu_grad_bf16(*a)
    assert rc == -1, (name, rc, capi.last_error())            # RTPOSE_E_INVAL, not a HIP error
    assert text in capi.last_error() and capi.last_error().startswith("relu_grad_bf16:"), (name, capi.last_error())
    assert "device memory" not in capi.last_error()           # returned before the pointers were looked at


def test_host_checks_pass_valid_arguments(capi):
    """with every host check passed the refusal is the pointer's (fake: no device owns it)"""
    lib = capi.lib
    lays, a = args(capi)
    assert lib.rtpose_relu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    # in place: out names gy's slice
    lays, a = args(capi)
    a[4], a[5] = a[2], a[3]
    assert lib.rtpose_relu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    # channel slices of one buffer that do not meet
    lays, a = args(capi)
    _out_into_gy(0, choff=0, cstride=48)(a, lays)
    lays[1].cstride, lays[1].choff = 48, 24
    assert lib.rtpose_relu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    # bases that are 2-byte but not 16-byte aligned are the element path's, not a refusal
    lays, a = args(capi)
    a[0], a[2], a[4] = Y + 2, GY + 6, OUT + 14
    assert lib.rtpose_relu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()


def test_grid_limits(capi):
    lib = capi.lib
    # a map above the launch limit of 2^31 - 256 pixels, in layouts that hold it
    lays, a = args(capi)
    for lay in lays:
        lay.ws, lay.hs, lay.lead = 1 << 15, 1 << 16, 0
    a[0], a[2], a[4] = 1 << 20, 1 << 50, 1 << 56
    a[7:10] = [1, 1 << 16, 1 << 15]
    assert lib.rtpose_relu_grad_bf16(*a) == -1 and "above the launch limit" in capi.last_error()
    # more than 65535 tiles of 64 channel units: 8 channels a unit where everything is 16-byte aligned, 1 where not
    wide = 64 * 8 * 65535
    lays = [capi.Layout.dense(wide + 8, 1, 1) for _ in range(3)]
    a = [1 << 20, C.byref(lays[0]), 1 << 50, C.byref(lays[1]), 1 << 56, C.byref(lays[2]), wide, 1, 1, 1, None]
    assert lib.rtpose_relu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
    a[6] = wide + 1
    assert lib.rtpose_relu_grad_bf16(*a) == -1 and "grid too large" in capi.last_error()
    a[0] += 2
    a[6] = 64 * 65535 + 1
    assert lib.rtpose_relu_grad_bf16(*a) == -1 and "grid too large" in capi.last_error()
    a[6] = 64 * 65535
    assert lib.rtpose_relu_grad_bf16(*a) != 0 and "device memory" in capi.last_error()
