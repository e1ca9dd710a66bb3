"""Host restatement of the bf16 depthwise 3x3 kernels (include/rtpose_mi355x.h section 2b continued:
rtpose_dwconv3x3_bf16_f32, rtpose_dwconv3x3_wgrad_bf16, rtpose_dwconv3x3_dgrad_bf16) and of
train.dwconv3x3(compute_dtype='bf16'), built on tests/dwconv_restate.py by import.

The contract has two rounding points and nothing else: x and gy are rounded to bf16 (nearest even) as they enter; the taps,
every accumulator, the output and both gradients are fp32.  So the emulation is: round to bf16, widen, then the fp32
restatements of dwconv_restate on the widened operands - wgrad_restate (float64 sums; a product of two bf16 values has 16
significant bits and is exact there), dgrad_restate (fp32, the header's order) - and a forward in the header's order:
from the bias, ky = 0, 1, 2 and within a row kx = 0, 1, 2, one rounding per product and one per add.

torch CPU + numpy only: no GPU, and no library call but the refusal tables', which list what the launchers refuse on the host.
"""
import ctypes as C

import numpy as np
import torch

import dwconv_restate as dr
import layout_restate as lr


def round_bf16(a):
    """float32 array / tensor -> the float32 values of its bf16 roundings (nearest even), by torch's own conversion"""
    t = torch.as_tensor(np.asarray(a, np.float32) if not torch.is_tensor(a) else a).float()
    return t.to(torch.bfloat16).float()


def bf16_bits(a):
    """float32 values that ARE bf16 numbers -> their uint16 bits"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def forward_restate(x, weight, stride, bias=None, dtype=np.float32):
    """y [n, c, ho, wo] in `dtype` arithmetic: acc = bias; for ky, kx ascending: acc += x * w, one rounding per product and
    one per add; x's taps outside the map are the zeros of the layout's gap"""
    x = np.asarray(x, np.float32).astype(dtype)
    wt = np.asarray(weight, np.float32).astype(dtype)
    n, c, h, w = x.shape
    ho, wo = dr.out_size(h, w, stride)
    xp = np.zeros((n, c, stride * (ho - 1) + 3, stride * (wo - 1) + 3), dtype)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    b = np.zeros(c, dtype) if bias is None else np.asarray(bias, np.float32).astype(dtype)
    acc = np.broadcast_to(b.reshape(1, c, 1, 1), (n, c, ho, wo)).astype(dtype)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            prod = (v * wt[:, 0, ky, kx].reshape(1, c, 1, 1)).astype(dtype)
            acc = (acc + prod).astype(dtype)
    return acc


def emulate(x, weight, gy, stride):
    """train.dwconv3x3(compute_dtype='bf16') on the host: (y fp32, dx fp32, dw float64 before its one rounding to fp32)"""
    xb, gb = round_bf16(x).numpy(), round_bf16(gy).numpy()
    wt = np.asarray(weight, np.float32)
    n, c, h, w = xb.shape
    y = forward_restate(xb, wt, stride)
    dx = dr.dgrad_restate(gb, wt, h, w, stride)
    dw = dr.wgrad_restate(xb, gb, stride)[0]
    return y, dx, dw


def sums_exact_in_fp64(x, gy, stride):
    """whether every partial sum of the weight gradient's terms, in any order, is a float64 number: all terms are multiples
    of one power of two q and the sum of their magnitudes stays below 2^53 q.  Then the kernel's fixed-order fp64 sum, numpy's
    pairwise one and the true sum are one value, and dw is that value rounded to fp32 once."""
    dw, db, sw, sb = dr.wgrad_restate(x, gy, stride)
    xs, gs = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(gy, np.float64))
    if not xs.any() or not gs.any():
        return True
    # the lowest set bit of any operand: frexp's exponent minus the 8 significant bits of a bf16 value
    qx = np.frexp(xs[xs > 0].min())[1] - 8
    qg = np.frexp(gs[gs > 0].min())[1] - 8
    return bool(sw.max() < 2.0 ** (53 + qx + qg) and sb.max() < 2.0 ** (53 + qg))


# ---- cases of tests/test_dwconv_bf16_gpu.py ----------------------------------------------------------------------------------------------
# The shapes of dwconv_restate.CASES, its slab cases included, with the buffer layouts in bf16 ELEMENTS chosen per alignment
# class: "x8": every bf16 cstride and choff a multiple of 8 on a 16-byte base (what the training path gives: 16-byte pieces);
# "x4": multiples of 4 only (8-byte pieces); "odd": element by element.  The backward kernels take their units of 4 channels
# in the first two (the header says why there are no units of 8) and single channels in the third; the forward's doors ask
# for the first.  dx is fp32: (cstride, choff) multiples of 4 for the wide form.  C = 58 in 64 and C = 6 in 8 leave a last
# unit of fewer live channels than a thread owns.
Case = dr.Case
def _up(v, m):
    return -(-v // m) * m


def _layouts_for(c, path):
    """(x, gy, dx) (cstride, choff) pairs that hold c channels on the load path `path`"""
    if path == "x8":
        return (_up(c, 8), 0), (_up(c + 8, 8), 8), (_up(c + 4, 4), 4)
    if path == "x4":        # multiples of 4 that are no multiples of 8
        return (_up(c + 4, 8) + 4, 4), (_up(c, 8) + 4, 0), (_up(c + 4, 4), 4)
    return ((c + 1) | 1, 1), ((c + 3) | 1, 3), (c + 3, 2)


def _cases():
    out = []
    shapes = [(c.n, c.c, c.h, c.w, c.stride) for c in dr.CASES]
    shapes += [(1, 6, 8, 6, s) for s in (1, 2)]          # C = 6 in 8: one unit of 8 with two dead channels
    seen = set()
    for i, (n, ch, h, w, s) in enumerate(shapes):
        for path in ("x8", "x4", "odd"):
            if (n, ch, h, w, s, path) in seen:
                continue
            seen.add((n, ch, h, w, s, path))
            x, gy, dx = _layouts_for(ch, path)
            out.append(Case(n, ch, h, w, s, x, gy, dx, path))
    return out


CASES = _cases()


def case_id(c):
    return "%s_%s" % (dr.case_id(c), c.tags)


def load_path(c):
    """the largest piece the case's bf16 layouts allow on a 16-byte base: 8, 4 or 1 elements"""
    for mult in (8, 4):
        if all(v % mult == 0 for v in c.x + c.gy):
            return mult
    return 1


def exact_operands(c, seed=0):
    """dwconv_restate's small integers: bf16 numbers already"""
    x, gy, wt = dr.exact_operands(c, seed)
    assert torch.equal(round_bf16(x), x) and torch.equal(round_bf16(gy), gy)
    return x, gy, wt


def random_operands(c, seed=0):
    """dwconv_restate's normal operands with x and gy rounded to bf16; the taps stay fp32"""
    x, gy, wt = dr.random_operands(c, seed)
    return round_bf16(x), round_bf16(gy), wt


# ---- what the launchers refuse on the host -------------------------------------------------------------------------------------------------
R_N, R_C, R_H, R_W, R_S = 2, 16, 5, 7, 2
# 16-byte aligned "device pointers" no refused launch touches
P_IN, P_W, P_B, P_OUT, P_GY, P_DW, P_DB, P_WS, P_DX = ((i + 1) << 24 for i in range(9))


def _lay(capi, c, h, w, gap, choff=0):
    return capi.Layout(*lr.padded(c, h, w, gap, choff))


def forward_args(capi):
    """valid arguments of rtpose_dwconv3x3_bf16_f32: [in, lin, w, bias, out, lout, C, N, H, W, stride, stream]"""
    ho, wo = dr.out_size(R_H, R_W, R_S)
    lays = [_lay(capi, 32, R_H, R_W, 1, 8), _lay(capi, 24, ho, wo, 0, 4)]
    return lays, [P_IN, C.byref(lays[0]), P_W, P_B, P_OUT, C.byref(lays[1]), R_C, R_N, R_H, R_W, R_S, None]


def wgrad_args(capi):
    """valid arguments of rtpose_dwconv3x3_wgrad_bf16: [x, lx, gy, lgy, dw, dbias, workspace, workspace_doubles, C, N, H, W,
    stride, stream]"""
    ho, wo = dr.out_size(R_H, R_W, R_S)
    lays = [_lay(capi, 19, R_H, R_W, 1, 2), _lay(capi, 17, ho, wo, 0, 1)]
    doubles = dr.workspace_doubles(R_C, R_N, R_H, R_W, R_S)
    return lays, [P_IN, C.byref(lays[0]), P_GY, C.byref(lays[1]), P_DW, P_DB, P_WS, doubles, R_C, R_N, R_H, R_W, R_S, None]


def dgrad_args(capi):
    """valid arguments of rtpose_dwconv3x3_dgrad_bf16: [gy, lgy, w, dx, ldx, C, N, H, W, stride, stream]"""
    ho, wo = dr.out_size(R_H, R_W, R_S)
    lays = [_lay(capi, 17, ho, wo, 1, 1), _lay(capi, 20, R_H, R_W, 0, 3)]
    return lays, [P_GY, C.byref(lays[0]), P_W, P_DX, C.byref(lays[1]), R_C, R_N, R_H, R_W, R_S, None]


def _arg(i, v):
    def f(a, lays):
        a[i] = v
    return f


def _field(j, field, v):
    def f(a, lays):
        setattr(lays[j], field, v)
    return f


def _no_gap(j):
    def f(a, lays):
        lays[j].lead = lays[j].ws      # a row of lead but not the pixel before the first one
    return f


def _past(j):
    def f(a, lays):
        lays[j].choff = lays[j].cstride - R_C + 1
    return f


def _huge(first):
    """a map above the launch limit in layouts that hold it; N, H, W start at index `first`"""
    def f(a, lays):
        for lay in lays:
            lay.ws, lay.hs, lay.lead = (1 << 15) + 1, (1 << 16) + 1, (1 << 15) + 2
        a[first:first + 3] = [1, 1 << 16, 1 << 15]
    return f


FORWARD_FAULTS = [
    ("null in", _arg(0, None), "NULL buffer (in)"),
    ("null lin", _arg(1, None), "NULL layout (in)"),
    ("null w", _arg(2, None), "NULL buffer (w or bias)"),
    ("null bias", _arg(3, None), "NULL buffer (w or bias)"),
    ("null out", _arg(4, None), "NULL buffer (out)"),
    ("null lout", _arg(5, None), "NULL layout (out)"),
    ("no channels", _arg(6, 0), "empty tensor"),
    ("no images", _arg(7, 0), "empty tensor"),
    ("no rows", _arg(8, -1), "empty tensor"),
    ("no columns", _arg(9, 0), "empty tensor"),
    ("stride 3", _arg(10, 3), "stride must be 1 or 2"),
    ("stride 0", _arg(10, 0), "stride must be 1 or 2"),
    ("C = 12", _arg(6, 12), "C must be a multiple of 8"),
    ("in without a gap", _no_gap(0), "needs a zero gap of at least 1"),
    ("in bad layout", _field(0, "cstride", 0), "bad layout (in)"),
    ("out bad layout", _field(1, "lead", -1), "bad layout (out)"),
    ("in slice past cstride", _past(0), "in slice exceeds cstride"),
    ("out slice past cstride", _past(1), "out slice exceeds cstride"),
    ("out rows shorter than the map", _field(1, "ws", 3), "layout smaller than the map (out)"),
    ("in choff 4", _field(0, "choff", 4), "16-byte aligned"),
    ("in cstride 36", _field(0, "cstride", 36), "16-byte aligned"),
    ("out choff 2", _field(1, "choff", 2), "16-byte aligned"),
    ("in base off 8 bytes", _arg(0, P_IN + 8), "16-byte aligned"),
    ("out base off 4 bytes", _arg(4, P_OUT + 4), "16-byte aligned"),
    ("above the launch limit", _huge(7), "above the launch limit"),
]

WGRAD_FAULTS = [
    ("null x", _arg(0, None), "NULL buffer (x)"),
    ("null lx", _arg(1, None), "NULL layout (x)"),
    ("null gy", _arg(2, None), "NULL buffer (gy)"),
    ("null lgy", _arg(3, None), "NULL layout (gy)"),
    ("null dw", _arg(4, None), "NULL buffer (dw)"),
    ("no workspace", _arg(6, None), "NULL workspace"),
    ("workspace off 4 bytes", _arg(6, P_WS + 4), "8-byte aligned"),
    ("workspace one double short", lambda a, lays: a.__setitem__(7, a[7] - 1), "rtpose_dwconv3x3_wgrad_workspace_doubles"),
    ("no channels", _arg(8, 0), "empty tensor"),
    ("negative channels", _arg(8, -4), "empty tensor"),
    ("no images", _arg(9, 0), "empty tensor"),
    ("no rows", _arg(10, 0), "empty tensor"),
    ("stride 3", _arg(12, 3), "stride must be 1 or 2"),
    ("stride 0", _arg(12, 0), "stride must be 1 or 2"),
    ("x without a gap", _no_gap(0), "needs a zero gap of at least 1"),
    ("x bad layout", _field(0, "hs", 0), "bad layout (x)"),
    ("x slice past cstride", _past(0), "x slice exceeds cstride"),
    ("gy slice past cstride", _past(1), "gy slice exceeds cstride"),
    ("gy rows shorter than the map", _field(1, "ws", 3), "layout smaller than the map (gy)"),
    ("an odd x base", _arg(0, P_IN + 1), "x must be 2-byte aligned"),
    ("an odd gy base", _arg(2, P_GY + 3), "gy must be 2-byte aligned"),
    ("above the launch limit", _huge(9), "above the launch limit"),
]

DGRAD_FAULTS = [
    ("null gy", _arg(0, None), "NULL buffer (gy)"),
    ("null lgy", _arg(1, None), "NULL layout (gy)"),
    ("null w", _arg(2, None), "NULL buffer (w)"),
    ("null dx", _arg(3, None), "NULL buffer (dx)"),
    ("null ldx", _arg(4, None), "NULL layout (dx)"),
    ("no channels", _arg(5, 0), "empty tensor"),
    ("no columns", _arg(8, 0), "empty tensor"),
    ("stride 3", _arg(9, 3), "stride must be 1 or 2"),
    ("gy without a gap", _no_gap(0), "needs a zero gap of at least 1"),
    ("gy bad layout", _field(0, "choff", -1), "bad layout (gy)"),
    ("gy slice past cstride", _past(0), "gy slice exceeds cstride"),
    ("dx slice past cstride", _past(1), "dx slice exceeds cstride"),
    ("dx rows shorter than the map", _field(1, "ws", R_W - 1), "layout smaller than the map (dx)"),
    ("an odd gy base", _arg(0, P_GY + 1), "gy must be 2-byte aligned"),
    ("above the launch limit", _huge(6), "above the launch limit"),
]

ENTRY_POINTS = {
    "rtpose_dwconv3x3_bf16_f32": ("dwconv3x3_bf16_f32", forward_args, FORWARD_FAULTS),
    "rtpose_dwconv3x3_wgrad_bf16": ("dwconv3x3_wgrad_bf16", wgrad_args, WGRAD_FAULTS),
    "rtpose_dwconv3x3_dgrad_bf16": ("dwconv3x3_dgrad_bf16", dgrad_args, DGRAD_FAULTS),
}


def refused(capi, fn, who, a, text):
    rc = fn(*a)
    err = capi.last_error()
    assert rc == -1, (rc, err)                                   # RTPOSE_E_INVAL, not a HIP error
    assert text in err and err.startswith(who + ":"), err
    assert "device memory" not in err                            # returned before the pointers were looked at
