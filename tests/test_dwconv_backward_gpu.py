"""GPU suite of the depthwise 3x3 backward kernels (header section 2b continued, csrc/dwconv_backward.hip):
rtpose_dwconv3x3_wgrad and rtpose_dwconv3x3_dgrad at both strides on slices of wider buffers whose other channels hold
conv_driver.SENTINEL NaNs - after every launch they are intact, bit for bit - against tests/dwconv_restate.py, which
tests/test_dwconv_backward_cpu.py holds to torch's float64 autograd.

The slices' own channels are zero in the gaps the kernels may read (x's around the map for the weight gradient, gy's for
the data gradient); gy's gaps hold the NaN too for the weight gradient, which reads gy at its valid pixels only; dx's
buffer, the workspace, dw and dbias are NaN-filled with guards on either side.

Exact sets (small integers: every partial sum is exact): dw and dbias == fp32 of the float64 sums, bit for bit.
Random operands: dw and dbias within 2^-24 |v| + (P_out + 8) 2^-53 sum |terms| of float64 (the header's bound); dx bit for
bit the fp32 restatement in the header's order of operations, on both kinds of operands.  Two runs give equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_driver as cd
import dwconv_restate as dr
import layout_restate as lr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel words on either side of an output


def slice_buffer(capi, lay, n, h, w, c, values=None, zero_gaps=True):
    """A layout buffer on the host, as uint32: SENTINEL everywhere but in the slice's own channels, which are zero at every
    pixel if `zero_gaps` (SENTINEL too otherwise) and hold `values` float32 [n, c, h, w] at the valid pixels"""
    a = np.full(cd.npx(capi, lay, n, h, w) * lay.cstride, cd.SENTINEL, dtype=np.uint32)
    if zero_gaps:
        a.reshape(-1, lay.cstride)[:, lay.choff:lay.choff + c] = 0
    return a if values is None else lr.scatter(a, lay, np.ascontiguousarray(values, np.float32).view(np.uint32))


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32).copy()).to(dev).view(torch.float32)


def guarded(words, dev):
    whole = torch.full((words + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + words].view(torch.float32)


def guards_intact(whole, words):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + words:] == cd.SENTINEL).all())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def run_wgrad(capi, dev, c, x, gy, bias=True, gap_x=1):
    """(dw float32 [c, 1, 3, 3], dbias float32 [c] or None)"""
    lib = capi.lib
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    lx, lgy, _ = dr.layouts(c, gap_x=gap_x, gap_gy=2)
    xh = slice_buffer(capi, lx, c.n, c.h, c.w, c.c, x.numpy())
    gh = slice_buffer(capi, lgy, c.n, ho, wo, c.c, gy.numpy(), zero_gaps=False)
    xbuf, gbuf = to_dev(xh, dev), to_dev(gh, dev)
    doubles = lib.rtpose_dwconv3x3_wgrad_workspace_doubles(c.c, c.n, c.h, c.w, c.stride)
    slabs = lib.rtpose_dwconv3x3_wgrad_slabs(c.c, c.n, c.h, c.w, c.stride)
    assert doubles == slabs * dr.TERMS * c.c > 0 and (slabs - 1) * dr.slab_geometry(c.n, c.h, c.w, c.stride)[0] < c.n * ho * wo
    dw_whole, dw = guarded(c.c * 9, dev)
    db_whole, db = guarded(c.c, dev)
    ws_whole, ws = guarded(2 * doubles, dev)
    capi.check(lib.rtpose_dwconv3x3_wgrad(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(gbuf), C.byref(cd.L(capi, lgy)), capi.ptr(dw),
                                          capi.ptr(db) if bias else None, capi.ptr(ws), doubles, c.c, c.n, c.h, c.w, c.stride,
                                          capi.current_stream()), "rtpose_dwconv3x3_wgrad")
    torch.cuda.synchronize()
    assert np.array_equal(cd.np_bits(xbuf), xh) and np.array_equal(cd.np_bits(gbuf), gh), "wgrad modified an input"
    assert guards_intact(dw_whole, c.c * 9) and guards_intact(db_whole, c.c) and guards_intact(ws_whole, 2 * doubles)
    if not bias:
        assert (cd.np_bits(db) == cd.SENTINEL).all(), "dbias = NULL but written"
    return cd.np_bits(dw).view(np.float32).reshape(c.c, 1, 3, 3).copy(), cd.np_bits(db).view(np.float32).copy() if bias else None


def run_dgrad(capi, dev, c, gy, wt, gap_gy=1):
    """dx float32 [n, c, h, w]"""
    lib = capi.lib
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    _, lgy, ldx = dr.layouts(c, gap_gy=gap_gy, gap_dx=1)
    gh = slice_buffer(capi, lgy, c.n, ho, wo, c.c, gy.numpy())
    gbuf = to_dev(gh, dev)
    dbuf = to_dev(slice_buffer(capi, ldx, c.n, c.h, c.w, c.c, zero_gaps=False), dev)
    w_whole, w9 = guarded(9 * c.c, dev)
    w9.copy_(torch.from_numpy(dr.tap_major(wt.numpy())).reshape(-1))
    w9h = cd.np_bits(w9)
    capi.check(lib.rtpose_dwconv3x3_dgrad(capi.ptr(gbuf), C.byref(cd.L(capi, lgy)), capi.ptr(w9), capi.ptr(dbuf), C.byref(cd.L(capi, ldx)),
                                          c.c, c.n, c.h, c.w, c.stride, capi.current_stream()), "rtpose_dwconv3x3_dgrad")
    torch.cuda.synchronize()
    assert np.array_equal(cd.np_bits(gbuf), gh) and np.array_equal(cd.np_bits(w9), w9h) and guards_intact(w_whole, 9 * c.c)
    bits, idx = cd.np_bits(dbuf), lr.index(ldx, c.n, c.h, c.w, c.c)
    assert lr.untouched(bits, idx, cd.SENTINEL), "dgrad wrote outside the valid pixels of the slice"
    return np.ascontiguousarray(np.transpose(bits[idx], (0, 3, 1, 2))).view(np.float32)


@pytest.mark.parametrize("c", dr.SLAB_CASES, ids=dr.case_id)
def test_slab_cases_by_the_query(capi, cuda, c):
    slabs = capi.lib.rtpose_dwconv3x3_wgrad_slabs(c.c, c.n, c.h, c.w, c.stride)
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    assert capi.lib.rtpose_dwconv3x3_wgrad_workspace_doubles(c.c, c.n, c.h, c.w, c.stride) == slabs * dr.TERMS * c.c
    slab = dr.SLAB_UNIT            # fewer than 1024 slabs: 64 pixels each
    assert slabs == -(-c.n * ho * wo // slab) >= 3
    assert dr.slab_facts(c, slab, slabs) == dict(slabs=slabs, ragged=True, inside=True, at_image=True)


@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_exact_sets_bit_for_bit(capi, cuda, c):
    x, gy, wt = dr.exact_operands(c)
    dw64, db64, sw, sb = dr.wgrad_restate(x.numpy(), gy.numpy(), c.stride)
    assert max(sw.max(), sb.max()) < 2 ** 53
    dw, db = run_wgrad(capi, cuda, c, x, gy)
    assert same_bits(dw, dw64.astype(np.float32)), "dw"
    assert same_bits(db, db64.astype(np.float32)), "dbias"
    dw2, db2 = run_wgrad(capi, cuda, c, x, gy, bias=False, gap_x=2)
    assert db2 is None and same_bits(dw2, dw), "dw without dbias, a wider gap"
    dx = run_dgrad(capi, cuda, c, gy, wt)
    assert same_bits(dx, dr.dgrad_restate(gy.numpy(), wt.numpy(), c.h, c.w, c.stride)), "dx"
    assert np.array_equal(dx.astype(np.float64), dr.autograd64(x, wt, gy, c.stride)[1].numpy())


_worst = {}


@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_random_operands(capi, cuda, c):
    x, gy, wt = dr.random_operands(c)
    ho, wo = dr.out_size(c.h, c.w, c.stride)
    p_out = c.n * ho * wo
    dw64, db64, sw, sb = dr.wgrad_restate(x.numpy(), gy.numpy(), c.stride)
    dw, db = run_wgrad(capi, cuda, c, x, gy)
    dw2, db2 = run_wgrad(capi, cuda, c, x, gy, gap_x=2)
    assert same_bits(dw, dw2) and same_bits(db, db2), "two launches gave different bits"
    rw = np.abs(dw.astype(np.float64) - dw64) / np.maximum(dr.wgrad_bound(dw64, sw, p_out), 1e-300)
    rb = np.abs(db.astype(np.float64) - db64) / np.maximum(dr.wgrad_bound(db64, sb, p_out), 1e-300)
    dx = run_dgrad(capi, cuda, c, gy, wt)
    dx2 = run_dgrad(capi, cuda, c, gy, wt, gap_gy=2)
    assert same_bits(dx, dx2), "two launches gave different bits"
    want = dr.dgrad_restate(gy.numpy(), wt.numpy(), c.h, c.w, c.stride)
    bad = int((dx.view(np.uint32) != want.view(np.uint32)).sum())
    print("dwconv backward %s: slabs %d, err / bound dw %.3g dbias %.3g; dx differs in %d of %d"
          % (dr.case_id(c), capi.lib.rtpose_dwconv3x3_wgrad_slabs(c.c, c.n, c.h, c.w, c.stride), rw.max(), rb.max(), bad, want.size))
    _worst[dr.case_id(c)] = {"dw": float(rw.max()), "dbias": float(rb.max())}
    cd.note("dwconv_backward_bounds.json", _worst)
    assert rw.max() <= 1.0 and rb.max() <= 1.0, "beyond the header's bound (err / bound): dw %g dbias %g" % (rw.max(), rb.max())
    assert bad == 0, "dx differs from the fp32 restatement in %d of %d elements" % (bad, want.size)


def test_refusals(capi, cuda):
    c = dr.CASES[3]
    assert (c.n, c.c, c.h, c.w, c.stride) == (2, 3, 5, 7, 2)
    bufs = [torch.zeros(1 << 16, dtype=torch.float64, device=cuda) for _ in range(7)]
    for what, rc in dr.host_refusals(capi, c, *[capi.ptr(b) for b in bufs]):
        assert rc == -1, what                                      # RTPOSE_E_INVAL
        assert capi.last_error(), what
    torch.cuda.synchronize()
    assert all(not b.any() for b in bufs), "a refused call wrote"
    # host memory in place of device memory is refused as well, before any launch
    lx, lgy, ldx = (C.byref(cd.L(capi, l)) for l in dr.layouts(c))
    host = np.zeros(1 << 16, np.float64)
    doubles = dr.workspace_doubles(c.c, c.n, c.h, c.w, c.stride)
    p = [capi.ptr(b) for b in bufs]
    assert capi.lib.rtpose_dwconv3x3_wgrad(capi.ptr(host), lx, p[1], lgy, p[2], p[3], p[4], doubles, c.c, c.n, c.h, c.w, c.stride,
                                           capi.current_stream()) == -1
    assert capi.lib.rtpose_dwconv3x3_dgrad(p[1], lgy, p[5], capi.ptr(host), ldx, c.c, c.n, c.h, c.w, c.stride, capi.current_stream()) == -1
