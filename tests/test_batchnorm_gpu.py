"""GPU suite of the training-mode BatchNorm passes (header section 2b continued, csrc/batchnorm.hip): rtpose_bn_stats,
rtpose_bn_apply and rtpose_bn_grad on slices of wider buffers whose other channels and gaps hold conv_driver.SENTINEL NaNs -
after every launch they are intact, bit for bit - against tests/bn_restate.py.

Exact sets (integer x and gy: every fp64 sum is exact, tests/test_batchnorm_cpu.py holds them to that): every per-channel
vector - the six save rows, both running statistics, dbias, dweight and the three dx coefficients - equals the numpy
evaluation of the header's fp64 expressions bit for bit (the device's fp64 division and square root are IEEE's), and y and
dx equal the fp32 restatement of the documented operation order, evaluated from the kernel's own vectors, bit for bit.
Random operands, |mean| = 1000 std included: the vectors lie within the bounds bn_restate derives against float64
F.batch_norm autograd, y and dx are again bit for bit from the kernel's own vectors AND within their derived bounds of the
pure float64 result; the ReLU runs use operands whose float64 pre-activations stay outside y's bound of zero, so no mask can
differ.  The worst err / bound of every vector goes through conv_driver.note (profiles/r23_hourglass_train.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_restate as br
import conv_driver as cd
import layout_restate as lr

pytestmark = pytest.mark.gpu

GUARD = 64              # sentinel floats on either side of an output


def sent_buffer(capi, lay, c, values=None):
    """A layout buffer on the host, as uint32: SENTINEL everywhere, `values` float32 [n, ch, h, w] at the valid pixels"""
    a = np.full(cd.npx(capi, lay, c.n, c.h, c.w) * lay.cstride, cd.SENTINEL, dtype=np.uint32)
    return a if values is None else lr.scatter(a, lay, np.ascontiguousarray(values, np.float32).view(np.uint32))


def to_dev(a, dev):
    return torch.from_numpy(a.view(np.int32).copy()).to(dev).view(torch.float32)


def guarded(numel, dev):
    whole = torch.full((numel + 2 * GUARD,), cd.SENTINEL, dtype=torch.int32, device=dev)
    return whole, whole[GUARD:GUARD + numel].view(torch.float32)


def guards_intact(whole, numel):
    bits = cd.np_bits(whole.view(torch.float32))
    return bool((bits[:GUARD] == cd.SENTINEL).all() and (bits[GUARD + numel:] == cd.SENTINEL).all())


def f32(bits):
    return bits.view(np.float32)


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def nchw(bits_nhwc):
    return np.ascontiguousarray(np.transpose(bits_nhwc, (0, 3, 1, 2)))


def vec(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


def run(capi, dev, c, x, gy, w, b, rm, rv, relu, inplace=False, alias=False, want="xwb", running=True):
    """stats, apply and grad of the case: a dict of save [6, ch], rm, rv (float32 arrays or None), y, dx [n, ch, h, w], dw, db,
    coef [3, ch] (or None).  inplace: y onto x's slice (a copy of the buffer); alias: dx onto gy's slice; want: which of
    dx / dweight / dbias are asked for; running: with running statistics."""
    lib, ch = capi.lib, c.channels
    lx, lgy, lout = br.layouts(c)
    stream = capi.current_stream()
    xh = sent_buffer(capi, lx, c, x.numpy())
    xbuf = to_dev(xh, dev)
    ix = lr.index(lx, c.n, c.h, c.w, ch)
    wd, bd_ = vec(w, dev), vec(b, dev)
    rmd, rvd = (vec(rm, dev), vec(rv, dev)) if running else (None, None)
    doubles = lib.rtpose_bn_workspace_doubles(ch, c.n, c.h, c.w)
    slabs = lib.rtpose_bn_slabs(ch, c.n, c.h, c.w)
    assert doubles == slabs * 2 * ch + 2 * ch > 0
    s_whole, save = guarded(br.SAVE_ROWS * ch, dev)
    w_whole, ws = guarded(2 * doubles, dev)
    capi.check(lib.rtpose_bn_stats(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(wd), capi.ptr(bd_), capi.ptr(rmd), capi.ptr(rvd),
                                   br.MOMENTUM, br.EPS, capi.ptr(save), capi.ptr(ws), doubles, ch, c.n, c.h, c.w, stream),
               "rtpose_bn_stats")
    torch.cuda.synchronize()
    assert np.array_equal(cd.np_bits(xbuf), xh), "stats modified x"
    assert guards_intact(s_whole, br.SAVE_ROWS * ch) and guards_intact(w_whole, 2 * doubles), "stats wrote outside save / workspace"
    out = dict(save=f32(cd.np_bits(save)).reshape(br.SAVE_ROWS, ch).copy(),
               rm=rmd.cpu().numpy() if running else None, rv=rvd.cpu().numpy() if running else None)

    # apply
    ly = lx if inplace else lout
    ybuf = to_dev(xh, dev) if inplace else to_dev(sent_buffer(capi, ly, c), dev)
    src = ybuf if inplace else xbuf
    capi.check(lib.rtpose_bn_apply(capi.ptr(src), C.byref(cd.L(capi, lx)), capi.ptr(save), capi.ptr(ybuf), C.byref(cd.L(capi, ly)),
                                   1 if relu else 0, ch, c.n, c.h, c.w, stream), "rtpose_bn_apply")
    torch.cuda.synchronize()
    bits, iy = cd.np_bits(ybuf), lr.index(ly, c.n, c.h, c.w, ch)
    if inplace:
        expect = xh.copy()
        expect[iy] = bits[iy]
        assert np.array_equal(bits, expect), "in place: something besides the valid pixels of the slice changed"
    else:
        assert lr.untouched(bits, iy, cd.SENTINEL), "apply wrote outside the valid pixels of the slice"
        assert np.array_equal(cd.np_bits(xbuf), xh), "apply modified x"
    out["y"] = f32(nchw(bits[iy]))

    # grad
    if gy is None:
        return out
    ld = lgy if alias else lout
    gh = sent_buffer(capi, lgy, c, gy.numpy())
    gbuf = to_dev(gh, dev)
    dbuf = gbuf if alias else to_dev(sent_buffer(capi, ld, c), dev)
    dw_whole, dw = guarded(ch, dev)
    db_whole, db = guarded(ch, dev)
    w_whole, ws = guarded(2 * doubles, dev)
    need_x, need_w, need_b = ("x" in want), ("w" in want), ("b" in want)
    capi.check(lib.rtpose_bn_grad(capi.ptr(xbuf), C.byref(cd.L(capi, lx)), capi.ptr(gbuf), C.byref(cd.L(capi, lgy)), capi.ptr(save),
                                  capi.ptr(wd), 1 if relu else 0, capi.ptr(dbuf) if need_x else None,
                                  C.byref(cd.L(capi, ld)) if need_x else None, capi.ptr(dw) if need_w else None,
                                  capi.ptr(db) if need_b else None, capi.ptr(ws), doubles, ch, c.n, c.h, c.w, stream),
               "rtpose_bn_grad")
    torch.cuda.synchronize()
    assert np.array_equal(cd.np_bits(xbuf), xh), "grad modified x"
    assert np.array_equal(f32(cd.np_bits(save)).reshape(br.SAVE_ROWS, ch).view(np.uint32), out["save"].view(np.uint32)), "grad modified save"
    assert guards_intact(dw_whole, ch) and guards_intact(db_whole, ch) and guards_intact(w_whole, 2 * doubles)
    bits, idx = cd.np_bits(dbuf), lr.index(ld, c.n, c.h, c.w, ch)
    if need_x:
        if alias:
            expect = gh.copy()
            expect[idx] = bits[idx]
            assert np.array_equal(bits, expect), "aliased: something besides the valid pixels of the slice changed"
        else:
            assert lr.untouched(bits, idx, cd.SENTINEL), "grad wrote outside the valid pixels of the slice"
            assert np.array_equal(cd.np_bits(gbuf), gh), "grad modified gy"
        out["dx"] = f32(nchw(bits[idx]))
        tail = f32(cd.np_bits(ws))[4 * slabs * ch:]
        out["coef"] = tail[:3 * ch].reshape(3, ch).copy()
    else:
        assert (bits == (gh if alias else cd.SENTINEL)).all(), "dx = NULL but something was written"
        out["dx"] = out["coef"] = None
    out["dw"] = f32(cd.np_bits(dw)).copy() if need_w else None
    out["db"] = f32(cd.np_bits(db)).copy() if need_b else None
    if not need_w:
        assert (cd.np_bits(dw) == cd.SENTINEL).all(), "dweight = NULL but written"
    if not need_b:
        assert (cd.np_bits(db) == cd.SENTINEL).all(), "dbias = NULL but written"
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def elementwise_from_own_vectors(r, x, gy, relu, what):
    """y and dx bit for bit from the restated operation order on the kernel's own per-channel vectors"""
    want_y = br.apply_restate(x.numpy(), r["save"], relu)
    bad = int((r["y"].view(np.uint32) != want_y.view(np.uint32)).sum())
    assert bad == 0, "%s: y differs from fl(fl(scale x) + shift) in %d of %d elements" % (what, bad, want_y.size)
    if r.get("dx") is not None:
        want_dx = br.dx_restate(x.numpy(), gy.numpy(), r["save"], r["coef"], relu)
        bad = int((r["dx"].view(np.uint32) != want_dx.view(np.uint32)).sum())
        assert bad == 0, "%s: dx differs from (g A - B) - (x - mean) C in %d of %d elements" % (what, bad, want_dx.size)


# ---- 1. exact sets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", br.CASES, ids=br.case_id)
def test_exact_sets_bit_for_bit(capi, cuda, c):
    x, gy = br.exact_operands(c)
    w, b, rm, rv = br.affine(c.channels, True)
    assert br.exact_margin(x, gy) < 2 ** 53
    save, rm1, rv1 = br.stats_restate(x.numpy(), w.numpy(), b.numpy(), rm.numpy(), rv.numpy())
    names = ("mean", "var", "invstd", "scale", "shift", "mean_lo")
    for i, relu in enumerate((False, True)):
        r = run(capi, cuda, c, x, gy, w, b, rm, rv, relu, inplace=bool(i), alias=bool(i))
        for row, name in enumerate(names):
            bad = np.flatnonzero(r["save"][row].view(np.uint32) != save[row].view(np.uint32))
            assert bad.size == 0, "%s: channels %s differ (%r vs %r)" % (name, bad[:8].tolist(), r["save"][row][bad[:3]], save[row][bad[:3]])
        assert same_bits(r["rm"], rm1) and same_bits(r["rv"], rv1), "running statistics"
        db, dw, coef = br.grad_vectors_restate(x.numpy(), gy.numpy(), save, w.numpy(), relu)
        assert same_bits(r["db"], db), "dbias (relu %s)" % relu
        assert same_bits(r["dw"], dw), "dweight (relu %s)" % relu
        assert same_bits(r["coef"], coef), "A, B, C (relu %s)" % relu
        elementwise_from_own_vectors(r, x, gy, relu, "relu %s" % relu)
        # frozen parameters and an input without a gradient: the same values from the launches that remain
        r2 = run(capi, cuda, c, x, gy, w, b, rm, rv, relu, alias=not i, want="x")
        assert r2["dw"] is None and r2["db"] is None and same_bits(r2["dx"], r["dx"]) and same_bits(r2["y"], r["y"])
        r3 = run(capi, cuda, c, x, gy, w, b, rm, rv, relu, alias=bool(i), want="wb", running=False)
        assert r3["dx"] is None and same_bits(r3["dw"], r["dw"]) and same_bits(r3["db"], r["db"])
        assert r3["rm"] is None and same_bits(r3["save"], r["save"]), "save without running statistics"
        r4 = run(capi, cuda, c, x, gy, w, b, rm, rv, relu, want="w")
        assert r4["db"] is None and same_bits(r4["dw"], r["dw"])


# ---- 2. random operands ---------------------------------------------------------------------------------------------------------------
_worst = {}
VECTORS = ("mean", "var", "invstd", "scale", "shift")


def check_random(capi, cuda, c, kind, x, gy, w, b, rm, rv, relu, t, bd):
    r = run(capi, cuda, c, x, gy, w, b, rm, rv, relu)
    again = run(capi, cuda, c, x, gy, w, b, rm, rv, relu, inplace=True, alias=True)
    for k in ("save", "rm", "rv", "y", "dx", "dw", "db", "coef"):
        assert same_bits(r[k], again[k]), "two launches (the second in place / aliased) gave different %s bits" % k
    ratios = {}
    got = dict(zip(VECTORS, r["save"][:5]), running_mean=r["rm"], running_var=r["rv"], dweight=r["dw"], dbias=r["db"])
    want = dict(t, dweight=t["dweight"], dbias=t["dbias"])
    for name, g in got.items():
        err = np.abs(f64(g) - want[name].numpy())
        ratios[name] = float((err / np.maximum(bd[name], 1e-300)).max())
    lo = np.abs(f64(r["save"][0]) + f64(r["save"][5]) - t["mean"].numpy())
    ratios["mean+mean_lo"] = float((lo / (bd["dm"] + 2.0 ** -47 * np.abs(t["mean"].numpy()) + 1e-300)).max())
    elementwise_from_own_vectors(r, x, gy, relu, kind)
    pre = br.apply_restate(x.numpy(), r["save"], False)
    pre64 = (t["scale"].view(1, -1, 1, 1) * x.double() + t["shift"].view(1, -1, 1, 1)).numpy()
    ratios["y"] = float((np.abs(f64(pre) - pre64) / np.maximum(br.y_bound(x.numpy(), t, bd), 1e-300)).max())
    if relu:
        assert ((r["y"] > 0) == (t["y"].numpy() > 0)).all(), "the ReLU masks differ although every float64 y clears its bound"
    # (a zero weight makes dx and its bound exactly zero: 0 / 1e-300)
    ratios["dx"] = float((np.abs(f64(r["dx"]) - t["dx"].numpy()) / np.maximum(br.dx_bound(x.numpy(), gy.numpy(), w.numpy(), t, bd, relu), 1e-300)).max())
    print("bn %s %s relu %s: slabs %d, err / bound %s" % (br.case_id(c), kind, relu, capi.lib.rtpose_bn_slabs(c.channels, c.n, c.h, c.w),
                                                           " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    _worst["%s %s%s" % (br.case_id(c), kind, " relu" if relu else "")] = ratios
    cd.note("bn_bounds.json", _worst)
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, "beyond the derived bound (err / bound): %s" % over


@pytest.mark.parametrize("kind", ["unit", "mean1000std"])
@pytest.mark.parametrize("c", br.CASES, ids=br.case_id)
def test_random_operands(capi, cuda, c, kind):
    x, gy = br.random_operands(c, big_mean=kind == "mean1000std")
    w, b, rm, rv = br.affine(c.channels, False)
    t = br.bn64(x, gy, w, b, rm, rv)
    bd = br.bounds(x.numpy(), gy.numpy(), w.numpy(), b.numpy(), t, rm.numpy(), rv.numpy())
    check_random(capi, cuda, c, kind, x, gy, w, b, rm, rv, False, t, bd)


@pytest.mark.parametrize("c", [c for c in br.CASES if c.n * c.h * c.w * c.channels <= 20000], ids=br.case_id)
def test_random_operands_relu(capi, cuda, c):
    r = br.relu_operands(c)
    assert r is not None, "no seed with a mask margin (tests/test_batchnorm_cpu.py holds every case of this size to one)"
    x, gy, w, b, rm, rv, t, bd, margin = r
    assert margin > 0
    check_random(capi, cuda, c, "relu margin %.3g" % margin, x, gy, w, b, rm, rv, True, t, bd)
