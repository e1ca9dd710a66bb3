"""The one driver of the pointwise-chain launcher tests (rtpose_pw_fused, rtpose_pw_fused_bf16, rtpose_pw_head,
rtpose_pw_head_bf16, rtpose_unit_bf16), modelled on tests/conv_driver.py: a case of tests/pw_restate.py and its operands
become device buffers, one launch, and host-read bits.

  * Inputs are built ON THE HOST (conv_slices.scatter_nchw / widen): no conversion kernel stands between the test and
    the kernel under test.  Two forms: 'compact', and 'slice' - the same data as a slice of a wider pixel at a nonzero
    16-byte aligned choff, finite +-2^10..2^11 decoys in the other channels of the real pixels, ZERO gaps (the header
    makes the gap the depthwise conv's padding).
  * Every word of an output buffer holds a NaN sentinel before the launch, except where the output buffer is also the
    input (the in-place rtpose_unit_bf16 form): there the pre-launch bits are kept and compared.
  * After the launch the bits are read on the host through lr.index / lr.index_map; `check` compares the written words
    with the restatement under ==, requires them finite, and requires every other word untouched, bit for bit.

Only the weights go through the library's packers.  Importing this module touches neither the GPU nor the library."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

import conv_driver as cd
import conv_slices as cs
import layout_restate as lr
import pw_restate as pr

SENTINEL = {"f32": cd.SENTINEL, "bf16": cd.SENTINEL >> 16}      # quiet NaNs with a recognisable payload
UNIT = {"f32": 4, "bf16": 8}                                    # elements of 16 bytes
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
BITS = {"f32": torch.int32, "bf16": torch.int16}


def up(v, m):
    return (v + m - 1) // m * m


def to_bits(values, kind):
    """float64 values (exact in the element type) -> the bits the kernel must store"""
    f = np.ascontiguousarray(values, dtype=np.float32)
    return f.view(np.uint32) if kind == "f32" else lr.bf16_rne(f)


def host_bits(t):
    """a device buffer of int32 / int16 words -> unsigned numpy bits"""
    t = t.cpu()
    return t.numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint16)


def values(bits, idx):
    """the words at offsets idx [n, h, w, c] as values: [n, c, h, w] fp32 (CPU tensor)"""
    v = bits[idx]
    f = v.view(np.float32) if v.dtype == np.uint32 else lr.bf16_to_f32(v)
    return torch.from_numpy(np.ascontiguousarray(np.transpose(f, (0, 3, 1, 2))))


def sentinel_buffer(numel, kind, dev):
    return torch.full((numel,), SENTINEL[kind], dtype=BITS[kind], device=dev)


def unchanged(bits, before, written):
    """lr.untouched for a buffer that had contents: every word outside `written` still holds its pre-launch bits"""
    mask = np.ones(bits.shape[0], dtype=bool)
    for w in written:
        mask[np.asarray(w, dtype=np.int64).ravel()] = False
    return bool(np.array_equal(bits[mask], before[mask]))


def nhwc(v):
    return np.ascontiguousarray(np.transpose(v, (0, 2, 3, 1)))


def i32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def f32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ---- input -------------------------------------------------------------------------------------------------------------------
def shuffled_planes(x, kind, rng, spare=3):
    """x [n, K, h, w] -> (x_phys [n, Cp, h, w], plane offsets [K / unit]): the 16-byte planes of K at shuffled plane slots of
    a wider pixel, decoys in the slots nobody reads"""
    u = UNIT[kind]
    n, K, h, w = x.shape
    npl = K // u
    pos = rng.permutation(npl + spare)[:npl].astype(np.int64) * u
    gen = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    xp = cs.decoys((n, (npl + spare) * u, h, w), gen, torch.float64).numpy()
    xp[:, pr.plane_channels(pos, u)] = x
    return xp, pos


def input_buffer(capi, kind, x_phys, pad, form, seed=0):
    """x_phys [n, Cp, h, w] float64 -> (host buffer of the element type, its lr.Lay): compact, or a slice at choff = 16 bytes
    of a pixel 32 bytes wider"""
    n, cp, h, w = x_phys.shape
    lay = lr.padded(cp, h, w, pad) if pad else lr.dense(cp, h, w)
    buf = cs.scatter_nchw(torch.from_numpy(x_phys), lay, cd.npx(capi, lay, n, h, w), DT[kind])
    if form == "slice":
        buf, lay = cs.widen(buf, lay, n, h, w, 2 * UNIT[kind], UNIT[kind], seed)
    else:
        assert form == "compact"
    return buf, lay


# ---- weights (the library's packers) ----------------------------------------------------------------------------------------------
def pack_pw(capi, dev, kind, w, b, K, coutp, keep):
    """w [cout, K], b [cout] -> (packed matrix, packed bias) on the device; columns past cout are zero"""
    lib, stream = capi.lib, capi.current_stream()
    cout = w.shape[0]
    wd, bd = f32(dev, w), f32(dev, b)
    bp = torch.zeros(coutp, device=dev)
    if kind == "f32":
        wp = torch.zeros(lib.rtpose_packed_pw_floats(K, coutp) + 64 * coutp, device=dev)
        capi.check(lib.rtpose_pack_pw_weights(capi.ptr(wd), capi.ptr(bd), cout, K, None, K, coutp, 0, capi.ptr(wp), capi.ptr(bp),
                                              stream))
    else:
        wp = torch.zeros(lib.rtpose_packed_pw_bytes_bf16(K, coutp) // 2, dtype=torch.int16, device=dev)
        cols = np.full(coutp, -1, dtype=np.int32)
        cols[:cout] = np.arange(cout)
        cm = i32(dev, cols)
        capi.check(lib.rtpose_pack_pw_weights_bf16(capi.ptr(wd), capi.ptr(bd), cout, K, None, K, coutp, capi.ptr(cm), coutp, 0,
                                                   capi.ptr(wp), capi.ptr(bp), stream))
    torch.cuda.synchronize()
    keep += [wp, bp]
    return wp, bp


def pack_taps(dev, dw, keep):
    """(taps [K, 3, 3], bias [K]) -> device [9][K] tap-major and [K]"""
    t, tb = f32(dev, dw[0].reshape(dw[0].shape[0], 9).T), f32(dev, dw[1])
    keep += [t, tb]
    return t, tb


# ---- the three launches ---------------------------------------------------------------------------------------------------------
def _finish(P, capi, dev, okind, lout, cso, n, h, w):
    P.okind, P.lout, P.numel = okind, lout, cd.npx(capi, lout, n, h, w) * cso
    P.dev, P.capi, P.before = dev, capi, None
    return P


def fresh(P):
    """a new output buffer: sentinel words, or (in place) the pre-launch contents of the stage buffer"""
    if P.before is not None:
        return P.stage0.clone()
    return sentinel_buffer(P.numel, P.okind, P.dev)


def prepare_fused(capi, dev, case, o, form):
    """rtpose_pw_fused / rtpose_pw_fused_bf16"""
    kind, n, h, w, K, cout = case.kind, case.n, case.h, case.w, case.K, case.cout
    out_f32 = kind == "f32" or getattr(case, "out_f32", False)
    okind, u, uo = ("f32" if out_f32 else "bf16"), UNIT[kind], (4 if out_f32 else 8)
    rng = np.random.default_rng(len(case.id))
    P = SimpleNamespace(case=case, keep=[], written=[])
    xp, pos = shuffled_planes(o.x, kind, rng) if case.planes else (o.x, None)
    buf, lin = input_buffer(capi, kind, xp, 1 if case.dw else case.pad_in, form)
    xin = buf.to(dev)
    wp, bp = pack_pw(capi, dev, kind, o.w, o.b, K, case.coutp, P.keep)
    d = capi.PwDesc()
    d.inp, d.w_packed, d.bias_packed = xin.data_ptr(), wp.data_ptr(), bp.data_ptr()
    d.lin, d.cin, d.cout, d.coutp, d.relu = cd.L(capi, lin), K, cout, case.coutp, case.relu
    if pos is not None:
        pl = i32(dev, pos)
        P.keep.append(pl)
        d.in_planes = pl.data_ptr()
    if case.dw:
        t, tb = pack_taps(dev, o.dw, P.keep)
        d.dw_w, d.dw_b = t.data_ptr(), tb.data_ptr()
    # the output pixel: [pass-through run 0 | gap | pass-through run 1 | gap | the GEMM's columns | gap], or a column map
    cmap, g0, pt = None, uo, None
    if case.pt is not None and case.pt[0] == "pairs":
        _, pairs, split = case.pt
        d1 = up(split, 8) + 8
        g0 = up(d1 + 2 * pairs - split, 8) + 8
        q = up(pairs, u)
        pt = pr.pt_interleave(pairs, 0, q, split, 0, d1)
        d.pt_pairs, d.pt_a, d.pt_b, d.pt_split, d.pt_d0, d.pt_d1 = pairs, 0, q, split, 0, d1
        ptw = 2 * q
    cso = g0 + up(cout, uo) + uo
    if case.cmap == "neg":        # reversed order, some columns (fp32 epilogues) / one group of 8 (bf16) not stored
        cmap = np.full(case.coutp, -1, dtype=np.int64)
        cols = np.arange(cout)
        if out_f32:
            cmap[:cout] = np.where(cols % 5 == 2, -1, g0 + cout - 1 - cols)
        else:
            ng = cout // 8
            cmap[:cout] = np.where(cols // 8 == ng // 2, -1, g0 + 8 * (ng - 1 - cols // 8) + cols % 8)
    elif case.cmap == "odd":      # cat + channel_shuffle(2): the GEMM's columns at the odd channels, x1 at the even ones
        cmap = np.full(case.coutp, -1, dtype=np.int64)
        cmap[:cout] = 2 * np.arange(cout) + 1
        cso = up(2 * cout, 4) + 4
        pt = pr.pt_scatter(2 * np.arange(case.pt[1]), case.pt[1])
        pc = i32(dev, pt[1])
        P.keep.append(pc)
        d.pt_cmap, d.pt_c = pc.data_ptr(), case.pt[1]
        ptw = up(case.pt[1], 4)
    pad_out = 1 if case.dw else 1 - case.pad_in
    lout = lr.padded(cso, h, w, pad_out, 0 if cmap is not None else g0) if pad_out else lr.dense(cso, h, w, 0 if cmap is not None else g0)
    if cmap is not None:
        cm = i32(dev, cmap)
        P.keep.append(cm)
        d.out_cmap = cm.data_ptr()
    d.lout = cd.L(capi, lout)
    ref = pr.restate(case, o)
    cols, chan = pr.out_columns(cout, lout.choff, cmap, 1 if out_f32 else 8)
    assert chan.max() < cso and len(set(chan.tolist())) == len(chan)
    P.written.append((lr.index_map(lout, n, h, w, chan), to_bits(nhwc(ref[:, cols]), okind)))
    if pt is not None:            # the pass-through source: a slice at 16 bytes of a pixel 32 bytes wider, always
        src = pr.pt_operands(case, ptw)
        pbuf, lpt = input_buffer(capi, kind, src, 1, "slice", 7)
        ptd = pbuf.to(dev)
        P.keep.append(ptd)
        d.pt_src, d.lpt = ptd.data_ptr(), cd.L(capi, lpt)
        assert pt[1].max() < cso and not set(pt[1].tolist()) & set(chan.tolist())
        P.written.append((lr.index_map(lout, n, h, w, pt[1]), to_bits(nhwc(src[:, pt[0]]), okind)))
    P.keep += [xin]
    P.d = d

    def call(out, nn):
        d.out = out.data_ptr()
        if kind == "f32":
            capi.check(capi.lib.rtpose_pw_fused(C.byref(d), nn, h, w, capi.current_stream()), "rtpose_pw_fused")
        else:
            capi.check(capi.lib.rtpose_pw_fused_bf16(C.byref(d), int(out_f32), nn, h, w, capi.current_stream()), "rtpose_pw_fused_bf16")
    P.call = call
    return _finish(P, capi, dev, okind, lout, cso, n, h, w)


def prepare_head(capi, dev, case, o, form):
    """rtpose_pw_head / rtpose_pw_head_bf16"""
    lib, stream = capi.lib, capi.current_stream()
    kind, n, h, w, cin, c1 = case.kind, case.n, case.h, case.w, case.cin, case.c1
    rng = np.random.default_rng(len(case.id))
    P = SimpleNamespace(case=case, keep=[], written=[])
    xp, pos = shuffled_planes(o.x, kind, rng) if case.planes else (o.x, None)
    buf, lin = input_buffer(capi, kind, xp, case.pad_in, form)
    xin = buf.to(dev)
    w1p, b1p = pack_pw(capi, dev, kind, o.w1, o.b1, cin, c1, P.keep)
    b2p = torch.zeros(pr.HEAD_COLS, device=dev)             # columns nobody owns are zero
    heads = [(f32(dev, o.wp), f32(dev, o.bp), pr.PAF, 0), (f32(dev, o.wh), f32(dev, o.bh), pr.HEAT, pr.HEAT_OFF)]
    if kind == "f32":
        w2p = torch.zeros(lib.rtpose_packed_pw_floats(c1, 64) + 64 * 64, device=dev)
        for wt, b, co, off in heads:
            capi.check(lib.rtpose_pack_pw_weights(capi.ptr(wt), capi.ptr(b), co, c1, None, c1, 64, off, capi.ptr(w2p), capi.ptr(b2p),
                                                  stream))
    else:
        w2p = torch.zeros(c1 * 64 + 4096, dtype=torch.int16, device=dev)
        for wt, b, co, off in heads:
            capi.check(lib.rtpose_pack_pw_head2_bf16(capi.ptr(wt), capi.ptr(b), co, c1, off, capi.ptr(w2p), capi.ptr(b2p), stream))
    torch.cuda.synchronize()
    pad_out = (n + h + w) & 1
    lout = lr.padded(72, h, w, pad_out, 4) if pad_out else lr.dense(72, h, w, 4)
    d1, d2 = capi.PwDesc(), capi.PwDesc()
    d1.inp, d1.w_packed, d1.bias_packed = xin.data_ptr(), w1p.data_ptr(), b1p.data_ptr()
    d1.lin, d1.cin, d1.cout, d1.coutp, d1.relu = cd.L(capi, lin), cin, c1, c1, 1
    if pos is not None:
        pl = i32(dev, pos)
        P.keep.append(pl)
        d1.in_planes = pl.data_ptr()
    d2.w_packed, d2.bias_packed = w2p.data_ptr(), b2p.data_ptr()
    d2.lout, d2.cin, d2.cout, d2.coutp, d2.relu = cd.L(capi, lout), c1, 64, 64, 0
    fits, entry = (lib.rtpose_pw_head_fits, lib.rtpose_pw_head) if kind == "f32" else (lib.rtpose_pw_head_bf16_fits, lib.rtpose_pw_head_bf16)
    assert fits(C.byref(d1), C.byref(d2)) == 1
    P.written.append((lr.index(lout, n, h, w, pr.HEAD_COLS), to_bits(nhwc(pr.restate(case, o)), "f32")))
    P.keep += [xin, w2p, b2p]
    P.d = (d1, d2)

    def call(out, nn):
        d2.out = out.data_ptr()
        capi.check(entry(C.byref(d1), C.byref(d2), nn, h, w, capi.current_stream()), "rtpose_pw_head")
    P.call = call
    return _finish(P, capi, dev, "f32", lout, 72, n, h, w)


def prepare_unit(capi, dev, case, o, form):
    """rtpose_unit_bf16: the stage buffer holds x2 (contiguous from the slice's first channel, or shuffled planes), the slots
    y goes to when the launch is in place, and slots nobody touches"""
    lib = capi.lib
    n, h, w, K1, Kt, cout = case.n, case.h, case.w, case.K1, case.Kt, case.cout
    rng = np.random.default_rng(len(case.id))
    P = SimpleNamespace(case=case, keep=[], written=[])
    npl, ngo = K1 // 8, cout // 8
    nslots = npl + ngo + 3
    slots = rng.permutation(nslots) if case.planes else np.arange(nslots)
    gen = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    xp = cs.decoys((n, nslots * 8, h, w), gen, torch.float64).numpy()
    pos = slots[:npl].astype(np.int64) * 8
    xp[:, pr.plane_channels(pos, 8)] = o.x
    buf, lin = input_buffer(capi, "bf16", xp, 1, form)
    stage = buf.view(torch.int16).to(dev)
    w0p, b0p = pack_pw(capi, dev, "bf16", o.w0, o.b0, K1, case.c1p, P.keep)
    w2p, b2p = pack_pw(capi, dev, "bf16", o.w2, o.b2, Kt, case.c2p, P.keep)
    t, tb = pack_taps(dev, o.dw, P.keep)
    if case.inplace:          # y's 8-channel groups: the other slots of the same pixel
        lout, cso = lin._replace(choff=0), lin.cstride
        chan = pr.plane_channels(lin.choff + slots[npl:npl + ngo].astype(np.int64) * 8, 8)
    else:                     # ... or shuffled groups of another buffer
        cso = cout + 24
        lout = lr.padded(cso, h, w, 1)
        chan = pr.plane_channels(rng.permutation(ngo + 3)[:ngo].astype(np.int64) * 8, 8)
    cmap = np.full(case.c2p, -1, dtype=np.int64)
    cmap[:cout] = chan
    cm = i32(dev, cmap)
    d0, d2 = capi.PwDesc(), capi.PwDesc()
    d0.inp, d0.w_packed, d0.bias_packed = stage.data_ptr(), w0p.data_ptr(), b0p.data_ptr()
    d0.lin, d0.cin, d0.cout, d0.coutp, d0.relu = cd.L(capi, lin), K1, case.c1p, case.c1p, 1
    d0.dw_w, d0.dw_b = t.data_ptr(), tb.data_ptr()
    if case.planes:
        pl = i32(dev, pos)
        P.keep.append(pl)
        d0.in_planes = pl.data_ptr()
    d2.w_packed, d2.bias_packed = w2p.data_ptr(), b2p.data_ptr()
    d2.lout, d2.cin, d2.cout, d2.coutp, d2.relu = cd.L(capi, lout), Kt, cout, case.c2p, 1
    d2.out_cmap = cm.data_ptr()
    assert lib.rtpose_unit_bf16_fits(C.byref(d0), C.byref(d2), h, w) == 1
    cols, ch = pr.out_columns(cout, 0, cmap, 8)
    assert np.array_equal(ch, chan) and chan.max() < cso
    P.written.append((lr.index_map(lout, n, h, w, chan), to_bits(nhwc(pr.restate(case, o)[:, cols]), "bf16")))
    P.keep += [stage, cm]
    P.d = (d0, d2)

    def call(out, nn):
        d2.out = out.data_ptr()
        d0.inp = out.data_ptr() if case.inplace else stage.data_ptr()
        capi.check(lib.rtpose_unit_bf16(C.byref(d0), C.byref(d2), nn, h, w, capi.current_stream()), "rtpose_unit_bf16")
    P.call = call
    _finish(P, capi, dev, "bf16", lout, cso, n, h, w)
    if case.inplace:
        P.stage0, P.before = stage, host_bits(stage)
    return P


PREPARE = {"fused": prepare_fused, "head": prepare_head, "unit": prepare_unit}


def prepare(capi, dev, case, o, form):
    return PREPARE[case.launch](capi, dev, case, o, form)


def launch(P, n=None):
    """one launch of n images (default: all) into a fresh output buffer -> its bits on the host"""
    out = fresh(P)
    P.call(out, P.case.n if n is None else n)
    torch.cuda.synchronize()
    return host_bits(out)


def written_bits(P, bits, images=None):
    """the written words, one array per written block (the GEMM's columns, the pass-through half)"""
    return [bits[idx[:images]] for idx, _ in P.written]


def check(P, bits, images=None):
    """== the restatement at every written word, finite there, and nothing else written"""
    for (idx, exp), got in zip(P.written, written_bits(P, bits, images)):
        nan = (got & 0x7F800000) == 0x7F800000 if got.dtype == np.uint32 else (got & 0x7F80) == 0x7F80
        assert not nan.any(), "%s: %d words of the output were not written (or are not finite)" % (P.case.id, int(nan.sum()))
        bad = got != exp[:images]
        assert not bad.any(), "%s: %d of %d output words differ from the restatement, first at (n, y, x, column) %s" % (
            P.case.id, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
    where = [idx[:images] for idx, _ in P.written]
    if P.before is None:
        assert lr.untouched(bits, where, SENTINEL[P.okind]), "%s: the launch wrote outside its channels / pixels" % P.case.id
    else:
        assert unchanged(bits, P.before, where), "%s: the launch changed words outside its output channels" % P.case.id
