"""Float64 restatement of the five ShuffleNetV2 pointwise-chain launches (rtpose_pw_fused, rtpose_pw_fused_bf16,
rtpose_pw_head, rtpose_pw_head_bf16, rtpose_unit_bf16), written from the contract in include/rtpose_mi355x.h (the
rtpose_pw_desc block) and not from the kernels.  numpy only: no library call, no GPU.  tests/test_pw_restate_cpu.py
checks this file on the CPU; tests/pw_driver.py and tests/test_pw_exact_gpu.py compare the launchers with it bit for bit.

The method: all five launches accumulate in fp32.  With small INTEGER operands (`exact_operands`: activations, pointwise
weights, depthwise taps and biases in {-1, 0, 1}) every partial sum is an integer below 2^24, so the sums are exact in
any order, every value that is rounded to bf16 is an integer of magnitude <= 256 (all of which bf16 holds), and the
kernel's result has ONE correct bit pattern - the one this file computes in float64.  `exact_bounds` returns the figures
the three conditions are asserted on; `EXACT_CASES` is the list, one entry per edge of the kernels' tiling.

Tensors are NCHW numpy float64 unless a name says otherwise."""
from types import SimpleNamespace

import numpy as np

import layout_restate as lr

# the kernels' constants the cases are derived from (csrc/pw_fused.hip, pw_fused_bf16.hip, pw_head.hip, pw_head_bf16.hip,
# unit_bf16.hip); tests/test_pw_restate_cpu.py recomputes every case's counts from them
BM, TILE, GROUP = 64, 8, 8                  # pixels of a strip, edge of a depthwise tile, channels of a k-group
CHUNK = {"f32": 32, "bf16": 64}             # channels of a K chunk
MAXK = 1024                                 # widest K of the fused kernels
HEAD_PX = {"f32": 32, "bf16": 128}          # pixels of a work item of the head launches
HEAD_MINK = {"f32": 32, "bf16": 16}         # narrowest conv5 input the head launchers accept
HEAD_MAXK = {"f32": 1024, "bf16": 480}
UNIT_MAXK = 256
HEAD_COLS, PAF, HEAT, HEAT_OFF = 64, 38, 19, 40
NOMINAL_CUS = 256                           # the CPU file's stand-in for the device's CU count (the GPU file reads it)


def rb(v):
    """a float64 array rounded to bf16 (RNE) where the header says a value is rounded; back as float64"""
    return lr.bf16_to_f32(lr.bf16_rne(np.asarray(v, dtype=np.float64).astype(np.float32))).astype(np.float64)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def _mm(x, w):
    n, c, h, wd = x.shape
    return np.matmul(w, x.reshape(n, c, h * wd)).reshape(n, w.shape[0], h, wd)


def pw64(x, w, b, relu):
    """1x1 conv: x [n, c, h, w], w [co, c], b [co]"""
    y = _mm(x, w) + b[None, :, None, None]
    return np.maximum(y, 0.0) if relu else y


def dw64(x, taps, tb, drop=None):
    """depthwise 3x3, zero padding 1, bias: taps [c, 3, 3], tb [c].  drop = (ky, kx): that tap is left out at the outputs
    of the last row (the mutation of the discrimination check)."""
    n, c, h, w = x.shape
    xp = np.zeros((n, c, h + 2, w + 2))
    xp[:, :, 1:h + 1, 1:w + 1] = x
    y = np.broadcast_to(tb[None, :, None, None], x.shape).copy()
    for ky in range(3):
        for kx in range(3):
            t = xp[:, :, ky:ky + h, kx:kx + w] * taps[None, :, ky, kx, None, None]
            if drop == (ky, kx):
                t[:, :, h - 1, :] = 0.0
            y += t
    return y


def pw_chain64(x, dw, w, b, relu, trace=None, drop=None):
    """rtpose_pw_fused: the optional depthwise 3x3 (dw = (taps, tb) or None), the 1x1 conv, bias, ReLU"""
    a = x if dw is None else dw64(x, dw[0], dw[1], drop)
    y = pw64(a, w, b, relu)
    if trace is not None:
        trace.update(a=a, y=y)
    return y


def pw_chain_bf16(x, dw, w, b, relu, out_f32=False, trace=None, drop=None):
    """rtpose_pw_fused_bf16: the depthwise result is rounded on its way into the LDS A tile, the output where it is
    stored as bf16; taps and biases stay fp32"""
    a = x if dw is None else rb(dw64(x, dw[0], dw[1], drop))
    y = pw64(a, w, b, relu)
    if trace is not None:
        trace.update(a=a, y=y, rounded=([] if dw is None else [a]) + ([] if out_f32 else [y]))
    return y if out_f32 else rb(y)


def _heads(f, wp, bp, wh, bh):
    n, _, h, w = f.shape
    out = np.zeros((n, HEAD_COLS, h, w))
    out[:, 0:PAF] = pw64(f, wp, bp, False)
    out[:, HEAT_OFF:HEAT_OFF + HEAT] = pw64(f, wh, bh, False)
    return out


def head64(x, w1, b1, wp, bp, wh, bh, trace=None):
    """rtpose_pw_head: conv5 + ReLU, then both heads in 64 columns (PAF at 0, heat maps at 40; the rest zero)"""
    f = pw64(x, w1, b1, True)
    if trace is not None:
        trace.update(f=f)
    return _heads(f, wp, bp, wh, bh)


def head_bf16(x, w1, b1, wp, bp, wh, bh, trace=None):
    """rtpose_pw_head_bf16: the conv5 feature is rounded to bf16 after its ReLU, the maps are fp32"""
    f = pw64(x, w1, b1, True)
    if trace is not None:
        trace.update(f=f, rounded=[f])
    return _heads(rb(f), wp, bp, wh, bh)


def unit64(x, w0, b0, dw, w2, b2, trace=None, drop=None):
    """conv.0 + ReLU -> depthwise 3x3 (zero padding: T1 does not exist outside the image) -> conv.2 + ReLU"""
    t1 = pw64(x, w0, b0, True)
    t2 = dw64(t1, dw[0], dw[1], drop)
    y = pw64(t2, w2, b2, True)
    if trace is not None:
        trace.update(t1=t1, t2=t2, y=y)
    return y


def unit_bf16(x, w0, b0, dw, w2, b2, trace=None, drop=None):
    """rtpose_unit_bf16: T1 and T2 are bf16 in LDS, y is stored as bf16"""
    t1 = pw64(x, w0, b0, True)
    t2 = dw64(rb(t1), dw[0], dw[1], drop)
    y = pw64(rb(t2), w2, b2, True)
    if trace is not None:
        trace.update(t1=t1, t2=t2, y=y, rounded=[t1, t2, y])
    return rb(y)


# ---- the channel bookkeeping, as index arithmetic ---------------------------------------------------------------------------------
def pack_pw(w, b, K, coutp, col_off, cin_map=None, col_map=None, ncols=None, wp=None, bp=None):
    """The fp32 pointwise packers (rtpose_pack_pw_weights; rtpose_pack_pw_weights_cols with col_map / ncols) restated: into
    packed [K / 4][coutp][4] and bias [coutp] (given, or zeros), column col_off + i takes output channel col_map[i] (None: i;
    outside [0, cout): a zero column, zero bias) of w [cout, cin_src] and b (None: zero bias), K row c reads input channel
    cin_map[c] (None: c; outside [0, cin_src): a zero row).  Every other word keeps what it held.  Returns flat copies."""
    cout, cin_src = w.shape
    ncols = cout if ncols is None else ncols
    wp = np.zeros(K * coutp, np.float32) if wp is None else np.array(wp, dtype=np.float32)
    bp = np.zeros(coutp, np.float32) if bp is None else np.array(bp, dtype=np.float32)
    w3 = wp.reshape(K // 4, coutp, 4)
    for i in range(ncols):
        n = i if col_map is None else int(col_map[i])
        live = 0 <= n < cout
        bp[col_off + i] = b[n] if live and b is not None else 0.0
        for c in range(K):
            src = (c if c < cin_src else -1) if cin_map is None else int(cin_map[c])
            w3[c // 4, col_off + i, c % 4] = w[n, src] if live and 0 <= src < cin_src else 0.0
    return wp, bp


def plane_channels(planes, unit):
    """in_planes: K channel k is channel planes[k // unit] + k % unit of the pixel (relative to lin.choff); unit = 4 (fp32)
    or 8 (bf16) channels = 16 bytes"""
    planes = np.asarray(planes, dtype=np.int64)
    return (planes[:, None] + np.arange(unit, dtype=np.int64)[None, :]).reshape(-1)


def out_columns(cout, choff, cmap, group):
    """(stored columns, their ABSOLUTE channels).  cmap None: column n < cout -> choff + n.  group = 1: cmap per column
    (the fp32 epilogues), 8: per group of 8 columns (bf16: columns 8 g .. 8 g + 7 at cmap[8 g] ..); < 0: not stored."""
    cols = np.arange(cout, dtype=np.int64)
    if cmap is None:
        return cols, choff + cols
    cmap = np.asarray(cmap, dtype=np.int64)
    chan = cmap[cols] if group == 1 else cmap[cols // group * group] + cols % group
    keep = (cmap[cols] >= 0) if group == 1 else (cmap[cols // group * group] >= 0)
    return cols[keep], chan[keep]


def pt_scatter(pt_cmap, pt_c):
    """(source channels relative to lpt.choff, absolute output channels) of the scatter form"""
    return np.arange(pt_c, dtype=np.int64), np.asarray(pt_cmap, dtype=np.int64)[:pt_c]


def pt_interleave(pairs, a, b, split, d0, d1):
    """(source channels relative to lpt.choff, absolute output channels) of the interleave form: output j < 2 pairs"""
    j = np.arange(2 * pairs, dtype=np.int64)
    return np.where(j & 1, b, a) + j // 2, np.where(j < split, d0 + j, d1 + j - split)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _case(launch, kind, tag, n, h, w, **kw):
    c = SimpleNamespace(launch=launch, kind=kind, tag=tag, n=n, h=h, w=w, relu=1, walk=None, dens_x=0.67, dens_w=1.0,
                        dens_t=0.67, planes=False, pad_in=1)
    c.__dict__.update(kw)
    c.id = "%s-%s-%s" % (launch, kind, tag)
    return c


def _fused(kind, tag, n, h, w, K, cout, coutp, **kw):
    d = dict(K=K, cout=cout, coutp=coutp, dw=False, cmap=None, pt=None)
    d.update(kw)
    return _case("fused", kind, tag, n, h, w, **d)


def _w_density(K):
    """pointwise weight density of a K-term sum of +-1 products whose result must stay within +-256"""
    return 1.0 if K <= 64 else (0.5 if K <= 256 else 0.125)


def _fused_cases(kind):
    f32 = kind == "f32"
    L = []
    # plain: the 64-pixel strip (pixel counts 1, 63, 64, 65, 129; strips across row and image gaps)
    K0 = 8 if f32 else 16
    for (n, h, w), pad in (((1, 1, 1), 0), ((1, 7, 9), 1), ((1, 8, 8), 0), ((5, 1, 13), 1), ((3, 1, 43), 1)):
        L.append(_fused(kind, "strip%d" % (n * h * w), n, h, w, K0, 8, 64, pad_in=pad, relu=int(n * h * w == 63)))
    # plain: K at the chunk edges (one group, one chunk, a chunk + a group, two chunks, the widest)
    for K in ((8, 32, 40, 64, 232, 1024) if f32 else (16, 64, 80, 1024)):
        L.append(_fused(kind, "K%d" % K, 2, 3, 11 if K < 1024 else 5, K, 16, 64, planes=K in (40, 80, 232), dens_w=_w_density(K),
                        relu=0 if K <= 16 else 1))
    # plain: the column arrangements and cout inside them
    for cout, coutp in ((1, 64), (19, 64), (58, 64), (100, 128), (256, 256), (512, 512)):
        if not f32 and cout % 8:
            cout = (cout + 7) // 8 * 8           # bf16 stores whole 8-channel groups
        L.append(_fused(kind, "cout%dof%d" % (cout, coutp), 1, 5, 15, 24 if f32 else 32, cout, coutp, pad_in=cout & 1,
                        relu=0 if cout <= 8 else 1))
    L.append(_fused(kind, "cmapneg", 2, 5, 7, 40 if f32 else 48, 24, 64, cmap="neg", planes=True))
    if not f32:
        L.append(_fused(kind, "outf32", 2, 5, 7, 48, 19, 64, out_f32=True, relu=0, cmap="neg"))
    # depthwise: maps around the 8 x 8 tile, the image gap as a halo, K of one chunk / three groups / a chunk + a group
    maps = ((1, 1), (1, 17), (17, 1), (7, 8), (9, 9), (8, 16), (16, 7), (17, 9))
    Ks = (8, 24, 40, 16, 24, 40, 8, 24) if f32 else (16, 48, 80, 16, 48, 80, 16, 48)
    for i, ((h, w), K) in enumerate(zip(maps, Ks)):
        L.append(_fused(kind, "dw%dx%d" % (h, w), 2 + (i & 1), h, w, K, 56, 64, dw=True, relu=i & 1))
    L.append(_fused(kind, "dwK%d" % (232 if f32 else 240), 2, 9, 9, 232 if f32 else 240, 232 if f32 else 240, 256, dw=True,
                    dens_w=0.125))
    # depthwise + pass-through: interleave form with pt_pairs % 4 = 0 .. 3, odd and even pt_split; the scatter form (fp32)
    for pairs, split in ((4, 4), (5, 5), (6, 6), (7, 8), (29, 29)):
        K = 2 * ((pairs + 3) // 4 * 4) if f32 else 2 * ((pairs + 7) // 8 * 8)
        L.append(_fused(kind, "pairs%dsplit%d" % (pairs, split), 2, 9, 10, K, K, 64, dw=True, pt=("pairs", pairs, split)))
    if f32:
        for pt_c in (6, 8, 58):
            L.append(_fused(kind, "ptc%d" % pt_c, 2, 9, 10, 8 if pt_c < 58 else 64, pt_c, 64, dw=True, pt=("scatter", pt_c),
                            relu=0 if pt_c < 58 else 1, cmap="odd"))
    # the walk: more work items than blocks, a ragged last round
    L.append(_fused(kind, "walk-nch1", 0, 1, 61, K0, 8, 64, walk="strips", relu=0))
    L.append(_fused(kind, "walk-2pass", 0, 1, 61, 2 * CHUNK[kind] + 8 * (1 if f32 else 2), 512, 512, walk="strips"))
    L.append(_fused(kind, "walk-dw-pt", 0, 9, 9, 24 if f32 else 48, 24 if f32 else 48, 64, dw=True, walk="tiles",
                    pt=("pairs", 10, 10)))
    return L


def _head(kind, tag, n, h, w, cin, c1, **kw):
    return _case("head", kind, tag, n, h, w, cin=cin, c1=c1, dens_w=_w_density(cin), dens_h=0.25 if c1 <= 256 else 0.125, **kw)


def _head_cases(kind):
    L = []
    px = HEAD_PX[kind]
    for m in sorted({1, 31, 32, 33, 65, px - 1, px, px + 1}):
        n, h, w = (1, 1, m) if m < 8 else ((1, m, 1) if m % 2 == 0 else (m, 1, 1))
        if m == 65:
            n, h, w = 5, 1, 13
        L.append(_head(kind, "px%d" % m, n, h, w, 32, 256))
    for cin in ((32, 48, 464) if kind == "f32" else (16, 32, 48, 480)):
        L.append(_head(kind, "cin%d" % cin, 2, 3, 7, cin, 256, planes=cin == 48))
    L.append(_head(kind, "c1-1024", 1, 5, 7, 48, 1024))
    L.append(_head(kind, "widest", 1, 3, 3, HEAD_MAXK[kind], 1024, planes=True))
    L.append(_head(kind, "walk", 0, 1, 61, 32 if kind == "f32" else 16, 256, walk="items"))
    return L


def _unit(tag, n, h, w, K1, Kt, cout, c2p, **kw):
    d = dict(K1=K1, Kt=Kt, cout=cout, c1p=128 if Kt <= 128 else 256, c2p=c2p, inplace=True,
             dens_w2=0.5 if Kt <= 64 else (0.25 if Kt <= 128 else 0.125))
    d.update(kw)
    return _case("unit", "bf16", tag, n, h, w, **d)


def _unit_cases():
    L = []
    maps = ((1, 1), (1, 17), (17, 1), (7, 8), (9, 9), (8, 16), (16, 7), (17, 9))
    chans = ((16, 16, 8, 128), (32, 64, 64, 128), (64, 128, 128, 128), (256, 256, 256, 256),
             (16, 64, 8, 256), (128, 128, 120, 256), (48, 16, 16, 128), (256, 192, 192, 256))
    for i, ((h, w), (K1, Kt, cout, c2p)) in enumerate(zip(maps, chans)):
        L.append(_unit("%dx%d-K%d-T%d" % (h, w, K1, Kt), 2 + (i & 1), h, w, K1, Kt, cout, c2p, inplace=not (i & 1),
                       planes=bool(i & 2)))
    L.append(_unit("walk", 0, 9, 9, 16, 16, 8, 128, walk="tiles"))
    L.append(_unit("walk-wide", 0, 9, 9, 32, 64, 64, 256, walk="tiles", inplace=False, planes=True))
    L.append(_unit("walk-widest", 0, 9, 9, 240, 240, 232, 256, walk="tiles", planes=True))      # K1, Kt < conv.2's 256 columns
    return L


EXACT_CASES = {
    "pw_fused": _fused_cases("f32"),
    "pw_fused_bf16": _fused_cases("bf16"),
    "pw_head": _head_cases("f32"),
    "pw_head_bf16": _head_cases("bf16"),
    "unit_bf16": _unit_cases(),
}


def walk_cap(case, cus):
    """the launcher's grid cap in work items: 2 blocks per CU (fused), a wave per SIMD (fp32 head), a block per CU"""
    if case.launch == "fused":
        return 2 * cus
    return 4 * cus if (case.launch == "head" and case.kind == "f32") else cus


def work_items(case, n):
    """work items of an n-image launch of the case"""
    m = n * case.h * case.w
    if case.launch == "head":
        return -(-m // HEAD_PX[case.kind])
    tiles = n * (-(-case.h // TILE)) * (-(-case.w // TILE))
    if case.launch == "unit":
        return tiles
    npass = 1 if case.coutp <= 128 else case.coutp // 256
    return (tiles if case.dw else -(-m // BM)) * npass


def walk_images(case, cus):
    """the smallest n whose work items exceed 1.5 x the grid cap and do not come out as whole rounds"""
    cap = walk_cap(case, cus)
    n = 1
    while work_items(case, n) < 1.5 * cap + 1 or work_items(case, n) % cap == 0:
        n += 1
    return n


def sized(case, cus=NOMINAL_CUS):
    """the case with its image count filled in (walk cases: from the CU count)"""
    if case.walk is None:
        return case
    c = SimpleNamespace(**case.__dict__)
    c.n = walk_images(case, cus)
    return c


# ---- operands and bounds ---------------------------------------------------------------------------------------------------------
def _ternary(rng, shape, density):
    return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < density).astype(np.float64) + 0.0      # (no -0.0)


def exact_operands(case, seed=0):
    """Ternary integer operands of a (sized) case: activations, pointwise weights and depthwise taps in {-1, 0, 1} at the
    case's densities, biases in {-1, 0, 1}."""
    rng = np.random.default_rng([seed, sum(map(ord, case.id))])
    t = lambda shape, d=2.0 / 3.0: _ternary(rng, shape, d)      # noqa: E731
    n, h, w = case.n, case.h, case.w
    o = SimpleNamespace()
    if case.launch == "fused":
        o.x = t((n, case.K, h, w), case.dens_x)
        o.dw = (t((case.K, 3, 3), case.dens_t), t((case.K,))) if case.dw else None
        o.w, o.b = t((case.cout, case.K), case.dens_w), t((case.cout,))
    elif case.launch == "head":
        o.x = t((n, case.cin, h, w), case.dens_x)
        o.w1, o.b1 = t((case.c1, case.cin), case.dens_w), t((case.c1,))
        o.wp, o.bp = t((PAF, case.c1), case.dens_h), t((PAF,))
        o.wh, o.bh = t((HEAT, case.c1), case.dens_h), t((HEAT,))
    else:
        o.x = t((n, case.K1, h, w), case.dens_x)
        o.w0, o.b0 = t((case.Kt, case.K1), 1.0 if case.K1 <= 64 else 0.125), t((case.Kt,))
        o.dw = (t((case.Kt, 3, 3), case.dens_t), t((case.Kt,)))
        o.w2, o.b2 = t((case.cout, case.Kt), case.dens_w2), t((case.cout,))
    return o


def pt_operands(case, width, seed=0):
    """the pass-through source of a case: [n, width, h, w] integers of magnitude 1 .. 99 (exact in bf16), never zero"""
    rng = np.random.default_rng([seed, 1, sum(map(ord, case.id))])
    shape = (case.n, width, case.h, case.w)
    return rng.integers(1, 100, shape).astype(np.float64) * (rng.integers(0, 2, shape) * 2 - 1)


def restate(case, o, trace=None, drop=None):
    """the launch of the case on operands o: [n, columns, h, w] float64 (bf16 outputs: the rounded values)"""
    bf = case.kind == "bf16"
    if case.launch == "fused":
        if bf:
            return pw_chain_bf16(o.x, o.dw, o.w, o.b, case.relu, getattr(case, "out_f32", False), trace, drop)
        return pw_chain64(o.x, o.dw, o.w, o.b, case.relu, trace, drop)
    if case.launch == "head":
        return (head_bf16 if bf else head64)(o.x, o.w1, o.b1, o.wp, o.bp, o.wh, o.bh, trace)
    return unit_bf16(o.x, o.w0, o.b0, o.dw, o.w2, o.b2, trace, drop)


def _S(x, w, b):
    return float((_mm(np.abs(x), np.abs(w)) + np.abs(b)[None, :, None, None]).max())


def exact_bounds(case, o):
    """(largest S = |b| + sum |w| |x| of any sum, largest magnitude of any value rounded to bf16 (0.0: none is), share of the
    final outputs that are nonzero) from the float64 intermediates"""
    tr = {}
    y = restate(case, o, tr)
    ones = lambda d: (np.abs(d[0]), np.abs(d[1]))      # noqa: E731
    if case.launch == "fused":
        S = _S(tr["a"], o.w, o.b)
        if o.dw is not None:
            S = max(S, float(dw64(np.abs(o.x), *ones(o.dw)).max()))
        share = float(np.count_nonzero(y)) / y.size
    elif case.launch == "head":
        S = max(_S(o.x, o.w1, o.b1), _S(tr["f"], o.wp, o.bp), _S(tr["f"], o.wh, o.bh))
        real = np.r_[0:PAF, HEAT_OFF:HEAT_OFF + HEAT]
        share = float(np.count_nonzero(y[:, real])) / y[:, real].size
    else:
        S = max(_S(o.x, o.w0, o.b0), float(dw64(np.abs(tr["t1"]), *ones(o.dw)).max()), _S(tr["t2"], o.w2, o.b2))
        share = float(np.count_nonzero(y)) / y.size
    rounded = max([float(np.abs(v).max()) for v in tr.get("rounded", [])] or [0.0])
    return S, rounded, share
