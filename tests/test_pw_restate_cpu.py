"""tests/pw_restate.py on the CPU: every exact case meets the three conditions its bit-for-bit comparison rests on and
reaches the edge its tag names; the restatement equals plain torch conv2d in float64 and oracle/shufflenet_oracle.py's
unit; the channel maps round-trip; and every case tells a correct kernel from the usual wrong ones."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layout_restate as lr
import pw_restate as pr
from oracle import shufflenet_oracle as so

ALL = [c for L in pr.EXACT_CASES.values() for c in L]
_ops = {}


def ops(case):
    """the sized case and its operands, drawn once"""
    if case.id not in _ops:
        c = pr.sized(case)
        _ops[case.id] = (c, pr.exact_operands(c))
    return _ops[case.id]


def cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_case_meets_the_three_conditions(case):
    c, o = ops(case)
    S, rounded, share = pr.exact_bounds(c, o)
    print("%s: largest S %d, largest rounded magnitude %d, nonzero share %.2f" % (c.id, S, rounded, share))
    assert S < 2 ** 24                      # every fp32 sum is exact in any order
    assert rounded <= 256                   # every value rounded to bf16 is an integer bf16 holds
    assert share >= 0.40                    # ReLU does not hide the case
    y = pr.restate(c, o)
    assert np.array_equal(y, np.round(y)) and np.abs(y).max() < 2 ** 24


def test_case_counts_and_figures():
    n = {k: len(v) for k, v in pr.EXACT_CASES.items()}
    worst_S = max(pr.exact_bounds(*ops(c))[0] for c in ALL)
    worst_r = max(pr.exact_bounds(*ops(c))[1] for c in ALL)
    print("cases per launcher %s; largest S %d; largest rounded magnitude %d" % (n, worst_S, worst_r))
    assert set(n) == {"pw_fused", "pw_fused_bf16", "pw_head", "pw_head_bf16", "unit_bf16"} and min(n.values()) >= 10
    assert len({c.id for c in ALL}) == len(ALL)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_case_reaches_the_edge_its_tag_names(case):
    c, _ = ops(case)
    tag, m = c.tag, c.n * c.h * c.w
    num = lambda s: int(re.search(r"\d+", s).group())      # noqa: E731
    if c.launch == "fused":
        chunk = pr.CHUNK[c.kind]
        assert c.K % (8 if c.kind == "f32" else 16) == 0 and c.K <= pr.MAXK and c.cout <= c.coutp
        assert c.coutp in (64, 128) or c.coutp % 256 == 0
        nch, last = cdiv(c.K, chunk), (c.K - 1) % chunk // pr.GROUP + 1      # chunks, k-groups of the last chunk
        npass = 1 if c.coutp <= 128 else c.coutp // 256
        ty, tx = cdiv(c.h, pr.TILE), cdiv(c.w, pr.TILE)
        assert pr.work_items(c, c.n) == (c.n * ty * tx if c.dw else cdiv(m, pr.BM)) * npass
        if tag.startswith("strip"):
            assert m == num(tag) and not c.dw and nch == 1
            assert cdiv(m, pr.BM) == {1: 1, 63: 1, 64: 1, 65: 2, 129: 3}[m]
            assert m < 64 or c.h * c.w < 64 or m == 64              # longer strips cross row / image gaps
        elif tag.startswith("K"):
            assert c.K == num(tag)
            want = {"f32": {8: (1, 1), 32: (1, 4), 40: (2, 1), 64: (2, 4), 232: (8, 1), 1024: (32, 4)},
                    "bf16": {16: (1, 2), 64: (1, 8), 80: (2, 2), 1024: (16, 8)}}[c.kind][c.K]
            assert (nch, last) == want
        elif tag.startswith("cout"):
            a, b = map(int, re.findall(r"\d+", tag))
            assert (c.cout, c.coutp) == (a, b) and npass == {64: 1, 128: 1, 256: 1, 512: 2}[b]
        elif tag.startswith("dw") and "x" in tag:
            assert c.dw and c.n >= 2 and (c.h, c.w) == tuple(map(int, re.findall(r"\d+", tag)))
            assert (ty, tx) == (cdiv(c.h, 8), cdiv(c.w, 8))
        elif tag.startswith("dwK"):
            assert c.dw and c.K == num(tag) and nch == cdiv(c.K, chunk) and nch > 2
        elif tag.startswith("pairs"):
            pairs, split = map(int, re.findall(r"\d+", tag))
            assert c.pt == ("pairs", pairs, split) and c.dw
        elif tag.startswith("ptc"):
            assert c.pt == ("scatter", num(tag)) and c.kind == "f32"
    if c.launch == "fused" and c.kind in ("f32", "bf16") and c.tag == "pairs4split4":
        rest = {x.pt[1] % 4 for x in pr.EXACT_CASES["pw_fused" if c.kind == "f32" else "pw_fused_bf16"] if x.pt and x.pt[0] == "pairs"}
        split = {x.pt[2] & 1 for x in pr.EXACT_CASES["pw_fused" if c.kind == "f32" else "pw_fused_bf16"] if x.pt and x.pt[0] == "pairs"}
        assert rest == {0, 1, 2, 3} and split == {0, 1}            # every remainder of pt_pairs, both store paths
    if c.launch == "head":
        px = pr.HEAD_PX[c.kind]
        assert pr.HEAD_MINK[c.kind] <= c.cin <= pr.HEAD_MAXK[c.kind] and c.cin % 16 == 0 and c.c1 % 256 == 0 and c.c1 <= 1024
        assert pr.work_items(c, c.n) == cdiv(m, px)
        if tag.startswith("px"):
            assert m == num(tag)
        elif tag.startswith("cin"):
            assert c.cin == num(tag)
        elif tag == "widest":
            assert (c.cin, c.c1) == (pr.HEAD_MAXK[c.kind], 1024)
    if c.launch == "unit":
        assert c.K1 % 16 == 0 and c.Kt % 16 == 0 and max(c.K1, c.Kt) <= pr.UNIT_MAXK and c.cout % 8 == 0 and c.cout <= c.c2p
        assert c.c1p == (128 if c.Kt <= 128 else 256) and c.c2p in (128, 256)
        assert pr.work_items(c, c.n) == c.n * cdiv(c.h, 8) * cdiv(c.w, 8)
        if c.walk is None:
            assert c.n >= 2 and "%dx%d-K%d-T%d" % (c.h, c.w, c.K1, c.Kt) == tag
    if c.walk is not None:
        cap, items = pr.walk_cap(c, pr.NOMINAL_CUS), pr.work_items(c, c.n)
        assert items >= 1.5 * cap and items % cap != 0                 # more than one round, a ragged last one
        if tag == "walk-nch1":
            assert cdiv(c.K, pr.CHUNK[c.kind]) == 1
        if tag == "walk-2pass":
            assert c.coutp == 512
        if tag == "walk-dw-pt":
            assert c.dw and c.pt is not None


def test_every_launcher_has_every_edge():
    for kind, name in (("f32", "pw_fused"), ("bf16", "pw_fused_bf16")):
        L = pr.EXACT_CASES[name]
        assert {c.n * c.h * c.w for c in L if c.tag.startswith("strip")} == {1, 63, 64, 65, 129}
        assert {c.coutp for c in L} >= {64, 128, 256, 512}
        assert {(c.h, c.w) for c in L if c.dw} >= {(1, 1), (1, 17), (17, 1), (9, 9), (7, 8), (8, 16)}
        assert {c.pad_in for c in L if not c.dw} == {0, 1} and {c.planes for c in L} == {False, True}
        assert {c.relu for c in L} == {0, 1} and any(c.cmap == "neg" for c in L)
        assert {c.tag for c in L if c.walk} == {"walk-nch1", "walk-2pass", "walk-dw-pt"}
    for kind, name in (("f32", "pw_head"), ("bf16", "pw_head_bf16")):
        L = pr.EXACT_CASES[name]
        assert {c.n * c.h * c.w for c in L if c.tag.startswith("px")} >= {1, 31, 32, 33, 65}
        assert {c.c1 for c in L} == {256, 1024} and {c.planes for c in L} == {False, True} and sum(c.walk is not None for c in L) == 1
    L = pr.EXACT_CASES["unit_bf16"]
    assert {c.K1 for c in L} >= {16, 256} and {c.Kt for c in L} >= {16, 64, 128, 256} and {c.cout for c in L} >= {8}
    assert {c.c1p for c in L} == {128, 256} == {c.c2p for c in L} and {c.inplace for c in L} == {False, True}
    assert {(c.h, c.w) for c in L} >= {(1, 1), (1, 17), (17, 1), (9, 9)}


# ---- the restatement against torch and the oracle ----------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _conv_unit(x, w0, b0, dw, w2, b2, rnd=lambda v: v):
    t1 = rnd(F.relu(F.conv2d(_t(x), _t(w0)[:, :, None, None], _t(b0))))
    t2 = rnd(F.conv2d(t1, _t(dw[0])[:, None], _t(dw[1]), padding=1, groups=w0.shape[0]))
    return rnd(F.relu(F.conv2d(t2, _t(w2)[:, :, None, None], _t(b2))))


def _rb_t(v):
    return v.float().to(torch.bfloat16).double()


def test_restatement_equals_torch_conv2d_in_float64():
    rng = np.random.default_rng(5)
    r = lambda *s: rng.standard_normal(s)      # noqa: E731
    x, w, b, dw = r(2, 24, 9, 11), r(19, 24), r(19), (r(24, 3, 3), r(24))
    for relu in (0, 1):
        ref = F.conv2d(_t(x), _t(w)[:, :, None, None], _t(b))
        assert np.allclose(pr.pw_chain64(x, None, w, b, relu), (F.relu(ref) if relu else ref).numpy(), rtol=0, atol=1e-12)
        a = F.conv2d(_t(x), _t(dw[0])[:, None], _t(dw[1]), padding=1, groups=24)
        ref = F.conv2d(a, _t(w)[:, :, None, None], _t(b))
        assert np.allclose(pr.pw_chain64(x, dw, w, b, relu), (F.relu(ref) if relu else ref).numpy(), rtol=0, atol=1e-12)
    w1, b1, wp, bp, wh, bh = r(32, 24), r(32), r(38, 32), r(38), r(19, 32), r(19)
    f = F.relu(F.conv2d(_t(x), _t(w1)[:, :, None, None], _t(b1)))
    got = pr.head64(x, w1, b1, wp, bp, wh, bh)
    assert np.allclose(got[:, :38], F.conv2d(f, _t(wp)[:, :, None, None], _t(bp)).numpy(), rtol=0, atol=1e-12)
    assert np.allclose(got[:, 40:59], F.conv2d(f, _t(wh)[:, :, None, None], _t(bh)).numpy(), rtol=0, atol=1e-12)
    assert not got[:, 38:40].any() and not got[:, 59:].any()
    w0, b0, dwu, w2, b2 = r(16, 24), r(16), (r(16, 3, 3), r(16)), r(8, 16), r(8)
    assert np.allclose(pr.unit64(x, w0, b0, dwu, w2, b2), _conv_unit(x, w0, b0, dwu, w2, b2).numpy(), rtol=0, atol=1e-12)
    # the bf16 forms on bf16 operands: the same rounding points; a float64 sum may land on the other side of a rounding
    # boundary than torch's (another order), so: within one bf16 ulp everywhere, identical almost everywhere
    xb, w0b, w2b = pr.rb(x), pr.rb(w0), pr.rb(w2)
    got, ref = pr.unit_bf16(xb, w0b, b0, dwu, w2b, b2), _conv_unit(xb, w0b, b0, dwu, w2b, b2, _rb_t).numpy()
    assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -7) and np.mean(got == ref) > 0.99
    got = pr.pw_chain_bf16(xb, dw, pr.rb(w), b, 1)
    ref = _rb_t(F.relu(F.conv2d(_rb_t(F.conv2d(_t(xb), _t(dw[0])[:, None], _t(dw[1]), padding=1, groups=24)),
                                _t(pr.rb(w))[:, :, None, None], _t(b)))).numpy()
    assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -7) and np.mean(got == ref) > 0.99
    fb = _rb_t(F.relu(F.conv2d(_t(xb), _t(pr.rb(w1))[:, :, None, None], _t(b1))))
    got = pr.head_bf16(xb, pr.rb(w1), b1, pr.rb(wp), bp, pr.rb(wh), bh)
    ref = F.conv2d(fb, _t(pr.rb(wp))[:, :, None, None], _t(bp)).numpy()
    assert np.abs(got[:, :38] - ref).max() <= 2.0 ** -7 * np.abs(ref).max() and np.mean(got[:, :38] == ref) > 0.95


def test_restatement_equals_the_oracle_unit():
    """one stride-1 unit with random weights: oracle/shufflenet_oracle.py's _block (fp32 torch) and _block_bf16 against
    unit64 / unit_bf16 + the interleave pass-through (cat + channel_shuffle(2))"""
    g = torch.Generator().manual_seed(11)
    h, p = 24, "u"
    sd = {}
    for name, shape in (("conv.0", (h, h, 1, 1)), ("conv.1", (h, 1, 3, 3)), ("conv.2", (h, h, 1, 1))):
        sd["%s.%s.0.weight" % (p, name)] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        sd["%s.%s.1.weight" % (p, name)] = torch.rand(h, generator=g) + 0.5
        sd["%s.%s.1.bias" % (p, name)] = torch.randn(h, generator=g) * 0.1
        sd["%s.%s.1.running_mean" % (p, name)] = torch.randn(h, generator=g) * 0.1
        sd["%s.%s.1.running_var" % (p, name)] = torch.rand(h, generator=g) + 0.5
    x = torch.randn(2, 2 * h, 9, 7, generator=g)
    fold = lambda name: [t.double().numpy() for t in so._fold(sd, "%s.%s" % (p, name))]      # noqa: E731
    (w0, b0), (wd, bd), (w2, b2) = fold("conv.0"), fold("conv.1"), fold("conv.2")
    src, dst = pr.pt_interleave(h, 0, h, 2 * h, 0, 0)              # x1 -> even channels, y -> odd channels

    def assemble(y, x1):
        out = np.zeros((2, 2 * h, 9, 7))
        out[:, dst] = np.concatenate([x1, y], 1)[:, src]
        return out
    xn = x.double().numpy()
    got = assemble(pr.unit64(xn[:, h:], w0[:, :, 0, 0], b0, (wd[:, 0], bd), w2[:, :, 0, 0], b2), xn[:, :h])
    ref = so._block(sd, p, x, 1, False).double().numpy()
    assert np.array_equal(got[:, 0::2], ref[:, 0::2]) and np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    xb = so._rb(x)
    xn = xb.double().numpy()
    got = assemble(pr.unit_bf16(xn[:, h:], pr.rb(w0[:, :, 0, 0]), b0, (wd[:, 0], bd), pr.rb(w2[:, :, 0, 0]), b2), xn[:, :h])
    ref = so._block_bf16(sd, p, xb, 1, False).double().numpy()
    assert np.array_equal(got[:, 0::2], ref[:, 0::2])
    assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -7 + 1e-30) and np.mean(got == ref) > 0.99


def test_channel_maps_round_trip():
    rng = np.random.default_rng(3)
    # in_planes: a gather through plane_channels undoes the scatter, for both plane widths
    for unit in (4, 8):
        pos = rng.permutation(9)[:6] * unit
        ch = pr.plane_channels(pos, unit)
        assert len(set(ch.tolist())) == 6 * unit and np.array_equal(ch[::unit], pos)
        x = rng.standard_normal((2, 6 * unit, 3, 3))
        wide = np.zeros((2, 9 * unit, 3, 3))
        wide[:, ch] = x
        assert np.array_equal(wide[:, ch], x)
    # out_cmap per column and per group of 8; negative entries drop exactly their columns
    cols, chan = pr.out_columns(19, 4, None, 1)
    assert np.array_equal(cols, np.arange(19)) and np.array_equal(chan, 4 + np.arange(19))
    cmap = np.where(np.arange(24) % 5 == 2, -1, 40 - np.arange(24))
    cols, chan = pr.out_columns(24, 0, cmap, 1)
    assert np.array_equal(cols, [c for c in range(24) if c % 5 != 2]) and np.array_equal(chan, cmap[cols])
    cmap8 = np.repeat([16, -1, 0], 8) + np.tile(np.arange(8), 3) * np.repeat([1, 0, 1], 8)
    cols, chan = pr.out_columns(24, 0, cmap8, 8)
    assert np.array_equal(cols, np.r_[0:8, 16:24]) and np.array_equal(chan, np.r_[16:24, 0:8])
    # both pass-through forms against cat + channel_shuffle(2) written out in torch
    for pairs in (4, 5, 6, 7, 29):
        q = (pairs + 3) // 4 * 4
        runs = rng.standard_normal((1, 2 * q, 2, 2))                      # [even run | odd run], padded to q each
        src, dst = pr.pt_interleave(pairs, 0, q, 2 * pairs, 0, 0)
        out = np.zeros((1, 2 * pairs, 2, 2))
        out[:, dst] = runs[:, src]
        ref = so._shuffle(torch.from_numpy(np.concatenate([runs[:, :pairs], runs[:, q:q + pairs]], 1)))
        assert np.array_equal(out, ref.numpy())
        for split in (pairs, pairs + 1 - (pairs & 1)):                      # two runs of the destination: a bijection
            src, dst = pr.pt_interleave(pairs, 0, q, split, 0, 100)
            assert len(set(dst.tolist())) == 2 * pairs and np.array_equal(np.sort(dst[dst < 100]), np.arange(min(split, 2 * pairs)))
    src, dst = pr.pt_scatter(2 * np.arange(6), 6)
    assert np.array_equal(src, np.arange(6)) and np.array_equal(dst, 2 * np.arange(6))
    # the layout index arithmetic the driver reads the bits through: scatter then gather
    lay = lr.padded(24, 5, 7, 1, 8)
    buf = np.zeros(lr.pixels(lay, 2) * 24)
    x = rng.standard_normal((2, 12, 5, 7))
    assert np.array_equal(lr.gather(lr.scatter(buf, lay, x), lay, 2, 5, 7, 12), x)


# ---- discrimination ------------------------------------------------------------------------------------------------------------
def _mutants(c, o):
    """(name, output of a wrong kernel) for every wrong kernel the case can meet"""
    cp = lambda **kw: SimpleNamespace(**{**o.__dict__, **kw})      # noqa: E731
    out = []

    def zero_last_group(w):
        w = w.copy()
        w[:, -pr.GROUP:] = 0.0
        return w
    if c.launch == "fused":
        out.append(("last k-group dropped", pr.restate(c, cp(w=zero_last_group(o.w)))))
    elif c.launch == "head":
        out.append(("last k-group of conv5 dropped", pr.restate(c, cp(w1=zero_last_group(o.w1)))))
        out.append(("last k-group of the heads dropped", pr.restate(c, cp(wp=zero_last_group(o.wp), wh=zero_last_group(o.wh)))))
    else:
        out.append(("last k-group of conv.0 dropped", pr.restate(c, cp(w0=zero_last_group(o.w0)))))
        out.append(("last k-group of conv.2 dropped", pr.restate(c, cp(w2=zero_last_group(o.w2)))))
    if getattr(c, "dw", c.launch == "unit"):
        out.append(("centre tap dropped at the last row", pr.restate(c, o, drop=(1, 1))))
        if c.h > 1:
            out.append(("upper tap dropped at the last row", pr.restate(c, o, drop=(0, 1))))
        if c.n > 1 and c.h * c.w > 1:       # the first pixel behind the image gap, as its neighbours' halo
            x = o.x.copy()
            x[1, :, 0, 0] = 0.0
            y = pr.restate(c, cp(x=x))
            y[1, :, 0, 0] = pr.restate(c, o)[1, :, 0, 0]
            out.append(("halo pixel behind the image gap zeroed", y))
    y = pr.restate(c, o).copy()
    y[-1, :, -1, -1] = 0.0                  # (an unwritten pixel of a zero-filled buffer; a sentinel differs always)
    out.append(("last pixel of the last strip dropped", y))
    return out


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_case_discriminates(case):
    c, o = ops(case)
    ref = pr.restate(c, o)
    for name, y in _mutants(c, o):
        assert (y != ref).any(), "%s cannot tell: %s" % (c.id, name)
    if c.launch == "fused" and c.pt is not None:      # one pass-through pair shifted: the source runs differ pair to pair
        src = (pr.pt_interleave(c.pt[1], 0, 32, c.pt[2], 0, 64) if c.pt[0] == "pairs" else pr.pt_scatter(np.arange(c.pt[1]), c.pt[1]))[0]
        v = pr.pt_operands(c, 64)
        shifted = src.copy()
        shifted[-1] -= 1
        assert (v[:, src] != v[:, shifted]).any()
