"""OpenPose_Model on the MI355X: the native fp32 forward (rtpose_openpose_create, csrc/net.hip) against the reference
outputs (tests/golden/openpose_small.npz) and the CPU restatement (tests/openpose_restate.py), its batch invariance and
independence of what an earlier forward left in the workspace; the PReLU epilogue of the conv kernels, the launchers
that refuse it; the decoder path through PoseEstimator."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import openpose_restate as R  # noqa: E402
import wino_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "openpose_small.npz")
CONFIGS = ((4, 2, 38, 19), (4, 2, 14, 9))


@pytest.fixture(scope="module")
def op(pkg):
    return importlib.import_module(pkg.__name__ + ".openpose")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _model(op, cfg, seed, winograd3=None):
    m = op.OpenPose_Model(*cfg)
    sd = R.seeded_state_dict(R.state_dict_spec(*cfg), seed)
    m.load_state_dict(sd)
    if winograd3 is not None:
        m.set_winograd(winograd3)
    return m.cuda().eval(), sd


def _check(outs, refs, what):
    for i, (a, b) in enumerate(zip(outs, refs)):
        b = torch.as_tensor(b)
        mx = b.abs().max().item()
        assert 0.1 <= mx <= 100.0, "%s: stage output %d max|value| %g (vanishing / exploding maps)" % (what, i, mx)
        err = (a.cpu() - b).abs().max().item()
        assert err <= 1e-3 * max(1.0, mx), "%s: stage output %d max abs err %g (ref max %g)" % (what, i, err, mx)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_forward_matches_the_reference_golden_outputs(op, gold, cuda, cfg):
    tag = "c%d_%d_%d_%d" % cfg
    m, _ = _model(op, cfg, int(gold["seed"]))
    with torch.no_grad():
        last, (paf_ret, heat_ret) = m(torch.from_numpy(gold["x"]).to(cuda))
    assert len(paf_ret) == cfg[0] and len(heat_ret) == cfg[1]
    assert last[0][0] is paf_ret[-2] and last[1][1] is heat_ret[-1]
    _check(paf_ret + heat_ret, [gold["%s_out%d" % (tag, i)] for i in range(cfg[0] + cfg[1])], tag)


@pytest.mark.parametrize("w3", [0, 1, 4, 'auto'])
def test_odd_map_sizes_match_the_restatement_in_every_3x3_form(op, cuda, w3):
    cfg = (2, 2, 38, 19)
    m, sd = _model(op, cfg, 11, w3)
    x = torch.rand(3, 3, 100, 76, generator=torch.Generator().manual_seed(5)) - 0.5  # pools floor at every level
    with torch.no_grad():
        _, (paf_ret, heat_ret) = m(x.to(cuda))
        paf_r, heat_r = R.forward(sd, x, cfg[0], cfg[1])
    forms = {f for _, f, _ in m.conv_numerics(m.plan_for(x.to(cuda)))}
    want = {0: {0}, 1: {0, 3}, 4: {0, 43}, 'auto': {0, 43, 3}}[w3]
    assert forms <= want and (w3 == 0 or forms - {0}), (w3, forms)
    _check(paf_ret + heat_ret, paf_r + heat_r, "winograd3=%s" % (w3,))


def test_a_32_image_368_batch_matches_the_restatement(op, cuda):
    cfg = (4, 2, 38, 19)
    m, sd = _model(op, cfg, 3)
    x = torch.rand(32, 3, 368, 368, generator=torch.Generator().manual_seed(8)) - 0.5
    with torch.no_grad():
        _, (paf_ret, heat_ret) = m(x.to(cuda))
        for i in (0, 31):
            paf_r, heat_r = R.forward(sd, x[i:i + 1], cfg[0], cfg[1])
            _check([t[i:i + 1] for t in paf_ret + heat_ret], paf_r + heat_r, "image %d" % i)


def test_an_images_maps_are_the_same_bits_in_every_batch_size(op, cuda):
    m, _ = _model(op, (4, 2, 38, 19), 3)
    x = (torch.rand(12, 3, 368, 368, generator=torch.Generator().manual_seed(9)) - 0.5).to(cuda)
    with torch.no_grad():
        ref = {}
        for i in (0, 4, 11):
            _, (p, h) = m(x[i:i + 1])
            ref[i] = [t.clone() for t in p + h]
        for n in (5, 12):
            _, (p, h) = m(x[:n])
            for i, r in ref.items():
                if i < n:
                    assert all(torch.equal(a[i:i + 1], b) for a, b in zip(p + h, r)), (n, i)


def test_a_forward_does_not_depend_on_what_an_earlier_one_left(op, capi, cuda):
    """The stage outputs live in slices of one stage-input buffer, and the PAF stages run before the heat-map stages write
    theirs: a stage that read an earlier forward's heat maps through zero taps would turn a NaN left there into NaN
    (0 x NaN).  After a forward on a NaN input and with NaN written into every PAF and heat-map position of that buffer,
    the next batch on the same plan gives the bits of a fresh plan."""
    cfg = (2, 2, 38, 19)
    lib = capi.lib
    x = (torch.rand(2, 3, 96, 80, generator=torch.Generator().manual_seed(4)) - 0.5).to(cuda)
    bad = x.clone()
    bad[0, :, 10:20, 10:20] = float('nan')
    bad[1] = float('nan')
    m1, _ = _model(op, cfg, 11)
    m2, _ = _model(op, cfg, 11)
    with torch.no_grad():
        m1(bad)
        plan = m1.plan_for(x)
        for which in (0, 1):
            base, lay, c, hh, ww = m1.output_view(plan, which)
            z = torch.zeros(x.shape[0], hh, ww, c, device=cuda)
            capi.check(lib.rtpose_layout_axpby(base, C.byref(lay), capi.ptr(z), c, x.shape[0], hh, ww, 0.0,
                                               float('nan'), None))
        capi.check(lib.rtpose_net_set_keep_intermediates(plan.handle, 0))
        assert torch.isnan(m1.read_output(plan, 1)).all() and torch.isnan(m1.read_output(plan, 3)).all()
        _, (p1, h1) = m1(x)
        _, (p2, h2) = m2(x)
    assert not any(torch.isnan(t).any() for t in p1 + h1)
    assert all(torch.equal(a, b) for a, b in zip(p1 + h1, p2 + h2))


# ---- kernels --------------------------------------------------------------------------------------------------------
def _launch(capi, cuda, n, h, w, cin, cout, k, form, slopes, seed=0, out_planes=False):
    """One conv + bias + PReLU through the C ABI (form 0: rtpose_conv2d, 2 / 4: rtpose_conv2d_winograd F(2x2,3x3) /
    F(4x4,3x3)) -> (NCHW result, F.prelu(F.conv2d(...)) reference)."""
    lib, L = capi.lib, capi.Layout
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, cin, h, w, generator=g) - 0.5
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.prelu(F.conv2d(x, wt, b, padding=k // 2), slopes)
    s = None
    lin = L.padded(cin, h, w, k // 2 if k > 1 else 0)
    xin = torch.zeros(lib.rtpose_layout_pixels(C.byref(lin), n, h, w) * cin, device=cuda)
    xd = x.to(cuda)
    capi.check(lib.rtpose_nchw_to_layout(capi.ptr(xd), capi.ptr(xin), C.byref(lin), cin, cin, n, h, w, s))
    wd, bd, sd = wt.to(cuda), b.to(cuda), slopes.to(cuda)
    bp = torch.zeros(lib.rtpose_packed_bias_floats(cout), device=cuda)
    if form == 0:
        wp = torch.zeros(lib.rtpose_packed_weight_floats(cout, cin, k), device=cuda)
        capi.check(lib.rtpose_pack_conv_weights(capi.ptr(wd), capi.ptr(bd), cout, cin, k, None, cin, capi.ptr(wp),
                                                capi.ptr(bp), s))
    else:
        wp = torch.zeros(lib.rtpose_packed_weight_floats_winograd3(cout, cin, form), device=cuda)
        capi.check(lib.rtpose_pack_conv_weights_winograd3(capi.ptr(wd), capi.ptr(bd), cout, cin, form, None, cin,
                                                          capi.ptr(wp), capi.ptr(bp), s))
    cs = cout + 5  # odd stride, offset slice: the kernel writes its slice only
    lout = L.padded(cs, h, w, 1, choff=8 if out_planes else 3)
    px = lib.rtpose_layout_pixels(C.byref(lout), n, h, w)
    obuf = torch.zeros(px * (((cs + 7) // 8 + 1) * 8 if out_planes else cs), device=cuda)
    d = capi.ConvDesc()
    d.inp, d.w_packed, d.bias_packed, d.out = xin.data_ptr(), wp.data_ptr(), bp.data_ptr(), obuf.data_ptr()
    d.lin, d.lout = lin, lout
    d.cin, d.cout, d.k, d.relu, d.pool = cin, cout, k, 0, 0
    d.wino_m = form
    d.prelu = sd.data_ptr()
    if out_planes:
        d.out_plane_pixels = px
    if form == 0:
        capi.check(lib.rtpose_conv2d(C.byref(d), 1, n, h, w, s), "rtpose_conv2d")
    else:
        assert lib.rtpose_conv2d_winograd_fits(C.byref(d), n, h, w) == 1
        capi.check(lib.rtpose_conv2d_winograd(C.byref(d), 1, n, h, w, s), "rtpose_conv2d_winograd")
    torch.cuda.synchronize()
    if out_planes:  # planes of 8 channels: channel c of pixel q at ((c / 8) * px + q) * 8 + c % 8
        o = obuf.view(-1, px, 8)
        lo = L.padded(8, h, w, 1)
        res = []
        for c0 in range(8, 8 + cout, 8):
            t = torch.empty(n, 8, h, w, device=cuda)
            plane = o[c0 // 8].contiguous()
            capi.check(lib.rtpose_layout_to_nchw(capi.ptr(plane), C.byref(lo), capi.ptr(t), 8, n, h, w, s))
            res.append(t)
        out = torch.cat(res, 1)[:, :cout]
        written = sum(o[c0 // 8].abs().sum().item() for c0 in range(8, 8 + cout, 8))
    else:
        out = torch.empty(n, cout, h, w, device=cuda)
        capi.check(lib.rtpose_layout_to_nchw(capi.ptr(obuf), C.byref(lout), capi.ptr(out), cout, n, h, w, s))
        written = out.abs().sum().item()
    torch.cuda.synchronize()
    assert abs(obuf.abs().sum().item() - written) <= 1e-3 * max(1.0, written), "wrote outside its slice"
    return out.cpu(), ref


# The kernel a case reaches depends on the grid against the device's CUs: tests/wino_cases.py has the rows, the F(4x4,3x3) ones
# beside the launch shape each selects on the MI355X's 256 (asserted on the CPU by tests/test_wino_reach_cpu.py).
@pytest.mark.parametrize("n,h,w,cin,cout,k,form,planes", [row for _, row in wc.PRELU_CASES])
def test_prelu_epilogue_in_every_form(capi, cuda, n, h, w, cin, cout, k, form, planes):
    slopes = torch.linspace(-1.5, 2.0, cout)  # negative slopes and slopes above 1
    out, ref = _launch(capi, cuda, n, h, w, cin, cout, k, form, slopes, out_planes=planes)
    assert (ref < 0).any() and (ref > 0).any()
    err = (out - ref).abs().max().item()
    assert err <= 2e-4 * max(1.0, ref.abs().max().item()), err


def test_launchers_without_a_prelu_epilogue_refuse_it(capi, cuda):
    lib = capi.lib
    sl = torch.ones(512, device=cuda)
    buf = torch.zeros(1 << 20, device=cuda)
    d = capi.ConvDesc()
    d.inp = d.w_packed = d.bias_packed = d.out = buf.data_ptr()
    d.lin = capi.Layout.padded(128, 8, 8, 3)
    d.lout = capi.Layout.padded(128, 8, 8, 3)
    d.cin, d.cout, d.k = 128, 128, 3
    d.prelu = sl.data_ptr()

    def refused(rc, who):
        assert rc == -1 and "PReLU" in capi.last_error(), (who, rc, capi.last_error())
    refused(lib.rtpose_conv2d_bf16(C.byref(d), 1, 1, 8, 8, 0, None), "bf16")
    refused(lib.rtpose_conv2d_bf16x3(C.byref(d), 1, 1, 8, 8, 0, None), "bf16x3")
    d.k = 7
    d.wino_m = 6
    refused(lib.rtpose_conv2d_winograd(C.byref(d), 1, 1, 8, 8, None), "F(6,7)")
    assert lib.rtpose_conv2d_winograd_fits(C.byref(d), 1, 8, 8) == 0
    d.wino_m = 0
    assert lib.rtpose_conv2d(C.byref(d), 1, 1, 8, 8, None) == -1  # the direct 7x7 has no PReLU instance
    d.k, d.cin = 3, 64
    assert lib.rtpose_conv3x3_c64_bf16_fits(C.byref(d), 1, 1, 8, 8) == 0
    refused(lib.rtpose_conv3x3_c64_bf16(C.byref(d), 1, 8, 8, None), "c64 bf16")
    d1, d2 = capi.ConvDesc(), capi.ConvDesc()
    for dd in (d1, d2):
        dd.inp = dd.w_packed = dd.bias_packed = dd.out = buf.data_ptr()
        dd.lin = dd.lout = capi.Layout.padded(128, 8, 8, 0)
        dd.k = 1
    d1.cin, d1.cout, d1.relu, d2.cin, d2.cout = 128, 128, 1, 128, 38
    assert lib.rtpose_conv1x1_pair_fits(C.byref(d1), C.byref(d2), 1) == 1
    d1.relu, d1.prelu = 0, sl.data_ptr()
    assert lib.rtpose_conv1x1_pair_fits(C.byref(d1), C.byref(d2), 1) == 0
    refused(lib.rtpose_conv1x1_pair(C.byref(d1), C.byref(d2), 1, 1, 8, 8, None), "1x1 pair")
    assert lib.rtpose_conv1x1_pair_bf16_fits(C.byref(d1), C.byref(d2), 1) == 0
    refused(lib.rtpose_conv1x1_pair_bf16(C.byref(d1), C.byref(d2), 1, 1, 8, 8, 0, None), "1x1 pair bf16")
    # PReLU with ReLU or a fused pool is refused by the launchers that have it
    d.k, d.cin, d.relu = 3, 128, 1
    assert lib.rtpose_conv2d(C.byref(d), 1, 1, 8, 8, None) == -1
    d.relu, d.pool = 0, 1
    assert lib.rtpose_conv2d(C.byref(d), 1, 1, 8, 8, None) == -1
    d.wino_m = 4
    assert lib.rtpose_conv2d_winograd_fits(C.byref(d), 1, 8, 8) == 0
    assert lib.rtpose_conv2d_winograd(C.byref(d), 1, 1, 8, 8, None) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


# ---- decoder path ---------------------------------------------------------------------------------------------------
def test_pose_estimator_records_match_the_oracle_and_the_pipelined_path(op, pkg, cuda):
    from oracle import post_oracle
    dec = importlib.import_module(pkg.__name__ + ".decode")
    synth = importlib.import_module(pkg.__name__ + ".synth")
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    m, _ = _model(op, (4, 2, 38, 19), 3)
    B, S = 4, 368

    def batch(r):
        g = torch.Generator().manual_seed(500 + r)
        h, p, _ = synth.make_batch(B, S, S, seed=600 + r)
        return (torch.rand(B, 3, S, S, generator=g) - 0.5).to(cuda), (torch.from_numpy(h).to(cuda),
                                                                      torch.from_numpy(p).to(cuda))

    def content(block):
        out = []
        for r in block:
            d = dec.parse_image(r)
            out.append((d["peaks"].view(np.uint32).tobytes(), d["parts"].tobytes(), d["score"].view(np.uint32).tobytes(),
                        d["flags"]))
        return out
    data = [batch(r) for r in range(2)]
    est = pipeline.PoseEstimator(m)
    want = []
    for x, scene in data:
        est(x, scene, scene_alpha=2e-2)                       # capacities settle
        bufs = est.enqueue(x, scene, scene_alpha=2e-2)
        recs = dec.fetch(bufs).copy()
        want.append(content(recs))
        # the maps the decoder read: the blended last PAF / heat maps, where the plan keeps them
        paf = m.read_output(bufs.plan, 3).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        heat = m.read_output(bufs.plan, 5).permute(0, 2, 3, 1).contiguous().cpu().numpy()
        humans = 0
        for i in range(B):
            d = dec.parse_image(recs[i])
            jl, ref = post_oracle.paf_to_pose(heat[i], paf[i])
            assert np.array_equal(d["peaks"][:, [0, 1, 3, 4]], jl[:, [0, 1, 3, 4]])
            assert np.array_equal(d["peaks"][:, 2].view(np.uint32), jl[:, 2].view(np.uint32))
            assert np.array_equal(d["parts"], ref["parts"])
            assert np.array_equal(d["score"].view(np.uint32), ref["score"].view(np.uint32))
            humans += len(d["parts"])
        assert humans > B
    order = [0, 1, 1, 0]
    prev, got = None, []
    for r in order:
        t = est.submit(*data[r], scene_alpha=2e-2)
        if prev is not None:
            got.append(content(est.collect(prev)[1].reshape(B, -1)))
        prev = t
    got.append(content(est.collect(prev)[1].reshape(B, -1)))
    torch.cuda.synchronize()
    for k, r in enumerate(order):
        assert got[k] == want[r], "step %d: the pipelined records differ from the serial path's" % k
