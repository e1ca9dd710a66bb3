"""Numerics of the Winograd forms that carry the fp32 headline (csrc/conv_wino.hip F(2x2,3x3), csrc/conv_wino7.hip
F(4,7) / F(6,7)) on HOSTILE statistics - what a trained rtpose_vgg (lib/network/rtpose_vgg.py:108-127 run with
pose_model.pth, README.md:19) feeds them and a zero-mean randn / He-init test never does: non-negative inputs with
mean >> std (post-ReLU), magnitudes spread over six decades, smooth ramps, heavy tails, all-positive and smooth
filters, the reference's own N(0, 0.01) init scaled up.

The claim tested is an ELEMENT-WISE ERROR BOUND against a float64 direct sum,

        |y - y64|  <=  gamma * 2^-24 * S,        S = sum |x| |w|  (+ |bias|)  over the output's receptive field,

the form every fp32 dot product obeys with gamma ~ its depth; a minimal-filtering form pays its transform
amplification on top (DESIGN.md §3.0 has the table of measured gammas; rtpose_winograd_amplification is the
data-independent estimate of the factor).  For inputs whose magnitude varies from pixel to pixel by decades the
Winograd error of an output depends on its tile neighbours too (the transforms mix m + r - 1 pixels), so there S is
taken over |x| dilated by one tile.  The measured gammas are written to gpurun_out/wino_gamma.json.

Then: the per-plan / per-layer choice of the form through the ABI (rtpose_net_options), the amplification estimate
against its exact definition (oracle/winograd_tables.py), whole-network runs on un-normalised inputs, large
activations and positive biases, the fp32 tier-B end-to-end check (GPU net -> GPU decode == oracle net -> oracle decode
on the 32 bench images, evaluate/coco_eval.py:270-272) and the runtime hardening (caller-owned scratch, graph replay
with persistent launches, hardware bounds clamp)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_driver as cd
import wino_cases as wc
from conv_driver import GAMMA_LIMIT, HETEROGENEOUS, INPUT_KINDS, U

pytestmark = pytest.mark.gpu


def _gpu_conv(capi, dev, x, wts, bias, k, form, relu=0, pool=0):
    """x [n,cin,h,w], wts [cout,cin,k,k] (CPU fp32) through the C ABI; form: 'direct', 3 (F(2x2,3x3): the library's default
    form, wino_m = 0), 43 (F(4x4,3x3)), 4 or 6 (F(m,7)).  The Winograd forms go through rtpose_conv2d_winograd."""
    fm = cd.Form("f32", k, {"direct": None, 3: 0, 43: 4}.get(form, form), entry="noex")
    P = cd.given(fm, [x], [wts], [bias], relu, pool, cin_pad=x.shape[1])
    return cd.run(capi, dev, P, cd.PLAIN, k // 2, 1)[0]


_GAMMAS = {}


def _record(form, kx, kw, g):
    _GAMMAS.setdefault(form, {})["%s/%s" % (kx, kw)] = round(float(g), 2)
    cd.note("wino_gamma.json", {"unit": "|err| / (2^-24 * sum|x||w|), worst element", "gamma": _GAMMAS,
                                "worst": {k: max(v.values()) for k, v in _GAMMAS.items()}})


@pytest.mark.parametrize("kw", ("he", "pos", "smooth", "ref_init_x30"))
def test_7x7_forms_elementwise_error_bound(capi, cuda, kw):
    """128 -> 128 at 2 x 46 x 46 (the Mconv2..5_stageN map).  One branch of two images is 24 tiles of F(6,7): twice that stays
    under the 256 CUs, so the launch runs the small-grid form wino7s_f32<1> - bit-identical to the headline instance
    wino7_f32<1,8,6,2>, which larger batches of this map select (tests/wino_cases.py, NUMERICS7); F(4,7) runs
    wino7_f32<1,12,4,1>."""
    g = torch.Generator().manual_seed(1000 + len(kw))
    n, h, w, c, cout = wc.NUMERICS7
    wts = cd.weights(kw, cout, c, 7, g)
    bias = torch.randn(cout, generator=g) * 0.1
    failures = []
    for kx in INPUT_KINDS:
        x = cd.inputs(kx, n, c, h, w, g)
        outs = {f: _gpu_conv(capi, cuda, x, wts, bias, 7, f) for f in ("direct", 4, 6)}
        for f, name, reach in (("direct", "direct7", 0), (4, "F(4,7)", 9), (6, "F(6,7)", 11)):
            het = kx in HETEROGENEOUS and reach
            y64, s = cd.ref64(x, wts, bias, 7, (0, reach) if het else None)
            gamma = ((outs[f].double() - y64).abs() / (U * s)).max().item()
            _record(name, kx, kw, gamma)
            if not gamma <= GAMMA_LIMIT[name]:
                failures.append((name, kx, kw, gamma))
    assert not failures, failures


@pytest.mark.parametrize("kw", ("he", "pos", "smooth", "ref_init_x30"))
def test_3x3_form_elementwise_error_bound(capi, cuda, kw):
    """F(2x2,3x3): 128 -> 128 (the <1,4,16> instance) and 64 -> 64 (conv1_2's <2,2,16>); F(4x4,3x3) (csrc/conv_wino4.hip,
    the plan default) on the same shapes - 46 x 46 and 48 x 40 maps: clamped patch rows / columns and exact tiles."""
    g = torch.Generator().manual_seed(2000 + len(kw))
    failures = []
    for (n, c, h, w, cout) in ((2, 128, 46, 46, 128), (1, 64, 48, 40, 64)):
        wts = cd.weights(kw, cout, c, 3, g)
        bias = torch.randn(cout, generator=g) * 0.1
        for kx in INPUT_KINDS:
            x = cd.inputs(kx, n, c, h, w, g)
            outs = {f: _gpu_conv(capi, cuda, x, wts, bias, 3, f) for f in ("direct", 3, 43)}
            for f, name in (("direct", "direct3"), (3, "F(2x2,3x3)"), (43, "F(4x4,3x3)")):
                het = kx in HETEROGENEOUS and f != "direct"
                y64, s = cd.ref64(x, wts, bias, 3, ((5, 5) if f == 43 else (3, 3)) if het else None)
                gamma = ((outs[f].double() - y64).abs() / (U * s)).max().item()
                _record(name, kx, kw, gamma)
                if not gamma <= GAMMA_LIMIT[name]:
                    failures.append((name, kx, kw, c, gamma))
    assert not failures, failures


def test_f43_kernel_against_its_cpu_restatement(capi, cuda):
    """csrc/conv_wino4.hip against oracle/winograd43_oracle.py (numpy float32, exact Toom-Cook matrices) on the same
    inputs: both are within gamma 2^-24 sum|x||w| of the float64 sum, so they are within twice that of each other - and
    in practice much closer, which is what the second assertion pins (same transforms, same rounding points; only the
    order of the channel sums differs)."""
    from oracle.winograd43_oracle import conv3x3_f43
    g = torch.Generator().manual_seed(43)
    for (n, cin, h, w, cout) in ((2, 32, 10, 13, 8), (1, 64, 8, 8, 64)):
        x = torch.randn(n, cin, h, w, generator=g)
        wts = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        bias = torch.randn(cout, generator=g) * 0.1
        y_gpu = _gpu_conv(capi, cuda, x, wts, bias, 3, 43)
        y_cpu = torch.from_numpy(np.stack([conv3x3_f43(x[i].numpy(), wts.numpy(), bias.numpy()) for i in range(n)]))
        _, s = cd.ref64(x, wts, bias, 3, None)
        d = (y_gpu.double() - y_cpu.double()).abs()
        assert (d / (U * s)).max().item() <= 2 * GAMMA_LIMIT["F(4x4,3x3)"]
        assert d.max().item() <= 2e-5 * max(1.0, y_cpu.abs().max().item())


# ---- amplification estimate and the choice of the form through the ABI ---------------------------------------

def _amp_exact(wts, k, m):
    """The definition in include/rtpose_mi355x.h from the exact Toom-Cook matrices (oracle/winograd_tables.py)."""
    from oracle.winograd_tables import toom_cook, POINTS_F4_7, POINTS_F6_7, POINTS_F2_3, POINTS_F4_3
    wd = wts.double().numpy()
    f = lambda M: np.array([[float(v) for v in row] for row in M])   # noqa: E731
    if k == 3:
        AT, G, BT = map(f, toom_cook(4, 3, POINTS_F4_3) if m == 4 else toom_cook(2, 3, POINTS_F2_3))
        Uf = np.einsum('ay,bx,ocyx->ocab', G, G, wd)
        a, b = np.abs(AT), np.abs(BT).sum(1)
        sfreq = np.abs(Uf).sum(1)
        num = np.einsum('ia,jb,oab->oij', a * b[None], a * b[None], sfreq).max((1, 2))
    else:
        AT, G, BT = map(f, toom_cook(m, 7, POINTS_F4_7 if m == 4 else POINTS_F6_7))
        Uf = np.einsum('fk,ocyk->ocyf', G, wd)
        a, b = np.abs(AT), np.abs(BT).sum(1)
        sfreq = np.abs(Uf).sum((1, 2))
        num = (a[None] * (b * sfreq)[:, None, :]).sum(2).max(1)
    return float((num / np.abs(wd).sum((1, 2, 3))).max())


def test_amplification_estimate_matches_its_definition(capi, cuda):
    lib = capi.lib
    g = torch.Generator().manual_seed(5)
    amp = torch.zeros(1, device=cuda)
    seen = {}
    for kind in ("he", "pos", "smooth"):
        for k, m in ((3, 0), (3, 4), (7, 4), (7, 6)):
            wts = cd.weights(kind, 24, 40, k, g)
            wd = wts.to(cuda)
            capi.check(lib.rtpose_winograd_amplification(capi.ptr(wd), 24, 40, k, m, capi.ptr(amp),
                                                         capi.current_stream()))
            got, want = amp.item(), _amp_exact(wts, k, m)
            assert abs(got - want) <= 2e-3 * want, (kind, k, m, got, want)
            seen[(kind, k, m)] = got
    # orientation: i.i.d. Gaussian filters ~3.3 / 62 / 115; F(6,7) amplifies more than F(4,7) for every kind, and
    # F(4x4,3x3) more than F(2x2,3x3)
    assert 2.5 < seen[("he", 3, 0)] < 4.5 and 40 < seen[("he", 7, 4)] < 90 and 80 < seen[("he", 7, 6)] < 160
    print("F(4x4,3x3) amplification estimates:", {k[0]: round(v, 1) for k, v in seen.items() if k[1:] == (3, 4)})
    for kind in ("he", "pos", "smooth"):
        assert seen[(kind, 7, 6)] > seen[(kind, 7, 4)] and seen[(kind, 3, 4)] > seen[(kind, 3, 0)]


@pytest.fixture(scope="module")
def model_and_sd(pkg, cuda):
    from oracle import net_oracle
    m = pkg.get_model('vgg19')
    sd = net_oracle.he_init_state_dict(m, seed=0)
    m.load_state_dict(sd)
    m = m.cuda().float().eval()
    return m, sd


def _forms(m, plan, k):
    return sorted({form for (nm, form, _), (_, mod) in zip(m.conv_numerics(plan), m._convs())
                   if mod.kernel_size[0] == k and mod.in_channels >= 32})


def test_form_is_chosen_per_plan_through_the_abi(model_and_sd, cuda):
    """rtpose_net_options: direct / F(4,7) / F(6,7) / per-layer AUTO by amplification limit, all from ONE weight
    arena; every choice stays inside the 1e-3 contract against the oracle and the forms really differ."""
    from oracle import net_oracle
    m, sd = model_and_sd
    x = torch.rand(2, 3, 64, 72, generator=torch.Generator().manual_seed(4)) - 0.5
    (paf_r, heat_r), _ = net_oracle.forward(sd, x)
    xd = x.to(cuda)
    outs = {}
    try:
        for name, kw, want7, want3 in (
                ("default", dict(), [6], [43]),
                ("direct", dict(winograd3=False, winograd7=0), [0], [0]),
                ("f47", dict(winograd7=4), [4], [43]),
                ("f67_w3off", dict(winograd3=False, winograd7=6), [6], [0]),
                ("f23", dict(winograd3=True), [6], [3]),
                ("auto_all", dict(winograd3='auto', winograd7='auto', amp_limit=1e9), [6], [43]),
                ("auto_f47", dict(winograd7='auto', amp_limit=90.0), [4], [43]),
                ("auto_none", dict(winograd3='auto', winograd7='auto', amp_limit=1.0), [0], [3])):
            m.set_winograd(**kw)
            plan = m.forward_native(xd, keep_intermediates=False)
            assert _forms(m, plan, 7) == want7, (name, _forms(m, plan, 7))
            assert _forms(m, plan, 3) == want3, (name, _forms(m, plan, 3))
            paf, heat = m.read_output(plan, 10).cpu(), m.read_output(plan, 11).cpu()
            assert (paf - paf_r).abs().max().item() <= 1e-3 and (heat - heat_r).abs().max().item() <= 1e-3, name
            assert m.device_status(plan) == 0
            outs[name] = (paf, heat)
            amps = [a for (_, _, a), (_, mod) in zip(m.conv_numerics(plan), m._convs()) if mod.kernel_size[0] == 7]
            assert all(40 < a[1] < 90 and 80 < a[2] < 160 and a[0] == 0 and a[3] == 0 for a in amps)
            amps3 = [a for (_, _, a), (_, mod) in zip(m.conv_numerics(plan), m._convs())
                     if mod.kernel_size[0] == 3 and mod.in_channels >= 32]
            assert all(a[3] > a[0] > 0 and a[1] == 0 for a in amps3)
    finally:
        m.set_winograd()
    assert len([k for k in m._weights if k[1] == 0]) == 1          # one fp32 arena served all eight plans
    assert torch.equal(outs["default"][0], outs["auto_all"][0])    # same forms, same bits
    assert torch.equal(outs["f47"][0], outs["auto_f47"][0])
    assert not torch.equal(outs["default"][0], outs["direct"][0])  # the forms differ by rounding ...
    assert not torch.equal(outs["default"][0], outs["f47"][0])
    assert not torch.equal(outs["default"][0], outs["f23"][0])
    assert (outs["default"][0] - outs["direct"][0]).abs().max().item() <= 2e-4   # ... and only by rounding


def _edge_filter_state_dict(sd, prefix):
    """`sd` with the 7x7 filters of conv `prefix` replaced by +-1 edge detectors (+c in column 0, -c in column 6 of
    every (output, input channel, row)): F(6,7) amplification estimate 273 > the default amp_limit 256, F(4,7) 156."""
    out = {k: v.clone() for k, v in sd.items()}
    w = out[prefix + ".weight"]
    c = (2.0 / (w.shape[1] * 14)) ** 0.5        # He scale for the 14 non-zero taps per input channel
    e = torch.zeros_like(w)
    e[:, :, :, 0] = c
    e[:, :, :, 6] = -c
    out[prefix + ".weight"] = e
    return out


def test_default_is_the_guarded_choice_and_one_hostile_layer_drops_alone(pkg, model_and_sd, cuda):
    """The library default of an fp32 plan (nothing set: what a user who loads pose_model.pth gets, README.md:19 /
    lib/network/rtpose_vgg.py:108-127) is the per-layer AUTO choice under amp_limit 256: with He filters every 7x7
    conv runs F(6,7) and every eligible 3x3 conv F(4x4,3x3) - bit for bit the forced plan - and with the filters of
    ONE 7x7 conv replaced by +-1 edge detectors (estimate 273) that conv's launch alone (both branches of the grouped
    grid) drops to F(4,7), the outputs staying inside the contract."""
    from oracle import net_oracle
    _, sd = model_and_sd
    x = torch.rand(2, 3, 64, 72, generator=torch.Generator().manual_seed(14)) - 0.5
    xd = x.to(cuda)
    m = pkg.get_model('vgg19')
    m.load_state_dict(sd)
    m = m.cuda().float().eval()
    with torch.no_grad():
        (p0, h0), _ = m(xd)
    plan = m.plan_for(xd)
    num = {nm: (form, amp) for nm, form, amp in m.conv_numerics(plan)}
    k7 = [nm for nm, mod in m._convs() if mod.kernel_size[0] == 7]
    k3 = [nm for nm, mod in m._convs() if mod.kernel_size[0] == 3 and mod.in_channels >= 32]
    assert all(num[nm][0] == 6 and num[nm][1][2] <= 256.0 for nm in k7)
    assert all(num[nm][0] == 43 and num[nm][1][3] <= 256.0 for nm in k3)
    m.set_winograd(winograd3=4, winograd7=6)                   # the forced forms of round 3
    try:
        with torch.no_grad():
            (p1, h1), _ = m(xd)
    finally:
        m.set_winograd()
    assert torch.equal(p0, p1) and torch.equal(h0, h1)

    sd_e = _edge_filter_state_dict(sd, "model3_1.4")
    m.load_state_dict(sd_e)
    (paf_r, heat_r), saved_r = net_oracle.forward(sd_e, x)
    with torch.no_grad():
        (p2, h2), saved = m(xd)
    num = {nm: (form, amp) for nm, form, amp in m.conv_numerics(plan)}
    assert 257.0 < num["model3_1.4"][1][2] < 290.0 and 140.0 < num["model3_1.4"][1][1] < 170.0, num["model3_1.4"]
    dropped = sorted(nm for nm in k7 if num[nm][0] != 6)
    assert dropped == ["model3_1.4", "model3_2.4"], dropped     # the grouped launch of the two branches, nothing else
    assert num["model3_1.4"][0] == 4 and num["model3_2.4"][0] == 4
    assert all(num[nm][0] == 43 for nm in k3)
    for a, b in zip(saved, saved_r):
        assert (a.cpu() - b).abs().max().item() <= 1e-3 * max(1.0, b.abs().max().item())
    assert m.device_status(plan) == 0


def test_channel_plane_buffers_follow_the_forms_of_their_convs(pkg, model_and_sd, cuda):
    """Round 4: the executor keeps a buffer as channel planes exactly while conv1_1 / F(4x4,3x3) launches are the only ones
    that touch it (csrc/net.hip: mark_plane_bufs).  A conv whose filters fail the amplification limit runs F(2x2,3x3), a
    pixel-major kernel: the buffers on both sides of it change storage - and are cleared first, the gaps of one storage being
    data of the other.  One 3x3 conv gets single-tap corner filters (F(4x4,3x3) estimate 205, the worst a 3x3 filter can do)
    under amp_limit 150: that conv alone leaves form 43, the maps stay in contract; with the He filters back, the first
    result returns bit for bit."""
    from oracle import net_oracle
    _, sd = model_and_sd
    x = torch.rand(2, 3, 64, 72, generator=torch.Generator().manual_seed(15)) - 0.5
    xd = x.to(cuda)
    m = pkg.get_model('vgg19')
    m.load_state_dict(sd)
    m = m.cuda().float().eval()
    m.set_winograd(winograd3='auto', winograd7='auto', amp_limit=150.0)
    k3 = [nm for nm, mod in m._convs() if mod.kernel_size[0] == 3 and mod.in_channels >= 32]
    with torch.no_grad():
        (p0, h0), _ = m(xd)
    plan = m.plan_for(xd)
    assert all(form == 43 for nm, form, _ in m.conv_numerics(plan) if nm in k3)
    sd_c = {k: v.clone() for k, v in sd.items()}
    wc = torch.zeros_like(sd_c["model0.12.weight"])
    wc[:, :, 2, 2] = (2.0 / wc.shape[1]) ** 0.5
    sd_c["model0.12.weight"] = wc
    m.load_state_dict(sd_c)
    (_, _), saved_r = net_oracle.forward(sd_c, x)
    with torch.no_grad():
        (_, _), saved = m(xd)
    num = {nm: (form, amp) for nm, form, amp in m.conv_numerics(plan)}
    assert 195.0 < num["model0.12"][1][3] < 215.0 and num["model0.12"][0] == 3, num["model0.12"]
    assert all(num[nm][0] == 43 for nm in k3 if nm != "model0.12")
    for a, b in zip(saved, saved_r):
        assert (a.cpu() - b).abs().max().item() <= 1e-3 * max(1.0, b.abs().max().item())
    m.load_state_dict(sd)
    with torch.no_grad():
        (p2, h2), _ = m(xd)
    assert all(form == 43 for nm, form, _ in m.conv_numerics(plan) if nm in k3)
    assert torch.equal(p0, p2) and torch.equal(h0, h2)
    assert m.device_status(plan) == 0


def test_auto_forms_follow_a_reload_made_through_a_sibling_plan(pkg, model_and_sd, cuda):
    """Plans of one module share ONE weight arena and the host re-packs through whichever plan sees the new
    parameters first.  Every other AUTO plan must re-decide its forms from the NEW filters' estimates (round-3 advisor
    finding: it kept the old ones): reload through plan A, then ask plan B - untouched since - for its numerics."""
    _, sd = model_and_sd
    m = pkg.get_model('vgg19')
    m.load_state_dict(sd)
    m = m.cuda().float().eval()
    xa = (torch.rand(1, 3, 64, 72, generator=torch.Generator().manual_seed(1)) - 0.5).to(cuda)
    xb = (torch.rand(2, 3, 64, 72, generator=torch.Generator().manual_seed(2)) - 0.5).to(cuda)
    with torch.no_grad():
        m(xa)
        (pb0, _), _ = m(xb)
    plan_a, plan_b = m.plan_for(xa), m.plan_for(xb)
    assert plan_a is not plan_b and plan_a.workspace.data_ptr() != plan_b.workspace.data_ptr()
    form_b = {nm: f for nm, f, _ in m.conv_numerics(plan_b)}
    assert form_b["model3_1.4"] == 6
    m.load_state_dict(_edge_filter_state_dict(sd, "model3_1.4"))
    with torch.no_grad():
        m(xa)                                                   # the re-pack goes through plan A
    num_b = {nm: (f, a) for nm, f, a in m.conv_numerics(plan_b)}   # straight to the C ABI on plan B's handle
    assert num_b["model3_1.4"][1][2] > 256.0, "plan B still reports the old filters' estimate"
    assert num_b["model3_1.4"][0] == 4 and num_b["model3_2.4"][0] == 4, "plan B kept forms chosen from the OLD filters"
    # and both plans run the same arithmetic for the same image
    with torch.no_grad():
        (pa, _), _ = m(xb[:1].contiguous())
        (pb, _), _ = m(xb)
    assert torch.equal(pa[0], pb[0]) and not torch.equal(pb, pb0)
    # back again through plan B this time; plan A follows
    m.load_state_dict(sd)
    with torch.no_grad():
        (pb1, _), _ = m(xb)
    assert torch.equal(pb1, pb0)
    assert {nm: f for nm, f, _ in m.conv_numerics(plan_a)}["model3_1.4"] == 6


def test_unknown_descriptor_form_is_refused(capi, cuda):
    """rtpose_conv_desc.wino_m of a descriptor that was not zero-initialised: refused, not run on the wrong packing."""
    lib = capi.lib
    d = (capi.ConvDesc * 1)()
    d[0].cin, d[0].cout, d[0].k = 32, 64, 3
    for bad in (1, 3, 6, 7, -1):
        d[0].wino_m = bad
        assert lib.rtpose_conv2d_winograd_fits(d, 1, 16, 16) == 0
        assert lib.rtpose_conv2d_winograd(d, 1, 1, 16, 16, capi.current_stream()) != 0
        assert "wino_m" in capi.last_error()
    d[0].k = 7
    d[0].wino_m = 5
    assert lib.rtpose_conv2d_winograd_fits(d, 1, 16, 16) == 0


def test_options_struct_is_validated(capi):
    lib = capi.lib
    h = C.c_void_p()
    bad = capi.NetOptions.make(0, 5, -1, 0.0)
    assert lib.rtpose_net_create_opts(1, 64, 64, C.byref(bad), C.byref(h)) != 0
    bad = capi.NetOptions.make(0, -1, 5, 0.0)
    assert lib.rtpose_net_create_opts(1, 64, 64, C.byref(bad), C.byref(h)) != 0
    short = capi.NetOptions.make(0, -1, -1, 0.0)
    short.struct_bytes = 8
    assert lib.rtpose_net_create_opts(1, 64, 64, C.byref(short), C.byref(h)) != 0
    assert "struct_bytes" in capi.last_error()


# ---- whole network on hostile statistics -----------------------------------------------------------------------

def _check_stages(m, sd, x, cuda, what):
    from oracle import net_oracle
    (_, _), saved_r = net_oracle.forward(sd, x)
    with torch.no_grad():
        (_, _), saved = m(x.to(cuda))
    worst = 0.0
    for i, (a, b) in enumerate(zip(saved, saved_r)):
        scale = max(1.0, b.abs().max().item())              # the contract's 1e-3 at the scale of the map
        rel = (a.cpu() - b).abs().max().item() / scale
        worst = max(worst, rel)
        assert rel <= 1e-3, "%s: stage output %d off by %g x max(1, max|ref|) (max|ref| %g)" % (what, i, rel, scale)
    return worst, max(b.abs().max().item() for b in saved_r)


@pytest.mark.parametrize("shape", [(2, 64, 72), (16, 368, 368)])
def test_network_on_unnormalised_inputs_large_activations_and_positive_biases(pkg, cuda, shape):
    """All 12 stage outputs within 1e-3 * max(1, max|ref|) of the oracle when (a) the input is raw pixel values
    (x = rand * 255, nobody subtracted 0.5), (b) the first layer is scaled so that late activations reach ~1e3,
    (c) every bias is +0.25: the post-ReLU activations of every layer are then non-negative with a mean well above
    their spread - the regime where transform-domain cancellation costs the Winograd forms most.
    At 2 x 64 x 72 the maps are 8 x 9 (small-grid kernels); at 16 x 368 x 368 the launches are the ones that carry the
    bench: the 46-wide wino7_f32<1,8,6,2> instance (16 x 12 strips x 2 branches = 384 tiles, persistent with split
    tiles) and persistent wino4_f32 rounds on every 3x3 layer."""
    from oracle import net_oracle
    n, h, w = shape
    m = pkg.get_model('vgg19')
    sd = net_oracle.he_init_state_dict(m, seed=3)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(n, 3, h, w, generator=g)
    m.load_state_dict(sd)
    m = m.cuda().float().eval()
    w0, mx0 = _check_stages(m, sd, x * 255.0, cuda, "x = rand * 255")
    plan = m.plan_for(x.to(cuda))
    forms = {f for _, f, _ in m.conv_numerics(plan)}
    assert {6, 43} <= forms, forms                 # the guarded default still selects the fast forms here
    sd_b = {k: (v * 1000.0 if k.startswith("model0.0.") else v.clone()) for k, v in sd.items()}
    m.load_state_dict(sd_b)
    w1, mx1 = _check_stages(m, sd_b, x - 0.5, cuda, "first layer x 1000")
    assert mx1 >= 500.0
    sd_c = {k: (torch.full_like(v, 0.25) if k.endswith(".bias") else v.clone()) for k, v in sd.items()}
    m.load_state_dict(sd_c)
    w2, mx2 = _check_stages(m, sd_c, x - 0.5, cuda, "all biases +0.25")
    assert m.device_status(plan) == 0
    cd.note("hostile_network_%dx%dx%d.json" % shape,
          {"unit": "worst |err| / max(1, max|ref|) over the 12 stage outputs", "x = rand * 255": [w0, mx0],
           "first layer x 1000": [w1, mx1], "all biases +0.25": [w2, mx2]})


def test_tier_b_fp32_end_to_end_keypoints_on_the_32_bench_images(pkg, model_and_sd, cuda):
    """SURVEY §7 'hard parts' (net -> post coupling), evaluate/coco_eval.py:270-272: for the 32 images of the
    bench workload the product - GPU forward (Winograd plan), blend, GPU decode - against the oracle chain - torch-CPU
    forward, the same blend in numpy, the C restatement of NMS + process_paf - on the SAME decoder input
    definition scene + 1e-3 * net_out.  The two nets differ by < 4e-5, the blended maps therefore by < 1 ulp; a
    peak's refined x8 coordinate can in principle flip between two bicubic samples that tie to 1e-7, so the assertion
    is: same people, same part assignment structure, every keypoint within 1 px and >= 99.8 % identical
    (measured: printed)."""
    from importlib import import_module
    from oracle import net_oracle, post_oracle
    synth = import_module(pkg.__name__ + ".synth")
    pipeline = import_module(pkg.__name__ + ".pipeline")
    m, sd = model_and_sd
    n = 32
    x = torch.rand(n, 3, 368, 368, generator=torch.Generator().manual_seed(0)) - 0.5
    heat_s, paf_s, _ = synth.make_batch(n, 368, 368, seed=100)
    est = pipeline.PoseEstimator(m)
    recs = est(x.to(cuda), (torch.from_numpy(heat_s).to(cuda), torch.from_numpy(paf_s).to(cuda)))
    tot = same = people = 0
    alpha = np.float32(1e-3)
    for i0 in range(0, n, 8):
        (paf_r, heat_r), _ = net_oracle.forward(sd, x[i0:i0 + 8])
        for j in range(8):
            i = i0 + j
            heat = (alpha * heat_r[j].permute(1, 2, 0).contiguous().numpy() + heat_s[i]).astype(np.float32)
            paf = (alpha * paf_r[j].permute(1, 2, 0).contiguous().numpy() + paf_s[i]).astype(np.float32)
            jl, r = post_oracle.paf_to_pose(heat, paf)
            got = recs[i]
            assert got["peaks"].shape == jl.shape, "image %d: %d vs %d peaks" % (i, len(got["peaks"]), len(jl))
            assert np.array_equal(got["parts"], r["parts"]), "image %d: person / part assignment differs" % i
            assert np.array_equal(got["peaks"][:, 3:5], jl[:, 3:5])           # ids and part types
            d = np.abs(got["peaks"][:, 0:2] - jl[:, 0:2])
            assert d.max() <= 1.0, "image %d: a keypoint moved by %g px" % (i, d.max())
            tot += len(jl)
            same += int((d.max(axis=1) == 0).sum())
            people += len(r["parts"])
    assert people >= 32 and tot >= 500
    cd.note("tier_b.json", {"images": n, "people": people, "keypoints": tot, "identical": same})
    assert same >= 0.998 * tot


# ---- runtime hardening ---------------------------------------------------------------------------------------------

def test_forward_allocates_nothing_and_graph_replay_covers_persistent_launches(pkg, capi, cuda, monkeypatch):
    """The hand-over scratch of the persistent 7x7 launches is part of the plan's workspace
    (rtpose_net_workspace_bytes): with 11 images (11 x 12 strips x 2 branches = 264 tiles on 256 CUs) the 7x7 layers
    run persistent blocks with split tiles, the launch list is captured into a hipGraph (RTPOSE_GRAPH=1) and the
    replayed forwards are bit-identical to the directly launched ones and to the same images in another batch."""
    from oracle import net_oracle
    lib = capi.lib
    x = torch.rand(11, 3, 368, 368, generator=torch.Generator().manual_seed(21)) - 0.5
    ref = None
    for graph in ("0", "1"):
        monkeypatch.setenv("RTPOSE_GRAPH", graph)
        m = pkg.get_model('vgg19')
        m.load_state_dict(net_oracle.he_init_state_dict(m, seed=0))
        m = m.cuda().float().eval()
        m.keep_intermediates = False
        free0 = torch.cuda.mem_get_info()[0]
        with torch.no_grad():
            outs = [m(x.to(cuda))[0] for _ in range(3)]
        plan = m.plan_for(x.to(cuda))
        assert lib.rtpose_net_graph_active(plan.handle) == int(graph)
        assert m.device_status(plan) == 0
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
        if ref is None:
            ref = outs[0]
            with torch.no_grad():
                (p3, h3), _ = m(x[:3].to(cuda))        # 72 tiles: one block per tile, no split
            assert torch.equal(p3, ref[0][:3]) and torch.equal(h3, ref[1][:3])
        else:
            assert torch.equal(outs[0][0], ref[0]) and torch.equal(outs[0][1], ref[1])
        del m, plan, free0


def test_reads_past_the_tensor_are_clamped_by_the_buffer_descriptor(capi, cuda):
    """The raw buffer descriptors of the Winograd kernels carry the real extent of the tensor they address
    (mfma_dev.h: make_rsrc): memory past the end of the input / the packed filters is never interpreted.  The
    input and the filters are placed in front of a NaN-filled region; outputs stay finite and equal to the run
    with a zero-filled neighbourhood.  F(4x4,3x3) - the plan default of 17 convs - is covered in all three launch
    forms: the 16 x 16 small-grid kernel (wino4s_f32), one round of 32 x 64 tiles, and persistent blocks
    (2 x 184 x 184 -> 133 m tiles x 2 column tiles = 266 tiles on 256 CUs: one round + 5 m tiles in the small form).
    The geometries: tests/wino_cases.py, CLAMP_CASES."""
    lib, Layout = capi.lib, capi.Layout
    stream = capi.current_stream()
    g = torch.Generator().manual_seed(3)
    for k, form, (n, cin, cout, h, w) in [row for _, row in wc.CLAMP_CASES]:
        pad = k // 2
        x = torch.randn(n, cin, h, w, generator=g).to(cuda)
        wts = (torch.randn(cout, cin, k, k, generator=g) * 0.05).to(cuda)
        b = torch.zeros(cout, device=cuda)
        lin = Layout.padded(cin, h, w, pad)
        lout = Layout.padded(cout, h, w, 1)
        nin = lib.rtpose_layout_pixels(C.byref(lin), n, h, w) * cin
        fm = cd.Form("f32", k, {3: 0, 43: 4}.get(form, form))
        nw = cd.packed_numel(capi, fm, cout, cin)
        res = []
        for fill in (0.0, float("nan")):
            arena = torch.full((nin + nw + (1 << 20),), fill, device=cuda)
            xin, wp = arena[:nin], arena[nin:nin + nw]
            xin.zero_()
            wp.zero_()
            capi.check(lib.rtpose_nchw_to_layout(capi.ptr(x), capi.ptr(xin), C.byref(lin), cin, cin, n, h, w, stream))
            _, bp = cd.pack(capi, cuda, fm, wts, b, cin, into=wp)
            obuf = torch.zeros(lib.rtpose_layout_pixels(C.byref(lout), n, h, w) * cout, device=cuda)
            d = (capi.ConvDesc * 1)()
            d[0].inp, d[0].w_packed, d[0].bias_packed, d[0].out = xin.data_ptr(), wp.data_ptr(), bp.data_ptr(), obuf.data_ptr()
            d[0].lin, d[0].lout = lin, lout
            d[0].cin, d[0].cout, d[0].k, d[0].relu, d[0].pool = cin, cout, k, 0, 0
            d[0].wino_m = form if k == 7 else 4 if form == 43 else 0
            capi.check(lib.rtpose_conv2d_winograd(d, 1, n, h, w, stream), "rtpose_conv2d_winograd")
            o = torch.empty(n, cout, h, w, device=cuda)
            capi.check(lib.rtpose_layout_to_nchw(capi.ptr(obuf), C.byref(lout), capi.ptr(o), cout, n, h, w, stream))
            torch.cuda.synchronize()
            res.append(o.cpu())
        what = "k=%d form %d at %dx%dx%d" % (k, form, n, h, w)
        assert torch.isfinite(res[1]).all(), "%s: a read past the tensor reached the outputs" % what
        assert torch.equal(res[0], res[1]), what
        if form == 43:   # and it is the convolution: against torch's CPU conv2d
            ref = F.conv2d(x.cpu(), wts.cpu(), b.cpu(), padding=1)
            assert (res[1] - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item()), what
