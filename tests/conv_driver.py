"""The one driver of the conv launcher tests: a conv problem (drawn from a seed or given), its input buffer filled by the
library's conversion kernel, an output buffer laid out by a policy, one descriptor array, the launch through the form's
entry point, and the slices read back on the host after an exact check that nothing else was written.  tests/test_conv_gpu.py,
test_wino_numerics_gpu.py, test_wino7_f8_gpu.py, test_bf16_gpu.py, test_bf16x3_gpu.py, test_conv_input_slices_gpu.py and
test_conv_forward_exact_gpu.py run their launches through it; `pack` and `call` are the only places that map a form to a packer and a launcher.

The tolerances and references those files (and the CPU files beside them) share live here as well, one definition each.
Importing this module touches neither the GPU nor the library: `capi` and the device are arguments."""
import ctypes as C
import json
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import layout_restate as lr
import wino7_f8_restate as f87

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-4            # fp32 direct and every Winograd form but F(8,7): relative to max(1, max|ref|); fma chain vs ATen order
X3_TOL = 3e-5         # bf16x3 against the exact fp32-operand conv (test_conv_bf16x3_is_fp32_grade has the derivation)
STEM7_TOL = 2e-4      # rtpose_conv7x7_s2 against conv2d (tests/test_hourglass_gpu.py)
U = 2.0 ** -24
SENTINEL = 0x7FC12345          # a quiet NaN with a recognisable payload

# gamma limits (own receptive field; dilated S for the spatially heterogeneous inputs).  Measured on MI355X (see
# profiles/r03_wino_gamma.json / DESIGN.md §3.0): the limits are ~2x the worst measured value of each form.
# Worst measured (28 input x filter statistics each): direct3 30, F(2x2,3x3) 18, direct7 120, F(4,7) 277, F(6,7) 439;
# zero-mean Gaussian inputs and filters: 4.3, 2.1, 5.3, 51, 108.
GAMMA_LIMIT = {"direct3": 64.0, "F(2x2,3x3)": 48.0, "F(4x4,3x3)": 100.0, "direct7": 256.0, "F(4,7)": 600.0,
               "F(6,7)": 1000.0}
HETEROGENEOUS = ("logu_px", "heavy")
INPUT_KINDS = ("randn", "relu", "relu_mean", "logu_ch", "logu_px", "ramp", "heavy")


def gamma_limit_f87(wts):
    """F(6,7)'s limit scaled by the ratio of the two forms' amplification for THIS filter bank, from the exact rational
    tables (not from the code under test): the element-wise error bound of a form is proportional to it."""
    return GAMMA_LIMIT["F(6,7)"] * f87.amp_exact(wts.numpy(), 8) / f87.amp_exact(wts.numpy(), 6)


def inputs(kind, n, c, h, w, g):
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    if kind == "randn":
        return r(n, c, h, w)
    if kind == "relu":                     # non-negative, mean ~ std
        return F.relu(r(n, c, h, w))
    if kind == "relu_mean":                # non-negative, mean >> std (100x)
        return F.relu(r(n, c, h, w)) * 0.05 + 5.0
    if kind == "logu_ch":                  # channel magnitudes log-uniform over six decades
        return r(n, c, h, w) * 10.0 ** (torch.rand(1, c, 1, 1, generator=g) * 6 - 3)
    if kind == "logu_px":                  # every element its own magnitude, six decades
        return r(n, c, h, w) * 10.0 ** (torch.rand(n, c, h, w, generator=g) * 6 - 3)
    if kind == "ramp":                     # smooth ramps on a large offset
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        return 100.0 + 0.7 * xx + 0.3 * yy + 0.01 * r(n, c, h, w)
    if kind == "heavy":                    # heavy-tailed, non-negative
        return r(n, c, h, w).abs() ** 4
    raise KeyError(kind)


def weights(kind, cout, cin, k, g):
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    he = (2.0 / (cin * k * k)) ** 0.5
    if kind == "he":
        return r(cout, cin, k, k) * he
    if kind == "pos":                      # all-positive filters: nothing cancels in the direct sum
        return r(cout, cin, k, k).abs() * he
    if kind == "smooth":                   # separable Gaussian bumps (what trained 7x7 filters tend to)
        t = torch.arange(k, dtype=torch.float32) - k // 2
        gk = torch.exp(-t * t / (2 * (k / 4.0) ** 2))
        return (gk[:, None] * gk[None, :])[None, None] * r(cout, cin, 1, 1) * he
    if kind == "ref_init_x30":             # the reference's own init N(0, 0.01) (rtpose_vgg.py:200-222), scaled up
        return r(cout, cin, k, k) * 0.3
    raise KeyError(kind)


def ref64(x, wts, bias, k, dil):
    """float64 direct sum and the bound quantity S (with |x| dilated by `dil` = (ry, rx) pixels if given)."""
    y = F.conv2d(x.double(), wts.double(), bias.double(), padding=k // 2)
    ax = x.abs().double()
    if dil is not None:
        ry, rx = dil
        ax = F.max_pool2d(ax, (2 * ry + 1, 2 * rx + 1), stride=1, padding=(ry, rx))
    s = F.conv2d(ax, wts.abs().double(), bias.abs().double(), padding=k // 2)
    return y, s


def note(name, obj):
    """Measured figures of a passing test, for DESIGN.md / profiles/ (gpurun_out/ travels back from the GPU box)."""
    out = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)
    except OSError:
        pass


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def check_bf16(out, ref, out_f32):
    scale = max(1.0, ref.abs().max().item())
    if out_f32:
        err = (out - ref).abs().max().item()
        assert err <= 2e-5 * scale, "fp32-out max abs err %g (scale %g)" % (err, scale)
    else:
        # within one bf16 ulp of the rounded reference (an fp32 sum that differs in the last
        # bits may round the other way); 2^-7 relative + a denormal-free floor
        rr = rb(ref)
        err = (out - rr).abs()
        bound = rr.abs() * 2.0 ** -7 + 1e-6 * scale
        bad = (err > bound).sum().item()
        assert bad == 0, "%d outputs further than 1 bf16 ulp from the reference (max err %g)" % (
            bad, err.max().item())
        exact = (out == rr).float().mean().item()
        assert exact > 0.98, "only %.3f of the outputs equal the RNE-rounded reference" % exact


# ---- the form of a launch, and the one ladder -----------------------------------------------------------------------------------
# kind: 'f32' | 'bf16' | 'x3'
# m:    None = the direct kernel; 0 = the library's default Winograd form (the k-generic packer, wino_m = 0); else the m of
#       F(m x m, 3x3) / F(m, 7) with the packer of that k
# entry: None = the form's usual launcher (rtpose_conv2d, rtpose_conv2d_winograd_ex, rtpose_conv2d_bf16, rtpose_conv2d_bf16x3);
#       'noex' = rtpose_conv2d_winograd; 'c64' = rtpose_conv3x3_c64_bf16
Form = namedtuple("Form", "kind k m out_f32 entry", defaults=(None, False, None))


def _packer(lib, form, cout, cin_p):
    """(elements of the packed filters, the packer, its k-or-m argument)"""
    k = form.k
    if form.kind == "bf16":
        return lib.rtpose_packed_weight_bytes_bf16(cout, cin_p, k) // 2, lib.rtpose_pack_conv_weights_bf16, k
    if form.kind == "x3":
        return lib.rtpose_packed_weight_bytes_bf16x3(cout, cin_p, k) // 2, lib.rtpose_pack_conv_weights_bf16x3, k
    if form.m is None:
        return lib.rtpose_packed_weight_floats(cout, cin_p, k), lib.rtpose_pack_conv_weights, k
    if form.m == 0:
        return lib.rtpose_packed_weight_floats_winograd(cout, cin_p, k), lib.rtpose_pack_conv_weights_winograd, k
    if k == 3:
        return lib.rtpose_packed_weight_floats_winograd3(cout, cin_p, form.m), lib.rtpose_pack_conv_weights_winograd3, form.m
    return lib.rtpose_packed_weight_floats_winograd7(cout, cin_p, form.m), lib.rtpose_pack_conv_weights_winograd7, form.m


def packed_numel(capi, form, cout, cin_p):
    return _packer(capi.lib, form, cout, cin_p)[0]


def pack(capi, dev, form, wt, b, cin_p, into=None):
    """wt [cout, cin, k, k], b [cout] (CPU or device fp32) -> (packed filters, packed bias) on the device, by the form's packer;
    into: the zeroed destination of the filters, where the caller places them itself."""
    cout, cin = wt.shape[:2]
    numel, fn, arg = _packer(capi.lib, form, cout, cin_p)
    wp = into if into is not None else torch.zeros(numel, device=dev, dtype=torch.float32 if form.kind == "f32" else torch.bfloat16)
    assert wp.numel() == numel
    bp = torch.zeros(capi.lib.rtpose_packed_bias_floats(cout), device=dev)
    wd, bd = wt.contiguous().to(dev), b.contiguous().to(dev)
    capi.check(fn(capi.ptr(wd), capi.ptr(bd), cout, cin, arg, None, cin_p, capi.ptr(wp), capi.ptr(bp), capi.current_stream()))
    torch.cuda.synchronize()            # (wd / bd may go once the pack kernel has run)
    return wp, bp


def call(capi, dev, form, descs, groups, n, h, w, scratch=True):
    """The launch of `descs` by the form's entry point.  A Winograd launch through rtpose_conv2d_winograd_ex gets the caller's
    hand-over scratch if `scratch` (the library allocates nothing), and its device error word must then be 0."""
    lib, stream = capi.lib, capi.current_stream()
    if form.entry == "c64":
        assert groups == 1 and lib.rtpose_conv3x3_c64_bf16_fits(descs, 1, n, h, w) == 1
        capi.check(lib.rtpose_conv3x3_c64_bf16(descs, n, h, w, stream), "rtpose_conv3x3_c64_bf16")
    elif form.kind == "bf16":
        capi.check(lib.rtpose_conv2d_bf16(descs, groups, n, h, w, int(form.out_f32), stream), "rtpose_conv2d_bf16")
    elif form.kind == "x3":
        capi.check(lib.rtpose_conv2d_bf16x3(descs, groups, n, h, w, int(form.out_f32), stream), "rtpose_conv2d_bf16x3")
    elif form.m is None:
        capi.check(lib.rtpose_conv2d(descs, groups, n, h, w, stream), "rtpose_conv2d")
    else:
        assert lib.rtpose_conv2d_winograd_fits(descs, n, h, w) == 1
        if form.entry == "noex":
            capi.check(lib.rtpose_conv2d_winograd(descs, groups, n, h, w, stream), "rtpose_conv2d_winograd")
        else:
            sc = torch.zeros(lib.rtpose_conv2d_winograd_scratch_bytes() // 4, dtype=torch.int32, device=dev) if scratch else None
            capi.check(lib.rtpose_conv2d_winograd_ex(descs, groups, n, h, w, capi.ptr(sc) if scratch else None,
                                                     sc.numel() * 4 if scratch else 0, stream), "rtpose_conv2d_winograd_ex")
            if scratch:
                word = C.c_int(-1)
                capi.check(lib.rtpose_conv2d_winograd_scratch_error(capi.ptr(sc), C.byref(word), stream))
                assert word.value == 0, "device error word %d" % word.value
    torch.cuda.synchronize()


# ---- the problem: inputs, one filter bank per branch, references (CPU; no library call) --------------------------------------------
def reference(form, x, wt, b, relu, pool, slopes, dtype=torch.float64):
    """conv2d (+ ReLU / PReLU / 2x2 max-pool) of the operands the launcher sees, in `dtype` arithmetic"""
    wq = rb(wt) if form.kind == "bf16" else wt          # (bf16: x is rounded already; bf16x3: the exact fp32-operand conv)
    y = F.conv2d(x.to(dtype), wq.to(dtype), b.to(dtype), padding=form.k // 2)
    if relu:
        y = F.relu(y)
    if slopes is not None:
        y = torch.where(y >= 0, y, slopes.to(dtype).view(1, -1, 1, 1) * y)
    if pool:
        y = F.max_pool2d(y, 2, 2, 0)
    return y


def given(form, xs, wts, biases, relu=0, pool=0, slopes=None, cin_pad=None):
    """A problem from explicit CPU tensors: xs [n, cin, h, w] (one, or one per branch), one filter bank per branch."""
    n, cin, h, w = xs[0].shape
    unit = 8 if form.kind == "f32" else 16
    return SimpleNamespace(form=form, n=n, h=h, w=w, cin=cin, cin_p=cin_pad or (cin + unit - 1) // unit * unit,
                           cout=wts[0].shape[0], relu=int(relu), pool=int(pool), groups=len(wts), xs=xs, wts=wts, biases=biases,
                           slopes=slopes or [None] * len(wts), refs=[None] * len(wts), wp=[], bp=[], sl=[])


def problem(form, n, h, w, cin, cout, relu=1, pool=0, prelu=0, groups=1, seed=0, ninputs=1, only_images=None, first_image=0,
            cin_pad=None, ref=torch.float64):
    """A problem drawn from `seed`: the inputs, then per branch filters, bias and (PReLU) slopes.  only_images / first_image:
    the same random stream, but only some images of the batch go through the kernel.  ref: the arithmetic of the references
    (P.refs), None = none (the CPU reference is the slow part of a case)."""
    g, k = torch.Generator().manual_seed(seed), form.k
    xs = [torch.randn(n, cin, h, w, generator=g) for _ in range(ninputs)]
    if form.kind == "bf16":
        xs = [rb(x) for x in xs]
    if only_images:
        xs = [x[first_image:first_image + only_images] for x in xs]
    wts, biases, slopes = [], [], []
    for _ in range(groups):
        wts.append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        biases.append(torch.randn(cout, generator=g) * 0.1)
        slopes.append((torch.rand(cout, generator=g) * 0.5 - 0.1) if prelu else None)
    P = given(form, xs, wts, biases, relu, pool, slopes, cin_pad)
    if ref is not None:
        P.refs = [reference(form, xs[gi % ninputs], wts[gi], biases[gi], relu, pool, slopes[gi], ref) for gi in range(groups)]
    return P


def pack_all(capi, dev, P):
    """the filters of every branch packed on the device (P.wp, P.bp), the slopes beside them (P.sl)"""
    for wt, b, sl in zip(P.wts, P.biases, P.slopes):
        wp, bp = pack(capi, dev, P.form, wt, b, P.cin_p)
        P.wp.append(wp)
        P.bp.append(bp)
        P.sl.append(None if sl is None else sl.to(dev))
    return P


# ---- input ---------------------------------------------------------------------------------------------------------------------
def L(capi, lay):
    return capi.Layout(lay.cstride, lay.choff, lay.ws, lay.hs, lay.lead)


def npx(capi, lay, n, h, w):
    return capi.lib.rtpose_layout_pixels(C.byref(L(capi, lay)), n, h, w)


def to_layout(capi, dev, P, x, pad_in, lead_extra=0):
    """x -> (compact input buffer on the device, its lr.Lay: cstride = the slice's elements, choff = 0), filled by the
    library's conversion kernel of the form's element type.  lead_extra: pixels of lead on top of the padding's."""
    lib, kind = capi.lib, P.form.kind
    lay = lr.padded((2 if kind == "x3" else 1) * P.cin_p, P.h, P.w, pad_in)
    lay = lay._replace(lead=lay.lead + lead_extra)
    buf = torch.zeros(npx(capi, lay, P.n, P.h, P.w) * lay.cstride, device=dev, dtype=torch.float32 if kind == "f32" else torch.bfloat16)
    fn = {"f32": lib.rtpose_nchw_to_layout, "bf16": lib.rtpose_nchw_to_layout_bf16, "x3": lib.rtpose_nchw_to_layout_split}[kind]
    xd = x.contiguous().to(dev)
    capi.check(fn(capi.ptr(xd), capi.ptr(buf), C.byref(L(capi, lay)), P.cin, P.cin_p, P.n, P.h, P.w, capi.current_stream()))
    torch.cuda.synchronize()
    return buf, lay


# ---- output policy -------------------------------------------------------------------------------------------------------------
# One buffer for all branches.  A branch's slice is `cout` channels rounded up to `piece`; a pixel holds the slices side by
# side and `extra` more channels, the first slice at channel `choff`; every word is `fill` before the launch.  (Split bf16x3
# outputs count two elements per channel.)  The gap between rows and images is the launch's pad_out.
Out = namedtuple("Out", "extra choff fill piece", defaults=(0, 1))
ODD = Out(3, 1)                 # odd stride + channel offsets: scalar stores
ALIGNED = Out(16, 8)            # 16-byte aligned slices, the layout the network uses
PIECES = Out(8, 8, 0, 8)        # bf16x3: 8-channel pieces
PLAIN = Out(0, 0)               # cstride = cout (one branch)


def sentinel(choff, extra_c):
    """every word outside the slices must still hold SENTINEL, every word inside a finite value"""
    return Out(extra_c, choff, SENTINEL)


def out_layouts(P, out, pad_out):
    """(elements per pixel, [lr.Lay per branch], element type, split)"""
    form = P.form
    ho, wo = (P.h // 2, P.w // 2) if P.pool else (P.h, P.w)
    split = form.kind == "x3" and not form.out_f32
    e = 2 if split else 1
    cw = (P.cout + out.piece - 1) // out.piece * out.piece
    cso = e * (cw * P.groups + out.extra)
    dt = torch.float32 if (form.kind == "f32" or form.out_f32) else torch.bfloat16
    return cso, [lr.padded(cso, ho, wo, pad_out, e * (gi * cw + out.choff)) for gi in range(P.groups)], dt, split


# ---- launch and read-back ---------------------------------------------------------------------------------------------------------
def launch(capi, dev, P, inputs, out, pad_out, scratch=True, hook=None, into=None):
    """inputs: one (buffer, lr.Lay) per branch.  Returns the output buffer (device) and its per-branch layouts.
    hook(gi, desc, obuf, lout): sets the fields of a branch's descriptor the driver has no argument for (out_cmap, residual,
    in_scale ...) before the launch; into: an output buffer of an earlier launch of the same problem and policy, written again."""
    form = P.form
    if not P.wp:
        pack_all(capi, dev, P)
    ho, wo = (P.h // 2, P.w // 2) if P.pool else (P.h, P.w)
    cso, louts, dt, _ = out_layouts(P, out, pad_out)
    ibits = torch.int32 if dt == torch.float32 else torch.int16
    obuf = into if into is not None else torch.full((npx(capi, louts[0], P.n, ho, wo) * cso,), out.fill, dtype=ibits,
                                                    device=dev).view(dt)
    descs = (capi.ConvDesc * P.groups)()            # zero-initialised: every field the form does not use stays 0
    for gi, (buf, lay) in enumerate(inputs):
        d = descs[gi]
        d.inp, d.w_packed, d.bias_packed, d.out = buf.data_ptr(), P.wp[gi].data_ptr(), P.bp[gi].data_ptr(), obuf.data_ptr()
        d.lin, d.lout = L(capi, lay), L(capi, louts[gi])
        d.cin, d.cout, d.k, d.relu, d.pool = P.cin_p, P.cout, form.k, P.relu, P.pool
        d.wino_m = form.m or 0
        if P.sl[gi] is not None:
            d.prelu = P.sl[gi].data_ptr()
        if hook is not None:
            hook(gi, d, obuf, louts[gi])
    call(capi, dev, form, descs, P.groups, P.n, P.h, P.w, scratch)
    return obuf, louts


def np_bits(t):
    t = t.cpu()
    return t.view(torch.int32).numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def outputs(P, obuf, louts, out, values=True, cmaps=None, pieces=None):
    """The branches' outputs [n, cout, ho, wo] (CPU fp32; values = False: none) read on the host through lr.index /
    lr.split_index (cmaps: per branch the absolute channels of an out_cmap launch, lr.index_map), after the exact check:
    every word of the output buffer outside the written slices still holds the policy's fill word, bit for bit.
    pieces: a list that receives, per branch of a split bf16x3 output, the (hi, lo) words as float32 [n, cout, ho, wo]."""
    ho, wo = (P.h // 2, P.w // 2) if P.pool else (P.h, P.w)
    split = P.form.kind == "x3" and not P.form.out_f32
    bits = np_bits(obuf)
    outs, written = [], []
    for gi, lo in enumerate(louts):
        if split:
            ih, il = lr.split_index(lo, P.n, ho, wo, P.cout)
            written += [ih, il]
            v = (lr.bf16_to_f32(bits[ih]) + lr.bf16_to_f32(bits[il])) if values else None
            if pieces is not None:
                pieces.append(tuple(np.ascontiguousarray(np.transpose(lr.bf16_to_f32(bits[i]), (0, 3, 1, 2))) for i in (ih, il)))
        else:
            idx = lr.index(lo, P.n, ho, wo, P.cout) if cmaps is None else lr.index_map(lo, P.n, ho, wo, cmaps[gi])
            written.append(idx)
            v = (bits[idx].view(np.float32) if bits.dtype == np.uint32 else lr.bf16_to_f32(bits[idx])) if values else None
        outs.append(torch.from_numpy(np.ascontiguousarray(np.transpose(v, (0, 3, 1, 2)))) if values else None)
    assert lr.untouched(bits, written, out.fill), "the conv wrote outside its slice / into the gaps"
    if out.fill and values:
        for o in outs:
            assert torch.isfinite(o).all(), "a pixel of the slice was not written"
    return outs


def run(capi, dev, P, out, pad_in, pad_out, scratch=True, lead_extra=0):
    """One launch of the problem on a compact input: the branches' outputs [n, cout, ho, wo] (CPU fp32)."""
    buf, lay = to_layout(capi, dev, P, P.xs[0], pad_in, lead_extra)
    obuf, louts = launch(capi, dev, P, [(buf, lay)] * P.groups, out, pad_out, scratch)
    return outputs(P, obuf, louts, out)


def check(P, gi, out, x):
    """branch gi's output against its float64 reference, within the tolerance of the form"""
    form, ref = P.form, P.refs[gi]
    if form.kind == "bf16":
        check_bf16(out, ref.float(), form.out_f32)
    elif form.k == 7 and form.m == 8:        # the element-wise bound of test_f87_matches_direct_kernel_and_float64
        y64, s = ref64(x, P.wts[gi], P.biases[gi], 7, None)
        y64 = F.relu(y64) if P.relu else y64
        gamma = ((out.double() - y64).abs() / (U * s)).max().item()
        assert gamma <= gamma_limit_f87(P.wts[gi]), ("F(8,7) gamma", gamma)
    else:
        err = (out.double() - ref).abs().max().item()
        tol = X3_TOL if form.kind == "x3" else TOL
        assert err <= tol * max(1.0, ref.abs().max().item()), "max abs err %g" % err
