"""CPU suite: the conv launchers refuse a malformed descriptor on the host (csrc/conv_desc.h and the launchers' own form
checks).  Each row is a valid base descriptor with ONE fault: a launcher returns RTPOSE_E_INVAL (-1) with the fault named
in rtpose_last_error(), a `_fits` function returns 0.  No row is a descriptor a launcher accepts.

The rows carry NULL or fake device pointers, so the module runs only where no GPU is visible: there a refused descriptor
returns before any HIP call, and a launcher that wrongly accepted a row fails at its first HIP call instead of launching a
kernel on the fake pointers."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="the rows pass fake device pointers: they run where no GPU is visible")

FAKE = 1 << 20          # a device pointer no refused launch touches
N, H, W = 1, 8, 8


class Case:
    """The descriptors and arguments of one call: `a` (the conv, or the first conv of a pair / pointwise unit, one entry
    per group) and `b` (the second conv of a pair / unit), the tensor size and the launcher's flags."""

    def __init__(self, a, b=(), n=N, h=H, w=W, out_f32=0, wino_m=None):
        self.a, self.b = list(a), list(b)
        self.n, self.h, self.w, self.out_f32 = n, h, w, out_f32
        self.ngroups = len(self.a)
        if wino_m is not None:
            for d in self.a:
                d.wino_m = wino_m


def conv(capi, k, cin, cout, in_elems=None, out_elems=None, pin=None, pout=0, h=H, w=W, relu=1):
    d = capi.ConvDesc()
    d.inp = d.w_packed = d.bias_packed = d.out = FAKE
    d.lin = capi.Layout.padded(in_elems or cin, h, w, k // 2 if pin is None else pin)
    d.lout = capi.Layout.padded(out_elems or cout, h, w, pout)
    d.cin, d.cout, d.k, d.relu = cin, cout, k, relu
    return d


def pw(capi, cin, cout, coutp, cs_in=None, cs_out=None, pin=0, relu=1):
    d = capi.PwDesc()
    d.inp = d.w_packed = d.bias_packed = d.out = FAKE
    d.lin = capi.Layout.padded(cs_in or cin, H, W, pin)
    d.lout = capi.Layout.padded(cs_out or coutp, H, W, 0)
    d.cin, d.cout, d.coutp, d.relu = cin, cout, coutp, relu
    return d


# ---- the valid bases ------------------------------------------------------------------------------------------------------
def base_direct(capi):                    # rtpose_conv2d / rtpose_conv2d_bf16: 3x3, 32 -> 64
    return Case([conv(capi, 3, 32, 64)])


def base_x3(capi):                        # rtpose_conv2d_bf16x3, fp32 output: input slice of 2 elements per channel
    return Case([conv(capi, 3, 32, 64, in_elems=64)], out_f32=1)


def base_wino2(capi):                     # F(2x2,3x3): two 16-channel chunks
    return Case([conv(capi, 3, 32, 128)], wino_m=2)


def base_wino4(capi):                     # F(4x4,3x3)
    return Case([conv(capi, 3, 32, 64)], wino_m=4)


def base_wino7(capi):                     # F(6,7) at 46 x 46
    return Case([conv(capi, 7, 128, 128, h=46, w=46)], h=46, w=46, wino_m=6)


def base_pair(capi):                      # 128 -> 128 (+ReLU) -> 38
    return Case([conv(capi, 1, 128, 128)], [conv(capi, 1, 128, 38, out_elems=64, relu=0)])


def base_c64(capi):                       # conv1_2 of the bf16 plan
    return Case([conv(capi, 3, 64, 64, pout=1)])


def base_pw(capi):                        # one pointwise GEMM, 32 -> 64
    return Case([pw(capi, 32, 64, 64)])


def base_head(capi):                      # 32 -> 256 (+ReLU) -> 38 head columns
    return Case([pw(capi, 32, 256, 256)], [pw(capi, 256, 38, 64, relu=0)])


def base_unit(capi):                      # bf16 ShuffleNetV2 unit: 1x1 (+ReLU) -> 3x3 depthwise -> 1x1 (+ReLU)
    d0, d2 = pw(capi, 32, 32, 128, pin=1), pw(capi, 32, 64, 128, cs_out=64)
    d0.dw_w = d0.dw_b = FAKE
    d2.out_cmap = FAKE
    return Case([d0], [d2])


# ---- the entry points -----------------------------------------------------------------------------------------------------
def _arr(capi, ds):
    return (capi.ConvDesc * 2)(*ds)         # room for two groups: no launcher reads past d[1]


CALLS = {
    "conv2d": lambda lib, c, capi: lib.rtpose_conv2d(_arr(capi, c.a), c.ngroups, c.n, c.h, c.w, None),
    "conv2d_bf16": lambda lib, c, capi: lib.rtpose_conv2d_bf16(_arr(capi, c.a), c.ngroups, c.n, c.h, c.w, c.out_f32, None),
    "conv2d_bf16x3": lambda lib, c, capi: lib.rtpose_conv2d_bf16x3(_arr(capi, c.a), c.ngroups, c.n, c.h, c.w, c.out_f32,
                                                                    None),
    "winograd_ex": lambda lib, c, capi: lib.rtpose_conv2d_winograd_ex(_arr(capi, c.a), c.ngroups, c.n, c.h, c.w, None, 0,
                                                                      None),
    "pair": lambda lib, c, capi: lib.rtpose_conv1x1_pair(_arr(capi, c.a), _arr(capi, c.b), c.ngroups, c.n, c.h, c.w, None),
    "pair_fits": lambda lib, c, capi: lib.rtpose_conv1x1_pair_fits(_arr(capi, c.a), _arr(capi, c.b), c.ngroups),
    "pair_bf16": lambda lib, c, capi: lib.rtpose_conv1x1_pair_bf16(_arr(capi, c.a), _arr(capi, c.b), c.ngroups, c.n, c.h,
                                                                    c.w, c.out_f32, None),
    "pair_bf16_fits": lambda lib, c, capi: lib.rtpose_conv1x1_pair_bf16_fits(_arr(capi, c.a), _arr(capi, c.b), c.ngroups),
    "c64": lambda lib, c, capi: lib.rtpose_conv3x3_c64_bf16(_arr(capi, c.a), c.n, c.h, c.w, None),
    "c64_fits": lambda lib, c, capi: lib.rtpose_conv3x3_c64_bf16_fits(_arr(capi, c.a), c.ngroups, c.n, c.h, c.w),
    "pw_fused": lambda lib, c, capi: lib.rtpose_pw_fused(C.byref(c.a[0]), c.n, c.h, c.w, None),
    "pw_fused_bf16": lambda lib, c, capi: lib.rtpose_pw_fused_bf16(C.byref(c.a[0]), c.out_f32, c.n, c.h, c.w, None),
    "pw_head": lambda lib, c, capi: lib.rtpose_pw_head(C.byref(c.a[0]), C.byref(c.b[0]), c.n, c.h, c.w, None),
    "pw_head_fits": lambda lib, c, capi: lib.rtpose_pw_head_fits(C.byref(c.a[0]), C.byref(c.b[0])),
    "pw_head_bf16": lambda lib, c, capi: lib.rtpose_pw_head_bf16(C.byref(c.a[0]), C.byref(c.b[0]), c.n, c.h, c.w, None),
    "pw_head_bf16_fits": lambda lib, c, capi: lib.rtpose_pw_head_bf16_fits(C.byref(c.a[0]), C.byref(c.b[0])),
    "unit_bf16": lambda lib, c, capi: lib.rtpose_unit_bf16(C.byref(c.a[0]), C.byref(c.b[0]), c.n, c.h, c.w, None),
    "unit_bf16_fits": lambda lib, c, capi: lib.rtpose_unit_bf16_fits(C.byref(c.a[0]), C.byref(c.b[0]), c.h, c.w),
}


# ---- faults -----------------------------------------------------------------------------------------------------------------
def set_(which, i, **kw):
    """fault: fields of descriptor `which`[i] (a Layout value may be given as the tuple of Layout.padded's arguments)"""
    def f(c, capi):
        d = getattr(c, which)[i]
        for k, v in kw.items():
            setattr(d, k, capi.Layout.padded(*v) if isinstance(v, tuple) else v)
    return f


def case_(**kw):
    def f(c, capi):
        for k, v in kw.items():
            setattr(c, k, v)
    return f


def second_group(**kw):
    """fault: a second group, a copy of the first with fields changed"""
    def f(c, capi):
        g = type(c.a[0]).from_buffer_copy(c.a[0])
        for k, v in kw.items():
            setattr(g, k, v)
        c.a.append(g)
        c.ngroups = 2
    return f


def prelu_with_relu(c, capi):
    for d in c.a:
        d.prelu = FAKE                   # slopes, and (the fault for the launchers that have the epilogue) relu = 1


def prelu_only(c, capi):
    for d in c.a:
        d.prelu, d.relu = FAKE, 0


def odd_pool(c, capi):
    c.h = c.w = 7
    for d in c.a:
        d.pool = 1
        d.lin = capi.Layout.padded(d.lin.cstride, 7, 7, d.k // 2)
        d.lout = capi.Layout.padded(d.lout.cstride, 4, 4, 0)


# (id, base, entry, fault, phrase).  NEW: refusals the parent library did not make (the output slice extent of the conv
# launchers; the input extent, out_cmap and output extent of the bf16 1x1 pair).
ROWS = [
    # rtpose_conv2d (fp32 direct)
    ("conv2d-ngroups", base_direct, "conv2d", case_(ngroups=3), "ngroups"),
    ("conv2d-empty", base_direct, "conv2d", case_(n=0), "empty tensor"),
    ("conv2d-k", base_direct, "conv2d", set_("a", 0, k=5), "k must be"),
    ("conv2d-cin", base_direct, "conv2d", set_("a", 0, cin=12), "multiple of 8"),
    ("conv2d-geometry", base_direct, "conv2d", second_group(relu=0), "share geometry"),
    ("conv2d-gap", base_direct, "conv2d", set_("a", 0, lin=(32, H, W, 0)), "layout gap"),
    ("conv2d-align", base_direct, "conv2d", set_("a", 0, lin=(40, H, W, 1, 2)), "16-byte aligned"),
    ("conv2d-in-extent", base_direct, "conv2d", set_("a", 0, lin=(32, H, W, 1, 4)), "exceeds cstride"),
    ("conv2d-out-extent-NEW", base_direct, "conv2d", set_("a", 0, lout=(64, H, W, 0, 8)), "exceeds cstride"),
    ("conv2d-pool", base_direct, "conv2d", odd_pool, "even H and W"),
    ("conv2d-planes", base_direct, "conv2d", set_("a", 0, in_plane_pixels=4096), "channel-plane"),
    ("conv2d-prelu-relu", base_direct, "conv2d", prelu_with_relu, "PReLU"),
    ("conv2d-prelu-k7", base_direct, "conv2d", lambda c, capi: (prelu_only(c, capi), set_("a", 0, k=7, lin=(32, H, W, 3))(c, capi)),
     "PReLU"),
    # rtpose_conv2d_bf16
    ("bf16-ngroups", base_direct, "conv2d_bf16", case_(ngroups=0), "ngroups"),
    ("bf16-empty", base_direct, "conv2d_bf16", case_(w=0), "empty tensor"),
    ("bf16-k", base_direct, "conv2d_bf16", set_("a", 0, k=5), "k must be"),
    ("bf16-cin", base_direct, "conv2d_bf16", set_("a", 0, cin=24), "multiple of 16"),
    ("bf16-geometry", base_direct, "conv2d_bf16", second_group(cout=200), "share geometry"),
    ("bf16-gap", base_direct, "conv2d_bf16", set_("a", 0, lin=(32, H, W, 0)), "layout gap"),
    ("bf16-align", base_direct, "conv2d_bf16", set_("a", 0, lin=(40, H, W, 1, 4)), "16-byte aligned"),
    ("bf16-in-extent", base_direct, "conv2d_bf16", set_("a", 0, lin=(32, H, W, 1, 8)), "exceeds cstride"),
    ("bf16-out-extent-NEW", base_direct, "conv2d_bf16", set_("a", 0, lout=(64, H, W, 0, 8)), "exceeds cstride"),
    ("bf16-pool", base_direct, "conv2d_bf16", odd_pool, "even H and W"),
    ("bf16-planes", base_direct, "conv2d_bf16", set_("a", 0, out_plane_pixels=4096), "channel-plane"),
    ("bf16-prelu", base_direct, "conv2d_bf16", prelu_only, "PReLU"),
    # rtpose_conv2d_bf16x3 (fp32 output)
    ("x3-align", base_x3, "conv2d_bf16x3", set_("a", 0, lin=(80, H, W, 1, 8)), "16-byte aligned"),
    ("x3-in-extent", base_x3, "conv2d_bf16x3", set_("a", 0, lin=(48, H, W, 1)), "exceeds cstride"),
    ("x3-out-extent-NEW", base_x3, "conv2d_bf16x3", set_("a", 0, lout=(64, H, W, 0, 4)), "exceeds cstride"),
    ("x3-out-cmap", base_x3, "conv2d_bf16x3", set_("a", 0, out_cmap=FAKE), "out_cmap"),
    ("x3-prelu", base_x3, "conv2d_bf16x3", prelu_only, "PReLU"),
    # rtpose_conv2d_winograd_ex, F(2x2,3x3)
    ("wino2-wino-m", base_wino2, "winograd_ex", set_("a", 0, wino_m=3), "wino_m"),
    ("wino2-ngroups", base_wino2, "winograd_ex", case_(ngroups=0), "ngroups"),
    ("wino2-empty", base_wino2, "winograd_ex", case_(h=0), "empty tensor"),
    ("wino2-k", base_wino2, "winograd_ex", set_("a", 0, cin=24), "k must be"),
    ("wino2-geometry", base_wino2, "winograd_ex", second_group(cin=48), "share geometry"),
    ("wino2-gap", base_wino2, "winograd_ex", set_("a", 0, lin=(32, H, W, 0)), "layout gap"),
    ("wino2-align", base_wino2, "winograd_ex", set_("a", 0, lin=(40, H, W, 1, 2)), "16-byte aligned"),
    ("wino2-in-extent", base_wino2, "winograd_ex", set_("a", 0, lin=(32, H, W, 1, 4)), "exceeds cstride"),
    ("wino2-out-extent-NEW", base_wino2, "winograd_ex", set_("a", 0, lout=(128, H, W, 0, 4)), "exceeds cstride"),
    ("wino2-out-cmap", base_wino2, "winograd_ex", set_("a", 0, out_cmap=FAKE), "out_cmap"),
    ("wino2-pool", base_wino2, "winograd_ex", odd_pool, "even H and W"),
    ("wino2-planes", base_wino2, "winograd_ex", set_("a", 0, in_plane_pixels=4096), "channel-plane"),
    ("wino2-prelu-relu", base_wino2, "winograd_ex", prelu_with_relu, "PReLU"),
    # rtpose_conv2d_winograd_ex, F(4x4,3x3)
    ("wino4-ngroups", base_wino4, "winograd_ex", case_(ngroups=0), "ngroups"),
    ("wino4-empty", base_wino4, "winograd_ex", case_(n=0), "empty tensor"),
    ("wino4-k", base_wino4, "winograd_ex", set_("a", 0, cin=16), "k must be"),
    ("wino4-geometry", base_wino4, "winograd_ex", second_group(pool=1), "share geometry"),
    ("wino4-gap", base_wino4, "winograd_ex", set_("a", 0, lin=(32, H, W, 0)), "layout gap"),
    ("wino4-align", base_wino4, "winograd_ex", set_("a", 0, lin=(40, H, W, 1, 2)), "16-byte aligned"),
    ("wino4-in-extent", base_wino4, "winograd_ex", set_("a", 0, lin=(32, H, W, 1, 4)), "exceeds cstride"),
    ("wino4-out-extent-NEW", base_wino4, "winograd_ex", set_("a", 0, lout=(64, H, W, 0, 8)), "exceeds cstride"),
    ("wino4-out-cmap", base_wino4, "winograd_ex", set_("a", 0, out_cmap=FAKE), "out_cmap"),
    ("wino4-pool", base_wino4, "winograd_ex", odd_pool, "even H and W"),
    ("wino4-plane-slots", base_wino4, "winograd_ex", set_("a", 0, in_plane_pixels=10), "channel-plane"),
    ("wino4-plane-cout", base_wino4, "winograd_ex", set_("a", 0, cout=60, out_plane_pixels=4096), "channel-plane"),
    ("wino4-prelu-pool", base_wino4, "winograd_ex",
     lambda c, capi: (prelu_only(c, capi), set_("a", 0, pool=1, lout=(64, 4, 4, 0))(c, capi)), "PReLU"),
    # rtpose_conv2d_winograd_ex, F(6,7)
    ("wino7-wino-m", base_wino7, "winograd_ex", set_("a", 0, wino_m=5), "wino_m"),
    ("wino7-ngroups", base_wino7, "winograd_ex", case_(ngroups=0), "ngroups"),
    ("wino7-geometry", base_wino7, "winograd_ex", second_group(relu=0), "share geometry"),
    ("wino7-gap", base_wino7, "winograd_ex", set_("a", 0, lin=(128, 46, 46, 2)), "layout gap"),
    ("wino7-align", base_wino7, "winograd_ex", set_("a", 0, lin=(136, 46, 46, 3, 2)), "16-byte aligned"),
    ("wino7-in-extent", base_wino7, "winograd_ex", set_("a", 0, lin=(132, 46, 46, 3, 8)), "exceeds cstride"),
    ("wino7-out-extent-NEW", base_wino7, "winograd_ex", set_("a", 0, lout=(128, 46, 46, 0, 4)), "exceeds cstride"),
    ("wino7-out-cmap", base_wino7, "winograd_ex", set_("a", 0, out_cmap=FAKE), "out_cmap"),
    ("wino7-planes", base_wino7, "winograd_ex", set_("a", 0, out_plane_pixels=4096), "channel-plane"),
    ("wino7-prelu", base_wino7, "winograd_ex", prelu_only, "PReLU"),
    # rtpose_conv1x1_pair (fp32) and its _fits
    ("pair-planes", base_pair, "pair", set_("a", 0, in_plane_pixels=4096), "channel-plane"),
    ("pair-prelu", base_pair, "pair", lambda c, capi: setattr(c.a[0], "prelu", FAKE), "PReLU"),
    ("pair-align", base_pair, "pair", set_("a", 0, lin=(132, H, W, 0, 2)), "pointwise convs"),
    ("pair-in-extent", base_pair, "pair", set_("a", 0, lin=(132, H, W, 0, 8)), "pointwise convs"),
    ("pair-out-extent", base_pair, "pair", set_("b", 0, lout=(64, H, W, 0, 32)), "pointwise convs"),
    ("pair-out-cmap", base_pair, "pair", set_("b", 0, out_cmap=FAKE), "pointwise convs"),
    ("pair-fits-prelu", base_pair, "pair_fits", lambda c, capi: setattr(c.b[0], "prelu", FAKE), None),
    ("pair-fits-relu2", base_pair, "pair_fits", set_("b", 0, relu=1), None),
    ("pair-fits-align", base_pair, "pair_fits", set_("a", 0, lin=(132, H, W, 0, 2)), None),
    ("pair-fits-in-extent", base_pair, "pair_fits", set_("a", 0, lin=(132, H, W, 0, 8)), None),
    ("pair-fits-out-extent", base_pair, "pair_fits", set_("b", 0, lout=(64, H, W, 0, 32)), None),
    ("pair-fits-out-cmap", base_pair, "pair_fits", set_("a", 0, out_cmap=FAKE), None),
    # rtpose_conv1x1_pair_bf16 and its _fits
    ("pair-bf16-empty", base_pair, "pair_bf16", case_(n=0), "empty tensor"),
    ("pair-bf16-prelu", base_pair, "pair_bf16", lambda c, capi: setattr(c.b[0], "prelu", FAKE), "PReLU"),
    ("pair-bf16-align", base_pair, "pair_bf16", set_("a", 0, lin=(136, H, W, 0, 4)), "16-byte aligned"),
    ("pair-bf16-in-extent-NEW", base_pair, "pair_bf16", set_("a", 0, lin=(128, H, W, 0, 8)), "exceeds cstride"),
    ("pair-bf16-out-extent", base_pair, "pair_bf16", set_("b", 0, lout=(64, H, W, 0, 32)), "exceeds cstride"),
    ("pair-bf16-out-cmap-NEW", base_pair, "pair_bf16", set_("b", 0, out_cmap=FAKE), "out_cmap"),
    ("pair-bf16-fits-prelu", base_pair, "pair_bf16_fits", lambda c, capi: setattr(c.a[0], "prelu", FAKE), None),
    ("pair-bf16-fits-align", base_pair, "pair_bf16_fits", set_("a", 0, lin=(136, H, W, 0, 4)), None),
    ("pair-bf16-fits-in-extent-NEW", base_pair, "pair_bf16_fits", set_("a", 0, lin=(128, H, W, 0, 8)), None),
    ("pair-bf16-fits-out-extent-NEW", base_pair, "pair_bf16_fits", set_("b", 0, lout=(64, H, W, 0, 32)), None),
    ("pair-bf16-fits-out-cmap-NEW", base_pair, "pair_bf16_fits", set_("a", 0, out_cmap=FAKE), None),
    # rtpose_conv3x3_c64_bf16 and its _fits
    ("c64-prelu", base_c64, "c64", prelu_only, "PReLU"),
    ("c64-align", base_c64, "c64", set_("a", 0, lin=(72, H, W, 1, 4)), "16-byte aligned"),
    ("c64-out-extent", base_c64, "c64", set_("a", 0, lout=(64, H, W, 1, 8)), "64 bf16 input channels"),
    ("c64-out-cmap", base_c64, "c64", set_("a", 0, out_cmap=FAKE), "64 bf16 input channels"),
    ("c64-fits-ngroups", base_c64, "c64_fits", case_(ngroups=2), None),
    ("c64-fits-align", base_c64, "c64_fits", set_("a", 0, lout=(72, H, W, 1, 4)), None),
    ("c64-fits-in-extent", base_c64, "c64_fits", set_("a", 0, lin=(64, H, W, 1, 8)), None),
    ("c64-fits-out-extent", base_c64, "c64_fits", set_("a", 0, lout=(64, H, W, 1, 8)), None),
    ("c64-fits-gap", base_c64, "c64_fits", set_("a", 0, lin=(64, H, W, 0)), None),
    ("c64-fits-pool", base_c64, "c64_fits", odd_pool, None),
    ("c64-fits-planes", base_c64, "c64_fits", set_("a", 0, in_plane_pixels=4096), None),
    # the pointwise launchers
    ("pw-empty", base_pw, "pw_fused", case_(n=0), "empty tensor"),
    ("pw-align", base_pw, "pw_fused", set_("a", 0, lin=(40, H, W, 0, 2)), "16-byte aligned"),
    ("pw-in-extent", base_pw, "pw_fused", set_("a", 0, lin=(32, H, W, 0, 4)), "inside the pixel"),
    ("pw-dw-gap", base_pw, "pw_fused", lambda c, capi: (setattr(c.a[0], "dw_w", FAKE), setattr(c.a[0], "dw_b", FAKE)),
     "layout gap"),
    ("pw-bf16-align", base_pw, "pw_fused_bf16", set_("a", 0, lin=(40, H, W, 0, 4)), "16-byte aligned"),
    ("pw-bf16-in-extent", base_pw, "pw_fused_bf16", set_("a", 0, lin=(32, H, W, 0, 8)), "inside the pixel"),
    ("pw-bf16-out-extent", base_pw, "pw_fused_bf16", set_("a", 0, lout=(64, H, W, 0, 8)), "inside the pixel"),
    ("pw-bf16-dw-gap", base_pw, "pw_fused_bf16", lambda c, capi: (setattr(c.a[0], "dw_w", FAKE), setattr(c.a[0], "dw_b", FAKE)),
     "layout gap"),
    ("head-in-extent", base_head, "pw_head", set_("a", 0, lin=(32, H, W, 0, 4)), "slices"),
    ("head-fits-align", base_head, "pw_head_fits", set_("a", 0, lin=(40, H, W, 0, 2)), None),
    ("head-fits-in-extent", base_head, "pw_head_fits", set_("a", 0, lin=(32, H, W, 0, 4)), None),
    ("head-fits-out-extent", base_head, "pw_head_fits", set_("b", 0, lout=(64, H, W, 0, 4)), None),
    ("head-fits-out-align", base_head, "pw_head_fits", set_("b", 0, lout=(70, H, W, 0, 2)), None),
    ("head-bf16-in-extent", base_head, "pw_head_bf16", set_("a", 0, lin=(32, H, W, 0, 8)), "64 head columns"),
    ("head-bf16-fits-align", base_head, "pw_head_bf16_fits", set_("a", 0, lin=(40, H, W, 0, 4)), None),
    ("head-bf16-fits-in-extent", base_head, "pw_head_bf16_fits", set_("a", 0, lin=(32, H, W, 0, 8)), None),
    ("head-bf16-fits-out-extent", base_head, "pw_head_bf16_fits", set_("b", 0, lout=(64, H, W, 0, 4)), None),
    ("unit-gap", base_unit, "unit_bf16", set_("a", 0, lin=(32, H, W, 0)), "unit_bf16_fits"),
    ("unit-fits-align", base_unit, "unit_bf16_fits", set_("a", 0, lin=(40, H, W, 1, 4)), None),
    ("unit-fits-gap", base_unit, "unit_bf16_fits", set_("a", 0, lin=(32, H, W, 0)), None),
    ("unit-fits-out-cstride", base_unit, "unit_bf16_fits", set_("b", 0, lout=(60, H, W, 0)), None),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_one_fault_is_refused_on_the_host(capi, row):
    _, base, entry, fault, phrase = row
    c = base(capi)
    fault(c, capi)
    rc = CALLS[entry](capi.lib, c, capi)
    if phrase is None:                       # a _fits function
        assert rc == 0, (entry, rc)
    else:
        err = capi.last_error()
        assert rc == -1, (entry, rc, err)    # RTPOSE_E_INVAL, not a HIP error of a launch that got through
        assert phrase in err, (entry, err)
