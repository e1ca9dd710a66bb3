// Host-side helpers shared by the conv launchers: what a valid rtpose_conv_desc slice is, the fill of a kernel's group
// struct from a descriptor (and of the fused pointwise kernels' arguments from theirs), the grid-id count of the XCD-aware block order and the launch of one kernel instance.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace rtpose {

// ---- layout predicates --------------------------------------------------------------------------------------------------
// cstride and choff multiples of `align` elements (16-byte pieces: 4 fp32, 8 bf16 elements)
inline bool slice_aligned(const rtpose_layout& l, int align) { return l.cstride % align == 0 && l.choff % align == 0; }
// `elems` elements from choff stay inside the pixel
inline bool slice_inside(const rtpose_layout& l, int elems) { return l.choff + elems <= l.cstride; }
inline bool slice_ok(const rtpose_layout& l, int elems, int align) { return slice_aligned(l, align) && slice_inside(l, elems); }
// the zero gap around an H x W map covers a conv padding of p pixels
inline bool gap_covers(const rtpose_layout& l, int H, int W, int p) {
  return l.ws >= W + p && l.hs >= H + p && l.lead >= p * l.ws + p;
}
// the whole buffer addressable with 32-bit element offsets
inline bool below_2g_elems(const rtpose_layout& l, int N, int H, int W) {
  return rtpose_layout_pixels(&l, N, H, W) * (size_t)l.cstride < ((size_t)1 << 31);
}
inline bool layout_sane(const rtpose_layout& l) { return l.cstride > 0 && l.choff >= 0 && l.ws > 0 && l.hs > 0 && l.lead >= 0; }
// ---- one launcher's view of a group of 1 or 2 descriptors -----------------------------------------------------------------
struct ConvSpec {
  const char* who;  // message prefix
  int align;        // input slice alignment, elements
  int elems;        // elements per input channel (2: bf16x3 hi / lo pieces)
  bool cmap;        // out_cmap taken
  bool planes;      // channel-plane slices taken (the form checks their rules itself)
  bool prelu;       // PReLU epilogue taken
  bool out_extent;  // the output slice counts channels: lout.choff + cout <= lout.cstride (pixel-major, no out_cmap)
  bool residual;    // residual epilogue taken (the form checks its rules itself)
  bool preact;      // input pre-activation taken (likewise)
};

inline bool desc_has_prelu(const rtpose_conv_desc* d, int ngroups) {
  for (int g = 0; d && g < ngroups && g < 2; ++g)
    if (d[g].prelu) return true;
  return false;
}
inline bool desc_has_planes(const rtpose_conv_desc* d, int ngroups) {
  for (int g = 0; d && g < ngroups && g < 2; ++g)
    if (d[g].in_plane_pixels || d[g].out_plane_pixels) return true;
  return false;
}

inline bool desc_has_residual(const rtpose_conv_desc* d, int ngroups) {
  for (int g = 0; d && g < ngroups && g < 2; ++g)
    if (d[g].residual) return true;
  return false;
}
inline bool desc_has_preact(const rtpose_conv_desc* d, int ngroups) {
  for (int g = 0; d && g < ngroups && g < 2; ++g)
    if (d[g].in_scale || d[g].in_shift || d[g].preact_cin) return true;
  return false;
}

// A launcher checks d[0..ngroups) in three steps, all before any HIP call: check_conv_features (group count, channel
// planes, PReLU), then the checks of its own form (k, cin, ...), then check_conv_layouts.  Each returns 0 or fail(...).
inline int check_conv_features(const rtpose_conv_desc* d, int ngroups, const ConvSpec& sp) {
  if (!d || ngroups < 1 || ngroups > 2) return fail(RTPOSE_E_INVAL, "%s: ngroups must be 1 or 2", sp.who);
  if (!sp.planes && desc_has_planes(d, ngroups))
    return fail(RTPOSE_E_INVAL, "%s: channel-plane slices (in_plane_pixels / out_plane_pixels) are read and written by "
                                "F(4x4,3x3) launches only (zero-initialise descriptors)", sp.who);
  if (desc_has_prelu(d, ngroups)) {
    if (!sp.prelu)
      return fail(RTPOSE_E_INVAL, "%s: no PReLU epilogue (rtpose_conv_desc.prelu is taken by the fp32 rtpose_conv2d and "
                                  "the fp32 k = 3 Winograd forms only)", sp.who);
    for (int i = 0; i < ngroups; ++i)
      if (!d[i].prelu || d[i].relu || d[i].pool)
        return fail(RTPOSE_E_INVAL, "%s: a PReLU launch has slopes in every group, relu = 0 and no fused pool", sp.who);
  }
  if (!sp.residual && desc_has_residual(d, ngroups))
    return fail(RTPOSE_E_INVAL, "%s: no residual epilogue (rtpose_conv_desc.residual is taken by the fp32 rtpose_conv2d "
                                "for k = 1 only; zero-initialise descriptors)", sp.who);
  if (!sp.preact && desc_has_preact(d, ngroups))
    return fail(RTPOSE_E_INVAL, "%s: no input pre-activation (rtpose_conv_desc.in_scale / in_shift / preact_cin are taken "
                                "by the fp32 rtpose_conv2d for k = 1 only; zero-initialise descriptors)", sp.who);
  return 0;
}

// the tensor, the groups' shared geometry, the input gap for the padding of d[0].k (a k the form accepted), both slices
// and the fused pool
inline int check_conv_layouts(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, const ConvSpec& sp) {
  if (N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "%s: empty tensor", sp.who);
  const rtpose_conv_desc& d0 = d[0];
  for (int i = 0; i < ngroups; ++i) {
    const rtpose_conv_desc& di = d[i];
    if (di.k != d0.k || di.cin != d0.cin || di.relu != d0.relu || di.pool != d0.pool ||
        cout_pad(di.cout) != cout_pad(d0.cout) || di.lin.ws != d0.lin.ws || di.lin.hs != d0.lin.hs)
      return fail(RTPOSE_E_INVAL, "%s: grouped convs must share geometry", sp.who);
    if (!gap_covers(di.lin, H, W, d0.k / 2))
      return fail(RTPOSE_E_INVAL, "%s: input layout gap smaller than the conv padding", sp.who);
    if (!slice_aligned(di.lin, sp.align)) return fail(RTPOSE_E_INVAL, "%s: input slice must be 16-byte aligned", sp.who);
    if (!slice_inside(di.lin, di.cin * sp.elems)) return fail(RTPOSE_E_INVAL, "%s: input slice exceeds cstride", sp.who);
    if (di.out_cmap && !sp.cmap) return fail(RTPOSE_E_INVAL, "%s: out_cmap is not supported", sp.who);
    if (sp.out_extent && !di.out_cmap && !di.out_plane_pixels && !slice_inside(di.lout, di.cout))
      return fail(RTPOSE_E_INVAL, "%s: output slice exceeds cstride", sp.who);
  }
  if (d0.pool && ((H | W) & 1)) return fail(RTPOSE_E_INVAL, "%s: fused pool needs even H and W", sp.who);
  return 0;
}

// The two 1x1 convs of one launch of conv_tail.hip / conv_tail_bf16.hip, branch g: d1[g] 128 -> 128 | 512 with ReLU, d2[g]
// -> 1..64 channels reading d1[g]'s output, no pool, PReLU or out_cmap; the input slice aligned to `align` elements, both
// slices inside their cstride.  relu2: d2 may have a ReLU (the same in every branch), else it has none.
inline bool conv_pair_fits(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups, int align, bool relu2) {
  if (!d1 || !d2 || ngroups < 1 || ngroups > 2 || desc_has_prelu(d1, ngroups) || desc_has_prelu(d2, ngroups)) return false;
  if (desc_has_residual(d1, ngroups) || desc_has_residual(d2, ngroups) || desc_has_preact(d1, ngroups) ||
      desc_has_preact(d2, ngroups))
    return false;
  for (int g = 0; g < ngroups; ++g) {
    const rtpose_conv_desc &a = d1[g], &b = d2[g];
    if (a.k != 1 || b.k != 1 || a.cin != 128 || (a.cout != 128 && a.cout != 512) || a.cout != d1[0].cout ||
        b.cin != a.cout || b.cout < 1 || b.cout > 64 || !a.relu || (relu2 ? b.relu != d2[0].relu : b.relu != 0) ||
        a.pool || b.pool || a.out_cmap || b.out_cmap || !slice_ok(a.lin, 128, align) || !slice_inside(b.lout, b.cout))
      return false;
  }
  return true;
}

// ---- kernel arguments from descriptors ----------------------------------------------------------------------------------
template <class G, class = void>
struct has_out_cmap : std::false_type {};
template <class G>
struct has_out_cmap<G, std::void_t<decltype(std::declval<G&>().out_cmap)>> : std::true_type {};

// the fields every conv kernel's group struct has (pointers, both layouts, cout, cout_pad; out_cmap where it exists)
template <class G>
inline void fill_group(G& g, const rtpose_conv_desc& d) {
  g.in = reinterpret_cast<decltype(g.in)>(d.in);
  g.w = reinterpret_cast<decltype(g.w)>(d.w_packed);
  g.bias = d.bias_packed;
  g.out = d.out;
  g.lin = to_lay(d.lin);
  g.lout = to_lay(d.lout);
  g.cout = d.cout;
  g.cout_pad = cout_pad(d.cout);
  if constexpr (has_out_cmap<G>::value) g.out_cmap = d.out_cmap;
}

// the PReLU slopes of a grouped launch (a single group reads its own slopes for both)
template <class A>
inline void set_prelu(A& a, const rtpose_conv_desc* d, int ngroups) {
  a.prelu[0] = d[0].prelu;
  a.prelu[1] = ngroups > 1 ? d[1].prelu : d[0].prelu;
}

// What the arguments of the fp32 and the bf16 fused pointwise kernel (pw_fused.hip, pw_fused_bf16.hip) have in common, from
// a descriptor the launcher has checked: pointers, layouts, the interleave pass-through, sizes and the FastDiv constants of
// the work-item decode.  bm: pixels of a block, tile: edge of a depthwise block's pixel tile.  Returns the grid: one block
// per work item, at most the 2 persistent blocks per CU.
template <class A>
inline int fill_pw_args(A& a, const rtpose_pw_desc* d, int N, int H, int W, int bm, int tile) {
  memset(&a, 0, sizeof(a));
  a.in = reinterpret_cast<decltype(a.in)>(d->in);
  a.lin = to_lay(d->lin);
  a.dw_w = d->dw_w;
  a.dw_b = d->dw_b;
  a.w = reinterpret_cast<decltype(a.w)>(d->w_packed);
  a.bias = d->bias_packed;
  a.out = d->out;
  a.lout = to_lay(d->lout);
  a.out_cmap = d->out_cmap;
  if (d->pt_src) {
    a.pt = reinterpret_cast<decltype(a.pt)>(d->pt_src);
    a.lpt = to_lay(d->lpt);
    a.pt_pairs = d->pt_pairs;
    a.pt_a = d->pt_a;
    a.pt_b = d->pt_b;
    a.pt_split = d->pt_split;
    a.pt_d0 = d->pt_d0;
    a.pt_d1 = d->pt_d1;
  }
  a.in_planes = d->in_planes;
  a.N = N;
  a.H = H;
  a.W = W;
  a.M = N * H * W;
  a.K = d->cin;
  a.coutp = d->coutp;
  a.cout = d->cout;
  a.relu = d->relu;
  const int npass = d->coutp <= 128 ? 1 : d->coutp / 256;
  a.fHW = make_fastdiv(H * W);
  a.fW = make_fastdiv(W);
  a.fnp = make_fastdiv(npass);
  a.ftx = make_fastdiv(ceil_div(W, tile));
  a.fty = make_fastdiv(ceil_div(H, tile));
  const int nwork = (d->dw_w ? N * ceil_div(H, tile) * ceil_div(W, tile) : ceil_div(a.M, bm)) * npass;
  return nwork < 2 * device_cu_count() ? nwork : 2 * device_cu_count();
}

// Block ids of a 1-D grid over mtiles x ncombo tiles.  XCD-aware order (xcd_remap = 1, when there are several column tiles /
// groups and at least 64 m tiles): the ncombo blocks of an m tile sit on one XCD, the m tiles padded to a multiple of 8.
inline int grid_ids(int mtiles, int ncombo, int& xcd_remap, long& ids, const char* who) {
  xcd_remap = (ncombo > 1 && mtiles >= 64) ? 1 : 0;
  ids = xcd_remap ? (long)8 * ncombo * ceil_div(mtiles, 8) : (long)mtiles * ncombo;
  if (ids > 0x7fffffffL) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);
  return 0;
}

// ---- launch -------------------------------------------------------------------------------------------------------------
// One launch of kernel instance Kern; its dynamic-LDS ceiling (`max_lds` bytes) is raised once per device.
template <auto Kern, class A>
inline int launch_kernel(dim3 grid, dim3 block, size_t lds, size_t max_lds, hipStream_t s, const A& a) {
  static PerDeviceOnce attr_set;  // zero-initialised; the attribute is per device
  const int dev = current_device();
  if (!attr_set.is_set(dev)) {
    RTPOSE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)max_lds));
    attr_set.set(dev);
  }
  hipLaunchKernelGGL(Kern, grid, block, lds, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- LDS geometry of the direct conv kernels (conv_mfma.hip, conv_mfma_bf16.hip) -----------------------------------------
// LDS plane size: pixel count rounded so that the 4 channel-group planes of one pixel land in different 16-byte bank slots
// on the staging writes.
inline int round_qs(int npix) {
  int qs = npix;
  while ((qs & 3) != 2) ++qs;
  return qs;
}
inline int halo_row_lds(int tw, int p) {
  int w = tw + 2 * p;
  while ((w & 15) != 8) ++w;  // consecutive tile rows half a bank-row apart
  return w;
}

}  // namespace rtpose
