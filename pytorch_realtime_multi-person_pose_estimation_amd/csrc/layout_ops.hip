// HBM-bound data-movement kernels around the conv path: NCHW <-> shared-gap padded NHWC, fp32 <-> bf16 and fp32 <-> split
// conversions at the edges of the net, slice copies and the 2x2 max-pool (nn.MaxPool2d(2,2,0),
// lib/network/rtpose_vgg.py:49-50).  All are one coalesced pass, 16 bytes per thread on the NHWC side where the slice
// is 16-byte aligned.  The ShuffleNetV2 building blocks are in shufflenet_ops.hip, the image work in image_ops.hip.
#include <hip/hip_runtime.h>

#include "pixel_walk.h"

namespace rtpose {

// One thread per (pixel, channel) with channel fastest on the NHWC side; the
// NCHW side is strided by H*W, served from L2 (tensors here are small or read
// once).  Used for the 3-channel input image and the 38/19-channel outputs.
__global__ void nchw_to_layout_kernel(const float* __restrict__ src, float* __restrict__ dst, Lay l,
                                      int C, int cpad, int N, int H, int W) {
  Walk q;
  if (!pixel_walk(cpad, N, H, W, q)) return;
  const float v = (q.c < C) ? src[(((size_t)q.n * C + q.c) * H + q.y) * W + q.x] : 0.f;
  dst[lay_off(l, q) + q.c] = v;
}

// x fastest on the NCHW side (coalesced writes); the NHWC reads of one wave hit
// 64 different pixels of the same channel: 64 sectors, but C (<=57) consecutive
// launches-worth of threads re-use them from L2.
__global__ void layout_to_nchw_kernel(const float* __restrict__ src, Lay l, float* __restrict__ dst,
                                      int C, int N, int H, int W) {
  Walk q;
  if (!nchw_walk(C, N, H, W, q)) return;
  dst[q.i] = src[lay_off(l, q) + q.c];
}

__global__ void layout_copy_kernel(const float* __restrict__ src, Lay ls, float* __restrict__ dst,
                                   Lay ld, int C, int N, int H, int W) {
  Walk q;
  if (!pixel_walk<4>(C >> 2, N, H, W, q)) return;
  *reinterpret_cast<ChanBits<float>*>(dst + lay_off(ld, q) + q.c) =
      *reinterpret_cast<const ChanBits<float>*>(src + lay_off(ls, q) + q.c);
}

__global__ void layout_copy_scalar_kernel(const float* __restrict__ src, Lay ls,
                                          float* __restrict__ dst, Lay ld, int C, int N, int H,
                                          int W) {
  Walk q;
  if (!pixel_walk(C, N, H, W, q)) return;
  dst[lay_off(ld, q) + q.c] = src[lay_off(ls, q) + q.c];
}

__global__ void maxpool2x2_kernel(const float* __restrict__ src, Lay ls, float* __restrict__ dst,
                                  Lay ld, int C, int N, int Ho, int Wo) {
  typedef ChanVec<float> V;
  Walk q;
  if (!pixel_walk<4>(C >> 2, N, Ho, Wo, q)) return;
  const V a = V::load(src + lay_off(ls, q.n, 2 * q.y, 2 * q.x) + q.c);
  const V b = V::load(src + lay_off(ls, q.n, 2 * q.y, 2 * q.x + 1) + q.c);
  const V d = V::load(src + lay_off(ls, q.n, 2 * q.y + 1, 2 * q.x) + q.c);
  const V e = V::load(src + lay_off(ls, q.n, 2 * q.y + 1, 2 * q.x + 1) + q.c);
  V r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.v[k] = fmaxf(fmaxf(a.v[k], b.v[k]), fmaxf(d.v[k], e.v[k]));
  r.store(dst + lay_off(ld, q) + q.c);
}

// ---- bf16 activation buffers (conv_mfma_bf16.hip) and the "split" activations of the bf16x3 plans: conversions at the
//      edges of the net.  Split: value v = hi + lo, hi = bf16(v), lo = bf16(v - hi), stored per 8 channels as
//      [hi x 8 | lo x 8] (32 bytes); split layouts count elements (2 per channel) ----

// One thread per (pixel, 8-channel piece): 16-byte stores.  src is dense NCHW fp32 (SRC_NCHW: x fastest, coalesced
// reads of each channel plane) or a layout slice; channels [C, cpad) are written as zero.  One gather, two packers:
// SPLIT stores the rounding's remainder behind the rounded values.
template <bool SRC_NCHW, bool SPLIT>
__global__ void f32_to_bf16_layout_kernel(const float* __restrict__ src, Lay ls, unsigned short* __restrict__ dst,
                                          Lay ld, int C, int cpad, int N, int H, int W) {
  Walk q;
  if (!pixel_walk<8, SRC_NCHW>(cpad >> 3, N, H, W, q)) return;
  unsigned short hi[8], lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = q.c + e;
    float f = 0.f;
    if (c < C) f = SRC_NCHW ? src[(((size_t)q.n * C + c) * H + q.y) * W + q.x] : src[lay_off(ls, q) + c];
    hi[e] = f32_to_bf16_rne(f);
    if (SPLIT) lo[e] = f32_to_bf16_rne(f - bf16_to_f32(hi[e]));
  }
  uint4* d = reinterpret_cast<uint4*>(dst + lay_off(ld, q) + (SPLIT ? 2 : 1) * q.c);
  d[0] = make_uint4(bf16_pair(hi[0], hi[1]), bf16_pair(hi[2], hi[3]), bf16_pair(hi[4], hi[5]), bf16_pair(hi[6], hi[7]));
  if (SPLIT)
    d[1] = make_uint4(bf16_pair(lo[0], lo[1]), bf16_pair(lo[2], lo[3]), bf16_pair(lo[4], lo[5]), bf16_pair(lo[6], lo[7]));
}

__global__ void layout_bf16_to_f32_kernel(const unsigned short* __restrict__ src, Lay ls,
                                          float* __restrict__ dst, Lay ld, int C, int N, int H, int W) {
  Walk q;
  if (!pixel_walk(C, N, H, W, q)) return;
  dst[lay_off(ld, q) + q.c] = bf16_to_f32(src[lay_off(ls, q) + q.c]);
}

__global__ void layout_split_to_f32_kernel(const unsigned short* __restrict__ src, Lay ls,
                                           float* __restrict__ dst, Lay ld, int C, int N, int H, int W) {
  Walk q;
  if (!pixel_walk(C, N, H, W, q)) return;
  // ls.choff counts elements and may sit inside an 8-channel group (the 19 heat-map channels
  // start at channel 166 of the concat buffer): address by absolute channel
  const int ca = (ls.choff >> 1) + q.c;
  const unsigned short* s = src + ((size_t)ls.lead + (size_t)(q.n * ls.hs + q.y) * ls.ws + q.x) * ls.cstride +
                            (ca >> 3) * 16 + (ca & 7);
  dst[lay_off(ld, q) + q.c] = bf16_to_f32(s[0]) + bf16_to_f32(s[8]);
}

// The four fp32 -> bf16 / split doors: the destination slice aligned to 8 elements (bf16: 16 bytes) or 16 (split: 32).
template <bool SRC_NCHW, bool SPLIT>
static int f32_to_bf16_layout(const char* who, const float* src, const rtpose_layout* lsrc, void* dst, const rtpose_layout* ldst,
                       int C, int cpad, int N, int H, int W, void* stream) {
  if ((cpad % 8) || !slice_aligned(ldst, SPLIT ? 16 : 8) || cpad < C)
    return fail(RTPOSE_E_INVAL, "%s: slice must be %d-byte aligned, cpad >= C", who, SPLIT ? 32 : 16);
  return launch_flat(f32_to_bf16_layout_kernel<SRC_NCHW, SPLIT>, (size_t)N * H * W * (cpad / 8), stream, src,
                     SRC_NCHW ? Lay{} : to_lay(lsrc), static_cast<unsigned short*>(dst), to_lay(ldst), C, cpad, N, H, W);
}

}  // namespace rtpose

using namespace rtpose;

extern "C" {

size_t rtpose_layout_pixels(const rtpose_layout* l, int N, int H, int W) {
  (void)H;
  (void)W;
  // tail slack: 2-D tiles may read up to ~36 rows past the last image, and the strip
  // mode's staging runs up to 14 piece sets (64 pixels each) past a halo
  return (size_t)l->lead + (size_t)N * l->hs * l->ws + (size_t)40 * l->ws + 4352;
}

int rtpose_nchw_to_layout(const float* src, float* dst, const rtpose_layout* ldst, int C, int cpad,
                          int N, int H, int W, void* stream) {
  if (cpad < C || ldst->choff + cpad > ldst->cstride)
    return fail(RTPOSE_E_INVAL, "nchw_to_layout: bad channel counts");
  return launch_flat(nchw_to_layout_kernel, (size_t)N * H * W * cpad, stream, src, dst, to_lay(ldst), C, cpad, N, H, W);
}

int rtpose_layout_to_nchw(const float* src, const rtpose_layout* lsrc, float* dst, int C, int N, int H,
                          int W, void* stream) {
  return launch_flat(layout_to_nchw_kernel, (size_t)N * H * W * C, stream, src, to_lay(lsrc), dst, C, N, H, W);
}

int rtpose_layout_copy(const float* src, const rtpose_layout* lsrc, float* dst,
                       const rtpose_layout* ldst, int C, int N, int H, int W, void* stream) {
  const bool vec = !(C % 4) && slice_aligned(lsrc, 4) && slice_aligned(ldst, 4);
  return launch_flat(vec ? layout_copy_kernel : layout_copy_scalar_kernel, (size_t)N * H * W * (vec ? C / 4 : C), stream,
                     src, to_lay(lsrc), dst, to_lay(ldst), C, N, H, W);
}

int rtpose_maxpool2x2(const float* in, const rtpose_layout* lin, float* out, const rtpose_layout* lout,
                      int C, int N, int H, int W, void* stream) {
  if ((C % 4) || !slice_aligned(lin, 4) || !slice_aligned(lout, 4))
    return fail(RTPOSE_E_INVAL, "maxpool: channel slices must be 16-byte aligned");
  const int Ho = H / 2, Wo = W / 2;
  return launch_flat(maxpool2x2_kernel, (size_t)N * Ho * Wo * (C / 4), stream, in, to_lay(lin), out, to_lay(lout), C, N,
                     Ho, Wo);
}

int rtpose_nchw_to_layout_bf16(const float* src_nchw, void* dst, const rtpose_layout* ldst, int C, int cpad,
                               int N, int H, int W, void* stream) {
  return f32_to_bf16_layout<true, false>("nchw_to_layout_bf16", src_nchw, nullptr, dst, ldst, C, cpad, N, H, W, stream);
}

int rtpose_layout_f32_to_bf16(const float* src, const rtpose_layout* lsrc, void* dst,
                              const rtpose_layout* ldst, int C, int cpad, int N, int H, int W, void* stream) {
  return f32_to_bf16_layout<false, false>("layout_f32_to_bf16", src, lsrc, dst, ldst, C, cpad, N, H, W, stream);
}

int rtpose_layout_bf16_to_f32(const void* src, const rtpose_layout* lsrc, float* dst, const rtpose_layout* ldst,
                              int C, int N, int H, int W, void* stream) {
  return launch_flat(layout_bf16_to_f32_kernel, (size_t)N * H * W * C, stream, static_cast<const unsigned short*>(src),
                     to_lay(lsrc), dst, to_lay(ldst), C, N, H, W);
}

int rtpose_nchw_to_layout_split(const float* src_nchw, void* dst, const rtpose_layout* ldst, int C, int cpad,
                                int N, int H, int W, void* stream) {
  return f32_to_bf16_layout<true, true>("nchw_to_layout_split", src_nchw, nullptr, dst, ldst, C, cpad, N, H, W, stream);
}

int rtpose_layout_f32_to_split(const float* src, const rtpose_layout* lsrc, void* dst,
                               const rtpose_layout* ldst, int C, int cpad, int N, int H, int W, void* stream) {
  return f32_to_bf16_layout<false, true>("layout_f32_to_split", src, lsrc, dst, ldst, C, cpad, N, H, W, stream);
}

int rtpose_layout_split_to_f32(const void* src, const rtpose_layout* lsrc, float* dst, const rtpose_layout* ldst,
                               int C, int N, int H, int W, void* stream) {
  if (lsrc->choff & 1) return fail(RTPOSE_E_INVAL, "layout_split_to_f32: choff counts elements (2 per channel)");
  return launch_flat(layout_split_to_f32_kernel, (size_t)N * H * W * C, stream, static_cast<const unsigned short*>(src),
                     to_lay(lsrc), dst, to_lay(ldst), C, N, H, W);
}

}  // extern "C"
