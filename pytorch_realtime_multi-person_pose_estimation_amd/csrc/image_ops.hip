// Image work around the net: the fused uint8 image preparation, the multi-scale TTA resize and the accumulate into a
// layout slice (the flip merge and the fused TTA kernel are in tta.hip).  One coalesced pass each.
#include <hip/hip_runtime.h>

#include "pixel_walk.h"

namespace rtpose {

// Fused caller-side image prep: crop_with_factor + rtpose/vgg_preprocess
// (lib/network/im_transform.py:119-134, lib/datasets/preprocessing.py:16-43) on the device:
// uint8 BGR HWC image -> cv2.resize(fx=fy=scale, INTER_LINEAR) in OpenCV's 11-bit fixed point
// -> zero pad to the network size -> normalise -> the net's NHWC8 input buffer.  Integer
// arithmetic identical to preprocess.resize_linear_u8 (the numpy restatement): bit-exact.
// Columns (resize.cpp's dx loop): taps that fall outside clamp BOTH the offset and the weight
// (f = 0).  Rows (the dy loop) keep their weight and resizeGeneric_Invoker clips the two source
// rows instead - same value in real arithmetic, not always the same 11-bit fixed-point sum.
template <bool ROWS>
__device__ __forceinline__ void lin_coeff(int d, int sn, double scale, int& s0, int& s1, int& a0, int& a1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (ROWS) {
    s0 = min(max(s, 0), sn - 1);
    s1 = min(max(s + 1, 0), sn - 1);
  } else {
    if (s < 0) {
      f = 0.f;
      s = 0;
    }
    if (s >= sn - 1) {
      f = 0.f;
      s = sn - 1;
    }
    s0 = s;
    s1 = min(s + 1, sn - 1);
  }
  a1 = (int)rintf(f * 2048.f);
  a0 = (int)rintf((1.f - f) * 2048.f);
}

// One image of a batch: where it is, how it is resized, which image slot of the network input it fills.
struct PrepImg {
  const unsigned char* img;  // device, BGR uint8 [h0][w0][3]
  double inv_scale;          // 1 / im_scale
  int h0, w0, hr, wr;        // source size; resized (valid) size inside the Hn x Wn padded input
  int flip, n;               // mirror inside the valid width; image index in the destination
};
constexpr int kPrepBatch = 64;  // descriptors per launch, passed by value (kernel argument: no device table)
struct PrepBatch {
  PrepImg im[kPrepBatch];
};

// grid (pixels of the padded Hn x Wn input / 256, images): one launch prepares a whole bucket of images
__global__ void preprocess_u8_kernel(PrepBatch batch, int mode, float* __restrict__ dst, Lay ld, int Hn, int Wn) {
  const PrepImg& d = batch.im[blockIdx.y];
  const unsigned char* __restrict__ img = d.img;
  const int h0 = d.h0, w0 = d.w0, hr = d.hr, wr = d.wr;
  const size_t total = (size_t)Hn * Wn;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = i % Wn, y = i / Wn;
  int px[3] = {0, 0, 0};  // padded area: pixel value 0 (im_transform.py:130-131)
  if (y < hr && x < wr) {
    int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
    // flip: this destination column shows the x-mirrored RESIZED image (valid region only)
    lin_coeff<false>(d.flip ? wr - 1 - x : x, w0, d.inv_scale, x0, x1, ax0, ax1);
    lin_coeff<true>(y, h0, d.inv_scale, y0, y1, ay0, ay1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int s00 = img[((size_t)y0 * w0 + x0) * 3 + c], s01 = img[((size_t)y0 * w0 + x1) * 3 + c];
      const int s10 = img[((size_t)y1 * w0 + x0) * 3 + c], s11 = img[((size_t)y1 * w0 + x1) * 3 + c];
      const int r0 = s00 * ax0 + s01 * ax1, r1 = s10 * ax0 + s11 * ax1;
      int v = ((((ay0 * (r0 >> 4)) >> 16) + ((ay1 * (r1 >> 4)) >> 16) + 2) >> 2);
      px[c] = min(max(v, 0), 255);
    }
  }
  float o[3];
  if (mode == 0) {  // rtpose_preprocess: x / 256 - 0.5, channel order kept (BGR)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (float)px[c] / 256.f - 0.5f;
  } else {          // vgg_preprocess: RGB, /255, ImageNet mean/std
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = ((float)px[2 - c] / 255.f - mean[c]) / sd[c];
  }
  float* q = dst + lay_off(ld, d.n, y, x);
  *reinterpret_cast<float4*>(q) = make_float4(o[0], o[1], o[2], 0.f);
  *reinterpret_cast<float4*>(q + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Multi-scale test-time augmentation: dst = beta * dst + alpha * bilinear_resize(src), dense
// NHWC, half-pixel centres, edge clamp (== F.interpolate(bilinear, align_corners=False) and
// cv2.resize INTER_LINEAR on float data).  (sy, sx) = source pixels per destination pixel.
__global__ void resize_bilinear_accum_kernel(const float* __restrict__ src, int hs, int ws,
                                             float* __restrict__ dst, int hd, int wd, int C, int N,
                                             float sy, float sx, float alpha, float beta) {
  Walk q;
  if (!pixel_walk(C, N, hd, wd, q)) return;
  float fy = ((float)q.y + 0.5f) * sy - 0.5f, fx = ((float)q.x + 0.5f) * sx - 0.5f;
  fy = fmaxf(fy, 0.f);
  fx = fmaxf(fx, 0.f);
  int y0 = (int)fy, x0 = (int)fx;
  y0 = min(y0, hs - 1);
  x0 = min(x0, ws - 1);
  const int y1 = min(y0 + 1, hs - 1), x1 = min(x0 + 1, ws - 1);
  const float ly = fminf(fy - (float)y0, 1.f), lx = fminf(fx - (float)x0, 1.f);
  const float* s0 = src + ((size_t)q.n * hs + y0) * ws * C + q.c;
  const float* s1 = src + ((size_t)q.n * hs + y1) * ws * C + q.c;
  const float top = s0[(size_t)x0 * C] * (1.f - lx) + s0[(size_t)x1 * C] * lx;
  const float bot = s1[(size_t)x0 * C] * (1.f - lx) + s1[(size_t)x1 * C] * lx;
  const float v = top * (1.f - ly) + bot * ly;
  dst[q.i] = (beta == 0.f ? 0.f : beta * dst[q.i]) + alpha * v;
}

// dst(n,y,x,c) = alpha * dst(n,y,x,c) + beta * src_dense[n][y][x][c]
__global__ void layout_axpby_kernel(float* __restrict__ dst, Lay ld, const float* __restrict__ src, int C,
                                    int N, int H, int W, float alpha, float beta) {
  Walk q;
  if (!pixel_walk(C, N, H, W, q)) return;
  float* d = dst + lay_off(ld, q) + q.c;
  *d = alpha * *d + beta * src[q.i];
}

}  // namespace rtpose

using namespace rtpose;

extern "C" {

int rtpose_layout_axpby(float* dst, const rtpose_layout* ldst, const float* src_nhwc, int C, int N, int H,
                        int W, float alpha, float beta, void* stream) {
  return launch_flat(layout_axpby_kernel, (size_t)N * H * W * C, stream, dst, to_lay(ldst), src_nhwc, C, N, H, W, alpha,
                     beta);
}

int rtpose_preprocess_u8_batch(const rtpose_prep_image* images, int count, int mode, float* dst,
                               const rtpose_layout* ldst, int Hn, int Wn, void* stream) {
  if (!images || count <= 0 || !dst || !ldst || (mode != 0 && mode != 1) || ldst->cstride < 8 ||
      !slice_aligned(ldst, 4) || Hn <= 0 || Wn <= 0)
    return fail(RTPOSE_E_INVAL, "preprocess_u8: bad arguments");
  for (int i = 0; i < count; ++i) {
    const rtpose_prep_image& d = images[i];
    if (!d.img_bgr || d.h0 <= 0 || d.w0 <= 0 || d.im_scale <= 0 || d.hr <= 0 || d.wr <= 0 || Hn < d.hr ||
        Wn < d.wr || d.n_index < 0)
      return fail(RTPOSE_E_INVAL, "preprocess_u8: bad image descriptor %d", i);
  }
  const size_t total = (size_t)Hn * Wn;
  for (int first = 0; first < count; first += kPrepBatch) {  // the descriptors travel as kernel arguments
    PrepBatch b;
    memset(&b, 0, sizeof(b));
    const int n = count - first < kPrepBatch ? count - first : kPrepBatch;
    for (int i = 0; i < n; ++i) {
      const rtpose_prep_image& d = images[first + i];
      PrepImg& o = b.im[i];
      o.img = static_cast<const unsigned char*>(d.img_bgr);
      o.inv_scale = 1.0 / d.im_scale;
      o.h0 = d.h0;
      o.w0 = d.w0;
      o.hr = d.hr;
      o.wr = d.wr;
      o.flip = d.flip ? 1 : 0;
      o.n = d.n_index;
    }
    hipLaunchKernelGGL(preprocess_u8_kernel, dim3(nblocks(total, 256), n), dim3(256), 0, as_stream(stream), b,
                       mode, dst, to_lay(ldst), Hn, Wn);
  }
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_preprocess_u8_flip(const unsigned char* img_bgr, int h0, int w0, double im_scale, int mode, float* dst,
                              const rtpose_layout* ldst, int n_index, int Hn, int Wn, int hr, int wr, int flip,
                              void* stream) {
  rtpose_prep_image d;
  d.img_bgr = img_bgr;
  d.h0 = h0;
  d.w0 = w0;
  d.im_scale = im_scale;
  d.hr = hr;
  d.wr = wr;
  d.flip = flip;
  d.n_index = n_index;
  return rtpose_preprocess_u8_batch(&d, 1, mode, dst, ldst, Hn, Wn, stream);
}

int rtpose_preprocess_u8(const unsigned char* img_bgr, int h0, int w0, double im_scale, int mode, float* dst,
                         const rtpose_layout* ldst, int n_index, int Hn, int Wn, int hr, int wr, void* stream) {
  return rtpose_preprocess_u8_flip(img_bgr, h0, w0, im_scale, mode, dst, ldst, n_index, Hn, Wn, hr, wr, 0, stream);
}

int rtpose_resize_bilinear_accum(const float* src, int hs, int ws, float* dst, int hd, int wd, int C, int N,
                                 float src_h_valid, float src_w_valid, float alpha, float beta, void* stream) {
  if (hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0 || C <= 0 || N <= 0 || src_h_valid <= 0 || src_w_valid <= 0)
    return fail(RTPOSE_E_INVAL, "resize_bilinear_accum: bad sizes");
  return launch_flat(resize_bilinear_accum_kernel, (size_t)N * hd * wd * C, stream, src, hs, ws, dst, hd, wd, C, N,
                     src_h_valid / (float)hd, src_w_valid / (float)wd, alpha, beta);
}

}  // extern "C"
