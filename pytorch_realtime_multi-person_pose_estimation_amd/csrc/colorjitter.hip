// Colour jitter of the padded canvas on the device (header section 4d): torchvision's ColorJitter and RandomGrayscale on
// the 8-bit RGB canvas, then ToTensor + Normalize and the valid-area mask - Pillow's bits.
//
//   lib/datasets/transforms.py:53-65 (image_transform_train; its JPEG step is jpeg_roundtrip.hip, header section 4e), lib/datasets/datasets.py:193-204,
//   Pillow's ImageEnhance.Brightness / Contrast / Color over ImagingBlend, convert('L'), convert('HSV'), convert('RGB')
//
// Every operation is restated in the number format Pillow's C uses for it (-ffp-contract=off: the order written is the
// order executed; fp32 and fp64 division are IEEE).  All but one are per pixel.  Contrast blends with the rounded mean
// of L over the whole canvas as the operations before it left it: jitter_lsum_kernel, grid (slabs, images with
// contrast), applies those operations on the fly and writes one uint32 partial per slab into the workspace;
// jitter_apply_kernel, grid (256-pixel pieces, images), adds the image's partials in uint64, forms the mean in fp64 and
// runs the whole chain on its pixel.  The sums are integers: no atomics and no order to keep, an image gives the same
// bits alone and inside any batch.
//
// Built like augment.hip without the vectorisers (csrc/Makefile): this is meant for a loader stream beside a forward.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;        // image descriptors per launch, passed by value
constexpr int kMaxSlabs = 1024;
constexpr int kOps = 4;

struct JitImg {
  int order[kOps];
  float factor[3];
  int hue, gray;
  int mask[4];
  int n_src, n_dst;
  int contrast_at;  // the index of contrast in order, or -1
  int slot;         // this image's partials in the workspace
};
struct JitBatch {
  JitImg im[kChunk];
};
struct JitCfg {
  int h, w, norm, nchw;
  unsigned pixels;  // h * w <= 65535^2 < 2^32
  unsigned slab;    // pixels per slab
  int slabs;
};

struct Rgb {
  int r, g, b;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// what a source float stands for: (int)v clamped to 0..255, NaN -> 0
__device__ __forceinline__ int read_u8(float v) { return v >= 0.0f ? (v <= 255.0f ? (int)v : 255) : 0; }

__device__ __forceinline__ int luma(const Rgb& p) { return (p.r * 19595 + p.g * 38470 + p.b * 7471 + 0x8000) >> 16; }

// Pillow's ImagingBlend(degenerate d, image x, alpha) on one uint8 channel
__device__ __forceinline__ int blend(int d, int x, float alpha) {
  const float fd = (float)d;
  const float diff = (float)x - fd;
  const float scaled = alpha * diff;
  const float t = fd + scaled;
  if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 255;
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (int)t;
}

__device__ __forceinline__ Rgb blend3(int d, const Rgb& p, float alpha) {
  return Rgb{blend(d, p.r, alpha), blend(d, p.g, alpha), blend(d, p.b, alpha)};
}

// Pillow's rgb2hsv_row, H moved by `shift` modulo 256, then its hsv2rgb
__device__ __forceinline__ Rgb hue_round_trip(const Rgb& p, int shift) {
  const int maxc = max(p.r, max(p.g, p.b)), minc = min(p.r, min(p.g, p.b));
  const int V = maxc;
  int H = 0, S = 0;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - p.r) / cr;
    const float gc = (float)(maxc - p.g) / cr;
    const float bc = (float)(maxc - p.b) / cr;
    float h;
    if (p.r == maxc) {
      h = bc - gc;
    } else if (p.g == maxc) {
      const double a = 2.0 + (double)rc;
      h = (float)(a - (double)bc);
    } else {
      const double a = 4.0 + (double)gc;
      h = (float)(a - (double)rc);
    }
    const double turn = (double)h / 6.0 + 1.0;  // in [5 / 6, 11 / 6]: fmod(turn, 1.0) is turn - floor(turn), exactly
    h = (float)(turn - floor(turn));
    H = clip8((int)((double)h * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) return Rgb{V, V, V};
  const double hf = (double)(float)H * 6.0 / 255.0;
  const double fl = floor(hf);
  const int i = (int)fl;
  const float f = (float)(hf - fl);
  const float fs = (float)((double)S / 255.0);
  const float fsf = fs * f;
  const double v = (double)V;
  const int pp = clip8((int)round(v * (1.0 - (double)fs)));
  const int qq = clip8((int)round(v * (1.0 - (double)fsf)));
  const int tt = clip8((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))));
  switch (i % 6) {
    case 0: return Rgb{V, tt, pp};
    case 1: return Rgb{qq, V, pp};
    case 2: return Rgb{pp, V, tt};
    case 3: return Rgb{pp, qq, V};
    case 4: return Rgb{tt, pp, V};
    default: return Rgb{V, pp, qq};
  }
}

// operations order[first .. last) of an image on one pixel; m is contrast's mean
__device__ __forceinline__ Rgb run_ops(Rgb p, const JitImg& d, int first, int last, int m) {
  for (int k = first; k < last; ++k) {
    const int op = d.order[k];
    if (op == 0)
      p = blend3(0, p, d.factor[0]);
    else if (op == 1)
      p = blend3(m, p, d.factor[1]);
    else if (op == 2)
      p = blend3(luma(p), p, d.factor[2]);
    else if (op == 3)
      p = hue_round_trip(p, d.hue);
  }
  return p;
}

__device__ __forceinline__ Rgb read_pixel(const float* src, size_t plane, int n, unsigned p) {
  const float* s = src + (size_t)n * 3 * plane + p;
  return Rgb{read_u8(s[0]), read_u8(s[plane]), read_u8(s[2 * plane])};
}

// grid (slabs, images with contrast): the host puts those first in the chunk
__global__ __launch_bounds__(kThreads) void jitter_lsum_kernel(const JitBatch b, const JitCfg c,
                                                               const float* __restrict__ src,
                                                               uint32_t* __restrict__ partials) {
  __shared__ uint32_t red[kThreads];
  const JitImg& d = b.im[blockIdx.y];
  const int t = threadIdx.x;
  uint32_t acc = 0;  // at most slab / 256 * 255 < 2^22
  if (d.contrast_at >= 0) {
    const size_t plane = (size_t)c.pixels;
    const unsigned p0 = blockIdx.x * c.slab;
    const unsigned left = c.pixels - p0;  // p0 < pixels: the grid has ceil(pixels / slab) slabs
    const unsigned n = left < c.slab ? left : c.slab;
    for (unsigned i = t; i < n; i += kThreads) {
      const Rgb q = run_ops(read_pixel(src, plane, d.n_src, p0 + i), d, 0, d.contrast_at, 0);
      acc += (uint32_t)luma(q);
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];  // a slab's sum: at most 2^22 * 255 < 2^30
    __syncthreads();
  }
  if (t == 0 && d.contrast_at >= 0) partials[(size_t)d.slot * c.slabs + blockIdx.x] = red[0];
}

// (src and dst may be the same memory: a thread reads its pixel before it writes it)
__global__ __launch_bounds__(kThreads) void jitter_apply_kernel(const JitBatch b, const JitCfg c, const float* src,
                                                                const uint32_t* __restrict__ partials, float* dst,
                                                                const Lay ld) {
  __shared__ unsigned long long red[kThreads];
  __shared__ int s_mean;
  const JitImg& d = b.im[blockIdx.y];
  const int t = threadIdx.x;
  int m = 0;
  if (d.contrast_at >= 0) {  // uniform over the block
    const uint32_t* ps = partials + (size_t)d.slot * c.slabs;
    unsigned long long acc = 0;
    for (int i = t; i < c.slabs; i += kThreads) acc += ps[i];
    red[t] = acc;
    __syncthreads();
    if (t == 0) {
      unsigned long long sum = 0;
      for (int i = 0; i < kThreads; ++i) sum += red[i];
      // ImageStat's mean and ImageEnhance.Contrast's int(mean + 0.5): sum and count are exact in fp64
      const double mean = (double)sum / (double)c.pixels;
      s_mean = (int)(mean + 0.5);
    }
    __syncthreads();
    m = s_mean;
  }
  const unsigned p = blockIdx.x * (unsigned)kThreads + t;
  if (p >= c.pixels) return;
  const size_t plane = (size_t)c.pixels;
  Rgb q = run_ops(read_pixel(src, plane, d.n_src, p), d, 0, kOps, m);
  if (d.gray) {
    const int l = luma(q);
    q = Rgb{l, l, l};
  }
  const unsigned y = p / (unsigned)c.w, x = p - y * (unsigned)c.w;
  const bool keep = (int)x >= d.mask[0] && (int)x < d.mask[2] && (int)y >= d.mask[1] && (int)y < d.mask[3];
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const int u[3] = {q.r, q.g, q.b};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float v = (float)u[ch];
    if (c.norm) {
      v = v / 255.0f;
      v = v - mean[ch];
      v = v / stdv[ch];
    }
    if (!keep) v = 0.0f;
    if (c.nchw)
      dst[((size_t)d.n_dst * 3 + ch) * plane + p] = v;
    else
      dst[lay_off(ld, d.n_dst, (int)y, (int)x) + ch] = v;
  }
}

int check_jitter_cfg(const rtpose_jitter_cfg* cfg) {
  if (!cfg) return fail(RTPOSE_E_INVAL, "jitter: NULL cfg");
  if (cfg->struct_bytes != sizeof(rtpose_jitter_cfg))
    return fail(RTPOSE_E_INVAL, "jitter: cfg.struct_bytes is %u, this library's rtpose_jitter_cfg has %zu", cfg->struct_bytes,
                sizeof(rtpose_jitter_cfg));
  if (cfg->norm != 0 && cfg->norm != 1) return fail(RTPOSE_E_INVAL, "jitter: cfg.norm %d is neither 0 nor 1", cfg->norm);
  if (cfg->nchw != 0 && cfg->nchw != 1) return fail(RTPOSE_E_INVAL, "jitter: cfg.nchw %d is neither 0 nor 1", cfg->nchw);
  if (cfg->h < 1 || cfg->h > 65535 || cfg->w < 1 || cfg->w > 65535)
    return fail(RTPOSE_E_INVAL, "jitter: canvas h %d x w %d outside [1,65535]", cfg->h, cfg->w);
  return 0;
}

// shape only: slabs of equal multiples of RTPOSE_JITTER_SLAB pixels but for the last one, at most kMaxSlabs of them
JitCfg geometry(const rtpose_jitter_cfg* cfg) {
  JitCfg c;
  c.h = cfg->h;
  c.w = cfg->w;
  c.norm = cfg->norm;
  c.nchw = cfg->nchw;
  const unsigned long long P = (unsigned long long)cfg->h * cfg->w;
  const unsigned long long per = (unsigned long long)RTPOSE_JITTER_SLAB * kMaxSlabs;
  c.pixels = (unsigned)P;
  c.slab = (unsigned)(RTPOSE_JITTER_SLAB * ((P + per - 1) / per));
  c.slabs = (int)((P + c.slab - 1) / c.slab);
  return c;
}

int check_jitter_image(const rtpose_jitter_image& d, int i, const rtpose_jitter_cfg* cfg) {
  static const char* const names[3] = {"brightness", "contrast", "saturation"};
  unsigned seen = 0;
  for (int k = 0; k < kOps; ++k) {
    const int op = d.order[k];
    if (op < -1 || op > 3) return fail(RTPOSE_E_INVAL, "jitter: image %d: order[%d] %d outside {-1, 0..3}", i, k, op);
    if (op < 0) continue;
    if (seen & (1u << op)) return fail(RTPOSE_E_INVAL, "jitter: image %d: order[%d] names operation %d twice", i, k, op);
    seen |= 1u << op;
  }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(d.factor[k]) || d.factor[k] < 0.0f)
      return fail(RTPOSE_E_INVAL, "jitter: image %d: factor[%d] (%s) %g is not finite or is negative", i, k, names[k],
                  (double)d.factor[k]);
  if (d.hue_shift < 0 || d.hue_shift > 255)
    return fail(RTPOSE_E_INVAL, "jitter: image %d: hue_shift %d outside [0,255]", i, d.hue_shift);
  if (d.mask[0] < 0 || d.mask[2] > cfg->w || d.mask[0] > d.mask[2])
    return fail(RTPOSE_E_INVAL, "jitter: image %d: mask x [%d,%d) outside the canvas [0,%d) or reversed", i, d.mask[0],
                d.mask[2], cfg->w);
  if (d.mask[1] < 0 || d.mask[3] > cfg->h || d.mask[1] > d.mask[3])
    return fail(RTPOSE_E_INVAL, "jitter: image %d: mask y [%d,%d) outside the canvas [0,%d) or reversed", i, d.mask[1],
                d.mask[3], cfg->h);
  if (d.n_src < 0 || d.n_src > 65535) return fail(RTPOSE_E_INVAL, "jitter: image %d: n_src %d outside [0,65535]", i, d.n_src);
  if (d.n_dst < 0 || d.n_dst > 65535) return fail(RTPOSE_E_INVAL, "jitter: image %d: n_dst %d outside [0,65535]", i, d.n_dst);
  return 0;
}

}  // namespace
}  // namespace rtpose

using namespace rtpose;

extern "C" {

size_t rtpose_jitter_workspace_bytes(const rtpose_jitter_cfg* cfg, int count) {
  if (count < 0 || check_jitter_cfg(cfg)) return 0;
  const size_t bytes = (size_t)count * geometry(cfg).slabs * sizeof(uint32_t);
  return round_up(bytes < 1 ? 1 : bytes, 256);
}

int rtpose_jitter_batch(const rtpose_jitter_image* images, int count, const rtpose_jitter_cfg* cfg, const float* src,
                        float* dst, const rtpose_layout* ldst, void* workspace, size_t workspace_bytes, void* stream) {
  if (!images) return fail(RTPOSE_E_INVAL, "jitter: NULL images");
  if (!src) return fail(RTPOSE_E_INVAL, "jitter: NULL src");
  if (!dst) return fail(RTPOSE_E_INVAL, "jitter: NULL dst");
  if (!workspace) return fail(RTPOSE_E_INVAL, "jitter: NULL workspace");
  if (int rc = check_jitter_cfg(cfg)) return rc;
  if (count < 0) return fail(RTPOSE_E_INVAL, "jitter: count %d is negative", count);
  if (!cfg->nchw) {
    if (!ldst) return fail(RTPOSE_E_INVAL, "jitter: NULL ldst with cfg.nchw == 0");
    if (ldst->cstride - ldst->choff < 3 || ldst->choff < 0)
      return fail(RTPOSE_E_INVAL, "jitter: ldst addresses %d channels from choff %d (cstride %d), 3 are written",
                  ldst->cstride - ldst->choff, ldst->choff, ldst->cstride);
    if (cfg->w > ldst->ws || cfg->h > ldst->hs)
      return fail(RTPOSE_E_INVAL, "jitter: a %d x %d canvas in a ldst view of %d x %d", cfg->h, cfg->w, ldst->hs, ldst->ws);
    if (dst == src) return fail(RTPOSE_E_INVAL, "jitter: dst == src with cfg.nchw == 0 (in place is dense only)");
  }
  for (int i = 0; i < count; ++i) {
    if (int rc = check_jitter_image(images[i], i, cfg)) return rc;
    if (dst == src && images[i].n_dst != images[i].n_src)
      return fail(RTPOSE_E_INVAL, "jitter: image %d: dst == src with n_dst %d != n_src %d (in place keeps the slot)", i,
                  images[i].n_dst, images[i].n_src);
  }
  const size_t need = rtpose_jitter_workspace_bytes(cfg, count);
  if (workspace_bytes < need)
    return fail(RTPOSE_E_INVAL, "jitter: workspace_bytes %zu below the %zu rtpose_jitter_workspace_bytes reports",
                workspace_bytes, need);
  if (count == 0) return 0;
  static thread_local CheckedPtr c_src, c_dst, c_ws;
  const int dev = current_device();
  int rc = c_src.check(src, dev, "jitter", "src");
  if (!rc) rc = c_dst.check(dst, dev, "jitter", "dst");
  if (!rc) rc = c_ws.check(workspace, dev, "jitter", "the workspace");
  if (rc) return rc;

  const JitCfg c = geometry(cfg);
  const Lay ld = cfg->nchw ? Lay{3, 0, cfg->w, cfg->h, 0} : to_lay(ldst);
  hipStream_t s = as_stream(stream);
  uint32_t* partials = static_cast<uint32_t*>(workspace);
  const unsigned pieces = (unsigned)(((unsigned long long)c.pixels + kThreads - 1) / kThreads);
  for (int first = 0; first < count; first += kChunk) {  // the descriptors travel as kernel arguments
    JitBatch b;
    memset(&b, 0, sizeof(b));
    const int n = count - first < kChunk ? count - first : kChunk;
    // the images with contrast lead the chunk's launch order so that the L-sum pass covers a prefix: [0, with)
    int with = 0;
    for (int pass = 0; pass < 2; ++pass) {
      int at = pass == 0 ? 0 : with;
      for (int i = 0; i < n; ++i) {
        const rtpose_jitter_image& d = images[first + i];
        int contrast_at = -1;
        for (int k = 0; k < kOps; ++k)
          if (d.order[k] == 1) contrast_at = k;
        if ((contrast_at >= 0) != (pass == 0)) continue;
        JitImg& o = b.im[at++];
        for (int k = 0; k < kOps; ++k) o.order[k] = d.order[k];
        for (int k = 0; k < 3; ++k) o.factor[k] = d.factor[k];
        o.hue = d.hue_shift;
        o.gray = d.gray ? 1 : 0;
        for (int k = 0; k < 4; ++k) o.mask[k] = d.mask[k];
        o.n_src = d.n_src;
        o.n_dst = d.n_dst;
        o.contrast_at = contrast_at;
        o.slot = first + i;
      }
      if (pass == 0) with = at;
    }
    if (with > 0) {
      hipLaunchKernelGGL(jitter_lsum_kernel, dim3(c.slabs, with), dim3(kThreads), 0, s, b, c, src, partials);
      RTPOSE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(jitter_apply_kernel, dim3(pieces, n), dim3(kThreads), 0, s, b, c, src, partials, dst, ld);
    RTPOSE_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
