// Training-batch augmentation on the device (header section 4c): uint8 RGB sources -> the reference's normalised, masked
// 3-channel network input, bit for bit.
//
//   train/train_VGG19.py:124-130 (Normalize, RandomApply(HFlip), RescaleRelative, Crop, CenterPad),
//   lib/datasets/transforms.py:159-207 / :263-313 / :316-362 / :365-389, lib/datasets/utils.py:36-54 (mask_valid_area),
//   Pillow's ImagingResample (Image.resize(size, BICUBIC) on 8-bit RGB)
//
// Pillow resamples in two separable integer passes with a uint8 intermediate.  Its 22-bit coefficients come from float64
// arithmetic with truncating int() casts: resample_entry() restates it in fp64, operation for operation
// (-ffp-contract=off: the order written is the order executed), so the integers are Pillow's.
//
// Two launches per chunk of images.  augment_table_kernel tabulates, per image, both axes of the crop window only
// (<= out_w + out_h entries of 2 + RTPOSE_AUG_MAX_TAPS ints) into the workspace.  augment_kernel, grid (canvas tiles x,
// canvas tiles y, images), owns a 32 x 32 tile of canvas pixels: it maps the tile through pad and crop to a window of
// resized coordinates, stages the source bytes the window's taps reach into LDS (in memory order: a flipped image is
// mirrored by the index the horizontal pass reads with), runs the horizontal pass into a uint8 LDS intermediate, then
// the vertical pass, pad fill, normalisation, mask and store.  The intermediate never goes to memory.  A tile whose source
// window does not fit the LDS budget (factors below 0.5) is walked as 16 x 16, 8 x 8, ... sub-tiles, the size chosen
// per image on the host.  No atomics: an image gives the same bits alone and inside a batch.
//
// Built like decode.hip without the vectorisers (csrc/Makefile): this is meant for a loader stream beside a forward.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                          // canvas pixels per block and axis
constexpr int kTaps = RTPOSE_AUG_MAX_TAPS;
constexpr int kEntry = 2 + kTaps;                  // (first source index, taps, coefficients)
constexpr int kSrcCap = 16384;                     // LDS bytes of the staged source window (73 x 73 x 3 = 15987 at 0.5)
constexpr int kMidCap = 8192;                      // LDS bytes of the horizontal pass's result (73 x 32 x 3 = 7008)
constexpr int kChunk = 32;                         // image descriptors per launch, passed by value
constexpr int kPrecisionBits = 32 - 8 - 2;

struct AugImg {
  const unsigned char* img;
  int h0, w0, hr, wr;
  int flip, crop_x, crop_y, n;
  int left, top, new_w, new_h;  // where the crop window sits in the canvas, and its size
  int mask[4];
  int ltw, lth;                 // log2 of the sub-tile a block stages at a time
  int slot;                     // table slot in the workspace
  int pad;
};
struct AugBatch {
  AugImg im[kChunk];
};
struct AugCfg {
  int out_h, out_w, norm, nchw;
  int fill[3];
};

__device__ __forceinline__ double bicubic(double t) {
  const double a = -0.5;
  if (t < 0.0) t = -t;
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
  return 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output xx of an axis of `in` pixels resampled to `out`:
// e[0] = first source index, e[1] = taps, e[2 + x] = the 22-bit coefficient of tap x (0 behind the taps).
__device__ void resample_entry(int in, int out, int xx, int32_t* __restrict__ e) {
  const double scale = (double)in / (double)out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const double center = ((double)xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  if (xmax > kTaps) xmax = kTaps;  // (the host refused a ksize above kTaps; taps <= ksize)
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += bicubic(((double)(x + xmin) - center + 0.5) * ss);
  e[0] = xmin;
  e[1] = xmax;
  for (int x = 0; x < kTaps; ++x) {
    int32_t k = 0;
    if (x < xmax) {
      double w = bicubic(((double)(x + xmin) - center + 0.5) * ss);
      if (ww != 0.0) w = w / ww;
      k = w < 0.0 ? (int32_t)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int32_t)(0.5 + w * (double)(1 << kPrecisionBits));
    }
    e[2 + x] = k;
  }
}

__global__ __launch_bounds__(kThreads) void resample_table_kernel(int in, int out, int first, int count,
                                                                  int32_t* __restrict__ bounds,
                                                                  int32_t* __restrict__ coeffs) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  int32_t e[kEntry];
  resample_entry(in, out, first + i, e);
  bounds[2 * i] = e[0];
  bounds[2 * i + 1] = e[1];
  for (int x = 0; x < kTaps; ++x) coeffs[(size_t)i * kTaps + x] = e[2 + x];
}

// grid (entries / 256, images): entry e < out_w is column e of the image's crop window, entry out_w + e its row e.
// An axis whose size does not change has no table (it copies).
__global__ __launch_bounds__(kThreads) void augment_table_kernel(const AugBatch b, int out_h, int out_w,
                                                                 int32_t* __restrict__ tables) {
  const AugImg& d = b.im[blockIdx.y];
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= out_w + out_h) return;
  int32_t* dst = tables + ((size_t)d.slot * (out_w + out_h) + e) * kEntry;
  if (e < out_w) {
    if (d.wr != d.w0 && e < d.new_w) resample_entry(d.w0, d.wr, d.crop_x + e, dst);
  } else {
    const int r = e - out_w;
    if (d.hr != d.h0 && r < d.new_h) resample_entry(d.h0, d.hr, d.crop_y + r, dst);
  }
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(kThreads) void augment_kernel(const AugBatch b, const AugCfg c,
                                                           const int32_t* __restrict__ tables,
                                                           float* __restrict__ dst, const Lay ld) {
  __shared__ unsigned char s_src[kSrcCap];   // [window rows][window columns in memory order][3]
  __shared__ unsigned char s_mid[kMidCap];   // [window rows][tile columns][3]
  __shared__ int32_t s_tx[kTile * kEntry];
  __shared__ int32_t s_ty[kTile * kEntry];
  const AugImg& d = b.im[blockIdx.z];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tw = 1 << d.ltw, th = 1 << d.lth;
  const bool fx = d.wr != d.w0, fy = d.hr != d.h0;
  const int32_t* tabx = tables + (size_t)d.slot * (c.out_w + c.out_h) * kEntry;
  const int32_t* taby = tabx + (size_t)c.out_w * kEntry;
  const unsigned char* __restrict__ img = d.img;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const size_t plane = (size_t)c.out_h * c.out_w;

  for (int oy = 0; oy < kTile; oy += th)
    for (int ox = 0; ox < kTile; ox += tw) {
      // canvas pixels [cx0, cx1) x [cy0, cy1) of this sub-tile (the conditions below are uniform over the block)
      const int cx0 = blockIdx.x * kTile + ox, cy0 = blockIdx.y * kTile + oy;
      if (cx0 >= c.out_w || cy0 >= c.out_h) continue;
      const int cx1 = min(cx0 + tw, c.out_w), cy1 = min(cy0 + th, c.out_h);
      // its part of the crop window: entries [ex0, ex1) x [ey0, ey1) of the tables = resized pixel - crop offset
      const int ex0 = max(cx0 - d.left, 0), ex1 = min(cx1 - d.left, d.new_w);
      const int ey0 = max(cy0 - d.top, 0), ey1 = min(cy1 - d.top, d.new_h);
      const int nw = ex1 - ex0, nh = ey1 - ey0;
      bool any = nw > 0 && nh > 0;
      bool overflow = false;
      int sx0 = 0, sy0 = 0, ww = 0, wh = 0;
      __syncthreads();  // the sub-tile before has been consumed
      if (any) {
        if (fx)
          for (int i = t; i < nw * kEntry; i += kThreads) s_tx[i] = tabx[(size_t)ex0 * kEntry + i];
        if (fy)
          for (int i = t; i < nh * kEntry; i += kThreads) s_ty[i] = taby[(size_t)ey0 * kEntry + i];
        __syncthreads();
        // first source index and bounds are non-decreasing along an axis: the window is first entry .. last entry
        sx0 = fx ? s_tx[0] : ex0 + d.crop_x;
        sy0 = fy ? s_ty[0] : ey0 + d.crop_y;
        ww = fx ? s_tx[(nw - 1) * kEntry] + s_tx[(nw - 1) * kEntry + 1] - sx0 : nw;
        wh = fy ? s_ty[(nh - 1) * kEntry] + s_ty[(nh - 1) * kEntry + 1] - sy0 : nh;
        // never taken while the host's sub-tile choice bounds the window; a NaN canvas would say it does not
        overflow = wh * ww * 3 > kSrcCap || wh * nw * 3 > kMidCap || ww < 1 || wh < 1;
        if (overflow) any = false;
      }
      if (any) {
        // source window in memory order: columns [mx0, mx0 + ww) of rows [sy0, sy0 + wh)
        const int mx0 = d.flip ? d.w0 - (sx0 + ww) : sx0;
        const int rowb = ww * 3;
        for (int r = wave; r < wh; r += kThreads / 64) {
          const unsigned char* g = img + ((size_t)(sy0 + r) * d.w0 + mx0) * 3;
          for (int q = lane; q < rowb; q += 64) s_src[r * rowb + q] = g[q];
        }
        __syncthreads();
        // horizontal pass (or copy) into s_mid[r][x][ch]
        const int midb = nw * 3;
        for (int r = wave; r < wh; r += kThreads / 64) {
          const unsigned char* row = s_src + r * rowb;
          for (int q = lane; q < midb; q += 64) {
            const int x = q / 3, ch = q - 3 * x;
            int v;
            if (fx) {
              const int32_t* e = s_tx + x * kEntry;
              const int m = e[0] - sx0, cnt = e[1];
              int acc = 1 << (kPrecisionBits - 1);
              for (int k = 0; k < cnt; ++k) {
                const int col = d.flip ? ww - 1 - (m + k) : m + k;
                acc += (int)row[col * 3 + ch] * e[2 + k];
              }
              v = clip8(acc >> kPrecisionBits);
            } else {
              const int col = d.flip ? ww - 1 - x : x;
              v = row[col * 3 + ch];
            }
            s_mid[r * midb + q] = (unsigned char)v;
          }
        }
        __syncthreads();
      }
      // vertical pass (or copy), pad fill, normalisation, mask, store: a thread per canvas pixel
      const int midb = nw * 3;
      for (int p = t; p < tw * th; p += kThreads) {
        const int py = p >> d.ltw, px = p & (tw - 1);
        const int cx = cx0 + px, cy = cy0 + py;
        if (cx >= cx1 || cy >= cy1) continue;
        const int ix = cx - d.left - ex0, iy = cy - d.top - ey0;
        const bool inside = any && ix >= 0 && ix < nw && iy >= 0 && iy < nh;
        const bool keep = cx >= d.mask[0] && cx < d.mask[2] && cy >= d.mask[1] && cy < d.mask[3];
        for (int ch = 0; ch < 3; ++ch) {
          int u = c.fill[ch];
          if (inside) {
            if (fy) {
              const int32_t* e = s_ty + iy * kEntry;
              const int m = e[0] - sy0, cnt = e[1];
              int acc = 1 << (kPrecisionBits - 1);
              for (int k = 0; k < cnt; ++k) acc += (int)s_mid[(m + k) * midb + ix * 3 + ch] * e[2 + k];
              u = clip8(acc >> kPrecisionBits);
            } else {
              u = s_mid[iy * midb + ix * 3 + ch];
            }
          }
          float v = (float)u;
          if (c.norm) {
            v = v / 255.0f;
            v = v - mean[ch];
            v = v / stdv[ch];
          }
          if (!keep) v = 0.0f;
          if (overflow) v = __builtin_nanf("");
          if (c.nchw)
            dst[((size_t)d.n * 3 + ch) * plane + (size_t)cy * c.out_w + cx] = v;
          else
            dst[lay_off(ld, d.n, cy, cx) + ch] = v;
        }
      }
    }
}

int ksize_of(int in, int out) {
  const double scale = (double)in / (double)out;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)std::ceil(support) * 2 + 1;
}

// upper bound of the source pixels the taps of n consecutive outputs reach: (n - 1) * scale + 2 * support + 1 and the
// truncations of the two bounds; n where the axis is copied
int window_bound(int n, int in, int out) {
  if (in == out) return n;
  return (int)std::ceil((n - 1) * ((double)in / (double)out)) + ksize_of(in, out) + 2;
}

int check_augment_cfg(const rtpose_augment_cfg* cfg) {
  if (!cfg) return fail(RTPOSE_E_INVAL, "augment: NULL cfg");
  if (cfg->struct_bytes != sizeof(rtpose_augment_cfg))
    return fail(RTPOSE_E_INVAL, "augment: cfg.struct_bytes is %u, this library's rtpose_augment_cfg has %zu",
                cfg->struct_bytes, sizeof(rtpose_augment_cfg));
  if (cfg->norm != 0 && cfg->norm != 1) return fail(RTPOSE_E_INVAL, "augment: cfg.norm %d is neither 0 nor 1", cfg->norm);
  if (cfg->nchw != 0 && cfg->nchw != 1) return fail(RTPOSE_E_INVAL, "augment: cfg.nchw %d is neither 0 nor 1", cfg->nchw);
  if (cfg->out_h < 1 || cfg->out_h > 65535 || cfg->out_w < 1 || cfg->out_w > 65535)
    return fail(RTPOSE_E_INVAL, "augment: canvas out_h %d x out_w %d outside [1,65535]", cfg->out_h, cfg->out_w);
  return 0;
}

int check_augment_image(const rtpose_augment_image& d, int i, const rtpose_augment_cfg* cfg) {
  if (!d.img_rgb) return fail(RTPOSE_E_INVAL, "augment: image %d: NULL img_rgb", i);
  if (d.h0 < 1 || d.w0 < 1) return fail(RTPOSE_E_INVAL, "augment: image %d: source size h0 %d x w0 %d below 1", i, d.h0, d.w0);
  if (d.hr < 1 || d.wr < 1) return fail(RTPOSE_E_INVAL, "augment: image %d: resized size hr %d x wr %d below 1", i, d.hr, d.wr);
  if ((long long)d.h0 * d.w0 > 0x7fffff00ll / 3)
    return fail(RTPOSE_E_INVAL, "augment: image %d: source h0 %d x w0 %d above 2^31 bytes", i, d.h0, d.w0);
  if (ksize_of(d.w0, d.wr) > RTPOSE_AUG_MAX_TAPS)
    return fail(RTPOSE_E_INVAL, "augment: image %d: wr %d from w0 %d needs %d taps, RTPOSE_AUG_MAX_TAPS is %d", i, d.wr, d.w0,
                ksize_of(d.w0, d.wr), RTPOSE_AUG_MAX_TAPS);
  if (ksize_of(d.h0, d.hr) > RTPOSE_AUG_MAX_TAPS)
    return fail(RTPOSE_E_INVAL, "augment: image %d: hr %d from h0 %d needs %d taps, RTPOSE_AUG_MAX_TAPS is %d", i, d.hr, d.h0,
                ksize_of(d.h0, d.hr), RTPOSE_AUG_MAX_TAPS);
  const int max_x = d.wr > cfg->out_w ? d.wr - cfg->out_w : 0, max_y = d.hr > cfg->out_h ? d.hr - cfg->out_h : 0;
  if (d.crop_x < 0 || d.crop_x > max_x)
    return fail(RTPOSE_E_INVAL, "augment: image %d: crop_x %d outside [0,%d]", i, d.crop_x, max_x);
  if (d.crop_y < 0 || d.crop_y > max_y)
    return fail(RTPOSE_E_INVAL, "augment: image %d: crop_y %d outside [0,%d]", i, d.crop_y, max_y);
  if (d.mask[0] < 0 || d.mask[2] > cfg->out_w || d.mask[0] > d.mask[2])
    return fail(RTPOSE_E_INVAL, "augment: image %d: mask x [%d,%d) outside the canvas [0,%d) or reversed", i, d.mask[0],
                d.mask[2], cfg->out_w);
  if (d.mask[1] < 0 || d.mask[3] > cfg->out_h || d.mask[1] > d.mask[3])
    return fail(RTPOSE_E_INVAL, "augment: image %d: mask y [%d,%d) outside the canvas [0,%d) or reversed", i, d.mask[1],
                d.mask[3], cfg->out_h);
  if (d.n_index < 0 || d.n_index > 65535) return fail(RTPOSE_E_INVAL, "augment: image %d: n_index %d outside [0,65535]", i, d.n_index);
  return 0;
}

}  // namespace
}  // namespace rtpose

using namespace rtpose;

extern "C" {

size_t rtpose_augment_workspace_bytes(const rtpose_augment_cfg* cfg, int count) {
  if (count < 0 || check_augment_cfg(cfg)) return 0;
  const size_t bytes = (size_t)count * (cfg->out_w + cfg->out_h) * kEntry * sizeof(int32_t);
  return round_up(bytes < 1 ? 1 : bytes, 256);
}

int rtpose_resample_table(int in_size, int out_size, int first, int count, int32_t* bounds, int32_t* coeffs,
                          void* stream) {
  if (!bounds) return fail(RTPOSE_E_INVAL, "resample_table: NULL bounds");
  if (!coeffs) return fail(RTPOSE_E_INVAL, "resample_table: NULL coeffs");
  if (in_size < 1 || out_size < 1)
    return fail(RTPOSE_E_INVAL, "resample_table: in_size %d / out_size %d below 1", in_size, out_size);
  if (ksize_of(in_size, out_size) > RTPOSE_AUG_MAX_TAPS)
    return fail(RTPOSE_E_INVAL, "resample_table: out_size %d from in_size %d needs %d taps, RTPOSE_AUG_MAX_TAPS is %d",
                out_size, in_size, ksize_of(in_size, out_size), RTPOSE_AUG_MAX_TAPS);
  if (first < 0 || count < 0 || first > out_size - count)
    return fail(RTPOSE_E_INVAL, "resample_table: first %d + count %d outside the %d outputs", first, count, out_size);
  if (count == 0) return 0;
  static thread_local CheckedPtr c_b, c_c;
  const int dev = current_device();
  int rc = c_b.check(bounds, dev, "resample_table", "bounds");
  if (!rc) rc = c_c.check(coeffs, dev, "resample_table", "coeffs");
  if (rc) return rc;
  hipLaunchKernelGGL(resample_table_kernel, dim3(ceil_div(count, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     in_size, out_size, first, count, bounds, coeffs);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_augment_batch(const rtpose_augment_image* images, int count, const rtpose_augment_cfg* cfg, float* dst,
                         const rtpose_layout* ldst, void* workspace, size_t workspace_bytes, void* stream) {
  if (!images) return fail(RTPOSE_E_INVAL, "augment: NULL images");
  if (!dst) return fail(RTPOSE_E_INVAL, "augment: NULL dst");
  if (!workspace) return fail(RTPOSE_E_INVAL, "augment: NULL workspace");
  if (int rc = check_augment_cfg(cfg)) return rc;
  if (count < 0) return fail(RTPOSE_E_INVAL, "augment: count %d is negative", count);
  if (!cfg->nchw) {
    if (!ldst) return fail(RTPOSE_E_INVAL, "augment: NULL ldst with cfg.nchw == 0");
    if (ldst->cstride - ldst->choff < 3 || ldst->choff < 0)
      return fail(RTPOSE_E_INVAL, "augment: ldst addresses %d channels from choff %d (cstride %d), 3 are written",
                  ldst->cstride - ldst->choff, ldst->choff, ldst->cstride);
    if (cfg->out_w > ldst->ws || cfg->out_h > ldst->hs)
      return fail(RTPOSE_E_INVAL, "augment: a %d x %d canvas in a ldst view of %d x %d", cfg->out_h, cfg->out_w, ldst->hs,
                  ldst->ws);
  }
  for (int i = 0; i < count; ++i)
    if (int rc = check_augment_image(images[i], i, cfg)) return rc;
  const size_t need = rtpose_augment_workspace_bytes(cfg, count);
  if (workspace_bytes < need)
    return fail(RTPOSE_E_INVAL, "augment: workspace_bytes %zu below the %zu rtpose_augment_workspace_bytes reports",
                workspace_bytes, need);
  if (count == 0) return 0;
  static thread_local CheckedPtr c_dst, c_ws;
  const int dev = current_device();
  int rc = c_dst.check(dst, dev, "augment", "dst");
  if (!rc) rc = c_ws.check(workspace, dev, "augment", "the workspace");
  for (int i = 0; i < count && !rc; ++i) rc = check_device_ptr(images[i].img_rgb, dev, "augment", "an image's img_rgb");
  if (rc) return rc;

  AugCfg c;
  c.out_h = cfg->out_h;
  c.out_w = cfg->out_w;
  c.norm = cfg->norm;
  c.nchw = cfg->nchw;
  for (int k = 0; k < 3; ++k) c.fill[k] = cfg->fill[k];
  const Lay ld = cfg->nchw ? Lay{3, 0, cfg->out_w, cfg->out_h, 0} : to_lay(ldst);
  hipStream_t s = as_stream(stream);
  int32_t* tables = static_cast<int32_t*>(workspace);
  for (int first = 0; first < count; first += kChunk) {  // the descriptors travel as kernel arguments
    AugBatch b;
    memset(&b, 0, sizeof(b));
    const int n = count - first < kChunk ? count - first : kChunk;
    bool any_table = false;
    for (int i = 0; i < n; ++i) {
      const rtpose_augment_image& d = images[first + i];
      AugImg& o = b.im[i];
      o.img = static_cast<const unsigned char*>(d.img_rgb);
      o.h0 = d.h0;
      o.w0 = d.w0;
      o.hr = d.hr;
      o.wr = d.wr;
      o.flip = d.hflip ? 1 : 0;
      o.crop_x = d.crop_x;
      o.crop_y = d.crop_y;
      o.n = d.n_index;
      // Crop.crop's new_w (transforms.py:301) and CenterPad.center_pad's left (:342)
      o.new_w = cfg->out_w < d.wr - d.crop_x ? cfg->out_w : d.wr - d.crop_x;
      o.new_h = cfg->out_h < d.hr - d.crop_y ? cfg->out_h : d.hr - d.crop_y;
      o.left = (cfg->out_w - o.new_w) / 2;
      o.top = (cfg->out_h - o.new_h) / 2;
      for (int k = 0; k < 4; ++k) o.mask[k] = d.mask[k];
      // the largest sub-tile whose source window and intermediate fit the LDS budget (a 1 x 1 sub-tile always does:
      // (ksize + 2)^2 * 3 bytes)
      int ltw = 5, lth = 5;
      for (;;) {
        const int wx = window_bound(1 << ltw, d.w0, d.wr), wy = window_bound(1 << lth, d.h0, d.hr);
        if ((wx * wy * 3 <= kSrcCap && wy * (1 << ltw) * 3 <= kMidCap) || (ltw == 0 && lth == 0)) break;
        if (lth > 0 && (wy >= wx || ltw == 0)) --lth; else --ltw;
      }
      o.ltw = ltw;
      o.lth = lth;
      o.slot = first + i;
      any_table = any_table || d.wr != d.w0 || d.hr != d.h0;
    }
    if (any_table) {
      hipLaunchKernelGGL(augment_table_kernel, dim3(ceil_div(cfg->out_w + cfg->out_h, kThreads), n), dim3(kThreads), 0, s, b,
                         cfg->out_h, cfg->out_w, tables);
      RTPOSE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(augment_kernel, dim3(ceil_div(cfg->out_w, kTile), ceil_div(cfg->out_h, kTile), n), dim3(kThreads), 0,
                       s, b, c, tables, dst, ld);
    RTPOSE_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
