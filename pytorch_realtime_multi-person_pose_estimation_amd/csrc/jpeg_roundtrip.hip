// JPEG re-compression of the padded canvas on the device (header section 4e): what saving an 8-bit RGB image as a JPEG
// and re-opening it does to its pixels - libjpeg-turbo's bits (4:2:0, JDCT_ISLOW, fancy up-sampling).
//
//   lib/datasets/transforms.py:28-31,58-61 (RandomApply([jpeg_compression_augmentation], p=0.1) of image_transform_train),
//   libjpeg's jccolor / jcsample / jfdctint / jcdctmgr on the way in, jidctint / jdsample / jdcolor on the way out
//
// Huffman coding is lossless, so the pixels that come back depend on integer arithmetic alone.  Two launches per 32 images:
// jpeg_codec_kernel, grid (runs of 4 MCUs, MCU rows, images), takes a 64 x 16 piece of the canvas through colour
// conversion, the edge rules, chroma down-sampling, the forward DCT, the quantiser, the inverse DCT and the range limit in
// LDS and stores the decoder's 8-bit Y, Cb and Cr samples into the caller's workspace; jpeg_upsample_kernel, grid
// (256-pixel pieces, images), up-samples chroma with the triangle filter - which reads across MCU borders: hence the
// workspace between the launches instead of halos -, converts to RGB and stores float(u).  Every image's codec launch
// precedes every up-sample launch on the stream: all sources are read before any destination is written, which is what
// makes in-place operation legal.  No floating-point arithmetic but the final int -> float; every intermediate is int32,
// as in libjpeg-turbo's SIMD passes (on binary noise at quality 1 the inverse DCT's sums of magnitudes reach 0.13 * 2^31).
//
// Built like colorjitter.hip without the vectorisers (csrc/Makefile): this is meant for a loader stream beside a forward.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;      // image descriptors per launch, passed by value
constexpr int kRun = 4;         // MCUs a block takes: 64 x 16 pixels = 16 Y blocks + 4 Cb blocks + 4 Cr blocks
constexpr int kBlocks = 24;
constexpr int kRowStride = 9;   // ints between the rows of an 8 x 8 block in LDS: the column passes walk 8 banks apart
constexpr int kBlkStride = 8 * kRowStride;
constexpr int kDctThreads = kBlocks * 8;  // one thread per row (or column) of a block

// jfdctint.c / jidctint.c: FIX(x) at CONST_BITS = 13
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

struct JpgImg {
  int n_src, n_dst;
  int slot;  // this image's planes in the workspace
};
struct JpgBatch {
  JpgImg im[kChunk];
};
struct JpgTabs {
  uint16_t q[2][64];  // luminance, chrominance; natural order
};
struct JpgCfg {
  int h, w;    // the canvas
  int ch, cw;  // the real chroma plane: ceil(h / 2) x ceil(w / 2)
  int ys, cs;  // bytes between the rows of the Y and of the chroma planes in the workspace: w and cw rounded up to 8
  unsigned pixels;
  unsigned long long img_bytes;  // Y, Cb, Cr of one image: ys * h + 2 * cs * ch, a multiple of 8
};

struct Ycc {
  int y, cb, cr;
};

// what a source float stands for: (int)v clamped to 0..255, NaN -> 0 (colorjitter.hip's read_u8)
__device__ __forceinline__ int read_u8(float v) { return v >= 0.0f ? (v <= 255.0f ? (int)v : 255) : 0; }

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jccolor.c rgb_ycc_convert on the pixel (y, x) of an image
__device__ __forceinline__ Ycc load_ycc(const float* s, size_t plane, int w, int y, int x) {
  const float* p = s + (size_t)y * w + x;
  const int r = read_u8(p[0]), g = read_u8(p[plane]), b = read_u8(p[2 * plane]);
  Ycc o;
  o.y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  o.cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  o.cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
  return o;
}

// one pass of jfdctint.c over d[0..8): the row pass scales up by PASS1_BITS = 2, the column pass takes it out again
template <bool kRowPass>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7];
  const int tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5];
  const int tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3;
  const int tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int n = kRowPass ? 11 : 15;
  d[0] = kRowPass ? (tmp10 + tmp11) << 2 : descale(tmp10 + tmp11, 2);
  d[4] = kRowPass ? (tmp10 - tmp11) << 2 : descale(tmp10 - tmp11, 2);
  const int e1 = (tmp12 + tmp13) * F_0_541;
  d[2] = descale(e1 + tmp13 * F_0_765, n);
  d[6] = descale(e1 + tmp12 * (-F_1_847), n);
  int z1 = tmp4 + tmp7, z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * F_1_175;
  const int o4 = tmp4 * F_0_298, o5 = tmp5 * F_2_053, o6 = tmp6 * F_3_072, o7 = tmp7 * F_1_501;
  z1 = z1 * (-F_0_899);
  z2 = z2 * (-F_2_562);
  z3 = z3 * (-F_1_961) + z5;
  z4 = z4 * (-F_0_390) + z5;
  d[7] = descale(o4 + z1 + z3, n);
  d[5] = descale(o5 + z2 + z4, n);
  d[3] = descale(o6 + z2 + z3, n);
  d[1] = descale(o7 + z1 + z4, n);
}

// one pass of jidctint.c over c[0..8), descaled by n bits: 11 for the column pass, 18 for the row pass
template <int n>
__device__ __forceinline__ void idct8(int (&c)[8]) {
  const int e1 = (c[2] + c[6]) * F_0_541;
  const int e2 = e1 + c[6] * (-F_1_847);
  const int e3 = e1 + c[2] * F_0_765;
  const int e0 = (c[0] + c[4]) << 13;
  const int e4 = (c[0] - c[4]) << 13;
  const int tmp10 = e0 + e3, tmp13 = e0 - e3;
  const int tmp11 = e4 + e2, tmp12 = e4 - e2;
  int tmp0 = c[7], tmp1 = c[5], tmp2 = c[3], tmp3 = c[1];
  int z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * F_1_175;
  tmp0 = tmp0 * F_0_298;
  tmp1 = tmp1 * F_2_053;
  tmp2 = tmp2 * F_3_072;
  tmp3 = tmp3 * F_1_501;
  z1 = z1 * (-F_0_899);
  z2 = z2 * (-F_2_562);
  z3 = z3 * (-F_1_961) + z5;
  z4 = z4 * (-F_0_390) + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  c[0] = descale(tmp10 + tmp3, n);
  c[7] = descale(tmp10 - tmp3, n);
  c[1] = descale(tmp11 + tmp2, n);
  c[6] = descale(tmp11 - tmp2, n);
  c[2] = descale(tmp12 + tmp1, n);
  c[5] = descale(tmp12 - tmp1, n);
  c[3] = descale(tmp13 + tmp0, n);
  c[4] = descale(tmp13 - tmp0, n);
}

// libjpeg's post-IDCT range-limit table as the function it is: sample_range_limit[128 + (x & 1023)].  For x in
// [-512, 511] this is x + 128 clamped to 0..255; beyond that the table wraps
__device__ __forceinline__ unsigned range_limit(int x) {
  const int i = x & 1023;
  return (unsigned)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

// grid (runs of kRun MCUs, MCU rows, images)
__global__ __launch_bounds__(kThreads) void jpeg_codec_kernel(const JpgBatch b, const JpgCfg c, const JpgTabs tabs,
                                                              const float* __restrict__ src,
                                                              unsigned char* __restrict__ planes) {
  __shared__ int blk[kBlocks * kBlkStride];  // Y blocks 0..15 (2 rows of 8), Cb 16..19, Cr 20..23
  __shared__ int qt[128];
  const JpgImg& d = b.im[blockIdx.z];
  const int t = threadIdx.x;
  if (t < 128) qt[t] = tabs.q[t >> 6][t & 63];

  {  // a thread takes one 2 x 2 cell of the run: four Y samples, one Cb, one Cr
    const int cx = t & 31, cy = t >> 5;
    const size_t plane = (size_t)c.pixels;
    const float* s = src + (size_t)d.n_src * 3 * plane;
    // the right edge: the last column of the full-resolution planes repeats out to the MCU width
    const int gx = (int)blockIdx.x * (16 * kRun) + 2 * cx;
    const int x0 = min(gx, c.w - 1), x1 = min(gx + 1, c.w - 1);
    // the bottom edge of Y: its last row repeats
    const int gy = (int)blockIdx.y * 16 + 2 * cy;
    const int y0 = min(gy, c.h - 1), y1 = min(gy + 1, c.h - 1);
    Ycc p00 = load_ycc(s, plane, c.w, y0, x0), p01 = load_ycc(s, plane, c.w, y0, x1);
    Ycc p10 = load_ycc(s, plane, c.w, y1, x0), p11 = load_ycc(s, plane, c.w, y1, x1);
    int* yb = blk + ((cy >> 2) * 8 + (cx >> 2)) * kBlkStride + ((2 * cy) & 7) * kRowStride + ((2 * cx) & 7);
    yb[0] = p00.y - 128;
    yb[1] = p01.y - 128;
    yb[kRowStride] = p10.y - 128;
    yb[kRowStride + 1] = p11.y - 128;
    // the bottom edge of chroma: the last full-resolution row repeats once if h is odd (y1 above), the cells are
    // averaged, then the chroma plane's own last row repeats - which is not the average of Y's repeated rows
    const int gcy = (int)blockIdx.y * 8 + cy;
    if (gcy >= c.ch) {
      const int r0 = 2 * (c.ch - 1), r1 = min(r0 + 1, c.h - 1);
      p00 = load_ycc(s, plane, c.w, r0, x0);
      p01 = load_ycc(s, plane, c.w, r0, x1);
      p10 = load_ycc(s, plane, c.w, r1, x0);
      p11 = load_ycc(s, plane, c.w, r1, x1);
    }
    const int bias = 1 + (cx & 1);  // h2v2_downsample: 1, 2, 1, 2 along a row (a run starts at an even chroma column)
    int* cb = blk + (16 + (cx >> 3)) * kBlkStride + cy * kRowStride + (cx & 7);
    cb[0] = ((p00.cb + p01.cb + p10.cb + p11.cb + bias) >> 2) - 128;
    cb[4 * kBlkStride] = ((p00.cr + p01.cr + p10.cr + p11.cr + bias) >> 2) - 128;
  }
  __syncthreads();

  const int bi = t >> 3, k = t & 7;  // block and row (or column) of a DCT thread
  int v[8];
  if (t < kDctThreads) {  // forward DCT, rows
    int* p = blk + bi * kBlkStride + k * kRowStride;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j];
    fdct8<true>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = v[j];
  }
  __syncthreads();
  if (t < kDctThreads) {  // forward DCT, columns; the quantiser and its inverse; inverse DCT, columns
    int* p = blk + bi * kBlkStride + k;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j * kRowStride];
    fdct8<false>(v);
    const int* q = qt + (bi >= 16 ? 64 : 0) + k;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // jcdctmgr.c: the divisor is Q * 8 (jfdctint leaves 8 times the DCT); plain division: exact quotients are the point
      const unsigned Q = (unsigned)q[j * 8], q8 = Q << 3;
      const unsigned a = ((unsigned)abs(v[j]) + (q8 >> 1)) / q8;
      const int deq = (int)(a * Q);
      v[j] = v[j] < 0 ? -deq : deq;
    }
    idct8<11>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j * kRowStride] = v[j];
  }
  __syncthreads();
  if (t < kDctThreads) {  // inverse DCT, rows; the range limit; 8 samples = one 8-byte store
    const int* p = blk + bi * kBlkStride + k * kRowStride;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j];
    idct8<18>(v);
    uint2 out;
    out.x = range_limit(v[0]) | range_limit(v[1]) << 8 | range_limit(v[2]) << 16 | range_limit(v[3]) << 24;
    out.y = range_limit(v[4]) | range_limit(v[5]) << 8 | range_limit(v[6]) << 16 | range_limit(v[7]) << 24;
    unsigned char* img = planes + (size_t)d.slot * c.img_bytes;
    // a block row is stored whole where it holds a real sample: x < ys (cs), the planes' rows being padded to 8
    if (bi < 16) {
      const int y = (int)blockIdx.y * 16 + (bi >> 3) * 8 + k, x = (int)blockIdx.x * (16 * kRun) + (bi & 7) * 8;
      if (y < c.h && x < c.w) *reinterpret_cast<uint2*>(img + (size_t)y * c.ys + x) = out;
    } else {
      const int comp = (bi - 16) >> 2;
      const int y = (int)blockIdx.y * 8 + k, x = (int)blockIdx.x * (8 * kRun) + ((bi - 16) & 3) * 8;
      unsigned char* cp = img + (size_t)c.ys * c.h + (size_t)comp * c.cs * c.ch;
      if (y < c.ch && x < c.cw) *reinterpret_cast<uint2*>(cp + (size_t)y * c.cs + x) = out;
    }
  }
}

// grid (256-pixel pieces, images): jdsample.c's h2v2_fancy_upsample (h2v2_upsample when the chroma plane is at most 2
// samples wide) on the real chroma plane, then jdcolor.c's ycc_rgb_convert
__global__ __launch_bounds__(kThreads) void jpeg_upsample_kernel(const JpgBatch b, const JpgCfg c,
                                                                 const unsigned char* __restrict__ planes,
                                                                 float* __restrict__ dst) {
  const JpgImg& d = b.im[blockIdx.y];
  const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (p >= c.pixels) return;
  const int y = (int)(p / (unsigned)c.w), x = (int)(p - (unsigned)y * (unsigned)c.w);
  const unsigned char* img = planes + (size_t)d.slot * c.img_bytes;
  const unsigned char* cbp = img + (size_t)c.ys * c.h;
  const unsigned char* crp = cbp + (size_t)c.cs * c.ch;
  const int Y = img[(size_t)y * c.ys + x];
  const int yn = y >> 1, xn = x >> 1;
  int cb, cr;
  if (c.cw <= 2) {  // box replication
    cb = cbp[(size_t)yn * c.cs + xn];
    cr = crp[(size_t)yn * c.cs + xn];
  } else {
    // the triangle filter: 3/4 of the nearer sample and 1/4 of the further one, vertically then horizontally; at an edge
    // of the real plane the missing neighbour is the sample itself
    const int yf = (y & 1) ? min(yn + 1, c.ch - 1) : max(yn - 1, 0);
    const int xf = (x & 1) ? min(xn + 1, c.cw - 1) : max(xn - 1, 0);
    const int bias = (x & 1) ? 7 : 8;
    const size_t nn = (size_t)yn * c.cs + xn, fn = (size_t)yf * c.cs + xn;
    const size_t nf = (size_t)yn * c.cs + xf, ff = (size_t)yf * c.cs + xf;
    cb = (3 * (3 * cbp[nn] + cbp[fn]) + (3 * cbp[nf] + cbp[ff]) + bias) >> 4;
    cr = (3 * (3 * crp[nn] + crp[fn]) + (3 * crp[nf] + crp[ff]) + bias) >> 4;
  }
  cb -= 128;
  cr -= 128;
  const int u[3] = {Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)};
  const size_t plane = (size_t)c.pixels;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int q = u[ch] < 0 ? 0 : (u[ch] > 255 ? 255 : u[ch]);
    dst[((size_t)d.n_dst * 3 + ch) * plane + p] = (float)q;
  }
}

int check_jpeg_cfg(const rtpose_jpeg_cfg* cfg) {
  if (!cfg) return fail(RTPOSE_E_INVAL, "jpeg: NULL cfg");
  if (cfg->struct_bytes != sizeof(rtpose_jpeg_cfg))
    return fail(RTPOSE_E_INVAL, "jpeg: cfg.struct_bytes is %u, this library's rtpose_jpeg_cfg has %zu", cfg->struct_bytes,
                sizeof(rtpose_jpeg_cfg));
  if (cfg->quality < 1 || cfg->quality > 100)
    return fail(RTPOSE_E_INVAL, "jpeg: cfg.quality %d outside [1,100]", cfg->quality);
  if (cfg->h < 1 || cfg->h > 65535 || cfg->w < 1 || cfg->w > 65535)
    return fail(RTPOSE_E_INVAL, "jpeg: canvas h %d x w %d outside [1,65535]", cfg->h, cfg->w);
  return 0;
}

JpgCfg geometry(const rtpose_jpeg_cfg* cfg) {
  JpgCfg c;
  c.h = cfg->h;
  c.w = cfg->w;
  c.ch = (cfg->h + 1) / 2;
  c.cw = (cfg->w + 1) / 2;
  c.ys = (cfg->w + 7) / 8 * 8;
  c.cs = (c.cw + 7) / 8 * 8;
  c.pixels = (unsigned)cfg->h * (unsigned)cfg->w;  // <= 65535^2 < 2^32
  c.img_bytes = (unsigned long long)c.ys * c.h + 2ull * c.cs * c.ch;
  return c;
}

// jpeg_set_quality(quality, force_baseline) over the tables of the JPEG specification's Annex K, natural order
JpgTabs tables(int quality) {
  static const uint8_t base[2][64] = {
      {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
       14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
      {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
       47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  JpgTabs t;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 64; ++i) {
      const int v = (base[k][i] * s + 50) / 100;
      t.q[k][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return t;
}

}  // namespace
}  // namespace rtpose

using namespace rtpose;

extern "C" {

size_t rtpose_jpeg_workspace_bytes(const rtpose_jpeg_cfg* cfg, int count) {
  if (count < 0 || check_jpeg_cfg(cfg)) return 0;
  const size_t bytes = (size_t)count * (size_t)geometry(cfg).img_bytes;
  return round_up(bytes < 1 ? 1 : bytes, 256);
}

int rtpose_jpeg_roundtrip_batch(const rtpose_jpeg_image* images, int count, const rtpose_jpeg_cfg* cfg, const float* src,
                                float* dst, void* workspace, size_t workspace_bytes, void* stream) {
  if (!images) return fail(RTPOSE_E_INVAL, "jpeg: NULL images");
  if (!src) return fail(RTPOSE_E_INVAL, "jpeg: NULL src");
  if (!dst) return fail(RTPOSE_E_INVAL, "jpeg: NULL dst");
  if (!workspace) return fail(RTPOSE_E_INVAL, "jpeg: NULL workspace");
  if (int rc = check_jpeg_cfg(cfg)) return rc;
  if (count < 0) return fail(RTPOSE_E_INVAL, "jpeg: count %d is negative", count);
  if (reinterpret_cast<uintptr_t>(workspace) & 7)
    return fail(RTPOSE_E_INVAL, "jpeg: workspace %p is not aligned to 8 bytes", workspace);
  {
    uint64_t seen[65536 / 64];
    memset(seen, 0, sizeof(seen));
    int lo_src = 65536, hi_src = -1, lo_dst = 65536, hi_dst = -1;
    for (int i = 0; i < count; ++i) {
      const rtpose_jpeg_image& d = images[i];
      if (d.n_src < 0 || d.n_src > 65535) return fail(RTPOSE_E_INVAL, "jpeg: image %d: n_src %d outside [0,65535]", i, d.n_src);
      if (d.n_dst < 0 || d.n_dst > 65535) return fail(RTPOSE_E_INVAL, "jpeg: image %d: n_dst %d outside [0,65535]", i, d.n_dst);
      if (seen[d.n_dst >> 6] >> (d.n_dst & 63) & 1)
        return fail(RTPOSE_E_INVAL, "jpeg: image %d: n_dst %d appears twice", i, d.n_dst);
      seen[d.n_dst >> 6] |= 1ull << (d.n_dst & 63);
      if (dst == src && d.n_dst != d.n_src)
        return fail(RTPOSE_E_INVAL, "jpeg: image %d: dst == src with n_dst %d != n_src %d (in place keeps the slot)", i,
                    d.n_dst, d.n_src);
      lo_src = d.n_src < lo_src ? d.n_src : lo_src;
      hi_src = d.n_src > hi_src ? d.n_src : hi_src;
      lo_dst = d.n_dst < lo_dst ? d.n_dst : lo_dst;
      hi_dst = d.n_dst > hi_dst ? d.n_dst : hi_dst;
    }
    if (dst != src && count > 0) {
      // two views of one allocation: the images written may not reach into the images read
      const uintptr_t image = (uintptr_t)3 * cfg->h * cfg->w * sizeof(float);
      const uintptr_t s0 = reinterpret_cast<uintptr_t>(src) + lo_src * image, s1 = reinterpret_cast<uintptr_t>(src) + (hi_src + 1) * image;
      const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst) + lo_dst * image, d1 = reinterpret_cast<uintptr_t>(dst) + (hi_dst + 1) * image;
      if (d0 < s1 && s0 < d1)
        return fail(RTPOSE_E_INVAL, "jpeg: dst images %d..%d overlap src images %d..%d in memory and dst != src (in place is "
                    "dst == src with n_dst == n_src)", lo_dst, hi_dst, lo_src, hi_src);
    }
  }
  const size_t need = rtpose_jpeg_workspace_bytes(cfg, count);
  if (workspace_bytes < need)
    return fail(RTPOSE_E_INVAL, "jpeg: workspace_bytes %zu below the %zu rtpose_jpeg_workspace_bytes reports", workspace_bytes,
                need);
  if (count == 0) return 0;
  static thread_local CheckedPtr c_src, c_dst, c_ws;
  const int dev = current_device();
  int rc = c_src.check(src, dev, "jpeg", "src");
  if (!rc) rc = c_dst.check(dst, dev, "jpeg", "dst");
  if (!rc) rc = c_ws.check(workspace, dev, "jpeg", "the workspace");
  if (rc) return rc;

  const JpgCfg c = geometry(cfg);
  const JpgTabs tabs = tables(cfg->quality);
  hipStream_t s = as_stream(stream);
  unsigned char* planes = static_cast<unsigned char*>(workspace);
  const int mcus_x = (c.w + 15) / 16, mcus_y = (c.h + 15) / 16;  // at most 4096 each
  const unsigned pieces = (unsigned)(((unsigned long long)c.pixels + kThreads - 1) / kThreads);
  // every codec launch before the first up-sample launch: all images are read before any is written
  for (int pass = 0; pass < 2; ++pass)
    for (int first = 0; first < count; first += kChunk) {  // the descriptors travel as kernel arguments
      JpgBatch b;
      memset(&b, 0, sizeof(b));
      const int n = count - first < kChunk ? count - first : kChunk;
      for (int i = 0; i < n; ++i) b.im[i] = JpgImg{images[first + i].n_src, images[first + i].n_dst, first + i};
      if (pass == 0)
        hipLaunchKernelGGL(jpeg_codec_kernel, dim3((mcus_x + kRun - 1) / kRun, mcus_y, n), dim3(kThreads), 0, s, b, c, tabs,
                           src, planes);
      else
        hipLaunchKernelGGL(jpeg_upsample_kernel, dim3(pieces, n), dim3(kThreads), 0, s, b, c, planes, dst);
      RTPOSE_HIP_CHECK(hipGetLastError());
    }
  return 0;
}

}  // extern "C"
