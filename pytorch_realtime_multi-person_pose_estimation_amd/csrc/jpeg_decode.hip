// The device stage of the JPEG decoder (header section 4f): the quantised coefficients that csrc/jpeg_entropy.cpp read
// from baseline files -> dense uint8 [h][w][3] RGB images, in the bits of Pillow on libjpeg-turbo.
//
//   lib/datasets/datasets.py:171-172 (Image.open(f).convert('RGB') of CocoKeypoints.__getitem__); libjpeg's jddctmgr /
//   jidctint (JDCT_ISLOW), jdsample (h2v2, h2v1 and h1v2 fancy up-sampling, box replication on narrow planes), jdcolor
//
// Two launches per 32 images, which differ in size and sampling: jpeg_idct_kernel, grid (runs of 32 blocks, images) over
// all blocks of all components of an image, de-quantises, runs both passes of the inverse DCT through an int32 LDS tile
// and stores the range-limited samples into 8-bit planes in the caller's workspace; jpeg_upsample_kernel, grid (runs of
// 1024 pixels, images), reads Y directly and chroma through the mode's filter - which reaches across block borders: hence
// the planes between the launches -, converts to RGB and stores 12 bytes per thread.  Integer arithmetic only: products
// of a coefficient and its quantiser entry lie inside int16 (the host stage refuses a file where one does not), so no
// int32 sum of the passes can overflow.  idct8, the range limit and the colour expression are those of
// jpeg_roundtrip.hip, which keeps its own copies: its object file stays what it was.
//
// Built like jpeg_roundtrip.hip without the vectorisers (csrc/Makefile): this is meant for a loader stream beside a forward.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "common.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;           // image descriptors per launch, passed by value
constexpr int kBlocksPerGroup = 32;  // 8 x 8 blocks a workgroup takes: eight threads each
constexpr int kRowStride = 9;        // ints between the rows of an 8 x 8 block in LDS: the column pass walks 8 banks apart
constexpr int kBlkStride = 8 * kRowStride;
constexpr int kRunPixels = 4;        // pixels per thread of the up-sample pass
constexpr int kMaxSide = 16384;

// jidctint.c: FIX(x) at CONST_BITS = 13
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

struct DecImg {
  int w, h, mode, comps;
  int bx0, bxc;  // blocks in a row of the Y and of a chroma block grid
  int n0, nc;    // blocks of Y and of one chroma component
  int cw, ch;    // the real chroma plane
  int ys, cs;    // bytes between the rows of the Y and of the chroma planes in the workspace: w and cw rounded up to 8
  unsigned long long coef, qtab;  // words into the coefficient buffer
  unsigned long long planes;      // bytes into the workspace: Y (ys * h), then Cb and Cr (cs * ch each)
  unsigned char* dst;
};
struct DecBatch {
  DecImg im[kChunk];
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

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

// libjpeg's post-IDCT range-limit table as the function it is: sample_range_limit[128 + (x & 1023)]
__device__ __forceinline__ unsigned range_limit(int x) {
  const int i = x & 1023;
  return (unsigned)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

// grid (runs of kBlocksPerGroup blocks, images); the blocks of Y, Cb and Cr follow each other in the coefficient buffer,
// so the flat block index addresses it directly
__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const DecBatch b, const int16_t* __restrict__ coef,
                                                             unsigned char* __restrict__ planes) {
  __shared__ int blk[kBlocksPerGroup * kBlkStride];
  const DecImg& d = b.im[blockIdx.y];
  const int t = threadIdx.x;
  const int bi = t >> 3, k = t & 7;  // block within the group; row, then column, then row of the block
  const int g = (int)blockIdx.x * kBlocksPerGroup + bi;
  const int total = d.n0 + (d.comps == 3 ? 2 * d.nc : 0);
  const bool live = g < total;  // the same for the eight threads of a block
  int comp = 0, local = g;
  if (live && g >= d.n0) {
    comp = g - d.n0 >= d.nc ? 2 : 1;
    local = g - d.n0 - (comp - 1) * d.nc;
  }
  int* tile = blk + bi * kBlkStride;
  int v[8];
  if (live) {  // one 16-byte row of coefficients times one 16-byte row of the component's table
    const uint4 c = *reinterpret_cast<const uint4*>(coef + d.coef + (size_t)g * 64 + k * 8);
    const uint4 q = *reinterpret_cast<const uint4*>(coef + d.qtab + comp * 64 + k * 8);
    const unsigned cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (int)(short)(cw[j] & 0xffffu) * (int)(qw[j] & 0xffffu);
      v[2 * j + 1] = ((int)cw[j] >> 16) * (int)(qw[j] >> 16);
    }
    int* p = tile + k * kRowStride;
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = v[j];
  }
  __syncthreads();
  if (live) {  // inverse DCT, columns
    int* p = tile + k;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j * kRowStride];
    idct8<11>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j * kRowStride] = v[j];
  }
  __syncthreads();
  if (live) {  // inverse DCT, rows; the range limit; 8 samples = one 8-byte store
    const int* p = tile + k * kRowStride;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j];
    idct8<18>(v);
    uint2 out;
    out.x = range_limit(v[0]) | range_limit(v[1]) << 8 | range_limit(v[2]) << 16 | range_limit(v[3]) << 24;
    out.y = range_limit(v[4]) | range_limit(v[5]) << 8 | range_limit(v[6]) << 16 | range_limit(v[7]) << 24;
    const int per_row = comp ? d.bxc : d.bx0;
    const int by = local / per_row, bxi = local - by * per_row;
    const int y = by * 8 + k, x = bxi * 8;
    const int rows = comp ? d.ch : d.h, cols = comp ? d.cw : d.w, stride = comp ? d.cs : d.ys;
    unsigned char* plane = planes + d.planes;
    if (comp) plane += (size_t)d.ys * d.h + (size_t)(comp - 1) * d.cs * d.ch;
    // a block row is stored whole where it holds a real sample: x < stride, the planes' rows being padded to 8
    if (y < rows && x < cols) *reinterpret_cast<uint2*>(plane + (size_t)y * stride + x) = out;
  }
}

// the chroma sample of output pixel (y, x) by the mode's rule, on the real plane c of d.ch rows of d.cw samples; a
// neighbour outside it is the sample itself
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ c, const DecImg& d, int y, int x) {
  const unsigned cs = (unsigned)d.cs;  // a plane has at most 16384 x 16384 bytes: 32-bit offsets
  switch (d.mode) {
    case RTPOSE_JPEG_420: {
      const int yn = y >> 1, xn = x >> 1;
      if (d.cw <= 2) return c[yn * cs + xn];  // h2v2_upsample: box replication
      const int yf = (y & 1) ? min(yn + 1, d.ch - 1) : max(yn - 1, 0);
      const int xf = (x & 1) ? min(xn + 1, d.cw - 1) : max(xn - 1, 0);
      const int bias = (x & 1) ? 7 : 8;
      return (3 * (3 * c[yn * cs + xn] + c[yf * cs + xn]) + (3 * c[yn * cs + xf] + c[yf * cs + xf]) + bias) >> 4;
    }
    case RTPOSE_JPEG_422: {
      const int xn = x >> 1;
      if (d.cw <= 2) return c[y * cs + xn];  // h2v1_upsample
      const int xf = (x & 1) ? min(xn + 1, d.cw - 1) : max(xn - 1, 0);
      return (3 * c[y * cs + xn] + c[y * cs + xf] + ((x & 1) ? 2 : 1)) >> 2;
    }
    case RTPOSE_JPEG_440: {
      const int yn = y >> 1;
      const int yf = (y & 1) ? min(yn + 1, d.ch - 1) : max(yn - 1, 0);
      return (3 * c[yn * cs + x] + c[yf * cs + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    default:
      return c[y * cs + x];  // 4:4:4
  }
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// grid (runs of kThreads * kRunPixels pixels, images): a thread takes kRunPixels consecutive pixels of the dense image
__global__ __launch_bounds__(kThreads) void jpeg_upsample_kernel(const DecBatch b, const unsigned char* __restrict__ planes) {
  const DecImg& d = b.im[blockIdx.y];
  const unsigned pixels = (unsigned)d.w * (unsigned)d.h;  // <= 2^28
  const unsigned p0 = (blockIdx.x * (unsigned)kThreads + threadIdx.x) * (unsigned)kRunPixels;
  if (p0 >= pixels) return;
  const unsigned char* yp = planes + d.planes;
  const unsigned char* cbp = yp + (size_t)d.ys * d.h;
  const unsigned char* crp = cbp + (size_t)d.cs * d.ch;
  int y = (int)(p0 / (unsigned)d.w), x = (int)(p0 - (unsigned)y * (unsigned)d.w);
  const int n = pixels - p0 < (unsigned)kRunPixels ? (int)(pixels - p0) : kRunPixels;
  unsigned u[3 * kRunPixels];
#pragma unroll
  for (int j = 0; j < kRunPixels; ++j) {
    unsigned r = 0, g = 0, bl = 0;
    if (j < n) {
      const int Y = yp[(unsigned)y * (unsigned)d.ys + (unsigned)x];
      if (d.comps == 1) {
        r = g = bl = (unsigned)Y;
      } else {
        const int cb = chroma_at(cbp, d, y, x) - 128, cr = chroma_at(crp, d, y, x) - 128;
        r = clamp255(Y + ((91881 * cr + 32768) >> 16));
        g = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        bl = clamp255(Y + ((116130 * cb + 32768) >> 16));
      }
      if (++x == d.w) {
        x = 0;
        ++y;
      }
    }
    u[3 * j] = r;
    u[3 * j + 1] = g;
    u[3 * j + 2] = bl;
  }
  unsigned char* o = d.dst + (size_t)p0 * 3;  // 12 bytes per run and a 4-byte aligned image: dword stores
  if (n == kRunPixels) {
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int j = 0; j < 3; ++j) o4[j] = u[4 * j] | u[4 * j + 1] << 8 | u[4 * j + 2] << 16 | u[4 * j + 3] << 24;
  } else {  // the last run of an image whose pixel count is no multiple of 4
#pragma unroll
    for (int j = 0; j < 3 * (kRunPixels - 1); ++j)
      if (j < 3 * n) o[j] = (unsigned char)u[j];
  }
}

// every grid, count and plane size of an image from its width, height and mode alone
struct Geometry {
  DecImg d;
  unsigned long long coef_words, plane_bytes;
};

int geometry(const rtpose_jpeg_decode_image& im, int i, Geometry* out) {
  if (im.width < 1 || im.width > kMaxSide || im.height < 1 || im.height > kMaxSide)
    return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: width %d x height %d outside [1,%d]", i, im.width, im.height, kMaxSide);
  int hs, vs, comps = 3;
  switch (im.mode) {
    case RTPOSE_JPEG_GRAY: hs = 1, vs = 1, comps = 1; break;
    case RTPOSE_JPEG_444: hs = 1, vs = 1; break;
    case RTPOSE_JPEG_422: hs = 2, vs = 1; break;
    case RTPOSE_JPEG_420: hs = 2, vs = 2; break;
    case RTPOSE_JPEG_440: hs = 1, vs = 2; break;
    default: return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: unknown mode %d", i, im.mode);
  }
  if (im.reserved != 0) return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: reserved is %d, not 0", i, im.reserved);
  DecImg& d = out->d;
  memset(&d, 0, sizeof(d));
  d.w = im.width;
  d.h = im.height;
  d.mode = im.mode;
  d.comps = comps;
  const int mcus_x = (d.w + 8 * hs - 1) / (8 * hs), mcus_y = (d.h + 8 * vs - 1) / (8 * vs);  // at most 2048 each
  d.bx0 = mcus_x * hs;
  d.bxc = mcus_x;
  d.n0 = d.bx0 * (mcus_y * vs);
  d.nc = mcus_x * mcus_y;
  d.cw = (d.w + hs - 1) / hs;
  d.ch = (d.h + vs - 1) / vs;
  d.ys = (d.w + 7) / 8 * 8;
  d.cs = (d.cw + 7) / 8 * 8;
  out->coef_words = 64ull * ((unsigned long long)d.n0 + (comps == 3 ? 2ull * d.nc : 0ull));
  out->plane_bytes = (unsigned long long)d.ys * d.h + (comps == 3 ? 2ull * d.cs * d.ch : 0ull);  // a multiple of 8
  return 0;
}

}  // namespace
}  // namespace rtpose

using namespace rtpose;

extern "C" {

size_t rtpose_jpeg_decode_workspace_bytes(const rtpose_jpeg_decode_image* images, int count) {
  if (count < 0 || (count > 0 && !images)) return 0;
  unsigned long long bytes = 0;
  for (int i = 0; i < count; ++i) {
    Geometry g;
    if (geometry(images[i], i, &g)) return 0;
    bytes += g.plane_bytes;
  }
  return round_up(bytes < 1 ? 1 : (size_t)bytes, 256);
}

int rtpose_jpeg_decode_batch(const rtpose_jpeg_decode_image* images, int count, const int16_t* coef, size_t coef_words,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!images) return fail(RTPOSE_E_INVAL, "jpeg decode: NULL images");
  if (!coef) return fail(RTPOSE_E_INVAL, "jpeg decode: NULL coef");
  if (!workspace) return fail(RTPOSE_E_INVAL, "jpeg decode: NULL workspace");
  if (count < 0) return fail(RTPOSE_E_INVAL, "jpeg decode: count %d is negative", count);
  if (reinterpret_cast<uintptr_t>(coef) & 15) return fail(RTPOSE_E_INVAL, "jpeg decode: coef %p is not aligned to 16 bytes", (const void*)coef);
  if (reinterpret_cast<uintptr_t>(workspace) & 7)
    return fail(RTPOSE_E_INVAL, "jpeg decode: workspace %p is not aligned to 8 bytes", workspace);
  std::vector<DecImg> descs((size_t)count);
  std::vector<std::pair<uintptr_t, uintptr_t>> spans((size_t)count);
  unsigned long long planes = 0;
  for (int i = 0; i < count; ++i) {
    const rtpose_jpeg_decode_image& im = images[i];
    Geometry g;
    if (int rc = geometry(im, i, &g)) return rc;
    if (!im.dst) return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: NULL dst", i);
    if (reinterpret_cast<uintptr_t>(im.dst) & 3)
      return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: dst %p is not aligned to 4 bytes", i, im.dst);
    if ((im.coef_offset & 7) || im.coef_offset > coef_words || g.coef_words > coef_words - im.coef_offset)
      return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: coef_offset %llu (a multiple of 8?) + its %llu coefficients beyond "
                  "coef_words %zu", i, (unsigned long long)im.coef_offset, g.coef_words, coef_words);
    if ((im.qtab_offset & 7) || im.qtab_offset > coef_words || 192 > coef_words - im.qtab_offset)
      return fail(RTPOSE_E_INVAL, "jpeg decode: image %d: qtab_offset %llu (a multiple of 8?) + 192 beyond coef_words %zu", i,
                  (unsigned long long)im.qtab_offset, coef_words);
    g.d.coef = im.coef_offset;
    g.d.qtab = im.qtab_offset;
    g.d.planes = planes;
    g.d.dst = static_cast<unsigned char*>(im.dst);
    planes += g.plane_bytes;
    descs[(size_t)i] = g.d;
    const uintptr_t begin = reinterpret_cast<uintptr_t>(im.dst);
    spans[(size_t)i] = {begin, begin + (uintptr_t)3 * (uintptr_t)im.width * (uintptr_t)im.height};
  }
  std::sort(spans.begin(), spans.end());
  for (int i = 1; i < count; ++i)
    if (spans[(size_t)i].first < spans[(size_t)i - 1].second)
      return fail(RTPOSE_E_INVAL, "jpeg decode: two destinations overlap in memory (%p and %p)", (void*)spans[(size_t)i - 1].first,
                  (void*)spans[(size_t)i].first);
  const size_t need = round_up(planes < 1 ? 1 : (size_t)planes, 256);
  if (workspace_bytes < need)
    return fail(RTPOSE_E_INVAL, "jpeg decode: workspace_bytes %zu below the %zu rtpose_jpeg_decode_workspace_bytes reports",
                workspace_bytes, need);
  if (count == 0) return 0;
  static thread_local CheckedPtr c_coef, c_ws, c_dst;
  const int dev = current_device();
  int rc = c_coef.check(coef, dev, "jpeg decode", "coef");
  if (!rc) rc = c_ws.check(workspace, dev, "jpeg decode", "the workspace");
  for (int i = 0; i < count && !rc; ++i) rc = c_dst.check(descs[(size_t)i].dst, dev, "jpeg decode", "a destination");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  // every IDCT launch before the first up-sample launch: the filters read across block borders
  for (int pass = 0; pass < 2; ++pass)
    for (int first = 0; first < count; first += kChunk) {  // the descriptors travel as kernel arguments
      DecBatch b;
      memset(&b, 0, sizeof(b));
      const int n = count - first < kChunk ? count - first : kChunk;
      unsigned groups = 1, runs = 1;
      for (int i = 0; i < n; ++i) {
        const DecImg& d = b.im[i] = descs[(size_t)(first + i)];
        const unsigned blocks = (unsigned)d.n0 + (d.comps == 3 ? 2u * (unsigned)d.nc : 0u);
        const unsigned pixels = (unsigned)d.w * (unsigned)d.h;
        groups = std::max(groups, (blocks + kBlocksPerGroup - 1) / kBlocksPerGroup);
        runs = std::max(runs, (pixels + kThreads * kRunPixels - 1) / (kThreads * kRunPixels));
      }
      if (pass == 0)
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(groups, n), dim3(kThreads), 0, s, b, coef, ws);
      else
        hipLaunchKernelGGL(jpeg_upsample_kernel, dim3(runs, n), dim3(kThreads), 0, s, b, ws);
      RTPOSE_HIP_CHECK(hipGetLastError());
    }
  return 0;
}

}  // extern "C"
