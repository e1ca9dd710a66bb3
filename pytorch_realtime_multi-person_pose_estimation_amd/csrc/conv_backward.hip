// Backward pass of the stride-1 "same" convs (k = 1, 3, 7): the weight gradient (+ bias gradient) from fp32 and from bf16
// layout slices, and the ReLU gradient.  The data gradient is rtpose_conv2d / rtpose_conv2d_bf16 on the flipped, transposed
// filter and has no kernel here (header section 2b).
//
//   dW[o][c][dy][dx] = sum over (n, y, x) of gy[n, y, x, o] * x[n, y + dy - k/2, x + dx - k/2, c]
//
// Per tap this is a GEMM with M = cout, N = cin and the valid pixels of the batch as its reduction dimension.
// Two launches, no atomics, no communication between workgroups:
//   1. a partial kernel, grid (M tiles * N tiles, taps, slabs).  The valid pixels p = (n * H + y) * W + x are cut into
//      slabs whose count and boundaries follow from the shape alone (wgrad_geometry).  A workgroup of four waves (2 x 2, each
//      TM x TN MFMA tiles of 32 x 32) walks its slab in chunks of pixels: one thread per pixel writes the chunk's element
//      offsets into LDS, every thread fetches its share of both tiles into registers while the MFMAs of the chunk before run,
//      and stores it to LDS afterwards.  Channels past cin / cout and pixels past the slab's end are staged as zero and never
//      read from memory.  Each workgroup writes its cout x cin partial tile of (slab, tap) into the caller's workspace,
//      [slab][tap][cout][cin]; the workgroups of N tile 0 and tap 0 also sum gy per channel, pixel by pixel in fp32, into
//      [slab][cout] behind it.
//   2. wgrad_reduce_kernel adds the slabs in slab order and writes dense OIHW dW (and dbias): overwritten, not accumulated.
// The same inputs therefore give the same bits on every run.
// The two partial kernels (wgrad_partial_kernel: fp32 operands; wgrad_bf16_partial_kernel: bf16 operands, the third kernel of
// a mixed-precision training step) share the geometry, the arguments, the workgroup's placement, the chunk-offset writer, the
// store of the partial tile and everything on the host (wgrad_launch); how the operands are staged and reach the lanes of
// their MFMA shares nothing and is written out in each.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "conv_desc.h"

namespace rtpose {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kChunkF32 = 32;       // pixels per LDS chunk: 16 MFMA steps of K = 2
constexpr int kChunkBf16 = 64;      // pixels per LDS chunk: 4 MFMA steps of K = 16
constexpr int kMinSlab = 512;       // pixels: no slab shorter than 16 / 8 chunks unless the whole batch is
constexpr int kTargetBlocks = 1024; // workgroups a launch aims for (4 per CU of an MI355X)
constexpr int kRowPad = 32;         // bf16: elements (64 bytes) behind a tile row, see the bank rule at the bf16 kernel

struct WgradGeom {
  int tm, tn;        // MFMA tiles per wave along M (cout) and N (cin): 1 or 2
  int mtiles, ntiles, taps;
  int slab;          // pixels per slab (a multiple of the chunk)
  int slabs;
  size_t tile_floats;  // taps * cout * cin
  size_t ws_floats;    // slabs * (tile_floats + cout), rounded up to 4
};

// shape only: nothing here looks at the device
WgradGeom wgrad_geometry(int chunk, int cin, int cout, int k, int N, int H, int W) {
  WgradGeom g;
  g.tm = cout > 64 ? 2 : 1;
  g.tn = cin > 64 ? 2 : 1;
  g.mtiles = ceil_div(cout, 64 * g.tm);
  g.ntiles = ceil_div(cin, 64 * g.tn);
  g.taps = k * k;
  const long P = (long)N * H * W;
  const long per_slab = (long)g.mtiles * g.ntiles * g.taps;
  long want = (kTargetBlocks + per_slab - 1) / per_slab;
  const long most = (P + kMinSlab - 1) / kMinSlab;
  if (want > most) want = most;
  if (want < 1) want = 1;
  g.slab = (int)(((P + want - 1) / want + chunk - 1) / chunk * chunk);
  g.slabs = (int)((P + g.slab - 1) / g.slab);
  g.tile_floats = (size_t)g.taps * cout * cin;
  g.ws_floats = round_up((size_t)g.slabs * (g.tile_floats + (size_t)cout), 4);
  return g;
}

bool shape_ok(int cin, int cout, int k, int N, int H, int W) {
  return cin >= 1 && cout >= 1 && (k == 1 || k == 3 || k == 7) && N >= 1 && H >= 1 && W >= 1 &&
         (long)N * H * W < (1L << 31) - kThreads && (long)k * k * cout * cin < (1L << 31) - kThreads;
}

// T: the operands' element, float or uint16_t (bf16)
template <class T>
struct WgradArgs {
  const T* x;
  const T* gy;
  float* ws;
  Lay lx, lgy;
  int cin, cout, k, H, W, P;  // P = N * H * W valid pixels
  int slab, ntiles;
  int want_bias;
  FastDiv d_w, d_h;
  size_t tile_floats;  // floats of one slab's [tap][cout][cin] partial
  size_t bias_base;    // float offset of the [slab][cout] bias partials
};

// ---- what the two partial kernels share --------------------------------------------------------------------------------------
// the workgroup's tile, tap and slab
struct WgradBlock {
  int mt, nt, tap, slab;
  long long tap_off;  // element offset of the tap's shifted pixel in x
  int p0, p1, chunks;
};

template <int CHUNK, class T>
__device__ __forceinline__ WgradBlock wgrad_block(const WgradArgs<T>& a) {
  WgradBlock b;
  b.mt = blockIdx.x / a.ntiles, b.nt = blockIdx.x - b.mt * a.ntiles;
  b.tap = blockIdx.y, b.slab = blockIdx.z;
  const int ky = b.tap / a.k, kx = b.tap - ky * a.k, half = a.k >> 1;
  b.tap_off = ((long long)(ky - half) * a.lx.ws + (kx - half)) * a.lx.cstride;
  b.p0 = b.slab * a.slab;
  b.p1 = min(b.p0 + a.slab, a.P);
  b.chunks = (b.p1 - b.p0 + CHUNK - 1) / CHUNK;
  return b;
}

// thread tid < CHUNK: the element offsets of pixel tid of chunk c in gy and in the tap-shifted x, -1 past the slab's end
template <int CHUNK, class T>
__device__ __forceinline__ void wgrad_offsets(const WgradArgs<T>& a, const WgradBlock& b, int c, int tid,
                                              long long (&offA)[2][CHUNK], long long (&offB)[2][CHUNK]) {
  if (tid < CHUNK) {
    const int p = b.p0 + c * CHUNK + tid;
    long long ga = -1, gb = -1;
    if (p < b.p1) {
      const int row = fast_div(p, a.d_w), xx = p - row * a.W;
      const int n = fast_div(row, a.d_h), yy = row - n * a.H;
      ga = (long long)lay_off(a.lgy, n, yy, xx);
      gb = (long long)lay_off(a.lx, n, yy, xx) + b.tap_off;
    }
    offA[c & 1][tid] = ga;
    offB[c & 1][tid] = gb;
  }
}

// the wave's TM x TN accumulators into the workspace's partial tile of (slab, tap), and the bias partial
// C / D map of the 32 x 32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
template <int TM, int TN, class T>
__device__ __forceinline__ void wgrad_store(const WgradArgs<T>& a, const WgradBlock& b, const f32x16 (&acc)[TM][TN], int tid,
                                            int wm, int wn, int l31, int lk, bool bias_block, float bsum) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  float* out = a.ws + (size_t)b.slab * a.tile_floats + (size_t)b.tap * a.cout * a.cin;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = b.nt * BN + wn + 32 * j + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = b.mt * BM + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (o < a.cout && c < a.cin) out[(size_t)o * a.cin + c] = acc[i][j][r];
      }
    }
  if (bias_block && tid < BM && b.mt * BM + tid < a.cout)
    a.ws[a.bias_base + (size_t)b.slab * a.cout + b.mt * BM + tid] = bsum;
}

// ---- fp32 operands ---------------------------------------------------------------------------------------------------------------
// fp32 operands, fp32 accumulate, v_mfma_f32_32x32x2_f32: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31],
// so with PIXEL-MAJOR LDS tiles the 32 lanes of a half-wave read 32 consecutive channels of one pixel, for gy (A) and for
// the tap-shifted x (B) alike: no bank conflict, no transposition while staging.  Chunks of 32 pixels.
template <int TM, int TN>
__global__ __launch_bounds__(kThreads) void wgrad_partial_kernel(const WgradArgs<float> a) {
  constexpr int kChunk = kChunkF32;
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int PA = kChunk * BM / kThreads, PB = kChunk * BN / kThreads;  // elements per thread and chunk
  constexpr int RA = kThreads / BM, RB = kThreads / BN;                    // pixel rows one pass of the block covers
  __shared__ float sA[kChunk * BM];
  __shared__ float sB[kChunk * BN];
  __shared__ long long offA[2][kChunk];
  __shared__ long long offB[2][kChunk];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WgradBlock b = wgrad_block<kChunk>(a);
  const bool bias_block = a.want_bias && b.nt == 0 && b.tap == 0;  // this workgroup also sums gy per channel

  // this thread's channel of each tile; a channel past the slice is staged as zero and never read from memory
  const int ca = tid & (BM - 1), cb = tid & (BN - 1);
  const int ra = tid / BM, rb = tid / BN;
  const int oa = b.mt * BM + ca, ob = b.nt * BN + cb;
  const bool va = oa < a.cout, vb = ob < a.cin;

  float ra_v[PA], rb_v[PB];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      const long long o = offA[c & 1][ra + i * RA];
      ra_v[i] = (va && o >= 0) ? a.gy[o + oa] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const long long o = offB[c & 1][rb + i * RB];
      rb_v[i] = (vb && o >= 0) ? a.x[o + ob] : 0.f;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bsum = 0.f;

  const int wm = (wave & 1) * 32 * TM, wn = (wave >> 1) * 32 * TN;
  const int l31 = lane & 31, lk = lane >> 5;

  wgrad_offsets(a, b, 0, tid, offA, offB);
  __syncthreads();
  fetch(0);
  for (int c = 0; c < b.chunks; ++c) {
#pragma unroll
    for (int i = 0; i < PA; ++i) sA[(ra + i * RA) * BM + ca] = ra_v[i];
#pragma unroll
    for (int i = 0; i < PB; ++i) sB[(rb + i * RB) * BN + cb] = rb_v[i];
    if (c + 1 < b.chunks) wgrad_offsets(a, b, c + 1, tid, offA, offB);
    __syncthreads();
    if (c + 1 < b.chunks) fetch(c + 1);  // in flight while the MFMAs below run
#pragma unroll
    for (int kk = 0; kk < kChunk / 2; ++kk) {
      const int px = 2 * kk + lk;
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = sA[px * BM + wm + 32 * i + l31];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = sB[px * BN + wn + 32 * j + l31];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (bias_block && tid < BM) {
      for (int px = 0; px < kChunk; ++px) bsum += sA[px * BM + tid];
    }
    __syncthreads();
  }

  wgrad_store<TM, TN>(a, b, acc, tid, wm, wn, l31, lk, bias_block, bsum);
}

// ---- bf16 operands ---------------------------------------------------------------------------------------------------------------
// bf16 operands, products exact in fp32, fp32 accumulation in v_mfma_f32_32x32x16_bf16.  Chunks of 64 pixels (4 MFMA steps of
// K = 16), fetched and staged in 16-byte pieces of 8 channels.
//
// Lane l of the 32x32x16 forms holds A[row l & 31][k = 8 (l >> 5) + j], j = 0 .. 7: EIGHT CONSECUTIVE PIXELS of one
// channel, while memory has the channels of one pixel side by side.  The tiles are staged as they lie in memory - rows =
// pixels, 16-byte loads and stores of 8 channels - and transposed by the LDS read itself: ds_read_b64_tr_b16 hands, per 16
// lanes, a block of 4 rows x 16 columns out column by column, so two reads (rows r .. r + 3 and r + 4 .. r + 7) are a lane's
// fragment.  Lane 4 q + p of a 16-lane group supplies the address of row q, columns 4 p .. 4 p + 3 of its block.
//   * every address is 8-byte aligned (row strides of 192 / 320 bytes, columns in fours);
//   * EXEC is all ones at every transposed read: the reads sit in the workgroup-uniform chunk loop, never under a lane-
//     dependent branch, and a workgroup is four whole waves.  Pixels past the slab's end, channel groups past the slice and
//     the channels of a group past the slice are ZEROS IN THE LDS TILE (a mask on the loaded 16 bytes), never a skipped read;
//   * banks: a 32-lane half reads 4 rows x 32 columns = 4 x 64 bytes.  With a row stride of 2 BM + 64 bytes (192 for a
//     64-channel tile, 320 for a 128-channel one: both 64 mod 128, and 4 consecutive rows start 0, 64, 128, 192 mod 256 in
//     some order) the four pieces tile the 256-byte bank row: conflict-free by the (a / 4) % 64 rule.  Unpadded rows of 128 /
//     256 bytes would be 2-way / 4-way.

// the 16 bytes of channels c0 .. c0 + 7 with the channels at and past `live` cleared: all ones, all zeros or a prefix
__device__ __forceinline__ u32x4 group_mask(int c0, int live) {
  u32x4 m;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    m[j] = (c0 + 2 * j < live ? 0x0000ffffu : 0u) | (c0 + 2 * j + 1 < live ? 0xffff0000u : 0u);
  return m;
}

// 4 rows x 16 columns of 16-bit elements per 16 lanes, handed out by columns (see above)
__device__ __forceinline__ i16x4 read_tr(const uint16_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)p);
}

// a lane's 8-pixel fragment: rows p .. p + 3 and p + 4 .. p + 7 of its block column
template <int STRIDE>
__device__ __forceinline__ bf16x8 fragment(const uint16_t* p) {
  const i16x4 lo = read_tr(p), hi = read_tr(p + 4 * STRIDE);
  return __builtin_bit_cast(bf16x8, (i16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int TM, int TN>
__global__ __launch_bounds__(kThreads) void wgrad_bf16_partial_kernel(const WgradArgs<uint16_t> a) {
  constexpr int kChunk = kChunkBf16;
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int SA = BM + kRowPad, SB = BN + kRowPad;    // LDS row strides, elements
  constexpr int GA = BM / 8, GB = BN / 8;                // 16-byte groups per tile row
  constexpr int RA = kThreads / GA, RB = kThreads / GB;  // pixel rows one pass of the block covers
  constexpr int PA = kChunk / RA, PB = kChunk / RB;      // 16-byte pieces per thread and chunk
  __shared__ __attribute__((aligned(16))) uint16_t sA[kChunk * SA];
  __shared__ __attribute__((aligned(16))) uint16_t sB[kChunk * SB];
  __shared__ long long offA[2][kChunk];
  __shared__ long long offB[2][kChunk];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WgradBlock b = wgrad_block<kChunk>(a);
  const bool bias_block = a.want_bias && b.nt == 0 && b.tap == 0;  // this workgroup also sums gy per channel

  // this thread's 8-channel group of each tile: a group past the slice is staged as zero and never read from memory, the
  // channels past the slice of the group that straddles its end are cleared after the load
  const int ga = tid % GA, gb = tid % GB;
  const int ra = tid / GA, rb = tid / GB;
  const int oa = b.mt * BM + 8 * ga, ob = b.nt * BN + 8 * gb;
  const bool va = oa < a.cout, vb = ob < a.cin;
  const u32x4 ma = group_mask(oa, a.cout), mb = group_mask(ob, a.cin);

  u32x4 ra_v[PA], rb_v[PB];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      const long long o = offA[c & 1][ra + i * RA];
      u32x4 v = {0u, 0u, 0u, 0u};
      if (va && o >= 0) v = *reinterpret_cast<const u32x4*>(a.gy + o + oa);
      ra_v[i] = v & ma;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      const long long o = offB[c & 1][rb + i * RB];
      u32x4 v = {0u, 0u, 0u, 0u};
      if (vb && o >= 0) v = *reinterpret_cast<const u32x4*>(a.x + o + ob);
      rb_v[i] = v & mb;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bsum = 0.f;

  const int wm = (wave & 1) * 32 * TM, wn = (wave >> 1) * 32 * TN;
  const int l31 = lane & 31, lk = lane >> 5;
  // the address this lane supplies to a transposed read of K step 0, MFMA tile 0: row 8 (l >> 5) + q, columns 16 (group & 1)
  // + 4 p of the wave's 32 columns, with q = (l & 15) >> 2 and p = l & 3
  const int trow = 8 * lk + ((lane & 15) >> 2), tcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const uint16_t* const fa = sA + trow * SA + wm + tcol;
  const uint16_t* const fb = sB + trow * SB + wn + tcol;

  wgrad_offsets(a, b, 0, tid, offA, offB);
  __syncthreads();
  fetch(0);
  for (int c = 0; c < b.chunks; ++c) {
#pragma unroll
    for (int i = 0; i < PA; ++i) *reinterpret_cast<u32x4*>(sA + (ra + i * RA) * SA + 8 * ga) = ra_v[i];
#pragma unroll
    for (int i = 0; i < PB; ++i) *reinterpret_cast<u32x4*>(sB + (rb + i * RB) * SB + 8 * gb) = rb_v[i];
    if (c + 1 < b.chunks) wgrad_offsets(a, b, c + 1, tid, offA, offB);
    __syncthreads();
    if (c + 1 < b.chunks) fetch(c + 1);  // in flight while the MFMAs below run
#pragma unroll
    for (int kk = 0; kk < kChunk / 16; ++kk) {
      bf16x8 av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = fragment<SA>(fa + 16 * kk * SA + 32 * i);
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = fragment<SB>(fb + 16 * kk * SB + 32 * j);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (bias_block && tid < BM) {
      for (int px = 0; px < kChunk; ++px) bsum += __uint_as_float((unsigned)sA[px * SA + tid] << 16);
    }
    __syncthreads();
  }

  wgrad_store<TM, TN>(a, b, acc, tid, wm, wn, l31, lk, bias_block, bsum);
}

// ---- the second launch of both -----------------------------------------------------------------------------------------------------
// thread i < taps * cout * cin: element (tap, o, c) of the partial tiles, summed in slab order and written at OIHW
// [o][c][tap]; the cout threads behind them do the same for the bias partials
__global__ __launch_bounds__(kThreads) void wgrad_reduce_kernel(const float* __restrict__ ws, size_t tile_floats,
                                                               size_t bias_base, int slabs, int cin, int cout, int taps,
                                                               float* __restrict__ dw, float* __restrict__ dbias) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < tile_floats) {
    float v = ws[i];
    for (int s = 1; s < slabs; ++s) v += ws[(size_t)s * tile_floats + i];
    const size_t per_tap = (size_t)cout * cin;
    const int tap = (int)(i / per_tap);
    const size_t oc = i - (size_t)tap * per_tap;
    dw[oc * taps + tap] = v;
  } else if (dbias && i < tile_floats + (size_t)cout) {
    const size_t o = i - tile_floats;
    float v = ws[bias_base + o];
    for (int s = 1; s < slabs; ++s) v += ws[bias_base + (size_t)s * cout + o];
    dbias[o] = v;
  }
}

// ---- host: one path for both entry points ---------------------------------------------------------------------------------------
// What an entry point is: its name in messages, its descriptor and operand element, its chunk, the exported function that
// reports its workspace, whether its operands are fetched in 16-byte pieces, and its partial kernel.
struct WgradF32 {
  using Desc = rtpose_wgrad_desc;
  using Elem = float;
  static constexpr const char* who = "conv2d_wgrad";
  static constexpr const char* reporter = "rtpose_conv2d_wgrad_workspace_floats";
  static constexpr int chunk = kChunkF32;
  static constexpr bool operands_aligned16 = false;
  template <int TM, int TN>
  static void launch(dim3 grid, hipStream_t s, const WgradArgs<float>& a) {
    hipLaunchKernelGGL((wgrad_partial_kernel<TM, TN>), grid, dim3(kThreads), 0, s, a);
  }
};

struct WgradBf16 {
  using Desc = rtpose_wgrad_bf16_desc;
  using Elem = uint16_t;
  static constexpr const char* who = "conv2d_wgrad_bf16";
  static constexpr const char* reporter = "rtpose_conv2d_wgrad_bf16_workspace_floats";
  static constexpr int chunk = kChunkBf16;
  static constexpr bool operands_aligned16 = true;  // the kernel's 16-byte loads: 8 bf16 elements
  template <int TM, int TN>
  static void launch(dim3 grid, hipStream_t s, const WgradArgs<uint16_t>& a) {
    hipLaunchKernelGGL((wgrad_bf16_partial_kernel<TM, TN>), grid, dim3(kThreads), 0, s, a);
  }
};

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// slabs and workspace floats of a shape, 0 where the shape is not supported
template <class E>
WgradGeom wgrad_query(int cin, int cout, int k, int N, int H, int W) {
  if (!shape_ok(cin, cout, k, N, H, W)) return WgradGeom{};
  return wgrad_geometry(E::chunk, cin, cout, k, N, H, W);
}

// every check in the order the entry points have always made them (a caller with two faults gets the same message), the
// arguments, the partial launch and the reduce launch
template <class E>
int wgrad_launch(const typename E::Desc* d, int N, int H, int W, void* stream) {
  const char* const who = E::who;
  if (!d) return fail(RTPOSE_E_INVAL, "%s: NULL descriptor", who);
  if (!d->x) return fail(RTPOSE_E_INVAL, "%s: NULL x", who);
  if (!d->gy) return fail(RTPOSE_E_INVAL, "%s: NULL gy", who);
  if (!d->dw) return fail(RTPOSE_E_INVAL, "%s: NULL dw", who);
  if (!d->workspace) return fail(RTPOSE_E_INVAL, "%s: NULL workspace", who);
  if (d->k != 1 && d->k != 3 && d->k != 7) return fail(RTPOSE_E_INVAL, "%s: k must be 1, 3 or 7", who);
  if (d->cin < 1 || d->cout < 1) return fail(RTPOSE_E_INVAL, "%s: cin and cout must be >= 1", who);
  if (N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "%s: empty tensor", who);
  if (!layout_sane(d->lx) || !layout_sane(d->lgy)) return fail(RTPOSE_E_INVAL, "%s: bad layout", who);
  if (!shape_ok(d->cin, d->cout, d->k, N, H, W)) return fail(RTPOSE_E_INVAL, "%s: tensor above the launch limit", who);
  if constexpr (E::operands_aligned16) {
    if (!aligned16(d->x) || !slice_aligned(d->lx, 8))
      return fail(RTPOSE_E_INVAL, "%s: input slice must be 16-byte aligned (base, choff and cstride in 8 bf16 elements)", who);
    if (!aligned16(d->gy) || !slice_aligned(d->lgy, 8))
      return fail(RTPOSE_E_INVAL, "%s: output-gradient slice must be 16-byte aligned (base, choff and cstride in 8 bf16 "
                                  "elements)", who);
  }
  if (!slice_inside(d->lx, d->cin)) return fail(RTPOSE_E_INVAL, "%s: input slice exceeds cstride", who);
  if (!slice_inside(d->lgy, d->cout)) return fail(RTPOSE_E_INVAL, "%s: output-gradient slice exceeds cstride", who);
  if (!gap_covers(d->lx, H, W, d->k / 2)) return fail(RTPOSE_E_INVAL, "%s: input layout gap smaller than the conv padding", who);
  if (!gap_covers(d->lgy, H, W, 0)) return fail(RTPOSE_E_INVAL, "%s: output-gradient layout smaller than the map", who);
  const WgradGeom g = wgrad_geometry(E::chunk, d->cin, d->cout, d->k, N, H, W);
  if (d->workspace_floats < g.ws_floats)
    return fail(RTPOSE_E_INVAL, "%s: workspace of %zu floats below the %zu %s reports", who, d->workspace_floats, g.ws_floats,
                E::reporter);
  if (!aligned16(d->dw) || !aligned16(d->workspace)) return fail(RTPOSE_E_INVAL, "%s: dw and workspace must be 16-byte aligned", who);
  if (g.slabs > 65535 || (long)g.mtiles * g.ntiles > 0x7fffffffL) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_x, c_gy, c_dw, c_ws, c_db;
  const int dev = current_device();
  int rc = c_x.check(d->x, dev, who, "x");
  if (!rc) rc = c_gy.check(d->gy, dev, who, "gy");
  if (!rc) rc = c_dw.check(d->dw, dev, who, "dw");
  if (!rc) rc = c_ws.check(d->workspace, dev, who, "workspace");
  if (!rc && d->dbias) rc = c_db.check(d->dbias, dev, who, "dbias");
  if (rc) return rc;

  WgradArgs<typename E::Elem> a;
  a.x = static_cast<const typename E::Elem*>(d->x);
  a.gy = static_cast<const typename E::Elem*>(d->gy);
  a.ws = d->workspace;
  a.lx = to_lay(&d->lx);
  a.lgy = to_lay(&d->lgy);
  a.cin = d->cin;
  a.cout = d->cout;
  a.k = d->k;
  a.H = H;
  a.W = W;
  a.P = N * H * W;
  a.slab = g.slab;
  a.ntiles = g.ntiles;
  a.want_bias = d->dbias ? 1 : 0;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  a.tile_floats = g.tile_floats;
  a.bias_base = (size_t)g.slabs * g.tile_floats;
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)(g.mtiles * g.ntiles), (unsigned)g.taps, (unsigned)g.slabs);
  if (g.tm == 2 && g.tn == 2)
    E::template launch<2, 2>(grid, s, a);
  else if (g.tm == 2)
    E::template launch<2, 1>(grid, s, a);
  else if (g.tn == 2)
    E::template launch<1, 2>(grid, s, a);
  else
    E::template launch<1, 1>(grid, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  const size_t items = g.tile_floats + (size_t)d->cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     (const float*)d->workspace, g.tile_floats, a.bias_base, g.slabs, d->cin, d->cout, g.taps, d->dw,
                     d->dbias);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

struct ReluGradArgs {
  const float* y;
  const uint32_t* gy;
  uint32_t* out;
  Lay ly, lgy, lout;
  int channels, H, W;
  size_t total;
  FastDiv d_c, d_w, d_h;
};

// one thread per (valid pixel, channel): the bits of gy where y > 0, else +0
__global__ __launch_bounds__(kThreads) void relu_grad_kernel(const ReluGradArgs a) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  const int e = (int)i;
  const int p = fast_div(e, a.d_c), c = e - p * a.channels;
  const int row = fast_div(p, a.d_w), xx = p - row * a.W;
  const int n = fast_div(row, a.d_h), yy = row - n * a.H;
  const float yv = a.y[lay_off(a.ly, n, yy, xx) + c];
  const uint32_t g = a.gy[lay_off(a.lgy, n, yy, xx) + c];
  a.out[lay_off(a.lout, n, yy, xx) + c] = yv > 0.f ? g : 0u;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_conv2d_wgrad_workspace_floats(int cin, int cout, int k, int N, int H, int W) {
  return wgrad_query<WgradF32>(cin, cout, k, N, H, W).ws_floats;
}

int rtpose_conv2d_wgrad_slabs(int cin, int cout, int k, int N, int H, int W) {
  return wgrad_query<WgradF32>(cin, cout, k, N, H, W).slabs;
}

int rtpose_conv2d_wgrad(const rtpose_wgrad_desc* d, int N, int H, int W, void* stream) {
  return wgrad_launch<WgradF32>(d, N, H, W, stream);
}

size_t rtpose_conv2d_wgrad_bf16_workspace_floats(int cin, int cout, int k, int N, int H, int W) {
  return wgrad_query<WgradBf16>(cin, cout, k, N, H, W).ws_floats;
}

int rtpose_conv2d_wgrad_bf16_slabs(int cin, int cout, int k, int N, int H, int W) {
  return wgrad_query<WgradBf16>(cin, cout, k, N, H, W).slabs;
}

int rtpose_conv2d_wgrad_bf16(const rtpose_wgrad_bf16_desc* d, int N, int H, int W, void* stream) {
  return wgrad_launch<WgradBf16>(d, N, H, W, stream);
}

int rtpose_relu_grad(const float* y, const rtpose_layout* ly, const float* gy, const rtpose_layout* lgy, float* out,
                     const rtpose_layout* lout, int channels, int N, int H, int W, void* stream) {
  if (!y || !gy || !out) return fail(RTPOSE_E_INVAL, "relu_grad: NULL buffer");
  if (!ly || !lgy || !lout) return fail(RTPOSE_E_INVAL, "relu_grad: NULL layout");
  if (channels < 1 || N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "relu_grad: empty tensor");
  if (!layout_sane(*ly) || !layout_sane(*lgy) || !layout_sane(*lout)) return fail(RTPOSE_E_INVAL, "relu_grad: bad layout");
  if (!slice_inside(*ly, channels) || !slice_inside(*lgy, channels) || !slice_inside(*lout, channels))
    return fail(RTPOSE_E_INVAL, "relu_grad: slice exceeds cstride");
  if (!gap_covers(*ly, H, W, 0) || !gap_covers(*lgy, H, W, 0) || !gap_covers(*lout, H, W, 0))
    return fail(RTPOSE_E_INVAL, "relu_grad: layout smaller than the map");
  const size_t total = (size_t)N * H * W * channels;
  if (total >= ((size_t)1 << 31)) return fail(RTPOSE_E_INVAL, "relu_grad: tensor above the launch limit");
  static thread_local CheckedPtr c_y, c_gy, c_out;
  const int dev = current_device();
  int rc = c_y.check(y, dev, "relu_grad", "y");
  if (!rc) rc = c_gy.check(gy, dev, "relu_grad", "gy");
  if (!rc) rc = c_out.check(out, dev, "relu_grad", "out");
  if (rc) return rc;
  ReluGradArgs a;
  a.y = y;
  a.gy = reinterpret_cast<const uint32_t*>(gy);
  a.out = reinterpret_cast<uint32_t*>(out);
  a.ly = to_lay(ly);
  a.lgy = to_lay(lgy);
  a.lout = to_lay(lout);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.total = total;
  a.d_c = make_fastdiv(channels);
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  hipLaunchKernelGGL(relu_grad_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
