// Backward pass of the stride-1 "same" convs (k = 1, 3, 7): the weight gradient (+ bias gradient) and the ReLU gradient.
// The data gradient is rtpose_conv2d on the flipped, transposed filter and has no kernel here (header section 2b).
//
//   dW[o][c][dy][dx] = sum over (n, y, x) of gy[n, y, x, o] * x[n, y + dy - k/2, x + dx - k/2, c]
//
// Per tap this is a GEMM with M = cout, N = cin and the valid pixels of the batch as its reduction dimension.  fp32
// operands, fp32 accumulate, v_mfma_f32_32x32x2_f32: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31],
// so with PIXEL-MAJOR LDS tiles the 32 lanes of a half-wave read 32 consecutive channels of one pixel, for gy (A) and for
// the tap-shifted x (B) alike: no bank conflict, no transposition while staging.
//
// Two launches, no atomics, no communication between workgroups:
//   1. wgrad_partial_kernel, grid (M tiles * N tiles, taps, slabs).  The valid pixels p = (n * H + y) * W + x are cut into
//      slabs whose count and boundaries follow from the shape alone (wgrad_geometry).  A workgroup of four waves (2 x 2, each
//      TM x TN MFMA tiles) walks its slab in chunks of 32 pixels: 32 threads write the chunk's element offsets into LDS,
//      every thread fetches its share of both tiles into registers while the MFMAs of the chunk before run, and stores it to
//      LDS afterwards.  Channels past cin / cout and pixels past the slab's end are staged as zero and never read from memory.
//      Each workgroup writes its cout x cin partial tile of (slab, tap) into the caller's workspace, [slab][tap][cout][cin];
//      the workgroups of N tile 0 and tap 0 also sum gy per channel, pixel by pixel, into [slab][cout] behind it.
//   2. wgrad_reduce_kernel adds the slabs in slab order and writes dense OIHW dW (and dbias): overwritten, not accumulated.
// The same inputs therefore give the same bits on every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "conv_desc.h"

namespace rtpose {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kChunk = 32;          // pixels per LDS chunk: 16 MFMA steps of K = 2
constexpr int kMinSlab = 512;       // pixels: no slab shorter than 16 chunks unless the whole batch is
constexpr int kTargetBlocks = 1024; // workgroups a launch aims for (4 per CU of an MI355X)

struct WgradGeom {
  int tm, tn;        // MFMA tiles per wave along M (cout) and N (cin): 1 or 2
  int mtiles, ntiles, taps;
  int slab;          // pixels per slab (a multiple of kChunk)
  int slabs;
  size_t tile_floats;  // taps * cout * cin
  size_t ws_floats;    // slabs * (tile_floats + cout), rounded up to 4
};

// shape only: nothing here looks at the device
WgradGeom wgrad_geometry(int cin, int cout, int k, int N, int H, int W) {
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
  g.slab = (int)(((P + want - 1) / want + kChunk - 1) / kChunk * kChunk);
  g.slabs = (int)((P + g.slab - 1) / g.slab);
  g.tile_floats = (size_t)g.taps * cout * cin;
  g.ws_floats = round_up((size_t)g.slabs * (g.tile_floats + (size_t)cout), 4);
  return g;
}

struct WgradArgs {
  const float* x;
  const float* gy;
  float* ws;
  Lay lx, lgy;
  int cin, cout, k, H, W, P;  // P = N * H * W valid pixels
  int slab, ntiles;
  int want_bias;
  FastDiv d_w, d_h;
  size_t tile_floats;  // floats of one slab's [tap][cout][cin] partial
  size_t bias_base;    // float offset of the [slab][cout] bias partials
};

template <int TM, int TN>
__global__ __launch_bounds__(kThreads) void wgrad_partial_kernel(const WgradArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int PA = kChunk * BM / kThreads, PB = kChunk * BN / kThreads;  // elements per thread and chunk
  constexpr int RA = kThreads / BM, RB = kThreads / BN;                    // pixel rows one pass of the block covers
  __shared__ float sA[kChunk * BM];
  __shared__ float sB[kChunk * BN];
  __shared__ long long offA[2][kChunk];
  __shared__ long long offB[2][kChunk];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mt = blockIdx.x / a.ntiles, nt = blockIdx.x - mt * a.ntiles;
  const int tap = blockIdx.y, slab = blockIdx.z;
  const int ky = tap / a.k, kx = tap - ky * a.k, half = a.k >> 1;
  const long long tap_off = ((long long)(ky - half) * a.lx.ws + (kx - half)) * a.lx.cstride;
  const int p0 = slab * a.slab;
  const int p1 = min(p0 + a.slab, a.P);
  const int chunks = (p1 - p0 + kChunk - 1) / kChunk;
  const bool bias_block = a.want_bias && nt == 0 && tap == 0;

  // this thread's channel of each tile; a channel past the slice is staged as zero and never read from memory
  const int ca = tid & (BM - 1), cb = tid & (BN - 1);
  const int ra = tid / BM, rb = tid / BN;
  const int oa = mt * BM + ca, ob = nt * BN + cb;
  const bool va = oa < a.cout, vb = ob < a.cin;

  auto offsets = [&](int c) {
    if (tid < kChunk) {
      const int p = p0 + c * kChunk + tid;
      long long ga = -1, gb = -1;
      if (p < p1) {
        const int row = fast_div(p, a.d_w), xx = p - row * a.W;
        const int n = fast_div(row, a.d_h), yy = row - n * a.H;
        ga = (long long)lay_off(a.lgy, n, yy, xx);
        gb = (long long)lay_off(a.lx, n, yy, xx) + tap_off;
      }
      offA[c & 1][tid] = ga;
      offB[c & 1][tid] = gb;
    }
  };
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

  offsets(0);
  __syncthreads();
  fetch(0);
  for (int c = 0; c < chunks; ++c) {
#pragma unroll
    for (int i = 0; i < PA; ++i) sA[(ra + i * RA) * BM + ca] = ra_v[i];
#pragma unroll
    for (int i = 0; i < PB; ++i) sB[(rb + i * RB) * BN + cb] = rb_v[i];
    if (c + 1 < chunks) offsets(c + 1);
    __syncthreads();
    if (c + 1 < chunks) fetch(c + 1);  // in flight while the MFMAs below run
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

  // C / D map of the 32 x 32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  float* out = a.ws + (size_t)slab * a.tile_floats + (size_t)tap * a.cout * a.cin;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int c = nt * BN + wn + 32 * j + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = mt * BM + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (o < a.cout && c < a.cin) out[(size_t)o * a.cin + c] = acc[i][j][r];
      }
    }
  if (bias_block && tid < BM && mt * BM + tid < a.cout) a.ws[a.bias_base + (size_t)slab * a.cout + mt * BM + tid] = bsum;
}

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

bool shape_ok(int cin, int cout, int k, int N, int H, int W) {
  return cin >= 1 && cout >= 1 && (k == 1 || k == 3 || k == 7) && N >= 1 && H >= 1 && W >= 1 &&
         (long)N * H * W < (1L << 31) - kThreads && (long)k * k * cout * cin < (1L << 31) - kThreads;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_conv2d_wgrad_workspace_floats(int cin, int cout, int k, int N, int H, int W) {
  if (!shape_ok(cin, cout, k, N, H, W)) return 0;
  return wgrad_geometry(cin, cout, k, N, H, W).ws_floats;
}

int rtpose_conv2d_wgrad_slabs(int cin, int cout, int k, int N, int H, int W) {
  if (!shape_ok(cin, cout, k, N, H, W)) return 0;
  return wgrad_geometry(cin, cout, k, N, H, W).slabs;
}

int rtpose_conv2d_wgrad(const rtpose_wgrad_desc* d, int N, int H, int W, void* stream) {
  if (!d) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: NULL descriptor");
  if (!d->x) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: NULL x");
  if (!d->gy) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: NULL gy");
  if (!d->dw) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: NULL dw");
  if (!d->workspace) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: NULL workspace");
  if (d->k != 1 && d->k != 3 && d->k != 7) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: k must be 1, 3 or 7");
  if (d->cin < 1 || d->cout < 1) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: cin and cout must be >= 1");
  if (N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: empty tensor");
  if (!layout_sane(d->lx) || !layout_sane(d->lgy)) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: bad layout");
  if (!shape_ok(d->cin, d->cout, d->k, N, H, W)) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: tensor above the launch limit");
  if (!slice_inside(d->lx, d->cin)) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: input slice exceeds cstride");
  if (!slice_inside(d->lgy, d->cout)) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: output-gradient slice exceeds cstride");
  if (!gap_covers(d->lx, H, W, d->k / 2))
    return fail(RTPOSE_E_INVAL, "conv2d_wgrad: input layout gap smaller than the conv padding");
  if (!gap_covers(d->lgy, H, W, 0)) return fail(RTPOSE_E_INVAL, "conv2d_wgrad: output-gradient layout smaller than the map");
  const WgradGeom g = wgrad_geometry(d->cin, d->cout, d->k, N, H, W);
  if (d->workspace_floats < g.ws_floats)
    return fail(RTPOSE_E_INVAL, "conv2d_wgrad: workspace of %zu floats below the %zu rtpose_conv2d_wgrad_workspace_floats reports",
                d->workspace_floats, g.ws_floats);
  if ((reinterpret_cast<uintptr_t>(d->dw) | reinterpret_cast<uintptr_t>(d->workspace)) % 16)
    return fail(RTPOSE_E_INVAL, "conv2d_wgrad: dw and workspace must be 16-byte aligned");
  if (g.slabs > 65535 || (long)g.mtiles * g.ntiles > 0x7fffffffL)
    return fail(RTPOSE_E_INVAL, "conv2d_wgrad: grid too large");

  static thread_local CheckedPtr c_x, c_gy, c_dw, c_ws, c_db;
  const int dev = current_device();
  int rc = c_x.check(d->x, dev, "conv2d_wgrad", "x");
  if (!rc) rc = c_gy.check(d->gy, dev, "conv2d_wgrad", "gy");
  if (!rc) rc = c_dw.check(d->dw, dev, "conv2d_wgrad", "dw");
  if (!rc) rc = c_ws.check(d->workspace, dev, "conv2d_wgrad", "workspace");
  if (!rc && d->dbias) rc = c_db.check(d->dbias, dev, "conv2d_wgrad", "dbias");
  if (rc) return rc;

  WgradArgs a;
  a.x = d->x;
  a.gy = d->gy;
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
    hipLaunchKernelGGL((wgrad_partial_kernel<2, 2>), grid, dim3(kThreads), 0, s, a);
  else if (g.tm == 2)
    hipLaunchKernelGGL((wgrad_partial_kernel<2, 1>), grid, dim3(kThreads), 0, s, a);
  else if (g.tn == 2)
    hipLaunchKernelGGL((wgrad_partial_kernel<1, 2>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((wgrad_partial_kernel<1, 1>), grid, dim3(kThreads), 0, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  const size_t items = g.tile_floats + (size_t)d->cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     (const float*)d->workspace, g.tile_floats, a.bias_base, g.slabs, d->cin, d->cout, g.taps, d->dw,
                     d->dbias);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
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
