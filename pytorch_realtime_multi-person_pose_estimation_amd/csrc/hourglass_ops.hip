// The two layers of the stacked hourglass (lib/network/rtpose_hourglass.py) that are not stride-1 convs, for gfx950 (MI355X),
// fp32:
//
//  * the stem, nn.Conv2d(3, 64, 7, stride 2, padding 3) + `bn1` (folded into filters and bias by the caller) + nn.ReLU
//    (:162-164): 0.35 GMAC per 384 x 384 image, 0.5 % of the network, against 9.4 MB of fp32 output per image.  K = 147 is
//    too short and too ragged (3 channels, stride 2) to be worth the A-operand gather of a matrix-core form, so this is the
//    plain form: a block owns a 32 x 16 tile of output pixels of one image, stages the 69 x 37 x 3 input halo (masked loads
//    give the zero padding; dense NCHW or a layout buffer, as conv_first.hip reads them) and the whole 147 x 64 filter matrix
//    in LDS, and a thread accumulates 2 pixels x 64 channels in registers: per tap 2 halo reads and 16 broadcast 16-byte
//    filter reads feed 128 v_fma_f32.  A pixel's 64 channels leave as 16 16-byte stores (256 contiguous bytes).  Blocks are
//    persistent (2 per CU) so the 38 KB of filters are staged once per block, not once per tile.
//  * `up1 + Upsample(scale_factor = 2)(low3)` (:84-85) as one pass: a thread owns 4 channels of one low-resolution pixel,
//    reads them once and adds them to the 2 x 2 pixels of `up` above it.  Bound by its 3 map passes of HBM traffic.
#include <hip/hip_runtime.h>

#include "conv_desc.h"
#include "launchers.h"

namespace rtpose {

namespace stem7 {

constexpr int TH = 32, TW = 16;                  // output pixels of a block tile: thread (ty, tx) owns rows ty and ty + 16
constexpr int HH = 2 * TH + 5, WW = 2 * TW + 5;  // input halo of a tile
constexpr int WS = WW + 1;                       // LDS row stride of the halo
constexpr int TAPS = 3 * 7 * 7;
constexpr int WFLOATS = TAPS * 64 + 64;          // filters [tap][64] and the bias behind them
constexpr int HFLOATS = 3 * HH * WS;
constexpr size_t LDS_BYTES = (size_t)(WFLOATS + HFLOATS) * sizeof(float);

struct Args {
  const float* x_nchw;  // dense [N, 3, H, W], or NULL: read `x_lay`
  const float* x_lay;   // layout buffer with >= 3 channels per pixel
  int xl_cstride, xl_choff, xl_ws, xl_hs, xl_lead;
  const float* wp;      // pack_stem7_kernel: [tap = (c * 7 + ky) * 7 + kx][64], then bias[64]
  float* out;
  int o_cstride, o_choff, o_ws, o_hs, o_lead;
  int N, H, W, Ho, Wo, relu, tiles_x, tiles_y;
};

__global__ __launch_bounds__(256, 2) void conv7x7_s2_kernel(const Args A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wsm = smem;
  float* halo = smem + WFLOATS;
  const int tid = threadIdx.x;
  const int tx = tid & (TW - 1), ty = tid >> 4;
  for (int i = tid; i < WFLOATS / 4; i += 256)
    reinterpret_cast<float4*>(wsm)[i] = reinterpret_cast<const float4*>(A.wp)[i];
  const int ntiles = A.N * A.tiles_y * A.tiles_x;
  for (int b = blockIdx.x; b < ntiles; b += gridDim.x) {
    const int txi = b % A.tiles_x, r0 = b / A.tiles_x;
    const int tyi = r0 % A.tiles_y, n = r0 / A.tiles_y;
    const int y0 = tyi * TH, x0 = txi * TW;
    __syncthreads();  // the previous tile's readers are done with the halo
    for (int i = tid; i < 3 * HH * WW; i += 256) {
      const int c = i / (HH * WW), r = i - c * (HH * WW);
      const int hy = r / WW, hx = r - hy * WW;
      const int yy = 2 * y0 - 3 + hy, xx = 2 * x0 - 3 + hx;
      float v = 0.f;
      if (yy >= 0 && yy < A.H && xx >= 0 && xx < A.W) {
        v = A.x_nchw ? A.x_nchw[((size_t)(n * 3 + c) * A.H + yy) * A.W + xx]
                     : A.x_lay[((size_t)A.xl_lead + (size_t)(n * A.xl_hs + yy) * A.xl_ws + xx) * A.xl_cstride + A.xl_choff + c];
      }
      halo[(c * HH + hy) * WS + hx] = v;
    }
    __syncthreads();  // halo (and, the first time round, the filters) staged
    float acc[2][64];
#pragma unroll
    for (int o = 0; o < 64; ++o) acc[0][o] = acc[1][o] = wsm[TAPS * 64 + o];
    for (int cy = 0; cy < 21; ++cy) {  // (channel, filter row)
      const int c = cy / 7, ky = cy - c * 7;
      const float* h0 = halo + (c * HH + 2 * ty + ky) * WS + 2 * tx;
      const float* h1 = h0 + 2 * (TH / 2) * WS;
      const float4* w4 = reinterpret_cast<const float4*>(wsm + cy * 7 * 64);
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float a0 = h0[kx], a1 = h1[kx];
#pragma unroll
        for (int o4 = 0; o4 < 16; ++o4) {
          const float4 w = w4[kx * 16 + o4];
          acc[0][4 * o4 + 0] = fmaf(a0, w.x, acc[0][4 * o4 + 0]);
          acc[0][4 * o4 + 1] = fmaf(a0, w.y, acc[0][4 * o4 + 1]);
          acc[0][4 * o4 + 2] = fmaf(a0, w.z, acc[0][4 * o4 + 2]);
          acc[0][4 * o4 + 3] = fmaf(a0, w.w, acc[0][4 * o4 + 3]);
          acc[1][4 * o4 + 0] = fmaf(a1, w.x, acc[1][4 * o4 + 0]);
          acc[1][4 * o4 + 1] = fmaf(a1, w.y, acc[1][4 * o4 + 1]);
          acc[1][4 * o4 + 2] = fmaf(a1, w.z, acc[1][4 * o4 + 2]);
          acc[1][4 * o4 + 3] = fmaf(a1, w.w, acc[1][4 * o4 + 3]);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int y = y0 + ty + p * (TH / 2), x = x0 + tx;
      if (y < A.Ho && x < A.Wo) {
        float* o = A.out + ((size_t)A.o_lead + (size_t)(n * A.o_hs + y) * A.o_ws + x) * A.o_cstride + A.o_choff;
#pragma unroll
        for (int o4 = 0; o4 < 16; ++o4) {
          float4 v = make_float4(acc[p][4 * o4], acc[p][4 * o4 + 1], acc[p][4 * o4 + 2], acc[p][4 * o4 + 3]);
          if (A.relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
          reinterpret_cast<float4*>(o)[o4] = v;
        }
      }
    }
  }
}

// wp[tap][o] <- w[o][c][ky][kx], tap = (c * 7 + ky) * 7 + kx = the OIHW offset inside one filter; bias behind
__global__ void pack_stem7_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 64) wp[TAPS * 64 + i] = bias ? bias[i] : 0.f;
  if (i >= TAPS * 64) return;
  const int o = i & 63, tap = i >> 6;
  wp[i] = w[o * TAPS + tap];
}

}  // namespace stem7

size_t conv7x7_s2_packed_floats() { return (size_t)stem7::WFLOATS; }

int conv7x7_s2_pack_launch(const float* w_oihw, const float* bias, float* wp, hipStream_t s) {
  if (!w_oihw || !wp) return fail(RTPOSE_E_INVAL, "pack_conv7x7_s2: NULL argument");
  hipLaunchKernelGGL(stem7::pack_stem7_kernel, dim3(ceil_div(stem7::TAPS * 64, 256)), dim3(256), 0, s, w_oihw, bias, wp);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

// H x W: the INPUT size; the output is ceil(H / 2) x ceil(W / 2)
int conv7x7_s2_launch(const float* x_nchw, const float* x_lay, const rtpose_layout* lx, const float* wp, float* out,
                      const rtpose_layout* lo, int relu, int N, int H, int W, hipStream_t s) {
  using namespace stem7;
  if ((!x_nchw && (!x_lay || !lx)) || !wp || !out || !lo || N <= 0 || H <= 0 || W <= 0)
    return fail(RTPOSE_E_INVAL, "conv7x7_s2: bad arguments");
  if (!x_nchw && !slice_inside(*lx, 3)) return fail(RTPOSE_E_INVAL, "conv7x7_s2: input slice exceeds cstride");
  if (!slice_ok(*lo, 64, 4)) return fail(RTPOSE_E_INVAL, "conv7x7_s2: the 64-channel output slice must be 16-byte aligned and inside cstride");
  if (reinterpret_cast<uintptr_t>(wp) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
    return fail(RTPOSE_E_INVAL, "conv7x7_s2: w_packed and out must be 16-byte aligned");
  Args a;
  memset(&a, 0, sizeof(a));
  a.x_nchw = x_nchw;
  a.x_lay = x_lay;
  if (lx) {
    a.xl_cstride = lx->cstride;
    a.xl_choff = lx->choff;
    a.xl_ws = lx->ws;
    a.xl_hs = lx->hs;
    a.xl_lead = lx->lead;
  }
  a.wp = wp;
  a.out = out;
  a.o_cstride = lo->cstride;
  a.o_choff = lo->choff;
  a.o_ws = lo->ws;
  a.o_hs = lo->hs;
  a.o_lead = lo->lead;
  a.N = N;
  a.H = H;
  a.W = W;
  a.Ho = (H + 1) / 2;
  a.Wo = (W + 1) / 2;
  if (a.Ho > lo->hs || a.Wo > lo->ws) return fail(RTPOSE_E_INVAL, "conv7x7_s2: the output layout is smaller than ceil(H / 2) x ceil(W / 2)");
  a.relu = relu;
  a.tiles_x = ceil_div(a.Wo, TW);
  a.tiles_y = ceil_div(a.Ho, TH);
  const long tiles = (long)N * a.tiles_x * a.tiles_y;
  if (tiles > 0x3fffffffL) return fail(RTPOSE_E_INVAL, "conv7x7_s2: too many tiles");
  const long blocks = tiles < 2L * device_cu_count() ? tiles : 2L * device_cu_count();
  return launch_kernel<conv7x7_s2_kernel>(dim3((unsigned)blocks), dim3(256), LDS_BYTES, LDS_BYTES, s, a);
}

// ---- out = up + upsample2(low) -------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// one thread per (low-resolution pixel, 4 channels); Hl x Wl is the low-resolution size.  `up` and `out` may be the same
// slice: a thread reads its 4 elements of `up` before it writes them and no other thread touches them.
__global__ void upsample2_add_kernel(const float* up, Lay lu, const float* __restrict__ low, Lay ll, float* out, Lay lo,
                                     int C, int N, int Hl, int Wl) {
  const int c4 = C >> 2;
  const size_t total = (size_t)N * Hl * Wl * c4;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % c4) * 4;
  size_t p = i / c4;
  const int x = p % Wl;
  p /= Wl;
  const int y = p % Hl;
  const int n = (int)(p / Hl);
  const float4 l = *reinterpret_cast<const float4*>(low + lay_off(ll, n, y, x) + c);
  float4 u[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    u[j] = *reinterpret_cast<const float4*>(up + lay_off(lu, n, 2 * y + (j >> 1), 2 * x + (j & 1)) + c);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<float4*>(out + lay_off(lo, n, 2 * y + (j >> 1), 2 * x + (j & 1)) + c) = add4(u[j], l);
}

}  // namespace

int upsample2_add_launch(const float* up, const rtpose_layout* lup, const float* low, const rtpose_layout* llow, float* out,
                         const rtpose_layout* lout, int C, int N, int H, int W, hipStream_t s) {
  if (!up || !lup || !low || !llow || !out || !lout || C <= 0 || N <= 0 || H <= 0 || W <= 0)
    return fail(RTPOSE_E_INVAL, "upsample2_add: bad arguments");
  if ((H | W) & 1) return fail(RTPOSE_E_INVAL, "upsample2_add: H and W (the size of `up` and `out`) must be even");
  if ((C % 4) || !slice_ok(*lup, C, 4) || !slice_ok(*llow, C, 4) || !slice_ok(*lout, C, 4))
    return fail(RTPOSE_E_INVAL, "upsample2_add: channel slices must be 16-byte aligned and inside cstride");
  if (H > lup->hs || W > lup->ws || H > lout->hs || W > lout->ws || H / 2 > llow->hs || W / 2 > llow->ws)
    return fail(RTPOSE_E_INVAL, "upsample2_add: a layout is smaller than its map");
  if ((reinterpret_cast<uintptr_t>(up) | reinterpret_cast<uintptr_t>(low) | reinterpret_cast<uintptr_t>(out)) % 16)
    return fail(RTPOSE_E_INVAL, "upsample2_add: buffers must be 16-byte aligned");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 4);
  if (total > 0x7fffffffull * 256) return fail(RTPOSE_E_INVAL, "upsample2_add: grid too large");
  hipLaunchKernelGGL(upsample2_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, up, to_lay(lup), low,
                     to_lay(llow), out, to_lay(lout), C, N, H / 2, W / 2);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace rtpose

extern "C" {

size_t rtpose_conv7x7_s2_packed_floats(void) { return rtpose::conv7x7_s2_packed_floats(); }

int rtpose_pack_conv7x7_s2(const float* w_oihw, const float* bias, float* w_packed, void* stream) {
  return rtpose::conv7x7_s2_pack_launch(w_oihw, bias, w_packed, rtpose::as_stream(stream));
}

int rtpose_conv7x7_s2(const float* x_nchw, const float* x_layout, const rtpose_layout* lx, const float* w_packed,
                      float* out, const rtpose_layout* lout, int relu, int N, int H, int W, void* stream) {
  return rtpose::conv7x7_s2_launch(x_nchw, x_layout, lx, w_packed, out, lout, relu, N, H, W, rtpose::as_stream(stream));
}

int rtpose_upsample2_add(const float* up, const rtpose_layout* lup, const float* low, const rtpose_layout* llow, float* out,
                         const rtpose_layout* lout, int C, int N, int H, int W, void* stream) {
  return rtpose::upsample2_add_launch(up, lup, low, llow, out, lout, C, N, H, W, rtpose::as_stream(stream));
}

}  // extern "C"
