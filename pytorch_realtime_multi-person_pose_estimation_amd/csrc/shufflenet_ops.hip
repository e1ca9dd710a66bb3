// ShuffleNetV2 building blocks (lib/network/rtpose_shufflenetV2.py) outside the pointwise chains: the affine input
// conversion, the stem conv (three forms), MaxPool2d(3, 2, ceil), the depthwise 3x3 and the channel-map copies.  HBM-bound,
// one coalesced pass each.  The element-wise ones are one template over the activation's element type: fp32, 4 channels
// per thread, or bf16 (bf16 plans, BASELINE config 4 "fp32 and bf16": bf16 activations in HBM, fp32 arithmetic), 8
// channels per thread - 16 bytes either way (ChanVec, pixel_walk.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chan_slab.h"
#include "pixel_walk.h"

namespace rtpose {

// NCHW -> layout with y = x * scale[c] + shift[c] (BatchNorm2d(3) on the input, :96).
__global__ void nchw_to_layout_affine_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                             Lay l, int C, int cpad, int N, int H, int W,
                                             const float* __restrict__ scale,
                                             const float* __restrict__ shift) {
  Walk q;
  if (!pixel_walk(cpad, N, H, W, q)) return;
  float v = 0.f;
  if (q.c < C) {
    v = src[(((size_t)q.n * C + q.c) * H + q.y) * W + q.x];
    if (scale) v = v * scale[q.c] + shift[q.c];
  }
  dst[lay_off(l, q) + q.c] = v;
}

// 3x3 stride-2 pad-1 dense conv, tiny cin (stem 3->24, :97).  HBM-bound: one thread = one
// output pixel x ALL output channels (COUT/4 float4 accumulators), the 9 x 8-channel input
// taps are two float4 loads each, and the weight index depends on loop counters only, so
// the weights arrive through the scalar cache (s_load), not the vector path.
// w[ky][kx][8][COUT].  The input layout's zero gaps are the padding: no bounds tests.
// Same conv fused with the two steps in front of it (rtpose_shufflenetV2.py:96-97): reads the dense
// NCHW fp32 image directly (3 planes, x fastest = coalesced), applies the input BatchNorm2d(3) as a
// per-channel affine (the conv's zero padding is applied AFTER it, as in the reference graph) and
// writes NHWC.  Removes the NHWC8 staging tensor (555 MB at batch 128) and 5/8 of the FMAs.
template <int COUT>
__global__ void stem_conv3x3_s2_nchw_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                            const float* __restrict__ shift, const float* __restrict__ w,
                                            const float* __restrict__ bias, float* __restrict__ out, Lay lo,
                                            int N, int H, int W, int Ho, int Wo, int relu, int out_bf16) {
  constexpr int C4 = COUT / 4;
  Walk q;
  if (!pixel_walk(N, Ho, Wo, q)) return;
  const int ox = q.x, oy = q.y, n = q.n;
  float4 acc[C4];
#pragma unroll
  for (int j = 0; j < C4; ++j) acc[j] = *reinterpret_cast<const float4*>(bias + 4 * j);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    const float* plane = x + ((size_t)n * 3 + c) * H * W;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy + ky - 1;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox + kx - 1;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const float v = in ? plane[(size_t)iy * W + ix] * sc + sh : 0.f;
        const float* wp = w + (size_t)((ky * 3 + kx) * 8 + c) * COUT;  // packed [ky][kx][8][COUT]
#pragma unroll
        for (int j = 0; j < C4; ++j) {
          const float4 ww = *reinterpret_cast<const float4*>(wp + 4 * j);
          acc[j].x += v * ww.x;
          acc[j].y += v * ww.y;
          acc[j].z += v * ww.z;
          acc[j].w += v * ww.w;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < C4; ++j) {
    if (relu) {
      acc[j].x = fmaxf(acc[j].x, 0.f);
      acc[j].y = fmaxf(acc[j].y, 0.f);
      acc[j].z = fmaxf(acc[j].z, 0.f);
      acc[j].w = fmaxf(acc[j].w, 0.f);
    }
  }
  if (out_bf16) {  // uniform: bf16 plans keep the stem output as 2-byte elements
    unsigned short* oh = reinterpret_cast<unsigned short*>(out) + lay_off(lo, q);
#pragma unroll
    for (int j = 0; j < C4; j += 2) {
      const ChanVec<unsigned short> u = {
          {acc[j].x, acc[j].y, acc[j].z, acc[j].w, acc[j + 1].x, acc[j + 1].y, acc[j + 1].z, acc[j + 1].w}};
      u.store(oh + 4 * j);
    }
    return;
  }
  float* op = out + lay_off(lo, q);
#pragma unroll
  for (int j = 0; j < C4; ++j) *reinterpret_cast<float4*>(op + 4 * j) = acc[j];
}

// Stem conv + max-pool in ONE launch (rtpose_shufflenetV2.py:96-99: BatchNorm2d(3) -> conv 3x3 s2 p1 + BN +
// ReLU -> MaxPool2d(3, 2, 0, ceil_mode=True)).  A block owns an 8 x 8 tile of pool outputs: it stages the
// 35 x 35 x 3 input patch (affine applied, zero outside the image: the conv's padding comes after the
// BatchNorm) in LDS, evaluates the 17 x 17 x 24 conv outputs the tile's windows
// touch (13 % recomputed at tile borders) into LDS, and writes the window maxima.  The 184 x 184 x 24
// stem tensor (416 MB fp32 / 208 MB bf16 at batch 128) is never stored: the two launches it replaces
// cost 0.60 (fp32) / 0.52 ms (bf16) of a 10.5 / 4.7 ms forward.
//
// Round 5: the kernel was bound by its VALU work around the matrix instructions, not by them (per block and wave ~4300
// issue cycles of address arithmetic, masks and selects against 2240 of MFMA).  Now
//  * VEC: image rows are read as aligned float4 (W % 4 == 0: the patch columns 32 bx - 4 .. 32 bx + 35 are ten whole
//    float4 per row, each entirely inside or outside the image): 5 loads per thread instead of 15, a quarter of the
//    index arithmetic; the scalar loader stays for other widths;
//  * the ReLU and the "conv output does not exist" mask left the MFMA write-out: the pool starts from 0 (max(0, .) IS
//    the ReLU) and only the tiles at the map's right / bottom edge test the window positions; the write-out is 16
//    ds_write_b32 at immediate offsets;
//  * tap offsets / filter registers are picked from compile-time tables and loaded before the patch arrives; fragments
//    wholly below the conv map are skipped; the waves that take the odd fragments rotate with the block index.
constexpr int kSpT = 8;                   // pool outputs per tile side
constexpr int kSpS = 2 * kSpT + 1;        // conv outputs per tile side (17)
constexpr int kSpI = 2 * kSpS + 1;        // input pixels per tile side (35)
constexpr int kSpIP = 40;                 // LDS row pitch of the input patch: column j holds image column ix0 - 3 + j
constexpr int kSpX0 = 3;                  // LDS column of the tile's first input pixel (ix0 = 32 bx - 1)
constexpr int kSpC = 24;
constexpr int kSpCP = 28;                 // LDS pitch of one conv output's channels (conflict skew)
constexpr int kSpF = (kSpS * kSpS + 31) / 32;  // MFMA fragments of 32 conv positions per tile (10)
// tap k = (ky * 3 + kx) * 3 + c of the K dimension (k = 27: tap 26 again, under a zero weight)
__host__ __device__ constexpr int sp_tap_off(int k) {
  const int kk = k < 26 ? k : 26;
  return ((kk % 3) * kSpI + (kk / 3) / 3) * kSpIP + (kk / 3) % 3 + kSpX0;
}
__host__ __device__ constexpr int sp_tap_w(int k) {  // packed filters [ky][kx][8][24]
  const int kk = k < 26 ? k : 26;
  return ((kk / 3) * 8 + kk % 3) * kSpC;
}
template <int OUT_BF16, int VEC>
__global__ __launch_bounds__(256) void stem_pool_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ w,
                                                        const float* __restrict__ bias, void* __restrict__ out_v,
                                                        Lay lo, int H, int W, int H1, int W1, int H2, int W2) {
  __shared__ __attribute__((aligned(16))) float s_in[3 * kSpI][kSpIP];
  __shared__ __attribute__((aligned(16))) float s_st[kSpF * 32][kSpCP];
  const int tid = threadIdx.x;
  const int n = blockIdx.z;
  const int py0 = blockIdx.y * kSpT, px0 = blockIdx.x * kSpT;
  const int sy0 = 2 * py0, sx0 = 2 * px0;        // first conv output of the tile
  const int iy0 = 2 * sy0 - 1, ix0 = 2 * sx0 - 1;  // first input pixel of the tile (may be -1: padding)
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
  // filter registers of the matrix phase (B operand: channel l31, tap 2 j + kh), requested before the patch
  float bw[14];
#pragma unroll
  for (int j = 0; j < 14; ++j) {
    const int wi = (kh ? sp_tap_w(2 * j + 1) : sp_tap_w(2 * j)) + min(l31, kSpC - 1);
    const float t = w[wi];
    bw[j] = (l31 < kSpC && 2 * j + kh < 27) ? t : 0.f;
  }
  const float bv = l31 < kSpC ? bias[min(l31, kSpC - 1)] : 0.f;
  const float sc[3] = {scale ? scale[0] : 1.f, scale ? scale[1] : 1.f, scale ? scale[2] : 1.f};
  const float sh[3] = {scale ? shift[0] : 0.f, scale ? shift[1] : 0.f, scale ? shift[2] : 0.f};
  const float* xn = x + (size_t)n * 3 * H * W;
  if (VEC) {  // rows as aligned float4: thread = (float4 q of the row, row r0 + 25 u of the 105 patch rows)
    constexpr int NR = 5;
    const int q = tid % 10, r0 = tid / 10;
    const int ix4 = ix0 - kSpX0 + 4 * q;
    const bool xin = ix4 >= 0 && ix4 < W && tid < 250;
    const int ixc = min(max(ix4, 0), W - 4);
    float4 v[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) {  // branch-free: clamped addresses, masked afterwards
      const int r = min(r0 + 25 * u, 3 * kSpI - 1);
      const int c = r / kSpI, yy = r - c * kSpI;
      const int iy = iy0 + yy;
      const bool in = xin && iy >= 0 && iy < H;
      const float4 t = *reinterpret_cast<const float4*>(xn + (size_t)(unsigned)(c * H + min(max(iy, 0), H - 1)) * (unsigned)W + ixc);
      const float a = c == 0 ? sc[0] : (c == 1 ? sc[1] : sc[2]), b = c == 0 ? sh[0] : (c == 1 ? sh[1] : sh[2]);
      v[u] = in ? make_float4(t.x * a + b, t.y * a + b, t.z * a + b, t.w * a + b) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      const int r = r0 + 25 * u;
      if (tid < 250 && r < 3 * kSpI) *reinterpret_cast<float4*>(&s_in[r][4 * q]) = v[u];
    }
  } else {  // any width: one pixel per load, all of a thread's loads issued before the first is used
    constexpr int NL = (3 * kSpI * kSpI + 255) / 256;
    float v[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int i = min(tid + 256 * u, 3 * kSpI * kSpI - 1);
      const int xx = i % kSpI;
      const int r = i / kSpI;
      const int yy = r % kSpI, c = r / kSpI;
      const int iy = iy0 + yy, ix = ix0 + xx;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float t = xn[(unsigned)(c * H + min(max(iy, 0), H - 1)) * (unsigned)W + (unsigned)min(max(ix, 0), W - 1)];
      const float a = c == 0 ? sc[0] : (c == 1 ? sc[1] : sc[2]), b = c == 0 ? sh[0] : (c == 1 ? sh[1] : sh[2]);
      v[u] = in ? t * a + b : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int i = tid + 256 * u;
      if (i < 3 * kSpI * kSpI) s_in[i / kSpI][i % kSpI + kSpX0] = v[u];
    }
  }
  __syncthreads();
  // conv outputs on the matrix pipe (round 4; v_mfma_f32_32x32x2_f32): the 17 x 17 positions are the M dimension (10
  // fragments of 32), the 24 output channels N (one fragment), the 27 taps K (14 steps of 2, the last one half empty).
  // A operand: lane (position, kh) reads tap k = 2 j + kh of ITS position from the input patch in LDS - an im2col that
  // exists only as 14 ds_read_b32 per fragment; B operand: the filter value of channel l31 for that tap, 14 registers
  // loaded once per block.  The scalar-FMA form this replaces issued 240 M VALU instructions per launch (address
  // arithmetic around 27 LDS reads and 324 FMAs per position, SQ_INSTS_VALU, profiles/r04_shufflenet_pmc_sq.txt)
  // and was bound by exactly that: 0.38 ms of an 8.9 / 4.05 ms forward.
  {
    typedef float floatx16 __attribute__((ext_vector_type(16)));
    // fragments whose positions all lie below the conv map are not computed (the tiles of the last tile row)
    const int nf = min(kSpF, (min(kSpS, H1 - sy0) * kSpS + 31) / 32);
    const int w0 = (wv + blockIdx.x + blockIdx.y) & 3;  // the SIMDs take turns at the third fragment
    for (int f = w0; f < nf; f += 4) {
      const int p = min(f * 32 + l31, kSpS * kSpS - 1);  // the position this lane feeds (rows past the end replay the last)
      const int sy = p / kSpS, sx = p - sy * kSpS;
      const float* ab = &s_in[2 * sy][2 * sx];
      floatx16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = bv;
#pragma unroll
      for (int j = 0; j < 14; ++j)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ab[kh ? sp_tap_off(2 * j + 1) : sp_tap_off(2 * j)], bw[j], acc, 0, 0, 0);
      // C layout: lane = channel l31, register r = position (r / 4) * 8 + 4 kh + r % 4 of the fragment
      if (l31 < kSpC) {
        float* st = &s_st[f * 32 + 4 * kh][l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) st[((r >> 2) * 8 + (r & 3)) * kSpCP] = acc[r];
      }
    }
  }
  __syncthreads();
  // window maxima: item = (pool output, 8-channel group).  The maxima start from 0 - the ReLU; windows that hang over the
  // conv map (ceil mode) skip the positions that do not exist (only tiles on the map's right / bottom edge can have any).
  const bool edge = sy0 + kSpS > H1 || sx0 + kSpS > W1;
  for (int it = tid; it < kSpT * kSpT * 3; it += 256) {
    const int g = it % 3, q = it / 3;
    const int ty = q / kSpT, tx = q - ty * kSpT;
    const int py = py0 + ty, px = px0 + tx;
    if (py >= H2 || px >= W2) continue;
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = 0.f;
    auto window = [&](auto masked) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          if (masked && !(sy0 + 2 * ty + dy < H1 && sx0 + 2 * tx + dx < W1)) continue;
          const float* sp = &s_st[(2 * ty + dy) * kSpS + 2 * tx + dx][8 * g];
          const float4 a = *reinterpret_cast<const float4*>(sp), b = *reinterpret_cast<const float4*>(sp + 4);
          m[0] = fmaxf(m[0], a.x), m[1] = fmaxf(m[1], a.y), m[2] = fmaxf(m[2], a.z), m[3] = fmaxf(m[3], a.w);
          m[4] = fmaxf(m[4], b.x), m[5] = fmaxf(m[5], b.y), m[6] = fmaxf(m[6], b.z), m[7] = fmaxf(m[7], b.w);
        }
    };
    if (edge)
      window(std::true_type{});
    else
      window(std::false_type{});
    if (OUT_BF16) {
      const ChanVec<unsigned short> u = {{m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]}};
      u.store(reinterpret_cast<unsigned short*>(out_v) + lay_off(lo, n, py, px) + 8 * g);
    } else {
      float* o = reinterpret_cast<float*>(out_v) + lay_off(lo, n, py, px) + 8 * g;
      *reinterpret_cast<float4*>(o) = make_float4(m[0], m[1], m[2], m[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(m[4], m[5], m[6], m[7]);
    }
  }
}

template <int COUT>
__global__ void stem_conv3x3_s2_kernel(const float* __restrict__ in, Lay li, const float* __restrict__ w,
                                       const float* __restrict__ bias, float* __restrict__ out, Lay lo,
                                       int N, int Ho, int Wo, int relu) {
  constexpr int C4 = COUT / 4;
  Walk q;
  if (!pixel_walk(N, Ho, Wo, q)) return;
  float4 acc[C4];
#pragma unroll
  for (int j = 0; j < C4; ++j) acc[j] = *reinterpret_cast<const float4*>(bias + 4 * j);
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      // input pixel (2y+ky-1, 2x+kx-1): offsets of -1 land in the layout gaps
      const float* ip = in + (long long)lay_off(li, q.n, 2 * q.y + ky, 2 * q.x + kx) -
                        (long long)(li.ws + 1) * li.cstride;
      const float4 v0 = *reinterpret_cast<const float4*>(ip);
      const float4 v1 = *reinterpret_cast<const float4*>(ip + 4);
      const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      const float* wp = w + (size_t)(ky * 3 + kx) * 8 * COUT;
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int j = 0; j < C4; ++j) {
          const float4 ww = *reinterpret_cast<const float4*>(wp + c * COUT + 4 * j);
          acc[j].x += v[c] * ww.x;
          acc[j].y += v[c] * ww.y;
          acc[j].z += v[c] * ww.z;
          acc[j].w += v[c] * ww.w;
        }
    }
  float* op = out + lay_off(lo, q);
#pragma unroll
  for (int j = 0; j < C4; ++j) {
    float4 a = acc[j];
    if (relu) {
      a.x = fmaxf(a.x, 0.f);
      a.y = fmaxf(a.y, 0.f);
      a.z = fmaxf(a.z, 0.f);
      a.w = fmaxf(a.w, 0.f);
    }
    *reinterpret_cast<float4*>(op + 4 * j) = a;
  }
}

// MaxPool2d(3, 2, 0, ceil_mode=True): windows are clipped to the input.
template <class T>
__global__ void maxpool3x3s2_ceil_kernel(const T* __restrict__ src, Lay ls, T* __restrict__ dst, Lay ld, int C, int N,
                                         int H, int W, int Ho, int Wo) {
  typedef ChanVec<T> V;
  Walk q;
  if (!pixel_walk<V::kLanes>(C >> V::kShift, N, Ho, Wo, q)) return;
  V r;
#pragma unroll
  for (int e = 0; e < V::kLanes; ++e) r.v[e] = -INFINITY;
  for (int dy = 0; dy < 3; ++dy)
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = 2 * q.y + dy, xx = 2 * q.x + dx;
      if (yy < H && xx < W) {
        const V v = V::load(src + lay_off(ls, q.n, yy, xx) + q.c);
#pragma unroll
        for (int e = 0; e < V::kLanes; ++e) r.v[e] = fmaxf(r.v[e], v.v[e]);
      }
    }
  r.store(dst + lay_off(ld, q) + q.c);
}

// depthwise 3x3, pad 1 (the input layout's zero gaps), stride 1 or 2, + bias; w[9][C].
// O: the output's element type - T's, or float behind a bf16 input (the training forward of a layout-resident run, whose
// BatchNorm reads the fp32 pre-activation: the accumulators are stored as they are, two 16-byte stores)
template <class T, class O = T>
__global__ void dwconv3x3_kernel(const T* __restrict__ in, Lay li, const float* __restrict__ w,
                                 const float* __restrict__ bias, O* __restrict__ out, Lay lo, int C, int N, int Ho,
                                 int Wo, int stride) {
  typedef ChanVec<T> V;
  Walk q;
  if (!pixel_walk<V::kLanes>(C >> V::kShift, N, Ho, Wo, q)) return;
  V acc = V::load_f32(bias + q.c);
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const T* ip = in + (long long)lay_off(li, q.n, stride * q.y + ky, stride * q.x + kx) -
                    (long long)(li.ws + 1) * li.cstride + q.c;
      const V v = V::load(ip);
      const V ww = V::load_f32(w + (size_t)(ky * 3 + kx) * C + q.c);
#pragma unroll
      for (int e = 0; e < V::kLanes; ++e) acc.v[e] += v.v[e] * ww.v[e];
    }
  if constexpr (std::is_same<O, T>::value) {
    acc.store(out + lay_off(lo, q) + q.c);
  } else {
    static_assert(V::kBf16 && std::is_same<O, float>::value, "bf16 in, fp32 out");
    float* op = out + lay_off(lo, q) + q.c;
    *reinterpret_cast<float4*>(op) = make_float4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    *reinterpret_cast<float4*>(op + 4) = make_float4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]);
  }
}

// depthwise 3x3, stride 1, fp32: FOUR consecutive output pixels of a row per thread.  The plain kernel
// issues 9 activation + 9 weight loads per output (it is load-instruction bound, ~2 TB/s); here
// the 3x6 input window and the 9 weight vectors are loaded once for four outputs (28 vs 76 loads).
__global__ void dwconv3x3_s1x4_kernel(const float* __restrict__ in, Lay li, const float* __restrict__ w,
                                      const float* __restrict__ bias, float* __restrict__ out, Lay lo, int C,
                                      int N, int H, int W) {
  typedef ChanVec<float> V;
  Walk q;
  if (!pixel_walk<4>(C / 4, N, H, (W + 3) >> 2, q)) return;
  const int c = q.c, x0 = q.x * 4;
  V acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o].v[e] = bias[c + e];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    float wv[3][4];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[kx][e] = w[(size_t)(ky * 3 + kx) * C + c + e];
    // input row y + ky - 1, columns x0 - 1 .. x0 + 4 (offsets of -1 land in the layout gaps; columns
    // past the row end read the gap / the next row and only feed outputs that are not stored)
    const long long row = (long long)lay_off(li, q.n, q.y + ky, x0) - (long long)(li.ws + 1) * li.cstride + c;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const V v = V::load(in + row + (long long)j * li.cstride);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int kx = j - o;  // input column j feeds output o through tap kx = j - o
        if (kx >= 0 && kx < 3) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[o].v[e] += v.v[e] * wv[kx][e];
        }
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if (x0 + o >= W) break;
    acc[o].store(out + lay_off(lo, q.n, q.y, x0 + o) + c);
  }
}

// 16 bytes of consecutive source channels per thread (one load), up to 4 (fp32) / 8 (bf16) mapped element stores
template <class T>
__global__ void layout_copy_cmap_vec_kernel(const T* __restrict__ src, Lay ls, T* __restrict__ dst, Lay ld, int C,
                                            const int32_t* __restrict__ cmap, int N, int H, int W) {
  constexpr int L = ChanVec<T>::kLanes;
  Walk q;
  if (!pixel_walk<L>((C + L - 1) >> ChanVec<T>::kShift, N, H, W, q)) return;
  const ChanBits<T> v = *reinterpret_cast<const ChanBits<T>*>(src + lay_off(ls, q) + q.c);
  T* d = dst + lay_off(ld, q) - ld.choff;
#pragma unroll
  for (int k = 0; k < L; ++k)
    if (q.c + k < C) d[cmap[q.c + k]] = v.lane(k);
}

__global__ void layout_copy_cmap_kernel(const float* __restrict__ src, Lay ls, float* __restrict__ dst,
                                        Lay ld, int C, const int32_t* __restrict__ cmap, int N, int H,
                                        int W) {
  Walk q;
  if (!pixel_walk(C, N, H, W, q)) return;
  dst[lay_off(ld, q) - ld.choff + cmap[q.c]] = src[lay_off(ls, q) + q.c];
}

// ---- the fp32 / bf16 door pairs: T is float or the bf16 bits, `who` the entry point's name in the message ----
template <class T>
static int maxpool3x3s2_ceil(const char* who, const void* in, const rtpose_layout* lin, void* out, const rtpose_layout* lout,
                      int C, int N, int H, int W, void* stream) {
  constexpr int L = ChanVec<T>::kLanes;
  if ((C % L) || !slice_aligned(lin, L) || !slice_aligned(lout, L) || H < 3 || W < 3)
    return fail(RTPOSE_E_INVAL, "%s: channel slices must be 16-byte aligned, H,W >= 3", who);
  const int Ho = (H - 3 + 1) / 2 + 1, Wo = (W - 3 + 1) / 2 + 1;  // ceil((H-3)/2)+1
  return launch_flat(maxpool3x3s2_ceil_kernel<T>, (size_t)N * Ho * Wo * (C / L), stream, static_cast<const T*>(in),
                     to_lay(lin), static_cast<T*>(out), to_lay(lout), C, N, H, W, Ho, Wo);
}

template <class T>
static int dwconv3x3(const char* who, const void* in_v, const rtpose_layout* lin, const float* w, const float* bias, void* out_v,
              const rtpose_layout* lout, int C, int N, int H, int W, int stride, void* stream) {
  constexpr int L = ChanVec<T>::kLanes;
  if ((C % L) || !slice_aligned(lin, L) || !slice_aligned(lout, L) || (stride != 1 && stride != 2) || lin->ws < W + 1 ||
      lin->hs < H + 1 || lin->lead < lin->ws + 1)
    return fail(RTPOSE_E_INVAL, "%s: unsupported layout / stride", who);
  const T* in = static_cast<const T*>(in_v);
  T* out = static_cast<T*>(out_v);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  // fp32, stride 1: 4 output pixels per thread
  // (the 4-pixels-per-thread form measured 2.6x SLOWER on bf16 - 32 accumulators x 8 channels per
  //  thread - so the bf16 plans keep one pixel per thread: 1.57 ms vs 4.03 ms over the 19 layers)
  if constexpr (std::is_same<T, float>::value)
    if (stride == 1)
      return launch_flat(dwconv3x3_s1x4_kernel, (size_t)N * H * ((W + 3) / 4) * (C / 4), stream, in, to_lay(lin), w, bias,
                         out, to_lay(lout), C, N, H, W);
  return launch_flat(dwconv3x3_kernel<T>, (size_t)N * Ho * Wo * (C / L), stream, in, to_lay(lin), w, bias, out,
                     to_lay(lout), C, N, Ho, Wo, stride);
}

// rtpose_dwconv3x3_bf16_f32: the doors of rtpose_dwconv3x3_bf16, with every argument checked as the training launchers
// check theirs (chan_slab.h)
static int dwconv3x3_bf16_f32(const char* who, const void* in, const rtpose_layout* lin, const float* w, const float* bias,
                              float* out, const rtpose_layout* lout, int C, int N, int H, int W, int stride, void* stream) {
  if (stride != 1 && stride != 2) return fail(RTPOSE_E_INVAL, "%s: stride must be 1 or 2 (got %d)", who, stride);
  long P;
  if (int rc = check_shape(who, C, N, H, W, P)) return rc;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (int rc = check_slice(who, "in", in, lin, C, H, W, 1)) return rc;
  if (int rc = check_slice(who, "out", out, lout, C, Ho, Wo, 0)) return rc;
  if (!w || !bias) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (w or bias)", who);
  if (C % 8) return fail(RTPOSE_E_INVAL, "%s: C must be a multiple of 8 (got %d)", who, C);
  if (!slice_aligned(lin, 8) || reinterpret_cast<uintptr_t>(in) % 16 || !aligned16(*lout, out))
    return fail(RTPOSE_E_INVAL, "%s: channel slices must be 16-byte aligned (in: base, cstride and choff multiples of 8 bf16 "
                                "elements; out: of 4 floats)", who);
  // (the kernel forms n * hs + y in an int)
  if (rtpose_layout_pixels(lin, N, H, W) >= ((size_t)1 << 31) || rtpose_layout_pixels(lout, N, Ho, Wo) >= ((size_t)1 << 31))
    return fail(RTPOSE_E_INVAL, "%s: tensor above the launch limit", who);

  static thread_local CheckedPtr c_in, c_w, c_b, c_out;
  const int dev = current_device();
  int rc = c_in.check(in, dev, who, "in");
  if (!rc) rc = c_w.check(w, dev, who, "w");
  if (!rc) rc = c_b.check(bias, dev, who, "bias");
  if (!rc) rc = c_out.check(out, dev, who, "out");
  if (rc) return rc;
  return launch_flat(dwconv3x3_kernel<unsigned short, float>, (size_t)N * Ho * Wo * (C / 8), stream,
                     static_cast<const unsigned short*>(in), to_lay(lin), w, bias, out, to_lay(lout), C, N, Ho, Wo, stride);
}

}  // namespace rtpose

using namespace rtpose;

extern "C" {

int rtpose_nchw_to_layout_affine(const float* src, float* dst, const rtpose_layout* ldst, int C, int cpad,
                                 int N, int H, int W, const float* scale, const float* shift,
                                 void* stream) {
  if (cpad < C || ldst->choff + cpad > ldst->cstride || (scale && !shift))
    return fail(RTPOSE_E_INVAL, "nchw_to_layout_affine: bad arguments");
  return launch_flat(nchw_to_layout_affine_kernel, (size_t)N * H * W * cpad, stream, src, dst, to_lay(ldst), C, cpad, N,
                     H, W, scale, shift);
}

int rtpose_stem_conv3x3_s2(const float* in, const rtpose_layout* lin, const float* w, const float* bias,
                           float* out, const rtpose_layout* lout, int cin_pad, int cout, int N, int H,
                           int W, int relu, void* stream) {
  if ((cout % 4) || !slice_aligned(lout, 4) || lin->ws < W + 1 || lin->hs < H + 1 ||
      lin->lead < lin->ws + 1 || lin->choff + cin_pad > lin->cstride)
    return fail(RTPOSE_E_INVAL, "stem_conv: unsupported layout / channel count");
  if (cin_pad != 8 || cout != 24 || !slice_aligned(lin, 4))
    return fail(RTPOSE_E_INVAL, "stem_conv: only cin_pad = 8, cout = 24 is instantiated");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return launch_flat(stem_conv3x3_s2_kernel<24>, (size_t)N * Ho * Wo, stream, in, to_lay(lin), w, bias, out, to_lay(lout),
                     N, Ho, Wo, relu);
}

int rtpose_stem_conv3x3_s2_nchw(const float* x_nchw, const float* scale, const float* shift, const float* w,
                                const float* bias, float* out, const rtpose_layout* lout, int cout, int N, int H,
                                int W, int relu, void* stream) {
  return rtpose_stem_conv3x3_s2_nchw_ex(x_nchw, scale, shift, w, bias, out, lout, cout, N, H, W, relu, 0, stream);
}

int rtpose_stem_conv3x3_s2_nchw_ex(const float* x_nchw, const float* scale, const float* shift, const float* w,
                                   const float* bias, void* out_v, const rtpose_layout* lout, int cout, int N,
                                   int H, int W, int relu, int out_bf16, void* stream) {
  if (cout != 24 || !slice_aligned(lout, out_bf16 ? 8 : 4))
    return fail(RTPOSE_E_INVAL, "stem_conv3x3_s2_nchw: only cout=24 (ShuffleNetV2 x1.0) is instantiated");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return launch_flat(stem_conv3x3_s2_nchw_kernel<24>, (size_t)N * Ho * Wo, stream, x_nchw, scale, shift, w, bias,
                     static_cast<float*>(out_v), to_lay(lout), N, H, W, Ho, Wo, relu, out_bf16 ? 1 : 0);
}

int rtpose_stem_pool_nchw(const float* x_nchw, const float* scale, const float* shift, const float* w,
                          const float* bias, void* out, const rtpose_layout* lout, int cout, int N, int H, int W,
                          int out_bf16, void* stream) {
  if (!x_nchw || !w || !bias || !out || !lout) return fail(RTPOSE_E_INVAL, "stem_pool: NULL argument");
  if (cout != 24 || !slice_aligned(lout, out_bf16 ? 8 : 4) || lout->choff + 24 > lout->cstride || (scale && !shift))
    return fail(RTPOSE_E_INVAL, "stem_pool: only cout=24 (ShuffleNetV2 x1.0), 16-byte aligned output slice");
  if (N <= 0 || H < 8 || W < 8) return fail(RTPOSE_E_INVAL, "stem_pool: need N >= 1, H, W >= 8");
  const int H1 = (H - 1) / 2 + 1, W1 = (W - 1) / 2 + 1;              // conv 3x3 s2 p1
  const int H2 = (H1 - 3 + 1) / 2 + 1, W2 = (W1 - 3 + 1) / 2 + 1;    // max-pool 3/2, ceil mode
  const dim3 grid(ceil_div(W2, kSpT), ceil_div(H2, kSpT), N);
  // rows as aligned float4 when the image allows it (every row starts on a 16-byte boundary)
  const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(x_nchw) % 16 == 0;
#define RTPOSE_STEM_POOL(B, V)                                                                                         \
  hipLaunchKernelGGL((stem_pool_kernel<B, V>), grid, dim3(256), 0, as_stream(stream), x_nchw, scale, shift, w, bias, \
                     out, to_lay(lout), H, W, H1, W1, H2, W2)
  if (out_bf16) {
    if (vec) RTPOSE_STEM_POOL(1, 1); else RTPOSE_STEM_POOL(1, 0);
  } else {
    if (vec) RTPOSE_STEM_POOL(0, 1); else RTPOSE_STEM_POOL(0, 0);
  }
#undef RTPOSE_STEM_POOL
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_maxpool3x3s2_ceil(const float* in, const rtpose_layout* lin, float* out, const rtpose_layout* lout,
                             int C, int N, int H, int W, void* stream) {
  return maxpool3x3s2_ceil<float>("maxpool3x3s2", in, lin, out, lout, C, N, H, W, stream);
}
int rtpose_maxpool3x3s2_ceil_bf16(const void* in, const rtpose_layout* lin, void* out, const rtpose_layout* lout,
                                  int C, int N, int H, int W, void* stream) {
  return maxpool3x3s2_ceil<unsigned short>("maxpool3x3s2_bf16", in, lin, out, lout, C, N, H, W, stream);
}

int rtpose_dwconv3x3(const float* in, const rtpose_layout* lin, const float* w, const float* bias, float* out,
                     const rtpose_layout* lout, int C, int N, int H, int W, int stride, void* stream) {
  return dwconv3x3<float>("dwconv3x3", in, lin, w, bias, out, lout, C, N, H, W, stride, stream);
}
int rtpose_dwconv3x3_bf16(const void* in, const rtpose_layout* lin, const float* w, const float* bias, void* out,
                          const rtpose_layout* lout, int C, int N, int H, int W, int stride, void* stream) {
  return dwconv3x3<unsigned short>("dwconv3x3_bf16", in, lin, w, bias, out, lout, C, N, H, W, stride, stream);
}
int rtpose_dwconv3x3_bf16_f32(const void* in, const rtpose_layout* lin, const float* w, const float* bias, float* out,
                              const rtpose_layout* lout, int C, int N, int H, int W, int stride, void* stream) {
  return dwconv3x3_bf16_f32("dwconv3x3_bf16_f32", in, lin, w, bias, out, lout, C, N, H, W, stride, stream);
}

int rtpose_layout_copy_cmap(const float* src, const rtpose_layout* lsrc, float* dst, const rtpose_layout* ldst,
                            int C, const int32_t* cmap, int N, int H, int W, void* stream) {
  if (!cmap) return fail(RTPOSE_E_INVAL, "layout_copy_cmap: cmap is NULL");
  // the source slice may be read 16 bytes at a time when it is aligned and either a
  // multiple of 4 wide or followed by readable (padding) channels inside the pixel
  const bool vec = slice_aligned(lsrc, 4) && lsrc->choff + ((C + 3) & ~3) <= lsrc->cstride;
  return launch_flat(vec ? layout_copy_cmap_vec_kernel<float> : layout_copy_cmap_kernel,
                     (size_t)N * H * W * (vec ? (C + 3) / 4 : C), stream, src, to_lay(lsrc), dst, to_lay(ldst), C, cmap,
                     N, H, W);
}
int rtpose_layout_copy_cmap_bf16(const void* src, const rtpose_layout* lsrc, void* dst, const rtpose_layout* ldst,
                                 int C, const int32_t* cmap, int N, int H, int W, void* stream) {
  if (!cmap || !slice_aligned(lsrc, 8))
    return fail(RTPOSE_E_INVAL, "layout_copy_cmap_bf16: cmap is NULL or the source slice is not 16-byte aligned");
  return launch_flat(layout_copy_cmap_vec_kernel<unsigned short>, (size_t)N * H * W * ((C + 7) / 8), stream,
                     static_cast<const unsigned short*>(src), to_lay(lsrc), static_cast<unsigned short*>(dst),
                     to_lay(ldst), C, cmap, N, H, W);
}

}  // extern "C"
