// What the data-movement kernels (layout_ops.hip, shufflenet_ops.hip, image_ops.hip) share: the decode of the flat thread
// index into a pixel and a channel group, the 16-byte channel vector of either element type (bf16 bits by mfma_dev.h), and on
// the host the one-dimensional launch and the alignment test of a layout slice.
#pragma once
#include <type_traits>

#include "common.h"
#include "mfma_dev.h"

namespace rtpose {

// ---- host: one thread per item, 256 per block ----
inline unsigned nblocks(size_t total, int threads) { return (unsigned)((total + threads - 1) / threads); }

// An empty call launches nothing and succeeds.
template <class K, class... A>
static int launch_flat(K kernel, size_t total, void* stream, A... args) {
  if (!total) return 0;
  hipLaunchKernelGGL(kernel, dim3(nblocks(total, 256)), dim3(256), 0, as_stream(stream), args...);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

// every pixel's slice of this layout starts on a multiple of k elements
inline bool slice_aligned(const rtpose_layout* l, int k) { return !(l->cstride % k) && !(l->choff % k); }

#ifdef __HIPCC__
// ---- 16 bytes of consecutive channels of element type T: 4 float, or 8 bf16 (unsigned short bits); lanes held as float ----
template <class T>
struct ChanVec {
  static constexpr bool kBf16 = std::is_same<T, unsigned short>::value;
  static_assert(kBf16 || std::is_same<T, float>::value, "float or bf16 bits");
  static constexpr int kLanes = kBf16 ? 8 : 4, kShift = kBf16 ? 3 : 2;  // C >> kShift channel groups
  float v[kLanes];

  static __device__ __forceinline__ ChanVec load(const T* p) {
    ChanVec r;
    if constexpr (kBf16) {
      const uint4 u = *reinterpret_cast<const uint4*>(p);
      const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r.v[2 * k] = __uint_as_float(w[k] << 16);
        r.v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
      }
    } else {
      const float4 t = *reinterpret_cast<const float4*>(p);
      r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    }
    return r;
  }
  // kLanes consecutive fp32 (a bias, a filter tap): the fp32 kernels read theirs as one 16-byte vector
  static __device__ __forceinline__ ChanVec load_f32(const float* p) {
    if constexpr (kBf16) {
      ChanVec r;
#pragma unroll
      for (int k = 0; k < kLanes; ++k) r.v[k] = p[k];
      return r;
    } else {
      return load(p);
    }
  }
  __device__ __forceinline__ void store(T* p) const {
    if constexpr (kBf16) {
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = bf16_pair(f32_to_bf16_rne(v[2 * k]), f32_to_bf16_rne(v[2 * k + 1]));
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
};
// the same 16 bytes as they are, for copies: no conversion touches a NaN's payload.  lane(k) is element k; the two
// element types keep the form their copies were written in (four floats; two 16-bit halves of each of four words)
template <class T>
struct ChanBits;
template <>
struct alignas(16) ChanBits<float> {
  float e[4];
  __device__ __forceinline__ float lane(int k) const { return e[k]; }
};
template <>
struct ChanBits<unsigned short> {
  uint4 u;
  __device__ __forceinline__ unsigned short lane(int k) const {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
    return (unsigned short)(w[k >> 1] >> (16 * (k & 1)));
  }
};

// ---- flat thread index -> pixel (n, y, x) and first channel c of the thread's group ----
struct Walk {
  size_t i;  // the flat index itself
  int n, y, x, c;
};
__device__ __forceinline__ void pixel_of(size_t p, int H, int W, Walk& q) {
  q.x = p % W;
  p /= W;
  q.y = p % H;
  q.n = p / H;
}
// `groups` channel groups of LANES channels per pixel, channel fastest (the layout side's order); PLANES: pixel fastest
// and group slowest, for coalesced reads of the channel planes of a dense NCHW source.  False past the end.  size_t
// throughout: the flat index passes 2^32.
template <int LANES = 1, bool PLANES = false>
__device__ __forceinline__ bool pixel_walk(int groups, int N, int H, int W, Walk& q) {
  const size_t total = (size_t)N * H * W * groups;
  q.i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q.i >= total) return false;
  if (PLANES) {
    q.c = (int)(q.i / ((size_t)N * H * W)) * LANES;
    pixel_of(q.i % ((size_t)N * H * W), H, W, q);
  } else {
    q.c = (q.i % groups) * LANES;
    pixel_of(q.i / groups, H, W, q);
  }
  return true;
}
// one thread per pixel, no channel
__device__ __forceinline__ bool pixel_walk(int N, int H, int W, Walk& q) {
  const size_t total = (size_t)N * H * W;
  q.i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q.i >= total) return false;
  q.c = 0;
  pixel_of(q.i, H, W, q);
  return true;
}
// the element order of a dense NCHW tensor: x fastest, then y, channel, image (coalesced on the NCHW side)
__device__ __forceinline__ bool nchw_walk(int C, int N, int H, int W, Walk& q) {
  const size_t total = (size_t)N * C * H * W;
  q.i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q.i >= total) return false;
  q.x = q.i % W;
  size_t p = q.i / W;
  q.y = p % H;
  p /= H;
  q.c = p % C;
  q.n = p / C;
  return true;
}
__device__ __forceinline__ size_t lay_off(const Lay& l, const Walk& q) { return lay_off(l, q.n, q.y, q.x); }
#endif

}  // namespace rtpose
