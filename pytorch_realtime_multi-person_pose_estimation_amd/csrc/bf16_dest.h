// The bf16 destination of the training passes that round at their store (prelu_backward.hip's and batchnorm.hip's *_bf16
// entry points): a unit's store, the alignment that lets it be one 8-byte store, and the host's test that the destination's
// bytes lie apart from every input's - such a pass never runs in place.
#pragma once
#include "chan_slab.h"
#include "mfma_dev.h"

namespace rtpose {

typedef uint32_t Word2 __attribute__((ext_vector_type(2)));

// the V channels of a unit rounded to bf16 at element offset o: one 8-byte store of a whole unit, else its live channels
template <int V>
__device__ __forceinline__ void store_bf16(uint16_t* dst, size_t o, const Place& t, const Unit<V>& u) {
  if constexpr (V == 4) {
    if (t.whole) {
      *reinterpret_cast<Word2*>(dst + o) = Word2{f32_to_bf16_rne(u.v[0]) | ((uint32_t)f32_to_bf16_rne(u.v[1]) << 16),
                                                 f32_to_bf16_rne(u.v[2]) | ((uint32_t)f32_to_bf16_rne(u.v[3]) << 16)};
      return;
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (v < t.nc) dst[o + v] = f32_to_bf16_rne(u.v[v]);
}

// 8-byte pieces of 4 bf16: every pixel's slice starts on one
inline bool aligned8_bf16(const rtpose_layout& l, const void* base) {
  return slice_aligned(l, 4) && reinterpret_cast<uintptr_t>(base) % 8 == 0;
}

// the bf16 slice out / lout against the bytes [i0, i1) of an input: apart, never in place; 0 or fail(...)
inline int check_apart(const char* who, const char* what, const void* out, const rtpose_layout& lout, uintptr_t i0,
                       uintptr_t i1, int channels, int N, int H, int W) {
  uintptr_t o0, o1;
  slice_span_bytes(out, lout, 2, channels, N, H, W, o0, o1);
  if (o1 <= i0 || i1 <= o0) return 0;
  return fail(RTPOSE_E_INVAL, "%s: the bytes of the bf16 destination overlap those of %s", who, what);
}

inline int check_apart_slice(const char* who, const char* what, const void* out, const rtpose_layout& lout, const float* in,
                             const rtpose_layout& lin, int channels, int N, int H, int W) {
  uintptr_t i0, i1;
  slice_span_bytes(in, lin, 4, channels, N, H, W, i0, i1);
  return check_apart(who, what, out, lout, i0, i1, channels, N, H, W);
}

// a per-channel fp32 vector of `floats` values against the bf16 slice
inline int check_apart_vector(const char* who, const char* what, const void* out, const rtpose_layout& lout, const float* in,
                              size_t floats, int channels, int N, int H, int W) {
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(in);
  return check_apart(who, what, out, lout, s0, s0 + 4 * floats, channels, N, H, W);
}

}  // namespace rtpose
