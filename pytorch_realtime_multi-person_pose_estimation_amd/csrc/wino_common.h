// Helpers shared by the two Winograd kernels (conv_wino.hip, conv_wino7.hip): packed-pair arithmetic for the
// input transforms and raw buffer loads for every global operand of the multiply loops.
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_dev.h"

namespace rtpose {
namespace winoc {

typedef floatx2 f2;

// 16 bytes as two packed pairs: the transform below is written on float2 so that it compiles to
// v_pk_fma_f32 / v_pk_add_f32 (fp32 VALU instructions take their cycles from the SAME ALUs the fp32 MFMAs
// run on - tools/exp/mfma_issue.hip: 64 -> 101 cycles per MFMA with 4 v_fma_f32 after each, at one or two
// waves per SIMD alike - so every VALU instruction in the multiply loop is paid for in matrix throughput).
struct F4 {
  f2 lo, hi;
};
__device__ __forceinline__ F4 fma4(float s, F4 a, F4 b) {  // s * a + b, one rounding
  const f2 ss = {s, s};
  return F4{__builtin_elementwise_fma(ss, a.lo, b.lo), __builtin_elementwise_fma(ss, a.hi, b.hi)};
}
__device__ __forceinline__ F4 mul4(float s, F4 a) {
  const f2 ss = {s, s};
  return F4{ss * a.lo, ss * a.hi};
}
__device__ __forceinline__ F4 add4(F4 a, F4 b) { return F4{a.lo + b.lo, a.hi + b.hi}; }
__device__ __forceinline__ F4 sub4(F4 a, F4 b) { return F4{a.lo - b.lo, a.hi - b.hi}; }
__device__ __forceinline__ float4 to_float4(F4 a) { return make_float4(a.lo.x, a.lo.y, a.hi.x, a.hi.y); }

// Raw buffer accesses (mfma_dev.h: make_rsrc and the 16-byte forms), as the packed pairs of the transforms and one dword
// at a time.
__device__ void llvm_raw_buffer_store_f32(float v, i32x4 rsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.store.f32");
// one dword per lane; a lane whose voff is >= the descriptor's range (kNoStore > kMaxRange) stores nothing: masked
// stores without a branch around them
constexpr unsigned kNoStore = 0x7fffffffu;
__device__ __forceinline__ void bstore(float v, i32x4 r, unsigned voff, unsigned soff) {
  llvm_raw_buffer_store_f32(v, r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ F4 bload(i32x4 r, unsigned voff, unsigned soff) {
  const floatx4 v = llvm_raw_buffer_load_v4f32(r, (int)voff, (int)soff, 0);
  return F4{f2{v.x, v.y}, f2{v.z, v.w}};
}

}  // namespace winoc
}  // namespace rtpose
