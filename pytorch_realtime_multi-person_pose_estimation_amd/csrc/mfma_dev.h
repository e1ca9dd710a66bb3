// Device vocabulary of the forward MFMA kernels (conv_*.hip, pw_*.hip, unit_bf16.hip): the vector types of the MFMA
// operands, 16-byte loads and stores that stay off the FLAT path, the accumulator read-out, the bf16 bit helpers, the
// schedule pin and the decode of a batch pixel.  Every helper is __forceinline__ and written once here; the per-file
// namespaces keep what is their own.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace rtpose {

#ifdef __HIPCC__
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Schedule pin: a compiler memory barrier and a scheduling barrier - the instruction scheduler moves nothing across it, so
// loads, LDS traffic and MFMAs issue in the groups the source wrote them in.
#define RTPOSE_PIN()             \
  asm volatile("" ::: "memory"); \
  __builtin_amdgcn_sched_barrier(0)

// ---- 16 bytes through the global address space -------------------------------------------------------------------------
// Explicit address space: if clang loses track of a pointer's provenance it falls back to FLAT loads, which also tick
// lgkmcnt and drag every LDS read behind a full `s_waitcnt vmcnt(0) lgkmcnt(0)` (seen in the tap loop of conv_mfma.hip;
// cost several %).
typedef const floatx4 __attribute__((address_space(1)))* gcf4_t;
typedef floatx4 __attribute__((address_space(1)))* gf4_t;
__device__ __forceinline__ float4 gload4(const void* p) {
  const floatx4 v = *(gcf4_t)(unsigned long long)(p);
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void gstore4(void* p, const float4& v) {
  const floatx4 t = {v.x, v.y, v.z, v.w};
  *(gf4_t)(unsigned long long)(p) = t;
}

// ---- 16 bytes through a buffer resource ----------------------------------------------------------------------------------
// Raw buffer accesses: address = base (4 SGPRs) + per-lane byte offset (1 VGPR) + uniform byte offset (1 SGPR, advanced by
// the scalar unit): no vector instruction is spent on address arithmetic.  Bound to the LLVM intrinsics by name.
__device__ floatx4 llvm_raw_buffer_load_v4f32(i32x4 rsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void llvm_raw_buffer_store_v4f32(floatx4 v, i32x4 rsrc, int voffset, int soffset, int aux) __asm(
    "llvm.amdgcn.raw.buffer.store.v4f32");
// `bytes` = what is addressable from p (the rest of the tensor / packed filter the pointer lies in): the hardware
// clamps every access against it - an over-read returns zeros and an over-write is dropped instead of touching a
// neighbouring allocation (a weight prefetch that ran 3 ky steps past the packed filters once reached a committed
// kernel with the clamp off).  Descriptors are based at a block's own first element, so the 32-bit range only
// saturates for tensors beyond 2 GiB from there, which the per-lane offsets cannot reach anyway.
constexpr unsigned kMaxRange = 0x7ffffffeu;
__device__ __forceinline__ i32x4 make_rsrc(const void* p, size_t bytes) {
  union {
    struct {
      const void* p;
      unsigned range, cfg;
    } s;
    i32x4 v;
  } u;
  u.s.p = p;
  u.s.range = bytes < (size_t)kMaxRange ? (unsigned)bytes : kMaxRange;  // bytes addressable from p
  u.s.cfg = 0x00020000;                                                 // raw buffer, 32-bit data format
  return u.v;
}
__device__ __forceinline__ float4 bload4(i32x4 r, unsigned voff, unsigned soff) {
  const floatx4 v = llvm_raw_buffer_load_v4f32(r, (int)voff, (int)soff, 0);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void bstore4(const float4& v, i32x4 r, unsigned voff) {
  const floatx4 t = {v.x, v.y, v.z, v.w};
  llvm_raw_buffer_store_v4f32(t, r, (int)voff, 0, 0);
}
// the same load through the compiler's own resource type (conv_mfma_bf16.hip builds its descriptors with
// __builtin_amdgcn_make_buffer_rsrc)
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  const floatx4 v = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
  return make_float4(v[0], v[1], v[2], v[3]);
}

// ---- MFMA operands and accumulators ---------------------------------------------------------------------------------------
// 16 bytes as the 8 bf16 of one lane's share of a K = 16 step
__device__ __forceinline__ bf16x8 as_bf8(const float4& v) {
  const floatx4 t = {v.x, v.y, v.z, v.w};
  return __builtin_bit_cast(bf16x8, t);
}
// One accumulator register -> a VGPR, HERE.  The allocator otherwise moves a pass' whole accumulator tile (128 registers)
// out of the accumulator file right behind the last MFMA - the VALU cannot read AGPRs - and spills around it; read one
// at a time, a fragment's values are live for the length of its own conversion only.
__device__ __forceinline__ float acc_read(float a) {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
  return v;
}
// The compiler's hazard recogniser does not know that the asm above reads an MFMA result: the wait states between the last
// MFMA that wrote an accumulator and its first v_accvgpr_read (up to 18 for a 16-pass 32x32x16) are inserted by hand,
// once, in front of every read-out section.  (Found the hard way: registers 0 and 1 of the first fragment read stale
// values in one instance of unit_bf16_kernel whose epilogue followed the last MFMA directly.)
__device__ __forceinline__ void mfma_drain() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }
// ReLU on the bit pattern: a negative float (and -0) is a negative int, a positive one orders like its bits - one
// v_max_i32 where fmaxf costs a canonicalising v_max_f32 more (no NaN reaches here that the reference would keep)
__device__ __forceinline__ float relu_bits(float v) {
  return __builtin_bit_cast(float, max(__builtin_bit_cast(int, v), 0));
}

// ---- bf16 bits: round to nearest even (Inf stays Inf, a NaN stays a NaN of its sign), and back ----------------------------
__device__ __forceinline__ unsigned short f32_to_bf16_rne(float v) {
  return __builtin_bit_cast(unsigned short, (__bf16)v);  // v_cvt_pk_bf16_f32
}
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
// two bf16 as one 32-bit word, `a` in the low half
__device__ __forceinline__ unsigned bf16_pair(unsigned short a, unsigned short b) { return a | ((unsigned)b << 16); }
// (bf16(a), bf16(b)) in one dword, `a` in the low half.  Three spellings of one result (all round to nearest even and give
// the same bits), because the compiler schedules, and in one case selects, other instructions for each, and every kernel
// keeps the instruction sequence it was tuned and measured with:
//   pack_bf16x2         one vector conversion                      conv_mfma_bf16, conv_c64_bf16, conv_tail_bf16, pw_head_bf16
//   pack_bf16x2_scalar  two scalar conversions into a vector       unit_bf16 (the vector form moves its conversions behind
//                                                                  the accumulator reads of the next pair)
//   pack_bf16x2_bits    two 16-bit results joined by shift and or  pw_fused_bf16's depthwise instances (either other form
//                                                                  changes their instruction count: a change to measure
//                                                                  on its own, not part of sharing the helper)
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
  const floatx2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ unsigned pack_bf16x2_scalar(float a, float b) {
  const bf16x2 t = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, t);
}
__device__ __forceinline__ unsigned pack_bf16x2_bits(float a, float b) {
  return bf16_pair(f32_to_bf16_rne(a), f32_to_bf16_rne(b));
}
// 8 bf16 (one 16-byte piece) -> 8 floats
__device__ __forceinline__ void unpack8(const float4& p, float* f) {
  const unsigned u[4] = {__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), __float_as_uint(p.w)};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(u[i] << 16);
    f[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
  }
}

// ---- pixel m of the batch as (image, row, column), by the launch's FastDiv constants ---------------------------------------
struct Pix {
  int n, y, x;
};
__device__ __forceinline__ Pix pix_of(int m, int HW, int W, const FastDiv fHW, const FastDiv fW) {
  Pix p;
  p.n = fast_div(m, fHW);
  const int r = m - p.n * HW;
  p.y = fast_div(r, fW);
  p.x = r - p.y * W;
  return p;
}
__device__ __forceinline__ int lay_pix(const Lay l, const Pix& p) { return lay_pix(l, p.n, p.y, p.x); }
#endif

}  // namespace rtpose
