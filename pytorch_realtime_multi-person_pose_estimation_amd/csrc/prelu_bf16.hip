// PReLU between the bf16 convs of a layout-resident training run (header section 2b, continued; train.dense_stage): the
// forward from a conv's fp32 PRE-activation z straight into the bf16 slice the next conv reads, and the backward from the
// same z and the fp32 data gradient(s) of the conv(s) that read that slice, straight into the bf16 gradient the conv below
// takes its weight and data gradients from.
//
//   rtpose_prelu_bf16       y[n,y,x,c]   = bf16(prelu1(z, slope[c]))                  (common.h: the fused epilogue's bits)
//   rtpose_prelu_grad_bf16  g            = gb ? ga + gb : ga                          (one fp32 add: two consumers)
//                           out[n,y,x,c] = bf16(z > 0 ? g : slope[c] * g)             (torch's prelu_backward)
//                           dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * g)
//
// bf16(): round to nearest even as rtpose_layout_f32_to_bf16 rounds (the compiler's fp32 -> __bf16 conversion: Inf stays
// Inf, a NaN stays a NaN of its sign).  The fp32 values rounded are those rtpose_prelu / rtpose_prelu_grad store, so the
// bits are those of either followed by rtpose_layout_f32_to_bf16.
// One kernel template, memory bound, on the slabs, rectangle and units of chan_slab.h, two pixels in flight; the walk, the
// thread's order of additions and the row-order / slab-order sums are prelu_backward.hip's, so dslope has the bits
// rtpose_prelu_grad gives on the summed gradient where both take the 4-channel units.  A pass without sums takes kSlabUnit
// pixels per workgroup.  V = 4: 16-byte loads of z / ga / gb and one 8-byte store of 4 bf16; V = 1 otherwise.  No LDS but
// the row sum's, no scratch, no atomics.  fp32, one rounding per product and per sum (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "chan_slab.h"

namespace rtpose {
namespace {

constexpr int kReduceThreads = 64;

typedef uint32_t Word2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t f32_to_bf16_rne(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

// slabs * channels, rounded up to 4
size_t ws_floats(int channels, const SlabGeom& g) { return round_up((size_t)g.slabs * (size_t)channels, 4); }

struct PreluBf16Args {
  const float* z;
  const float* slope;
  const float* ga;  // backward only
  const float* gb;  // backward with two consumers only
  uint16_t* out;    // y of the forward
  float* ws;        // [slab][channels] partials, or NULL
  Lay lz, lga, lgb, lout;
  int channels, H, W, P;
  int slab;
  Rect r;
  FastDiv d_w, d_h;
};

// the V channels of a unit rounded to bf16 at element offset o: one 8-byte store of a whole unit, else its live channels
template <int V>
__device__ __forceinline__ void store_bf16(uint16_t* dst, size_t o, const Place& t, const Unit<V>& u) {
  if constexpr (V == 4) {
    if (t.whole) {
      *reinterpret_cast<Word2*>(dst + o) = Word2{f32_to_bf16_rne(u.v[0]) | (f32_to_bf16_rne(u.v[1]) << 16),
                                                 f32_to_bf16_rne(u.v[2]) | (f32_to_bf16_rne(u.v[3]) << 16)};
      return;
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (v < t.nc) dst[o + v] = (uint16_t)f32_to_bf16_rne(u.v[v]);
}

// V: channels per unit.  GRAD: the backward (else y = prelu1(z, slope)).  TWO: g = ga + gb.  SUM: with the slope-gradient
// partials.
template <int V, bool GRAD, bool TWO, bool SUM>
__global__ __launch_bounds__(kThreads) void prelu_bf16_kernel(const PreluBf16Args a) {
  const Place t = place<V>(a.r, a.channels, a.slab, a.P);

  float sl[V], acc[1][V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    sl[v] = (t.live && v < t.nc) ? a.slope[t.c0 + v] : 0.f;
    acc[0][v] = 0.f;
  }

  struct Offs {
    size_t z, ga, gb, out;
  };
  auto pixel = [&](int p) {
    const Pixel q = pixel_of(p, a.H, a.W, a.d_h, a.d_w);
    Offs o;
    o.z = lay_off(a.lz, q) + t.c0;
    o.out = lay_off(a.lout, q) + t.c0;
    o.ga = GRAD ? lay_off(a.lga, q) + t.c0 : 0;
    o.gb = TWO ? lay_off(a.lgb, q) + t.c0 : 0;
    return o;
  };
  auto finish = [&](size_t oo, const Unit<V>& zv, const Unit<V>& av, const Unit<V>& bv) {
    Unit<V> r;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (GRAD) {
        const float g = TWO ? av.v[v] + bv.v[v] : av.v[v];
        const bool pos = zv.v[v] > 0.f;  // torch's rule: z == 0 and NaN z take the slope path
        r.v[v] = __uint_as_float(pos ? __float_as_uint(g) : __float_as_uint(sl[v] * g));
        if (SUM) acc[0][v] += pos ? 0.f : zv.v[v] * g;
      } else {
        r.v[v] = prelu1(zv.v[v], sl[v]);
      }
    }
    store_bf16<V>(a.out, oo, t, r);
  };

  if (t.live) {
    // two pixels in flight: both are fetched before either is stored
    for (int p = t.p0 + t.row; p < t.p1; p += 2 * a.r.ty) {
      const int q = p + a.r.ty;
      const bool second = q < t.p1;
      const Offs o0 = pixel(p), o1 = pixel(second ? q : p);  // (the last pixel of an odd walk is fetched twice, stored once)
      const Unit<V> z0 = fetch<V>(a.z, o0.z, t), z1 = fetch<V>(a.z, o1.z, t);
      Unit<V> a0 = z0, a1 = z1, b0 = z0, b1 = z1;
      if (GRAD) a0 = fetch<V>(a.ga, o0.ga, t), a1 = fetch<V>(a.ga, o1.ga, t);
      if (TWO) b0 = fetch<V>(a.gb, o0.gb, t), b1 = fetch<V>(a.gb, o1.gb, t);
      finish(o0.out, z0, a0, b0);
      if (second) finish(o1.out, z1, a1, b1);
    }
  }

  if constexpr (SUM) sum_rows<V, 1, 1>(t, a.r, acc, a.ws, a.channels);
}

// thread c < channels
__global__ __launch_bounds__(kReduceThreads) void prelu_grad_bf16_reduce_kernel(const float* __restrict__ ws, int slabs,
                                                                              int channels, float* __restrict__ dslope) {
  const int c = (int)blockIdx.x * kReduceThreads + threadIdx.x;
  if (c >= channels) return;
  float v[1];
  sum_slabs<1, 8>(ws, slabs, 1, channels, 0, c, v);
  dslope[c] = v[0];
}

// 8-byte pieces of 4 bf16: every pixel's slice starts on one
bool aligned8_bf16(const rtpose_layout& l, const void* base) {
  return slice_aligned(l, 4) && reinterpret_cast<uintptr_t>(base) % 8 == 0;
}

// the bytes [first, last) the valid pixels' slices of a layout of `esize`-byte elements span
void span_bytes(const void* base, const rtpose_layout& l, int esize, int channels, int N, int H, int W, uintptr_t& first,
                uintptr_t& last) {
  const size_t lo = (size_t)l.lead * l.cstride + l.choff;
  const size_t hi = ((size_t)l.lead + ((size_t)(N - 1) * l.hs + (H - 1)) * l.ws + (W - 1)) * l.cstride + l.choff + channels;
  first = reinterpret_cast<uintptr_t>(base) + (size_t)esize * lo;
  last = reinterpret_cast<uintptr_t>(base) + (size_t)esize * hi;
}

// the bf16 slice out / lout against the bytes [i0, i1) of an input; 0 or fail(...)
int check_apart(const char* who, const char* what, const void* out, const rtpose_layout& lout, uintptr_t i0, uintptr_t i1,
                int channels, int N, int H, int W) {
  uintptr_t o0, o1;
  span_bytes(out, lout, 2, channels, N, H, W, o0, o1);
  if (o1 <= i0 || i1 <= o0) return 0;
  return fail(RTPOSE_E_INVAL, "%s: the bytes of the bf16 destination overlap those of %s", who, what);
}

int check_apart_slice(const char* who, const char* what, const void* out, const rtpose_layout& lout, const float* in,
                      const rtpose_layout& lin, int channels, int N, int H, int W) {
  uintptr_t i0, i1;
  span_bytes(in, lin, 4, channels, N, H, W, i0, i1);
  return check_apart(who, what, out, lout, i0, i1, channels, N, H, W);
}

// what both entry points ask of their bf16 destination beside check_slice; 0 or fail(...)
int check_dest(const char* who, const char* what, const void* out, const rtpose_layout& lout, const float* z,
               const rtpose_layout& lz, const float* slope, int channels, int N, int H, int W) {
  if (reinterpret_cast<uintptr_t>(out) % 2) return fail(RTPOSE_E_INVAL, "%s: %s must be 2-byte aligned", who, what);
  if (int rc = check_apart_slice(who, "z", out, lout, z, lz, channels, N, H, W)) return rc;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(slope);
  return check_apart(who, "slope", out, lout, s0, s0 + 4 * (size_t)channels, channels, N, H, W);
}

// the arguments but the pointers of the gradients, the rectangle and the grid of either pass; 0 or fail(...)
int prelu_bf16_args(PreluBf16Args& a, dim3& grid, bool vec, bool sums, const char* who, const float* z, const rtpose_layout* lz,
                    const float* slope, void* out, const rtpose_layout* lout, int channels, int H, int W, long P) {
  const SlabGeom g = slab_geometry(P);
  a.z = z;
  a.slope = slope;
  a.ga = a.gb = nullptr;
  a.out = static_cast<uint16_t*>(out);
  a.ws = nullptr;
  a.lz = a.lga = a.lgb = to_lay(lz);
  a.lout = to_lay(lout);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = (int)P;
  a.slab = sums ? g.slab : kSlabUnit;  // the values of an element-wise pass do not depend on how the pixels are cut
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  const int xblocks = sums ? g.slabs : (int)((P + kSlabUnit - 1) / kSlabUnit);
  return set_rectangle(a.r, channels, vec ? 4 : 1, xblocks, grid, who);
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_prelu_grad_bf16_workspace_floats(int channels, int N, int H, int W) {
  if (channels < 1 || pixel_count(N, H, W) <= 0) return 0;
  return ws_floats(channels, slab_geometry(pixel_count(N, H, W)));
}

int rtpose_prelu_grad_bf16_slabs(int channels, int N, int H, int W) {
  if (channels < 1 || pixel_count(N, H, W) <= 0) return 0;
  return slab_geometry(pixel_count(N, H, W)).slabs;
}

int rtpose_prelu_bf16(const float* z, const rtpose_layout* lz, const float* slope, void* y, const rtpose_layout* ly,
                      int channels, int N, int H, int W, void* stream) {
  const char* who = "prelu_bf16";
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "z", z, lz, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "y", y, ly, channels, H, W, 0)) return rc;
  if (!slope) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (slope)", who);
  if (int rc = check_dest(who, "y", y, *ly, z, *lz, slope, channels, N, H, W)) return rc;

  PreluBf16Args a;
  dim3 grid;
  const bool vec = aligned16(*lz, z) && aligned8_bf16(*ly, y);
  if (int rc = prelu_bf16_args(a, grid, vec, false, who, z, lz, slope, y, ly, channels, H, W, P)) return rc;

  static thread_local CheckedPtr c_z, c_s, c_y;
  const int dev = current_device();
  int rc = c_z.check(z, dev, who, "z");
  if (!rc) rc = c_s.check(slope, dev, who, "slope");
  if (!rc) rc = c_y.check(y, dev, who, "y");
  if (rc) return rc;

  launch_units<prelu_bf16_kernel<4, false, false, false>, prelu_bf16_kernel<1, false, false, false>>(vec, grid,
                                                                                                     as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_prelu_grad_bf16(const float* z, const rtpose_layout* lz, const float* slope, const float* ga,
                           const rtpose_layout* lga, const float* gb, const rtpose_layout* lgb, void* out,
                           const rtpose_layout* lout, float* dslope, float* workspace, size_t workspace_floats, int channels,
                           int N, int H, int W, void* stream) {
  const char* who = "prelu_grad_bf16";
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "z", z, lz, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "ga", ga, lga, channels, H, W, 0)) return rc;
  if (gb)  // (gb == NULL: one consumer, and lgb is not looked at)
    if (int rc = check_slice(who, "gb", gb, lgb, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "out", out, lout, channels, H, W, 0)) return rc;
  if (!slope) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (slope)", who);
  if (int rc = check_dest(who, "out", out, *lout, z, *lz, slope, channels, N, H, W)) return rc;
  if (int rc = check_apart_slice(who, "ga", out, *lout, ga, *lga, channels, N, H, W)) return rc;
  if (gb)
    if (int rc = check_apart_slice(who, "gb", out, *lout, gb, *lgb, channels, N, H, W)) return rc;
  const SlabGeom g = slab_geometry(P);
  if (dslope)  // (no dslope: no sums, and the workspace is not looked at)
    if (int rc = check_workspace(who, workspace, workspace_floats, ws_floats(channels, g),
                                 "rtpose_prelu_grad_bf16_workspace_floats"))
      return rc;

  PreluBf16Args a;
  dim3 grid;
  const bool vec = aligned16(*lz, z) && aligned16(*lga, ga) && (!gb || aligned16(*lgb, gb)) && aligned8_bf16(*lout, out);
  if (int rc = prelu_bf16_args(a, grid, vec, dslope != nullptr, who, z, lz, slope, out, lout, channels, H, W, P)) return rc;
  a.ga = ga;
  a.lga = to_lay(lga);
  if (gb) {
    a.gb = gb;
    a.lgb = to_lay(lgb);
  }
  a.ws = dslope ? workspace : nullptr;

  static thread_local CheckedPtr c_z, c_s, c_ga, c_gb, c_out, c_ds, c_ws;
  const int dev = current_device();
  int rc = c_z.check(z, dev, who, "z");
  if (!rc) rc = c_s.check(slope, dev, who, "slope");
  if (!rc) rc = c_ga.check(ga, dev, who, "ga");
  if (!rc && gb) rc = c_gb.check(gb, dev, who, "gb");
  if (!rc) rc = c_out.check(out, dev, who, "out");
  if (!rc && dslope) rc = c_ds.check(dslope, dev, who, "dslope");
  if (!rc && dslope) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if (dslope) {
    if (gb)
      launch_units<prelu_bf16_kernel<4, true, true, true>, prelu_bf16_kernel<1, true, true, true>>(vec, grid, s, a);
    else
      launch_units<prelu_bf16_kernel<4, true, false, true>, prelu_bf16_kernel<1, true, false, true>>(vec, grid, s, a);
    RTPOSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(prelu_grad_bf16_reduce_kernel, dim3((unsigned)ceil_div(channels, kReduceThreads)),
                       dim3(kReduceThreads), 0, s, (const float*)workspace, g.slabs, channels, dslope);
  } else if (gb) {
    launch_units<prelu_bf16_kernel<4, true, true, false>, prelu_bf16_kernel<1, true, true, false>>(vec, grid, s, a);
  } else {
    launch_units<prelu_bf16_kernel<4, true, false, false>, prelu_bf16_kernel<1, true, false, false>>(vec, grid, s, a);
  }
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
