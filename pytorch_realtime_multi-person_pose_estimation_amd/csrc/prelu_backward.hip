// PReLU as a pass of its own, for training (header section 2b): the forward from a conv's PRE-activation z and the
// backward from the same z.  The inference kernels fuse y = z >= 0 ? z : slope[c] * z into the conv epilogue and keep only
// y; with slopes of either sign sign(y) says nothing about sign(z), so a training forward launches the conv without an
// activation, keeps z and runs rtpose_prelu, and the backward runs rtpose_prelu_grad on z.
//
//   rtpose_prelu       y[n,y,x,c]   = prelu1(z, slope[c])                  (common.h: the fused epilogue's bits)
//   rtpose_prelu_grad  out[n,y,x,c] = z > 0 ? gy : slope[c] * gy           (torch's prelu_backward; gy's bits where z > 0)
//                      dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * gy)
//
// and the same two passes between the bf16 convs of a layout-resident training run (train.dense_stage): from the fp32 z
// straight into the bf16 slice the next conv reads, and from z and the fp32 data gradient(s) of the conv(s) that read that
// slice straight into the bf16 gradient the conv below takes its weight and data gradients from.
//
//   rtpose_prelu_bf16       y[n,y,x,c]   = bf16(prelu1(z, slope[c]))
//   rtpose_prelu_grad_bf16  g            = gb ? ga + gb : ga                          (one fp32 add: two consumers)
//                           out[n,y,x,c] = bf16(z > 0 ? g : slope[c] * g)
//                           dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * g)
//
// bf16(): round to nearest even as rtpose_layout_f32_to_bf16 rounds (the compiler's fp32 -> __bf16 conversion: Inf stays
// Inf, a NaN stays a NaN of its sign).  The fp32 values rounded are those rtpose_prelu / rtpose_prelu_grad store, so the
// bits are those of either followed by rtpose_layout_f32_to_bf16.
//
// One kernel template for all four, memory bound, on the slabs, rectangle and units of chan_slab.h, two pixels in flight.
// z and the gradients are read once: the thread adds its z * g terms in its pixel order, chan_slab.h's row-order and
// slab-order sums (one term, fp32) make dslope of them, overwriting it - so dslope of the bf16 pass has the bits
// rtpose_prelu_grad gives on the summed gradient where both take the 4-channel units.  V = 4: 16-byte loads of z / ga / gb
// and one 16-byte store of 4 floats or one 8-byte store of 4 bf16; V = 1 otherwise.  No LDS but the row sum's, no scratch,
// no atomics.  fp32, one rounding per product and per sum (the library is built with -ffp-contract=off: slope * g and z * g
// are single multiplies, never part of an fma).
//
// Three things differ between the fp32 and the bf16 entry points on purpose.  They were decided when each was written, not by
// the change that put them into one file, and none is this file's to unify:
//   * aliasing: every element reads only its own gy element, so the fp32 out / lout may name the slice gy / lgy name.  The
//     bf16 destination must lie bytes apart from every input (check_dest; bf16_dest.h) and be 2-byte aligned;
//   * grid: the fp32 passes take slab_geometry's slab and slab count with or without sums, the bf16 element-wise passes (no
//     sums) kSlabUnit pixels per workgroup.  The values do not depend on it;
//   * the 4-channel units: aligned16 on every fp32 slice; aligned8_bf16 on the bf16 destination.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bf16_dest.h"
#include "chan_slab.h"
#include "pixel_walk.h"

namespace rtpose {
namespace {

constexpr int kReduceThreads = 64;

bool shape_ok(int channels, int N, int H, int W) { return channels >= 1 && pixel_count(N, H, W) > 0; }

// slabs * channels, rounded up to 4
size_t ws_floats(int channels, const SlabGeom& g) { return round_up((size_t)g.slabs * (size_t)channels, 4); }

struct PreluArgs {
  const float* z;
  const float* slope;
  const float* ga;  // backward only
  const float* gb;  // backward with two consumers only
  void* out;        // y of the forward: float or bf16
  float* ws;        // [slab][channels] partials, or NULL
  Lay lz, lga, lgb, lout;
  int channels, H, W, P;
  int slab;
  Rect r;
  FastDiv d_w, d_h;
};

// V: channels per unit.  OUT: float, or uint16_t for a bf16 destination.  GRAD: the backward (else y = prelu1(z, slope)).
// TWO: g = ga + gb.  SUM: with the slope-gradient partials.
template <int V, class OUT, bool GRAD, bool TWO, bool SUM>
__global__ __launch_bounds__(kThreads) void prelu_kernel(const PreluArgs a) {
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
    if constexpr (std::is_same_v<OUT, float>)
      store<V>(static_cast<float*>(a.out), oo, t, r);
    else
      store_bf16<V>(static_cast<uint16_t*>(a.out), oo, t, r);
  };

  if (t.live) {
    // two pixels in flight: both are fetched before either is stored (the fp32 out may be gy: an element reads only itself)
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
__global__ __launch_bounds__(kReduceThreads) void prelu_grad_reduce_kernel(const float* __restrict__ ws, int slabs,
                                                                         int channels, float* __restrict__ dslope) {
  const int c = (int)blockIdx.x * kReduceThreads + threadIdx.x;
  if (c >= channels) return;
  float v[1];
  sum_slabs<1, 8>(ws, slabs, 1, channels, 0, c, v);
  dslope[c] = v[0];
}

// what the bf16 entry points ask of their destination beside check_slice; 0 or fail(...)
int check_dest(const char* who, const char* what, const void* out, const rtpose_layout& lout, const float* z,
               const rtpose_layout& lz, const float* slope, int channels, int N, int H, int W) {
  if (reinterpret_cast<uintptr_t>(out) % 2) return fail(RTPOSE_E_INVAL, "%s: %s must be 2-byte aligned", who, what);
  if (int rc = check_apart_slice(who, "z", out, lout, z, lz, channels, N, H, W)) return rc;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(slope);
  return check_apart(who, "slope", out, lout, s0, s0 + 4 * (size_t)channels, channels, N, H, W);
}

// the arguments but the gradients' and the workspace's, the rectangle and the grid of either pass; unit_slabs: kSlabUnit
// pixels per workgroup instead of slab_geometry's slabs; 0 or fail(...)
int prelu_args(PreluArgs& a, dim3& grid, bool vec, bool unit_slabs, const char* who, const float* z, const rtpose_layout* lz,
               const float* slope, void* out, const rtpose_layout* lout, int channels, int H, int W, long P) {
  const SlabGeom g = slab_geometry(P);
  a.z = z;
  a.slope = slope;
  a.ga = a.gb = nullptr;
  a.out = out;
  a.ws = nullptr;
  a.lz = a.lga = a.lgb = to_lay(lz);
  a.lout = to_lay(lout);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = (int)P;
  a.slab = unit_slabs ? kSlabUnit : g.slab;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  const int xblocks = unit_slabs ? (int)((P + kSlabUnit - 1) / kSlabUnit) : g.slabs;
  return set_rectangle(a.r, channels, vec ? 4 : 1, xblocks, grid, who);
}

size_t prelu_ws_query(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return ws_floats(channels, slab_geometry(pixel_count(N, H, W)));
}

int prelu_slabs_query(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return slab_geometry(pixel_count(N, H, W)).slabs;
}

// rtpose_prelu (OUT = float) and rtpose_prelu_bf16 (OUT = uint16_t)
template <class OUT>
int prelu_forward(const char* who, const float* z, const rtpose_layout* lz, const float* slope, void* y,
                  const rtpose_layout* ly, int channels, int N, int H, int W, void* stream) {
  constexpr bool kBf16 = !std::is_same_v<OUT, float>;
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "z", z, lz, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "y", y, ly, channels, H, W, 0)) return rc;
  if (!slope) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (slope)", who);
  if constexpr (kBf16)
    if (int rc = check_dest(who, "y", y, *ly, z, *lz, slope, channels, N, H, W)) return rc;

  PreluArgs a;
  dim3 grid;
  const bool vec = aligned16(*lz, z) && (kBf16 ? aligned8_bf16(*ly, y) : aligned16(*ly, y));
  if (int rc = prelu_args(a, grid, vec, kBf16, who, z, lz, slope, y, ly, channels, H, W, P)) return rc;

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_z, c_s, c_y;
  const int dev = current_device();
  int rc = c_z.check(z, dev, who, "z");
  if (!rc) rc = c_s.check(slope, dev, who, "slope");
  if (!rc) rc = c_y.check(y, dev, who, "y");
  if (rc) return rc;

  launch_units<prelu_kernel<4, OUT, false, false, false>, prelu_kernel<1, OUT, false, false, false>>(vec, grid,
                                                                                                     as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

template <class OUT, bool TWO, bool SUM>
void launch_grad(bool vec, dim3 grid, hipStream_t s, const PreluArgs& a) {
  launch_units<prelu_kernel<4, OUT, true, TWO, SUM>, prelu_kernel<1, OUT, true, TWO, SUM>>(vec, grid, s, a);
}

// rtpose_prelu_grad (OUT = float; its one gradient is "gy", gb = NULL) and rtpose_prelu_grad_bf16 (OUT = uint16_t)
template <class OUT>
int prelu_backward(const char* who, const char* ga_name, const char* reporter, const float* z, const rtpose_layout* lz,
                   const float* slope, const float* ga, const rtpose_layout* lga, const float* gb, const rtpose_layout* lgb,
                   void* out, const rtpose_layout* lout, float* dslope, float* workspace, size_t workspace_floats, int channels,
                   int N, int H, int W, void* stream) {
  constexpr bool kBf16 = !std::is_same_v<OUT, float>;
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "z", z, lz, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, ga_name, ga, lga, channels, H, W, 0)) return rc;
  if (gb)  // (gb == NULL: one consumer, and lgb is not looked at)
    if (int rc = check_slice(who, "gb", gb, lgb, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "out", out, lout, channels, H, W, 0)) return rc;
  if (!slope) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (slope)", who);
  if constexpr (kBf16) {
    if (int rc = check_dest(who, "out", out, *lout, z, *lz, slope, channels, N, H, W)) return rc;
    if (int rc = check_apart_slice(who, ga_name, out, *lout, ga, *lga, channels, N, H, W)) return rc;
    if (gb)
      if (int rc = check_apart_slice(who, "gb", out, *lout, gb, *lgb, channels, N, H, W)) return rc;
  }
  const SlabGeom g = slab_geometry(P);
  if (dslope)  // (no dslope: no sums, and the workspace is not looked at)
    if (int rc = check_workspace(who, workspace, workspace_floats, ws_floats(channels, g), reporter)) return rc;

  PreluArgs a;
  dim3 grid;
  const bool vec = aligned16(*lz, z) && aligned16(*lga, ga) && (!gb || aligned16(*lgb, gb)) &&
                   (kBf16 ? aligned8_bf16(*lout, out) : aligned16(*lout, out));
  if (int rc = prelu_args(a, grid, vec, kBf16 && !dslope, who, z, lz, slope, out, lout, channels, H, W, P)) return rc;
  a.ga = ga;
  a.lga = to_lay(lga);
  if (gb) {
    a.gb = gb;
    a.lgb = to_lay(lgb);
  }
  a.ws = dslope ? workspace : nullptr;

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_z, c_s, c_ga, c_gb, c_out, c_ds, c_ws;
  const int dev = current_device();
  int rc = c_z.check(z, dev, who, "z");
  if (!rc) rc = c_s.check(slope, dev, who, "slope");
  if (!rc) rc = c_ga.check(ga, dev, who, ga_name);
  if (!rc && gb) rc = c_gb.check(gb, dev, who, "gb");
  if (!rc) rc = c_out.check(out, dev, who, "out");
  if (!rc && dslope) rc = c_ds.check(dslope, dev, who, "dslope");
  if (!rc && dslope) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if constexpr (kBf16) {  // (the fp32 entry point has one gradient: no TWO instance of it is built)
    if (gb) dslope ? launch_grad<OUT, true, true>(vec, grid, s, a) : launch_grad<OUT, true, false>(vec, grid, s, a);
  }
  if (!gb) dslope ? launch_grad<OUT, false, true>(vec, grid, s, a) : launch_grad<OUT, false, false>(vec, grid, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  if (dslope) {
    hipLaunchKernelGGL(prelu_grad_reduce_kernel, dim3((unsigned)ceil_div(channels, kReduceThreads)), dim3(kReduceThreads), 0, s,
                       (const float*)workspace, g.slabs, channels, dslope);
    RTPOSE_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_prelu_grad_workspace_floats(int channels, int N, int H, int W) { return prelu_ws_query(channels, N, H, W); }

int rtpose_prelu_grad_slabs(int channels, int N, int H, int W) { return prelu_slabs_query(channels, N, H, W); }

size_t rtpose_prelu_grad_bf16_workspace_floats(int channels, int N, int H, int W) { return prelu_ws_query(channels, N, H, W); }

int rtpose_prelu_grad_bf16_slabs(int channels, int N, int H, int W) { return prelu_slabs_query(channels, N, H, W); }

int rtpose_prelu(const float* z, const rtpose_layout* lz, const float* slope, float* y, const rtpose_layout* ly,
                 int channels, int N, int H, int W, void* stream) {
  return prelu_forward<float>("prelu", z, lz, slope, y, ly, channels, N, H, W, stream);
}

int rtpose_prelu_bf16(const float* z, const rtpose_layout* lz, const float* slope, void* y, const rtpose_layout* ly,
                      int channels, int N, int H, int W, void* stream) {
  return prelu_forward<uint16_t>("prelu_bf16", z, lz, slope, y, ly, channels, N, H, W, stream);
}

int rtpose_prelu_grad(const float* z, const rtpose_layout* lz, const float* slope, const float* gy,
                      const rtpose_layout* lgy, float* out, const rtpose_layout* lout, float* dslope, float* workspace,
                      size_t workspace_floats, int channels, int N, int H, int W, void* stream) {
  return prelu_backward<float>("prelu_grad", "gy", "rtpose_prelu_grad_workspace_floats", z, lz, slope, gy, lgy, nullptr, nullptr,
                               out, lout, dslope, workspace, workspace_floats, channels, N, H, W, stream);
}

int rtpose_prelu_grad_bf16(const float* z, const rtpose_layout* lz, const float* slope, const float* ga,
                           const rtpose_layout* lga, const float* gb, const rtpose_layout* lgb, void* out,
                           const rtpose_layout* lout, float* dslope, float* workspace, size_t workspace_floats, int channels,
                           int N, int H, int W, void* stream) {
  return prelu_backward<uint16_t>("prelu_grad_bf16", "ga", "rtpose_prelu_grad_bf16_workspace_floats", z, lz, slope, ga, lga, gb,
                                  lgb, out, lout, dslope, workspace, workspace_floats, channels, N, H, W, stream);
}

}  // extern "C"
