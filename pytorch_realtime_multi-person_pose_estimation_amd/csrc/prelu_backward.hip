// PReLU as a pass of its own, for training (header section 2b): the forward from a conv's PRE-activation z and the
// backward from the same z.  The inference kernels fuse y = z >= 0 ? z : slope[c] * z into the conv epilogue and keep only
// y; with slopes of either sign sign(y) says nothing about sign(z), so a training forward launches the conv without an
// activation, keeps z and runs rtpose_prelu, and the backward runs rtpose_prelu_grad on z.
//
//   rtpose_prelu       y[n,y,x,c]   = prelu1(z, slope[c])                  (common.h: the fused epilogue's bits)
//   rtpose_prelu_grad  out[n,y,x,c] = z > 0 ? gy : slope[c] * gy           (torch's prelu_backward; gy's bits where z > 0)
//                      dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * gy)
//
// One kernel template, memory bound, on the slabs, rectangle and units of chan_slab.h, two pixels in flight.  z and gy
// are read once: the thread adds its z * gy terms in its pixel order, chan_slab.h's row-order and slab-order sums (one
// term, fp32) make dslope of them, overwriting it.  fp32, one rounding per product (the library is built with
// -ffp-contract=off: slope * gy and z * gy are single multiplies, never part of an fma).
// Every element reads only its own gy element, so out / lout may name the slice gy / lgy name.
#include <hip/hip_runtime.h>

#include "chan_slab.h"

namespace rtpose {
namespace {

constexpr int kReduceThreads = 64;

bool shape_ok(int channels, int N, int H, int W) { return channels >= 1 && pixel_count(N, H, W) > 0; }

// slabs * channels, rounded up to 4
size_t ws_floats(int channels, const SlabGeom& g) { return round_up((size_t)g.slabs * (size_t)channels, 4); }

struct PreluArgs {
  const float* z;
  const float* slope;
  const float* gy;  // backward only
  float* out;       // y of the forward
  float* ws;        // [slab][channels] partials, or NULL
  Lay lz, lgy, lout;
  int channels, H, W, P;
  int slab;
  Rect r;
  FastDiv d_w, d_h;
};

// V: channels per unit.  GRAD: the backward (else y = prelu1(z, slope)).  SUM: with the slope-gradient partials.
template <int V, bool GRAD, bool SUM>
__global__ __launch_bounds__(kThreads) void prelu_kernel(const PreluArgs a) {
  const Place t = place<V>(a.r, a.channels, a.slab, a.P);

  float sl[V], acc[1][V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    sl[v] = (t.live && v < t.nc) ? a.slope[t.c0 + v] : 0.f;
    acc[0][v] = 0.f;
  }

  auto pixel = [&](int p, size_t& oz, size_t& og, size_t& oo) {
    const Pixel q = pixel_of(p, a.H, a.W, a.d_h, a.d_w);
    oz = lay_off(a.lz, q) + t.c0;
    oo = lay_off(a.lout, q) + t.c0;
    og = GRAD ? lay_off(a.lgy, q) + t.c0 : 0;
  };
  auto finish = [&](size_t oo, const Unit<V>& zv, const Unit<V>& gv) {
    Unit<V> r;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (GRAD) {
        const bool pos = zv.v[v] > 0.f;  // torch's rule: z == 0 and NaN z take the slope path
        r.v[v] = __uint_as_float(pos ? __float_as_uint(gv.v[v]) : __float_as_uint(sl[v] * gv.v[v]));
        if (SUM) acc[0][v] += pos ? 0.f : zv.v[v] * gv.v[v];
      } else {
        r.v[v] = prelu1(zv.v[v], sl[v]);
      }
    }
    store<V>(a.out, oo, t, r);
  };

  if (t.live) {
    // two pixels in flight: both are fetched before either is stored (out may be gy: an element reads only itself)
    for (int p = t.p0 + t.row; p < t.p1; p += 2 * a.r.ty) {
      const int q = p + a.r.ty;
      const bool second = q < t.p1;
      size_t oz0, og0, oo0, oz1, og1, oo1;
      pixel(p, oz0, og0, oo0);
      pixel(second ? q : p, oz1, og1, oo1);  // (the last pixel of an odd walk is fetched twice and stored once)
      const Unit<V> z0 = fetch<V>(a.z, oz0, t), z1 = fetch<V>(a.z, oz1, t);
      Unit<V> g0 = z0, g1 = z1;
      if (GRAD) g0 = fetch<V>(a.gy, og0, t), g1 = fetch<V>(a.gy, og1, t);
      finish(oo0, z0, g0);
      if (second) finish(oo1, z1, g1);
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

// the arguments, the rectangle and the grid of either pass (the forward: gy = NULL, lgy = lz); 0 or fail(...)
int prelu_args(PreluArgs& a, dim3& grid, bool& vec, const char* who, const float* z, const rtpose_layout* lz,
               const float* slope, const float* gy, const rtpose_layout* lgy, float* out, const rtpose_layout* lout, float* ws,
               int channels, int H, int W, long P) {
  const SlabGeom g = slab_geometry(P);
  a.z = z;
  a.slope = slope;
  a.gy = gy;
  a.out = out;
  a.ws = ws;
  a.lz = to_lay(lz);
  a.lgy = to_lay(lgy);
  a.lout = to_lay(lout);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = (int)P;
  a.slab = g.slab;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  vec = aligned16(*lz, z) && (!gy || aligned16(*lgy, gy)) && aligned16(*lout, out);
  return set_rectangle(a.r, channels, vec ? 4 : 1, g.slabs, grid, who);
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_prelu_grad_workspace_floats(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return ws_floats(channels, slab_geometry(pixel_count(N, H, W)));
}

int rtpose_prelu_grad_slabs(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return slab_geometry(pixel_count(N, H, W)).slabs;
}

int rtpose_prelu(const float* z, const rtpose_layout* lz, const float* slope, float* y, const rtpose_layout* ly,
                 int channels, int N, int H, int W, void* stream) {
  const char* who = "prelu";
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "z", z, lz, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "y", y, ly, channels, H, W, 0)) return rc;
  if (!slope) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (slope)", who);

  PreluArgs a;
  dim3 grid;
  bool vec;
  if (int rc = prelu_args(a, grid, vec, who, z, lz, slope, nullptr, lz, y, ly, nullptr, channels, H, W, P)) return rc;

  static thread_local CheckedPtr c_z, c_s, c_y;
  const int dev = current_device();
  int rc = c_z.check(z, dev, who, "z");
  if (!rc) rc = c_s.check(slope, dev, who, "slope");
  if (!rc) rc = c_y.check(y, dev, who, "y");
  if (rc) return rc;

  launch_units<prelu_kernel<4, false, false>, prelu_kernel<1, false, false>>(vec, grid, as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_prelu_grad(const float* z, const rtpose_layout* lz, const float* slope, const float* gy,
                      const rtpose_layout* lgy, float* out, const rtpose_layout* lout, float* dslope, float* workspace,
                      size_t workspace_floats, int channels, int N, int H, int W, void* stream) {
  const char* who = "prelu_grad";
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "z", z, lz, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "out", out, lout, channels, H, W, 0)) return rc;
  if (!slope) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (slope)", who);
  const SlabGeom g = slab_geometry(P);
  if (dslope)  // (no dslope: no sums, and the workspace is not looked at)
    if (int rc = check_workspace(who, workspace, workspace_floats, ws_floats(channels, g), "rtpose_prelu_grad_workspace_floats"))
      return rc;

  PreluArgs a;
  dim3 grid;
  bool vec;
  if (int rc = prelu_args(a, grid, vec, who, z, lz, slope, gy, lgy, out, lout, dslope ? workspace : nullptr, channels, H, W, P))
    return rc;

  static thread_local CheckedPtr c_z, c_s, c_gy, c_out, c_ds, c_ws;
  const int dev = current_device();
  int rc = c_z.check(z, dev, who, "z");
  if (!rc) rc = c_s.check(slope, dev, who, "slope");
  if (!rc) rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_out.check(out, dev, who, "out");
  if (!rc && dslope) rc = c_ds.check(dslope, dev, who, "dslope");
  if (!rc && dslope) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if (dslope) {
    launch_units<prelu_kernel<4, true, true>, prelu_kernel<1, true, true>>(vec, grid, s, a);
    RTPOSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(prelu_grad_reduce_kernel, dim3((unsigned)ceil_div(channels, kReduceThreads)), dim3(kReduceThreads), 0, s,
                       (const float*)workspace, g.slabs, channels, dslope);
  } else {
    launch_units<prelu_kernel<4, true, false>, prelu_kernel<1, true, false>>(vec, grid, s, a);
  }
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
