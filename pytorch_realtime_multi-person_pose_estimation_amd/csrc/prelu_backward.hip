// PReLU as a pass of its own, for training (header section 2b): the forward from a conv's PRE-activation z and the
// backward from the same z.  The inference kernels fuse y = z >= 0 ? z : slope[c] * z into the conv epilogue and keep only
// y; with slopes of either sign sign(y) says nothing about sign(z), so a training forward launches the conv without an
// activation, keeps z and runs rtpose_prelu, and the backward runs rtpose_prelu_grad on z.
//
//   rtpose_prelu       y[n,y,x,c]   = prelu1(z, slope[c])                  (common.h: the fused epilogue's bits)
//   rtpose_prelu_grad  out[n,y,x,c] = z > 0 ? gy : slope[c] * gy           (torch's prelu_backward; gy's bits where z > 0)
//                      dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * gy)
//
// One kernel template, memory bound.  The valid pixels p = (n * H + y) * W + x are cut into slabs whose size follows from
// the shape alone (prelu_geometry: equal multiples of 64 pixels but for the last one).  A workgroup of 256 threads is a
// tx x ty rectangle: a thread owns one unit of V channels (V = 4: 16-byte loads and stores, where every cstride, choff and
// base allows it; V = 1 otherwise; a last unit with fewer than 4 live channels goes element by element) and walks the
// pixels p0 + row, p0 + row + ty, ... of its slab, two pixels in flight.  z and gy are read once: the thread adds its
// z * gy terms in that pixel order, the rows of a unit are added in row order through LDS, and the slab's [channels]
// partial goes to the caller's workspace, [slab][channels].  prelu_grad_reduce_kernel adds the partials in slab order and
// overwrites dslope: no atomics, the same inputs give the same bits on every run.  fp32, one rounding per product (the
// library is built with -ffp-contract=off: slope * gy and z * gy are single multiplies, never part of an fma).
// Gaps and the channels beside the slices are neither read nor written; every element reads only its own gy element, so
// out / lout may name the slice gy / lgy name.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "conv_desc.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kReduceThreads = 64;
constexpr int kSlabUnit = 64;    // pixels: every slab but the last is a multiple of it
constexpr int kMaxSlabs = 1024;  // slabs grow beyond kSlabUnit pixels once there would be more than these
constexpr int kMaxTX = 64;       // channel units a workgroup is wide: 1 KB of one pixel with V = 4

struct PreluGeom {
  int slab;   // pixels per slab
  int slabs;
  size_t ws_floats;  // slabs * channels, rounded up to 4
};

// the valid pixels as a count the kernels index with an int, or -1
long pixel_count(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return -1;
  const long nh = (long)N * H;
  if (nh >= (1L << 31)) return -1;
  const long P = nh * W;
  return P < (1L << 31) - kThreads ? P : -1;
}

bool shape_ok(int channels, int N, int H, int W) { return channels >= 1 && pixel_count(N, H, W) > 0; }

// shape only: nothing here looks at the device
PreluGeom prelu_geometry(int channels, int N, int H, int W) {
  PreluGeom g;
  const long P = pixel_count(N, H, W);
  const long per = (long)kSlabUnit * kMaxSlabs;
  g.slab = (int)(kSlabUnit * ((P + per - 1) / per));
  g.slabs = (int)((P + g.slab - 1) / g.slab);
  g.ws_floats = round_up((size_t)g.slabs * (size_t)channels, 4);
  return g;
}

struct PreluArgs {
  const float* z;
  const float* slope;
  const float* gy;  // backward only
  float* out;       // y of the forward
  float* ws;        // [slab][channels] partials, or NULL
  Lay lz, lgy, lout;
  int channels, H, W, P;
  int slab;
  int tx, ty;  // the workgroup's rectangle: tx channel units x ty pixel rows, tx * ty <= kThreads
  FastDiv d_tx, d_w, d_h;
};

template <int V>
struct Unit {
  float v[V];
};

// V: channels per unit.  GRAD: the backward (else y = prelu1(z, slope)).  SUM: with the slope-gradient partials.
template <int V, bool GRAD, bool SUM>
__global__ __launch_bounds__(kThreads) void prelu_kernel(const PreluArgs a) {
  __shared__ float red[SUM ? kThreads * V : 1];
  const int tid = threadIdx.x;
  const int row = fast_div(tid, a.d_tx), col = tid - row * a.tx;
  const int c0 = ((int)blockIdx.y * a.tx + col) * V;
  const int nc = min(V, a.channels - c0);  // live channels of this thread's unit (<= 0: none)
  const bool live = row < a.ty && nc > 0;
  const bool whole = V > 1 && nc == V;
  const int p0 = (int)blockIdx.x * a.slab;
  const int p1 = min(p0 + a.slab, a.P);

  float sl[V], acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    sl[v] = (live && v < nc) ? a.slope[c0 + v] : 0.f;
    acc[v] = 0.f;
  }

  auto pixel = [&](int p, size_t& oz, size_t& og, size_t& oo) {
    const int r = fast_div(p, a.d_w), xx = p - r * a.W;
    const int n = fast_div(r, a.d_h), yy = r - n * a.H;
    oz = lay_off(a.lz, n, yy, xx) + c0;
    oo = lay_off(a.lout, n, yy, xx) + c0;
    og = GRAD ? lay_off(a.lgy, n, yy, xx) + c0 : 0;
  };
  auto fetch = [&](const float* src, size_t o) {
    Unit<V> u;
    if constexpr (V == 4) {
      if (whole) {
        const float4 t = *reinterpret_cast<const float4*>(src + o);
        u.v[0] = t.x, u.v[1] = t.y, u.v[2] = t.z, u.v[3] = t.w;
        return u;
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) u.v[v] = v < nc ? src[o + v] : 0.f;
    return u;
  };
  auto finish = [&](size_t oo, const Unit<V>& zv, const Unit<V>& gv) {
    Unit<V> r;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (GRAD) {
        const bool pos = zv.v[v] > 0.f;  // torch's rule: z == 0 and NaN z take the slope path
        r.v[v] = __uint_as_float(pos ? __float_as_uint(gv.v[v]) : __float_as_uint(sl[v] * gv.v[v]));
        if (SUM) acc[v] += pos ? 0.f : zv.v[v] * gv.v[v];
      } else {
        r.v[v] = prelu1(zv.v[v], sl[v]);
      }
    }
    if constexpr (V == 4) {
      if (whole) {
        *reinterpret_cast<float4*>(a.out + oo) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        return;
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (v < nc) a.out[oo + v] = r.v[v];
  };

  if (live) {
    // two pixels in flight: both are fetched before either is stored (out may be gy: an element reads only itself)
    for (int p = p0 + row; p < p1; p += 2 * a.ty) {
      const int q = p + a.ty;
      const bool second = q < p1;
      size_t oz0, og0, oo0, oz1, og1, oo1;
      pixel(p, oz0, og0, oo0);
      pixel(second ? q : p, oz1, og1, oo1);  // (the last pixel of an odd walk is fetched twice and stored once)
      const Unit<V> z0 = fetch(a.z, oz0), z1 = fetch(a.z, oz1);
      Unit<V> g0 = z0, g1 = z1;
      if (GRAD) g0 = fetch(a.gy, og0), g1 = fetch(a.gy, og1);
      finish(oo0, z0, g0);
      if (second) finish(oo1, z1, g1);
    }
  }

  if (SUM) {
    if (live) {
#pragma unroll
      for (int v = 0; v < V; ++v) red[(row * a.tx + col) * V + v] = acc[v];
    }
    __syncthreads();
    if (live && row == 0) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float s = red[col * V + v];
        for (int r = 1; r < a.ty; ++r) s += red[(r * a.tx + col) * V + v];
        if (v < nc) a.ws[(size_t)blockIdx.x * a.channels + c0 + v] = s;
      }
    }
  }
}

// thread c < channels: the slabs' partials of channel c, added in slab order
__global__ __launch_bounds__(kReduceThreads) void prelu_grad_reduce_kernel(const float* __restrict__ ws, int slabs,
                                                                         int channels, float* __restrict__ dslope) {
  const int c = (int)blockIdx.x * kReduceThreads + threadIdx.x;
  if (c >= channels) return;
  float v = ws[c];
#pragma unroll 8
  for (int s = 1; s < slabs; ++s) v += ws[(size_t)s * channels + c];
  dslope[c] = v;
}

bool layout_sane(const rtpose_layout& l) { return l.cstride > 0 && l.choff >= 0 && l.ws > 0 && l.hs > 0 && l.lead >= 0; }

bool aligned16(const rtpose_layout& l, const void* base) {
  return slice_aligned(l, 4) && reinterpret_cast<uintptr_t>(base) % 16 == 0;
}

// the rectangle and the grid of a launch; 0 or fail(...)
int set_rectangle(PreluArgs& a, int V, int slabs, dim3& grid, const char* who) {
  const int units = ceil_div(a.channels, V);
  a.tx = units < kMaxTX ? units : kMaxTX;
  a.ty = kThreads / a.tx;
  a.d_tx = make_fastdiv(a.tx);
  const int ctiles = ceil_div(units, a.tx);
  if (ctiles > 65535) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);
  grid = dim3((unsigned)slabs, (unsigned)ctiles);
  return 0;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_prelu_grad_workspace_floats(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return prelu_geometry(channels, N, H, W).ws_floats;
}

int rtpose_prelu_grad_slabs(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return prelu_geometry(channels, N, H, W).slabs;
}

int rtpose_prelu(const float* z, const rtpose_layout* lz, const float* slope, float* y, const rtpose_layout* ly,
                 int channels, int N, int H, int W, void* stream) {
  if (!z || !slope || !y) return fail(RTPOSE_E_INVAL, "prelu: NULL buffer");
  if (!lz || !ly) return fail(RTPOSE_E_INVAL, "prelu: NULL layout");
  if (channels < 1 || N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "prelu: empty tensor");
  if (!layout_sane(*lz) || !layout_sane(*ly)) return fail(RTPOSE_E_INVAL, "prelu: bad layout");
  if (!slice_inside(*lz, channels)) return fail(RTPOSE_E_INVAL, "prelu: z slice exceeds cstride");
  if (!slice_inside(*ly, channels)) return fail(RTPOSE_E_INVAL, "prelu: y slice exceeds cstride");
  if (!gap_covers(*lz, H, W, 0) || !gap_covers(*ly, H, W, 0)) return fail(RTPOSE_E_INVAL, "prelu: layout smaller than the map");
  if (!shape_ok(channels, N, H, W)) return fail(RTPOSE_E_INVAL, "prelu: tensor above the launch limit");

  const PreluGeom g = prelu_geometry(channels, N, H, W);
  PreluArgs a;
  a.z = z;
  a.slope = slope;
  a.gy = nullptr;
  a.out = y;
  a.ws = nullptr;
  a.lz = to_lay(lz);
  a.lgy = to_lay(lz);
  a.lout = to_lay(ly);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = N * H * W;
  a.slab = g.slab;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  const bool vec = aligned16(*lz, z) && aligned16(*ly, y);
  dim3 grid;
  if (int rc = set_rectangle(a, vec ? 4 : 1, g.slabs, grid, "prelu")) return rc;

  static thread_local CheckedPtr c_z, c_s, c_y;
  const int dev = current_device();
  int rc = c_z.check(z, dev, "prelu", "z");
  if (!rc) rc = c_s.check(slope, dev, "prelu", "slope");
  if (!rc) rc = c_y.check(y, dev, "prelu", "y");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL((prelu_kernel<4, false, false>), grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((prelu_kernel<1, false, false>), grid, dim3(kThreads), 0, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_prelu_grad(const float* z, const rtpose_layout* lz, const float* slope, const float* gy,
                      const rtpose_layout* lgy, float* out, const rtpose_layout* lout, float* dslope, float* workspace,
                      size_t workspace_floats, int channels, int N, int H, int W, void* stream) {
  if (!z || !slope || !gy || !out) return fail(RTPOSE_E_INVAL, "prelu_grad: NULL buffer");
  if (!lz || !lgy || !lout) return fail(RTPOSE_E_INVAL, "prelu_grad: NULL layout");
  if (channels < 1 || N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "prelu_grad: empty tensor");
  if (!layout_sane(*lz) || !layout_sane(*lgy) || !layout_sane(*lout)) return fail(RTPOSE_E_INVAL, "prelu_grad: bad layout");
  if (!slice_inside(*lz, channels)) return fail(RTPOSE_E_INVAL, "prelu_grad: z slice exceeds cstride");
  if (!slice_inside(*lgy, channels)) return fail(RTPOSE_E_INVAL, "prelu_grad: gy slice exceeds cstride");
  if (!slice_inside(*lout, channels)) return fail(RTPOSE_E_INVAL, "prelu_grad: out slice exceeds cstride");
  if (!gap_covers(*lz, H, W, 0) || !gap_covers(*lgy, H, W, 0) || !gap_covers(*lout, H, W, 0))
    return fail(RTPOSE_E_INVAL, "prelu_grad: layout smaller than the map");
  if (!shape_ok(channels, N, H, W)) return fail(RTPOSE_E_INVAL, "prelu_grad: tensor above the launch limit");
  const PreluGeom g = prelu_geometry(channels, N, H, W);
  if (dslope) {
    if (!workspace) return fail(RTPOSE_E_INVAL, "prelu_grad: dslope needs a workspace (NULL workspace)");
    if (workspace_floats < g.ws_floats)
      return fail(RTPOSE_E_INVAL, "prelu_grad: workspace of %zu floats below the %zu rtpose_prelu_grad_workspace_floats reports",
                  workspace_floats, g.ws_floats);
  }

  PreluArgs a;
  a.z = z;
  a.slope = slope;
  a.gy = gy;
  a.out = out;
  a.ws = dslope ? workspace : nullptr;
  a.lz = to_lay(lz);
  a.lgy = to_lay(lgy);
  a.lout = to_lay(lout);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = N * H * W;
  a.slab = g.slab;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  const bool vec = aligned16(*lz, z) && aligned16(*lgy, gy) && aligned16(*lout, out);
  dim3 grid;
  if (int rc = set_rectangle(a, vec ? 4 : 1, g.slabs, grid, "prelu_grad")) return rc;

  static thread_local CheckedPtr c_z, c_s, c_gy, c_out, c_ds, c_ws;
  const int dev = current_device();
  int rc = c_z.check(z, dev, "prelu_grad", "z");
  if (!rc) rc = c_s.check(slope, dev, "prelu_grad", "slope");
  if (!rc) rc = c_gy.check(gy, dev, "prelu_grad", "gy");
  if (!rc) rc = c_out.check(out, dev, "prelu_grad", "out");
  if (!rc && dslope) rc = c_ds.check(dslope, dev, "prelu_grad", "dslope");
  if (!rc && dslope) rc = c_ws.check(workspace, dev, "prelu_grad", "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if (dslope) {
    if (vec)
      hipLaunchKernelGGL((prelu_kernel<4, true, true>), grid, dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL((prelu_kernel<1, true, true>), grid, dim3(kThreads), 0, s, a);
    RTPOSE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(prelu_grad_reduce_kernel, dim3((unsigned)ceil_div(channels, kReduceThreads)), dim3(kReduceThreads), 0, s,
                       (const float*)workspace, g.slabs, channels, dslope);
  } else {
    if (vec)
      hipLaunchKernelGGL((prelu_kernel<4, true, false>), grid, dim3(kThreads), 0, s, a);
    else
      hipLaunchKernelGGL((prelu_kernel<1, true, false>), grid, dim3(kThreads), 0, s, a);
  }
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
