// Backward pass of the depthwise 3x3 convolution, padding 1, stride 1 or 2 (header section 2b, continued): what
// nn.Conv2d(C, C, 3, stride, 1, groups = C, bias = False) of the ShuffleNetV2 blocks needs to train (train.dwconv3x3).
// The forward is rtpose_dwconv3x3 (shufflenet_ops.hip).  H, W are the conv's INPUT size, Ho = (H - 1) / stride + 1, Wo likewise.
//
//   rtpose_dwconv3x3_wgrad   dw[c][0][ky][kx] = sum over (n, yo, xo) of gy[n, yo, xo, c] * x[n, stride yo + ky - 1, stride xo + kx - 1, c]
//                            dbias[c]         = sum over (n, yo, xo) of gy[n, yo, xo, c]
//                            x has zero gaps of at least 1, so a tap is a constant pixel offset; gy is read at its valid pixels.
//   rtpose_dwconv3x3_dgrad   dx[n, y, x, c] = sum over the taps (ky, kx) with (y + 1 - ky) and (x + 1 - kx) divisible by stride of
//                                             w[ky * 3 + kx][c] * gy[n, (y + 1 - ky) / stride, (x + 1 - kx) / stride, c]
//                            fp32, one rounding per product and one per add (the library is built with -ffp-contract=off), from
//                            +0, the taps in order of ascending gy row, then ascending gy column (ky = 2, 1, 0; kx = 2, 1, 0).
//                            gy has zero gaps of at least 1: a tap on yo = -1, yo = Ho, xo = -1 or xo = Wo reads a gap.
//
// Sums and walks: chan_slab.h, over the valid OUTPUT pixels p = (n * Ho + yo) * Wo + xo.  A thread adds its 9 + 1 terms
// per channel in fp64 (the product of two fp32 values is exact there); they go through LDS one term at a time; the
// slab's partials are [slab][10][C] doubles, and a second launch of one thread per (channel, term) adds them in slab
// order, rounds once to fp32 and writes dw in OIHW order.  No scratch.  The data gradient is an element-wise pass over
// the dx pixels.  Of gy's gaps only the zero ring of 1 is read.
//
// And the same two passes on the bf16 slices of a layout-resident training run (train.unit_chain): the same device code
// with the element type of its loads a template parameter (IN = uint16_t: bf16 bits, widened exactly on load).
//
//   rtpose_dwconv3x3_wgrad_bf16   x and gy bf16; dw, dbias fp32.  A bf16 x bf16 product is exact in fp64: the fp32 kernel's
//                                 bits on the widened operands.
//   rtpose_dwconv3x3_dgrad_bf16   gy bf16, the taps and dx fp32: the fp32 kernel's bits on the widened gy.
// Both keep the fp32 kernels' units of 4 channels (one 8-byte load of 4 bf16; aligned8_bf16) or 1.  Units of 8 channels - one
// 16-byte load, two 16-byte stores - were built and measured for the data gradient: 1.2 - 1.45 times SLOWER than units of 4 at
// every depthwise shape of the network (profiles/r37_branch_resident.txt), and the weight gradient's acc[10][8] doubles would
// be 160 registers before a single load.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bf16_dest.h"
#include "chan_slab.h"

namespace rtpose {
namespace {

constexpr int kFinalThreads = 64;
constexpr int kTerms = 10;  // nine taps and the bias

struct DwGeom {
  int Ho, Wo;
  long P_in, P_out;  // valid pixels of x / dx and of gy, or -1: a shape the launchers refuse
  SlabGeom s;        // of the output pixels
  size_t ws_doubles;
};

// shape only: nothing here looks at the device
DwGeom dw_geometry(int C, int N, int H, int W, int stride) {
  DwGeom g{};
  g.P_in = g.P_out = -1;
  if (C < 1 || (stride != 1 && stride != 2)) return g;
  g.P_in = pixel_count(N, H, W);
  if (g.P_in < 0) return g;
  g.Ho = (H - 1) / stride + 1;
  g.Wo = (W - 1) / stride + 1;
  g.P_out = pixel_count(N, g.Ho, g.Wo);
  g.s = slab_geometry(g.P_out);
  g.ws_doubles = (size_t)g.s.slabs * kTerms * (size_t)C;
  return g;
}

// IN: float, or uint16_t for bf16 bits
template <class IN>
struct WgArgs {
  const IN* x;
  const IN* gy;
  double* ws;  // [slab][kTerms][C]
  Lay lx, lgy;
  int C, Ho, Wo, P;  // P: output pixels
  int slab, stride;
  Rect r;
  FastDiv d_wo, d_ho;
};

// the V channels of a unit at element offset o, as fp32: chan_slab.h's fetch of fp32 elements; of bf16 bits one 8-byte load of
// a whole unit of 4, else its live channels one by one, each widened exactly
template <int V, class IN>
__device__ __forceinline__ Unit<V> load_unit(const IN* src, long long o, const Place& t) {
  if constexpr (std::is_same_v<IN, float>) {
    return fetch<V>(src, o, t);
  } else {
    Unit<V> u;
    if constexpr (V == 4) {
      if (t.whole) {
        const Word2 f = *reinterpret_cast<const Word2*>(src + o);
        u.v[0] = __uint_as_float(f.x << 16), u.v[1] = __uint_as_float(f.x & 0xffff0000u);
        u.v[2] = __uint_as_float(f.y << 16), u.v[3] = __uint_as_float(f.y & 0xffff0000u);
        return u;
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) u.v[v] = v < t.nc ? bf16_to_f32(src[o + v]) : 0.f;
    return u;
  }
}

template <int V, class IN = float>
__global__ __launch_bounds__(kThreads) void dw_wgrad_kernel(const WgArgs<IN> a) {
  const Place t = place<V>(a.r, a.C, a.slab, a.P);

  double acc[kTerms][V];
#pragma unroll
  for (int k = 0; k < kTerms; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[k][v] = 0.0;

  if (t.live) {
    const long long row_step = (long long)a.lx.ws * a.lx.cstride;
    for (int p = t.p0 + t.row; p < t.p1; p += a.r.ty) {
      const Pixel q = pixel_of(p, a.Ho, a.Wo, a.d_ho, a.d_wo);
      const Unit<V> gv = load_unit<V>(a.gy, lay_off_signed(a.lgy, q.n, q.y, q.x) + t.c0, t);
      // the tap (0, 0): input pixel (stride yo - 1, stride xo - 1), in the gap for yo = 0 or xo = 0
      const long long base = lay_off_signed(a.lx, q.n, a.stride * q.y - 1, a.stride * q.x - 1) + t.c0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const Unit<V> xv = load_unit<V>(a.x, base + ky * row_step + (long long)kx * a.lx.cstride, t);
#pragma unroll
          for (int v = 0; v < V; ++v) acc[ky * 3 + kx][v] += (double)gv.v[v] * (double)xv.v[v];
        }
#pragma unroll
      for (int v = 0; v < V; ++v) acc[9][v] += (double)gv.v[v];
    }
  }

  sum_rows<V, kTerms, 1>(t, a.r, acc, a.ws, a.C);
}

struct WgFinalArgs {
  const double* ws;
  float* dw;     // [C][1][3][3]
  float* dbias;  // or NULL
  int slabs, C;
};

// thread i < C * kTerms: term k = i % kTerms of channel c = i / kTerms
__global__ __launch_bounds__(kFinalThreads) void dw_wgrad_final_kernel(const WgFinalArgs a) {
  const int i = (int)blockIdx.x * kFinalThreads + threadIdx.x;
  if (i >= a.C * kTerms) return;
  const int c = i / kTerms, k = i - c * kTerms;
  double s[1];
  sum_slabs<1, 16>(a.ws, a.slabs, kTerms, a.C, k, c, s);
  if (k < 9)
    a.dw[c * 9 + k] = (float)s[0];
  else if (a.dbias)
    a.dbias[c] = (float)s[0];
}

template <class IN>
struct DgArgs {
  const IN* gy;
  const float* w;  // [9][C], the forward's packing
  float* dx;
  Lay lgy, ldx;
  int C, H, W, P;  // P: input pixels
  int stride;
  Rect r;
  FastDiv d_w, d_h;
};

template <int V, class IN = float>
__global__ __launch_bounds__(kThreads) void dw_dgrad_kernel(const DgArgs<IN> a) {
  const Place t = place<V>(a.r, a.C, kSlabUnit, a.P);
  if (!t.live) return;

  float wv[9][V];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) wv[k][v] = v < t.nc ? a.w[(size_t)k * a.C + t.c0 + v] : 0.f;

  for (int p = t.p0 + t.row; p < t.p1; p += a.r.ty) {
    const Pixel q = pixel_of(p, a.H, a.W, a.d_h, a.d_w);
    Unit<V> acc;
#pragma unroll
    for (int v = 0; v < V; ++v) acc.v[v] = 0.f;
    // ascending gy row, then ascending gy column: ky = 2, 1, 0 and kx = 2, 1, 0
#pragma unroll
    for (int ky = 2; ky >= 0; --ky) {
      const int sy = q.y + 1 - ky;  // stride * yo; -1 only for y = 0, ky = 2: odd, so stride 2 skips it
      if (a.stride == 2 && (sy & 1)) continue;
      const int yo = a.stride == 2 ? sy >> 1 : sy;
#pragma unroll
      for (int kx = 2; kx >= 0; --kx) {
        const int sx = q.x + 1 - kx;
        if (a.stride == 2 && (sx & 1)) continue;
        const int xo = a.stride == 2 ? sx >> 1 : sx;
        const Unit<V> g = load_unit<V>(a.gy, lay_off_signed(a.lgy, q.n, yo, xo) + t.c0, t);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float prod = wv[ky * 3 + kx][v] * g.v[v];
          acc.v[v] = acc.v[v] + prod;
        }
      }
    }
    store<V>(a.dx, lay_off_signed(a.ldx, q.n, q.y, q.x) + t.c0, t, acc);
  }
}

int check_shape_dw(const char* who, int C, int N, int H, int W, int stride, DwGeom& g) {
  if (stride != 1 && stride != 2) return fail(RTPOSE_E_INVAL, "%s: stride must be 1 or 2 (got %d)", who, stride);
  long P;
  if (int rc = check_shape(who, C, N, H, W, P)) return rc;
  g = dw_geometry(C, N, H, W, stride);
  if (g.P_out < 0) return fail(RTPOSE_E_INVAL, "%s: tensor above the launch limit", who);
  return 0;
}

// a bf16 slice beside check_slice: its base holds 2-byte elements
int check_bf16_base(const char* who, const char* what, const void* p) {
  if (reinterpret_cast<uintptr_t>(p) % 2) return fail(RTPOSE_E_INVAL, "%s: %s must be 2-byte aligned", who, what);
  return 0;
}

// rtpose_dwconv3x3_wgrad (IN = float) and rtpose_dwconv3x3_wgrad_bf16 (IN = uint16_t); the finalising launch is the same
// instance for both
template <class IN>
int dw_wgrad(const char* who, const IN* x, const rtpose_layout* lx, const IN* gy, const rtpose_layout* lgy, float* dw,
             float* dbias, double* workspace, size_t workspace_doubles, int C, int N, int H, int W, int stride, void* stream) {
  constexpr bool kBf16 = !std::is_same_v<IN, float>;
  DwGeom g;
  if (int rc = check_shape_dw(who, C, N, H, W, stride, g)) return rc;
  if (int rc = check_slice(who, "x", x, lx, C, H, W, 1)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, C, g.Ho, g.Wo, 0)) return rc;
  if constexpr (kBf16) {
    if (int rc = check_bf16_base(who, "x", x)) return rc;
    if (int rc = check_bf16_base(who, "gy", gy)) return rc;
  }
  if (!dw) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (dw)", who);
  if (int rc = check_workspace(who, workspace, workspace_doubles, g.ws_doubles, "rtpose_dwconv3x3_wgrad_workspace_doubles"))
    return rc;

  WgArgs<IN> a{};
  a.x = x;
  a.gy = gy;
  a.ws = workspace;
  a.lx = to_lay(lx);
  a.lgy = to_lay(lgy);
  a.C = C;
  a.Ho = g.Ho;
  a.Wo = g.Wo;
  a.P = (int)g.P_out;
  a.slab = g.s.slab;
  a.stride = stride;
  a.d_wo = make_fastdiv(g.Wo);
  a.d_ho = make_fastdiv(g.Ho);
  bool vec;
  if constexpr (kBf16)
    vec = aligned8_bf16(*lx, x) && aligned8_bf16(*lgy, gy);
  else
    vec = aligned16(*lx, x) && aligned16(*lgy, gy);
  dim3 grid;
  if (int rc = set_rectangle(a.r, C, vec ? 4 : 1, g.s.slabs, grid, who)) return rc;
  if ((long)C * kTerms > 0x7fffffffL - kFinalThreads) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_x, c_gy, c_dw, c_db, c_ws;
  const int dev = current_device();
  int rc = c_x.check(x, dev, who, "x");
  if (!rc) rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_dw.check(dw, dev, who, "dw");
  if (!rc && dbias) rc = c_db.check(dbias, dev, who, "dbias");
  if (!rc) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  launch_units<dw_wgrad_kernel<4, IN>, dw_wgrad_kernel<1, IN>>(vec, grid, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  WgFinalArgs f{};
  f.ws = workspace;
  f.dw = dw;
  f.dbias = dbias;
  f.slabs = g.s.slabs;
  f.C = C;
  hipLaunchKernelGGL(dw_wgrad_final_kernel, dim3((unsigned)ceil_div(C * kTerms, kFinalThreads)), dim3(kFinalThreads), 0, s, f);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

// rtpose_dwconv3x3_dgrad (IN = float) and rtpose_dwconv3x3_dgrad_bf16 (IN = uint16_t)
template <class IN>
int dw_dgrad(const char* who, const IN* gy, const rtpose_layout* lgy, const float* w, float* dx, const rtpose_layout* ldx, int C,
             int N, int H, int W, int stride, void* stream) {
  constexpr bool kBf16 = !std::is_same_v<IN, float>;
  DwGeom g;
  if (int rc = check_shape_dw(who, C, N, H, W, stride, g)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, C, g.Ho, g.Wo, 1)) return rc;
  if (int rc = check_slice(who, "dx", dx, ldx, C, H, W, 0)) return rc;
  if constexpr (kBf16)
    if (int rc = check_bf16_base(who, "gy", gy)) return rc;
  if (!w) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (w)", who);

  DgArgs<IN> a{};
  a.gy = gy;
  a.w = w;
  a.dx = dx;
  a.lgy = to_lay(lgy);
  a.ldx = to_lay(ldx);
  a.C = C;
  a.H = H;
  a.W = W;
  a.P = (int)g.P_in;
  a.stride = stride;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  bool vec = aligned16(*ldx, dx);
  if constexpr (kBf16)
    vec = vec && aligned8_bf16(*lgy, gy);
  else
    vec = vec && aligned16(*lgy, gy);
  dim3 grid;
  if (int rc = set_rectangle(a.r, C, vec ? 4 : 1, ceil_div(a.P, kSlabUnit), grid, who)) return rc;

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_gy, c_w, c_dx;
  const int dev = current_device();
  int rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_w.check(w, dev, who, "w");
  if (!rc) rc = c_dx.check(dx, dev, who, "dx");
  if (rc) return rc;

  launch_units<dw_dgrad_kernel<4, IN>, dw_dgrad_kernel<1, IN>>(vec, grid, as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_dwconv3x3_wgrad_workspace_doubles(int C, int N, int H, int W, int stride) {
  const DwGeom g = dw_geometry(C, N, H, W, stride);
  return g.P_in < 0 || g.P_out < 0 ? 0 : g.ws_doubles;
}

int rtpose_dwconv3x3_wgrad_slabs(int C, int N, int H, int W, int stride) {
  const DwGeom g = dw_geometry(C, N, H, W, stride);
  return g.P_in < 0 || g.P_out < 0 ? 0 : g.s.slabs;
}

int rtpose_dwconv3x3_wgrad(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy, float* dw,
                           float* dbias, double* workspace, size_t workspace_doubles, int C, int N, int H, int W, int stride,
                           void* stream) {
  return dw_wgrad<float>("dwconv3x3_wgrad", x, lx, gy, lgy, dw, dbias, workspace, workspace_doubles, C, N, H, W, stride, stream);
}

int rtpose_dwconv3x3_wgrad_bf16(const void* x, const rtpose_layout* lx, const void* gy, const rtpose_layout* lgy, float* dw,
                                float* dbias, double* workspace, size_t workspace_doubles, int C, int N, int H, int W,
                                int stride, void* stream) {
  return dw_wgrad<uint16_t>("dwconv3x3_wgrad_bf16", static_cast<const uint16_t*>(x), lx, static_cast<const uint16_t*>(gy), lgy, dw,
                            dbias, workspace, workspace_doubles, C, N, H, W, stride, stream);
}

int rtpose_dwconv3x3_dgrad(const float* gy, const rtpose_layout* lgy, const float* w, float* dx, const rtpose_layout* ldx, int C,
                           int N, int H, int W, int stride, void* stream) {
  return dw_dgrad<float>("dwconv3x3_dgrad", gy, lgy, w, dx, ldx, C, N, H, W, stride, stream);
}

int rtpose_dwconv3x3_dgrad_bf16(const void* gy, const rtpose_layout* lgy, const float* w, float* dx, const rtpose_layout* ldx,
                                int C, int N, int H, int W, int stride, void* stream) {
  return dw_dgrad<uint16_t>("dwconv3x3_dgrad_bf16", static_cast<const uint16_t*>(gy), lgy, w, dx, ldx, C, N, H, W, stride, stream);
}

}  // extern "C"
