// Backward pass of the depthwise 3x3 convolution, padding 1, stride 1 or 2 (header section 2b, continued): what
// nn.Conv2d(C, C, 3, stride, 1, groups = C, bias = False) of the ShuffleNetV2 blocks needs to train (train.dwconv3x3).
// The forward is rtpose_dwconv3x3 (layout_ops.hip).  H, W are the conv's INPUT size, Ho = (H - 1) / stride + 1, Wo likewise.
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
// Sums: rtpose_bn_grad's scheme.  The valid OUTPUT pixels p = (n * Ho + yo) * Wo + xo are cut into slabs whose size follows
// from the shape alone (equal multiples of 64 pixels but for the last one, across image boundaries).  A workgroup of 256
// threads is a tx x ty rectangle: a thread owns one unit of V channels (V = 4: 16-byte loads where every cstride, choff and
// base allows it; V = 1 otherwise; a last unit with fewer than 4 live channels goes element by element) and walks the
// pixels p0 + row, p0 + row + ty, ... of its slab, adding its 9 + 1 terms per channel in that order in fp64 (the product
// of two fp32 values is exact there); the rows of a unit are added in row order through LDS, one term at a time; the
// slab's [10][C] partials go to the caller's workspace, [slab][10][C] doubles, and a second launch of one thread per
// (channel, term) adds them in slab order, rounds once to fp32 and writes dw in OIHW order.  No atomics, no scratch: the
// same inputs give the same bits on every run, and with integer operands every sum is exact whatever its order.
// The data gradient is element-wise: 64 dx pixels per workgroup, the same rectangle.
// Gaps and the channels beside the slices are never written; of gy's gaps only the zero ring of 1 is read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "conv_desc.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kFinalThreads = 64;
constexpr int kSlabUnit = 64;    // pixels: every slab but the last is a multiple of it
constexpr int kMaxSlabs = 1024;  // slabs grow beyond kSlabUnit pixels once there would be more than these
constexpr int kMaxTX = 64;       // channel units a workgroup is wide
constexpr int kTerms = 10;       // nine taps and the bias

struct DwGeom {
  int Ho, Wo;
  long P_in, P_out;  // valid pixels of x / dx and of gy, or -1: a shape the launchers refuse
  int slab, slabs;   // of the output pixels
  size_t ws_doubles;
};

long pixel_count(int N, int H, int W) {
  const long nh = (long)N * H;
  if (nh >= (1L << 31)) return -1;
  const long P = nh * W;
  return P < (1L << 31) - kThreads ? P : -1;
}

// shape only: nothing here looks at the device
DwGeom dw_geometry(int C, int N, int H, int W, int stride) {
  DwGeom g{};
  g.P_in = g.P_out = -1;
  if (C < 1 || N < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return g;
  g.Ho = (H - 1) / stride + 1;
  g.Wo = (W - 1) / stride + 1;
  g.P_in = pixel_count(N, H, W);
  if (g.P_in < 0) return g;
  g.P_out = pixel_count(N, g.Ho, g.Wo);
  const long per = (long)kSlabUnit * kMaxSlabs;
  g.slab = (int)(kSlabUnit * ((g.P_out + per - 1) / per));
  g.slabs = (int)((g.P_out + g.slab - 1) / g.slab);
  g.ws_doubles = (size_t)g.slabs * kTerms * (size_t)C;
  return g;
}

template <int V>
struct Unit {
  float v[V];
};

// the V channels of a unit at element offset o: one 16-byte load of a whole unit, else its nc live channels one by one
template <int V>
__device__ __forceinline__ Unit<V> fetch(const float* src, long long o, int nc, bool whole) {
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
}

// element offset of channel 0 of the view at pixel (y, x) of image n; y and x may be -1 (a gap)
__device__ __forceinline__ long long lay_off_signed(const Lay& l, int n, int y, int x) {
  return ((long long)l.lead + ((long long)n * l.hs + y) * l.ws + x) * l.cstride + l.choff;
}

struct WgArgs {
  const float* x;
  const float* gy;
  double* ws;  // [slab][kTerms][C]
  Lay lx, lgy;
  int C, Ho, Wo, P;  // P: output pixels
  int slab, stride;
  int tx, ty;  // the workgroup's rectangle: tx channel units x ty pixel rows, tx * ty <= kThreads
  FastDiv d_tx, d_wo, d_ho;
};

template <int V>
__global__ __launch_bounds__(kThreads) void dw_wgrad_kernel(const WgArgs a) {
  __shared__ double red[kThreads * V];
  const int tid = threadIdx.x;
  const int row = fast_div(tid, a.d_tx), col = tid - row * a.tx;
  const int c0 = ((int)blockIdx.y * a.tx + col) * V;
  const int nc = min(V, a.C - c0);  // live channels of this thread's unit (<= 0: none)
  const bool live = row < a.ty && nc > 0;
  const bool whole = V > 1 && nc == V;
  const int p0 = (int)blockIdx.x * a.slab;
  const int p1 = min(p0 + a.slab, a.P);

  double acc[kTerms][V];
#pragma unroll
  for (int t = 0; t < kTerms; ++t)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[t][v] = 0.0;

  if (live) {
    const long long row_step = (long long)a.lx.ws * a.lx.cstride;
    for (int p = p0 + row; p < p1; p += a.ty) {
      const int r = fast_div(p, a.d_wo), xo = p - r * a.Wo;
      const int n = fast_div(r, a.d_ho), yo = r - n * a.Ho;
      const Unit<V> gv = fetch<V>(a.gy, lay_off_signed(a.lgy, n, yo, xo) + c0, nc, whole);
      // the tap (0, 0): input pixel (stride yo - 1, stride xo - 1), in the gap for yo = 0 or xo = 0
      const long long base = lay_off_signed(a.lx, n, a.stride * yo - 1, a.stride * xo - 1) + c0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const Unit<V> xv = fetch<V>(a.x, base + ky * row_step + (long long)kx * a.lx.cstride, nc, whole);
#pragma unroll
          for (int v = 0; v < V; ++v) acc[ky * 3 + kx][v] += (double)gv.v[v] * (double)xv.v[v];
        }
#pragma unroll
      for (int v = 0; v < V; ++v) acc[9][v] += (double)gv.v[v];
    }
  }

  // the rows of a unit in row order, one term at a time through the same LDS
#pragma unroll
  for (int t = 0; t < kTerms; ++t) {
    if (live) {
#pragma unroll
      for (int v = 0; v < V; ++v) red[(row * a.tx + col) * V + v] = acc[t][v];
    }
    __syncthreads();
    if (live && row == 0) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        double s = red[col * V + v];
        for (int r = 1; r < a.ty; ++r) s += red[(r * a.tx + col) * V + v];
        if (v < nc) a.ws[((size_t)blockIdx.x * kTerms + t) * a.C + c0 + v] = s;
      }
    }
    __syncthreads();
  }
}

struct WgFinalArgs {
  const double* ws;
  float* dw;     // [C][1][3][3]
  float* dbias;  // or NULL
  int slabs, C;
};

// thread i < C * kTerms: term t = i % kTerms of channel c = i / kTerms, its slabs' partials added in slab order
__global__ __launch_bounds__(kFinalThreads) void dw_wgrad_final_kernel(const WgFinalArgs a) {
  const int i = (int)blockIdx.x * kFinalThreads + threadIdx.x;
  if (i >= a.C * kTerms) return;
  const int c = i / kTerms, t = i - c * kTerms;
  double s = a.ws[(size_t)t * a.C + c];
  // (unrolled: the loads of sixteen slabs are in flight at once; the additions keep their order)
#pragma unroll 16
  for (int k = 1; k < a.slabs; ++k) s += a.ws[((size_t)k * kTerms + t) * a.C + c];
  if (t < 9)
    a.dw[c * 9 + t] = (float)s;
  else if (a.dbias)
    a.dbias[c] = (float)s;
}

struct DgArgs {
  const float* gy;
  const float* w;  // [9][C], the forward's packing
  float* dx;
  Lay lgy, ldx;
  int C, H, W, P;  // P: input pixels
  int stride;
  int tx, ty;
  FastDiv d_tx, d_w, d_h;
};

template <int V>
__global__ __launch_bounds__(kThreads) void dw_dgrad_kernel(const DgArgs a) {
  const int tid = threadIdx.x;
  const int row = fast_div(tid, a.d_tx), col = tid - row * a.tx;
  const int c0 = ((int)blockIdx.y * a.tx + col) * V;
  const int nc = min(V, a.C - c0);
  if (row >= a.ty || nc <= 0) return;
  const bool whole = V > 1 && nc == V;
  const int p0 = (int)blockIdx.x * kSlabUnit;
  const int p1 = min(p0 + kSlabUnit, a.P);

  float wv[9][V];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int v = 0; v < V; ++v) wv[t][v] = v < nc ? a.w[(size_t)t * a.C + c0 + v] : 0.f;

  for (int p = p0 + row; p < p1; p += a.ty) {
    const int r = fast_div(p, a.d_w), xx = p - r * a.W;
    const int n = fast_div(r, a.d_h), yy = r - n * a.H;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    // ascending gy row, then ascending gy column: ky = 2, 1, 0 and kx = 2, 1, 0
#pragma unroll
    for (int ky = 2; ky >= 0; --ky) {
      const int sy = yy + 1 - ky;  // stride * yo; -1 only for yy = 0, ky = 2: odd, so stride 2 skips it
      if (a.stride == 2 && (sy & 1)) continue;
      const int yo = a.stride == 2 ? sy >> 1 : sy;
#pragma unroll
      for (int kx = 2; kx >= 0; --kx) {
        const int sx = xx + 1 - kx;
        if (a.stride == 2 && (sx & 1)) continue;
        const int xo = a.stride == 2 ? sx >> 1 : sx;
        const Unit<V> g = fetch<V>(a.gy, lay_off_signed(a.lgy, n, yo, xo) + c0, nc, whole);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float prod = wv[ky * 3 + kx][v] * g.v[v];
          acc[v] = acc[v] + prod;
        }
      }
    }
    const long long o = lay_off_signed(a.ldx, n, yy, xx) + c0;
    if constexpr (V == 4) {
      if (whole) {
        *reinterpret_cast<float4*>(a.dx + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        continue;
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (v < nc) a.dx[o + v] = acc[v];
  }
}

bool layout_sane(const rtpose_layout& l) { return l.cstride > 0 && l.choff >= 0 && l.ws > 0 && l.hs > 0 && l.lead >= 0; }

bool aligned16(const rtpose_layout& l, const void* base) {
  return slice_aligned(l, 4) && reinterpret_cast<uintptr_t>(base) % 16 == 0;
}

// the rectangle and the grid of a launch; 0 or fail(...)
template <class A>
int set_rectangle(A& a, int V, int xblocks, dim3& grid, const char* who) {
  const int units = ceil_div(a.C, V);
  a.tx = units < kMaxTX ? units : kMaxTX;
  a.ty = kThreads / a.tx;
  a.d_tx = make_fastdiv(a.tx);
  const int ctiles = ceil_div(units, a.tx);
  if (ctiles > 65535) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);
  grid = dim3((unsigned)xblocks, (unsigned)ctiles);
  return 0;
}

// what an entry point asks of one of its slices: `gap` pixels of zero gap around an h x w map; 0 or fail(...)
int check_slice(const char* who, const char* what, const void* p, const rtpose_layout* l, int C, int h, int w, int gap) {
  if (!p) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (%s)", who, what);
  if (!l) return fail(RTPOSE_E_INVAL, "%s: NULL layout (%s)", who, what);
  if (!layout_sane(*l)) return fail(RTPOSE_E_INVAL, "%s: bad layout (%s)", who, what);
  if (!slice_inside(*l, C)) return fail(RTPOSE_E_INVAL, "%s: %s slice exceeds cstride", who, what);
  if (!gap_covers(*l, h, w, gap))
    return fail(RTPOSE_E_INVAL, gap ? "%s: the layout of %s needs a zero gap of at least 1 around the map"
                                    : "%s: layout smaller than the map (%s)", who, what);
  return 0;
}

int check_shape(const char* who, int C, int N, int H, int W, int stride, DwGeom& g) {
  if (stride != 1 && stride != 2) return fail(RTPOSE_E_INVAL, "%s: stride must be 1 or 2 (got %d)", who, stride);
  if (C < 1 || N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "%s: empty tensor", who);
  g = dw_geometry(C, N, H, W, stride);
  if (g.P_in < 0 || g.P_out < 0) return fail(RTPOSE_E_INVAL, "%s: tensor above the launch limit", who);
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
  return g.P_in < 0 || g.P_out < 0 ? 0 : g.slabs;
}

int rtpose_dwconv3x3_wgrad(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy, float* dw,
                           float* dbias, double* workspace, size_t workspace_doubles, int C, int N, int H, int W, int stride,
                           void* stream) {
  const char* who = "dwconv3x3_wgrad";
  DwGeom g;
  if (int rc = check_shape(who, C, N, H, W, stride, g)) return rc;
  if (int rc = check_slice(who, "x", x, lx, C, H, W, 1)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, C, g.Ho, g.Wo, 0)) return rc;
  if (!dw) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (dw)", who);
  if (!workspace) return fail(RTPOSE_E_INVAL, "%s: NULL workspace", who);
  if (reinterpret_cast<uintptr_t>(workspace) % 8) return fail(RTPOSE_E_INVAL, "%s: workspace must be 8-byte aligned", who);
  if (workspace_doubles < g.ws_doubles)
    return fail(RTPOSE_E_INVAL, "%s: workspace of %zu doubles below the %zu rtpose_dwconv3x3_wgrad_workspace_doubles reports",
                who, workspace_doubles, g.ws_doubles);

  WgArgs a{};
  a.x = x;
  a.gy = gy;
  a.ws = workspace;
  a.lx = to_lay(lx);
  a.lgy = to_lay(lgy);
  a.C = C;
  a.Ho = g.Ho;
  a.Wo = g.Wo;
  a.P = (int)g.P_out;
  a.slab = g.slab;
  a.stride = stride;
  a.d_wo = make_fastdiv(g.Wo);
  a.d_ho = make_fastdiv(g.Ho);
  const bool vec = aligned16(*lx, x) && aligned16(*lgy, gy);
  dim3 grid;
  if (int rc = set_rectangle(a, vec ? 4 : 1, g.slabs, grid, who)) return rc;
  if ((long)C * kTerms > 0x7fffffffL - kFinalThreads) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);

  static thread_local CheckedPtr c_x, c_gy, c_dw, c_db, c_ws;
  const int dev = current_device();
  int rc = c_x.check(x, dev, who, "x");
  if (!rc) rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_dw.check(dw, dev, who, "dw");
  if (!rc && dbias) rc = c_db.check(dbias, dev, who, "dbias");
  if (!rc) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(dw_wgrad_kernel<4>, grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(dw_wgrad_kernel<1>, grid, dim3(kThreads), 0, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  WgFinalArgs f{};
  f.ws = workspace;
  f.dw = dw;
  f.dbias = dbias;
  f.slabs = g.slabs;
  f.C = C;
  hipLaunchKernelGGL(dw_wgrad_final_kernel, dim3((unsigned)ceil_div(C * kTerms, kFinalThreads)), dim3(kFinalThreads), 0, s, f);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_dwconv3x3_dgrad(const float* gy, const rtpose_layout* lgy, const float* w, float* dx, const rtpose_layout* ldx, int C,
                           int N, int H, int W, int stride, void* stream) {
  const char* who = "dwconv3x3_dgrad";
  DwGeom g;
  if (int rc = check_shape(who, C, N, H, W, stride, g)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, C, g.Ho, g.Wo, 1)) return rc;
  if (int rc = check_slice(who, "dx", dx, ldx, C, H, W, 0)) return rc;
  if (!w) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (w)", who);

  DgArgs a{};
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
  const bool vec = aligned16(*lgy, gy) && aligned16(*ldx, dx);
  dim3 grid;
  if (int rc = set_rectangle(a, vec ? 4 : 1, ceil_div(a.P, kSlabUnit), grid, who)) return rc;

  static thread_local CheckedPtr c_gy, c_w, c_dx;
  const int dev = current_device();
  int rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_w.check(w, dev, who, "w");
  if (!rc) rc = c_dx.check(dx, dev, who, "dx");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(dw_dgrad_kernel<4>, grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(dw_dgrad_kernel<1>, grid, dim3(kThreads), 0, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
