// The deterministic per-channel sum of the training kernels (prelu_backward.hip, batchnorm.hip, dwconv_backward.hip), and
// the element-wise passes that walk the same way (prelu_backward.hip's forwards, act_grad_bf16.hip).
//
// The valid pixels p = (n * H + y) * W + x of a map are cut into slabs whose size follows from the shape alone
// (slab_geometry: equal multiples of 64 pixels but for the last one, across image boundaries).  A workgroup of 256 threads
// is a tx x ty rectangle (set_rectangle): a thread owns one unit of V channels (V = 4: 16-byte loads and stores, where every
// cstride, choff and base allows it - aligned16; V = 1 otherwise; a last unit with fewer than 4 live channels goes element
// by element) and walks the pixels p0 + row, p0 + row + ty, ... of its slab (place, pixel_of), adding each of its terms in
// that order.  The rows of a unit are added in row order 0, 1, ..., ty - 1 through LDS and the slab's partials go to the
// caller's workspace, [slab][term][channel] (sum_rows); a second launch adds them in slab order 0, 1, ..., slabs - 1
// (sum_slabs) and finishes with its kernel's own arithmetic.  No atomics: the same inputs give the same bits on every run,
// and sums whose terms are exact (integer operands; fp32 values and products of two in fp64) are exact whatever the order.
// An element-wise pass is the same walk without sums; its values do not depend on how the pixels are cut, so it takes
// kSlabUnit pixels per workgroup whatever the slab of the sums.
// Gaps and the channels beside a slice are never written, and read only where a kernel says so (the depthwise taps).
#pragma once
#include <cstdint>

#include "conv_desc.h"

namespace rtpose {

constexpr int kThreads = 256;
constexpr int kSlabUnit = 64;    // pixels: every slab but the last is a multiple of it
constexpr int kMaxSlabs = 1024;  // slabs grow beyond kSlabUnit pixels once there would be more than these
constexpr int kMaxTX = 64;       // channel units a workgroup is wide: 1 KB of one pixel with V = 4

// ---- host: shape, slabs, checks ------------------------------------------------------------------------------------------
// the valid pixels as a count the kernels index with an int, or -1
inline long pixel_count(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return -1;
  const long nh = (long)N * H;
  if (nh >= (1L << 31)) return -1;
  const long P = nh * W;
  return P < (1L << 31) - kThreads ? P : -1;
}

struct SlabGeom {
  int slab;  // pixels per slab
  int slabs;
};

// shape only: nothing here looks at the device
inline SlabGeom slab_geometry(long P) {
  SlabGeom g;
  const long per = (long)kSlabUnit * kMaxSlabs;
  g.slab = (int)(kSlabUnit * ((P + per - 1) / per));
  g.slabs = (int)((P + g.slab - 1) / g.slab);
  return g;
}

inline bool aligned16(const rtpose_layout& l, const void* base) {
  return slice_aligned(l, 4) && reinterpret_cast<uintptr_t>(base) % 16 == 0;
}

// the bytes [first, last) the valid pixels' slices of a layout of `esize`-byte elements span
inline void slice_span_bytes(const void* base, const rtpose_layout& l, int esize, int channels, int N, int H, int W,
                             uintptr_t& first, uintptr_t& last) {
  const size_t lo = (size_t)l.lead * l.cstride + l.choff;
  const size_t hi = ((size_t)l.lead + ((size_t)(N - 1) * l.hs + (H - 1)) * l.ws + (W - 1)) * l.cstride + l.choff + channels;
  first = reinterpret_cast<uintptr_t>(base) + (size_t)esize * lo;
  last = reinterpret_cast<uintptr_t>(base) + (size_t)esize * hi;
}

// P = pixel_count of a non-empty tensor; 0 or fail(...)
inline int check_shape(const char* who, int channels, int N, int H, int W, long& P) {
  if (channels < 1 || N <= 0 || H <= 0 || W <= 0) return fail(RTPOSE_E_INVAL, "%s: empty tensor", who);
  P = pixel_count(N, H, W);
  if (P < 0) return fail(RTPOSE_E_INVAL, "%s: tensor above the launch limit", who);
  return 0;
}

// what an entry point asks of one of its slices: `gap` pixels of zero gap around an h x w map; 0 or fail(...)
inline int check_slice(const char* who, const char* what, const void* p, const rtpose_layout* l, int channels, int h, int w,
                       int gap) {
  if (!p) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (%s)", who, what);
  if (!l) return fail(RTPOSE_E_INVAL, "%s: NULL layout (%s)", who, what);
  if (!layout_sane(*l)) return fail(RTPOSE_E_INVAL, "%s: bad layout (%s)", who, what);
  if (!slice_inside(*l, channels)) return fail(RTPOSE_E_INVAL, "%s: %s slice exceeds cstride", who, what);
  if (!gap_covers(*l, h, w, gap))
    return fail(RTPOSE_E_INVAL, gap ? "%s: the layout of %s needs a zero gap of at least 1 around the map"
                                    : "%s: layout smaller than the map (%s)", who, what);
  return 0;
}

// the caller's workspace of floats or doubles against what `reporter` (the exported *_workspace_* function) reports
template <class T>
inline int check_workspace(const char* who, const T* ws, size_t given, size_t need, const char* reporter) {
  const char* unit = sizeof(T) == 8 ? "doubles" : "floats";
  if (!ws) return fail(RTPOSE_E_INVAL, "%s: NULL workspace", who);
  if (reinterpret_cast<uintptr_t>(ws) % sizeof(T))
    return fail(RTPOSE_E_INVAL, "%s: workspace must be %zu-byte aligned", who, sizeof(T));
  if (given < need)
    return fail(RTPOSE_E_INVAL, "%s: workspace of %zu %s below the %zu %s reports", who, given, unit, need, reporter);
  return 0;
}

// ---- host: the rectangle and the launch ----------------------------------------------------------------------------------
// the workgroup's rectangle: tx channel units x ty pixel rows, tx * ty <= kThreads
struct Rect {
  int tx, ty;
  FastDiv d_tx;
};

// the rectangle and the grid of a launch over `xblocks` slabs; 0 or fail(...)
inline int set_rectangle(Rect& r, int channels, int V, int xblocks, dim3& grid, const char* who) {
  const int units = ceil_div(channels, V);
  r.tx = units < kMaxTX ? units : kMaxTX;
  r.ty = kThreads / r.tx;
  r.d_tx = make_fastdiv(r.tx);
  const int ctiles = ceil_div(units, r.tx);
  if (ctiles > 65535) return fail(RTPOSE_E_INVAL, "%s: grid too large", who);
  grid = dim3((unsigned)xblocks, (unsigned)ctiles);
  return 0;
}

// the V = 4 instance of a kernel template where every slice is aligned16, else the V = 1 one
template <auto Kern4, auto Kern1, class A>
inline void launch_units(bool vec, dim3 grid, hipStream_t s, const A& a) {
  if (vec)
    hipLaunchKernelGGL(Kern4, grid, dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(Kern1, grid, dim3(kThreads), 0, s, a);
}

// ---- device --------------------------------------------------------------------------------------------------------------
template <int V>
struct Unit {
  float v[V];
};

// a thread's place in the rectangle and its slab
struct Place {
  int row, col;
  int c0, nc;   // first channel of the unit, its live channels (<= 0: none)
  int p0, p1;   // the slab's pixels
  bool live;    // a row of the rectangle and a unit with channels
  bool whole;   // all V channels live: 16-byte accesses
};

template <int V>
__device__ __forceinline__ Place place(const Rect& r, int channels, int slab, int P) {
  Place t;
  const int tid = threadIdx.x;
  t.row = fast_div(tid, r.d_tx), t.col = tid - t.row * r.tx;
  t.c0 = ((int)blockIdx.y * r.tx + t.col) * V;
  t.nc = min(V, channels - t.c0);
  t.live = t.row < r.ty && t.nc > 0;
  t.whole = V > 1 && t.nc == V;
  t.p0 = (int)blockIdx.x * slab;
  t.p1 = min(t.p0 + slab, P);
  return t;
}

struct Pixel {
  int n, y, x;
};

__device__ __forceinline__ Pixel pixel_of(int p, int H, int W, const FastDiv d_h, const FastDiv d_w) {
  const int r = fast_div(p, d_w), x = p - r * W;
  const int n = fast_div(r, d_h), y = r - n * H;
  return Pixel{n, y, x};
}

__device__ __forceinline__ size_t lay_off(const Lay& l, const Pixel& q) { return lay_off(l, q.n, q.y, q.x); }

// element offset of channel 0 of the view at pixel (y, x) of image n; y and x may be -1 (a gap)
__device__ __forceinline__ long long lay_off_signed(const Lay& l, int n, int y, int x) {
  return ((long long)l.lead + ((long long)n * l.hs + y) * l.ws + x) * l.cstride + l.choff;
}

// (a vector type of the compiler's own: one 16-byte access whatever the optimiser makes of the paths around it - it takes
// float4, a struct, apart and has sunk its last store into the element-wise path's, leaving a 12-byte and a 4-byte store)
typedef float Float4 __attribute__((ext_vector_type(4)));

// the V channels of a unit at element offset o: one 16-byte access of a whole unit, else its live channels one by one
template <int V>
__device__ __forceinline__ Unit<V> fetch(const float* src, long long o, const Place& t) {
  Unit<V> u;
  if constexpr (V == 4) {
    if (t.whole) {
      const Float4 f = *reinterpret_cast<const Float4*>(src + o);
      u.v[0] = f.x, u.v[1] = f.y, u.v[2] = f.z, u.v[3] = f.w;
      return u;
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) u.v[v] = v < t.nc ? src[o + v] : 0.f;
  return u;
}

template <int V>
__device__ __forceinline__ void store(float* dst, long long o, const Place& t, const Unit<V>& u) {
  if constexpr (V == 4) {
    if (t.whole) {
      *reinterpret_cast<Float4*>(dst + o) = Float4{u.v[0], u.v[1], u.v[2], u.v[3]};
      return;
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v)
    if (v < t.nc) dst[o + v] = u.v[v];
}

// The rows of a unit added in row order, PER of the TERMS terms per pass through LDS, and this slab's partials written to
// ws, [slab][TERMS][channels].  Every thread of the workgroup calls it.
template <int V, int TERMS, int PER, class T>
__device__ __forceinline__ void sum_rows(const Place& t, const Rect& r, const T (&acc)[TERMS][V], T* ws, int channels) {
  static_assert(TERMS % PER == 0, "whole passes");
  __shared__ T red[kThreads * V * PER];
  T* const out = ws + (size_t)blockIdx.x * TERMS * channels + t.c0;  // this slab's [TERMS][channels] at the unit's channels
#pragma unroll
  for (int t0 = 0; t0 < TERMS; t0 += PER) {
    if (t.live) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int k = 0; k < PER; ++k) red[((t.row * r.tx + t.col) * V + v) * PER + k] = acc[t0 + k][v];
    }
    __syncthreads();
    if (t.live && t.row == 0) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        T s[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) s[k] = red[(t.col * V + v) * PER + k];
        for (int row = 1; row < r.ty; ++row)
#pragma unroll
          for (int k = 0; k < PER; ++k) s[k] += red[((row * r.tx + t.col) * V + v) * PER + k];
        if (v < t.nc) {
#pragma unroll
          for (int k = 0; k < PER; ++k) out[(size_t)(t0 + k) * channels + v] = s[k];
        }
      }
    }
    if (t0 + PER < TERMS) __syncthreads();  // the next pass writes the same LDS
  }
}

// s[k] = the slabs' partials of term t0 + k of channel c, added in slab order; ws is [slab][terms][channels].
// (UNROLL: that many slabs' loads in flight at once; the additions keep their order)
template <int N, int UNROLL, class T>
__device__ __forceinline__ void sum_slabs(const T* ws, int slabs, int terms, int channels, int t0, int c, T (&s)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = ws[(size_t)(t0 + k) * channels + c];
#pragma unroll UNROLL
  for (int i = 1; i < slabs; ++i)
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += ws[((size_t)i * terms + t0 + k) * channels + c];
}

}  // namespace rtpose
