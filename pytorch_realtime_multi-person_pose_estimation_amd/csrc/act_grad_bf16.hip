// The gradient through a conv's fused ReLU on bf16 layout slices, for training runs whose activations and gradients stay in
// the layouts between convs (header section 2b; train.conv_chain):
//
//   rtpose_relu_grad_bf16  out[n,y,x,c] = y[n,y,x,c] > 0 ? gy[n,y,x,c] : +0        (all three bf16)
//
// y is the conv's output as it was stored (out_f32 = 0) - the buffer the next conv read -, so the comparison is on the bf16
// value: a bf16 h is positive when 0x0001 <= h <= 0x7f80 (subnormals and +Inf included; +-0, NaN and every negative are
// not).  Where it is, out holds gy's 16 bits untouched; no arithmetic touches a value.
// One kernel template, memory bound, on the rectangle and units of chan_slab.h without its sums: a workgroup takes
// kSlabUnit valid pixels, a thread one unit of V channels (V = 8: one 16-byte load of y and of gy and one 16-byte store per
// pixel, where every base, cstride and choff allows it; V = 1 otherwise; a last unit with fewer than 8 live channels goes
// element by element), two pixels in flight.  No LDS, no scratch, no atomics.
// Every element reads only its own y and gy element, so out / lout may name the slice gy / lgy name.
#include <hip/hip_runtime.h>

#include "chan_slab.h"

namespace rtpose {
namespace {

typedef uint32_t Word4 __attribute__((ext_vector_type(4)));

struct ReluGradBf16Args {
  const uint16_t* y;
  const uint16_t* gy;
  uint16_t* out;
  Lay ly, lgy, lout;
  int channels, H, W, P;
  Rect r;
  FastDiv d_w, d_h;
};

__device__ __forceinline__ bool bf16_positive(uint32_t h) { return h - 1u < 0x7f80u; }  // h: 16 bits, zero-extended

// the two bf16 of a word: gy's halves where y's are positive
__device__ __forceinline__ uint32_t mask_pair(uint32_t yw, uint32_t gw) {
  const uint32_t m = (bf16_positive(yw & 0xffffu) ? 0x0000ffffu : 0u) | (bf16_positive(yw >> 16) ? 0xffff0000u : 0u);
  return gw & m;
}

template <int V>
struct Bits {
  uint32_t w[V == 8 ? 4 : 1];  // V = 8: four words of two bf16; V = 1: one bf16, zero-extended
};

template <int V>
__device__ __forceinline__ Bits<V> fetch_bits(const uint16_t* src, size_t o, const Place& t) {
  Bits<V> b;
  if constexpr (V == 8) {
    if (t.whole) {
      const Word4 f = *reinterpret_cast<const Word4*>(src + o);
      b.w[0] = f.x, b.w[1] = f.y, b.w[2] = f.z, b.w[3] = f.w;
      return b;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t lo = 2 * i < t.nc ? src[o + 2 * i] : 0u, hi = 2 * i + 1 < t.nc ? src[o + 2 * i + 1] : 0u;
      b.w[i] = lo | (hi << 16);
    }
  } else {
    b.w[0] = src[o];
  }
  return b;
}

template <int V>
__device__ __forceinline__ void store_bits(uint16_t* dst, size_t o, const Place& t, const Bits<V>& b) {
  if constexpr (V == 8) {
    if (t.whole) {
      *reinterpret_cast<Word4*>(dst + o) = Word4{b.w[0], b.w[1], b.w[2], b.w[3]};
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (2 * i < t.nc) dst[o + 2 * i] = (uint16_t)(b.w[i] & 0xffffu);
      if (2 * i + 1 < t.nc) dst[o + 2 * i + 1] = (uint16_t)(b.w[i] >> 16);
    }
  } else {
    dst[o] = (uint16_t)b.w[0];
  }
}

// V: channels per unit (8 or 1)
template <int V>
__global__ __launch_bounds__(kThreads) void relu_grad_bf16_kernel(const ReluGradBf16Args a) {
  const Place t = place<V>(a.r, a.channels, kSlabUnit, a.P);
  if (!t.live) return;

  auto pixel = [&](int p, size_t& oy, size_t& og, size_t& oo) {
    const Pixel q = pixel_of(p, a.H, a.W, a.d_h, a.d_w);
    oy = lay_off(a.ly, q) + t.c0;
    og = lay_off(a.lgy, q) + t.c0;
    oo = lay_off(a.lout, q) + t.c0;
  };
  auto finish = [&](size_t oo, const Bits<V>& yv, const Bits<V>& gv) {
    Bits<V> r;
    if constexpr (V == 8) {
#pragma unroll
      for (int i = 0; i < 4; ++i) r.w[i] = mask_pair(yv.w[i], gv.w[i]);
    } else {
      r.w[0] = bf16_positive(yv.w[0]) ? gv.w[0] : 0u;
    }
    store_bits<V>(a.out, oo, t, r);
  };

  // two pixels in flight: both are fetched before either is stored (out may be gy: an element reads only itself)
  for (int p = t.p0 + t.row; p < t.p1; p += 2 * a.r.ty) {
    const int q = p + a.r.ty;
    const bool second = q < t.p1;
    size_t oy0, og0, oo0, oy1, og1, oo1;
    pixel(p, oy0, og0, oo0);
    pixel(second ? q : p, oy1, og1, oo1);  // (the last pixel of an odd walk is fetched twice and stored once)
    const Bits<V> y0 = fetch_bits<V>(a.y, oy0, t), y1 = fetch_bits<V>(a.y, oy1, t);
    const Bits<V> g0 = fetch_bits<V>(a.gy, og0, t), g1 = fetch_bits<V>(a.gy, og1, t);
    finish(oo0, y0, g0);
    if (second) finish(oo1, y1, g1);
  }
}

// 16-byte pieces of 8 bf16: every pixel's slice starts on one
bool aligned16_bf16(const rtpose_layout& l, const void* base) {
  return slice_aligned(l, 8) && reinterpret_cast<uintptr_t>(base) % 16 == 0;
}

bool same_slice(const void* a, const rtpose_layout& la, const void* b, const rtpose_layout& lb) {
  return a == b && la.cstride == lb.cstride && la.choff == lb.choff && la.ws == lb.ws && la.hs == lb.hs && la.lead == lb.lead;
}

// out against a slice it reads: the same slice (in place), channel slices of one buffer that do not meet, or bytes apart
bool out_apart(const void* out, const rtpose_layout& lo, const void* in, const rtpose_layout& li, int channels, int N, int H,
               int W) {
  if (same_slice(out, lo, in, li)) return true;
  if (out == in && lo.cstride == li.cstride && lo.ws == li.ws && lo.hs == li.hs && lo.lead == li.lead)
    return lo.choff + channels <= li.choff || li.choff + channels <= lo.choff;
  uintptr_t o0, o1, i0, i1;
  slice_span_bytes(out, lo, 2, channels, N, H, W, o0, o1);
  slice_span_bytes(in, li, 2, channels, N, H, W, i0, i1);
  return o1 <= i0 || i1 <= o0;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

int rtpose_relu_grad_bf16(const void* y, const rtpose_layout* ly, const void* gy, const rtpose_layout* lgy, void* out,
                          const rtpose_layout* lout, int channels, int N, int H, int W, void* stream) {
  const char* who = "relu_grad_bf16";
  long P;
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "y", y, ly, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "out", out, lout, channels, H, W, 0)) return rc;
  if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(out)) % 2)
    return fail(RTPOSE_E_INVAL, "%s: y, gy and out must be 2-byte aligned", who);
  if (!out_apart(out, *lout, gy, *lgy, channels, N, H, W))
    return fail(RTPOSE_E_INVAL, "%s: out overlaps gy without being the same slice", who);
  if (!out_apart(out, *lout, y, *ly, channels, N, H, W))
    return fail(RTPOSE_E_INVAL, "%s: out overlaps y without being the same slice", who);

  ReluGradBf16Args a;
  a.y = static_cast<const uint16_t*>(y);
  a.gy = static_cast<const uint16_t*>(gy);
  a.out = static_cast<uint16_t*>(out);
  a.ly = to_lay(ly);
  a.lgy = to_lay(lgy);
  a.lout = to_lay(lout);
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = (int)P;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
  const bool vec = aligned16_bf16(*ly, y) && aligned16_bf16(*lgy, gy) && aligned16_bf16(*lout, out);
  dim3 grid;
  if (int rc = set_rectangle(a.r, channels, vec ? 8 : 1, (int)((P + kSlabUnit - 1) / kSlabUnit), grid, who)) return rc;

  static thread_local CheckedPtr c_y, c_gy, c_out;
  const int dev = current_device();
  int rc = c_y.check(y, dev, who, "y");
  if (!rc) rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_out.check(out, dev, who, "out");
  if (rc) return rc;

  launch_units<relu_grad_bf16_kernel<8>, relu_grad_bf16_kernel<1>>(vec, grid, as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
