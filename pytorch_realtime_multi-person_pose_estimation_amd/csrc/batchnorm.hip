// Training-mode BatchNorm2d (+ ReLU) on layout slices (header section 2b, continued): batch statistics, the normalisation
// from them and the backward through them.  The inference plans fold a BatchNorm's RUNNING statistics into a conv or hand
// them to it as a per-channel (scale, shift); a training forward needs the statistics of the batch itself.
//
//   rtpose_bn_stats  per channel c over the P = N H W valid pixels, K[c] = x[0, 0, 0, c]:
//                      S1 = sum (x - K), S2 = sum (x - K)^2                         (fp64; the SHIFTED sums, one pass)
//                      md = S1 / P; mean = K + md; var = max(S2 / P - md * md, 0)   (fp64; NaN stays NaN)
//                      invstd = 1 / sqrt(var + eps); scale = weight * invstd; shift = bias - mean * scale   (fp64)
//                    save[0..5][c] = fp32(mean), fp32(var), fp32(invstd), fp32(scale), fp32(shift), fp32(mean - fp32(mean))
//                    running_mean = fp32((1 - m) * running_mean + m * mean),
//                    running_var  = fp32((1 - m) * running_var + m * (var * P / (P - 1)))           (fp64, if given)
//   rtpose_bn_apply  y = scale[c] * x + shift[c] (one fp32 multiply, one fp32 add; the library is built with
//                    -ffp-contract=off), then relu: y <= 0 ? +0 : y (a NaN y stays NaN, as torch's relu has it)
//   rtpose_bn_grad   g = relu ? (scale[c] * x + shift[c] > 0 ? gy : 0) : gy      (the mask RECOMPUTED from x: apply's bits)
//                      G1 = sum g, G2 = sum g * (x - K)                              (fp64)
//                      mdk = (mean + mean_lo) - K; dbias = G1; dweight = invstd * (G2 - mdk * G1)   (fp64 -> fp32)
//                      A = weight * invstd; B = A * G1 / P; C = A * invstd * dweight / P            (fp64 -> fp32 each)
//                    dx = (g * A - B) - (x - mean) * C       (fp32: a multiply, a subtract, a subtract and a multiply, a subtract)
//
// Sums and walks: chan_slab.h.  The two sum passes add their two terms per channel in fp64 (an fp32 value and the product
// of two are exact there) and take both through LDS in one pass; the slab's partials are [slab][2][channels] doubles, and
// the second launch of one thread per channel adds them in slab order and finalises.  apply and dx are the element-wise
// passes.  Every element reads only its own x / gy element, so y may name the slice x names and dx the slice gy names.
//
// And the two element-wise passes between the bf16 convs of a layout-resident training run (train.preact_chain): the same
// device code with the store rounded to bf16 (OUT = uint16_t; bf16_dest.h), straight into the slice the next conv reads.
//
//   rtpose_bn_apply_bf16  y  = bf16(rtpose_bn_apply's fp32 y)
//   rtpose_bn_grad_bf16   dx = bf16(rtpose_bn_grad's fp32 dx); the sum pass and the finalising launch ARE rtpose_bn_grad's
//
// bf16(): round to nearest even as rtpose_layout_f32_to_bf16 rounds (Inf stays Inf, a NaN stays a NaN of its sign), so the
// bits are those of the fp32 entry point followed by rtpose_layout_f32_to_bf16.  The bf16 destination lies bytes apart from
// every input and is 2-byte aligned; its 4-channel units ask aligned8_bf16 of it where the fp32 ones ask aligned16.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "bf16_dest.h"
#include "chan_slab.h"

namespace rtpose {
namespace {

constexpr int kFinalThreads = 64;
static_assert(RTPOSE_BN_SAVE_ROWS == 6, "save rows: mean, var, invstd, scale, shift, mean_lo");

bool shape_ok(int channels, int N, int H, int W) { return channels >= 1 && pixel_count(N, H, W) > 1; }

// slabs * 2 * channels partials + 2 * channels (the three fp32 dx coefficients of a channel)
size_t ws_doubles(int channels, const SlabGeom& g) { return (size_t)g.slabs * 2 * (size_t)channels + 2 * (size_t)channels; }

struct BnArgs {
  const float* x;
  const float* gy;     // grad only
  const float* save;   // [kSaveRows][channels]; NULL for the statistics
  const float* coef;   // [3][channels] A, B, C: the dx pass
  void* out;           // y / dx: float, or bf16 bits
  double* ws;          // [slab][2][channels] partials: the two sum passes
  Lay lx, lgy, lout;
  int channels, H, W, P;
  int slab;
  int relu;
  Rect r;
  FastDiv d_w, d_h;
};

enum { kStats = 0, kGradSums = 1, kApply = 2, kGradDx = 3 };

// OUT: float, or uint16_t for a bf16 destination (the element-wise passes only)
template <int V, int MODE, class OUT = float>
__global__ __launch_bounds__(kThreads) void bn_kernel(const BnArgs a) {
  constexpr bool SUM = MODE == kStats || MODE == kGradSums;
  constexpr bool GRAD = MODE == kGradSums || MODE == kGradDx;
  const Place t = place<V>(a.r, a.channels, a.slab, a.P);

  // per channel: the shift K of the sums, the fp32 (scale, shift) of apply and of the mask, mean and the dx coefficients
  double kk[V], acc[2][V];
  float sc[V], sh[V], mean[V], cA[V], cB[V], cC[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool on = t.live && v < t.nc;
    const int c = t.c0 + v;
    kk[v] = (SUM && on) ? (double)a.x[lay_off(a.lx, 0, 0, 0) + c] : 0.0;
    sc[v] = (MODE != kStats && on) ? a.save[3 * a.channels + c] : 0.f;
    sh[v] = (MODE != kStats && on) ? a.save[4 * a.channels + c] : 0.f;
    mean[v] = (MODE == kGradDx && on) ? a.save[c] : 0.f;
    cA[v] = (MODE == kGradDx && on) ? a.coef[c] : 0.f;
    cB[v] = (MODE == kGradDx && on) ? a.coef[a.channels + c] : 0.f;
    cC[v] = (MODE == kGradDx && on) ? a.coef[2 * a.channels + c] : 0.f;
    acc[0][v] = acc[1][v] = 0.0;
  }

  if (t.live) {
    // (unrolled: the sum passes store nothing, so the loads of four pixels are in flight; the additions keep their order)
#pragma unroll 4
    for (int p = t.p0 + t.row; p < t.p1; p += a.r.ty) {
      const Pixel q = pixel_of(p, a.H, a.W, a.d_h, a.d_w);
      const Unit<V> xv = fetch<V>(a.x, lay_off(a.lx, q) + t.c0, t);
      Unit<V> gv = xv, res;
      if (GRAD) gv = fetch<V>(a.gy, lay_off(a.lgy, q) + t.c0, t);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        float y = 0.f;
        if (MODE != kStats) {
          y = sc[v] * xv.v[v];
          y = y + sh[v];
        }
        // the gradient through the ReLU: gy's bits where apply's y > 0, +0 elsewhere (a NaN y: +0; apply stores that NaN, so the
        // loss is NaN already)
        const float g = (GRAD && a.relu) ? (y > 0.f ? gv.v[v] : 0.f) : gv.v[v];
        if (MODE == kStats) {
          const double d = (double)xv.v[v] - kk[v];
          acc[0][v] += d;
          acc[1][v] += d * d;
        } else if (MODE == kGradSums) {
          const double d = (double)xv.v[v] - kk[v];
          acc[0][v] += (double)g;
          acc[1][v] += (double)g * d;
        } else if (MODE == kApply) {
          res.v[v] = a.relu ? (y <= 0.f ? 0.f : y) : y;  // torch's relu: a NaN y stays NaN
        } else {
          const float xm = xv.v[v] - mean[v];
          float t0 = g * cA[v];
          t0 = t0 - cB[v];
          const float u = xm * cC[v];
          res.v[v] = t0 - u;
        }
      }
      if constexpr (!SUM) {
        if constexpr (std::is_same_v<OUT, float>)
          store<V>(static_cast<float*>(a.out), lay_off(a.lout, q) + t.c0, t, res);
        else
          store_bf16<V>(static_cast<uint16_t*>(a.out), lay_off(a.lout, q) + t.c0, t, res);
      }
    }
  }

  if constexpr (SUM) sum_rows<V, 2, 2>(t, a.r, acc, a.ws, a.channels);
}

struct FinalArgs {
  const double* ws;
  const float* x0;      // channel 0 of the slice at pixel (0, 0, 0): K
  const float* weight;
  const float* bias;    // statistics only
  float* running_mean;  // or NULL (both)
  float* running_var;
  float* save;          // written by the statistics, read by the gradient
  float* coef;          // gradient: [3][channels], or NULL (no dx)
  float* dweight;       // or NULL
  float* dbias;         // or NULL
  double momentum, eps;
  int slabs, channels, P;
};

// thread c < channels
__global__ __launch_bounds__(kFinalThreads) void bn_stats_final_kernel(const FinalArgs a) {
  const int c = (int)blockIdx.x * kFinalThreads + threadIdx.x;
  if (c >= a.channels) return;
  double s[2];
  sum_slabs<2, 1>(a.ws, a.slabs, 2, a.channels, 0, c, s);
  const double s1 = s[0], s2 = s[1];
  const double P = (double)a.P;
  const double md = s1 / P;
  const double mean = (double)a.x0[c] + md;
  double var = s2 / P - md * md;
  var = var <= 0.0 ? 0.0 : var;  // (this way round a NaN variance stays NaN; `var > 0 ? var : 0` would store 0 and a finite scale)
  const double invstd = 1.0 / sqrt(var + a.eps);
  const double scale = (double)a.weight[c] * invstd;
  const double shift = (double)a.bias[c] - mean * scale;
  const float meanf = (float)mean;
  a.save[c] = meanf;
  a.save[a.channels + c] = (float)var;
  a.save[2 * a.channels + c] = (float)invstd;
  a.save[3 * a.channels + c] = (float)scale;
  a.save[4 * a.channels + c] = (float)shift;
  a.save[5 * a.channels + c] = (float)(mean - (double)meanf);
  if (a.running_mean) {
    const double keep = 1.0 - a.momentum;
    const double unbiased = var * P / (double)(a.P - 1);
    a.running_mean[c] = (float)(keep * (double)a.running_mean[c] + a.momentum * mean);
    a.running_var[c] = (float)(keep * (double)a.running_var[c] + a.momentum * unbiased);
  }
}

__global__ __launch_bounds__(kFinalThreads) void bn_grad_final_kernel(const FinalArgs a) {
  const int c = (int)blockIdx.x * kFinalThreads + threadIdx.x;
  if (c >= a.channels) return;
  double s[2];
  sum_slabs<2, 1>(a.ws, a.slabs, 2, a.channels, 0, c, s);
  const double g1 = s[0], g2 = s[1];
  const double P = (double)a.P;
  const double mean = (double)a.save[c] + (double)a.save[5 * a.channels + c];
  const double mdk = mean - (double)a.x0[c];
  const double invstd = (double)a.save[2 * a.channels + c];
  const double dw = invstd * (g2 - mdk * g1);
  if (a.dbias) a.dbias[c] = (float)g1;
  if (a.dweight) a.dweight[c] = (float)dw;
  if (a.coef) {
    const double A = (double)a.weight[c] * invstd;
    a.coef[c] = (float)A;
    a.coef[a.channels + c] = (float)(A * g1 / P);
    a.coef[2 * a.channels + c] = (float)(A * invstd * dw / P);
  }
}

int check_shape_bn(const char* who, int channels, int N, int H, int W, long& P) {
  if (int rc = check_shape(who, channels, N, H, W, P)) return rc;
  if (P == 1)
    return fail(RTPOSE_E_INVAL, "%s: N * H * W = 1: a channel of one value has no batch statistics (torch refuses it too)", who);
  return 0;
}

int check_ws(const char* who, const double* ws, size_t given, int channels, const SlabGeom& g) {
  return check_workspace(who, ws, given, ws_doubles(channels, g), "rtpose_bn_workspace_doubles");
}

// slab: g.slab for the sums; kSlabUnit for apply and dx (element-wise, chan_slab.h), for more workgroups in flight
void fill_args(BnArgs& a, int channels, int H, int W, long P, int slab) {
  a.channels = channels;
  a.H = H;
  a.W = W;
  a.P = (int)P;
  a.slab = slab;
  a.d_w = make_fastdiv(W);
  a.d_h = make_fastdiv(H);
}

template <int MODE, class OUT = float>
void launch_bn(bool vec, dim3 grid, hipStream_t s, const BnArgs& a) {
  launch_units<bn_kernel<4, MODE, OUT>, bn_kernel<1, MODE, OUT>>(vec, grid, s, a);
}

// whether a destination slice takes the 4-channel units
template <class OUT>
bool dest_vec(const rtpose_layout& l, const void* p) {
  if constexpr (std::is_same_v<OUT, float>)
    return aligned16(l, p);
  else
    return aligned8_bf16(l, p);
}

// what the bf16 entry points ask of their destination beside check_slice: 2-byte aligned, and bytes apart from x, gy (or
// NULL), save and weight (or NULL); 0 or fail(...)
int check_dest(const char* who, const char* what, const void* out, const rtpose_layout& lout, const float* x,
               const rtpose_layout& lx, const float* gy, const rtpose_layout* lgy, const float* save, const float* weight,
               int channels, int N, int H, int W) {
  if (reinterpret_cast<uintptr_t>(out) % 2) return fail(RTPOSE_E_INVAL, "%s: %s must be 2-byte aligned", who, what);
  if (int rc = check_apart_slice(who, "x", out, lout, x, lx, channels, N, H, W)) return rc;
  if (gy)
    if (int rc = check_apart_slice(who, "gy", out, lout, gy, *lgy, channels, N, H, W)) return rc;
  if (int rc = check_apart_vector(who, "save", out, lout, save, (size_t)RTPOSE_BN_SAVE_ROWS * channels, channels, N, H, W))
    return rc;
  if (weight)
    if (int rc = check_apart_vector(who, "weight", out, lout, weight, (size_t)channels, channels, N, H, W)) return rc;
  return 0;
}

// rtpose_bn_apply (OUT = float) and rtpose_bn_apply_bf16 (OUT = uint16_t)
template <class OUT>
int bn_apply(const char* who, const float* x, const rtpose_layout* lx, const float* save, void* y, const rtpose_layout* ly,
             int relu, int channels, int N, int H, int W, void* stream) {
  constexpr bool kBf16 = !std::is_same_v<OUT, float>;
  long P;
  if (int rc = check_shape_bn(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "x", x, lx, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "y", y, ly, channels, H, W, 0)) return rc;
  if (!save) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (save)", who);
  if constexpr (kBf16)
    if (int rc = check_dest(who, "y", y, *ly, x, *lx, nullptr, nullptr, save, nullptr, channels, N, H, W)) return rc;

  BnArgs a{};
  a.x = x;
  a.save = save;
  a.out = y;
  a.lx = a.lgy = to_lay(lx);
  a.lout = to_lay(ly);
  a.relu = relu ? 1 : 0;
  fill_args(a, channels, H, W, P, kSlabUnit);
  const bool vec = aligned16(*lx, x) && dest_vec<OUT>(*ly, y);
  dim3 grid;
  if (int rc = set_rectangle(a.r, channels, vec ? 4 : 1, ceil_div(a.P, kSlabUnit), grid, who)) return rc;

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_x, c_s, c_y;
  const int dev = current_device();
  int rc = c_x.check(x, dev, who, "x");
  if (!rc) rc = c_s.check(save, dev, who, "save");
  if (!rc) rc = c_y.check(y, dev, who, "y");
  if (rc) return rc;

  launch_bn<kApply, OUT>(vec, grid, as_stream(stream), a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

// rtpose_bn_grad (OUT = float) and rtpose_bn_grad_bf16 (OUT = uint16_t): the sum pass and the finalising launch are the
// same instances for both, the dx pass is OUT's
template <class OUT>
int bn_grad(const char* who, const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy,
            const float* save, const float* weight, int relu, void* dx, const rtpose_layout* ldx, float* dweight, float* dbias,
            double* workspace, size_t workspace_doubles, int channels, int N, int H, int W, void* stream) {
  constexpr bool kBf16 = !std::is_same_v<OUT, float>;
  long P;
  if (int rc = check_shape_bn(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "x", x, lx, channels, H, W, 0)) return rc;
  if (int rc = check_slice(who, "gy", gy, lgy, channels, H, W, 0)) return rc;
  if (dx)
    if (int rc = check_slice(who, "dx", dx, ldx, channels, H, W, 0)) return rc;
  if (!save || !weight) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (save or weight)", who);
  if (!dx && !dweight && !dbias) return fail(RTPOSE_E_INVAL, "%s: nothing to compute (dx, dweight and dbias are all NULL)", who);
  if constexpr (kBf16)
    if (dx)
      if (int rc = check_dest(who, "dx", dx, *ldx, x, *lx, gy, lgy, save, weight, channels, N, H, W)) return rc;
  const SlabGeom g = slab_geometry(P);
  if (int rc = check_ws(who, workspace, workspace_doubles, channels, g)) return rc;

  BnArgs a{};
  a.x = x;
  a.gy = gy;
  a.save = save;
  a.ws = workspace;
  a.lx = to_lay(lx);
  a.lgy = to_lay(lgy);
  a.lout = to_lay(dx ? ldx : lgy);
  a.relu = relu ? 1 : 0;
  fill_args(a, channels, H, W, P, g.slab);
  float* coef = reinterpret_cast<float*>(workspace + (size_t)g.slabs * 2 * (size_t)channels);
  const bool vec_in = aligned16(*lx, x) && aligned16(*lgy, gy);
  const bool vec = vec_in && (!dx || dest_vec<OUT>(*ldx, dx));
  dim3 grid_in, grid;
  if (int rc = set_rectangle(a.r, channels, vec_in ? 4 : 1, g.slabs, grid_in, who)) return rc;

  // (statics of a function template: each entry point has its own set)
  static thread_local CheckedPtr c_x, c_gy, c_s, c_w, c_dx, c_dw, c_db, c_ws;
  const int dev = current_device();
  int rc = c_x.check(x, dev, who, "x");
  if (!rc) rc = c_gy.check(gy, dev, who, "gy");
  if (!rc) rc = c_s.check(save, dev, who, "save");
  if (!rc) rc = c_w.check(weight, dev, who, "weight");
  if (!rc && dx) rc = c_dx.check(dx, dev, who, "dx");
  if (!rc && dweight) rc = c_dw.check(dweight, dev, who, "dweight");
  if (!rc && dbias) rc = c_db.check(dbias, dev, who, "dbias");
  if (!rc) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  launch_bn<kGradSums>(vec_in, grid_in, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  FinalArgs f{};
  f.ws = workspace;
  f.x0 = x + ((size_t)lx->lead * lx->cstride + lx->choff);
  f.weight = weight;
  f.save = const_cast<float*>(save);
  f.coef = dx ? coef : nullptr;
  f.dweight = dweight;
  f.dbias = dbias;
  f.slabs = g.slabs;
  f.channels = channels;
  f.P = a.P;
  hipLaunchKernelGGL(bn_grad_final_kernel, dim3((unsigned)ceil_div(channels, kFinalThreads)), dim3(kFinalThreads), 0, s, f);
  RTPOSE_HIP_CHECK(hipGetLastError());
  if (dx) {
    a.out = dx;
    a.coef = coef;
    a.slab = kSlabUnit;
    if (int rc2 = set_rectangle(a.r, channels, vec ? 4 : 1, ceil_div(a.P, kSlabUnit), grid, who)) return rc2;
    launch_bn<kGradDx, OUT>(vec, grid, s, a);
    RTPOSE_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace rtpose

extern "C" {

using namespace rtpose;

size_t rtpose_bn_workspace_doubles(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return ws_doubles(channels, slab_geometry(pixel_count(N, H, W)));
}

int rtpose_bn_slabs(int channels, int N, int H, int W) {
  if (!shape_ok(channels, N, H, W)) return 0;
  return slab_geometry(pixel_count(N, H, W)).slabs;
}

int rtpose_bn_stats(const float* x, const rtpose_layout* lx, const float* weight, const float* bias, float* running_mean,
                    float* running_var, double momentum, double eps, float* save, double* workspace,
                    size_t workspace_doubles, int channels, int N, int H, int W, void* stream) {
  const char* who = "bn_stats";
  long P;
  if (int rc = check_shape_bn(who, channels, N, H, W, P)) return rc;
  if (int rc = check_slice(who, "x", x, lx, channels, H, W, 0)) return rc;
  if (!weight || !bias || !save) return fail(RTPOSE_E_INVAL, "%s: NULL buffer (weight, bias or save)", who);
  if ((running_mean == nullptr) != (running_var == nullptr))
    return fail(RTPOSE_E_INVAL, "%s: running_mean and running_var are given together or not at all", who);
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(RTPOSE_E_INVAL, "%s: eps must be a positive finite number", who);
  if (running_mean && !(momentum >= 0.0 && momentum <= 1.0))
    return fail(RTPOSE_E_INVAL, "%s: momentum must lie in [0, 1]", who);
  const SlabGeom g = slab_geometry(P);
  if (int rc = check_ws(who, workspace, workspace_doubles, channels, g)) return rc;

  BnArgs a{};
  a.x = x;
  a.ws = workspace;
  a.lx = a.lgy = a.lout = to_lay(lx);
  fill_args(a, channels, H, W, P, g.slab);
  const bool vec = aligned16(*lx, x);
  dim3 grid;
  if (int rc = set_rectangle(a.r, channels, vec ? 4 : 1, g.slabs, grid, who)) return rc;

  static thread_local CheckedPtr c_x, c_w, c_b, c_rm, c_rv, c_s, c_ws;
  const int dev = current_device();
  int rc = c_x.check(x, dev, who, "x");
  if (!rc) rc = c_w.check(weight, dev, who, "weight");
  if (!rc) rc = c_b.check(bias, dev, who, "bias");
  if (!rc && running_mean) rc = c_rm.check(running_mean, dev, who, "running_mean");
  if (!rc && running_var) rc = c_rv.check(running_var, dev, who, "running_var");
  if (!rc) rc = c_s.check(save, dev, who, "save");
  if (!rc) rc = c_ws.check(workspace, dev, who, "workspace");
  if (rc) return rc;

  hipStream_t s = as_stream(stream);
  launch_bn<kStats>(vec, grid, s, a);
  RTPOSE_HIP_CHECK(hipGetLastError());
  FinalArgs f{};
  f.ws = workspace;
  f.x0 = x + ((size_t)lx->lead * lx->cstride + lx->choff);
  f.weight = weight;
  f.bias = bias;
  f.running_mean = running_mean;
  f.running_var = running_var;
  f.save = save;
  f.momentum = momentum;
  f.eps = eps;
  f.slabs = g.slabs;
  f.channels = channels;
  f.P = a.P;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)ceil_div(channels, kFinalThreads)), dim3(kFinalThreads), 0, s, f);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int rtpose_bn_apply(const float* x, const rtpose_layout* lx, const float* save, float* y, const rtpose_layout* ly, int relu,
                    int channels, int N, int H, int W, void* stream) {
  return bn_apply<float>("bn_apply", x, lx, save, y, ly, relu, channels, N, H, W, stream);
}

int rtpose_bn_apply_bf16(const float* x, const rtpose_layout* lx, const float* save, void* y, const rtpose_layout* ly, int relu,
                         int channels, int N, int H, int W, void* stream) {
  return bn_apply<uint16_t>("bn_apply_bf16", x, lx, save, y, ly, relu, channels, N, H, W, stream);
}

int rtpose_bn_grad(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy, const float* save,
                   const float* weight, int relu, float* dx, const rtpose_layout* ldx, float* dweight, float* dbias,
                   double* workspace, size_t workspace_doubles, int channels, int N, int H, int W, void* stream) {
  return bn_grad<float>("bn_grad", x, lx, gy, lgy, save, weight, relu, dx, ldx, dweight, dbias, workspace, workspace_doubles,
                        channels, N, H, W, stream);
}

int rtpose_bn_grad_bf16(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy, const float* save,
                        const float* weight, int relu, void* dx, const rtpose_layout* ldx, float* dweight, float* dbias,
                        double* workspace, size_t workspace_doubles, int channels, int N, int H, int W, void* stream) {
  return bn_grad<uint16_t>("bn_grad_bf16", x, lx, gy, lgy, save, weight, relu, dx, ldx, dweight, dbias, workspace,
                           workspace_doubles, channels, N, H, W, stream);
}

}  // extern "C"
