// People -> heat-map / PAF training targets on the device, for any skeleton (header section 4b), and the reference's
// per-stage loss term read off a plan's padded-NHWC view (rtpose_stage_mse).
//
//   lib/datasets/datasets.py:259-308 (get_ground_truth), lib/datasets/heatmap.py:20-36 (putGaussianMaps),
//   lib/datasets/paf.py:18-68 (putVecMaps), train/train_VGG19.py:143-174 (get_loss: nn.MSELoss(reduction='mean'))
//
// The targets follow the reference OPERATION FOR OPERATION in fp64 (-ffp-contract=off: the order written is the order
// executed) and are rounded to fp32 at the store: the three decisions `e <= 4.6052`, `|cross| < 1` and the half-even
// rounding of the limb box are discontinuities, a flipped one changes a PAF cell by up to 1.
//
// Two launches.  encode_prep_kernel writes one record per (image, person) into the workspace: per part (x, y, present),
// per limb (a, u, the box, valid).  encode_raster_kernel, grid (row pieces, h, N), owns whole cells: a thread per
// (cell, channel) walks the image's people IN PEOPLE ORDER through LDS in chunks of RTPOSE_ENCODE_CHUNK records, so
// max_people has no small cap and the sums do not depend on the launch geometry.  No atomics anywhere.  The skeleton
// travels by value as a launch argument of the prep kernel, as in decode.hip, and the raster kernel gets the small
// channel map made from it on the host: nothing is uploaded.
//
// Built like decode.hip without the vectorisers (csrc/Makefile): these kernels may run beside a forward.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = RTPOSE_ENCODE_CHUNK;
constexpr int kMaxHeat = RTPOSE_SKEL_MAX_PARTS + 1;   // parts + background
constexpr int kMaxPaf = 2 * RTPOSE_SKEL_MAX_LIMBS;
constexpr int kPartWords = 3;  // x, y, present (1.0 / 0.0)
constexpr int kLimbWords = 7;  // ax, ay, ux, uy, (x0, x1), (y0, y1), (valid, 0): 8-byte words

struct Box {
  int32_t lo, hi;
};

// which limb writes a PAF channel, and which component of its unit vector (-1: no limb names the channel, it is
// written as 0).  Where two limbs name one channel the first in table order owns it.
struct ChanMap {
  int8_t limb[kMaxPaf];
  int8_t comp[kMaxPaf];
};

struct Geom {
  int h, w, stride, CH, CP, P, L, bg, cells, words, max_people;
  double sigma, start, input_w, input_h;
};

__device__ __forceinline__ int people_of(const int32_t* n_people, int n, int max_people) {
  if (!n_people) return max_people;
  const int v = n_people[n];
  return v < 0 ? 0 : (v > max_people ? max_people : v);
}

// One thread per (image, person, part or limb).  remove_illegal_joint (datasets.py:216-225) and the `> 0.5` tests of
// :280 / :291 become `present`; paf.py:19-38 becomes a limb's a, u and box.
__global__ __launch_bounds__(kThreads) void encode_prep_kernel(const double* __restrict__ kp,
                                                               const int32_t* __restrict__ n_people, int total,
                                                               const Geom g, const rtpose_skeleton skel,
                                                               const FastDiv d_items, const FastDiv d_people,
                                                               double* __restrict__ ws) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int items = g.P + g.L;
  const int person = fast_div(t, d_items);
  const int item = t - person * items;
  const int n = fast_div(person, d_people);
  const int k = person - n * g.max_people;
  if (k >= people_of(n_people, n, g.max_people)) return;
  const double* q = kp + (size_t)person * g.P * 3;
  double* rec = ws + (size_t)person * g.words;
  auto present = [&](int j) -> bool {
    const double x = q[3 * j], y = q[3 * j + 1], v = q[3 * j + 2];
    return v > 0.5 && x >= 0.0 && x < g.input_w && y >= 0.0 && y < g.input_h;
  };
  if (item < g.P) {
    double* r = rec + kPartWords * item;
    r[0] = q[3 * item];
    r[1] = q[3 * item + 1];
    r[2] = present(item) ? 1.0 : 0.0;
    return;
  }
  const int l = item - g.P;
  double* r = rec + kPartWords * g.P + kLimbWords * l;
  const int A = skel.limb_part[l][0], B = skel.limb_part[l][1];
  double ax = 0.0, ay = 0.0, ux = 0.0, uy = 0.0;
  Box bx = {0, 0}, by = {0, 0}, valid = {0, 0};
  if (present(A) && present(B)) {
    const double s = (double)g.stride;
    const double bxx = q[3 * B] / s, byy = q[3 * B + 1] / s;
    ax = q[3 * A] / s;
    ay = q[3 * A + 1] / s;
    const double vx = bxx - ax, vy = byy - ay;
    const double nrm = sqrt(vx * vx + vy * vy);
    if (nrm != 0.0) {
      ux = vx / nrm;
      uy = vy / nrm;
      // present parts lie in [0, input): the rounded bounds are small integers
      bx.lo = max((int)rint(fmin(ax, bxx) - 1.0), 0);
      bx.hi = min((int)rint(fmax(ax, bxx) + 1.0), g.w);
      by.lo = max((int)rint(fmin(ay, byy) - 1.0), 0);
      by.hi = min((int)rint(fmax(ay, byy) + 1.0), g.h);
      valid.lo = 1;
    }
  }
  r[0] = ax;
  r[1] = ay;
  r[2] = ux;
  r[3] = uy;
  reinterpret_cast<Box*>(r)[4] = bx;
  reinterpret_cast<Box*>(r)[5] = by;
  reinterpret_cast<Box*>(r)[6] = valid;
}

// grid (row pieces, h, N).  A block owns g.cells whole cells of one row: thread t is channel t % (CH + CP) of cell
// t / (CH + CP), the heat map's channels first.  LDS: the chunk of person records (dynamic) and the cell's part values for
// the background channel.
__global__ __launch_bounds__(kThreads) void encode_raster_kernel(const double* __restrict__ ws,
                                                                 const int32_t* __restrict__ n_people, const Geom g,
                                                                 const ChanMap cm, const FastDiv d_chan,
                                                                 float* __restrict__ heat, float* __restrict__ paf) {
  extern __shared__ double recs[];           // kChunk * g.words
  __shared__ double part_val[kThreads];      // [cell][part]: cells * P <= cells * (CH + CP) <= kThreads
  const int t = threadIdx.x;
  const int ctot = g.CH + g.CP;
  const int cell = fast_div(t, d_chan);
  const int c = t - cell * ctot;
  const int x = blockIdx.x * g.cells + cell;
  const int y = blockIdx.y, n = blockIdx.z;
  const bool active = cell < g.cells && x < g.w;
  // role of the thread: a part's Gaussian sum, a limb's running average, or a value that needs no people
  const bool is_part = active && c < g.P;
  int limb = -1, comp = 0;
  if (active && c >= g.CH) {
    limb = cm.limb[c - g.CH];
    comp = cm.comp[c - g.CH];
  }
  const double gx = (double)(x * g.stride) + g.start, gy = (double)(y * g.stride) + g.start;
  const double fx = (double)x, fy = (double)y;
  double acc = 0.0;
  int count = 0;
  const int np = people_of(n_people, n, g.max_people);
  for (int base = 0; base < np; base += kChunk) {
    const int cnt = min(kChunk, np - base);
    __syncthreads();  // the chunk before has been consumed
    const double* src = ws + ((size_t)n * g.max_people + base) * g.words;
    for (int i = t; i < cnt * g.words; i += kThreads) recs[i] = src[i];
    __syncthreads();
    if (is_part) {
      for (int k = 0; k < cnt; ++k) {
        const double* r = recs + k * g.words + kPartWords * c;
        if (r[2] == 0.0) continue;
        const double dx = gx - r[0], dy = gy - r[1];
        const double e = (dx * dx + dy * dy) / 2.0 / g.sigma / g.sigma;
        if (e <= 4.6052) acc += exp(-e);
        if (acc > 1.0) acc = 1.0;
      }
    } else if (limb >= 0) {
      for (int k = 0; k < cnt; ++k) {
        const double* r = recs + k * g.words + kPartWords * g.P + kLimbWords * limb;
        const Box* b = reinterpret_cast<const Box*>(r);
        if (!b[6].lo) continue;
        const double ax = r[0], ay = r[1], ux = r[2], uy = r[3];
        bool m = x >= b[4].lo && x < b[4].hi && y >= b[5].lo && y < b[5].hi;
        if (m) m = fabs((fx - ax) * uy - (fy - ay) * ux) < 1.0;
        // paf.py:53-54: the count moves where the masked unit vector has a non-zero component
        m = m && (fabs(ux) > 0.0 || fabs(uy) > 0.0);
        acc = acc * (double)count;
        if (m) {
          acc += comp ? uy : ux;
          count += 1;
        }
        acc = acc / (double)max(count, 1);
      }
    }
  }
  if (is_part) part_val[cell * g.P + c] = acc;
  __syncthreads();
  if (!active) return;
  const size_t pix = ((size_t)n * g.h + y) * g.w + x;
  if (c < g.CH) {
    if (c == g.P && g.bg) {  // datasets.py:304-307
      double mx = part_val[cell * g.P];
      for (int j = 1; j < g.P; ++j) mx = fmax(mx, part_val[cell * g.P + j]);
      acc = fmax(1.0 - mx, 0.0);
    }
    heat[pix * g.CH + c] = (float)acc;  // channels behind the parts (and background) stay 0
  } else {
    paf[pix * g.CP + (c - g.CH)] = (float)acc;
  }
}

int check_encode_cfg(const rtpose_encode_cfg* cfg, const rtpose_skeleton* skel, int heat_channels, int paf_channels) {
  if (!cfg) return fail(RTPOSE_E_INVAL, "encode: NULL cfg");
  if (cfg->struct_bytes != sizeof(rtpose_encode_cfg))
    return fail(RTPOSE_E_INVAL, "encode: cfg.struct_bytes is %u, this library's rtpose_encode_cfg has %zu",
                cfg->struct_bytes, sizeof(rtpose_encode_cfg));
  if (!skel) return fail(RTPOSE_E_INVAL, "encode: NULL skeleton");
  if (heat_channels > kMaxHeat || paf_channels > kMaxPaf)
    return fail(RTPOSE_E_INVAL, "encode: heat_channels %d / paf_channels %d above %d / %d", heat_channels, paf_channels,
                kMaxHeat, kMaxPaf);
  if (int rc = rtpose_skeleton_check(skel, heat_channels, paf_channels)) return rc;
  if (cfg->background && heat_channels <= skel->num_parts)
    return fail(RTPOSE_E_INVAL, "encode: background wants heat channel %d but heat_channels is %d", skel->num_parts,
                heat_channels);
  if (cfg->stride < 1) return fail(RTPOSE_E_INVAL, "encode: stride %d below 1", cfg->stride);
  if (!(cfg->sigma > 0.0)) return fail(RTPOSE_E_INVAL, "encode: sigma %g is not greater than 0", cfg->sigma);
  if (cfg->input_h < 1 || cfg->input_w < 1 || cfg->input_h / cfg->stride < 1 || cfg->input_w / cfg->stride < 1)
    return fail(RTPOSE_E_INVAL, "encode: input size %d x %d gives an empty grid at stride %d", cfg->input_h, cfg->input_w,
                cfg->stride);
  if (cfg->input_h / cfg->stride > 65535)
    return fail(RTPOSE_E_INVAL, "encode: grid height %d above the launch limit 65535", cfg->input_h / cfg->stride);
  return 0;
}

inline int record_words(const rtpose_skeleton* skel) { return kPartWords * skel->num_parts + kLimbWords * skel->num_limbs; }

// what the prep kernel's 1-D grid and the people loops can index
int check_people(int N, int max_people, const rtpose_skeleton* skel) {
  if (N < 0 || N > 65535) return fail(RTPOSE_E_INVAL, "encode: N %d outside [0,65535] (grid limit)", N);
  if (max_people < 0) return fail(RTPOSE_E_INVAL, "encode: max_people %d is negative", max_people);
  if ((long long)N * max_people * (skel->num_parts + skel->num_limbs) > 0x7fffff00ll)
    return fail(RTPOSE_E_INVAL, "encode: N %d x max_people %d records above the launch limit", N, max_people);
  return 0;
}

constexpr int kMseThreads = 256;
constexpr int kMsePerBlock = 4 * kMseThreads;
constexpr int kMseMaxBlocks = 4096;

int mse_blocks(long long total) {
  const long long b = (total + kMsePerBlock - 1) / kMsePerBlock;
  return (int)(b < 1 ? 1 : (b > kMseMaxBlocks ? kMseMaxBlocks : b));
}

__device__ __forceinline__ double block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  for (int o = kMseThreads / 2; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
  }
  __syncthreads();
  return s[0];
}

// Stage 1: block b sums (pred - target)^2 over the elements b * 256 + t + k * gridDim.x * 256 of the dense (n, y, x, c)
// order, each thread in ascending order, then a fixed tree over the block.
__global__ __launch_bounds__(kMseThreads) void stage_mse_partial_kernel(const float* __restrict__ pred, const Lay lp,
                                                                        const float* __restrict__ target, int total,
                                                                        int h, int w, int C, const FastDiv dC,
                                                                        const FastDiv dW, const FastDiv dH,
                                                                        double* __restrict__ partials) {
  __shared__ double s[kMseThreads];
  double sum = 0.0;
  const long long step = (long long)gridDim.x * kMseThreads;
  for (long long i = (long long)blockIdx.x * kMseThreads + threadIdx.x; i < total; i += step) {
    const int e = (int)i;
    const int pix = fast_div(e, dC), c = e - pix * C;
    const int row = fast_div(pix, dW), x = pix - row * w;
    const int n = fast_div(row, dH), y = row - n * h;
    const double d = (double)pred[lay_off(lp, n, y, x) + c] - (double)target[e];
    sum += d * d;
  }
  const double b = block_sum(sum, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

// Stage 2: one block adds the partials in a fixed order and writes fp32(sum / count).
__global__ __launch_bounds__(kMseThreads) void stage_mse_final_kernel(const double* __restrict__ partials, int count,
                                                                      double elements, float* __restrict__ loss) {
  __shared__ double s[kMseThreads];
  double sum = 0.0;
  for (int i = threadIdx.x; i < count; i += kMseThreads) sum += partials[i];
  const double b = block_sum(sum, s);
  if (threadIdx.x == 0) *loss = (float)(b / elements);
}

}  // namespace
}  // namespace rtpose

using namespace rtpose;

extern "C" {

size_t rtpose_encode_workspace_bytes(const rtpose_encode_cfg* cfg, const rtpose_skeleton* skel, int N, int max_people) {
  if (!cfg || cfg->struct_bytes != sizeof(rtpose_encode_cfg) || !skel) return 0;
  if (rtpose_skeleton_check(skel, kMaxHeat, kMaxPaf) || check_people(N, max_people, skel)) return 0;
  const size_t bytes = (size_t)N * max_people * record_words(skel) * sizeof(double);
  return round_up(bytes < 1 ? 1 : bytes, 256);
}

int rtpose_encode_targets_skel(const double* keypoints, const int32_t* n_people, int N, int max_people,
                               const rtpose_encode_cfg* cfg, const rtpose_skeleton* skel, int heat_channels,
                               int paf_channels, float* heat, float* paf, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!keypoints) return fail(RTPOSE_E_INVAL, "encode: NULL keypoints");
  if (!heat) return fail(RTPOSE_E_INVAL, "encode: NULL heat");
  if (!paf) return fail(RTPOSE_E_INVAL, "encode: NULL paf");
  if (!workspace) return fail(RTPOSE_E_INVAL, "encode: NULL workspace");
  int rc = check_encode_cfg(cfg, skel, heat_channels, paf_channels);
  if (!rc) rc = check_people(N, max_people, skel);
  if (rc) return rc;
  const size_t need = rtpose_encode_workspace_bytes(cfg, skel, N, max_people);
  if (workspace_bytes < need)
    return fail(RTPOSE_E_INVAL, "encode: workspace_bytes %zu below the %zu rtpose_encode_workspace_bytes reports",
                workspace_bytes, need);
  if (N == 0) return 0;
  static thread_local CheckedPtr c_kp, c_np, c_heat, c_paf, c_ws;
  const int dev = current_device();
  rc = c_kp.check(keypoints, dev, "encode", "the keypoints");
  if (!rc && n_people) rc = c_np.check(n_people, dev, "encode", "n_people");
  if (!rc) rc = c_heat.check(heat, dev, "encode", "the heat-map tensor");
  if (!rc) rc = c_paf.check(paf, dev, "encode", "the PAF tensor");
  if (!rc) rc = c_ws.check(workspace, dev, "encode", "the workspace");
  if (rc) return rc;

  Geom g;
  g.h = cfg->input_h / cfg->stride;
  g.w = cfg->input_w / cfg->stride;
  g.stride = cfg->stride;
  g.CH = heat_channels;
  g.CP = paf_channels;
  g.P = skel->num_parts;
  g.L = skel->num_limbs;
  g.bg = cfg->background ? 1 : 0;
  g.cells = kThreads / (g.CH + g.CP);  // >= 2: at most 33 + 64 channels
  g.words = record_words(skel);
  g.max_people = max_people;
  g.sigma = cfg->sigma;
  g.start = cfg->stride / 2.0 - 0.5;
  g.input_w = (double)cfg->input_w;
  g.input_h = (double)cfg->input_h;
  ChanMap cm;
  memset(&cm, 0xff, sizeof(cm));
  for (int l = g.L - 1; l >= 0; --l)  // descending: the first limb that names a channel owns it
    for (int k = 0; k < 2; ++k) {
      cm.limb[skel->limb_paf[l][k]] = (int8_t)l;
      cm.comp[skel->limb_paf[l][k]] = (int8_t)k;
    }
  hipStream_t s = as_stream(stream);
  const int total = N * max_people * (g.P + g.L);
  if (total > 0) {
    hipLaunchKernelGGL(encode_prep_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, s, keypoints, n_people,
                       total, g, *skel, make_fastdiv(g.P + g.L), make_fastdiv(max_people),
                       static_cast<double*>(workspace));
    RTPOSE_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(encode_raster_kernel, dim3(ceil_div(g.w, g.cells), g.h, N), dim3(kThreads),
                     (size_t)kChunk * g.words * sizeof(double), s, static_cast<const double*>(workspace), n_people, g,
                     cm, make_fastdiv(g.CH + g.CP), heat, paf);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

size_t rtpose_stage_mse_partials(int N, int h, int w, int channels) {
  if (N < 1 || h < 1 || w < 1 || channels < 1) return 0;
  const long long total = (long long)N * h * w * channels;
  if (total > 0x7fffff00ll) return 0;
  return (size_t)mse_blocks(total);
}

int rtpose_stage_mse(const float* pred, const rtpose_layout* lpred, const float* target, int N, int h, int w,
                     int channels, double* partials, size_t partial_count, float* loss_out, void* stream) {
  if (!pred) return fail(RTPOSE_E_INVAL, "stage_mse: NULL pred");
  if (!lpred) return fail(RTPOSE_E_INVAL, "stage_mse: NULL lpred");
  if (!target) return fail(RTPOSE_E_INVAL, "stage_mse: NULL target");
  if (!partials) return fail(RTPOSE_E_INVAL, "stage_mse: NULL partials");
  if (!loss_out) return fail(RTPOSE_E_INVAL, "stage_mse: NULL loss_out");
  if (N < 1 || h < 1 || w < 1 || channels < 1)
    return fail(RTPOSE_E_INVAL, "stage_mse: bad sizes (N %d, h %d, w %d, channels %d)", N, h, w, channels);
  if (channels > lpred->cstride - lpred->choff)
    return fail(RTPOSE_E_INVAL, "stage_mse: channels %d but the view addresses %d (cstride %d - choff %d)", channels,
                lpred->cstride - lpred->choff, lpred->cstride, lpred->choff);
  if (w > lpred->ws || h > lpred->hs)
    return fail(RTPOSE_E_INVAL, "stage_mse: a %d x %d map in a view of %d x %d", h, w, lpred->hs, lpred->ws);
  const size_t need = rtpose_stage_mse_partials(N, h, w, channels);
  if (!need) return fail(RTPOSE_E_INVAL, "stage_mse: %d x %d x %d x %d elements above the launch limit", N, h, w, channels);
  if (partial_count < need)
    return fail(RTPOSE_E_INVAL, "stage_mse: partial_count %zu below the %zu rtpose_stage_mse_partials reports",
                partial_count, need);
  static thread_local CheckedPtr c_pred, c_tgt, c_part, c_loss;
  const int dev = current_device();
  int rc = c_pred.check(pred, dev, "stage_mse", "pred");
  if (!rc) rc = c_tgt.check(target, dev, "stage_mse", "target");
  if (!rc) rc = c_part.check(partials, dev, "stage_mse", "partials");
  if (!rc) rc = c_loss.check(loss_out, dev, "stage_mse", "loss_out");
  if (rc) return rc;
  const int total = N * h * w * channels;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(stage_mse_partial_kernel, dim3((unsigned)need), dim3(kMseThreads), 0, s, pred, to_lay(lpred), target,
                     total, h, w, channels, make_fastdiv(channels), make_fastdiv(w), make_fastdiv(h), partials);
  RTPOSE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(stage_mse_final_kernel, dim3(1), dim3(kMseThreads), 0, s, partials, (int)need, (double)total,
                     loss_out);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
