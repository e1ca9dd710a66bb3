// Flip merge (handle_paf_and_heat, evaluate/coco_eval.py:197-242) and the fused multi-scale TTA kernel, with the
// left / right permutation as data: one kernel pair for every skeleton.  The rtpose_flip_table travels by value as a
// launch argument, like rtpose_skeleton in decode.hip: nothing is uploaded, two streams may merge different skeletons
// at once.  The entry points without a table argument (rtpose_flip_merge, rtpose_tta_accumulate, at the end) call
// the launchers below with coco18_flip_table(): derived once on the host from coco18_skeleton() and the part mirror.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "decode.h"

namespace rtpose {
namespace {

constexpr int kThreads = 256;

// handle_paf_and_heat (evaluate/coco_eval.py:197-242): average a map with the x-mirrored, left/right-channel-swapped map
// of the flipped image; the PAF x components change sign.
// grid (pieces of one output row, rows, images): a thread owns one (x, channel) of the row, channels fastest over the
// heat map's and then the PAF's, so a wave's stores are two contiguous runs per pixel.  The only division left is
// x = t / (heat + PAF channels), by a launch-time constant (FastDiv: one mul-hi and a shift).
__global__ __launch_bounds__(kThreads) void flip_merge_kernel(
    const float* __restrict__ heat, const float* __restrict__ heat_f, const float* __restrict__ paf,
    const float* __restrict__ paf_f, int h, int w, float* __restrict__ heat_avg, float* __restrict__ paf_avg,
    const rtpose_flip_table tab, const FastDiv dc) {
  const int CH = tab.heat_channels, CP = tab.paf_channels;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= w * (CH + CP)) return;
  const int x = fast_div(t, dc);
  const int c = t - x * (CH + CP);
  const size_t row = (size_t)blockIdx.z * h + blockIdx.y;  // n*h + y
  const size_t p = row * w + x;
  const size_t pf = row * w + (w - 1 - x);
  if (c < CH) {
    heat_avg[p * CH + c] = (heat[p * CH + c] + heat_f[pf * CH + tab.heat_src[c]]) / 2.f;
  } else {
    const int k = c - CH;
    // coco_eval.py:237 negates the channels listed in swap_paf[::2] in place (:236 is a no-op), then :238 gathers with
    // swap_paf: output channel k reads flipped channel swap_paf[k], negated iff swap_paf[k] is one of the swap_paf[::2]
    // entries, i.e. iff it is an even channel index.  The sign therefore belongs to the OUTPUT channel and is applied
    // after the gather: bit k of paf_neg_mask (for COCO-18 exactly the k with swap_paf[k] even).
    float v = paf_f[pf * CP + tab.paf_src[k]];
    if ((tab.paf_neg_mask >> k) & 1) v = -v;
    paf_avg[p * CP + k] = (paf[p * CP + k] + v) / 2.f;
  }
}

// Fused test-time-augmentation merge for one scale (BASELINE config 3): reads the stage-6 maps of B normal passes (images
// [0,B)) and, if flip, B x-mirrored passes (images [B,2B)) where the net wrote them, forms handle_paf_and_heat's average
// (evaluate/coco_eval.py:197-242; mirror inside the first wv columns only, left/right channel swap, PAF x sign) at the
// four bilinear taps and accumulates alpha * resize(...) into the dense scale-1 maps.  Same expressions as
// flip_merge_kernel followed by image_ops.hip's resize_bilinear_accum_kernel; the grid is flip_merge_kernel's over the
// destination.
__global__ __launch_bounds__(kThreads) void tta_accumulate_kernel(
    const float* __restrict__ heat, Lay lh, const float* __restrict__ paf, Lay lp, int B, int hs, int wv,
    float* __restrict__ acc_heat, float* __restrict__ acc_paf, int hd, int wd, float sy, float sx, float alpha,
    float beta, int flip, const rtpose_flip_table tab, const FastDiv dc) {
  const int CH = tab.heat_channels, CP = tab.paf_channels;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= wd * (CH + CP)) return;
  const int x = fast_div(t, dc);
  const int cc = t - x * (CH + CP);
  const int y = blockIdx.y, b = blockIdx.z;
  const size_t p = ((size_t)b * hd + y) * wd + x;
  float fy = ((float)y + 0.5f) * sy - 0.5f, fx = ((float)x + 0.5f) * sx - 0.5f;
  fy = fmaxf(fy, 0.f);
  fx = fmaxf(fx, 0.f);
  int y0 = (int)fy, x0 = (int)fx;
  y0 = min(y0, hs - 1);
  x0 = min(x0, wv - 1);
  const int y1 = min(y0 + 1, hs - 1), x1 = min(x0 + 1, wv - 1);
  const float ly = fminf(fy - (float)y0, 1.f), lx = fminf(fx - (float)x0, 1.f);
  const bool is_heat = cc < CH;
  const int c = is_heat ? cc : cc - CH;
  const float* src = is_heat ? heat : paf;
  const Lay& l = is_heat ? lh : lp;
  const int sc = is_heat ? tab.heat_src[c] : tab.paf_src[c];
  const bool neg = !is_heat && ((tab.paf_neg_mask >> c) & 1);
  auto tap = [&](int yy, int xx) -> float {
    const float a = src[lay_off(l, b, yy, xx) + c];
    if (!flip) return a;
    float v = src[lay_off(l, B + b, yy, wv - 1 - xx) + sc];
    if (neg) v = -v;
    return (a + v) / 2.f;
  };
  const float top = tap(y0, x0) * (1.f - lx) + tap(y0, x1) * lx;
  const float bot = tap(y1, x0) * (1.f - lx) + tap(y1, x1) * lx;
  const float v = top * (1.f - ly) + bot * ly;
  float* d = is_heat ? acc_heat + p * CH + c : acc_paf + p * CP + c;
  *d = (beta == 0.f ? 0.f : beta * *d) + alpha * v;
}

int check_table(const rtpose_flip_table* t) {
  if (!t) return fail(RTPOSE_E_INVAL, "flip table: NULL argument");
  if (t->struct_bytes != sizeof(rtpose_flip_table))
    return fail(RTPOSE_E_INVAL, "flip table: struct_bytes is %u, this library's rtpose_flip_table has %zu",
                t->struct_bytes, sizeof(rtpose_flip_table));
  const int CH = t->heat_channels, CP = t->paf_channels;
  if (CH < 1 || CH > RTPOSE_FLIP_MAX_HEAT)
    return fail(RTPOSE_E_INVAL, "flip table: heat_channels %d outside [1,%d]", CH, RTPOSE_FLIP_MAX_HEAT);
  if (CP < 1 || CP > RTPOSE_FLIP_MAX_PAF)
    return fail(RTPOSE_E_INVAL, "flip table: paf_channels %d outside [1,%d]", CP, RTPOSE_FLIP_MAX_PAF);
  if (CP < 64 && (t->paf_neg_mask >> CP))
    return fail(RTPOSE_E_INVAL, "flip table: paf_neg_mask has bits at or above paf_channels %d", CP);
  for (int c = 0; c < CH; ++c) {
    const int s = t->heat_src[c];
    if (s >= CH) return fail(RTPOSE_E_INVAL, "flip table: heat channel %d reads channel %d, outside [0,%d)", c, s, CH);
    if (t->heat_src[s] != c)
      return fail(RTPOSE_E_INVAL, "flip table: heat channel %d reads %d but %d reads %d: flipping twice is not the identity",
                  c, s, s, (int)t->heat_src[s]);
  }
  for (int c = 0; c < CP; ++c) {
    const int s = t->paf_src[c];
    if (s >= CP) return fail(RTPOSE_E_INVAL, "flip table: PAF channel %d reads channel %d, outside [0,%d)", c, s, CP);
    if (t->paf_src[s] != c)
      return fail(RTPOSE_E_INVAL, "flip table: PAF channel %d reads %d but %d reads %d: flipping twice is not the identity",
                  c, s, s, (int)t->paf_src[s]);
    if (((t->paf_neg_mask >> c) & 1) != ((t->paf_neg_mask >> s) & 1))
      return fail(RTPOSE_E_INVAL, "flip table: PAF channels %d and %d read each other with different signs", c, s);
  }
  return 0;
}

// one PAF channel's (source, sign); the same channel named by two limbs must receive the same pair
int assign(rtpose_flip_table* t, bool* set, int limb, int c, int s, bool neg) {
  if (set[c] && (t->paf_src[c] != s || (bool)((t->paf_neg_mask >> c) & 1) != neg))
    return fail(RTPOSE_E_INVAL, "flip table: limb %d gives PAF channel %d the source %s%d, another limb gave it %s%d", limb,
                c, neg ? "-" : "+", s, ((t->paf_neg_mask >> c) & 1) ? "-" : "+", (int)t->paf_src[c]);
  set[c] = true;
  t->paf_src[c] = (uint8_t)s;
  if (neg) t->paf_neg_mask |= 1ull << c;
  return 0;
}

// COCO-18's table for the entry points without a table argument: derived once from the decoder's coco18_skeleton() and the
// part mirror (lib/utils/common.py:5-24: R / L shoulder, elbow, wrist, hip, knee, ankle, eye, ear change places), which
// gives coco_eval.py's swap_heat / swap_paf lists and their signs.  A derivation that failed (it cannot, short of an edit
// to one of the two tables: tests/test_skeleton_flip_cpu.py derives the same table) returns NULL with the error text
// set, and those entry points fail with it.
const rtpose_flip_table* coco18_flip_table() {
  static const rtpose_flip_table coco = [] {
    static const int32_t mirror18[RTPOSE_NUM_PART] = {0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16};
    rtpose_flip_table t;
    if (rtpose_flip_table_from_skeleton(coco18_skeleton(), mirror18, 1, 38, &t)) memset(&t, 0, sizeof(t));
    return t;
  }();
  if (coco.struct_bytes) return &coco;
  fail(RTPOSE_E_INVAL, "the library's own COCO-18 flip table could not be derived from its skeleton and part mirror");
  return nullptr;
}

// The one argument check and launch of each kernel; `who` is the entry point's name in the messages.  The 3-D grid bounds
// N / B and the rows at 65535 and a row at 0x7fffff00 threads.
int flip_merge_launch(const char* who, const float* heat, const float* heat_flipped, const float* paf,
                      const float* paf_flipped, int N, int h, int w, float* heat_avg, float* paf_avg,
                      const rtpose_flip_table* table, void* stream) {
  if (!heat || !heat_flipped || !paf || !paf_flipped || !heat_avg || !paf_avg)
    return fail(RTPOSE_E_INVAL, "%s: NULL map", who);
  const int rc = check_table(table);
  if (rc) return rc;
  if (N == 0) return 0;
  if (N < 0 || N > 65535 || h <= 0 || h > 65535 || w <= 0)
    return fail(RTPOSE_E_INVAL, "%s: bad sizes (N %d, h %d, w %d; N and h at most 65535)", who, N, h, w);
  const int ctot = table->heat_channels + table->paf_channels;
  if ((long long)w * ctot > 0x7fffff00ll)
    return fail(RTPOSE_E_INVAL, "%s: row of %d pixels too long (at most %d)", who, w, 0x7fffff00 / ctot);
  hipLaunchKernelGGL(flip_merge_kernel, dim3(ceil_div(w * ctot, kThreads), h, N), dim3(kThreads), 0, as_stream(stream),
                     heat, heat_flipped, paf, paf_flipped, h, w, heat_avg, paf_avg, *table, make_fastdiv(ctot));
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

int tta_accumulate_launch(const char* who, const float* heat, const rtpose_layout* lheat, const float* paf,
                          const rtpose_layout* lpaf, int B, int hs, int w_valid, float* acc_heat, float* acc_paf, int hd,
                          int wd, float src_h_valid, float src_w_valid, float alpha, float beta, int flip,
                          const rtpose_flip_table* table, void* stream) {
  if (!heat || !lheat || !paf || !lpaf || !acc_heat || !acc_paf) return fail(RTPOSE_E_INVAL, "%s: NULL argument", who);
  const int rc = check_table(table);
  if (rc) return rc;
  if (table->heat_channels > lheat->cstride - lheat->choff)
    return fail(RTPOSE_E_INVAL, "%s: the table has %d heat-map channels, the view addresses %d", who, table->heat_channels,
                lheat->cstride - lheat->choff);
  if (table->paf_channels > lpaf->cstride - lpaf->choff)
    return fail(RTPOSE_E_INVAL, "%s: the table has %d PAF channels, the view addresses %d", who, table->paf_channels,
                lpaf->cstride - lpaf->choff);
  if (B == 0) return 0;
  if (B < 0 || B > 65535 || hs <= 0 || hs > lheat->hs || hs > lpaf->hs || hd <= 0 || hd > 65535 || wd <= 0 ||
      !(src_h_valid > 0) || !(src_w_valid > 0))
    return fail(RTPOSE_E_INVAL, "%s: bad sizes (B %d, hs %d, hd %d, wd %d; B and hd at most 65535)", who, B, hs, hd, wd);
  if (w_valid < 1 || w_valid > lheat->ws || w_valid > lpaf->ws)
    return fail(RTPOSE_E_INVAL, "%s: w_valid %d outside [1,%d]", who, w_valid, lheat->ws < lpaf->ws ? lheat->ws : lpaf->ws);
  const int ctot = table->heat_channels + table->paf_channels;
  if ((long long)wd * ctot > 0x7fffff00ll)
    return fail(RTPOSE_E_INVAL, "%s: row of %d pixels too long (at most %d)", who, wd, 0x7fffff00 / ctot);
  hipLaunchKernelGGL(tta_accumulate_kernel, dim3(ceil_div(wd * ctot, kThreads), hd, B), dim3(kThreads), 0,
                     as_stream(stream), heat, to_lay(lheat), paf, to_lay(lpaf), B, hs, w_valid, acc_heat, acc_paf, hd, wd,
                     src_h_valid / (float)hd, src_w_valid / (float)wd, alpha, beta, flip ? 1 : 0, *table,
                     make_fastdiv(ctot));
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace rtpose

using namespace rtpose;

extern "C" {

int rtpose_flip_table_check(const rtpose_flip_table* table) { return check_table(table); }

int rtpose_flip_table_from_skeleton(const rtpose_skeleton* skel, const int32_t* part_mirror, int background,
                                    int paf_channels, rtpose_flip_table* out) {
  if (!skel || !part_mirror || !out) return fail(RTPOSE_E_INVAL, "flip table: NULL argument");
  if (paf_channels < 1 || paf_channels > RTPOSE_FLIP_MAX_PAF)
    return fail(RTPOSE_E_INVAL, "flip table: paf_channels %d outside [1,%d]", paf_channels, RTPOSE_FLIP_MAX_PAF);
  const int bg = background ? 1 : 0;
  int rc = rtpose_skeleton_check(skel, skel->num_parts + bg, paf_channels);
  if (rc) return rc;
  const int P = skel->num_parts, L = skel->num_limbs;
  for (int i = 0; i < P; ++i) {
    const int m = part_mirror[i];
    if (m < 0 || m >= P) return fail(RTPOSE_E_INVAL, "flip table: part %d mirrors to %d, outside [0,%d)", i, m, P);
    if (part_mirror[m] != i)
      return fail(RTPOSE_E_INVAL, "flip table: part %d mirrors to %d but %d mirrors to %d: the mirror is not an involution",
                  i, m, m, part_mirror[m]);
  }
  rtpose_flip_table t;
  memset(&t, 0, sizeof(t));
  t.struct_bytes = (uint32_t)sizeof(t);
  t.heat_channels = P + bg;
  t.paf_channels = paf_channels;
  for (int i = 0; i < P; ++i) t.heat_src[i] = (uint8_t)part_mirror[i];
  if (bg) t.heat_src[P] = (uint8_t)P;
  bool set[RTPOSE_FLIP_MAX_PAF] = {false};
  for (int l = 0; l < L; ++l) {
    const int ma = part_mirror[skel->limb_part[l][0]], mb = part_mirror[skel->limb_part[l][1]];
    const int cx = skel->limb_paf[l][0], cy = skel->limb_paf[l][1];
    int same = -1, rev = -1;
    for (int k = 0; k < L; ++k) {
      if (skel->limb_part[k][0] == ma && skel->limb_part[k][1] == mb) same = k;
      if (skel->limb_part[k][0] == mb && skel->limb_part[k][1] == ma) rev = k;
    }
    // the mirrored field is (-x, y); read along a limb walked the other way it is (x, -y)
    const int k = same >= 0 ? same : rev;
    if (k < 0)
      return fail(RTPOSE_E_INVAL, "flip table: limb %d (parts %d -> %d) has no mirror: no limb joins parts %d and %d", l,
                  skel->limb_part[l][0], skel->limb_part[l][1], ma, mb);
    const bool reversed = same < 0;
    rc = assign(&t, set, l, cx, skel->limb_paf[k][0], !reversed);
    if (!rc) rc = assign(&t, set, l, cy, skel->limb_paf[k][1], reversed);
    if (rc) return rc;
  }
  for (int c = 0; c < paf_channels; ++c)
    if (!set[c]) t.paf_src[c] = (uint8_t)c;  // a channel no limb reads: itself, sign +
  rc = check_table(&t);
  if (rc) return rc;
  *out = t;
  return 0;
}

int rtpose_flip_merge_skel(const float* heat, const float* heat_flipped, const float* paf, const float* paf_flipped,
                           int N, int h, int w, float* heat_avg, float* paf_avg, const rtpose_flip_table* table,
                           void* stream) {
  return flip_merge_launch("flip_merge_skel", heat, heat_flipped, paf, paf_flipped, N, h, w, heat_avg, paf_avg, table,
                           stream);
}

int rtpose_tta_accumulate_skel(const float* heat, const rtpose_layout* lheat, const float* paf,
                               const rtpose_layout* lpaf, int B, int hs, int w_valid, float* acc_heat, float* acc_paf,
                               int hd, int wd, float src_h_valid, float src_w_valid, float alpha, float beta, int flip,
                               const rtpose_flip_table* table, void* stream) {
  return tta_accumulate_launch("tta_accumulate_skel", heat, lheat, paf, lpaf, B, hs, w_valid, acc_heat, acc_paf, hd, wd,
                               src_h_valid, src_w_valid, alpha, beta, flip, table, stream);
}

// COCO-18's flip merge and fused TTA merge: the same kernels and argument check over the table the library derives for
// itself.  As before, a flip merge without pixels (h or w 0 as well as N 0) is a no-op ...
int rtpose_flip_merge(const float* heat, const float* heat_flipped, const float* paf, const float* paf_flipped, int N,
                      int h, int w, float* heat_avg, float* paf_avg, void* stream) {
  if (N == 0 || h == 0 || w == 0) return 0;
  const rtpose_flip_table* t = coco18_flip_table();
  return !t ? RTPOSE_E_INVAL
            : flip_merge_launch("flip_merge", heat, heat_flipped, paf, paf_flipped, N, h, w, heat_avg, paf_avg, t, stream);
}

// ... and unlike rtpose_tta_accumulate_skel, this door refuses the empty batch
int rtpose_tta_accumulate(const float* heat, const rtpose_layout* lheat, const float* paf, const rtpose_layout* lpaf,
                          int B, int hs, int w_valid, float* acc_heat, float* acc_paf, int hd, int wd, float src_h_valid,
                          float src_w_valid, float alpha, float beta, int flip, void* stream) {
  if (B == 0) return fail(RTPOSE_E_INVAL, "tta_accumulate: B is 0");
  const rtpose_flip_table* t = coco18_flip_table();
  return !t ? RTPOSE_E_INVAL
            : tta_accumulate_launch("tta_accumulate", heat, lheat, paf, lpaf, B, hs, w_valid, acc_heat, acc_paf, hd, wd,
                                    src_h_valid, src_w_valid, alpha, beta, flip, t, stream);
}

}  // extern "C"
