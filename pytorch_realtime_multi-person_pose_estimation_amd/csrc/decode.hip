// Batched pose decoding on the GPU — replaces the numpy/scipy/cv2 control flow
// of lib/utils/paf_to_pose.py (NMS :67-145, find_peaks :25-38) and the serial
// C++ of lib/pafprocess/pafprocess.cpp (process_paf :22-194) with three
// wavefront-level kernels, one launch each for a whole batch of images:
//
//   nms_refine_kernel      grid (P parts, N)    peak test + ordered compaction +
//                                               8x bicubic patch refine/arg-max
//   limb_assign_kernel     grid (L limbs, N)    10-sample PAF line integral for
//                                               every (a,b) pair + greedy 1:1
//   group_kernel           grid (N)             subset merge + prune (one wave)
//
// Integer outputs (peak coordinates, ids, part->peak assignments) are bit-exact
// to the reference; float scores reproduce its operation order (this file is
// compiled with -ffp-contract=off; hipcc's default correctly rounded fp32
// divide/sqrt is relied upon).  All HBM reads are of the low-resolution maps:
// the x8 nearest-neighbour up-sampling of paf_to_pose.py:382-385 is an index
// computation (floor(x * 1/8)), never materialised.
//
// The skeleton is DATA - the part count P, the limbs as (part A, part B, PAF x channel, PAF y channel) and the limbs that
// may start a person (rtpose_skeleton, header section 4a) - and there is one set of kernels for every skeleton:
//
//   * the skeleton travels BY VALUE as a kernel argument (528 bytes of the kernarg segment, read with scalar loads at an
//     index that is uniform per block).  It is not uploaded to a __constant__ symbol: that would make a launch depend on
//     what another stream uploaded last, and the decoder runs on a side stream beside the next forward;
//   * the record is laid out by decode.h's size functions (peaks at word max(32, round_up(8 + P, 4)), subset rows of
//     P + 3 floats, conn lists and the score / tie sections of L limbs), and every fit decision of the launcher is taken on
//     those byte counts.
//
// rtpose_decode_batch[_ex] / rtpose_nms_batch[_ex] and the legacy process_paf are doors onto the same kernels with the
// COCO-18 tables of pafprocess.h:16-24 (coco18_skeleton()); the `_skel` entry points take the caller's.  The line
// references in the comments below are into the reference's COCO-18 code: what they say of "18 parts" holds for P.
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.h"
#include "decode.h"
#include "decode_dev.h"

namespace rtpose {

// ------------------------------------------------------------------------------
// 1. NMS + refine
// ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nms_refine_kernel(MapView heat, int h, int w, int up, double inv_up, float thr,
                                                         int pcap, int32_t* __restrict__ result, int result_words,
                                                         int peaks_word) {
  const int part = blockIdx.x, n = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* res = result + (size_t)n * result_words;

  __shared__ int s_sx[kMaxDst];
  __shared__ float s_alpha[kMaxDst][4];
  __shared__ int s_wcount[kPeakBatch][4];
  __shared__ int s_px[kDecodeMaxPeaks], s_py[kDecodeMaxPeaks];
  __shared__ float s_patch[4][25];
  __shared__ float s_hbuf[4][5 * kMaxDst];

  // per-destination-index source offset and cubic weights (cv2.resize INTER_CUBIC:
  // fx = (float)((dx+0.5)*scale - 0.5); sx = floor(fx); fx -= sx)
  if (tid < 5 * up) {
    // (double)(tid + 0.5) * inv_up - 0.5 rounded to float: exact in fp32 when up is a power of two (no double-precision
    // instruction then: see limb_assign_kernel)
    float fx = (up & (up - 1)) == 0 ? ((float)tid + 0.5f) * (float)inv_up - 0.5f
                                    : (float)(((double)tid + 0.5) * inv_up - 0.5);
    const int sx = (int)floorf(fx);
    fx -= (float)sx;
    float c[4];
    cubic_coeffs(fx, c);
    s_sx[tid] = sx;
    s_alpha[tid][0] = c[0];
    s_alpha[tid][1] = c[1];
    s_alpha[tid][2] = c[2];
    s_alpha[tid][3] = c[3];
  }

  const int count = find_peaks_block(heat, n, part, h, w, thr, pcap, s_wcount, s_px, s_py, res);

  // ---- refine (paf_to_pose.py:106-142): one wave per peak
  rtpose_peak* peaks = reinterpret_cast<rtpose_peak*>(res + peaks_word) + (size_t)part * pcap;
  for (int i = wave; i < count; i += 4) {
    const int px = s_px[i], py = s_py[i];
    const int x_min = max(0, px - 2), y_min = max(0, py - 2);
    const int x_max = min(w - 1, px + 2), y_max = min(h - 1, py + 2);
    const int pw = x_max - x_min + 1, ph = y_max - y_min + 1;
    const int dw = pw * up, dh = ph * up;
    if (lane < pw * ph) {
      const int r = lane / pw, c = lane - r * pw;
      s_patch[wave][lane] = map_at(heat, n, y_min + r, x_min + c, part);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // horizontal pass: hbuf[r][dx] = sum_j patch[r][clamp(sx-1+j)] * alpha[dx][j]
    for (int e = lane; e < ph * dw; e += 64) {
      const int r = e / dw, dx = e - r * dw;
      const int sx = s_sx[dx];
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sxj = min(max(sx - 1 + j, 0), pw - 1);
        v = v + s_patch[wave][r * pw + sxj] * s_alpha[dx][j];
      }
      s_hbuf[wave][r * dw + dx] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // vertical pass + running arg-max (first maximum in row-major order)
    float best = -INFINITY;
    int best_idx = 0x7fffffff;
    for (int e = lane; e < dh * dw; e += 64) {
      const int dy = e / dw, dx = e - dy * dw;
      const int sy = s_sx[dy];
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int syj = min(max(sy - 1 + j, 0), ph - 1);
        const float t = s_hbuf[wave][syj * dw + dx] * s_alpha[dy][j];
        v = (j == 0) ? t : v + t;
      }
      if (v > best) {
        best = v;
        best_idx = e;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(best_idx, o);
      if (ob > best || (ob == best && oi < best_idx)) {
        best = ob;
        best_idx = oi;
      }
    }
    if (lane == 0) {
      const int dy = best_idx / dw, dx = best_idx - dy * dw;
      rtpose_peak p;
      p.x = x_min * up + dx;  // paf_to_pose.py:129-141 collapses to this
      p.y = y_min * up + dy;
      p.score = best;
      p.id = i;  // rebased to the running counter by the prefix / grouping kernel
      peaks[i] = p;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// The two optional branches of NMS (paf_to_pose.py:67): bool_gaussian_filt=True smooths the
// up-sampled patch with scipy.ndimage.gaussian_filter(sigma=3) before the arg-max (:121-122);
// bool_refine_center=False skips the patch altogether (:135-139).  Neither is used by the
// reference's callers, so this kernel favours clarity: the whole block works on one peak at a time.
// gaussian_filter = correlate1d along axis 0 (rows), then axis 1, mode 'reflect', each pass
// accumulated in double in scipy's symmetric-kernel order and stored as float32
// (ndimage/src/ni_filters.c NI_Correlate1D).
__global__ __launch_bounds__(256) void nms_refine_opt_kernel(MapView heat, int h, int w, int up, double inv_up, float thr,
                                                             int pcap, int32_t* __restrict__ result, int result_words,
                                                             int flags, GaussW gw, int peaks_word) {
  const int part = blockIdx.x, n = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* res = result + (size_t)n * result_words;
  extern __shared__ float s_dyn[];  // [2][(5 up)^2]: the up-sampled patch and the first Gaussian pass
  __shared__ int s_sx[kMaxDst];
  __shared__ float s_alpha[kMaxDst][4];
  __shared__ int s_wcount[kPeakBatch][4];
  __shared__ int s_px[kDecodeMaxPeaks], s_py[kDecodeMaxPeaks];
  __shared__ float s_patch[25];
  __shared__ float s_hbuf[5 * kMaxDst];
  __shared__ float s_best[4];
  __shared__ int s_besti[4];
  float* s_up = s_dyn;
  float* s_tmp = s_dyn + 25 * up * up;

  if (tid < 5 * up) {
    // (double)(tid + 0.5) * inv_up - 0.5 rounded to float: exact in fp32 when up is a power of two (no double-precision
    // instruction then: see limb_assign_kernel)
    float fx = (up & (up - 1)) == 0 ? ((float)tid + 0.5f) * (float)inv_up - 0.5f
                                    : (float)(((double)tid + 0.5) * inv_up - 0.5);
    const int sx = (int)floorf(fx);
    fx -= (float)sx;
    float c[4];
    cubic_coeffs(fx, c);
    s_sx[tid] = sx;
    s_alpha[tid][0] = c[0];
    s_alpha[tid][1] = c[1];
    s_alpha[tid][2] = c[2];
    s_alpha[tid][3] = c[3];
  }
  const int count = find_peaks_block(heat, n, part, h, w, thr, pcap, s_wcount, s_px, s_py, res);
  rtpose_peak* peaks = reinterpret_cast<rtpose_peak*>(res + peaks_word) + (size_t)part * pcap;

  if (flags & RTPOSE_NMS_NO_REFINE) {
    // :135-139 + compute_resized_coords (:41-64): the peak's cell centre (c + 0.5) * up - 0.5 in
    // float64, score = the low-res map value.  Stored truncated (what process_paf's (int) cast of
    // the joint_list column makes of it, pafprocess.cpp:28-29); NMS() on the host re-derives the float.
    for (int i = tid; i < count; i += 256) {
      rtpose_peak p;
      p.x = (int)(((double)s_px[i] + 0.5) * (double)up - 0.5);
      p.y = (int)(((double)s_py[i] + 0.5) * (double)up - 0.5);
      p.score = map_at(heat, n, s_py[i], s_px[i], part);
      p.id = i;
      peaks[i] = p;
    }
    return;
  }

  for (int i = 0; i < count; ++i) {
    const int px = s_px[i], py = s_py[i];
    const int x_min = max(0, px - 2), y_min = max(0, py - 2);
    const int x_max = min(w - 1, px + 2), y_max = min(h - 1, py + 2);
    const int pw = x_max - x_min + 1, ph = y_max - y_min + 1;
    const int dw = pw * up, dh = ph * up;
    if (tid < pw * ph) {
      const int r = tid / pw, c = tid - r * pw;
      s_patch[tid] = map_at(heat, n, y_min + r, x_min + c, part);
    }
    __syncthreads();
    for (int e = tid; e < ph * dw; e += 256) {  // cv2.resize INTER_CUBIC, horizontal pass
      const int r = e / dw, dx = e - r * dw;
      const int sx = s_sx[dx];
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sxj = min(max(sx - 1 + j, 0), pw - 1);
        v = v + s_patch[r * pw + sxj] * s_alpha[dx][j];
      }
      s_hbuf[r * dw + dx] = v;
    }
    __syncthreads();
    for (int e = tid; e < dh * dw; e += 256) {  // vertical pass (same expression order as nms_refine_kernel)
      const int dy = e / dw, dx = e - dy * dw;
      const int sy = s_sx[dy];
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int syj = min(max(sy - 1 + j, 0), ph - 1);
        const float t = s_hbuf[syj * dw + dx] * s_alpha[dy][j];
        v = (j == 0) ? t : v + t;
      }
      s_up[e] = v;
    }
    __syncthreads();
    if (flags & RTPOSE_NMS_GAUSSIAN) {
      const double* wc = gw.w + kGaussR;
      for (int e = tid; e < dh * dw; e += 256) {  // axis 0
        const int y = e / dw, x = e - y * dw;
        double acc = (double)s_up[e] * wc[0];
        for (int j = -kGaussR; j < 0; ++j)
          acc += ((double)s_up[reflect_idx(y + j, dh) * dw + x] + (double)s_up[reflect_idx(y - j, dh) * dw + x]) * wc[j];
        s_tmp[e] = (float)acc;
      }
      __syncthreads();
      for (int e = tid; e < dh * dw; e += 256) {  // axis 1
        const int y = e / dw, x = e - y * dw;
        double acc = (double)s_tmp[e] * wc[0];
        for (int j = -kGaussR; j < 0; ++j)
          acc += ((double)s_tmp[y * dw + reflect_idx(x + j, dw)] + (double)s_tmp[y * dw + reflect_idx(x - j, dw)]) * wc[j];
        s_up[e] = (float)acc;
      }
      __syncthreads();
    }
    float best = -INFINITY;  // first maximum in row-major order (:125-126)
    int best_idx = 0x7fffffff;
    for (int e = tid; e < dh * dw; e += 256) {
      const float v = s_up[e];
      if (v > best) {
        best = v;
        best_idx = e;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(best_idx, o);
      if (ob > best || (ob == best && oi < best_idx)) {
        best = ob;
        best_idx = oi;
      }
    }
    if (lane == 0) {
      s_best[wave] = best;
      s_besti[wave] = best_idx;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < 4; ++k)
        if (s_best[k] > best || (s_best[k] == best && s_besti[k] < best_idx)) {
          best = s_best[k];
          best_idx = s_besti[k];
        }
      const int dy = best_idx / dw, dx = best_idx - dy * dw;
      rtpose_peak p;
      p.x = x_min * up + dx;
      p.y = y_min * up + dy;
      p.score = best;
      p.id = i;
      peaks[i] = p;
    }
    __syncthreads();
  }
}

// ids = running counter over parts then peaks (paf_to_pose.py:141-142); also
// totals in the header.  One wave per image.  (NMS only: a full decode leaves both to group_kernel<true, ...>.)
__global__ void peak_prefix_kernel(int pcap, int32_t* __restrict__ result, int result_words, int nparts, int P,
                                   int peaks_word) {
  const int n = blockIdx.x, lane = threadIdx.x;
  int32_t* res = result + (size_t)n * result_words;
  __shared__ int s_start[RTPOSE_SKEL_MAX_PARTS + 1];
  if (lane == 0) {
    int acc = 0;
    for (int p = 0; p < P; ++p) {
      s_start[p] = acc;
      acc += (p < nparts) ? res[kResPartCount + p] : 0;
    }
    s_start[P] = acc;
    res[kResHeader + 0] = acc;
  }
  __syncthreads();
  rtpose_peak* peaks = reinterpret_cast<rtpose_peak*>(res + peaks_word);
  for (int p = 0; p < nparts; ++p) {
    const int cnt = res[kResPartCount + p];
    for (int i = lane; i < cnt; i += 64) peaks[(size_t)p * pcap + i].id = s_start[p] + i;
  }
}

// ------------------------------------------------------------------------------
// 2. PAF scoring + greedy assignment (pafprocess.cpp:46-124, :220-246): grid (L limbs, N);
//    the limb's parts and PAF channels come from `sk`
// ------------------------------------------------------------------------------

// Round 5: (a) SCORES_IN_LDS is a template parameter - the score matrix is addressed with LDS instructions (or global
// ones), not through a generic pointer (flat_load / flat_store, the aperture decided per access); (b) NO double-precision
// instruction in the per-sample loop: the reference's (int)(v + 0.5) on a double and floor(l / up) are computed exactly
// in integers / fp32 (v >= 0 and up a power of two, the only case the configs use; any other `up` keeps the doubles),
// and the length penalty needs its double division only for limbs longer than half the image.
// Round 6: (c) A32 - a sample's two map values through the SGPR-base form of global_load_dword with one 32-bit byte offset
// (two 24-bit multiplies): no 64-bit integer VALU instruction between the peak loads and the last map load; (d) this file is
// compiled WITHOUT clang's vectorisers (csrc/Makefile).  With the decoder on a second stream beside the bf16 forward's first
// launches (pipeline.SideDecoder), the vectorised build of this loop - v_pk_mul_f32 (vx, vy) x (px, py) on the loaded map
// values and op_sel-swizzled v_pk_add_f32 behind them - returned, in ~1 of 150 launches, ONE candidate score computed from a
// wrong sample, always in lanes 48..63 (most often the top active lane), with maps and peaks bit-identical before and after,
// never in the serial flow, never on CUs the forward does not use.  Eight discriminating builds and three stand-alone
// victims: DESIGN.md 3.3, profiles/r06_decoder_beside_forward.txt.  (a) - (c) were each tried as the cure and are not it
// (they stay: fewer instructions); (d) is.
template <bool SCORES_IN_LDS, bool UP_POW2, bool A32>
__global__ __launch_bounds__(256) void limb_assign_kernel(rtpose_skeleton sk, int peaks_word, MapView paf, int h, int w,
                                                          double inv_up, int up_shift, int h1, int pcap,
                                                          const int32_t* __restrict__ result, int result_words,
                                                          int32_t* __restrict__ conn, int conn_words,
                                                          float* __restrict__ score_ws,
                                                          unsigned long long* __restrict__ tie_ws) {
  const int pair_id = blockIdx.x, n = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* res = result + (size_t)n * result_words;
  int32_t* cn = conn + (size_t)n * conn_words + (size_t)pair_id * (1 + 3 * pcap);

  extern __shared__ __attribute__((aligned(16))) float s_score_lds[];  // [pcap * pcap] candidate scores, 0 = none (when they fit), then the tie list
  __shared__ unsigned char s_usedA[kDecodeMaxPeaks], s_usedB[kDecodeMaxPeaks];
  __shared__ float s_wbest[4];
  __shared__ int s_widx[4], s_wcnt[4];
  __shared__ int s_nconn;
  __shared__ int s_stack[kSortStack];
  // the limb's connections (a, b, score bits) as they are accepted; written to the workspace in one parallel sweep at the end
  // (round 6: thread 0 stored each one to global memory inside the greedy loop, and the store had to land before the loop's
  // barrier let the next step start - a global round trip per connection)
  __shared__ int s_conn[3 * kDecodeMaxPeaks];

  const int partA = sk.limb_part[pair_id][0], partB = sk.limb_part[pair_id][1];
  const int chx = sk.limb_paf[pair_id][0], chy = sk.limb_paf[pair_id][1];
  const int nA = res[kResPartCount + partA], nB = res[kResPartCount + partB];
  if (tid == 0) s_nconn = 0;
  if (nA == 0 || nB == 0) {
    if (tid == 0) cn[0] = 0;
    return;
  }
  const rtpose_peak* pA = reinterpret_cast<const rtpose_peak*>(res + peaks_word) + (size_t)partA * pcap;
  const rtpose_peak* pB = reinterpret_cast<const rtpose_peak*>(res + peaks_word) + (size_t)partB * pcap;
  for (int i = tid; i < kDecodeMaxPeaks; i += 256) {
    s_usedA[i] = 0;
    s_usedB[i] = 0;
  }

  const int npairs = nA * nB;
  // A32: the image's two PAF channel planes as wave-uniform bases (SGPR pairs) + ONE 32-bit byte offset per sample
  // (global_load_dword v, v_off, s[base:base+1]); the host picks it when every offset of an image fits 31 bits.  The y
  // plane may lie below the x plane (a skeleton names its channels freely): the difference is signed
  const char* const img_x =
      reinterpret_cast<const char*>(paf.base + ((size_t)paf.lead + (size_t)n * paf.hs * paf.ws) * paf.cstride + paf.choff + chx);
  const char* const img_y = img_x + (ptrdiff_t)(chy - chx) * (ptrdiff_t)sizeof(float);
  const unsigned pix_bytes = (unsigned)paf.cstride * (unsigned)sizeof(float);
  // the score matrix lives in LDS unless the tables were grown past what LDS holds
  // (junk maps with hundreds of peaks per part): then in the global workspace
  float* const score_g = score_ws + ((size_t)n * sk.num_limbs + pair_id) * pcap * pcap;
  auto s_score = [&](int p) -> float& {
    if constexpr (SCORES_IN_LDS)
      return s_score_lds[p];
    else
      return score_g[p];
  };
  for (int p = tid; p < npairs; p += 256) {
    const int a = p / nB, b = p - a * nB;
    const rtpose_peak A = pA[a], B = pB[b];
    float cand = 0.f;
    float vx = (float)(B.x - A.x), vy = (float)(B.y - A.y);
    const float norm = sqrtf(vx * vx + vy * vy);
    if (norm > 0.f) {  // (double)norm < 1e-12 of the reference: norm is the root of a sum of integer squares, 0 or >= 1
      vx = vx / norm;
      vy = vy / norm;
      const float step_x = (float)(B.x - A.x) / 10.f;
      const float step_y = (float)(B.y - A.y) / 10.f;
      float scores = 0.f;
      int crit1 = 0;
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        // lx = (int)(v + 0.5) evaluated in double (pafprocess.cpp:232-233): v >= 0 is a float, so v + 0.5 is exact there
        // and the cast is floor(v + 0.5) = trunc(v) + (frac(v) >= 0.5), frac exact in fp32
        const float fx = (float)A.x + (float)i * step_x, fy = (float)A.y + (float)i * step_y;
        int lx = (int)fx, ly = (int)fy;
        if (fx - (float)lx >= 0.5f) ++lx;
        if (fy - (float)ly >= 0.5f) ++ly;
        // nearest x8 up-sampling of the PAF as an index map (paf_to_pose.py:382): floor(l / up)
        int sx, sy;
        if constexpr (UP_POW2) {
          sx = lx >> up_shift;
          sy = ly >> up_shift;
        } else {
          sx = (int)floor((double)lx * inv_up);
          sy = (int)floor((double)ly * inv_up);
        }
        sx = min(max(sx, 0), w - 1);
        sy = min(max(sy, 0), h - 1);
        float px, py;
        if constexpr (A32) {
          // two full-rate 24-bit multiplies, spelled out: the compiler turns __umul24 into v_mad_u64_u32 + v_mul_lo_u32
          unsigned pix, boff;
          asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(pix) : "v"(sy), "s"(paf.ws), "v"(sx));
          asm("v_mul_u32_u24 %0, %1, %2" : "=v"(boff) : "s"(pix_bytes), "v"(pix));
          px = *reinterpret_cast<const float*>(img_x + boff);
          py = *reinterpret_cast<const float*>(img_y + boff);
        } else {
          px = map_at(paf, n, sy, sx, chx);
          py = map_at(paf, n, sy, sx, chy);
        }
        const float s = vx * px + vy * py;
        scores = scores + s;
        if (s > 0.05f) ++crit1;
      }
      // min(0.5 h1 / norm - 1, 0) in double (cpp:238-240): 0 for every limb no longer than half the image (the quotient is
      // >= 1 then, and adding 0.0 to a float widened to double changes nothing)
      float crit2 = scores / 10.f;
      if (2.f * norm > (float)h1) {
        const double pen = fmin(0.0, 0.5 * (double)h1 / (double)norm - 1.0);
        crit2 = (float)((double)crit2 + pen);
      }
      if (crit1 > 6 && crit2 > 0.f) cand = crit2;
    }
    s_score(p) = cand;
  }
  __threadfence_block();
  __syncthreads();

  // greedy: repeatedly take the best remaining candidate whose endpoints are
  // both free == scanning the list sorted by descending score (cpp:96-124).
  // That equivalence needs the best free candidate to be UNIQUE at every step: when two free
  // candidates share the best score, std::sort's moves decide which the reference meets first
  // (and, if they do not exclude each other, the order of their connections, which orders the
  // subset rows).  Every step therefore also counts the free candidates AT the best score; a
  // count above one sends the limb to the replay below.  (Equal scores of which at most one is
  // still free when their turn comes cannot change anything: a used peak stays used.)
  const int max_conn = min(nA, nB);
  bool tie = false;
  for (int it = 0; it < max_conn; ++it) {
    float best = 0.f;
    int bidx = 0x7fffffff, cnt = 0;
    for (int p = tid; p < npairs; p += 256) {
      const float s = s_score(p);
      if (s >= best && s > 0.f) {
        const int a = p / nB, b = p - a * nB;
        if (!s_usedA[a] && !s_usedB[b]) {
          if (s > best) {
            best = s;
            bidx = p;
            cnt = 1;
          } else {
            ++cnt;  // p ascends: bidx stays the lowest
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bidx, o);
      const int oc = __shfl_xor(cnt, o);
      if (ob > best) {
        best = ob;
        bidx = oi;
        cnt = oc;
      } else if (ob == best) {
        bidx = min(bidx, oi);
        cnt += oc;
      }
    }
    if (lane == 0) {
      s_wbest[wave] = best;
      s_widx[wave] = bidx;
      s_wcnt[wave] = cnt;
    }
    __syncthreads();
    best = s_wbest[0];
    bidx = s_widx[0];
    cnt = s_wcnt[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (s_wbest[k] > best) {
        best = s_wbest[k];
        bidx = s_widx[k];
        cnt = s_wcnt[k];
      } else if (s_wbest[k] == best) {
        bidx = min(bidx, s_widx[k]);
        cnt += s_wcnt[k];
      }
    }
    if (!(best > 0.f)) break;  // uniform
    if (cnt > 1) {             // uniform
      tie = true;
      break;
    }
    if (tid == 0) {
      const int a = bidx / nB, b = bidx - a * nB;
      s_usedA[a] = 1;
      s_usedB[b] = 1;
      const int k = s_nconn++;
      s_conn[3 * k + 0] = a;
      s_conn[3 * k + 1] = b;
      s_conn[3 * k + 2] = __float_as_int(best);
    }
    __syncthreads();
  }
  __syncthreads();
  if (tie) {
    // the reference's own sequence for this limb, from the start: candidates in push order
    // (a ascending, b ascending, cpp:56-94), libstdc++'s std::sort, scan (cpp:98-123)
    for (int i = tid; i < kDecodeMaxPeaks; i += 256) {
      s_usedA[i] = 0;
      s_usedB[i] = 0;
    }
    __syncthreads();
    // candidates in push order: ordered compaction by ballot / popcount, like the peak ids
    unsigned long long* lds_list =
        reinterpret_cast<unsigned long long*>(s_score_lds + (SCORES_IN_LDS ? ((pcap * pcap + 1) & ~1) : 0));
    unsigned long long* ws_list = tie_ws + ((size_t)n * sk.num_limbs + pair_id) * pcap * pcap;
    for (int pass = 0; pass < 2; ++pass) {  // pass 0 counts (LDS or workspace?), pass 1 writes
      unsigned long long* list = (s_nconn <= kTieLdsCands) ? lds_list : ws_list;  // (s_nconn = the count after pass 0)
      int base = 0;
      for (int start = 0; start < npairs; start += 256) {
        const int p = start + tid;
        const float sc = p < npairs ? s_score(p) : 0.f;
        const bool c = sc > 0.f;
        const unsigned long long mask = __ballot(c);
        if (lane == 0) s_wcnt[wave] = __popcll(mask);
        __syncthreads();
        int off = base;
        for (int k = 0; k < wave; ++k) off += s_wcnt[k];
        if (c && pass == 1)
          list[off + __popcll(mask & ((1ull << lane) - 1ull))] =
              ((unsigned long long)__float_as_uint(sc) << 32) | (unsigned)p;
        base += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
      }
      if (tid == 0) s_nconn = base;
      __syncthreads();
    }
    __threadfence_block();
    if (tid == 0) {
      const int nc = s_nconn;
      unsigned long long* list = (nc <= kTieLdsCands) ? lds_list : ws_list;
      SortReplay sr{list, s_stack};
      sr.sort_desc(nc);
      int k = 0;
      for (int c = 0; c < nc && k < max_conn; ++c) {
        const unsigned long long e = list[c];
        const int p = (int)(unsigned)e;
        const int a = p / nB, b = p - a * nB;
        if (s_usedA[a] || s_usedB[b]) continue;
        s_usedA[a] = 1;
        s_usedB[b] = 1;
        s_conn[3 * k + 0] = a;
        s_conn[3 * k + 1] = b;
        s_conn[3 * k + 2] = (int)(unsigned)(e >> 32);
        ++k;
      }
      s_nconn = k;
    }
    __syncthreads();
  }
  __syncthreads();
  const int nconn = s_nconn;
  if (tid == 0) cn[0] = nconn;
  for (int i = tid; i < 3 * nconn; i += 256) cn[1 + i] = s_conn[i];
}


// ------------------------------------------------------------------------------
// 3. Person grouping + prune (pafprocess.cpp:126-191), one wave per image
// ------------------------------------------------------------------------------
// A subset row (the reference's `subset` entry, 18 + 2 floats there) is P + 3 floats: [0, P) the parts' cids, [P] the score
// sum, [P + 1] the part count, [P + 2] alive; lanes below P (P <= 32) work on a row.  A limb may start a person when its bit
// of sk.seed_mask is set (COCO-18: the first 18 of the 19 limbs, the `pair_id < 18` of cpp:173).
// The walk over the connections is the reference's serial loop (every connection sees the rows the previous one left), so
// what it costs is the latency of one step.  Round 6: a limb's connections are STAGED first - the 64 lanes fetch the
// (a, b, score) triples, the two peak ids and the two peak scores of up to 64 connections at a time into LDS, in parallel - and
// the serial walk then touches LDS only (round 5: three dependent global loads per connection, ~1.6 us each step: 164 us per
// batch whatever its size; now ~20).  WRITE_IDS: the running peak ids of paf_to_pose.py:141-142 (the former peak_prefix_kernel
// launch) are written here - and taken arithmetically, id = s_start[part] + index, instead of read back; false for the legacy
// process_paf, whose peak tables carry the ids of the caller's joint list.
// STAGE_ALL: the connections of ALL L limbs are staged in one sweep over the flattened (limb, connection) list - every
// global round trip of the kernel is then taken once, with all lanes' loads in flight together, instead of once per limb (the
// host picks it when the L * pcap staged connections and the LDS-resident rows fit 96 KiB together: for COCO-18 up to pcap 230
// with 128 rows in LDS, up to 258 with the rows in the workspace).
// ROWS_IN_LDS: the rows are addressed with LDS instructions or global ones, decided by the host on their byte count
// (decode_rows_in_lds) - a template parameter for the reason SCORES_IN_LDS is one.
template <bool WRITE_IDS, bool STAGE_ALL, bool ROWS_IN_LDS>
__global__ __launch_bounds__(64) void group_kernel(rtpose_skeleton sk, int peaks_word, int pcap, int hcap,
                                                   int32_t* __restrict__ result, int result_words,
                                                   const int32_t* __restrict__ conn, int conn_words, int row_cap,
                                                   float* __restrict__ rows_ws) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int P = sk.num_parts, L = sk.num_limbs;
  const int RW = P + 3, kSum = P, kCnt = P + 1, kAlive = P + 2;
  int32_t* res = result + (size_t)n * result_words;
  const int32_t* cnb = conn + (size_t)n * conn_words;
  extern __shared__ float rows_lds[];
  // [row_cap][P + 2 + alive]: the reference's `subset`; LDS unless grown past kLdsRowBytes; then the staged connections (of
  // one limb, or of all)
  float* rows = ROWS_IN_LDS ? rows_lds : rows_ws + (size_t)n * row_cap * RW;
  float* stage = rows_lds + (ROWS_IN_LDS ? (size_t)row_cap * RW : 0);

  __shared__ int s_start[RTPOSE_SKEL_MAX_PARTS + 1];
  if (lane == 0) {
    int acc = 0;
    for (int p = 0; p < P; ++p) {
      s_start[p] = acc;
      acc += res[kResPartCount + p];
    }
    s_start[P] = acc;
    if (WRITE_IDS) res[kResHeader + 0] = acc;
  }
  __syncthreads();
  rtpose_peak* peaks = reinterpret_cast<rtpose_peak*>(res + peaks_word);
  if (WRITE_IDS) {
    // ids = running counter over parts then peaks (paf_to_pose.py:141-142)
    for (int p = 0; p < P; ++p) {
      const int cnt = s_start[p + 1] - s_start[p];
      for (int i = lane; i < cnt; i += 64) peaks[(size_t)p * pcap + i].id = s_start[p] + i;
    }
  }
  // peak_infos_line[pos] (cpp:38-43): part-major position -> peak (WRITE_IDS = false only).  The part is the number of
  // starts at or below pos - s_start ascends - counted eight at a time, so that the LDS reads are independent and
  // in flight together: walking the starts one dependent read after the other cost the legacy process_paf 1.4 us per call
  // (profiles/r12_one_decoder.txt)
  auto line_peak_score = [&](int pos) -> float {
    int p = 0;
#pragma unroll 8
    for (int q = 1; q < P; ++q) p += pos >= s_start[q] ? 1 : 0;
    return peaks[(size_t)p * pcap + (pos - s_start[p])].score;
  };
  const int npeaks = s_start[P];

  // everything the walk needs from global memory about connection c of limb `limb`, into st[0 .. kStageWords)
  auto stage_conn = [&](int limb, int c, float* st) {
    const int part1 = sk.limb_part[limb][0], part2 = sk.limb_part[limb][1];
    const int32_t* cn = cnb + (size_t)limb * (1 + 3 * pcap);
    const rtpose_peak* pA = peaks + (size_t)part1 * pcap;
    const rtpose_peak* pB = peaks + (size_t)part2 * pcap;
    const int ia = cn[1 + 3 * c], ib = cn[1 + 3 * c + 1];
    const int id1 = WRITE_IDS ? s_start[part1] + ia : pA[ia].id;
    const int id2 = WRITE_IDS ? s_start[part2] + ib : pB[ib].id;
    st[0] = (float)id1;
    st[1] = (float)id2;
    st[2] = __int_as_float(cn[1 + 3 * c + 2]);
    st[3] = (id2 >= 0 && id2 < npeaks) ? (WRITE_IDS ? pB[ib].score : line_peak_score(id2)) : 0.f;
    st[4] = (id1 >= 0 && id1 < npeaks) ? (WRITE_IDS ? pA[ia].score : line_peak_score(id1)) : 0.f;
  };
  __shared__ int s_cbase[RTPOSE_SKEL_MAX_LIMBS + 1];
  if (STAGE_ALL) {
    if (lane < L) s_cbase[lane + 1] = cnb[(size_t)lane * (1 + 3 * pcap)];
    __syncthreads();
    if (lane == 0) {
      s_cbase[0] = 0;
      for (int l = 0; l < L; ++l) s_cbase[l + 1] += s_cbase[l];
    }
    __syncthreads();
    const int total = s_cbase[L];
    for (int i = lane; i < total; i += 64) {
      int limb = 0;
      while (i >= s_cbase[limb + 1]) ++limb;
      stage_conn(limb, i - s_cbase[limb], stage + (size_t)i * kStageWords);
    }
    __threadfence_block();
    __syncthreads();
  }

  int nrows = 0;
  bool overflow = false;
  for (int pair_id = 0; pair_id < L; ++pair_id) {
    const int part1 = sk.limb_part[pair_id][0], part2 = sk.limb_part[pair_id][1];
    const bool may_seed = (sk.seed_mask >> pair_id) & 1u;
    int nconn;
    const float* lst = stage;
    if (STAGE_ALL) {
      nconn = s_cbase[pair_id + 1] - s_cbase[pair_id];
      lst = stage + (size_t)s_cbase[pair_id] * kStageWords;
    } else {
      // stage this limb's connections, 64 in flight at a time
      nconn = cnb[(size_t)pair_id * (1 + 3 * pcap)];
      for (int c = lane; c < nconn; c += 64) stage_conn(pair_id, c, stage + (size_t)c * kStageWords);
      __threadfence_block();
      __syncthreads();
    }
    for (int c = 0; c < nconn; ++c) {
      const float* st = lst + (size_t)c * kStageWords;
      const float cid1 = st[0], cid2 = st[1], cscore = st[2], s2 = st[3];
      // search alive rows in order
      int found = 0, idx1 = 0, idx2 = 0;
      for (int r0 = 0; r0 < nrows; r0 += 64) {
        const int r = r0 + lane;
        bool hit = false;
        if (r < nrows && rows[(size_t)r * RW + kAlive] != 0.f)
          hit = rows[(size_t)r * RW + part1] == cid1 || rows[(size_t)r * RW + part2] == cid2;
        unsigned long long m = __ballot(hit);
        while (m) {
          const int b = __ffsll((long long)m) - 1;
          if (found == 0) idx1 = r0 + b;
          if (found == 1) idx2 = r0 + b;
          ++found;
          m &= m - 1;
        }
      }
      if (found == 1) {
        float* row = rows + (size_t)idx1 * RW;
        if (lane == 0 && row[part2] != cid2) {
          row[part2] = cid2;
          row[kCnt] = row[kCnt] + 1.f;
          row[kSum] = row[kSum] + (s2 + cscore);
        }
      } else if (found == 2) {
        float* r1 = rows + (size_t)idx1 * RW;
        float* r2 = rows + (size_t)idx2 * RW;
        bool both = false;
        if (lane < P) both = r1[lane] > 0.f && r2[lane] > 0.f;  // cid 0 reads as absent (cpp:155)
        const bool membership = __any(both);
        if (!membership) {
          if (lane < P) r1[lane] = r1[lane] + (r2[lane] + 1.f);
          if (lane == 0) {
            r1[kCnt] = r1[kCnt] + r2[kCnt];
            r1[kSum] = r1[kSum] + r2[kSum];
            r1[kSum] = r1[kSum] + cscore;
            r2[kAlive] = 0.f;  // erase(subset_idx2): order of the survivors is kept
          }
        } else if (lane == 0) {
          r1[part2] = cid2;
          r1[kCnt] = r1[kCnt] + 1.f;
          r1[kSum] = r1[kSum] + (s2 + cscore);
        }
      } else if (found == 0 && may_seed) {
        if (nrows < row_cap) {
          float* row = rows + (size_t)nrows * RW;
          const float s1 = st[4];
          if (lane < P) row[lane] = (lane == part1) ? cid1 : ((lane == part2) ? cid2 : -1.f);
          if (lane == 0) {
            row[kCnt] = 2.f;
            row[kSum] = (s1 + s2) + cscore;
            row[kAlive] = 1.f;
          }
          ++nrows;
        } else {
          overflow = true;
        }
      }
      __threadfence_block();
      __syncthreads();  // single-wave block: orders the row updates
    }
  }

  // prune (cpp:187-191) and emit
  int nh = 0;
  int32_t* hparts = res + peaks_word + 4 * P * pcap;
  float* hscore = reinterpret_cast<float*>(hparts + (size_t)P * hcap);
  for (int r = 0; r < nrows; ++r) {
    const float* row = rows + (size_t)r * RW;
    if (row[kAlive] == 0.f) continue;
    if (row[kCnt] < 4.f || row[kSum] / row[kCnt] < 0.3f) continue;
    if (nh < hcap) {
      if (lane < P) hparts[(size_t)nh * P + lane] = (int)row[lane];
      if (lane == 0) hscore[nh] = row[kSum] / row[kCnt];
      ++nh;
    } else {
      overflow = true;
    }
  }
  if (lane == 0) {
    res[kResHeader + 1] = nh;
    if (overflow) atomicOr(&res[kResHeader + 2], kOverflowHumans);
  }
}

// header + part counts of every record <- 0, except the words that describe the record: [3] / [4] = the capacities the
// record is laid out for (max_peaks_per_part, max_humans) - a record block describes itself, a consumer that parses it
// later, after the producer has grown its tables, does not need the producer's cfg of that moment - and [5] / [6] = the two
// values the caller passes: the skeleton's part and limb counts from the `_skel` entry points, 0 / 0 from the COCO-18
// ones, whose records define words 0..4 only (0 / 0 reads as 18 / 19).
__global__ void clear_header_kernel(int32_t* __restrict__ result, int result_words, int N, int pcap, int hcap, int P,
                                    int L, int peaks_word) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N * peaks_word) {
    const int wd = i % peaks_word;
    result[(size_t)(i / peaks_word) * result_words + wd] = wd == kResHeader + 3   ? pcap
                                                           : wd == kResHeader + 4 ? hcap
                                                           : wd == kResHeader + 5 ? P
                                                           : wd == kResHeader + 6 ? L
                                                                                  : 0;
  }
}

// ------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------
static const int kCoco18Limbs[19][4] = {  // (part A, part B, PAF x, PAF y): pafprocess.h:16-24's CocoPairs / CocoPairsNetwork
    {1, 2, 12, 13},  {1, 5, 20, 21},   {2, 3, 14, 15},   {3, 4, 16, 17},   {5, 6, 22, 23},  {6, 7, 24, 25},  {1, 8, 0, 1},
    {8, 9, 2, 3},    {9, 10, 4, 5},    {1, 11, 6, 7},    {11, 12, 8, 9},   {12, 13, 10, 11}, {1, 0, 28, 29}, {0, 14, 30, 31},
    {14, 16, 34, 35}, {0, 15, 32, 33}, {15, 17, 36, 37}, {2, 16, 18, 19},  {5, 17, 26, 27}};

// BODY_25 (25 parts, heat-map channel 25 = background; 26 limbs over 52 PAF channels), written from memory of upstream
// OpenPose's poseParameters.cpp: NOT VERIFIED against CMU's weights - no copy of that file or of the weights was at hand.
// The grouping run over these tables is this project's (the tf-pose pafprocess algorithm this file implements), not
// OpenPose's own bodyPartConnector.
static const int kBody25Limbs[26][4] = {
    {1, 8, 0, 1},     {1, 2, 14, 15},   {1, 5, 22, 23},   {2, 3, 16, 17},   {3, 4, 18, 19},   {5, 6, 24, 25},  {6, 7, 26, 27},
    {8, 9, 6, 7},     {9, 10, 2, 3},    {10, 11, 4, 5},   {8, 12, 8, 9},    {12, 13, 10, 11}, {13, 14, 12, 13}, {1, 0, 30, 31},
    {0, 15, 32, 33},  {15, 17, 36, 37}, {0, 16, 34, 35},  {16, 18, 38, 39}, {2, 17, 20, 21},  {5, 18, 28, 29}, {14, 19, 40, 41},
    {19, 20, 42, 43}, {14, 21, 44, 45}, {11, 22, 46, 47}, {22, 23, 48, 49}, {11, 24, 50, 51}};

static int fill_skeleton(rtpose_skeleton* s, int P, int L, const int (*limbs)[4], uint32_t seed_mask) {
  if (!s) return fail(RTPOSE_E_INVAL, "skeleton: NULL argument");
  memset(s, 0, sizeof(*s));
  s->struct_bytes = (uint32_t)sizeof(*s);
  s->num_parts = P;
  s->num_limbs = L;
  for (int l = 0; l < L; ++l) {
    s->limb_part[l][0] = limbs[l][0];
    s->limb_part[l][1] = limbs[l][1];
    s->limb_paf[l][0] = limbs[l][2];
    s->limb_paf[l][1] = limbs[l][3];
  }
  s->seed_mask = seed_mask;
  return 0;
}

// everything about the tables themselves; the channel counts of the maps are checked on top when they are known
static int check_skeleton(const rtpose_skeleton* s, bool with_channels, int heat_channels, int paf_channels) {
  if (!s) return fail(RTPOSE_E_INVAL, "skeleton: NULL argument");
  if (s->struct_bytes != sizeof(rtpose_skeleton))
    return fail(RTPOSE_E_INVAL, "skeleton: struct_bytes is %u, this library's rtpose_skeleton has %zu", s->struct_bytes,
                sizeof(rtpose_skeleton));
  const int P = s->num_parts, L = s->num_limbs;
  if (P < 1 || P > RTPOSE_SKEL_MAX_PARTS)
    return fail(RTPOSE_E_INVAL, "skeleton: num_parts %d outside [1,%d]", P, RTPOSE_SKEL_MAX_PARTS);
  if (L < 1 || L > RTPOSE_SKEL_MAX_LIMBS)
    return fail(RTPOSE_E_INVAL, "skeleton: num_limbs %d outside [1,%d]", L, RTPOSE_SKEL_MAX_LIMBS);
  if (L < 32 && (s->seed_mask >> L) != 0)
    return fail(RTPOSE_E_INVAL, "skeleton: seed_mask 0x%x has bits at or above num_limbs %d", s->seed_mask, L);
  if (with_channels && heat_channels < P)
    return fail(RTPOSE_E_INVAL, "skeleton: %d parts need at least %d heat-map channels, the map has %d", P, P, heat_channels);
  for (int l = 0; l < L; ++l) {
    const int a = s->limb_part[l][0], b = s->limb_part[l][1], cx = s->limb_paf[l][0], cy = s->limb_paf[l][1];
    if (a < 0 || a >= P || b < 0 || b >= P)
      return fail(RTPOSE_E_INVAL, "skeleton: limb %d joins parts %d and %d, outside [0,%d)", l, a, b, P);
    if (a == b) return fail(RTPOSE_E_INVAL, "skeleton: limb %d joins part %d with itself", l, a);
    if (cx < 0 || cy < 0) return fail(RTPOSE_E_INVAL, "skeleton: limb %d reads PAF channels %d and %d", l, cx, cy);
    if (with_channels && (cx >= paf_channels || cy >= paf_channels))
      return fail(RTPOSE_E_INVAL, "skeleton: limb %d reads PAF channels %d and %d, the map has %d", l, cx, cy, paf_channels);
    if (cx == cy) return fail(RTPOSE_E_INVAL, "skeleton: limb %d has the same PAF channel %d for x and y", l, cx);
    for (int k = 0; k < l; ++k)
      if (s->limb_part[k][0] == a && s->limb_part[k][1] == b)
        return fail(RTPOSE_E_INVAL, "skeleton: limb %d repeats limb %d (parts %d -> %d)", l, k, a, b);
  }
  return 0;
}

const rtpose_skeleton* coco18_skeleton() {
  static const rtpose_skeleton coco = [] {
    rtpose_skeleton s;
    fill_skeleton(&s, RTPOSE_NUM_PART, RTPOSE_NUM_LIMB, kCoco18Limbs, 0x3FFFFu);
    return s;
  }();
  return &coco;
}

// max_parts: the skeleton's part count (18 behind the entry points that take no skeleton)
static int check_cfg(const rtpose_decode_cfg* cfg, int max_parts) {
  if (!cfg) return fail(RTPOSE_E_INVAL, "decode: cfg is NULL");
  if (cfg->num_keypoints < 1 || cfg->num_keypoints > max_parts)
    return fail(RTPOSE_E_INVAL, "decode: num_keypoints must be in [1,%d]", max_parts);
  if (cfg->upsample < 1 || cfg->upsample > kMaxUp)
    return fail(RTPOSE_E_INVAL, "decode: upsample must be in [1,%d]", kMaxUp);
  if (cfg->max_peaks_per_part < 1 || cfg->max_peaks_per_part > kDecodeMaxPeaks)
    return fail(RTPOSE_E_INVAL, "decode: max_peaks_per_part must be in [1,%d]", kDecodeMaxPeaks);
  if (cfg->max_humans < 1) return fail(RTPOSE_E_INVAL, "decode: max_humans must be >= 1");
  return 0;
}

// cfg and sk have been checked by the caller.  header_P / header_L: what the records' header words 5 / 6 say.
// with_ids: also run peak_prefix_kernel (the running peak ids + the peak total); a full decode leaves that to
// assign_group_launch(write_ids = true), which writes them in its grouping kernel: one launch less
static int nms_launch(const float* heat, const rtpose_layout* lheat, int N, int h, int w, const rtpose_decode_cfg* cfg,
                      const rtpose_skeleton* sk, int header_P, int header_L, void* result, hipStream_t s, int flags,
                      bool with_ids) {
  if (N <= 0 || h <= 0 || w <= 0) return fail(RTPOSE_E_INVAL, "decode: empty batch");
  if (flags & ~(RTPOSE_NMS_NO_REFINE | RTPOSE_NMS_GAUSSIAN)) return fail(RTPOSE_E_INVAL, "nms: unknown flag");
  const int P = sk->num_parts;
  const int words = decode_result_words(cfg, P), peaks_word = decode_peaks_word(P);
  const int pcap = cfg->max_peaks_per_part, up = cfg->upsample;
  int32_t* res = static_cast<int32_t*>(result);
  hipLaunchKernelGGL(clear_header_kernel, dim3(ceil_div(N * peaks_word, 256)), dim3(256), 0, s, res, words, N, pcap,
                     cfg->max_humans, header_P, header_L, peaks_word);
  if (flags) {
    const size_t dyn = (size_t)2 * 25 * up * up * sizeof(float);
    hipLaunchKernelGGL(nms_refine_opt_kernel, dim3(cfg->num_keypoints, N), dim3(256), dyn, s, to_view(heat, lheat), h, w, up,
                       1.0 / (double)up, cfg->thresh_heatmap, pcap, res, words, flags, gauss_weights(), peaks_word);
  } else {
    hipLaunchKernelGGL(nms_refine_kernel, dim3(cfg->num_keypoints, N), dim3(256), 0, s, to_view(heat, lheat), h, w, up,
                       1.0 / (double)up, cfg->thresh_heatmap, pcap, res, words, peaks_word);
  }
  if (with_ids)
    hipLaunchKernelGGL(peak_prefix_kernel, dim3(N), dim3(64), 0, s, pcap, res, words, cfg->num_keypoints, P, peaks_word);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

// assignment + grouping on the peak tables in `result`; every switch below is taken on byte counts computed from P and L
int assign_group_launch(const float* paf, const rtpose_layout* lpaf, int N, int h, int w, double inv_up, int h1,
                        const rtpose_decode_cfg* cfg, const rtpose_skeleton* sk, void* workspace, size_t workspace_bytes,
                        void* result, hipStream_t s, bool write_ids) {
  const int P = sk->num_parts, L = sk->num_limbs;
  if (workspace_bytes < decode_workspace_bytes(cfg, P, L, N)) return fail(RTPOSE_E_INVAL, "decode: workspace too small");
  const int pcap = cfg->max_peaks_per_part;
  const int words = decode_result_words(cfg, P), peaks_word = decode_peaks_word(P);
  const int conn_words = decode_conn_words(cfg, L);
  int32_t* res = static_cast<int32_t*>(result);
  int32_t* conn = static_cast<int32_t*>(workspace);
  char* wsb = static_cast<char*>(workspace);
  size_t off = decode_ws_conn_bytes(cfg, L, N);
  float* score_ws = reinterpret_cast<float*>(wsb + off);
  off += decode_ws_score_bytes(cfg, L, N);
  float* rows_ws = reinterpret_cast<float*>(wsb + off);
  off += decode_ws_rows_bytes(cfg, P, N);
  unsigned long long* tie_ws = reinterpret_cast<unsigned long long*>(wsb + off);
  // scores (when they fit) + the LDS-resident candidate list of a limb that replays std::sort
  const bool in_lds = decode_scores_in_lds(cfg);
  const size_t lds = (in_lds ? (size_t)((pcap * pcap + 1) & ~1) * sizeof(float) : 0) +
                     (size_t)kTieLdsCands * sizeof(unsigned long long);
  static PerDeviceOnce attr_set;  // zero-initialised; the attribute is per device
  const int dev = current_device();
  if (!attr_set.is_set(dev)) {
    const void* limb_kernels[8] = {reinterpret_cast<const void*>(limb_assign_kernel<true, true, true>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<true, false, true>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<false, true, true>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<false, false, true>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<true, true, false>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<true, false, false>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<false, true, false>),
                                   reinterpret_cast<const void*>(limb_assign_kernel<false, false, false>)};
    for (const void* k : limb_kernels)
      RTPOSE_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    const void* group_kernels[8] = {reinterpret_cast<const void*>(group_kernel<true, true, true>),
                                    reinterpret_cast<const void*>(group_kernel<true, false, true>),
                                    reinterpret_cast<const void*>(group_kernel<true, true, false>),
                                    reinterpret_cast<const void*>(group_kernel<true, false, false>),
                                    reinterpret_cast<const void*>(group_kernel<false, true, true>),
                                    reinterpret_cast<const void*>(group_kernel<false, false, true>),
                                    reinterpret_cast<const void*>(group_kernel<false, true, false>),
                                    reinterpret_cast<const void*>(group_kernel<false, false, false>)};
    for (const void* k : group_kernels)
      RTPOSE_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    attr_set.set(dev);
  }
  const int up = cfg->upsample;
  int up_shift = -1;  // log2(up) when it is a power of two
  for (int k = 0; k < 8; ++k)
    if (up == (1 << k)) up_shift = k;
  // 32-bit per-sample offsets when an image's maps span less than 2^31 bytes and the pixel index fits the 24-bit multiplier
  const bool a32 = (long long)lpaf->hs * lpaf->ws < (1ll << 24) && (long long)lpaf->cstride * (long long)sizeof(float) < (1 << 24) &&
                   (long long)lpaf->hs * lpaf->ws * lpaf->cstride * (long long)sizeof(float) < (1ll << 31);
  {
#define RTPOSE_LIMB_A(LD, PW, A)                                                                                       \
  hipLaunchKernelGGL((limb_assign_kernel<LD, PW, A>), dim3(L, N), dim3(256), lds, s, *sk, peaks_word, to_view(paf, lpaf), \
                     h, w, inv_up, up_shift, h1, pcap, res, words, conn, conn_words, score_ws, tie_ws)
#define RTPOSE_LIMB(LD, PW)              \
  do {                                   \
    if (a32) RTPOSE_LIMB_A(LD, PW, true); \
    else RTPOSE_LIMB_A(LD, PW, false);   \
  } while (0)
    if (in_lds && up_shift >= 0) RTPOSE_LIMB(true, true);
    else if (in_lds) RTPOSE_LIMB(true, false);
    else if (up_shift >= 0) RTPOSE_LIMB(false, true);
    else RTPOSE_LIMB(false, false);
#undef RTPOSE_LIMB_A
#undef RTPOSE_LIMB
  }
  const int row_cap = decode_row_cap(cfg);
  // subset rows (when they fit) + the staged connections: of all L limbs when that fits beside the rows, else of one limb
  const bool rows_in_lds = decode_rows_in_lds(cfg, P);
  const size_t rows_bytes = rows_in_lds ? decode_rows_bytes(cfg, P) : 0;
  const size_t all_bytes = (size_t)L * pcap * kStageWords * sizeof(float);
  const bool stage_all = rows_bytes + all_bytes <= 96 * 1024;
  const size_t rows_lds = rows_bytes + (stage_all ? all_bytes : (size_t)pcap * kStageWords * sizeof(float));
#define RTPOSE_GROUP_W(W, S, R)                                                                                      \
  hipLaunchKernelGGL((group_kernel<W, S, R>), dim3(N), dim3(64), rows_lds, s, *sk, peaks_word, pcap, cfg->max_humans, \
                     res, words, conn, conn_words, row_cap, rows_ws)
#define RTPOSE_GROUP(S, R)                    \
  do {                                        \
    if (write_ids) RTPOSE_GROUP_W(true, S, R); \
    else RTPOSE_GROUP_W(false, S, R);         \
  } while (0)
  if (stage_all && rows_in_lds) RTPOSE_GROUP(true, true);
  else if (stage_all) RTPOSE_GROUP(true, false);
  else if (rows_in_lds) RTPOSE_GROUP(false, true);
  else RTPOSE_GROUP(false, false);
#undef RTPOSE_GROUP_W
#undef RTPOSE_GROUP
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace rtpose

using namespace rtpose;

extern "C" {

// ---- the COCO-18 entry points: the tables of coco18_skeleton(), header words 5 / 6 left 0 --------------------------------
size_t rtpose_decode_workspace_bytes(const rtpose_decode_cfg* cfg, int N) {
  if (check_cfg(cfg, RTPOSE_NUM_PART) || N <= 0) return 0;
  return decode_workspace_bytes(cfg, RTPOSE_NUM_PART, RTPOSE_NUM_LIMB, N);
}

size_t rtpose_decode_result_bytes(const rtpose_decode_cfg* cfg, int N) {
  if (check_cfg(cfg, RTPOSE_NUM_PART) || N <= 0) return 0;
  return (size_t)N * decode_result_words(cfg, RTPOSE_NUM_PART) * sizeof(int32_t);
}

int rtpose_nms_batch_ex(const float* heat, const rtpose_layout* lheat, int N, int h, int w,
                        const rtpose_decode_cfg* cfg, int nms_flags, void* result, void* stream) {
  if (!heat || !lheat || !result) return fail(RTPOSE_E_INVAL, "nms: NULL argument");
  static thread_local CheckedPtr c_heat, c_res;
  const int dev = current_device();
  int rcd = c_heat.check(heat, dev, "nms", "the heat-map tensor");
  if (!rcd) rcd = c_res.check(result, dev, "nms", "the result block");
  if (rcd) return rcd;
  if (int rc = check_cfg(cfg, RTPOSE_NUM_PART)) return rc;
  return nms_launch(heat, lheat, N, h, w, cfg, coco18_skeleton(), 0, 0, result, as_stream(stream), nms_flags,
                    /*with_ids=*/true);
}

int rtpose_nms_batch(const float* heat, const rtpose_layout* lheat, int N, int h, int w,
                     const rtpose_decode_cfg* cfg, void* result, void* stream) {
  return rtpose_nms_batch_ex(heat, lheat, N, h, w, cfg, 0, result, stream);
}

int rtpose_gaussian_kernel1d(double* weights, int cap) {
  if (!weights || cap < 2 * kGaussR + 1) return fail(RTPOSE_E_INVAL, "gaussian_kernel1d: need room for 25 doubles");
  const GaussW g = gauss_weights();
  for (int i = 0; i < 2 * kGaussR + 1; ++i) weights[i] = g.w[i];
  return 2 * kGaussR + 1;
}

int rtpose_decode_batch(const float* heat, const rtpose_layout* lheat, const float* paf,
                        const rtpose_layout* lpaf, int N, int h, int w, const rtpose_decode_cfg* cfg,
                        void* workspace, size_t workspace_bytes, void* result, void* stream) {
  return rtpose_decode_batch_ex(heat, lheat, paf, lpaf, N, h, w, cfg, 0, workspace, workspace_bytes, result, stream);
}

int rtpose_decode_batch_ex(const float* heat, const rtpose_layout* lheat, const float* paf,
                           const rtpose_layout* lpaf, int N, int h, int w, const rtpose_decode_cfg* cfg,
                           int nms_flags, void* workspace, size_t workspace_bytes, void* result, void* stream) {
  if (!heat || !lheat || !paf || !lpaf || !workspace || !result)
    return fail(RTPOSE_E_INVAL, "decode: NULL argument");
  // (the look-ups are repeated only when a caller passes other pointers than last time on this thread)
  static thread_local CheckedPtr c_heat, c_paf, c_ws, c_res;
  const int dev = current_device();
  int rcd = c_heat.check(heat, dev, "decode", "the heat-map tensor");
  if (!rcd) rcd = c_paf.check(paf, dev, "decode", "the PAF tensor");
  if (!rcd) rcd = c_ws.check(workspace, dev, "decode", "the workspace");
  if (!rcd) rcd = c_res.check(result, dev, "decode", "the result block");
  if (rcd) return rcd;
  int rc = check_cfg(cfg, RTPOSE_NUM_PART);
  if (!rc) rc = nms_launch(heat, lheat, N, h, w, cfg, coco18_skeleton(), 0, 0, result, as_stream(stream), nms_flags,
                           /*with_ids=*/false);
  if (rc) return rc;
  return assign_group_launch(paf, lpaf, N, h, w, 1.0 / (double)cfg->upsample, h * cfg->upsample, cfg, coco18_skeleton(),
                             workspace, workspace_bytes, result, as_stream(stream), /*write_ids=*/true);
}

// ---- the `_skel` entry points: the caller's tables, header words 5 / 6 = P / L ------------------------------------------
int rtpose_skeleton_coco18(rtpose_skeleton* skel) { return fill_skeleton(skel, 18, 19, kCoco18Limbs, 0x3FFFFu); }

int rtpose_skeleton_body25(rtpose_skeleton* skel) { return fill_skeleton(skel, 25, 26, kBody25Limbs, 0x3FFFFFFu); }

int rtpose_skeleton_check(const rtpose_skeleton* skel, int heat_channels, int paf_channels) {
  return check_skeleton(skel, true, heat_channels, paf_channels);
}

size_t rtpose_decode_workspace_bytes_skel(const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel, int N) {
  if (check_skeleton(skel, false, 0, 0) || check_cfg(cfg, skel->num_parts) || N <= 0) return 0;
  return decode_workspace_bytes(cfg, skel->num_parts, skel->num_limbs, N);
}

size_t rtpose_decode_result_bytes_skel(const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel, int N) {
  if (check_skeleton(skel, false, 0, 0) || check_cfg(cfg, skel->num_parts) || N <= 0) return 0;
  return (size_t)N * decode_result_words(cfg, skel->num_parts) * sizeof(int32_t);
}

int rtpose_nms_batch_skel(const float* heat, const rtpose_layout* lheat, int N, int h, int w, const rtpose_decode_cfg* cfg,
                          const rtpose_skeleton* skel, int nms_flags, void* result, void* stream) {
  if (!heat || !lheat || !result) return fail(RTPOSE_E_INVAL, "nms: NULL argument");
  int rc = check_skeleton(skel, false, 0, 0);
  if (!rc) rc = check_cfg(cfg, skel->num_parts);
  if (!rc && lheat->cstride - lheat->choff < cfg->num_keypoints)
    rc = fail(RTPOSE_E_INVAL, "nms: num_keypoints %d but the heat-map view has %d channels", cfg->num_keypoints,
              lheat->cstride - lheat->choff);
  if (rc) return rc;
  static thread_local CheckedPtr c_heat, c_res;
  const int dev = current_device();
  int rcd = c_heat.check(heat, dev, "nms", "the heat-map tensor");
  if (!rcd) rcd = c_res.check(result, dev, "nms", "the result block");
  if (rcd) return rcd;
  return nms_launch(heat, lheat, N, h, w, cfg, skel, skel->num_parts, skel->num_limbs, result, as_stream(stream), nms_flags,
                    /*with_ids=*/true);
}

int rtpose_decode_batch_skel(const float* heat, const rtpose_layout* lheat, const float* paf, const rtpose_layout* lpaf,
                             int N, int h, int w, const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel, int nms_flags,
                             void* workspace, size_t workspace_bytes, void* result, void* stream) {
  if (!heat || !lheat || !paf || !lpaf || !workspace || !result) return fail(RTPOSE_E_INVAL, "decode: NULL argument");
  // the channels a view can address: the kernels index the maps with the skeleton's numbers
  int rc = check_skeleton(skel, true, lheat->cstride - lheat->choff, lpaf->cstride - lpaf->choff);
  if (!rc) rc = check_cfg(cfg, skel->num_parts);
  if (rc) return rc;
  static thread_local CheckedPtr c_heat, c_paf, c_ws, c_res;
  const int dev = current_device();
  int rcd = c_heat.check(heat, dev, "decode", "the heat-map tensor");
  if (!rcd) rcd = c_paf.check(paf, dev, "decode", "the PAF tensor");
  if (!rcd) rcd = c_ws.check(workspace, dev, "decode", "the workspace");
  if (!rcd) rcd = c_res.check(result, dev, "decode", "the result block");
  if (rcd) return rcd;
  rc = nms_launch(heat, lheat, N, h, w, cfg, skel, skel->num_parts, skel->num_limbs, result, as_stream(stream), nms_flags,
                  /*with_ids=*/false);
  if (rc) return rc;
  return assign_group_launch(paf, lpaf, N, h, w, 1.0 / (double)cfg->upsample, h * cfg->upsample, cfg, skel, workspace,
                             workspace_bytes, result, as_stream(stream), /*write_ids=*/true);
}

}  // extern "C"
