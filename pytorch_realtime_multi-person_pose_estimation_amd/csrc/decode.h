// Layout of the decode result block and scratch (shared by host and device code).
#pragma once
#include "common.h"

namespace rtpose {

constexpr int kDecodeMaxPeaks = 1024;  // per (image, part) table capacity limit
constexpr int kLdsPairs = 110 * 110;   // candidate-score matrix entries that fit in LDS
constexpr int kLdsRowBytes = 720 * 21 * (int)sizeof(float);  // the LDS share of the subset rows (720 COCO-18 rows of 21 floats)
constexpr int kTieLdsCands = 4096;     // candidates (8 bytes each) of a limb that replays std::sort in LDS

// word (4-byte) offsets inside one image's result record
constexpr int kResHeader = 0;      // [0] n_peaks [1] n_humans [2] overflow flags [3] max_peaks_per_part [4] max_humans
                                   // [5] parts [6] limbs of the skeleton (0 / 0 from the COCO-18 entry points: reads as 18 / 19)
constexpr int kResPartCount = 8;   // int32[P]
constexpr int kResPeaks = 32;      // rtpose_peak[P * pcap], then human tables: here for every P up to 24 (decode_peaks_word)

constexpr int kOverflowPeaks = 1;   // a part had more than max_peaks_per_part peaks
constexpr int kOverflowHumans = 2;  // more subset rows / humans than capacity

// ---- sizes for a skeleton of P parts and L limbs: every one a function of P and L, and every fit decision taken on bytes.
// ---- The COCO-18 entry points and the legacy process_paf pass RTPOSE_NUM_PART / RTPOSE_NUM_LIMB (18 / 19).

// peaks start behind the part counts, at a multiple of 4 words and never below kResPeaks: any P up to 24 lays out alike
__host__ __device__ inline int decode_peaks_word(int P) {
  const int w = (kResPartCount + P + 3) & ~3;
  return w < kResPeaks ? kResPeaks : w;
}
inline int decode_result_words(const rtpose_decode_cfg* c, int P) {
  const int w = decode_peaks_word(P) + 4 * P * c->max_peaks_per_part + (P + 1) * c->max_humans;
  return (w + 3) & ~3;
}
// per image: L x { count, (a, b, score) x pcap }
inline int decode_conn_words(const rtpose_decode_cfg* c, int L) { return L * (1 + 3 * c->max_peaks_per_part); }
// subset rows alive at any time before pruning; LDS resident up to kLdsRowBytes, in the global workspace beyond
inline int decode_row_cap(const rtpose_decode_cfg* c) {
  int r = 2 * c->max_humans;
  if (r < 64) r = 64;
  return r;
}
// a subset row: P cids, the score sum, the part count, alive
inline size_t decode_rows_bytes(const rtpose_decode_cfg* c, int P) {
  return (size_t)decode_row_cap(c) * (P + 3) * sizeof(float);
}
inline bool decode_rows_in_lds(const rtpose_decode_cfg* c, int P) { return decode_rows_bytes(c, P) <= (size_t)kLdsRowBytes; }
inline bool decode_scores_in_lds(const rtpose_decode_cfg* c) {
  const size_t p = (size_t)c->max_peaks_per_part;
  return p * p * sizeof(float) <= (size_t)kLdsPairs * sizeof(float);
}
// workspace: [conn lists][candidate-score matrices when they exceed LDS][subset rows when
// they exceed LDS][candidate lists of the limbs that replay std::sort on an exact score tie]
inline size_t decode_ws_conn_bytes(const rtpose_decode_cfg* c, int L, int N) {
  return round_up((size_t)N * decode_conn_words(c, L) * sizeof(int32_t), 256);
}
inline size_t decode_ws_score_bytes(const rtpose_decode_cfg* c, int L, int N) {
  const size_t p = (size_t)c->max_peaks_per_part;
  return decode_scores_in_lds(c) ? 0 : round_up((size_t)N * L * p * p * sizeof(float), 256);
}
inline size_t decode_ws_rows_bytes(const rtpose_decode_cfg* c, int P, int N) {
  return decode_rows_in_lds(c, P) ? 0 : round_up((size_t)N * decode_rows_bytes(c, P), 256);
}
// (a limb's candidate list is at most p * p long and stays in LDS up to kTieLdsCands entries: at the default capacities -
//  p = 32 ... 64 - nothing is reserved; at p = 1024 this was 5.1 GB for 32 images whatever the maps held)
inline size_t decode_ws_tie_bytes(const rtpose_decode_cfg* c, int L, int N) {
  const size_t p = (size_t)c->max_peaks_per_part;
  if (p * p * sizeof(unsigned long long) <= (size_t)kTieLdsCands * sizeof(unsigned long long)) return 0;
  return round_up((size_t)N * L * p * p * sizeof(unsigned long long), 256);
}
inline size_t decode_workspace_bytes(const rtpose_decode_cfg* c, int P, int L, int N) {
  return decode_ws_conn_bytes(c, L, N) + decode_ws_score_bytes(c, L, N) + decode_ws_rows_bytes(c, P, N) +
         decode_ws_tie_bytes(c, L, N);
}

// the COCO-18 tables (pafprocess.h:16-24) as a skeleton, built once on the host: what the entry points without a skeleton
// argument and the legacy process_paf hand to the launchers
const rtpose_skeleton* coco18_skeleton();
// assignment + grouping on the peak tables in `result`.  write_ids = false: the peak tables already carry the caller's ids
// (legacy process_paf: ids of the caller's joint list); true: the grouping kernel writes the running ids and the peak total
int assign_group_launch(const float* paf, const rtpose_layout* lpaf, int N, int h, int w, double inv_up, int h1,
                        const rtpose_decode_cfg* cfg, const rtpose_skeleton* sk, void* workspace, size_t workspace_bytes,
                        void* result, hipStream_t s, bool write_ids);

}  // namespace rtpose
