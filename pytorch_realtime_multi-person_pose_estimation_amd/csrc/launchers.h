// Host entry points that one translation unit of the library defines and another calls: the kernel launchers, the
// weight packers and the geometry / size queries that go with them.  Declared here once and included by the callers
// (net.hip, shufflenet.hip, conv_wino.hip, conv_mfma_bf16.hip) and by the files that define them, so a prototype
// that drifts from its definition fails to compile (return type) or to link (arguments, -z defs).  Host-only
// declarations: nothing here reaches device code.
#pragma once
#include "common.h"

namespace rtpose {

// ---- fp32 direct conv (conv_mfma.hip) ----
// relu_max: the fused ReLU as max(v, 0), which stores a NaN sum as 0 - the form the inference executor launches (its outputs
// stay what they were; header section 2, "Non-finite values").  false (rtpose_conv2d): torch's relu, a NaN stays NaN
int conv2d_launch(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, hipStream_t s, bool relu_max);
int pack_weights_launch(const float* w, const float* bias, int cout, int cin_src, int k,
                        const int32_t* cin_map, int cin_packed, float* wp, float* bp, hipStream_t s);

// ---- conv1_1 (conv_first.hip) ----
size_t conv_first_packed_floats();
int conv_first_pack_launch(const float* w_oihw, const float* bias, float* wp, hipStream_t s, int to_bf16);
int conv_first_launch(const float* x_nchw, const float* x_lay, const rtpose_layout* lx, const float* wp, float* out,
                      const rtpose_layout* lo, int out_plane_pixels, int relu, int N, int H, int W, hipStream_t s,
                      int out_bf16);

// ---- stacked hourglass: the 7x7 stride-2 stem and up1 + upsample2(low3) (hourglass_ops.hip) ----
size_t conv7x7_s2_packed_floats();
int conv7x7_s2_pack_launch(const float* w_oihw, const float* bias, float* wp, hipStream_t s);
int conv7x7_s2_launch(const float* x_nchw, const float* x_lay, const rtpose_layout* lx, const float* wp, float* out,
                      const rtpose_layout* lo, int relu, int N, int H, int W, hipStream_t s);
int upsample2_add_launch(const float* up, const rtpose_layout* lup, const float* low, const rtpose_layout* llow, float* out,
                         const rtpose_layout* lout, int C, int N, int H, int W, hipStream_t s);

// ---- Winograd forms: F(2x2,3x3) and the form dispatch (conv_wino.hip) ----
int conv2d_winograd_fits(int k, int cin, int cout, int pool, int N, int H, int W, int hs, int fm);
int conv2d_wino_launch(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, hipStream_t s);
double conv2d_wino_issued_flops(int cin, int cout, int N, int H, int W);
// F(4x4,3x3) (conv_wino4.hip)
int conv2d_wino4_ok(int cin, int cout);
size_t packed_weight_floats_wino4(int cout, int cin);
int conv2d_wino4_launch(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, hipStream_t s);
int pack_weights_wino4_launch(const float* w, const float* bias, int cout, int cin_src, const int32_t* cin_map,
                              int cin_packed, float* wp, float* bp, hipStream_t s);
int wino4_amplification_launch(const float* w, int cout, int cin, float* amp, hipStream_t s);
double conv2d_wino4_issued_flops(int cin, int cout, int N, int H, int W);
// F(4,7) / F(6,7) / F(8,7) (conv_wino7.hip)
int wino7_default_fm();
int conv2d_wino7_fits(int cin, int cout, int N, int H, int W, int hs, int fm);
int conv2d_wino7_launch(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, int fm, void* scratch,
                        size_t scratch_bytes, hipStream_t s);
double conv2d_wino7_issued_flops(int cin, int cout, int N, int H, int W, int hs, int fm);
// hand-over scratch of a persistent launch in F(fm,7): fm = 8 needs 14 accumulators per wave, 4 / 6 twelve
size_t conv2d_wino7_scratch_bytes(int blocks, int fm = 6);
int* conv2d_wino7_scratch_err(void* scratch, int blocks);
size_t packed_weight_floats_wino7(int cout, int cin, int fm);
int pack_weights_wino7_launch(const float* w, const float* bias, int cout, int cin_src, const int32_t* cin_map,
                              int cin_packed, int fm, float* wp, float* bp, hipStream_t s);
int wino_amplification_launch(const float* w, int cout, int cin, int k, int fm, float* amp, hipStream_t s);

// ---- back-to-back 1x1 pairs: Mconv6 + Mconv7 of a stage as one launch (conv_tail.hip, conv_tail_bf16.hip) ----
int conv_tail_launch(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups, int N, int H, int W,
                     hipStream_t s);
int conv_tail_bf16_launch(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups, int N, int H, int W,
                          int out_f32, hipStream_t s);

// ---- bf16 conv (conv_mfma_bf16.hip) and its 64-channel instance (conv_c64_bf16.hip) ----
int conv2d_bf16_launch(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, int out_f32, int split,
                       hipStream_t s);
int pack_weights_bf16_launch(const float* w, const float* bias, int cout, int cin_src, int k,
                             const int32_t* cin_map, int cin_packed, void* wp, float* bp, int split,
                             hipStream_t s);
int conv_c64_bf16_fits(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, int out_f32, int split);
int conv_c64_bf16_launch(const rtpose_conv_desc* d, int N, int H, int W, hipStream_t s);

// ---- ShuffleNetV2: fused pointwise chains of the fp32 plan (pw_fused.hip) ----
int pw_fused_launch(const rtpose_pw_desc* d, int N, int H, int W, hipStream_t s);
int pack_pw_launch(const float* w, const float* bias, int cout, int cin_src, const int32_t* cin_map, int K,
                   int coutp, int col_off, float* wp, float* bp, hipStream_t s);
int pw_halo_stride(const rtpose_layout& l, int H, int W);
// column-mapped fp32 packing: a layer's columns in the memory order of the runs it writes
int pack_pw_cols_launch(const float* w, const float* bias, int cout, int cin_src, const int32_t* cin_map, int K,
                        int ncols, const int32_t* col_map, int coutp, int col_off, float* wp, float* bp,
                        hipStream_t s);
// ... and of the bf16 plan (pw_fused_bf16.hip)
int pw_fused_bf16_launch(const rtpose_pw_desc* d, int out_f32, int N, int H, int W, hipStream_t s);
int pack_pw_bf16_launch(const float* w, const float* bias, int cout, int cin_src, const int32_t* cin_map, int K,
                        int ncols, const int32_t* col_map, int coutp, int col_off, void* wp, float* bp,
                        hipStream_t s);
// conv5 + the two heads as one back-to-back launch (pw_head.hip)
int pw_head_launch(const rtpose_pw_desc* d1, const rtpose_pw_desc* d2, int N, int H, int W, hipStream_t s);
int pw_zero_columns_launch(float* wp, float* bp, int K, int coutp, int c0, int c1, hipStream_t s);
// ... and of the bf16 plan (pw_head_bf16.hip)
int pw_head_bf16_launch(const rtpose_pw_desc* d1, const rtpose_pw_desc* d2, int N, int H, int W, hipStream_t s);
int pack_head_w2_bf16_launch(const float* w, const float* bias, int cout, int K, int col_off, void* wp, float* bp,
                             hipStream_t s);
int zero_head_columns_bf16_launch(void* wp, float* bp, int K, int c0, int c1, hipStream_t s);
// conv.0 -> depthwise -> conv.2 of a stride-1 unit as one launch (unit_bf16.hip)
int unit_bf16_fits(const rtpose_pw_desc* d0, const rtpose_pw_desc* d2, int H, int W);
int unit_bf16_launch(const rtpose_pw_desc* d0, const rtpose_pw_desc* d2, int N, int H, int W, hipStream_t s);

}  // namespace rtpose
