/*
 * rtpose_mi355x.h — C ABI of librtpose_mi355x.so (gfx950 / MI355X only).
 *
 * This is the drop-in boundary for ONE hot path of
 * tensorboy/pytorch_Realtime_Multi-Person_Pose_Estimation:
 *
 *   rtpose_vgg forward  ->  heat-map peak NMS + sub-pixel refine  ->  PAF
 *   line-integral scoring  ->  greedy limb assignment  ->  person grouping
 *
 * Plain pointers and sizes only: no torch / numpy types cross this line.
 * Device pointers are HIP device pointers; `stream` is a hipStream_t passed
 * as void* (NULL = the default stream).  The library never allocates device
 * memory on the forward path: the host language (Python + torch here) owns
 * every buffer and hands in pointers + byte counts that the *_bytes() queries
 * report.
 *
 * Each entry point cites the reference interface (file:line under
 * /root/reference) it stands in for.
 *
 * Return codes: 0 = ok, negative = RTPOSE_E_* below.  The library never
 * falls back to a CPU path: without a HIP device every compute entry point
 * returns RTPOSE_E_NODEVICE (or the HIP error, negated and offset).
 */
#ifndef RTPOSE_MI355X_H
#define RTPOSE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPOSE_OK 0
#define RTPOSE_E_INVAL (-1)     /* bad argument / unsupported shape          */
#define RTPOSE_E_NODEVICE (-2)  /* no HIP device / HIP runtime error         */
#define RTPOSE_E_CAPACITY (-3)  /* a fixed-capacity device table overflowed  */
#define RTPOSE_E_STATE (-4)     /* call order violated (e.g. not bound)      */
#define RTPOSE_E_HIP(code) (-1000 - (int)(code))

/* ------------------------------------------------------------------------
 * 0. Library
 * ---------------------------------------------------------------------- */
const char* rtpose_version(void);
/* Last error text of the calling thread ("" if none). */
const char* rtpose_last_error(void);

/* ------------------------------------------------------------------------
 * 1. Activation layout ("shared-gap padded NHWC")
 *
 * Every activation tensor lives in HBM as rows of pixels, `cstride` floats
 * per pixel.  Pixel (n, y, x) sits at pixel index
 *        q = lead + (n * hs + y) * ws + x
 * with ws >= W + pad and hs >= H + pad, lead >= pad * ws + pad.  The pixels
 * that are not (n, y<H, x<W) are never written and stay zero, so a k x k
 * stencil tap (dy, dx) is the constant pixel offset dy * ws + dx and needs no
 * bounds test: the right gap of one row is the left gap of the next, and the
 * bottom gap of one image is the top gap of the next.
 * A plain dense NHWC tensor is the case lead = 0, ws = W, hs = H.
 * ---------------------------------------------------------------------- */
typedef struct rtpose_layout {
  int32_t cstride; /* floats per pixel                                     */
  int32_t choff;   /* first channel of the slice this view addresses       */
  int32_t ws;      /* row stride, pixels                                   */
  int32_t hs;      /* image stride, rows                                   */
  int32_t lead;    /* pixel index of (0,0,0)                               */
} rtpose_layout;

/* Pixels (not bytes) a buffer with this layout needs for N images of H x W,
 * including the tail slack the 2-D tile mode may read. */
size_t rtpose_layout_pixels(const rtpose_layout* l, int N, int H, int W);

/* ------------------------------------------------------------------------
 * 2. Convolution (stride 1, "same" padding, k in {1,3,7}) + bias (+ReLU)
 *    stands in for torch.nn.Conv2d + nn.ReLU as instantiated by
 *    lib/network/rtpose_vgg.py:23-35, :49-55 (ATen conv2d on the reference).
 *
 * Weights are consumed in the packed order produced by
 * rtpose_pack_conv_weights (shape independent).  fp32 in, fp32 accumulate
 * (v_mfma_f32_32x32x2_f32), fp32 out.
 * ---------------------------------------------------------------------- */
/* floats needed for the packed form of a [cout][cin][k][k] filter */
size_t rtpose_packed_weight_floats(int cout, int cin, int k);
/* floats needed for the padded bias */
size_t rtpose_packed_bias_floats(int cout);

/* Pack device OIHW fp32 weights (+bias) for the conv kernel.
 * `cin_map` (device or NULL): packed input channel c reads source channel
 * cin_map[c] (-1 = zero); NULL = identity over cin_src channels.
 * cin_packed is the channel count of the activation slice the conv will read
 * (>= cin_src, multiple of 8). */
int rtpose_pack_conv_weights(const float* w_oihw, const float* bias, int cout,
                             int cin_src, int k, const int32_t* cin_map,
                             int cin_packed, float* w_packed,
                             float* bias_packed, void* stream);

typedef struct rtpose_conv_desc {
  const float* in;       /* activation buffer base (layout `lin`)           */
  const float* w_packed; /* from rtpose_pack_conv_weights                   */
  const float* bias_packed;
  float* out;            /* activation buffer base (layout `lout`)          */
  rtpose_layout lin;
  rtpose_layout lout; /* the output slice: lout.choff + cout <= lout.cstride, or the launch is refused
                   (RTPOSE_E_INVAL) - rtpose_conv2d, rtpose_conv2d_bf16, rtpose_conv2d_bf16x3 with out_f32 and
                   the Winograd launches with pixel-major outputs.  Not checked where out_cmap places the
                   channels (absolute) or for the split hi / lo pieces of bf16x3 bf16 outputs.          */
  int32_t cin;  /* packed input channels (multiple of 8)                    */
  int32_t cout; /* real output channels                                     */
  int32_t k;    /* 1, 3 or 7                                                */
  int32_t relu; /* 0/1                                                      */
  int32_t pool; /* 0, or 1 = fuse MaxPool2d(2,2,0): `lout` is then the
                   half-resolution layout (rtpose_vgg.py:49-50)             */
  const int32_t* out_cmap; /* device int32[cout] or NULL: output channel n is
                   written at channel out_cmap[n] of the pixel (absolute, lout.choff
                   ignored) - folds channel_shuffle / concat of the ShuffleNetV2
                   blocks (rtpose_shufflenetV2.py:56-62) into the store        */
  int32_t wino_m; /* rtpose_conv2d_winograd* only (rtpose_conv2d ignores it): the form of THIS launch.
                   k = 3: 0 or 2 = F(2x2,3x3), 4 = F(4x4,3x3);  k = 7: 6 = F(6,7), 4 = F(4,7), 8 = F(8,7), 0 = the
                   library default (6; 4 with RTPOSE_WINOGRAD7_M=4 in the environment; never 8).  `w_packed` must
                   come from the packing of the same form.  Any other value is refused
                   (RTPOSE_E_INVAL): ZERO-INITIALISE descriptors (memset / `= {0}`) - the struct has
                   grown by trailing fields and may again.                                  */
  int32_t in_plane_pixels;  /* F(4x4,3x3) launches (k = 3, wino_m = 4) only; every other launch refuses a non-zero
                   value.  0: `in` is pixel-major as §1 describes.  Q > 0: the input slice is stored as CHANNEL PLANES -
                   channel c of the pixel with index q (§1) at float ((c / 8) * Q + q) * 8 + c % 8 of `in`, c counted
                   from channel 0 of the buffer (lin.choff, a multiple of 8, selects the first plane; lin.cstride is not
                   used); Q >= rtpose_layout_pixels(&lin, N, H, W) is the number of pixel slots per plane.  A chunk of
                   the kernel reads 8 channels of the 36 pixels of a patch: in planes those are whole 128-byte lines
                   instead of a quarter of each (csrc/conv_wino4.hip; 3x3 layers of the 32-image forward -8 %).       */
  int32_t out_plane_pixels; /* the same for the output slice (cout and lout.choff multiples of 8): a chain of F(4x4,3x3)
                   convs keeps its intermediates in planes, its first launch reads and its last one writes pixel-major.
                   rtpose_conv_first_planes writes planes for conv1_1.                                               */
  const float* prelu; /* device float[>= cout] or NULL: per-output-channel PReLU after the bias, y = x >= 0 ? x : prelu[n] * x
                   (nn.PReLU(num_parameters = cout), lib/network/openpose.py:56-63); `relu` must then be 0 and `pool` 0.
                   Taken by the fp32 rtpose_conv2d (k = 1, 3) and the fp32 k = 3 Winograd forms (F(2x2,3x3), F(4x4,3x3));
                   every other launcher refuses a non-NULL value (RTPOSE_E_INVAL).                                   */
  /* ---- residual epilogue and input pre-activation: the pre-activation Bottleneck of the stacked hourglass
   * (lib/network/rtpose_hourglass.py:9-46).  Taken by the fp32 rtpose_conv2d for k = 1, one group, no fused pool, no
   * out_cmap and no PReLU; every other launcher (and rtpose_conv2d for k != 1) refuses a non-zero value of any of these
   * fields (RTPOSE_E_INVAL).                                                                                          */
  const float* residual; /* device base or NULL: out = conv + bias + residual, read through `lres` at the output pixel and
                   at channel lres.choff + n for output channel n (`out += residual` of the Bottleneck, and the
                   x + fc_(y) + ... hand-over between stacks); `relu` must be 0 - nothing follows the sum.  Every output
                   element reads only its own residual element, so residual / lres may name the very slice out / lout
                   name: the conv then adds into the buffer.                                                        */
  const float* in_scale; /* device float[cin] or NULL (16-byte aligned), with in_shift: the conv reads                  */
  const float* in_shift; /* relu(in_scale[c] * x + in_shift[c]) where it would read input channel c - an inference
                   BatchNorm2d + ReLU in FRONT of the conv (`bn1` + `relu` of the Bottleneck), applied while the input
                   tile is staged: no pass of its own over the map.  Both or neither.  The ReLU / bias of the epilogue
                   are independent of it.                                                                           */
  rtpose_layout lres;    /* layout of `residual`: lres.choff + cout <= lres.cstride                                    */
  int32_t preact_cin;    /* real input channels of a pre-activated conv whose slice is padded to `cin`: channels
                   preact_cin .. cin - 1 are staged as 0 whatever the buffer, in_scale and in_shift hold there (their
                   taps stay zero taps).  0 = all `cin` channels are real.                                           */
} rtpose_conv_desc;

/* Launch one conv, or `ngroups` (<= 2) convs of identical geometry in one
 * grid (the L1/L2 branches of a CPM stage, rtpose_vgg.py:163-164). */
int rtpose_conv2d(const rtpose_conv_desc* d, int ngroups, int N, int H, int W,
                  void* stream);

/* Non-finite values.  A training run that diverges must say so: the loss of the reference becomes NaN, and so must ours.
 * PROMISED for the entry points a training step calls - rtpose_conv2d (bias and ReLU), rtpose_conv2d_bf16 (every instance it
 * dispatches to, the 64-input-channel kernel of rtpose_conv3x3_c64_bf16 included; without a fused pool),
 * rtpose_conv2d_wgrad, rtpose_conv2d_wgrad_bf16, rtpose_bn_stats / _apply / _grad, rtpose_dwconv3x3 with its _dgrad /
 * _wgrad, rtpose_conv7x7_s2 with relu = 0, rtpose_prelu_bf16, rtpose_prelu_grad_bf16 and the fp32 -> bf16 conversions
 * rtpose_nchw_to_layout_bf16, rtpose_layout_f32_to_bf16, rtpose_nchw_to_layout_split: NaN and Inf travel through the sums as IEEE arithmetic has them
 * (Inf + finite = Inf, Inf - Inf = NaN, anything + NaN = NaN; the class of a sum does not depend on its order), a fused
 * ReLU is torch's relu - NaN stays NaN, +Inf stays +Inf, -Inf, every negative value and -0 give +0 -, relu = 0 stores the
 * sum whatever it is (no clamp: -Inf and sums below -3.0e38 included), a conversion to bf16 keeps a NaN a NaN of its sign,
 * and a per-channel kernel keeps a non-finite value inside its channel.  The gap pixels of a slice are zeros that ARE
 * multiplied (no bounds test), so an Inf filter tap or an Inf of gy next to a border meets 0 and gives NaN where a sum over
 * the map alone has no such term (F.conv2d's own backward forms the same products).  The exceptions of the BatchNorm
 * passes stand next to rtpose_bn_stats and rtpose_bn_grad.  The backward masks - rtpose_relu_grad*, the recomputed mask of
 * rtpose_bn_grad, rtpose_prelu_grad - keep their documented comparisons: a NaN y passes no gradient; its forward has
 * stored that NaN already and the loss is NaN.
 * NOT PROMISED: inference.  The network executors (rtpose_net_*, every topology) launch the fp32 direct kernel with the
 * ReLU as max(v, 0), which stores a NaN sum as 0: what a plan computes is what it computed before this paragraph existed.
 * The fused 2x2 max-pool of any conv launcher, the Winograd, pointwise-pair, pointwise-chain and rtpose_conv_first*
 * kernels, the max-pools and the in_scale / in_shift pre-activation use max instructions as well.
 * tests/test_nonfinite_gpu.py. */

/* ---- 2b. Backward pass of these convs: what `total_loss.backward()` of train/train_VGG19.py:216 runs through
 * nn.Conv2d + nn.ReLU (ATen convolution_backward and threshold_backward on the reference).  csrc/conv_backward.hip.
 *
 * Weight gradient (+ bias gradient) of a stride-1 "same" conv, k in {1, 3, 7}:
 *     dw[o][c][dy][dx] = sum over (n, y, x) of gy[n, y, x, o] * x[n, y + dy - k/2, x + dx - k/2, c]
 *     dbias[o]         = sum over (n, y, x) of gy[n, y, x, o]                         (dbias != NULL)
 * `x` / `lx` is the conv's input slice: `cin` real channels from lx.choff, zero gaps of at least k/2 (the tap is the
 * constant pixel offset of §1, no bounds test); `gy` / `lgy` the gradient with respect to the conv's output: `cout`
 * channels from lgy.choff, read at the valid pixels only.  cin and cout are any value >= 1 and need no alignment:
 * channels outside the two slices are never read.  `dw` is dense OIHW fp32 (the shape of nn.Conv2d.weight), `dbias`
 * cout floats; both are OVERWRITTEN.  fp32 operands, fp32 accumulate (v_mfma_f32_32x32x2_f32).  The valid pixels are
 * cut, in (n, y, x) order, into rtpose_conv2d_wgrad_slabs() slabs that depend on the shape only - equal multiples of
 * 32 pixels but for the last one, across image boundaries; every slab's partial sums go to
 * `workspace` (device memory of the caller, rtpose_conv2d_wgrad_workspace_floats() floats, 16-byte aligned as `dw`)
 * and a second launch adds them in slab order: no atomics, the same inputs give the same bits on every run.
 * ZERO-INITIALISE the descriptor. */
typedef struct rtpose_wgrad_desc {
  const float* x;
  const float* gy;
  float* dw;
  float* dbias;     /* or NULL */
  float* workspace;
  size_t workspace_floats;
  rtpose_layout lx;
  rtpose_layout lgy;
  int32_t cin;
  int32_t cout;
  int32_t k;
} rtpose_wgrad_desc;
size_t rtpose_conv2d_wgrad_workspace_floats(int cin, int cout, int k, int N, int H, int W);
int rtpose_conv2d_wgrad_slabs(int cin, int cout, int k, int N, int H, int W);
int rtpose_conv2d_wgrad(const rtpose_wgrad_desc* d, int N, int H, int W, void* stream);
/* out = y > 0 ? gy : 0 over `channels` channels of the valid pixels (the gradient through a conv's fused ReLU, from the
 * conv's OUTPUT y): gaps are neither read nor written, so a zero-initialised `out` keeps its zero gaps and stays
 * convolvable.  Every element reads only its own gy element: out / lout may name the slice gy / lgy name.
 * The comparison is IEEE's on the fp32 y: +0, -0, NaN, -Inf and every negative y give +0; any other y - subnormals and
 * +Inf included - passes gy's 32 bits through untouched, NaN payloads and both Infs included.
 *
 * Data gradient: no entry point of its own.  The gradient with respect to a conv's input is rtpose_conv2d (relu = 0,
 * zero bias) of gy with the filter w.flip(2, 3).transpose(0, 1), packed by rtpose_pack_conv_weights. */
int rtpose_relu_grad(const float* y, const rtpose_layout* ly, const float* gy, const rtpose_layout* lgy,
                     float* out, const rtpose_layout* lout, int channels, int N, int H, int W, void* stream);
/* The same gradient on bf16 slices (csrc/act_grad_bf16.hip), for a training run whose activations and gradients stay in
 * the layouts between convs: y, gy and out are 2-byte bf16 slices and their layouts count ELEMENTS.  `y` is the conv's
 * output as rtpose_conv2d_bf16(out_f32 = 0) stored it - the buffer the next conv read; no other copy of y is needed -,
 * `ly` and `lgy` may differ in every field (gaps of 1 and 3, say).  Gaps and the channels beside the slices are neither
 * read nor written; every element reads only its own y and gy element, so out / lout may name the slice gy / lgy name.
 * The comparison is on the bf16 value: +0, -0, NaN and every negative y give +0; any other y - subnormals and +Inf
 * included - passes gy's 16 bits through untouched, NaN and Inf included.  This is where the pass can differ from
 * rtpose_relu_grad on the fp32 y the conv accumulated: 0 < y <= 2^-134 rounds to a bf16 +0 and masks the gradient here.
 * 16-byte loads and stores (8 bf16) where every base is 16-byte aligned and every cstride and choff a multiple of 8,
 * element by element otherwise: the same bits either way.  Every argument is checked on the host before any HIP call
 * (RTPOSE_E_INVAL with a text): NULL pointers or layouts, channels / N / H / W < 1, choff + channels > cstride, a layout
 * smaller than the map, N * H * W above the launch limit of 2^31 - 256 pixels, an odd base, and an `out` whose bytes
 * overlap those of gy or y without being the same slice (disjoint channel slices of one buffer are fine). */
int rtpose_relu_grad_bf16(const void* y, const rtpose_layout* ly, const void* gy, const rtpose_layout* lgy, void* out,
                          const rtpose_layout* lout, int channels, int N, int H, int W, void* stream);

/* ---- 2b, continued.  PReLU as a pass of its own, for training (csrc/prelu_backward.hip).  The conv launchers fuse
 * nn.PReLU(num_parameters = cout) into their epilogue (rtpose_conv_desc.prelu) and keep only its output; slopes may have
 * either sign (the reference draws them from N(0, 0.01)), so the sign of the output says nothing about the sign of the
 * PRE-activation z and a backward pass needs z itself.  A training forward launches the conv with relu = 0 and
 * prelu = NULL into z and then rtpose_prelu; the backward runs rtpose_prelu_grad on the same z.
 *
 * All three entry points check every argument on the host before any HIP call (RTPOSE_E_INVAL with a text), launch on
 * `stream`, and read and write only `channels` channels from `choff` at the valid pixels of each layout: gaps and
 * neighbouring channels are neither read nor written.  `slope` is device float[channels], read where it is: nothing is
 * packed or cached.  16-byte loads and stores where every cstride and choff is a multiple of 4 floats and every base is
 * 16-byte aligned, element by element otherwise: the same values either way.
 *
 * y = z >= 0 ? z : slope[c] * z : the bits of the fused epilogue (prelu1 in common.h), from a conv launched with
 * relu = 0 and prelu = NULL.  It differs from torch's F.prelu only in the sign of a zero under a negative slope.
 * y / ly may name the slice z / lz names. */
int rtpose_prelu(const float* z, const rtpose_layout* lz, const float* slope, float* y, const rtpose_layout* ly,
                 int channels, int N, int H, int W, void* stream);

/* torch's prelu_backward from the PRE-activation z:
 *     out[n,y,x,c] = z > 0 ? gy : slope[c] * gy              (out / lout may name gy / lgy)
 *     dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * gy)     (dslope != NULL; OVERWRITTEN)
 * z == 0 (either sign) and a NaN z take the slope path, as in torch: the forward's `>=` and the backward's `>` differ on
 * purpose.  Where z > 0 `out` holds gy's bits, a NaN's payload included.  fp32, one rounding per product.
 * z and gy are read once.  The valid pixels are cut, in (n, y, x) order, into rtpose_prelu_grad_slabs() slabs that
 * depend on the shape only - equal multiples of 64 pixels but for the last one, across image boundaries; within a slab a
 * thread owns fixed channels and adds its terms in a fixed pixel order, the threads of a channel are added in a fixed
 * order through LDS, every slab's [channels] partial goes to `workspace` (device memory of the caller,
 * rtpose_prelu_grad_workspace_floats() >= slabs * channels floats) and a second launch adds the partials in slab
 * order: no atomics, the same inputs give the same bits on every run.
 * dslope == NULL (frozen slopes): no reduction is launched and workspace may be NULL.
 * Both queries return 0 for a shape the launcher refuses (channels < 1, an empty map, N * H * W above the launch limit
 * of 2^31 - 256 pixels). */
size_t rtpose_prelu_grad_workspace_floats(int channels, int N, int H, int W);
int rtpose_prelu_grad_slabs(int channels, int N, int H, int W);
int rtpose_prelu_grad(const float* z, const rtpose_layout* lz, const float* slope, const float* gy,
                      const rtpose_layout* lgy, float* out, const rtpose_layout* lout, float* dslope,
                      float* workspace, size_t workspace_floats, int channels, int N, int H, int W, void* stream);

/* ---- 2b, continued.  PReLU between the bf16 convs of a layout-resident training run (csrc/prelu_backward.hip;
 * train.dense_stage): the two passes above with the rounding of rtpose_layout_f32_to_bf16 at their store, so that the
 * fp32 y and the fp32 masked gradient never exist.  `z`, `ga`, `gb` are fp32 slices; `y` / `out` are 2-byte bf16 slices
 * whose layouts count ELEMENTS.  Gaps and the channels beside the slices are neither read nor written, so a
 * zero-initialised destination keeps its zero gaps and stays convolvable, and several launches may fill disjoint channel
 * slices of one buffer (the concatenation of a dense block is that buffer).
 *
 *     y[n,y,x,c]   = bf16(z >= 0 ? z : slope[c] * z)                           (rtpose_prelu's fp32 value, rounded)
 *     g            = gb ? ga + gb : ga                                          (one fp32 add; gb may be NULL)
 *     out[n,y,x,c] = bf16(z > 0 ? g : slope[c] * g)                             (rtpose_prelu_grad's fp32 value on g, rounded)
 *     dslope[c]    = sum over valid (n,y,x) of (z > 0 ? 0 : z * g)              (dslope != NULL; fp32; OVERWRITTEN)
 *
 * bf16() rounds to nearest even as rtpose_layout_f32_to_bf16 does: Inf stays Inf, a NaN stays a NaN of its sign.  So y
 * has the bits of rtpose_prelu followed by rtpose_layout_f32_to_bf16 - what the next conv's input conversion makes of the
 * fp32 y -, and out the bits of rtpose_prelu_grad on the fp32 sum ga + gb followed by rtpose_layout_f32_to_bf16.  `gb` is
 * the gradient of a second consumer of the activation (a dense block's concatenation and the block's next conv both read
 * it): the sum autograd forms for it, which does not depend on the order of its two operands.  gb == NULL adds nothing
 * (ga's -0 stays -0, where ga + (+0) is +0).  z == 0 of either sign and a NaN z take the slope path; where z > 0, out is g
 * rounded.  A NaN z stores a NaN y.
 * The sums walk as rtpose_prelu_grad's do - the same slabs (rtpose_prelu_grad_bf16_slabs() == rtpose_prelu_grad_slabs()),
 * rectangle, unit and order, no atomics: the same inputs give the same bits on every run, and dslope has the bits
 * rtpose_prelu_grad gives on the summed gradient whenever both take their 4-channel units.  dslope == NULL (a frozen
 * slope): no reduction is launched, workspace may be NULL and is not written.
 * 16-byte loads and one 8-byte store of 4 bf16 where every fp32 slice has a 16-byte-aligned base and a cstride and choff
 * that are multiples of 4, and the bf16 slice an 8-byte-aligned base and a cstride and choff that are multiples of 4
 * elements; element by element otherwise: the same bits of y / out either way.
 * Every argument is checked on the host before any HIP call (RTPOSE_E_INVAL with a text): NULL pointers or layouts (gb
 * alone may be NULL, and lgb is then not looked at), channels / N / H / W < 1, choff + channels > cstride, a layout
 * smaller than the map, N * H * W above the launch limit of 2^31 - 256 pixels, an odd base of the bf16 slice, a bf16
 * slice whose bytes overlap those of z, ga, gb or slope, and a workspace below
 * rtpose_prelu_grad_bf16_workspace_floats() floats.  Both queries return 0 for a shape the launcher refuses. */
int rtpose_prelu_bf16(const float* z, const rtpose_layout* lz, const float* slope, void* y, const rtpose_layout* ly,
                      int channels, int N, int H, int W, void* stream);
size_t rtpose_prelu_grad_bf16_workspace_floats(int channels, int N, int H, int W);
int rtpose_prelu_grad_bf16_slabs(int channels, int N, int H, int W);
int rtpose_prelu_grad_bf16(const float* z, const rtpose_layout* lz, const float* slope, const float* ga,
                           const rtpose_layout* lga, const float* gb, const rtpose_layout* lgb, void* out,
                           const rtpose_layout* lout, float* dslope, float* workspace, size_t workspace_floats,
                           int channels, int N, int H, int W, void* stream);

/* ---- 2b, continued.  Training-mode BatchNorm2d (+ ReLU) on layout slices (csrc/batchnorm.hip): what the stacked
 * hourglass needs to train (train.batch_norm).  The inference plans know a BatchNorm only by its RUNNING statistics
 * (folded into a conv, or a per-channel (scale, shift) a 1x1 conv applies while it stages its input); these three compute
 * the statistics of the batch, normalise by them and differentiate through them.
 *
 * All three check every argument on the host before any HIP call (RTPOSE_E_INVAL with a text), launch on `stream`, and
 * read and write only `channels` channels from `choff` at the valid pixels of each layout: gaps and neighbouring channels
 * are neither read nor written, so a zero-initialised output keeps its zero gaps and stays convolvable.  16-byte loads and
 * stores where every cstride and choff is a multiple of 4 floats and every base is 16-byte aligned, element by element
 * otherwise: the same values either way.  No atomics and no scratch: the same inputs give the same bits on every run.
 * P = N * H * W below; P = 1 is refused, as torch refuses it.
 *
 * Sums.  The valid pixels are cut, in (n, y, x) order, into rtpose_bn_slabs() slabs that depend on the shape only - equal
 * multiples of 64 pixels but for the last one, across image boundaries; within a slab a thread owns fixed channels and
 * adds its terms in a fixed pixel order IN FP64 (an fp32 value and the product of two are exact there; the passes are
 * memory bound), the threads of a channel are added in a fixed order through LDS, every slab's two [channels] partials go
 * to `workspace` (device memory of the caller, 8-byte aligned, rtpose_bn_workspace_doubles() = slabs * 2 * channels +
 * 2 * channels doubles) and a second launch of one thread per channel adds them in slab order and finalises.
 * Both queries return 0 for a shape the launchers refuse (channels < 1, an empty map, P = 1, P above 2^31 - 256).
 *
 * rtpose_bn_stats.  ONE pass over x with SHIFTED sums, K[c] = x[0, 0, 0, c] (the channel's first value), all in fp64
 * (a NaN or Inf of x stays in its channel and gives the mean, variance and running statistics torch gives - but an Inf AT
 * pixel (0, 0, 0) is K itself: every x - K is NaN or -Inf and the mean is NaN where torch's is Inf):
 *     S1 = sum (x - K)      S2 = sum (x - K) * (x - K)
 *     md = S1 / P           mean = K + md           var = max(S2 / P - md * md, 0)        (the biased variance; NaN stays)
 *     invstd = 1 / sqrt(var + eps)      scale = weight * invstd      shift = bias - mean * scale
 * each rounded to fp32 once into save[RTPOSE_BN_SAVE_ROWS][channels]: rows mean, var, invstd, scale, shift, and mean_lo =
 * fp32(mean - fp32(mean)), the part of the mean its fp32 value lost (the backward's sums use mean + mean_lo).  (scale,
 * shift) is the pair _native_state.bn_scale_shift makes from the running statistics, here from the batch's.
 * |md| is of the order of the channel's standard deviation whatever its mean, so S2 / P - md * md does not cancel for
 * |mean| >> std.  Bounds against the float64 values m, v of the same fp32 inputs, u = 2^-53, D1 = sum |x - K| / P,
 * D2 = sum (x - K)^2 / P:   |mean - m| <= 2^-24 |m| + (P + 8) u (D1 + |m|),   |var - v| <= 2^-24 v + (3 P + 8) u D2
 * - one fp32 rounding plus fp64 dust; invstd, scale and shift are smooth functions of these in fp64, rounded once.
 * running_mean / running_var (both or neither; device float[channels]) are updated in place by torch's rule, in fp64:
 *     r = fp32((1 - momentum) * r + momentum * v),   v = mean, and var * P / (P - 1) for the variance. */
#define RTPOSE_BN_SAVE_ROWS 6
size_t rtpose_bn_workspace_doubles(int channels, int N, int H, int W);
int rtpose_bn_slabs(int channels, int N, int H, int W);
int rtpose_bn_stats(const float* x, const rtpose_layout* lx, const float* weight, const float* bias, float* running_mean,
                    float* running_var, double momentum, double eps, float* save, double* workspace,
                    size_t workspace_doubles, int channels, int N, int H, int W, void* stream);
/* y = scale[c] * x + shift[c] with save's rows 3 and 4: one fp32 multiply and one fp32 add, never fused (the expression
 * of the inference plan's pre-activation), then y <= 0 ? +0 : y if relu (a NaN y stays NaN).  y / ly may name the slice x / lx names. */
int rtpose_bn_apply(const float* x, const rtpose_layout* lx, const float* save, float* y, const rtpose_layout* ly, int relu,
                    int channels, int N, int H, int W, void* stream);
/* torch's native_batch_norm_backward (training) from x, gy, save and weight.
 *     g = relu ? (scale[c] * x + shift[c] > 0 ? gy : 0) : gy
 * - the mask is RECOMPUTED from x with apply's two fp32 operations, so it is the mask of the y apply wrote; no y is kept.
 * First pass, fp64, the two-stage reduction above:   G1 = sum g      G2 = sum g * (x - K)
 *     mdk = (mean + mean_lo) - K      dbias = G1      dweight = invstd * (G2 - mdk * G1)         (invstd: save's fp32 value)
 *     A = weight * invstd             B = A * G1 / P  C = A * invstd * dweight / P   (dweight before its rounding)
 * dbias, dweight, A, B, C rounded to fp32 once each; A, B, C go to the workspace's tail (float[3][channels] at double
 * offset slabs * 2 * channels).  Second pass, element by element in fp32, each operation rounded on its own:
 *     dx = (g * A - B) - (x - mean) * C
 * x - mean is formed first, so nothing cancels for |mean| >> std.  dweight and dbias are OVERWRITTEN; either may be NULL
 * (frozen) - the sums are still taken for dx.  dx may be NULL (the input needs no gradient): only the reduction runs.
 * dx / ldx may name the slice gy / lgy names.
 * Non-finite values stay in their channel.  The mask is IEEE's `> 0`: a NaN y passes no gradient (dbias of a channel whose
 * y is NaN is +0, where torch's threshold_backward passes gy; apply has stored that NaN, so the loss is NaN).  A NaN of gy
 * gives the NaN dbias, dweight and dx torch gives.  An Inf of gy gives torch's dbias; dweight is the difference of two
 * shifted sums, G2 - mdk * G1, and is torch's signed Inf or, where the two agree in sign, Inf - Inf = NaN; dx meets
 * Inf - Inf in another order than torch's and is not held to its class. */
int rtpose_bn_grad(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy, const float* save,
                   const float* weight, int relu, float* dx, const rtpose_layout* ldx, float* dweight, float* dbias,
                   double* workspace, size_t workspace_doubles, int channels, int N, int H, int W, void* stream);

/* ---- 2b, continued.  The two element-wise BatchNorm passes between the bf16 convs of a layout-resident training run
 * (csrc/batchnorm.hip; train.preact_chain): rtpose_bn_apply and the second pass of rtpose_bn_grad with the rounding of
 * rtpose_layout_f32_to_bf16 at their store, so that the fp32 y and the fp32 dx of a BatchNorm that sits between two bf16
 * convs never exist.  `x`, `gy` are fp32 slices; `y` / `dx` are 2-byte bf16 slices whose layouts count ELEMENTS, as in
 * rtpose_prelu_bf16.  Gaps and the channels beside the slices are neither read nor written, so a zero-initialised
 * destination keeps its zero gaps and stays convolvable.
 *
 *     y[n,y,x,c]  = bf16(rtpose_bn_apply's y)       v = scale[c] * x + shift[c], one fp32 multiply and one fp32 add, never
 *                                                   fused; relu: v <= 0 ? +0 : v (a NaN v stays NaN); then the rounding
 *     dx[n,y,x,c] = bf16(rtpose_bn_grad's dx)       (g * A - B) - (x - mean) * C, its five fp32 operations; then the rounding
 *
 * bf16() rounds to nearest even as rtpose_layout_f32_to_bf16 does: Inf stays Inf, a NaN stays a NaN of its sign.  So y has
 * the bits of rtpose_bn_apply followed by rtpose_layout_f32_to_bf16 - what the next conv's input conversion makes of the
 * fp32 y - and dx the bits of rtpose_bn_grad's fp32 dx followed by rtpose_layout_f32_to_bf16.
 * rtpose_bn_grad_bf16's first pass and finalising launch ARE rtpose_bn_grad's - the same kernel instances on the same slabs
 * (rtpose_bn_slabs()), the same fp64 sums in the same order, no atomics -, so dweight, dbias and the workspace tail A, B, C
 * have the bits rtpose_bn_grad gives on the same inputs.  The workspace is rtpose_bn_workspace_doubles() doubles; there
 * are no queries of their own.  dx == NULL, dweight == NULL and dbias == NULL behave as they do there (all three NULL is
 * refused; dx == NULL launches the reduction only).
 * Non-finite values: what rtpose_bn_apply / rtpose_bn_grad do with a NaN or an Inf of x or gy (above), then the rounding:
 * a finite fp32 value above bf16's largest rounds to Inf of its sign.
 * 16-byte loads and one 8-byte store of 4 bf16 where every fp32 slice has a 16-byte-aligned base and a cstride and choff
 * that are multiples of 4, and the bf16 slice an 8-byte-aligned base and a cstride and choff that are multiples of 4
 * elements (rtpose_prelu_bf16's rule); element by element otherwise: the same bits either way.  No scratch.
 * Every argument is checked on the host before any HIP call (RTPOSE_E_INVAL with a text): NULL pointers or layouts,
 * channels / N / H / W < 1, N * H * W = 1, choff + channels > cstride, a layout smaller than the map, N * H * W above the
 * launch limit of 2^31 - 256 pixels, an odd base of the bf16 slice, a bf16 slice whose bytes overlap those of x, gy, save or
 * weight (these passes never run in place), and a workspace below rtpose_bn_workspace_doubles() doubles. */
int rtpose_bn_apply_bf16(const float* x, const rtpose_layout* lx, const float* save, void* y, const rtpose_layout* ly,
                         int relu, int channels, int N, int H, int W, void* stream);
int rtpose_bn_grad_bf16(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy,
                        const float* save, const float* weight, int relu, void* dx, const rtpose_layout* ldx, float* dweight,
                        float* dbias, double* workspace, size_t workspace_doubles, int channels, int N, int H, int W,
                        void* stream);

/* ---- 2b, continued.  Backward pass of the depthwise 3x3 convolution, padding 1, stride 1 or 2 (csrc/dwconv_backward.hip):
 * what nn.Conv2d(C, C, 3, stride, 1, groups = C, bias = False) of the ShuffleNetV2 blocks needs to train
 * (train.dwconv3x3); the forward is rtpose_dwconv3x3.  H, W are the conv's INPUT size, stride is 1 or 2,
 * Ho = (H - 1) / stride + 1 and Wo likewise: rtpose_dwconv3x3's rule.
 *
 * Both launchers check every argument on the host before any HIP call (RTPOSE_E_INVAL with a text), launch on `stream`,
 * accept any C >= 1, and read and write only C channels from `choff`: neighbouring channels are neither read nor written,
 * and nothing but the valid pixels of an output slice is written.  16-byte loads and stores where every cstride and choff
 * is a multiple of 4 floats and every base is 16-byte aligned, element by element otherwise: the same values either way.
 * No atomics and no scratch: the same inputs give the same bits on every run.
 *
 * Weight gradient.
 *     dw[c][0][ky][kx] = sum over (n, yo, xo) of gy[n, yo, xo, c] * x[n, stride * yo + ky - 1, stride * xo + kx - 1, c]
 *     dbias[c]         = sum over (n, yo, xo) of gy[n, yo, xo, c]                  (dbias may be NULL)
 * Both are OVERWRITTEN; dw is dense [C][1][3][3] fp32, the shape of the nn.Conv2d.weight, dbias float[C].  `x` / lx is the
 * conv's input, H x W with zero gaps of at least 1 (a tap is a constant pixel offset, no bounds test); `gy` / lgy is
 * Ho x Wo and is read at its valid pixels only.  The sums follow rtpose_bn_grad's scheme: the valid OUTPUT pixels are cut,
 * in (n, yo, xo) order, into rtpose_dwconv3x3_wgrad_slabs() slabs that depend on the shape only - equal multiples of 64
 * pixels but for the last one, across image boundaries; within a slab a thread owns fixed channels and adds its 9 (+ 1)
 * terms in a fixed pixel order IN FP64 (the product of two fp32 values is exact there; the pass is memory bound), the
 * threads of a channel are added in a fixed order through LDS, every slab's [10][C] partials go to `workspace` (device
 * memory of the caller, 8-byte aligned, rtpose_dwconv3x3_wgrad_workspace_doubles() = slabs * 10 * C doubles) and a second
 * launch adds them in slab order and rounds once to fp32.  Against the float64 sum v of the same fp32 operands:
 * |result - v| <= 2^-24 |v| + (P_out + 8) 2^-53 sum |terms|, P_out = N * Ho * Wo; with integer operands whose sums of
 * absolute terms stay below 2^53 the result is fp32(v), bit for bit.
 * Both queries return 0 for a shape the launcher refuses (C < 1, an empty map, a stride other than 1 or 2, N * H * W above
 * the launch limit of 2^31 - 256 pixels). */
size_t rtpose_dwconv3x3_wgrad_workspace_doubles(int C, int N, int H, int W, int stride);
int rtpose_dwconv3x3_wgrad_slabs(int C, int N, int H, int W, int stride);
int rtpose_dwconv3x3_wgrad(const float* x, const rtpose_layout* lx, const float* gy, const rtpose_layout* lgy, float* dw,
                           float* dbias, double* workspace, size_t workspace_doubles, int C, int N, int H, int W, int stride,
                           void* stream);
/* Data gradient.  `w` is the forward's [9][C] tap-major packing (w[ky * 3 + kx][c]), UNFLIPPED: the kernel does the flip.
 *     dx[n, y, x, c] = sum over the taps (ky, kx) with (y + 1 - ky) and (x + 1 - kx) divisible by stride of
 *                      w[ky * 3 + kx][c] * gy[n, (y + 1 - ky) / stride, (x + 1 - kx) / stride, c]
 * `gy` / lgy is Ho x Wo with zero gaps of at least 1: a tap that lands on yo = -1, yo = Ho, xo = -1 or xo = Wo reads a gap
 * (an even H at stride 2 does reach yo = Ho).  fp32, one rounding per product and one per add, never fused, from +0, the
 * contributing taps in order of ascending gy row, then ascending gy column (ky = 2, 1, 0, within a row kx = 2, 1, 0): a
 * host restatement reproduces the bits.  At stride 1 this is what rtpose_dwconv3x3 computes with flipped taps and a zero
 * bias.  All H x W valid pixels of `dx` / ldx are written; dx must not overlap gy. */
int rtpose_dwconv3x3_dgrad(const float* gy, const rtpose_layout* lgy, const float* w, float* dx, const rtpose_layout* ldx, int C,
                           int N, int H, int W, int stride, void* stream);

/* ---- 2b, continued.  The depthwise 3x3 conv of a layout-resident bf16 training run (train.unit_chain,
 * train.dwconv3x3(compute_dtype='bf16')): the three kernels above with bf16 activations and gradients.  The taps, the
 * bias, every accumulator and every OUTPUT stay fp32 - a BatchNorm in training mode reads the fp32 pre-activation on one
 * side and writes an fp32-computed gradient on the other -, so each kernel differs from its fp32 form only in the element
 * type it loads: a bf16 value is widened exactly, and the arithmetic, its order and its roundings are the fp32 kernel's.
 * Each result therefore has the bits of the fp32 entry point run on the widened operands (rtpose_layout_bf16_to_f32).
 * bf16 slices point at 2-byte elements and their layouts count ELEMENTS per pixel; their gaps are bf16 zeros.
 *
 * rtpose_dwconv3x3_bf16_f32 (csrc/shufflenet_ops.hip).  out = bias + sum over the taps of widen(in) * w, in fp32: from the
 * bias, ky = 0, 1, 2 and within a row kx = 0, 1, 2, one rounding per product and one per add, never fused - the order of
 * rtpose_dwconv3x3 at either stride, whose bits it gives on the widened input.  `in` / lin is H x W with a zero gap of at
 * least 1, `out` / lout Ho x Wo fp32 (any gap; gaps are not written); `w` [9][C] and `bias` [C] fp32, neither NULL.  The
 * doors of rtpose_dwconv3x3_bf16: C % 8 == 0, both bases 16-byte aligned, lin's cstride and choff multiples of 8 elements,
 * lout's multiples of 4 floats, stride 1 or 2.  out must not overlap in.
 *
 * rtpose_dwconv3x3_wgrad_bf16 (csrc/dwconv_backward.hip).  rtpose_dwconv3x3_wgrad's scheme unchanged: the slabs of
 * rtpose_dwconv3x3_wgrad_slabs(), fp64 terms, the fixed-order LDS sum, per-slab partials, the second launch in slab order;
 * the workspace is rtpose_dwconv3x3_wgrad_workspace_doubles() doubles.  The product of two bf16 values is exact in fp64
 * (16 significant bits).  `x` (zero gap >= 1) and `gy` (read at its valid pixels only) are bf16; dw, dbias fp32, OVERWRITTEN.
 *
 * rtpose_dwconv3x3_dgrad_bf16 (csrc/dwconv_backward.hip).  rtpose_dwconv3x3_dgrad's expression in its order, on a bf16
 * `gy` (zero gap >= 1, of which only the ring of 1 is read), the fp32 [9][C] taps and an fp32 `dx`.
 *
 * The two backward forms accept any C >= 1 on slices of wider buffers.  A thread owns 4 channels, as in the fp32 kernels
 * (one 8-byte load of 4 bf16; the data gradient stores 16 bytes), where every bf16 slice has an 8-byte-aligned base and a
 * cstride and choff that are multiples of 4 elements (rtpose_prelu_bf16's rule) and the data gradient's dx a
 * 16-byte-aligned base and a cstride and choff that are multiples of 4 floats; one channel otherwise.  (Units of 8
 * channels, 16-byte loads, were measured for the data gradient and are slower at every depthwise shape of ShuffleNetV2;
 * the weight gradient's 10 fp64 accumulators per channel leave no registers for them.)  A last unit with fewer than 4 live
 * channels goes element by element.  The same bits in every form.  No scratch, no atomics: the same inputs give the same
 * bits on every run.  Neighbouring channels and gaps are never written.
 * Non-finite values: a NaN or an Inf of x / gy comes out where the fp32 kernel puts it.
 * Every argument is checked on the host before any HIP call (RTPOSE_E_INVAL with a text), as the fp32 launchers check
 * theirs: NULL pointers or layouts, C / N / H / W < 1, a stride other than 1 or 2, choff + C > cstride, a gap below 1
 * where one is read, a layout smaller than its map, an odd base of a bf16 slice, a tensor above the launch limit, a
 * workspace below the query's size, and memory that is not of the current device. */
int rtpose_dwconv3x3_bf16_f32(const void* in, const rtpose_layout* lin, const float* w, const float* bias, float* out,
                              const rtpose_layout* lout, int C, int N, int H, int W, int stride, void* stream);
int rtpose_dwconv3x3_wgrad_bf16(const void* x, const rtpose_layout* lx, const void* gy, const rtpose_layout* lgy, float* dw,
                                float* dbias, double* workspace, size_t workspace_doubles, int C, int N, int H, int W,
                                int stride, void* stream);
int rtpose_dwconv3x3_dgrad_bf16(const void* gy, const rtpose_layout* lgy, const float* w, float* dx, const rtpose_layout* ldx,
                                int C, int N, int H, int W, int stride, void* stream);

/* ---- 2b, continued.  Mixed-precision training: the weight gradient (+ bias gradient) of a stride-1 "same" conv,
 * k in {1, 3, 7}, from bf16 layout slices (csrc/conv_backward.hip; train.conv2d(compute_dtype='bf16')).  The forward
 * and the data gradient of such a step are rtpose_conv2d_bf16 (out_f32 = 1); this is the third kernel.  The reference has
 * no reduced-precision training: the contract is this project's.
 *     dw[o][c][dy][dx] = sum over (n, y, x) of gy[n, y, x, o] * x[n, y + dy - k/2, x + dx - k/2, c]
 *     dbias[o]         = sum over (n, y, x) of gy[n, y, x, o]                         (dbias != NULL)
 * `x` and `gy` point at bf16 elements and their layouts count ELEMENTS per pixel.  Products of two bf16 values are exact
 * in fp32; they are accumulated in fp32 (v_mfma_f32_32x32x16_bf16), dbias in fp32 pixel by pixel.  `dw` is dense OIHW
 * fp32, `dbias` cout floats; both are OVERWRITTEN.
 * The slices: both bases 16-byte aligned, choff and cstride multiples of 8 elements (the kernel loads 16 bytes = 8
 * channels of a pixel at a time); the gaps of `x` at least k/2 wide and bf16 zero; `gy` is read at its valid pixels only.
 * cin and cout are any value >= 1.  Channels outside [choff, choff + cin) of x and [choff, choff + cout) of gy never
 * reach a sum; those that share a 16-byte group with the last channels of a slice are loaded and cleared.
 * The sums follow rtpose_conv2d_wgrad's scheme: the valid pixels are cut, in (n, y, x) order, into
 * rtpose_conv2d_wgrad_bf16_slabs() slabs that depend on the shape only - equal multiples of 64 pixels but for the last
 * one, across image boundaries; every slab's partial sums go to `workspace` (device memory of the caller,
 * rtpose_conv2d_wgrad_bf16_workspace_floats() = slabs * (k * k * cout * cin + cout) floats rounded up to 4, 16-byte
 * aligned as `dw`) and a second launch adds them in slab order: no atomics, the same inputs give the same bits on every
 * run.  Every argument is checked on the host before any launch (RTPOSE_E_INVAL with a text); both queries are host-only
 * and return 0 for a shape the launcher refuses.  ZERO-INITIALISE the descriptor. */
typedef struct rtpose_wgrad_bf16_desc {
  const void* x;    /* bf16 layout slices */
  const void* gy;
  float* dw;
  float* dbias;     /* or NULL */
  float* workspace;
  size_t workspace_floats;
  rtpose_layout lx;   /* count ELEMENTS per pixel */
  rtpose_layout lgy;
  int32_t cin;
  int32_t cout;
  int32_t k;
} rtpose_wgrad_bf16_desc;
size_t rtpose_conv2d_wgrad_bf16_workspace_floats(int cin, int cout, int k, int N, int H, int W);
int rtpose_conv2d_wgrad_bf16_slabs(int cin, int cout, int k, int N, int H, int W);
int rtpose_conv2d_wgrad_bf16(const rtpose_wgrad_bf16_desc* d, int N, int H, int W, void* stream);

/* ---- the first layer: nn.Conv2d(3, 64, 3, 1, 1) (+ nn.ReLU), conv1_1 of the VGG-19 front end
 * (lib/network/rtpose_vgg.py:23-35, `model0.0`; csrc/conv_first.hip).  Reads the image where it is -
 * dense NCHW fp32 (`x_nchw`), or, with x_nchw = NULL, a layout buffer with >= 3 channels per pixel
 * (`x_layout` / `lx`: the plan's NHWC8 input written by rtpose_preprocess_u8) - and writes 64 channels
 * into `out` / `lout`: no NCHW -> NHWC conversion pass, no padding of the 3 input channels to 8.
 * The three channels are a slice of the pixel like any other: lx->choff + 3 > lx->cstride is refused
 * (RTPOSE_E_INVAL) by this launcher, by rtpose_conv_first_planes and by rtpose_conv_first_bf16.
 * `w_packed` (rtpose_conv_first_packed_floats() floats) from rtpose_pack_conv_first(w [64,3,3,3], bias [64]). */
size_t rtpose_conv_first_packed_floats(void);
int rtpose_pack_conv_first(const float* w_oihw, const float* bias, float* w_packed, void* stream);
int rtpose_conv_first(const float* x_nchw, const float* x_layout, const rtpose_layout* lx,
                      const float* w_packed, float* out, const rtpose_layout* lout, int relu, int N,
                      int H, int W, void* stream);
/* The same conv writing its 64 channels as 8 channel planes of `out_plane_pixels` pixel slots each (see
 * rtpose_conv_desc.in_plane_pixels; out_plane_pixels >= rtpose_layout_pixels(lout, N, H, W), lout->choff a multiple of 8,
 * lout->cstride unused): computed as the transposed product - a lane holds one pixel and 16 channels - so that 32 lanes
 * store 1 KB runs of a plane.  Same values, bit for bit. */
int rtpose_conv_first_planes(const float* x_nchw, const float* x_layout, const rtpose_layout* lx,
                             const float* w_packed, float* out, const rtpose_layout* lout, int out_plane_pixels,
                             int relu, int N, int H, int W, void* stream);

/* The same layer in the bf16 plan's arithmetic (BASELINE configs[2]; round 6): image and filters rounded to bf16 (round to
 * nearest even - what the plan's input conversion and rtpose_pack_conv_weights_bf16 do), products exact, fp32 accumulation,
 * + fp32 bias (+ReLU), output rounded to bf16.  `out` holds bf16 elements, `lout` counts them (cstride and choff multiples
 * of 8: a lane stores the 8 channels of a 16-byte piece); `w_packed` from rtpose_pack_conv_first_bf16 (the same
 * rtpose_conv_first_packed_floats() floats, filters rounded).  The source is fp32 either way - the image or an fp32 layout
 * buffer: the plan's NCHW -> bf16 NHWC16 conversion launch and its generic 16-channel conv1_1 are both replaced by this one
 * (the product of two bf16 values is exact in fp32, so the fp32 matrix instruction on rounded operands is this arithmetic). */
int rtpose_pack_conv_first_bf16(const float* w_oihw, const float* bias, float* w_packed, void* stream);
int rtpose_conv_first_bf16(const float* x_nchw, const float* x_layout, const rtpose_layout* lx,
                           const float* w_packed, void* out_bf16, const rtpose_layout* lout, int relu, int N,
                           int H, int W, void* stream);

/* ---- the stem of the stacked hourglass: nn.Conv2d(3, 64, 7, stride 2, padding 3) with `bn1` folded into filters and bias
 * by the caller (+ nn.ReLU), lib/network/rtpose_hourglass.py:162-164 (csrc/hourglass_ops.hip).  The only strided conv of
 * the library: H x W in, ceil(H / 2) x ceil(W / 2) out.  Reads the image like rtpose_conv_first (dense NCHW fp32, or with
 * x_nchw = NULL a layout buffer with >= 3 channels per pixel; the zero padding is masked loads, no gap is needed) and writes
 * 64 channels of `out` / `lout` (cstride and choff multiples of 4).  `w_packed` (rtpose_conv7x7_s2_packed_floats() floats)
 * from rtpose_pack_conv7x7_s2(w [64,3,7,7], bias [64] or NULL).  H and W are the INPUT size. */
size_t rtpose_conv7x7_s2_packed_floats(void);
int rtpose_pack_conv7x7_s2(const float* w_oihw, const float* bias, float* w_packed, void* stream);
int rtpose_conv7x7_s2(const float* x_nchw, const float* x_layout, const rtpose_layout* lx,
                      const float* w_packed, float* out, const rtpose_layout* lout, int relu, int N,
                      int H, int W, void* stream);

/* ---- two pointwise convs back to back: nn.Conv2d(128, 128, 1) + nn.ReLU -> nn.Conv2d(128, cout2 <= 64, 1), the
 * Mconv6 / Mconv7 pair that ends every stage-2..6 branch (lib/network/rtpose_vgg.py:120-127), as ONE launch
 * (csrc/conv_tail.hip; `ngroups` <= 2 branches per grid).  d1[g] / d2[g] are rtpose_conv_desc of the two convs
 * with the plain k = 1 packing (rtpose_pack_conv_weights); d1[g].out / lout are ignored - the 128-channel
 * intermediate never leaves the CU - and d2[g] reads it.  Same sums, in the same order, as two rtpose_conv2d
 * launches.  rtpose_conv1x1_pair_fits: 1 if the pair has this shape, its input slice (128 channels of d1[g].lin) and
 * output slice (d2[g].cout channels of d2[g].lout) lie inside their cstride and neither conv has an out_cmap. */
int rtpose_conv1x1_pair_fits(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups);
int rtpose_conv1x1_pair(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups, int N,
                        int H, int W, void* stream);

/* ---- fp32 Winograd forms of the 3x3 and 7x7 convs (csrc/conv_wino.hip, csrc/conv_wino7.hip) ------
 * Same module boundary as rtpose_conv2d (nn.Conv2d + nn.ReLU (+ nn.MaxPool2d) of
 * lib/network/rtpose_vgg.py:23-35, :49-55, :108-127), fewer matrix-core multiplies:
 *   k = 3: F(2x2, 3x3), 16 instead of 36 multiplies per 2 x 2 outputs and input channel (2.25x);
 *   k = 7: F(6, 7) along x, direct along y: 84 instead of 294 per 6 outputs (3.5x), no fused pool;
 *          or F(4, 7), 70 instead of 196 per 4 outputs (2.8x), selected per launch with
 *          rtpose_conv_desc.wino_m = 4 and the matching packing (rtpose_pack_conv_weights_winograd7);
 *          or F(8, 7), 98 instead of 392 per 8 outputs (4x; points of F(6,7) and +-5/4), wino_m = 8 and
 *          its packing: 12.5 % fewer matrix multiplies than F(6,7) for an error bound ~8x F(6,7)'s -
 *          opt-in only, no default selects it (DESIGN.md §3.0 has the measured error and times).
 * fp32 MFMA throughout; results differ from the direct sum by rounding only (k = 3: a few ulp,
 * k = 7: ~3e-5 at magnitude 4; whole network < 4e-5 on the stage outputs; contract 1e-3).
 * The descriptor is rtpose_conv_desc with `w_packed` from rtpose_pack_conv_weights_winograd
 * (transformed filters: 16/9 resp. 70/49 the size) and out_cmap = NULL.
 * rtpose_conv2d_winograd_fits: 1 when the conv described by `d` (k, cin, cout, pool, lin.hs) has a
 * Winograd instance at N x H x W (k = 3: cin a multiple of 16, or of 8 when cout_pad is 64 modulo
 * 128; k = 7: cin a multiple of 8, cout_pad a multiple of 128, and the transformed rows of a block
 * fit the LDS), else 0 - callers then use rtpose_conv2d with the plain packing. */
int rtpose_conv2d_winograd_fits(const rtpose_conv_desc* d, int N, int H, int W);
size_t rtpose_packed_weight_floats_winograd(int cout, int cin, int k);
int rtpose_pack_conv_weights_winograd(const float* w_oihw, const float* bias, int cout,
                                      int cin_src, int k, const int32_t* cin_map,
                                      int cin_packed, float* w_packed, float* bias_packed,
                                      void* stream);
int rtpose_conv2d_winograd(const rtpose_conv_desc* d, int ngroups, int N, int H, int W,
                           void* stream);
/* k = 3 with an explicit form m: 0 / 2 = F(2x2,3x3) (as above), 4 = F(4x4,3x3) (csrc/conv_wino4.hip): 36 instead of
 * 144 multiplies per 4 x 4 outputs and input channel (4x fewer than the direct sum), interpolation points
 * 0, +-3/4, +-3/2, inf; cin a multiple of 16, >= 32; transformed filters 36/9 the size.  Launch with
 * rtpose_conv_desc.wino_m = 4 and this packing.  Results differ from the direct sum by rounding only
 * (element-wise error bound ~3x F(2x2,3x3)'s, tests/test_wino_numerics_gpu.py). */
size_t rtpose_packed_weight_floats_winograd3(int cout, int cin, int m);
int rtpose_pack_conv_weights_winograd3(const float* w_oihw, const float* bias, int cout,
                                       int cin_src, int m, const int32_t* cin_map,
                                       int cin_packed, float* w_packed, float* bias_packed,
                                       void* stream);
/* k = 7 with an explicit form m (4, 6 or 8; 0 = default), see rtpose_conv_desc.wino_m;
 * (7 (m + 6) cin + 96) * cout_pad floats */
size_t rtpose_packed_weight_floats_winograd7(int cout, int cin, int m);
int rtpose_pack_conv_weights_winograd7(const float* w_oihw, const float* bias, int cout,
                                       int cin_src, int m, const int32_t* cin_map,
                                       int cin_packed, float* w_packed, float* bias_packed,
                                       void* stream);
/* The 7x7 kernel balances launches whose tiles do not come out as whole rounds over the CUs by
 * running persistent blocks that split tiles (results bit-identical either way).  A split tile is
 * handed from one block to the next through `scratch`: device memory OWNED BY THE CALLER
 * (256-byte aligned, rtpose_conv2d_winograd_scratch_bytes() of it, for the current device: sized for
 * the widest form, F(8,7)),
 * because the library allocates nothing on the forward path.  One scratch serves all launches that
 * are serialised on one stream.  With scratch = NULL (and through rtpose_conv2d_winograd) every
 * launch runs one block per tile.  The last int of the flag area is a device error word: bit 0 is
 * raised if a hand-over wait ever ran out (results of that launch are then invalid);
 * rtpose_conv2d_winograd_scratch_error copies it back (synchronises the stream). */
size_t rtpose_conv2d_winograd_scratch_bytes(void);
int rtpose_conv2d_winograd_ex(const rtpose_conv_desc* d, int ngroups, int N, int H, int W,
                              void* scratch, size_t scratch_bytes, void* stream);
int rtpose_conv2d_winograd_scratch_error(const void* scratch, int* error_word, void* stream);
/* Amplification estimate of a filter bank w[cout][cin][k][k] (device, OIHW fp32) in Winograd form:
 * k = 3 -> F(2x2,3x3); k = 7 -> F(m,7), m = 4, 6 or 8 (0 = default).  Writes ONE float to the device
 * address `amp_device`: the worst ratio over the output channels of the element-wise rounding-error
 * BOUND of the form to the direct sum's for inputs of uniform magnitude,
 *   max_i sum_f |AT[i][f]| (sum_n |BT[f][n]|) sum_{c,ky} |U[ky][f][c][o]|  /  sum_{c,ky,kx} |w[o][c][ky][kx]|
 * (i.i.d. Gaussian filters: 3.3, 62, 115, F(8,7) ~900; k = 3, m = 4 - F(4x4,3x3): see DESIGN.md §3.0).  The rtpose_vgg executor uses it to choose the form of a
 * layer (rtpose_net_options.winograd7 = RTPOSE_WINO7_AUTO). */
int rtpose_winograd_amplification(const float* w_oihw, int cout, int cin, int k, int m,
                                  float* amp_device, void* stream);

/* ---- fused pointwise chain of the ShuffleNetV2 pose network (BASELINE configs[3]) ----
 * stands in for lib/network/rtpose_shufflenetV2.py BasicBlock (:22-63): conv_bn_relu 1x1, optionally
 * preceded by the conv_bn depthwise 3x3 (stride 1) that feeds it and followed by
 * torch.cat((x1, x2), 1) + channel_shuffle(2) - ONE launch: the depthwise result is produced in LDS
 * and never stored, the pass-through half x1 is copied to its shuffled slots by the same blocks.
 *   out[p][cmap(n)] = act( bias[n] + sum_c A[p][c] * W[n][c] ),
 *   A[p][c] = in[p][c]                                            (dw_w == NULL)
 *           = dw_b[c] + sum_{ky,kx} dw_w[ky*3+kx][c] * in[p + (ky-1, kx-1)][c]   (zero padding = the layout gap)
 *   out[p][pt_cmap[i]] = pt_src[p][i], i < pt_c                   (pt_src != NULL)
 * fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32) / fp32 out. */
typedef struct rtpose_pw_desc {
  const float* in;          /* activation buffer base (layout `lin`; gap >= 1 when dw_w != NULL)   */
  const float* dw_w;        /* NULL, or device [9][cin] depthwise taps (BN folded), tap-major          */
  const float* dw_b;        /* device [cin] depthwise bias                                            */
  const float* w_packed;    /* from rtpose_pack_pw_weights: [cin/4][coutp][4]                          */
  const float* bias_packed; /* [coutp]                                                                */
  float* out;               /* activation buffer base (layout `lout`)                                 */
  rtpose_layout lin;
  rtpose_layout lout;
  int32_t cin;              /* packed input channels (multiple of 8)                                  */
  int32_t cout;             /* columns that are stored                                                */
  int32_t coutp;            /* columns of the packed matrix: 64, 128 or a multiple of 256             */
  int32_t relu;
  const int32_t* out_cmap;  /* NULL (column n -> channel lout.choff + n) or device int32[coutp]: column
                               n -> absolute channel of the pixel, < 0 = not stored                   */
  const float* pt_src;      /* NULL, or the buffer holding the pass-through channels (layout `lpt`)   */
  rtpose_layout lpt;
  const int32_t* pt_cmap;   /* device int32[pt_c]: pass-through channel i -> absolute output channel  */
  int32_t pt_c;
  /* pass-through, interleave form (pt_pairs > 0; pt_cmap / pt_c unused): output channel j < 2 pt_pairs is
   * source channel pt_a + j/2 (j even) or pt_b + j/2 (j odd) of `pt_src`, stored at channel
   * (j < pt_split ? pt_d0 + j : pt_d1 + j - pt_split): the next unit's x1 when both buffers keep their
   * channels as four runs [even-low | even-high | odd-low | odd-high] (contiguous loads and stores).     */
  int32_t pt_pairs, pt_a, pt_b, pt_split, pt_d0, pt_d1;
  const int32_t* in_planes; /* NULL (the input is the contiguous slice lin.choff .. + cin) or device
                               int32[cin / 4]: channel offset, relative to lin.choff, of every 4-channel
                               group of the GEMM's K axis (a 16-byte granular gather: x2 of a unit is two runs) */
} rtpose_pw_desc;
size_t rtpose_packed_pw_floats(int cin_packed, int coutp);
/* w_oi: device [cout][cin_src] (a 1x1 conv's OIHW weights), written to columns
 * [col_off, col_off + cout) of the packed matrix - several layers may share one matrix (the PAF and
 * heat-map heads, rtpose_shufflenetV2.py:107-108, run as one 128-column GEMM). */
int rtpose_pack_pw_weights(const float* w_oi, const float* bias, int cout, int cin_src,
                           const int32_t* cin_map, int cin_packed, int coutp, int col_off,
                           float* w_packed, float* bias_packed, void* stream);
int rtpose_pw_fused(const rtpose_pw_desc* d, int N, int H, int W, void* stream);

/* Column-mapped packing: packed column col_off + i = output channel col_map[i] of w_oi (NULL: i; < 0 or >= cout: a
 * zero column, zero bias) for i < ncols; K row c reads input channel cin_map[c] (NULL: c; < 0: a zero row).  The
 * ShuffleNetV2 plans store a layer's columns [0, cout) as CONTIGUOUS channels (out_cmap = NULL), so a layer that
 * writes runs of the four-run layout has its columns packed in memory order, and K may be padded with zero rows. */
int rtpose_pack_pw_weights_cols(const float* w_oi, const float* bias, int cout, int cin_src,
                                const int32_t* cin_map, int cin_packed, int ncols, const int32_t* col_map,
                                int coutp, int col_off, float* w_packed, float* bias_packed, void* stream);

/* ---- conv5 + both heads of the ShuffleNetV2 pose network as ONE back-to-back GEMM launch (csrc/pw_head.hip):
 *   slim.conv_bn_relu('conv5', 464, 1024, 1) -> { self.paf = nn.Conv2d(1024, 38, 1), self.heatmap = nn.Conv2d(1024, 19, 1) }
 * (lib/network/rtpose_shufflenetV2.py:104, :107-108, :143-147).  d1 = the wide conv (+ReLU): `in` / `lin` a contiguous
 * slice of cin channels (a multiple of 16, 32 <= cin <= 1024: below one 32-channel chunk the launcher refuses the
 * shape before any launch) or, with d1->in_planes, a gather of cin / 4 16-byte planes of
 * the pixel; w_packed [cin / 4][coutp][4] with cout = coutp a multiple of 256; d1->out is
 * ignored - the intermediate never leaves the registers.  d2 = the heads: ONE shared matrix [coutp1 / 4][64][4] whose
 * columns sit at their output channels (rtpose_pack_pw_weights with col_off; columns nobody owns must be zero), bias
 * [64]; 64 channels are stored at d2->lout.choff (16 bytes per lane, no column map).  Both GEMMs run transposed so
 * that the accumulators of the first are the B operand of the second (see the source).  fp32 in / accumulate / out. */
int rtpose_pw_head_fits(const rtpose_pw_desc* d1, const rtpose_pw_desc* d2);
int rtpose_pw_head(const rtpose_pw_desc* d1, const rtpose_pw_desc* d2, int N, int H, int W, void* stream);

/* bf16 form (the bf16 plan of BASELINE configs[3]): bf16 activations and pointwise weights, fp32 accumulate
 * (v_mfma_f32_32x32x16_bf16), depthwise taps / biases fp32, outputs rounded to bf16 (round-to-nearest-even)
 * or written fp32 (out_f32 != 0: the two heads).  In the desc `in`, `out`, `pt_src` point at 2-byte elements
 * (out: 4-byte when out_f32), the layouts count ELEMENTS, slices are multiples of 8 elements, cin a
 * multiple of 16.  The bf16 epilogue stores the GEMM's columns [0, cout) as the CONTIGUOUS channels
 * lout.choff .. (16 bytes per lane), so a layer that writes runs of the four-run layout is packed with a
 * column map (`col_map[i]` = output channel of packed column col_off + i, < 0 = a zero column).  out_cmap, if given,
 * is read per GROUP OF 8 COLUMNS by the bf16 epilogue: the columns 8 g .. 8 g + 7 are stored as the 8 contiguous
 * channels from out_cmap[8 g] (absolute, a multiple of 8; < 0: the group is not stored) - the zero-copy channel
 * shuffle of the ShuffleNetV2 plans scatters a layer's output over the slot groups the unit's x2 vacated; the fp32
 * (out_f32) epilogue reads it per column.  The pass-through half exists in its interleave form only.
 * Contract: oracle/shufflenet_oracle.py:forward_bf16_emulated (the reference has no bf16 path). */
size_t rtpose_packed_pw_bytes_bf16(int cin_packed, int coutp);
int rtpose_pack_pw_weights_bf16(const float* w_oi, const float* bias, int cout, int cin_src,
                                const int32_t* cin_map, int cin_packed, int ncols,
                                const int32_t* col_map, int coutp, int col_off, void* w_packed,
                                float* bias_packed, void* stream);
int rtpose_pw_fused_bf16(const rtpose_pw_desc* d, int out_f32, int N, int H, int W, void* stream);

/* conv5 + both heads as ONE launch in the bf16 plan (csrc/pw_head_bf16.hip; same reference lines as rtpose_pw_head):
 * d1 = the wide conv (+ReLU): bf16 input slice (layouts count ELEMENTS, multiples of 8) or a gather of cin / 8 16-byte
 * planes (d1->in_planes), cin a multiple of 16 up to 480, w_packed [cin / 8][coutp][8 bf16] from
 * rtpose_pack_pw_weights_bf16 (plain column order), cout = coutp a multiple of 256 up to 1024; d2 = the heads: ONE shared matrix [coutp1 / 8][64][8 bf16] packed by rtpose_pack_pw_head2_bf16
 * (the k order in which the first GEMM's accumulators come out of the matrix pipe; columns at their output channels,
 * columns nobody owns must be zero), fp32 bias [64], 64 fp32 channels stored at d2->lout.choff.  The conv5 feature is
 * rounded to bf16 (RNE) after its ReLU and never leaves the registers; sums are fp32 in a fixed order. */
/* One stride-1 ShuffleNetV2 unit - conv.0 (1x1 + ReLU) -> conv.1 (depthwise 3x3) -> conv.2 (1x1 + ReLU),
 * lib/network/rtpose_shufflenetV2.py:31-39 - as ONE launch in the bf16 plan (csrc/unit_bf16.hip): the conv.0 output only
 * exists in LDS (8 x 8 output tiles, conv.0 recomputed on the 10 x 10 halo; halo pixels outside the image are zero, as
 * the depthwise conv's padding wants).  d0 = conv.0: `in` / `lin` the stage buffer (bf16, ELEMENT counts, layout gap >= 1)
 * as a contiguous slice or a gather of cin / 8 planes (in_planes), cin a multiple of 16 up to 256, w_packed
 * [cin / 8][coutp][8 bf16] with coutp = 128 or 256 and zero columns past the real ones; d0->dw_w / dw_b = conv.1's fp32
 * taps [9][Kt] and bias [Kt], Kt = d2->cin (a multiple of 16, <= d0->coutp).  d2 = conv.2: w_packed [Kt / 8][coutp][8 bf16],
 * coutp = 128 or 256, `cout` existing columns (a multiple of 8), out_cmap[column] = absolute channel of the output pixel
 * (groups of 8 columns contiguous and 8-aligned, < 0: not stored), `out` / `lout` = the output buffer (may be the input
 * buffer when the output channels are not read by this launch: other blocks read x2 as their halo). */
int rtpose_unit_bf16_fits(const rtpose_pw_desc* d0, const rtpose_pw_desc* d2, int H, int W);
int rtpose_unit_bf16(const rtpose_pw_desc* d0, const rtpose_pw_desc* d2, int N, int H, int W, void* stream);

int rtpose_pw_head_bf16_fits(const rtpose_pw_desc* d1, const rtpose_pw_desc* d2);
int rtpose_pw_head_bf16(const rtpose_pw_desc* d1, const rtpose_pw_desc* d2, int N, int H, int W, void* stream);
int rtpose_pack_pw_head2_bf16(const float* w_oi, const float* bias, int cout, int cin, int col_off, void* w_packed,
                              float* bias_packed, void* stream);

/* ---- bf16 variant (BASELINE config 3: "bf16, multi-scale x4 + flip") ----------------
 * Same modules, bf16 activations and weights, fp32 accumulate
 * (v_mfma_f32_32x32x16_bf16), bias/ReLU/pool in fp32, output rounded to bf16
 * (round-to-nearest-even) or written as fp32 (out_f32 != 0).  The reference has no
 * reduced-precision path; the contract is pinned by oracle/net_oracle.py
 * (forward_bf16_emulated).  In a desc used here `in`, `w_packed` and `out` point at 2-byte
 * elements (out: 4-byte when out_f32) and the layouts count ELEMENTS per pixel; input slices
 * are multiples of 8 elements, cin a multiple of 16. */
size_t rtpose_packed_weight_bytes_bf16(int cout, int cin, int k);
int rtpose_pack_conv_weights_bf16(const float* w_oihw, const float* bias, int cout,
                                  int cin_src, int k, const int32_t* cin_map,
                                  int cin_packed, void* w_packed, float* bias_packed,
                                  void* stream);
int rtpose_conv2d_bf16(const rtpose_conv_desc* d, int ngroups, int N, int H, int W,
                       int out_f32, void* stream);
/* Two pointwise convs back to back in this arithmetic (round 6; csrc/conv_tail_bf16.hip - the bf16 sibling of
 * rtpose_conv1x1_pair): nn.Conv2d(128, 128 | 512, 1) + nn.ReLU -> nn.Conv2d(128 | 512, cout2 <= 64, 1), the pair that ends every
 * stage branch (lib/network/rtpose_vgg.py:101-105, :120-127), `ngroups` <= 2 branches per grid, as ONE launch: the
 * intermediate is rounded to bf16 where the two-launch form rounded it and never leaves the CU.  d1[g] / d2[g] are the
 * descs of the two convs with the k = 1 packing of rtpose_pack_conv_weights_bf16; d1[g].in / lin: 16-byte aligned bf16
 * slice; d1[g].out is ignored; d2[g].out / lout: bf16 elements, or fp32 when out_f32 (any channel offset).  Same contract
 * as two rtpose_conv2d_bf16 launches; the fp32 sums run in another order, so not bit for bit the same.  `_fits` says 1
 * only when, as for rtpose_conv1x1_pair_fits, both slices lie inside their cstride and neither conv has an out_cmap. */
int rtpose_conv1x1_pair_bf16_fits(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups);
int rtpose_conv1x1_pair_bf16(const rtpose_conv_desc* d1, const rtpose_conv_desc* d2, int ngroups, int N,
                             int H, int W, int out_f32, void* stream);
/* 3x3 convs with 64 bf16 INPUT channels - conv1_2 (+ fused 2x2 max-pool) and conv2_1 of the VGG-19 front end
 * (lib/network/rtpose_vgg.py:23-35, :69-72) - in their own kernel (round 6; csrc/conv_c64_bf16.hip): the whole K = 576 of a
 * 16 x 32 pixel tile in one LDS halo, persistent blocks, 16-byte stores from the accumulators.  d[0]: k = 3, cin = 64,
 * cout a multiple of 64, the packing of rtpose_pack_conv_weights_bf16, bf16 input and output slices 16-byte aligned, no
 * out_cmap; same contract as rtpose_conv2d_bf16, which takes this path by itself whenever `_fits` says 1 (the fp32 sums run
 * in another order than in its generic kernel: the last bits).  `_fits` is host-only. */
int rtpose_conv3x3_c64_bf16_fits(const rtpose_conv_desc* d, int ngroups, int N, int H, int W);
int rtpose_conv3x3_c64_bf16(const rtpose_conv_desc* d, int N, int H, int W, void* stream);
/* dense NCHW fp32 -> bf16 layout slice (channels [C, cpad) zero; cpad % 8 == 0) */
int rtpose_nchw_to_layout_bf16(const float* src_nchw, void* dst, const rtpose_layout* ldst,
                               int C, int cpad, int N, int H, int W, void* stream);
/* fp32 layout slice -> bf16 layout slice, and back */
int rtpose_layout_f32_to_bf16(const float* src, const rtpose_layout* lsrc, void* dst,
                              const rtpose_layout* ldst, int C, int cpad, int N, int H,
                              int W, void* stream);
int rtpose_layout_bf16_to_f32(const void* src, const rtpose_layout* lsrc, float* dst,
                              const rtpose_layout* ldst, int C, int N, int H, int W,
                              void* stream);

/* ---- bf16x3 variant: fp32-grade results from the bf16 matrix pipe ---------------------
 * Every fp32 operand v travels as two bf16s, hi = bf16(v) and lo = bf16(v - hi) (16 significant
 * bits), and a product is accumulated as hi*lo + lo*hi + hi*hi in fp32 (the lo*lo term, 2^-18
 * relative, is dropped): 3 MFMAs of the 16x faster bf16 pipe instead of fp32 MFMAs.  Activations
 * are stored per 8 channels as [hi x 8 | lo x 8] (32 B: the fp32 footprint); layouts of such
 * buffers count ELEMENTS (2 per channel, slices on 8-channel boundaries), `cin`/`cout` still
 * count channels.  Contract: oracle/net_oracle.py:forward_bf16x3_emulated; measured against the
 * fp32 oracle it stays inside the 1e-3 bound of the fp32 path (tests/test_bf16x3_gpu.py). */
size_t rtpose_packed_weight_bytes_bf16x3(int cout, int cin, int k);
int rtpose_pack_conv_weights_bf16x3(const float* w_oihw, const float* bias, int cout,
                                    int cin_src, int k, const int32_t* cin_map,
                                    int cin_packed, void* w_packed, float* bias_packed,
                                    void* stream);
int rtpose_conv2d_bf16x3(const rtpose_conv_desc* d, int ngroups, int N, int H, int W,
                         int out_f32, void* stream);
int rtpose_nchw_to_layout_split(const float* src_nchw, void* dst, const rtpose_layout* ldst,
                                int C, int cpad, int N, int H, int W, void* stream);
int rtpose_layout_f32_to_split(const float* src, const rtpose_layout* lsrc, void* dst,
                               const rtpose_layout* ldst, int C, int cpad, int N, int H,
                               int W, void* stream);
int rtpose_layout_split_to_f32(const void* src, const rtpose_layout* lsrc, float* dst,
                               const rtpose_layout* ldst, int C, int N, int H, int W,
                               void* stream);

/* MaxPool2d(kernel 2, stride 2, pad 0) between two layouts
 * (rtpose_vgg.py:49-50; floor semantics of nn.MaxPool2d). */
int rtpose_maxpool2x2(const float* in, const rtpose_layout* lin, float* out,
                      const rtpose_layout* lout, int C, int N, int H, int W,
                      void* stream);

/* out = up + Upsample(scale_factor 2, nearest)(low) as one pass: `up1 + self.upsample(low3)` of the stacked hourglass
 * (lib/network/rtpose_hourglass.py:84-85; csrc/hourglass_ops.hip).  `up` and `out` are H x W maps, `low` is H/2 x W/2 (H and W
 * even); C channels (a multiple of 4, as are every cstride and choff: 16-byte pieces) of each slice.  Each output element
 * reads only its own `up` element, so out / lout may name the slice up / lup names.  The sum is up + low, bit for bit what
 * the reference adds. */
int rtpose_upsample2_add(const float* up, const rtpose_layout* lup, const float* low,
                         const rtpose_layout* llow, float* out, const rtpose_layout* lout, int C,
                         int N, int H, int W, void* stream);

/* NCHW dense fp32 -> layout (channels [0,C) of the slice; extra channels of
 * the slice up to cpad are written as zero). */
int rtpose_nchw_to_layout(const float* src_nchw, float* dst,
                          const rtpose_layout* ldst, int C, int cpad, int N,
                          int H, int W, void* stream);
/* layout slice -> dense NCHW fp32 */
int rtpose_layout_to_nchw(const float* src, const rtpose_layout* lsrc,
                          float* dst_nchw, int C, int N, int H, int W,
                          void* stream);
/* layout slice -> layout slice (C channels) */
int rtpose_layout_copy(const float* src, const rtpose_layout* lsrc, float* dst,
                       const rtpose_layout* ldst, int C, int N, int H, int W,
                       void* stream);

/* ---- ShuffleNetV2 building blocks (lib/network/rtpose_shufflenetV2.py) -------
 * All HBM-bound, one pass.  BatchNorm (eval) is folded into weights/bias by the host. */
/* NCHW -> layout with a per-channel affine (the input BatchNorm2d(3), :96);
 * scale/shift: device float[C] or NULL. */
int rtpose_nchw_to_layout_affine(const float* src_nchw, float* dst, const rtpose_layout* ldst,
                                 int C, int cpad, int N, int H, int W, const float* scale,
                                 const float* shift, void* stream);
/* dense 3x3 stride-2 pad-1 conv for a tiny input channel count (stem, :97):
 * w packed [ky][kx][cin_pad][cout] fp32, cout % 4 == 0, bias[cout], fused ReLU. */
int rtpose_stem_conv3x3_s2(const float* in, const rtpose_layout* lin, const float* w,
                           const float* bias, float* out, const rtpose_layout* lout,
                           int cin_pad, int cout, int N, int H, int W, int relu, void* stream);
/* The same conv fused with what precedes it (:96-97): dense NCHW fp32 image -> per-channel
 * affine (the input BatchNorm2d(3); scale/shift device float[3] or NULL) -> conv 3x3 s2 p1
 * (zero padding applied after the affine, as in the reference graph) -> ReLU -> NHWC. */
int rtpose_stem_conv3x3_s2_nchw(const float* x_nchw, const float* scale, const float* shift,
                                const float* w, const float* bias, float* out,
                                const rtpose_layout* lout, int cout, int N, int H, int W,
                                int relu, void* stream);
/* The stem conv AND the max-pool that follows it (:96-99) in one launch: the 184 x 184 x 24 conv tensor is
 * never stored.  out: fp32 or (out_bf16) bf16 NHWC layout of the pooled map; scale/shift = the input
 * BatchNorm2d(3) or NULL; w packed [ky][kx][8][24] as for rtpose_stem_conv3x3_s2. */
int rtpose_stem_pool_nchw(const float* x_nchw, const float* scale, const float* shift, const float* w,
                          const float* bias, void* out, const rtpose_layout* lout, int cout, int N,
                          int H, int W, int out_bf16, void* stream);
int rtpose_stem_conv3x3_s2_nchw_ex(const float* x_nchw, const float* scale, const float* shift,
                                   const float* w, const float* bias, void* out,
                                   const rtpose_layout* lout, int cout, int N, int H, int W,
                                   int relu, int out_bf16, void* stream);
/* bf16 forms (bf16 plans: 2-byte activations, fp32 arithmetic, fp32 weights; C % 8 == 0) */
int rtpose_maxpool3x3s2_ceil_bf16(const void* in, const rtpose_layout* lin, void* out,
                                  const rtpose_layout* lout, int C, int N, int H, int W, void* stream);
int rtpose_dwconv3x3_bf16(const void* in, const rtpose_layout* lin, const float* w, const float* bias,
                          void* out, const rtpose_layout* lout, int C, int N, int H, int W, int stride,
                          void* stream);
int rtpose_layout_copy_cmap_bf16(const void* src, const rtpose_layout* lsrc, void* dst,
                                 const rtpose_layout* ldst, int C, const int32_t* cmap, int N, int H,
                                 int W, void* stream);
/* MaxPool2d(3, 2, 0, ceil_mode=True) (:98) */
int rtpose_maxpool3x3s2_ceil(const float* in, const rtpose_layout* lin, float* out,
                             const rtpose_layout* lout, int C, int N, int H, int W, void* stream);
/* depthwise 3x3, pad 1, stride 1 or 2 (+bias, no activation) (:35-38, :48-50);
 * w [9][C] fp32 (tap-major), C % 4 == 0, input layout gap >= 1. */
int rtpose_dwconv3x3(const float* in, const rtpose_layout* lin, const float* w, const float* bias,
                     float* out, const rtpose_layout* lout, int C, int N, int H, int W, int stride,
                     void* stream);
/* dst[.., cmap[c]] = src[.., c] for c < C (cmap: device int32[C], absolute dst channel) */
int rtpose_layout_copy_cmap(const float* src, const rtpose_layout* lsrc, float* dst,
                            const rtpose_layout* ldst, int C, const int32_t* cmap, int N, int H,
                            int W, void* stream);

/* dst(n,y,x,c) = alpha * dst(n,y,x,c) + beta * src[n][y][x][c] over a layout
 * slice (src dense NHWC).  Not on the reference's path: bench.py and the tests
 * use it to superimpose rasterised synthetic scenes on the outputs of the
 * randomly initialised network (no trained weights exist offline), so that the
 * decoder sees realistic peak counts while still consuming what the net wrote. */
int rtpose_layout_axpby(float* dst, const rtpose_layout* ldst, const float* src_nhwc,
                        int C, int N, int H, int W, float alpha, float beta,
                        void* stream);

/* ------------------------------------------------------------------------
 * 3. The rtpose_vgg network (lib/network/rtpose_vgg.py:60-225)
 *
 *   get_model('vgg19')       -> rtpose_net_create + rtpose_net_load_conv x92
 *   rtpose_model.forward     -> rtpose_net_forward   (rtpose_vgg.py:158-198)
 *
 * Conv index order == state_dict order of the reference module:
 *   model0.{0,2,5,7,10,12,14,16,19,21,23,25}, model1_1.{0,2,4,6,8},
 *   model2_1.{0,2,4,6,8,10,12} ... model6_1, model1_2 ..., model6_2
 *   (rtpose_vgg.py:141-155 registration order).
 * ---------------------------------------------------------------------- */
typedef struct rtpose_net rtpose_net;

int rtpose_net_create(int N, int H, int W, rtpose_net** out);
/* dtype: arithmetic of the plan.  RTPOSE_DTYPE_BF16 = bf16 activations/weights with fp32
 * accumulation (H, W multiples of 8); inputs, stage-output records and the final PAF /
 * heat-map stay fp32 at the API.  Weight arenas of the two dtypes are NOT interchangeable. */
#define RTPOSE_DTYPE_F32 0
#define RTPOSE_DTYPE_BF16 1
#define RTPOSE_DTYPE_BF16X3 2 /* split bf16 operands, 3 MFMAs per product: fp32-grade results */
int rtpose_net_create_ex(int N, int H, int W, int dtype, rtpose_net** out);
/* Per-plan choice of the arithmetic of the fp32 convs (the Winograd forms sum fewer, transformed
 * products: results differ from the direct sum by rounding, bounds in DESIGN.md §3.0).  The weight
 * arena of fp32 plans holds every packing a plan may choose (direct, F(2x2,3x3), F(4,7), F(6,7)), so
 * plans with different options share one arena and the choice costs nothing at run time.  The one
 * exception is winograd7 = 8: such a plan's arena is the standard layout FOLLOWED BY the F(8,7) packings
 * of the 7x7 convs (rtpose_net_weight_bytes reports the larger size, rtpose_net_load_conv through it
 * writes them too); an arena of that size also serves every other plan, not the other way round.
 *   winograd3: RTPOSE_WINO_DEFAULT (= RTPOSE_WINO3_AUTO since round 4; the environment's RTPOSE_WINOGRAD=0|7 ->
 *              direct, RTPOSE_WINOGRAD3_M=2|4 -> F(2x2,3x3) | F(4x4,3x3) forced), 0 = direct 3x3 kernels,
 *              1 = F(2x2,3x3), 4 = F(4x4,3x3) forced (layers without an F(4x4,3x3) instance: F(2x2,3x3)),
 *              RTPOSE_WINO3_AUTO = per layer F(4x4,3x3) if its amplification estimate is <= amp_limit, else
 *              F(2x2,3x3); decided by rtpose_net_finalize_weights
 *   winograd7: RTPOSE_WINO_DEFAULT (= RTPOSE_WINO7_AUTO since round 4; the environment's RTPOSE_WINOGRAD=0|3 ->
 *              direct, RTPOSE_WINOGRAD7_M=4|6|8 -> F(4,7) | F(6,7) | F(8,7) forced), 0 = direct, 4 = F(4,7),
 *              6 = F(6,7), 8 = F(8,7) forced (opt-in: ~8x the error bound of F(6,7), inside the 1e-3 contract for
 *              He / N(0, 0.01) filters; never chosen by AUTO), RTPOSE_WINO7_AUTO = per layer the fastest form whose amplification estimate
 *              (rtpose_winograd_amplification of the loaded filters) is <= amp_limit: F(6,7), else F(4,7),
 *              else direct; decided by rtpose_net_finalize_weights
 *   The default is the guarded one because the forms' error bounds scale with the estimate and nobody can
 *   vouch for filters that have not been seen (pose_model.pth, README.md:19): i.i.d. Gaussian / He filters
 *   estimate 115-120 in F(6,7) and 42-43 in F(4x4,3x3) and keep the fast forms; +-1 edge filters (273) do not.
 *   amp_limit: the AUTO modes only; <= 0 = the library default (256: twice what i.i.d. Gaussian
 *              filters give in F(6,7))
 * Fields are ignored by bf16 / bf16x3 plans.  A form that has no kernel instance at the plan's
 * geometry falls back to the next one (F(8,7) -> F(6,7) -> F(4,7) -> direct) whatever the options say. */
#define RTPOSE_WINO_DEFAULT (-1)
#define RTPOSE_WINO7_AUTO 1
#define RTPOSE_WINO3_AUTO 3
typedef struct rtpose_net_options {
  uint32_t struct_bytes; /* sizeof(rtpose_net_options) of the caller */
  int32_t dtype;         /* RTPOSE_DTYPE_*                            */
  int32_t winograd3;
  int32_t winograd7;
  float amp_limit;
} rtpose_net_options;
int rtpose_net_create_opts(int N, int H, int W, const rtpose_net_options* opt, rtpose_net** out);
int rtpose_net_dtype(const rtpose_net* net);
void rtpose_net_destroy(rtpose_net* net);
size_t rtpose_net_workspace_bytes(const rtpose_net* net);
size_t rtpose_net_weight_bytes(const rtpose_net* net);
/* Hand in the two device arenas.  The workspace is zero-filled on `stream`
 * (the gaps of every activation layout must be zero); the weight arena may be
 * shared by nets of different N/H/W (its packing is shape independent). */
int rtpose_net_bind(rtpose_net* net, void* workspace, size_t workspace_bytes,
                    void* weights, size_t weight_bytes, int zero_workspace,
                    void* stream);
int rtpose_net_num_convs(const rtpose_net* net);
/* name: e.g. "model0.0" (state_dict prefix); returns 0 or RTPOSE_E_INVAL */
int rtpose_net_conv_info(const rtpose_net* net, int idx, char* name,
                         int name_cap, int* cout, int* cin, int* k);
/* Pack one conv's OIHW weight + bias (device pointers) into the weight arena */
int rtpose_net_load_conv(rtpose_net* net, int idx, const float* w_oihw,
                         const float* bias, void* stream);
/* After the last rtpose_net_load_conv: fixes the form of every conv of an RTPOSE_WINO7_AUTO / RTPOSE_WINO3_AUTO plan from
 * the amplification estimates of the filters just loaded (synchronises `stream` once to read them).
 * Optional for the other modes and called by the next forward if the host did not.  Plans that share one
 * weight arena may be loaded through any one of them: every fp32 rtpose_net_load_conv advances the arena's
 * generation, and each plan re-reads the estimates and re-decides its forms (here, in rtpose_net_forward* and
 * in rtpose_net_conv_numerics) when the generation it decided at is no longer the arena's. */
int rtpose_net_finalize_weights(rtpose_net* net, void* stream);
/* Arithmetic of conv idx in this plan: *form = 0 direct, 3 = F(2x2,3x3), 43 = F(4x4,3x3), 4 = F(4,7), 6 = F(6,7),
 * 8 = F(8,7); amp[4] = amplification estimates of the loaded filters in F(2x2,3x3) / F(4,7) / F(6,7) / F(4x4,3x3) (0 where
 * the form does not apply; F(8,7) has no entry - rtpose_winograd_amplification(w, cout, cin, 7, 8, ..) computes its estimate; synchronises `stream` if they have not been read back yet).  Either may be NULL. */
int rtpose_net_conv_numerics(rtpose_net* net, int idx, int* form, float* amp, void* stream);
/* Device-side error word of the plan (synchronises `stream`): bit 0 = a split-tile hand-over of a
 * persistent 7x7 launch timed out (see rtpose_conv2d_winograd_ex); 0 = none.  The word is cleared. */
int rtpose_net_device_status(rtpose_net* net, int* error_word, void* stream);
/* The persistent 7x7 launches (>= one tile per CU, not whole rounds) split tiles between neighbouring blocks and hand
 * the partial sums over through device flags - valid on a device that dispatches a 1-D grid in order with the blocks of
 * a round resident together, i.e. an exclusive, unmasked MI355X.  enable = 0 makes every 7x7 launch of the plan run one
 * block per tile instead: the same results, bit for bit (the sums run in the order of an unsplit tile either way), a
 * few per cent slower at batch 32 - for CU-masked or shared devices.  Default 1, or 0 when RTPOSE_W7_PERSIST=0 is in the
 * environment; rtpose_net_device_status switches it off by itself when it reads a timed-out hand-over (captured launch
 * lists are dropped with it); a caller of rtpose_net_device_status_async that later finds bit 0 in its host word calls
 * rtpose_net_set_persistent7(net, 0) itself (pipeline.py does). */
int rtpose_net_set_persistent7(rtpose_net* net, int enable);
/* A consumer that reads the stage-6 maps where the net wrote them (rtpose_net_output_view) on ANOTHER stream - the pose
 * decoder of batch k under the forward of batch k + 1 - hands in the HIP event it records behind its last read: every
 * later forward of the plan waits for that event (hipStreamWaitEvent on the forward's stream) in front of its first launch
 * that writes the maps' buffer, and for nothing else (fp32: conv4_4_CPM, which writes the out1 channels of the same concat
 * buffer - the reader runs beside the trunk; bf16 / bf16x3: the last launch).  RTPOSE_GUARD_WHOLE_FORWARD=1 (or
 * RTPOSE_GUARD_FINE=0) in the environment moves the wait in FRONT of the launch list (the reader never beside this
 * plan's kernels; 1 % slower).
 * The guard stays installed until it is replaced or removed: NULL = no guard.  The event must have been recorded and must
 * outlive the guard.  (History, DESIGN.md 3.3: a decoder built with packed-fp32 VALU instructions returned wrong limb scores
 * beside the bf16 plan's kernels; the library's decoder is built without them.) */
int rtpose_net_set_output_guard(rtpose_net* net, void* hip_event);
/* Index (rtpose_net_launch_info numbering) of the launch a guarded forward waits in front of - decided, like the guard
 * itself, the first time either function is called on the plan (the environment is read then); host-only. */
int rtpose_net_output_guard_launch(rtpose_net* net);
int rtpose_net_persistent7(const rtpose_net* net);
/* The same without the wait: queues the copy of the error word into *host_word (pinned host memory, or the copy
 * is not asynchronous) and its clearing on `stream` and returns; the word is valid once the caller has waited for
 * anything it queued on `stream` afterwards (an event behind the D2H of a batch's records: the host that
 * pipelines batches never synchronises the whole stream for it). */
int rtpose_net_device_status_async(rtpose_net* net, int* host_word, void* stream);
/* 1 when forwards of this plan replay a captured hipGraph (RTPOSE_GRAPH=1 in the environment and the capture
 * succeeded), else 0. */
int rtpose_net_graph_active(const rtpose_net* net);
/* Enqueue the whole forward on `stream`: x is dense NCHW fp32 [N,3,H,W]. */
int rtpose_net_forward(rtpose_net* net, const float* x_nchw, void* stream);
/* The net's own NHWC8 input buffer, for producers that write it directly
 * (rtpose_preprocess_u8), and the forward that then skips the NCHW conversion.
 * The view holds what the PRODUCER wrote: rtpose_net_forward of an fp32 plan reads the NCHW
 * image directly (conv1_1, csrc/conv_first.hip) and does not refresh it. */
int rtpose_net_input_view(const rtpose_net* net, float** base, rtpose_layout* layout);
int rtpose_net_forward_prepared(rtpose_net* net, void* stream);
/* Copy stage output `which` (0..11 = saved_for_loss order: out1_1, out1_2,
 * ... out6_1, out6_2; rtpose_vgg.py:166-196) as dense NCHW.  Only the last
 * two survive a forward unless keep_intermediates was set. */
int rtpose_net_set_keep_intermediates(rtpose_net* net, int keep);
int rtpose_net_read_output(rtpose_net* net, int which, float* dst_nchw,
                           void* stream);
/* In-place view of the final PAF (which=0, 38 ch) / heat-map (which=1, 19 ch)
 * so the post-processing reads them where the last conv wrote them. */
int rtpose_net_output_view(const rtpose_net* net, int which, const float** base,
                           rtpose_layout* layout, int* C, int* H, int* W);
/* The same for any stage output, numbered as rtpose_net_read_output numbers them (rtpose_vgg: 0..11 =
 * saved_for_loss order): where the maps are right now - in the stage records under keep_intermediates,
 * else where the stage's last launch left them, which only the last stages' still are (RTPOSE_E_STATE for
 * the others).  rtpose_stage_mse (section 4b) reads the loss terms off these views. */
int rtpose_net_stage_view(const rtpose_net* net, int which, const float** base,
                          rtpose_layout* layout, int* C, int* H, int* W);
/* Per-layer HIP-event timing of the next forwards (bench.py roofline leg). */
int rtpose_net_set_profiling(rtpose_net* net, int enable);
int rtpose_net_num_launches(const rtpose_net* net);
/* After the stream has been synchronised: milliseconds of launch i of the
 * LAST forward, its conv kernel size (0 = not a conv), and algorithmic flops. */
int rtpose_net_launch_info(rtpose_net* net, int i, float* ms, int* k,
                           double* flops, char* name, int name_cap);
/* Matrix-core flops launch i actually ISSUES (padded channels / columns included; the Winograd
 * forms issue 16/36 resp. 70/196 of the direct sum's), and whether it runs in Winograd form:
 * algorithmic flops / time can exceed the MFMA peak, executed flops / time cannot. */
int rtpose_net_launch_executed_flops(const rtpose_net* net, int i, double* flops,
                                     int* winograd);

/* ------------------------------------------------------------------------
 * 3a. The OpenPose_Model network (lib/network/openpose.py:114-210): the same VGG19 trunk with PReLU on
 *     conv4_2, conv4_3_CPM and conv4_4_CPM, then `l2_stages` PAF stages and `l1_stages` heat-map stages of
 *     five dense blocks (three 3x3 conv + PReLU, outputs concatenated) and a 1x1 PReLU + 1x1 linear head.
 *
 *   OpenPose_Model(l2, l1, paf, heat) -> rtpose_openpose_create + rtpose_net_load_conv x114
 *                                        + rtpose_net_load_prelu x99
 *   OpenPose_Model.forward            -> rtpose_net_forward   (openpose.py:160-177)
 *
 * The handle is an rtpose_net: bind, load_conv, finalize_weights, conv_numerics, profiling, launch_info,
 * launch_executed_flops, device_status, output_view and the output guard work on it unchanged.  Conv index
 * order == the reference module's state_dict order, names are its prefixes ("feature_extractor.21",
 * "l2_stages.0.Mconv1_0.Mconv", "l1_stages.1.Mconv7").  fp32 only.
 *   rtpose_net_read_output(which): saved_for_loss flattened - the l2_stages PAF maps, then the l1_stages
 *     heat maps; only the last of each survive a forward unless keep_intermediates was set.
 *   rtpose_net_output_view(0 / 1): the last PAF / heat map, where the last stage heads wrote them.
 * ---------------------------------------------------------------------- */
typedef struct rtpose_openpose_options {
  uint32_t struct_bytes; /* sizeof(rtpose_openpose_options) of the caller          */
  int32_t l2_stages;     /* PAF stages, >= 2                                       */
  int32_t l1_stages;     /* heat-map stages, >= 2                                  */
  int32_t paf_channels;  /* 1..64                                                  */
  int32_t heat_channels; /* 1..64                                                  */
  int32_t winograd3;     /* as rtpose_net_options.winograd3                        */
  float amp_limit;       /* as rtpose_net_options.amp_limit                        */
} rtpose_openpose_options;
int rtpose_openpose_create(int N, int H, int W, const rtpose_openpose_options* opt, rtpose_net** out);
/* Slopes (device float[cout]) of the nn.PReLU that follows conv `idx`; RTPOSE_E_INVAL for a conv without one. */
int rtpose_net_load_prelu(rtpose_net* net, int idx, const float* slope, void* stream);
/* Host-only: 1 if conv `idx` is followed by a PReLU (its state_dict prefix, e.g. "feature_extractor.22" or
 * "l2_stages.0.Mconv1_0.MPrelu", goes to `name`), 0 if not, negative on a bad index. */
int rtpose_net_prelu_info(const rtpose_net* net, int idx, char* name, int name_cap);

/* ------------------------------------------------------------------------
 * 3a'. The stacked hourglass (lib/network/rtpose_hourglass.py), a third topology of the same executor:
 *   hg(num_stacks, num_blocks, paf_classes, ht_classes) -> rtpose_hourglass_create + rtpose_net_load_conv per conv
 *                                                          + rtpose_net_load_preact per Bottleneck
 *   HourglassNet.forward (eval)                         -> rtpose_net_forward   (rtpose_hourglass.py:162-189)
 *
 * The handle is an rtpose_net, as above.  fp32 only, inference only.  H and W must be multiples of 64: the sizes the
 * reference itself accepts (`out = up1 + up2`, rtpose_hourglass.py:85, fails for any other).  Conv index order == the
 * order of the nn.Conv2d in the reference's state_dict: "conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.0.conv3",
 * "layer1.0.downsample.0", ..., "hg.3.hg.2.1.0.conv3", ..., "res.0.0.conv1", "fc.0.0", "score_ht.0", "score_paf.0",
 * "fc_.0", "paf_score_.0", "ht_score_.0" (393 for hg(8, 1, 38, 19)).
 * BatchNorm2d (running statistics; scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale) enters
 * through the host in two ways:
 *   - a BatchNorm that FOLLOWS a conv (bn2 after conv1, bn3 after conv2, fc.i.1 after fc.i.0, bn1 after the stem) is
 *     folded into that conv: rtpose_net_load_conv gets w * scale[cout] and b * scale + shift, and the conv runs with a ReLU;
 *   - `bn1` of a Bottleneck precedes its conv1 and follows a residual sum several modules read: its (scale, shift) go to
 *     rtpose_net_load_preact of that conv1 and are applied where the conv stages its input (rtpose_conv_desc.in_scale).
 *   rtpose_net_preact_info names that BatchNorm ("layer1.0.bn1"), as rtpose_net_prelu_info names a PReLU.
 * rtpose_net_read_output(which): 0 = score_paf, 1 = score_ht of the LAST stack (what forward returns), at stride 4;
 *   2 + 2 s / 3 + 2 s = score_paf / score_ht of stack s, kept only under keep_intermediates.
 * rtpose_net_output_view(0 / 1): the last stack's maps in place.
 * ---------------------------------------------------------------------- */
typedef struct rtpose_hourglass_options {
  uint32_t struct_bytes; /* sizeof(rtpose_hourglass_options) of the caller         */
  int32_t num_stacks;    /* 1..64                                                  */
  int32_t num_blocks;    /* Bottlenecks per residual module, 1..16                 */
  int32_t paf_classes;   /* 1..64                                                  */
  int32_t ht_classes;    /* 1..64                                                  */
  int32_t winograd3;     /* as rtpose_net_options.winograd3 (the 3x3 conv2 of every Bottleneck) */
  float amp_limit;       /* as rtpose_net_options.amp_limit                        */
} rtpose_hourglass_options;
int rtpose_hourglass_create(int N, int H, int W, const rtpose_hourglass_options* opt, rtpose_net** out);
/* (scale, shift) (device float[cin] each) of the BatchNorm2d + ReLU in front of conv `idx`; RTPOSE_E_INVAL for a conv
 * without one. */
int rtpose_net_load_preact(rtpose_net* net, int idx, const float* scale, const float* shift, void* stream);
/* Host-only: 1 if conv `idx` reads its input through a BatchNorm2d + ReLU (the BatchNorm's state_dict prefix goes to
 * `name`), 0 if not, negative on a bad index. */
int rtpose_net_preact_info(const rtpose_net* net, int idx, char* name, int name_cap);

/* ------------------------------------------------------------------------
 * 3b. The ShuffleNetV2 x1.0 pose network (lib/network/rtpose_shufflenetV2.py:80-148,
 *     BASELINE config 4).  Same ownership rules as rtpose_net.  The host folds eval-mode
 *     BatchNorm into each conv and loads layers in rtpose_shufflenet_layer_info order
 *     (names are the reference state_dict prefixes, e.g. "network.3.0.conv0.1").
 * ---------------------------------------------------------------------- */
typedef struct rtpose_shufflenet rtpose_shufflenet;
int rtpose_shufflenet_create(int N, int H, int W, rtpose_shufflenet** out);
/* dtype: RTPOSE_DTYPE_F32 or RTPOSE_DTYPE_BF16 (bf16 activations + pointwise weights, fp32
 * accumulate; depthwise / stem weights and all biases stay fp32; outputs fp32) */
int rtpose_shufflenet_create_ex(int N, int H, int W, int dtype, rtpose_shufflenet** out);
void rtpose_shufflenet_destroy(rtpose_shufflenet* net);
size_t rtpose_shufflenet_workspace_bytes(const rtpose_shufflenet* net);
size_t rtpose_shufflenet_weight_bytes(const rtpose_shufflenet* net);
int rtpose_shufflenet_bind(rtpose_shufflenet* net, void* workspace, size_t workspace_bytes,
                           void* weights, size_t weight_bytes, int zero_workspace, void* stream);
int rtpose_shufflenet_num_layers(const rtpose_shufflenet* net);
/* kind: 0 = input affine (w = scale[3], b = shift[3]), 1 = stem conv [24,3,3,3],
 * 2 = depthwise [C,1,3,3], 3 = pointwise [cout,cin,1,1] */
int rtpose_shufflenet_layer_info(const rtpose_shufflenet* net, int idx, char* name, int name_cap,
                                 int* kind, int* cout, int* cin);
int rtpose_shufflenet_load(rtpose_shufflenet* net, int idx, const float* w, const float* b,
                           void* stream);
int rtpose_shufflenet_forward(rtpose_shufflenet* net, const float* x_nchw, void* stream);
/* which: 0 = PAF (38), 1 = heat-map (19) */
int rtpose_shufflenet_read_output(rtpose_shufflenet* net, int which, float* dst_nchw, void* stream);
int rtpose_shufflenet_output_view(const rtpose_shufflenet* net, int which, const float** base,
                                  rtpose_layout* layout, int* C, int* H, int* W);
int rtpose_shufflenet_set_profiling(rtpose_shufflenet* net, int enable);
int rtpose_shufflenet_num_launches(const rtpose_shufflenet* net);
int rtpose_shufflenet_launch_info(rtpose_shufflenet* net, int i, float* ms, double* flops, char* name,
                                  int name_cap);

/* ------------------------------------------------------------------------
 * 4. Batched pose decoding on the device
 *    stands in for lib/utils/paf_to_pose.py:372-406 (paf_to_pose_cpp):
 *      NMS            paf_to_pose.py:67-145   (find_peaks :25-38)
 *      process_paf    lib/pafprocess/pafprocess.cpp:22-194
 * ---------------------------------------------------------------------- */
/* Fused image prep on the device (caller side of get_outputs, evaluate/coco_eval.py:87-94):
 * uint8 BGR HWC image (device) -> cv2.resize(fx=fy=im_scale, INTER_LINEAR, 11-bit fixed point) ->
 * zero pad to Hn x Wn -> rtpose (mode 0) / vgg (mode 1) normalisation -> image n_index of an
 * NHWC8 layout buffer (e.g. rtpose_net_input_view).  hr x wr = cvRound(h0*s) x cvRound(w0*s). */
int rtpose_preprocess_u8(const unsigned char* img_bgr, int h0, int w0, double im_scale, int mode,
                         float* dst, const rtpose_layout* ldst, int n_index, int Hn, int Wn, int hr,
                         int wr, void* stream);

/* A whole bucket of images in ONE launch: `images` is a HOST array of `count` descriptors (they
 * travel as kernel arguments, 64 per launch; nothing is allocated or copied), every image has its
 * own source size, scale, valid size and destination slot; all share the padded size Hn x Wn of
 * the destination (the evaluation driver buckets images by it, evaluate/coco_eval.py:258-272). */
typedef struct rtpose_prep_image {
  const void* img_bgr; /* device, uint8 [h0][w0][3]                               */
  double im_scale;     /* crop_with_factor's im_scale (im_transform.py:124)       */
  int32_t h0, w0;      /* source size                                             */
  int32_t hr, wr;      /* cvRound(h0 * im_scale), cvRound(w0 * im_scale)          */
  int32_t flip;        /* != 0: x-mirrored inside the valid width (flip TTA pass) */
  int32_t n_index;     /* image slot of the destination layout                    */
} rtpose_prep_image;
int rtpose_preprocess_u8_batch(const rtpose_prep_image* images, int count, int mode, float* dst,
                               const rtpose_layout* ldst, int Hn, int Wn, void* stream);

/* Same, with flip != 0 writing the x-mirrored RESIZED image (columns [0, wr) mirrored, the
 * zero padding stays on the right): the second pass of flip test-time augmentation. */
int rtpose_preprocess_u8_flip(const unsigned char* img_bgr, int h0, int w0, double im_scale, int mode,
                              float* dst, const rtpose_layout* ldst, int n_index, int Hn, int Wn, int hr,
                              int wr, int flip, void* stream);

/* Multi-scale test-time augmentation (BASELINE config 3; the scale set is NOT pinned by
 * the reference tree - SURVEY.md §3.2): dst = beta*dst + alpha*bilinear_resize(src), dense
 * NHWC, half-pixel centres, edge clamp.  Only the top-left src_h_valid x src_w_valid
 * (fractional) region of src is mapped onto dst, so the zero padding of a scaled input
 * (im_transform.py:128-132) is cropped away on the fly. */
int rtpose_resize_bilinear_accum(const float* src, int hs, int ws, float* dst, int hd, int wd,
                                 int C, int N, float src_h_valid, float src_w_valid,
                                 float alpha, float beta, void* stream);

/* One scale of batched multi-scale (+flip) TTA, fused: heat/paf are the network's own output
 * views (rtpose_net_output_view) of a batch of 2B images - [0,B) normal, [B,2B) mirrored
 * (B images if flip == 0).  Forms the handle_paf_and_heat average (coco_eval.py:197-242;
 * mirror inside the first w_valid columns) and accumulates
 *   acc = beta * acc + alpha * bilinear_resize(average)   (dense [B,hd,wd,19] / [B,hd,wd,38])
 * exactly as rtpose_flip_merge followed by rtpose_resize_bilinear_accum would.  This is
 * rtpose_tta_accumulate_skel (section 5a) over COCO-18's table, with that entry's argument
 * check: NULL pointers or layouts, w_valid outside 1..ws or hs above the views' hs, a view
 * that addresses fewer than 19 / 38 channels (cstride - choff) are refused before any
 * launch.  Unlike it, B == 0 is refused too.  The kernel's grid is (row pieces, hd, B):
 * B or hd above 65535, or wd above 0x7fffff00 / 57 pixels, are refused (a 65536-row map
 * is a 524288-pixel-tall image at stride 8). */
int rtpose_tta_accumulate(const float* heat, const rtpose_layout* lheat, const float* paf,
                          const rtpose_layout* lpaf, int B, int hs, int w_valid, float* acc_heat,
                          float* acc_paf, int hd, int wd, float src_h_valid, float src_w_valid,
                          float alpha, float beta, int flip, void* stream);

#define RTPOSE_NUM_PART 18
#define RTPOSE_NUM_LIMB 19

typedef struct rtpose_decode_cfg {
  int32_t num_keypoints;  /* cfg.MODEL.NUM_KEYPOINTS (18)   default.py:40  */
  int32_t upsample;       /* cfg.MODEL.DOWNSAMPLE   (8)     default.py:41  */
  float thresh_heatmap;   /* cfg.TEST.THRESH_HEATMAP (0.1)  default.py:126 */
  int32_t max_peaks_per_part; /* device table capacity per (image, part)   */
  int32_t max_humans;         /* device table capacity per image           */
} rtpose_decode_cfg;

/* One decoded peak: paf_to_pose.py:141-142 row (x, y, score, id). */
typedef struct rtpose_peak {
  int32_t x, y; /* refined, at upsampled (input) resolution                */
  float score;
  int32_t id;   /* running counter over parts then peaks (pafprocess cid)  */
} rtpose_peak;

/* Bytes of the caller-provided device scratch + result block for N images. */
size_t rtpose_decode_workspace_bytes(const rtpose_decode_cfg* cfg, int N);
/* Bytes of the compact result record block (device or host copy of it). */
size_t rtpose_decode_result_bytes(const rtpose_decode_cfg* cfg, int N);

/* Enqueue NMS + refine + PAF scoring + assignment + grouping for N images.
 * heat: 19-channel (>= num_keypoints used) map, paf: 38-channel map, any
 * layout (dense HWC = lead 0, ws = w, hs = h, cstride = C).
 * `result` (device, rtpose_decode_result_bytes) receives, per image:
 *   int32 header[8]: n_peaks, n_humans, overflow_flags, max_peaks_per_part, max_humans (the
 *                    capacities the record is laid out for: a block describes itself), 0...
 *   int32 part_count[18]
 *   rtpose_peak peaks[18 * max_peaks_per_part]   (grouped by part, cid order)
 *   int32 human_parts[max_humans][18]            (cid, -1 = absent)
 *   float human_score[max_humans]                (get_score, cpp:204-206)
 */
int rtpose_decode_batch(const float* heat, const rtpose_layout* lheat,
                        const float* paf, const rtpose_layout* lpaf, int N,
                        int h, int w, const rtpose_decode_cfg* cfg,
                        void* workspace, size_t workspace_bytes, void* result,
                        void* stream);

/* Stage-wise entry points (same kernels, for tests and the legacy API).      */
/* NMS only (paf_to_pose.py:67-145): fills part_count + peaks of `result`.    */
int rtpose_nms_batch(const float* heat, const rtpose_layout* lheat, int N,
                     int h, int w, const rtpose_decode_cfg* cfg, void* result,
                     void* stream);

/* The two optional branches of NMS (lib/utils/paf_to_pose.py:67; neither is enabled by
 * the reference's own callers): RTPOSE_NMS_GAUSSIAN = bool_gaussian_filt=True — the x8
 * patch is smoothed with scipy.ndimage.gaussian_filter(sigma=3) before the arg-max
 * (:121-122); RTPOSE_NMS_NO_REFINE = bool_refine_center=False — no patch, the peak is
 * the cell centre (c + 0.5) * up - 0.5 with the low-resolution map value as score
 * (:135-139); rtpose_peak.x / .y then hold that coordinate truncated to int, which is
 * what process_paf makes of the joint_list column (pafprocess.cpp:28-29). */
#define RTPOSE_NMS_NO_REFINE 1
#define RTPOSE_NMS_GAUSSIAN 2
int rtpose_nms_batch_ex(const float* heat, const rtpose_layout* lheat, int N,
                        int h, int w, const rtpose_decode_cfg* cfg, int nms_flags,
                        void* result, void* stream);
int rtpose_decode_batch_ex(const float* heat, const rtpose_layout* lheat,
                           const float* paf, const rtpose_layout* lpaf, int N,
                           int h, int w, const rtpose_decode_cfg* cfg,
                           int nms_flags, void* workspace,
                           size_t workspace_bytes, void* result, void* stream);
/* The 25 normalised float64 weights RTPOSE_NMS_GAUSSIAN correlates with
 * (scipy _gaussian_kernel1d(sigma=3, radius=12)); returns 25, or < 0. */
int rtpose_gaussian_kernel1d(double* weights, int cap);

/* ---- 4a. The same decoder with the skeleton as data ---------------------------------
 * The entry points above decode COCO-18 maps (18 parts, 19 limbs over 38 PAF channels:
 * the library's own COCO-18 table).  The `_skel` entry points below run the same kernels
 * and so the same algorithm - NMS and the bicubic patch refine, the ten-sample PAF score with its two
 * thresholds, the score-sorted greedy assignment (std::sort replayed on an exact tie),
 * subset-row grouping and merging (cid 0 reads as absent; a person needs at least 4 parts
 * and a score ratio of at least 0.3) - over a table the caller passes:
 *   limb l joins part limb_part[l][0] (A) to limb_part[l][1] (B); its field is PAF
 *   channel limb_paf[l][0] (x) and limb_paf[l][1] (y); the limbs are walked in table
 *   order; bit l of seed_mask: a connection of limb l that matches no person starts one
 *   (the reference's `pair_id < 18` is 0x3FFFF for COCO-18).
 * The struct travels by value into the kernels as a launch argument: nothing is uploaded,
 * two streams may decode different skeletons at the same time.
 *
 * Record of the _skel entry points, per image (P = num_parts, L = num_limbs):
 *   int32 header[8]: n_peaks, n_humans, overflow_flags, max_peaks_per_part, max_humans,
 *                    P, L, 0   (the entry points above leave words 5 and 6 zero: a
 *                    record with 0 there is a COCO-18 record, 18 / 19)
 *   int32 part_count[P]                          at word 8
 *   rtpose_peak peaks[P * max_peaks_per_part]    at word max(32, round_up(8 + P, 4)):
 *                                                any P up to 24 lays out as above
 *   int32 human_parts[max_humans][P]             (cid, -1 = absent)
 *   float human_score[max_humans]
 * and the whole rounded up to 4 words.  A block describes itself: P, L and both capacities
 * are in its header.  With rtpose_skeleton_coco18 the record equals the one of
 * rtpose_decode_batch_ex word for word except header words 5 and 6.
 *
 * Flip merge and multi-scale TTA take the skeleton's left / right permutation as a
 * rtpose_flip_table (section 5: rtpose_flip_merge_skel / rtpose_tta_accumulate_skel).
 * Not covered by a skeleton (COCO-18 only): the legacy process_paf API of section 6. */
#define RTPOSE_SKEL_MAX_PARTS 32
#define RTPOSE_SKEL_MAX_LIMBS 32 /* 64 PAF channels: the limit of the native models */

typedef struct rtpose_skeleton {
  uint32_t struct_bytes;      /* sizeof(rtpose_skeleton)                            */
  int32_t num_parts;          /* P, 1..32 (the heat map has at least P channels)    */
  int32_t num_limbs;          /* L, 1..32                                           */
  int32_t limb_part[RTPOSE_SKEL_MAX_LIMBS][2]; /* (part A, part B)                  */
  int32_t limb_paf[RTPOSE_SKEL_MAX_LIMBS][2];  /* (PAF x channel, PAF y channel)    */
  uint32_t seed_mask;         /* bit l: limb l may start a person                   */
} rtpose_skeleton;

/* Presets.  COCO-18: the tables of lib/pafprocess/pafprocess.h:16-24.
 * BODY_25: 25 parts (heat-map channel 25 is background), 26 limbs over 52 PAF channels,
 * every limb may seed; the tables were written from memory of upstream OpenPose's
 * poseParameters.cpp and are NOT VERIFIED against CMU's weights.  The grouping run over
 * them is this library's (the tf-pose pafprocess algorithm), not OpenPose's own. */
int rtpose_skeleton_coco18(rtpose_skeleton* skel);
int rtpose_skeleton_body25(rtpose_skeleton* skel);

/* Host only.  0, or an error whose message names the limb: a part index outside
 * [0, num_parts) or a PAF channel outside [0, paf_channels); a limb with A == B; the same
 * (A, B) limb twice; x channel == y channel; num_parts / num_limbs outside 1..32 or more
 * parts than heat_channels; seed bits at or above num_limbs; a wrong struct_bytes. */
int rtpose_skeleton_check(const rtpose_skeleton* skel, int heat_channels, int paf_channels);

/* Sizes for N images; 0 on a bad cfg / skeleton.  cfg->num_keypoints must be in
 * 1..num_parts (parts at or above it keep empty peak lists). */
size_t rtpose_decode_workspace_bytes_skel(const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel, int N);
size_t rtpose_decode_result_bytes_skel(const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel, int N);

int rtpose_nms_batch_skel(const float* heat, const rtpose_layout* lheat, int N, int h, int w,
                          const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel,
                          int nms_flags, void* result, void* stream);
/* The skeleton is checked against the channels the two views can address
 * (cstride - choff) before anything is launched. */
int rtpose_decode_batch_skel(const float* heat, const rtpose_layout* lheat, const float* paf,
                             const rtpose_layout* lpaf, int N, int h, int w,
                             const rtpose_decode_cfg* cfg, const rtpose_skeleton* skel,
                             int nms_flags, void* workspace, size_t workspace_bytes,
                             void* result, void* stream);

/* ---- 4b. The way back: people -> heat-map / PAF targets, and the stage loss terms ------
 * stands in for lib/datasets/datasets.py:259-308 (CocoKeypoints.get_ground_truth) with
 * lib/datasets/heatmap.py:20-36 (putGaussianMaps) and lib/datasets/paf.py:18-68 (putVecMaps), for any
 * skeleton and a batch of images, and for one term of train/train_VGG19.py:143-174 (get_loss).
 *
 * h = input_h / stride, w = input_w / stride (integer division, datasets.py:261-262).  A part is
 * present iff v > 0.5 and 0 <= x < input_w and 0 <= y < input_h (remove_illegal_joint, :216-225).
 * Heat channel j at cell (y, x): cell centre gx = x * stride + (stride / 2.0 - 0.5), gy likewise; for
 * each person in order e = ((gx - cx)^2 + (gy - cy)^2) / 2.0 / sigma / sigma (three divisions in that
 * order); exp(-e) is added iff e <= 4.6052 and the running sum clipped to 1.  background != 0: heat
 * channel num_parts = max(1 - max over the parts, 0).  Heat channels behind those are written as 0.
 * Limb l = (A, B, chx, chy), for each person in order with both parts present: a = A / stride,
 * b = B / stride, v = b - a, n = sqrt(vx vx + vy vy); n == 0 skips the person; u = v / n; the box is
 * x0 = max(int(rint(min(ax, bx) - 1)), 0), x1 = min(int(rint(max(ax, bx) + 1)), w) (rint: half to
 * even, Python's round), y likewise; a cell is in the mask iff it lies in [x0, x1) x [y0, y1) and
 * |(x - ax) uy - (y - ay) ux| < 1; then for EVERY cell of the map acc = acc * count, acc += mask ? u : 0,
 * count += mask, acc = acc / max(count, 1) - the reference's running average, which re-rounds a cell
 * outside the box by * count / count (paf.py:56-66).  acc_x goes to channel chx, acc_y to chy; PAF
 * channels no limb names are written as 0; a channel two limbs name belongs to the first of them.
 * All of it in fp64, operation for operation in the reference's order, rounded to fp32 at the store:
 * every decision (e <= 4.6052, |cross| < 1, the half-even box) is the reference's, the PAF values are
 * its bits, the heat values are within 1 fp32 ulp (exp).  Not the reference's: np.linalg.norm may use a
 * fused multiply-add inside BLAS's dot; n here is the unfused sqrt(vx vx + vy vy).
 *
 * The skeleton travels by value into the kernels as a launch argument; nothing is uploaded.  People are
 * summed in people order whatever the launch geometry (no atomics): an image encodes to the same bits
 * alone and inside a batch.  The raster kernel walks an image's people through LDS in chunks of
 * RTPOSE_ENCODE_CHUNK records; max_people has no cap but the grid limit below. */
#define RTPOSE_ENCODE_CHUNK 16

typedef struct rtpose_encode_cfg {
  uint32_t struct_bytes;     /* sizeof(rtpose_encode_cfg)                                        */
  int32_t input_h, input_w;  /* network input size in pixels (reference: input_y, input_x)       */
  int32_t stride;            /* 8 for rtpose_vgg / OpenPose_Model, 4 for the hourglass           */
  double sigma;              /* reference: 7.0 (input pixels)                                    */
  int32_t background;        /* != 0: heat channel num_parts = max(1 - max over parts, 0)        */
  int32_t reserved;          /* 0                                                                */
} rtpose_encode_cfg;

/* Bytes of the caller-provided device workspace (the per-person records); 0 on a bad cfg, skeleton or count. */
size_t rtpose_encode_workspace_bytes(const rtpose_encode_cfg* cfg, const rtpose_skeleton* skel, int N,
                                     int max_people);
/* keypoints: device fp64 [N][max_people][num_parts][3] = (x, y, v) in input pixels; n_people: device
 * int32 [N] (clamped to 0..max_people) or NULL = max_people everywhere; heat / paf: dense
 * [N][h][w][heat_channels] / [N][h][w][paf_channels], EVERY element is written.  N == 0 is a no-op.
 * Refused before any launch, the message naming the argument: NULL pointers; a wrong struct_bytes; a
 * skeleton that fails rtpose_skeleton_check for these channel counts; more than 33 heat-map or 64 PAF
 * channels; background != 0 with heat_channels <= num_parts; stride < 1; sigma not greater than 0; an empty
 * grid; N or h above 65535, or N * max_people * (num_parts + num_limbs) above 0x7fffff00 (grid limits);
 * a workspace smaller than the query reports. */
int rtpose_encode_targets_skel(const double* keypoints, const int32_t* n_people, int N, int max_people,
                               const rtpose_encode_cfg* cfg, const rtpose_skeleton* skel,
                               int heat_channels, int paf_channels, float* heat, float* paf,
                               void* workspace, size_t workspace_bytes, void* stream);

/* nn.MSELoss(reduction='mean') of one stage output against a target (train_VGG19.py:147, :156-157):
 * `pred` is read in place through its padded-NHWC view (rtpose_net_stage_view / rtpose_net_output_view),
 * `target` is dense NHWC [N][h][w][channels].  Both operands are widened to fp64 before the subtraction,
 * squares and sums are fp64: per-block partials, then one block adds them in a fixed order and writes
 * fp32(sum / (N h w channels)) to *loss_out (device).  No atomics: the same bits on every run.
 * `partials`: device fp64 workspace of at least rtpose_stage_mse_partials(N, h, w, channels) elements
 * (0 = sizes out of range: any below 1, or more than 0x7fffff00 elements).  Refused before any launch:
 * NULL pointers, channels > cstride - choff, a map larger than the view, partial_count too small. */
size_t rtpose_stage_mse_partials(int N, int h, int w, int channels);
int rtpose_stage_mse(const float* pred, const rtpose_layout* lpred, const float* target, int N, int h,
                     int w, int channels, double* partials, size_t partial_count, float* loss_out,
                     void* stream);

/* ---- 4c. Training-batch augmentation: flip, rescale, crop, pad, normalise, mask -----------
 * stands in for the image side of the preprocess chain of train/train_VGG19.py:124-130
 * (RandomApply(HFlip), RescaleRelative, Crop, CenterPad of lib/datasets/transforms.py), for
 * image_transform (ToTensor + ImageNet Normalize) and for utils.mask_valid_area
 * (lib/datasets/utils.py:36-54): uint8 RGB sources in, the network's 3-channel fp32 input out, the
 * reference's bits.  The random draws and the annotation side are host work (augment.py); the
 * caller passes their results per image.
 *
 * RescaleRelative is Pillow's Image.resize((wr, hr), BICUBIC) on 8-bit RGB (ImagingResample).  Per axis
 * with `in` pixels in and `out` pixels out, in float64 with every operation unfused:
 *   scale = in / out, filterscale = max(scale, 1.0), support = 2.0 * filterscale,
 *   ksize = int(ceil(support)) * 2 + 1; for output xx: center = (xx + 0.5) * scale, ss = 1.0 / filterscale,
 *   xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) - xmin
 *   (int() truncates), w[x] = bicubic((x + xmin - center + 0.5) * ss) for x < xmax with a = -0.5:
 *   |t| < 1: ((a + 2) t - (a + 3)) t t + 1, |t| < 2: (((t - 5) t + 8) t - 4) a, else 0; ww = the sum of
 *   w[x] in index order, w[x] /= ww if ww != 0; k[x] = int(0.5 + w[x] * 2^22), int(-0.5 + w[x] * 2^22)
 *   for w[x] < 0.
 * The horizontal pass runs first and only if wr != w0, the vertical pass on its uint8 result and only
 * if hr != h0; each output is clip(((1 << 21) + sum pixel * k) >> 22, 0, 255) per channel (arithmetic
 * shift); an axis whose size does not change is copied, not filtered.  hflip mirrors the SOURCE before
 * the resize (a mirrored resize is not a resized mirror: xmin truncates).
 * Crop takes the window [crop_x, crop_x + min(out_w, wr - crop_x)) of the resized image, CenterPad puts
 * it at left = (out_w - width) / 2 (integer division) of the canvas and fills the rest with `fill`;
 * y likewise.  norm == 1: (float(u) / 255.0f - mean) / std per channel, mean (0.485, 0.456, 0.406),
 * std (0.229, 0.224, 0.225) as fp32, every fp32 operation correctly rounded and unfused; the fill is
 * normalised like a pixel.  Last, canvas pixels outside mask = [x0, x1) x [y0, y1) are exactly 0.0f.
 *
 * Every element of the three channels of every named slot is written; nothing else of dst is touched
 * (not the other channels, the gaps of a padded layout, or unnamed slots).  No atomics: an image gives
 * the same bits alone and inside a batch.  `images` is a HOST array whose entries travel as kernel
 * arguments in chunks, as in rtpose_preprocess_u8_batch: the library allocates and copies nothing.  Per
 * chunk: one launch tabulates both axes of every image's crop window into the workspace (at most
 * out_w + out_h entries per image), one fused launch does the rest; the horizontal pass's result
 * lives in LDS only. */
#define RTPOSE_AUG_MAX_TAPS 17 /* ksize at factor 0.25; smaller factors are refused */

typedef struct rtpose_augment_image {
  const void* img_rgb;    /* device uint8 [h0][w0][3], RGB                                   */
  int32_t h0, w0;         /* source size                                                      */
  int32_t hr, wr;         /* size after RescaleRelative: int(h0 * f), int(w0 * f)             */
  int32_t hflip;          /* != 0: source mirrored before the resize                          */
  int32_t crop_x, crop_y; /* Crop's offsets in the resized image                              */
  int32_t mask[4];        /* x0, y0, x1, y1: canvas pixels outside [x0,x1) x [y0,y1) are 0    */
  int32_t n_index;        /* destination slot                                                 */
} rtpose_augment_image;

typedef struct rtpose_augment_cfg {
  uint32_t struct_bytes; /* sizeof(rtpose_augment_cfg)                                        */
  int32_t out_h, out_w;  /* the canvas (Crop's long_edge == CenterPad's target)               */
  int32_t norm;          /* 0: float(u) in 0..255; 1: ToTensor + ImageNet mean/std            */
  int32_t nchw;          /* 0: dst through the rtpose_layout (3 channels from choff);
                            1: dense [N][3][out_h][out_w] (ldst is not read)                  */
  uint8_t fill[4];       /* CenterPad's fill, (124, 116, 104, 0)                              */
} rtpose_augment_cfg;

/* Bytes of the caller-provided device workspace (the tables) for `count` images; 0 on a bad cfg or a
 * negative count. */
size_t rtpose_augment_workspace_bytes(const rtpose_augment_cfg* cfg, int count);
/* The table above for outputs [first, first + count) of one axis, made on the device in fp64 by the
 * device function the batch call uses: bounds[i] = (xmin, xmax), coeffs[i][x] = k[x], 0 for x >= xmax
 * (both device int32).  Refused: NULL pointers, sizes below 1, a ksize above RTPOSE_AUG_MAX_TAPS, a
 * range outside [0, out_size].  count == 0 is a no-op. */
int rtpose_resample_table(int in_size, int out_size, int first, int count, int32_t* bounds,
                          int32_t* coeffs, void* stream);
/* Refused before any launch, the message naming the argument and for an image its index: NULL pointers
 * (ldst only when nchw == 0); a wrong struct_bytes; norm or nchw outside {0, 1}; a canvas side outside
 * [1, 65535]; h0, w0, hr or wr below 1; a ksize above RTPOSE_AUG_MAX_TAPS on either axis; crop_x
 * outside [0, max(wr - out_w, 0)], crop_y likewise; a mask outside the canvas or with x0 > x1, y
 * likewise; n_index outside [0, 65535]; with nchw == 0 a ldst with fewer than 3 channels from choff or
 * a view smaller than the canvas; a workspace smaller than the query reports.  count == 0 is a no-op. */
int rtpose_augment_batch(const rtpose_augment_image* images, int count, const rtpose_augment_cfg* cfg,
                         float* dst, const rtpose_layout* ldst, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- 4d. Colour jitter of the padded canvas: ColorJitter, RandomGrayscale, normalise, mask ----
 * stands in for image_transform_train of lib/datasets/transforms.py:53-65 but for its JPEG step, which
 * is section 4e:
 * torchvision's ColorJitter and RandomGrayscale on the 8-bit RGB PIL image CenterPad left (the canvas,
 * fill included), then ToTensor + ImageNet Normalize and utils.mask_valid_area.  On a PIL image every
 * one of these operations is integer, fp32 or fp64 arithmetic inside Pillow (ImageEnhance, Image.blend,
 * convert('L' / 'HSV' / 'RGB')); it is restated here operation for operation.  The random draws are
 * host work (augment.py); the caller passes their results per image.  JPEG re-compression
 * (RandomApply([jpeg], p=0.1)) sits between ColorJitter and RandomGrayscale and is not pointwise: it is
 * rtpose_jpeg_roundtrip_batch of section 4e, between one call here with gray = 0, norm = 0 and a
 * whole-canvas mask and a second one with an empty order (augment.py: color_jitter(jpeg=True)).
 *
 * `src` is dense fp32 [N][3][h][w] holding the integers 0..255 - what rtpose_augment_batch writes with
 * norm == 0, nchw == 1 and a whole-canvas mask.  A value v is read as u = (int)v clamped to 0..255,
 * NaN -> 0.  Per image, on the uint8 (r, g, b) of every canvas pixel, the operations of `order` in turn:
 *   L(r, g, b) = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16          (convert('L'))
 *   blend(d, x, alpha): t = float(d) + alpha * (float(x) - float(d)), three fp32 operations, unfused and
 *     correctly rounded; 0 <= alpha <= 1: (uint8)(int)t (truncating); otherwise 0 if t <= 0, 255 if
 *     t >= 255, else (int)t                                                   (ImagingBlend)
 *   0 brightness: blend(0, x, factor[0]) per channel
 *   1 contrast:   blend(m, x, factor[1]) per channel, m = int(sum_L / (h * w) + 0.5) in fp64, sum_L the
 *                 integer sum of L over the whole canvas (fill included, the mask ignored) as it stands
 *                 when contrast's turn comes, i.e. after the operations before it in `order`
 *   2 saturation: blend(L(r, g, b), x, factor[2]) per channel
 *   3 hue:        convert('HSV'), H = (H + hue_shift) mod 256, convert('RGB') - always, a shift of 0
 *                 still takes the lossy round trip:
 *     RGB -> HSV: maxc, minc the largest and smallest channel; V = maxc; minc == maxc: H = S = 0; else in
 *       fp32 cr = maxc - minc, s = cr / maxc, rc = (maxc - r) / cr, gc, bc likewise; r == maxc:
 *       h = bc - gc in fp32; else g == maxc: h = 2.0 + rc - bc in fp64; else h = 4.0 + gc - rc in fp64;
 *       h rounded to fp32; h = fmod(h / 6.0 + 1.0, 1.0) in fp64, rounded to fp32;
 *       H = clip8((int)(h * 255.0)), S = clip8((int)(s * 255.0)), the products in fp64.
 *     HSV -> RGB: S == 0: grey V; else in fp64 hf = float(H) * 6.0 / 255.0, i = floor(hf),
 *       f = (float)(hf - i), fs = (float)(S / 255.0); p = round(V * (1.0 - fs)),
 *       q = round(V * (1.0 - fs * f)) with the product fs * f in fp32,
 *       t = round(V * (1.0 - fs * (1.0 - f))), round = C's half away from zero, each clipped to 0..255;
 *       i % 6 = 0: (V, t, p), 1: (q, V, p), 2: (p, V, t), 3: (p, q, V), 4: (t, p, V), 5: (V, p, q).
 * then, if `gray`, r = g = b = L(r, g, b) (RandomGrayscale), then norm and mask as in 4c: norm == 1:
 * (float(u) / 255.0f - mean) / std, norm == 0: float(u); exactly 0.0f outside the mask.
 *
 * dst, ldst, norm and nchw mean what they mean in rtpose_augment_batch: every element of the three
 * channels of every named destination slot is written and nothing else.  dst == src is allowed where
 * nchw == 1 and every image has n_dst == n_src (in place; no two images may then name the same slot),
 * and refused otherwise.
 * Launches, per chunk of images (they travel by value as kernel arguments; the library allocates and
 * copies nothing): the L-sum pass, over the images that have contrast only, applies the operations before
 * contrast on the fly and writes one uint32 partial per slab of RTPOSE_JITTER_SLAB * ceil(h * w /
 * (RTPOSE_JITTER_SLAB * 1024)) pixels into the workspace; the apply pass adds an image's partials in
 * uint64 and applies the whole chain per pixel.  Integer sums, no atomics: an image gives the same bits
 * alone and inside any batch. */
#define RTPOSE_JITTER_SLAB 2048

typedef struct rtpose_jitter_image {
  int32_t order[4];     /* operations in the order applied: 0 brightness, 1 contrast, 2 saturation,
                           3 hue; -1 = slot unused; an operation may appear at most once             */
  float factor[3];      /* brightness, contrast, saturation: Pillow's alpha, (float)python_factor    */
  int32_t hue_shift;    /* 0..255, added to H modulo 256                                              */
  int32_t gray;         /* != 0: RandomGrayscale fired                                                */
  int32_t mask[4];      /* as rtpose_augment_image.mask                                               */
  int32_t n_src, n_dst; /* source and destination slots                                               */
} rtpose_jitter_image;

typedef struct rtpose_jitter_cfg {
  uint32_t struct_bytes; /* sizeof(rtpose_jitter_cfg)                                                 */
  int32_t h, w;          /* the canvas                                                                */
  int32_t norm, nchw;    /* as in rtpose_augment_cfg                                                  */
} rtpose_jitter_cfg;

/* Bytes of the caller-provided device workspace (the slab partials) for `count` images; 0 on a bad cfg
 * or a negative count. */
size_t rtpose_jitter_workspace_bytes(const rtpose_jitter_cfg* cfg, int count);
/* Refused before any launch, the message naming the argument and for an image its index: NULL pointers
 * (ldst only when nchw == 0); a wrong struct_bytes; norm or nchw outside {0, 1}; h or w outside
 * [1, 65535]; an order entry outside {-1, 0..3} or an operation twice; a factor that is not finite or
 * is negative; hue_shift outside 0..255; a mask outside the canvas or with x0 > x1, y likewise; n_src
 * or n_dst outside [0, 65535]; with nchw == 0 a ldst with fewer than 3 channels from choff or a view
 * smaller than the canvas; dst == src unless in place as above; a workspace smaller than the query
 * reports.  count == 0 is a no-op. */
int rtpose_jitter_batch(const rtpose_jitter_image* images, int count, const rtpose_jitter_cfg* cfg,
                        const float* src, float* dst, const rtpose_layout* ldst, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- 4e. JPEG re-compression of the padded canvas: save at a quality, re-open ----
 * stands in for RandomApply([jpeg_compression_augmentation], p=0.1) of lib/datasets/transforms.py:28-31,
 * 58-61: Image.save(f, 'jpeg', quality=q) and Image.open(f) on the 8-bit RGB canvas, the step of
 * image_transform_train between ColorJitter and RandomGrayscale.  Huffman coding is lossless: the
 * pixels that come back depend only on integer arithmetic, restated here from libjpeg-turbo (default
 * 4:2:0 sampling, JDCT_ISLOW, fancy up-sampling) - a Pillow built on another libjpeg may give other
 * bits.  `>>` is an arithmetic shift, D(x, n) = (x + (1 << (n - 1))) >> n.
 *
 * `src` and `dst` are dense fp32 [N][3][h][w] holding the integers 0..255 (a source value is read as in
 * 4d); image i is read from slot n_src and written to slot n_dst.  Per image:
 *   RGB -> YCbCr:  Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *                  Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *                  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   edges: the last column of the full-resolution planes repeats out to the MCU width (a multiple of
 *     16); the last row repeats once if h is odd; chroma is down-sampled; then each plane's own last
 *     row repeats to the MCU height (for chroma that is not the average of Y's repeated rows).
 *   chroma down-sampling: (a + b + c + d + bias) >> 2 over each 2 x 2 cell, bias 1 at even output
 *     columns and 2 at odd ones.
 *   quantiser tables: the luminance and chrominance tables of the JPEG specification's Annex K, scaled
 *     by s = 5000 / quality (integer) below quality 50, else 200 - 2 * quality: an entry is
 *     (base * s + 50) / 100 clamped to 1..255.
 *   forward DCT (jfdctint) on sample - 128 per 8 x 8 block, rows then columns, constants at 13 bits
 *     (2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172): row pass outputs 0 and 4
 *     << 2, the others D(.., 11); column pass outputs 0 and 4 D(.., 2), the others D(.., 15).
 *   quantise and de-quantise: a = (|c| + (Q * 8 >> 1)) / (Q * 8), the sign restored, times Q.
 *   inverse DCT (jidctint): columns with D(.., 11), the even part from (in0 +- in4) << 13; rows with
 *     D(.., 18); then the range-limit table as a function of that x: with i = x & 1023, i + 128 for
 *     i < 128, 255 for i < 512, 0 for i < 896, else i - 896 (x + 128 clamped to 0..255 for x in
 *     [-512, 511], a wrap beyond).
 *   up-sampling, on the real chroma plane of ceil(h / 2) x ceil(w / 2) samples (h2v2_fancy_upsample):
 *     vertically s = 3 * near + far, far the row above for even output rows and the row below for odd
 *     ones; horizontally (3 s[x] + s[x - 1] + 8) >> 4 at even output columns and
 *     (3 s[x] + s[x + 1] + 7) >> 4 at odd ones; a neighbour outside the real plane is the sample
 *     itself.  Where that plane is at most 2 samples wide (w <= 4) libjpeg replicates each chroma sample
 *     over its 2 x 2 cell instead (h2v2_upsample), and so does this: every w from 1 is served.
 *   YCbCr -> RGB with cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16),
 *     G = Y + ((-22554 cb + 32768 - 46802 cr) >> 16), B = Y + ((116130 cb + 32768) >> 16), each
 *     clamped to 0..255 and stored as float(u).
 *
 * Launches, per chunk of 32 images (they and the two tables travel by value as kernel arguments; the
 * library allocates and copies nothing): the codec pass, a block per run of 4 MCUs, stores the decoder's
 * 8-bit Y (h rows of w rounded up to 8 bytes), Cb and Cr (ceil(h / 2) rows of ceil(w / 2) rounded up to
 * 8 bytes) planes of image i at workspace + i * (those three sizes); the up-sample pass reads them - the
 * chroma filter reaches across MCU borders - and writes dst.  Every codec launch of a call precedes its
 * first up-sample launch on the stream, so all images are read before any is written: dst == src is
 * allowed where every image has n_dst == n_src (in place).  No atomics, no order to keep: an image gives
 * the same bits alone and inside any batch. */
typedef struct rtpose_jpeg_image {
  int32_t n_src, n_dst; /* source and destination slots                                               */
} rtpose_jpeg_image;

typedef struct rtpose_jpeg_cfg {
  uint32_t struct_bytes; /* sizeof(rtpose_jpeg_cfg)                                                   */
  int32_t h, w;          /* the canvas                                                                */
  int32_t quality;       /* 1..100, libjpeg's scale; the reference saves at 50                        */
} rtpose_jpeg_cfg;

/* Bytes of the caller-provided device workspace (the decoded planes) for `count` images; 0 on a bad cfg
 * or a negative count. */
size_t rtpose_jpeg_workspace_bytes(const rtpose_jpeg_cfg* cfg, int count);
/* Refused before any launch, the message naming the argument and for an image its index: NULL pointers;
 * a wrong struct_bytes; quality outside [1, 100]; h or w outside [1, 65535]; a negative count; a
 * workspace not aligned to 8 bytes; n_src or n_dst outside [0, 65535]; an n_dst that appears twice;
 * dst == src with an image whose n_dst != n_src; dst != src with the span of images written
 * overlapping the span of images read in memory (two views of one tensor: stricter than the launch
 * order needs, and cheap to tell); a workspace smaller than the query reports.  count == 0 is a no-op. */
int rtpose_jpeg_roundtrip_batch(const rtpose_jpeg_image* images, int count, const rtpose_jpeg_cfg* cfg,
                                const float* src, float* dst, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ---- 4f. Decoding baseline JPEG files into training sources ----
 * stands in for lib/datasets/datasets.py:171-172, Image.open(f).convert('RGB') of CocoKeypoints.__getitem__:
 * the bytes of a file -> the dense uint8 [h][w][3] RGB image that section 4c takes as a source, in the bits
 * of Pillow on libjpeg-turbo (JDCT_ISLOW, fancy up-sampling).  Two stages: the host reads the markers and
 * the Huffman-coded scan into quantised coefficients (csrc/jpeg_entropy.cpp: plain C++, no device, no state,
 * callable from any thread); the device de-quantises, runs the inverse DCT, up-samples and converts
 * (csrc/jpeg_decode.hip).  D(x, n) and `>>` as in 4e.
 *
 * Served: SOF0 (baseline sequential Huffman) frames of 8-bit precision with 8-bit quantiser tables and one
 * scan that interleaves all components; one component sampled 1 x 1 (gray), or three components - read as
 * Y, Cb, Cr - with chroma sampled 1 x 1 and luma 1 x 1 (4:4:4), 2 x 1 (4:2:2), 2 x 2 (4:2:0) or 1 x 2
 * (4:4:0, h x v); width and height 1..16384.  0xFF fill bytes, stuffed FF 00, APPn / COM and other
 * segments with a length are skipped; several DQT / DHT segments and tables redefined before SOS are
 * followed; with DRI, each RSTn resets the DC predictors and its number is checked.
 *
 * Refused, by a reason code (RTPOSE_JPEG_R_*, positive; rtpose_jpeg_reason_text gives its sentence), never
 * by a crash and never with a partial result a caller may use: anything that is not a JPEG file or whose
 * segments are malformed (SYNTAX: a length below 2, a table or frame segment of the wrong size, a Huffman
 * table whose codes do not fit their lengths or whose DC symbols exceed 15, a quantiser entry of 0, ...);
 * SOF1..SOF15, DAC and JPG markers (FRAME: extended, progressive, lossless, differential, arithmetic) and
 * a scan whose spectral selection is not 0..63 or whose approximation is not 0; precision other than 8
 * (PRECISION); 16-bit quantiser tables (QTABLE16); component counts other than 1 and 3 (COMPONENTS); an
 * APP14 segment that begins "Adobe" (ADOBE) and the component ids 'R', 'G', 'B' (COLORSPACE) - either
 * makes libjpeg choose another colour transform; any other sampling (SAMPLING); a scan that does not
 * list the frame's components in the frame's order, or a second SOS behind the first scan (SCANS); a DNL
 * marker or a height of 0 (DNL); a width or height of 0 or above 16384 (SIZE); a DC category above 11 or
 * an AC size above 10 (CATEGORY); a zero run that passes coefficient 63 (RUN); a code in no table (CODE); a
 * table selector never defined (TABLE); a missing, misplaced or wrongly numbered RSTn (RST); data that
 * ends, or runs into a marker, before the last MCU, or that lacks the EOI marker (TRUNCATED); whole bytes
 * other than fill bytes and EOI behind the last MCU (TRAILING); `capacity` below coef_count (CAPACITY);
 * and any coefficient - the accumulated DC value included - whose product with its quantiser entry lies
 * outside int16 (RANGE): libjpeg-turbo's SIMD inverse DCT multiplies in 16 bits and its C code does not,
 * so outside that range "libjpeg's bits" is not one thing; inside it no int32 sum of the device's passes
 * can overflow.  libjpeg pads a truncated scan with zeros and warns; this refuses.  Refusing too much is
 * safe: the caller decodes a refused file elsewhere (augment.decode_jpegs: Pillow).
 *
 * Coefficients: int16, quantised as the file holds them (the device multiplies).  Component c occupies
 * blocks_y[c] x blocks_x[c] blocks (the MCU grid times its sampling factors, so padded to whole MCUs) in
 * raster order from coef + coef_offset[c], 64 words per block in natural order (row-major: word 8 r + k is
 * row r, column k of the block; the file's zig-zag order is undone).  coef_count is their sum.  `qtab`
 * receives each component's quantiser table in the same natural order (gray: all three rows the same).
 *
 * Up-sampling, on the real planes - component c has ceil(h * v_c / vmax) rows of ceil(w * h_c / hmax)
 * samples, the rest of its blocks is padding - with a neighbour outside the real plane standing for the
 * sample itself:
 *   4:2:0  h2v2_fancy_upsample and, where the chroma plane is at most 2 samples wide, box replication,
 *          exactly as in 4e.
 *   4:2:2  h2v1_fancy_upsample: (3 c[x] + c[x - 1] + 1) >> 2 at even output columns, (3 c[x] + c[x + 1] +
 *          2) >> 2 at odd ones (so the first and the last column of the up-sampled row are the sample
 *          itself); box replication where the chroma plane is at most 2 samples wide.
 *   4:4:0  h1v2_fancy_upsample: (3 c[y] + c[y - 1] + 1) >> 2 at even output rows, (3 c[y] + c[y + 1] + 2)
 *          >> 2 at odd ones; no width condition.
 *   4:4:4  none.   gray: Y into all three channels (convert('RGB') of an 'L' image).
 * Then 4e's YCbCr -> RGB expression, clamped to 0..255, stored as bytes. */
enum {
  RTPOSE_JPEG_GRAY = 0, RTPOSE_JPEG_444 = 1, RTPOSE_JPEG_422 = 2, RTPOSE_JPEG_420 = 3, RTPOSE_JPEG_440 = 4
};
enum {
  RTPOSE_JPEG_R_ARGUMENT = 1, RTPOSE_JPEG_R_NOT_JPEG = 2, RTPOSE_JPEG_R_SYNTAX = 3, RTPOSE_JPEG_R_TRUNCATED = 4,
  RTPOSE_JPEG_R_FRAME = 5, RTPOSE_JPEG_R_PRECISION = 6, RTPOSE_JPEG_R_QTABLE16 = 7, RTPOSE_JPEG_R_COMPONENTS = 8,
  RTPOSE_JPEG_R_ADOBE = 9, RTPOSE_JPEG_R_COLORSPACE = 10, RTPOSE_JPEG_R_SAMPLING = 11, RTPOSE_JPEG_R_SCANS = 12,
  RTPOSE_JPEG_R_DNL = 13, RTPOSE_JPEG_R_SIZE = 14, RTPOSE_JPEG_R_CATEGORY = 15, RTPOSE_JPEG_R_RUN = 16,
  RTPOSE_JPEG_R_CODE = 17, RTPOSE_JPEG_R_TABLE = 18, RTPOSE_JPEG_R_RST = 19, RTPOSE_JPEG_R_CAPACITY = 20,
  RTPOSE_JPEG_R_RANGE = 21, RTPOSE_JPEG_R_TRAILING = 22
};

typedef struct rtpose_jpeg_info {
  uint32_t struct_bytes;    /* sizeof(rtpose_jpeg_info), set by rtpose_jpeg_probe                        */
  int32_t width, height;
  int32_t components;       /* 1 or 3                                                                    */
  int32_t mode;             /* RTPOSE_JPEG_GRAY .. RTPOSE_JPEG_440                                       */
  int32_t hsamp[3], vsamp[3]; /* sampling factors                                                        */
  int32_t mcus_x, mcus_y;   /* the MCU grid: ceil(width / (8 hmax)) x ceil(height / (8 vmax))            */
  int32_t blocks_x[3], blocks_y[3]; /* per component: mcus_x * hsamp x mcus_y * vsamp                    */
  int32_t restart_interval; /* MCUs between RSTn markers, 0 = none                                       */
  int32_t reason;           /* 0 = served, else RTPOSE_JPEG_R_* (every other field is then 0)            */
  uint64_t coef_offset[3];  /* int16 words from the image's first coefficient to component c's           */
  uint64_t coef_count;      /* int16 words of the whole image: 64 * the sum of the block grids           */
} rtpose_jpeg_info;

/* Both walk host memory only, set no rtpose_last_error text and return 0 or the reason.  Probe reads the
 * markers up to and including the SOS header; the refusals that only the scan can show (CATEGORY, RUN, CODE,
 * RST, TRUNCATED, TRAILING, RANGE, a second scan) come from the decode.  The decode reads the file again
 * by itself and requires `info` to agree (ARGUMENT otherwise); it zero-fills and writes coef[0 ..
 * coef_count) - `capacity` is in words - and, on success only, qtab.  After a refusal coef holds no image. */
int rtpose_jpeg_probe(const void* data, size_t len, rtpose_jpeg_info* info);
int rtpose_jpeg_entropy_decode(const void* data, size_t len, const rtpose_jpeg_info* info, int16_t* coef,
                               size_t capacity, uint16_t qtab[3][64]);
const char* rtpose_jpeg_reason_text(int reason);

/* The device stage.  `coef` is one device buffer of coef_words int16 words, 16-byte aligned, that holds for
 * every image its coefficients (coef_count(width, height, mode) words from coef_offset, laid out as above)
 * and its three quantiser tables (192 uint16 words from qtab_offset, natural order); both offsets are
 * multiples of 8 words.  The tables travel in that buffer and not in the descriptor so that a chunk of 32
 * images stays a kernel argument of 2.5 KB (with three 64-entry tables each it would be 13 KB); a host
 * writes them in front of the image's coefficients and uploads both with one copy.  `dst` is the image: dense uint8 [height][width][3] device
 * memory, 4-byte aligned.  The library derives every grid, count and plane size from width, height and
 * mode; it allocates and copies nothing.
 *
 * Launches, per chunk of 32 images (descriptors by value): the IDCT pass - eight threads per block, 32
 * blocks per 256-thread workgroup, all blocks of all components of an image flattened; a thread loads one
 * 16-byte row of coefficients and of the table, multiplies, and the workgroup runs jidctint's column pass
 * D(.., 11), row pass D(.., 18) and the range limit of 4e through an int32 LDS tile - stores 8-bit planes
 * in the workspace, a component's rows padded to 8 bytes, blocks wholly outside the real plane left out;
 * the up-sample pass, a thread per run of 4 pixels, reads Y and chroma by the rules above and stores 12
 * bytes.  Every IDCT launch of a call precedes its first up-sample launch on the stream (the filters read
 * across block borders).  Integer arithmetic only, no atomics: an image gives the same bits alone and in
 * any batch. */
typedef struct rtpose_jpeg_decode_image {
  int32_t width, height;  /* 1..16384                                                                   */
  int32_t mode;           /* RTPOSE_JPEG_GRAY .. RTPOSE_JPEG_440                                        */
  int32_t reserved;       /* 0                                                                          */
  uint64_t coef_offset;   /* words into coef                                                            */
  uint64_t qtab_offset;   /* words into coef                                                            */
  void* dst;
} rtpose_jpeg_decode_image;

/* Bytes of the caller-provided device workspace (the decoded planes of all images); 0 on a bad argument. */
size_t rtpose_jpeg_decode_workspace_bytes(const rtpose_jpeg_decode_image* images, int count);
/* Refused before any launch, the message naming the argument and for an image its index: NULL pointers; a
 * negative count; width or height outside 1..16384; an unknown mode; a non-zero reserved; a coefficient or
 * table offset that is no multiple of 8 or whose range ends beyond coef_words; a coef not aligned to 16
 * bytes; a dst not aligned to 4 bytes; two destinations that overlap; a workspace that is not aligned to 8
 * bytes or smaller than the query reports.  count == 0 is a no-op. */
int rtpose_jpeg_decode_batch(const rtpose_jpeg_decode_image* images, int count, const int16_t* coef,
                             size_t coef_words, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * 5. Flip test-time-augmentation merge
 *    stands in for evaluate/coco_eval.py:197-242 (handle_paf_and_heat).
 *    All four inputs dense HWC fp32 on the device, outputs likewise.
 *    This is rtpose_flip_merge_skel (5a) over COCO-18's table: NULL maps are
 *    refused; a call without pixels (N, h or w == 0) is a no-op.  The kernel's
 *    grid is (row pieces, h, N): N or h above 65535, or w above
 *    0x7fffff00 / 57 pixels, are refused.
 * ---------------------------------------------------------------------- */
int rtpose_flip_merge(const float* heat, const float* heat_flipped,
                      const float* paf, const float* paf_flipped, int N, int h,
                      int w, float* heat_avg, float* paf_avg, void* stream);

/* ---- 5a. The same merge with the left / right permutation as data --------------------
 * One kernel pair serves every skeleton.  The `_skel` entry points below take the
 * permutation as a flip table: output heat-map channel c averages with channel
 * heat_src[c] of the x-mirrored pass, PAF channel c with channel paf_src[c], negated iff
 * bit c of paf_neg_mask is set.  rtpose_flip_merge and rtpose_tta_accumulate (section 4)
 * are these entry points over COCO-18's table, which the library derives once from
 * rtpose_skeleton_coco18 and the part mirror: same kernels, same argument check, same
 * bits.  The struct travels by value into the kernels as a launch argument (nothing is
 * uploaded; two streams may merge different skeletons at the same time). */
#define RTPOSE_FLIP_MAX_HEAT 33 /* 32 parts + background */
#define RTPOSE_FLIP_MAX_PAF 64

typedef struct rtpose_flip_table {
  uint32_t struct_bytes;   /* sizeof(rtpose_flip_table)                              */
  int32_t heat_channels;   /* 1..33: channels of the heat maps                        */
  int32_t paf_channels;    /* 1..64: channels of the PAF maps                         */
  uint32_t reserved;       /* 0                                                       */
  uint64_t paf_neg_mask;   /* bit c: PAF channel c takes its source negated           */
  uint8_t heat_src[RTPOSE_FLIP_MAX_HEAT];
  uint8_t paf_src[RTPOSE_FLIP_MAX_PAF];
} rtpose_flip_table;

/* Host only.  The table of a skeleton whose part i becomes part part_mirror[i] in the
 * mirrored image (num_parts entries); background != 0: the heat map carries one more
 * channel behind the parts, which reads itself.  Limb (A, B, cx, cy) looks up the limb
 * that joins part_mirror[A] and part_mirror[B]: found in that direction as (sx, sy), cx
 * reads -sx and cy reads +sy; found only as part_mirror[B] -> part_mirror[A], the vector
 * changes direction too: cx reads +sx and cy reads -sy.  A PAF channel no limb reads maps
 * to itself.  Errors: a skeleton that fails rtpose_skeleton_check for these channel counts;
 * a part_mirror that is not an involution over [0, num_parts); a limb whose mirror is in
 * the table neither way (the message names the limb); a channel that two limbs would give
 * different (source, sign) pairs. */
int rtpose_flip_table_from_skeleton(const rtpose_skeleton* skel, const int32_t* part_mirror,
                                    int background, int paf_channels, rtpose_flip_table* out);

/* Host only; for a table filled in by hand.  0, or an error: a wrong struct_bytes or a
 * channel count out of range; a source index outside the map; mask bits at or above
 * paf_channels; a table that applied twice is not the identity (src[src[c]] != c, or PAF
 * channels c and src[c] carrying different signs). */
int rtpose_flip_table_check(const rtpose_flip_table* table);

/* rtpose_flip_merge over a table: all maps dense NHWC fp32 on the device, the heat maps
 * with table->heat_channels and the PAF maps with table->paf_channels channels.  N == 0
 * is a no-op; NULL maps, a table that fails the check, N or h above 65535 are refused. */
int rtpose_flip_merge_skel(const float* heat, const float* heat_flipped, const float* paf,
                           const float* paf_flipped, int N, int h, int w, float* heat_avg,
                           float* paf_avg, const rtpose_flip_table* table, void* stream);

/* rtpose_tta_accumulate over a table: heat / paf are the network's own output views of a
 * batch of 2B images ([0,B) normal, [B,2B) mirrored; B images if flip == 0), the
 * accumulators dense [B,hd,wd,heat_channels] / [B,hd,wd,paf_channels].  Accumulates exactly
 * as rtpose_flip_merge_skel followed by rtpose_resize_bilinear_accum would.  B == 0 is a
 * no-op; refused before any launch: NULL pointers, w_valid outside 1..ws or hs above the
 * views' hs, a table with more channels than a view addresses (cstride - choff) or that
 * fails the check, B or hd above 65535. */
int rtpose_tta_accumulate_skel(const float* heat, const rtpose_layout* lheat, const float* paf,
                               const rtpose_layout* lpaf, int B, int hs, int w_valid,
                               float* acc_heat, float* acc_paf, int hd, int wd,
                               float src_h_valid, float src_w_valid, float alpha, float beta,
                               int flip, const rtpose_flip_table* table, void* stream);

/* ------------------------------------------------------------------------
 * 6. Legacy single-image API — same seven names and argument meaning as the
 *    SWIG module (lib/pafprocess/pafprocess.h:53-59, pafprocess.i:14-15).
 *    Host pointers in, results kept in process-global state until the next
 *    process_paf (pafprocess.cpp:12-13), guarded by a mutex.  The scoring /
 *    assignment / grouping run on the GPU; getters are bounds-checked and
 *    return -1 / NaN instead of the reference's undefined behaviour.
 * ---------------------------------------------------------------------- */
int process_paf(int p1, int p2, int p3, float* peaks, int h1, int h2, int h3,
                float* heatmap, int f1, int f2, int f3, float* pafmap);
int get_num_humans(void);
int get_part_cid(int human_id, int part_id);
float get_score(int human_id);
int get_part_x(int cid);
int get_part_y(int cid);
float get_part_score(int cid);

#ifdef __cplusplus
}
#endif
#endif /* RTPOSE_MI355X_H */
