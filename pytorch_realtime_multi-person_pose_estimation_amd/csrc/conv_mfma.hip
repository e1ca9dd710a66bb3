// fp32 implicit-GEMM convolution for gfx950 (MI355X), stride 1, "same" padding,
// k in {1,3,7}, fused bias (+ReLU) (+2x2 max-pool), or bias + per-channel PReLU (k = 1, 3: the
// nn.PReLU of lib/network/openpose.py:56-63; a separate instantiation, see ConvArgsP).
//
// Stands in for the nn.Conv2d / nn.ReLU / nn.MaxPool2d modules instantiated by
// lib/network/rtpose_vgg.py:23-35 and :49-55 (ATen kernels on the reference).
//
// Design (MI355X-first, not a translation of any CUDA kernel):
//  * GEMM view: M = output pixels, N = output channels, K = taps x channels.
//    Block tile 128(M) x 64(N), 4 wave64s as 2(M) x 2(N), each wave a 64 x 32
//    tile = two 32x32 accumulators of v_mfma_f32_32x32x2_f32 (exact fp32, the
//    only fp32-input matrix op on CDNA4; 64 cycles/instruction/SIMD).
//  * Activations use the shared-gap padded NHWC layout (include/rtpose_mi355x.h
//    §1): a stencil tap is a constant pixel offset, so the A operand is NOT an
//    im2col gather: per 16-channel chunk the block stages ONE halo of input
//    pixels in LDS and re-uses it for all k*k taps (49x re-use for 7x7).
//    LDS image is [channel/4][pixel][4 floats]; every A fragment read is one
//    conflict-free ds_read_b128 per lane (4 consecutive k for its k-half).
//  * The B operand (weights, pre-packed [chunk][tap][c/4][cout][4]) goes
//    straight from L2 to registers with a one-tap-deep register prefetch: a
//    wave reads 1 KiB contiguous per instruction, no LDS, no per-tap barrier.
//    One barrier per channel chunk (k*k*16 MFMAs per wave apart).
//  * The next chunk's halo is fetched one 16-byte piece per thread per tap
//    underneath the MFMAs and written to the other LDS buffer.
//  * Two tilings: MODE 0 "strip" = 128 consecutive pixels of the flattened
//    (n,y,x) space (no tile waste on the 46x46 maps: 32*46*46 = 529 * 128);
//    MODE 1 = TH x TW 2-D tiles inside one image for wide maps (bounded halo).
//  * 2 blocks per CU (launch bounds) so one block's chunk barrier / epilogue
//    hides under the other's MFMAs.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "conv_desc.h"
#include "launchers.h"
#include "mfma_dev.h"

namespace rtpose {

struct ConvGroup {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  Lay lin, lout;
  int cout, cout_pad;
  const int32_t* out_cmap;  // optional output-channel scatter (see rtpose_conv_desc)
};

// The fused ReLU.  kReluKeepsNan (rtpose_conv2d): torch's relu by a compare and a select - NaN stays NaN, +Inf stays +Inf,
// -Inf, negatives and -0 give +0.  kReluMax (the inference executor): max(v, 0), which returns the operand that is not NaN.
// Finite sums get the same bits from both.  `form` is wave-uniform.
constexpr int kReluMax = 1, kReluKeepsNan = 2;
__device__ __forceinline__ float relu_of(float v, int form) {
  return form == kReluKeepsNan ? (v <= 0.f ? 0.f : v) : fmaxf(v, 0.f);
}

struct ConvArgs {
  ConvGroup g[2];
  int N, H, W, M;     // output == input spatial size (before pooling)
  int cin;            // packed input channels
  int relu, pool;     // relu: 0, kReluMax or kReluKeepsNan
  int qs;             // LDS pixels per channel-group plane
  int hw_lds;         // MODE 1: LDS row stride of the halo (pixels)
  int tw_log2;        // MODE 1: log2(tile width); tile height = 128 >> tw_log2
  int tiles_x, tiles_y;
  int mtiles, ntiles, nbig;  // block-id decoding (see conv_mfma_f32)
  int ncombo, xcd_remap;
  int dephase_mode;          // 0 off (every launch: the stagger measured 0 %), 1: ids [n_cu, 2 n_cu), 2: odd ids
  int dephase_cycles, n_cu;  // start-up delay that puts the 2 blocks of a CU half a tile apart
};

// PReLU launches: the slopes of the two groups follow the arguments the other instantiations read, so those keep
// their argument offsets and instruction streams
struct ConvArgsP : ConvArgs {
  const float* prelu[2];  // float[cout] per group
};
template <bool PR>
using ConvArgsT = typename std::conditional<PR, ConvArgsP, ConvArgs>::type;

// Residual epilogue and input pre-activation (rtpose_conv_desc.residual / in_scale / in_shift; k = 1, one group): the
// pre-activation Bottleneck of the stacked hourglass.  A kernel of its own (conv_mfma_f32_x) with the operands behind the
// arguments the other instantiations read, for the same reason as ConvArgsP.
struct ConvX {
  const float* res;       // NULL: no residual
  Lay lres;
  const float* in_scale;  // NULL: no pre-activation; float[cin], 16-byte aligned
  const float* in_shift;
  int pre_cin;            // input channels >= pre_cin are staged as 0
};
struct ConvArgsX : ConvArgs {
  ConvX x;
};
// relu(scale * x + shift) of one 16-byte piece with `left` real channels from its first one: the others are staged as 0
// whatever the buffer and the vectors hold there (their filter taps are zero, and 0 * x has to be 0)
__device__ __forceinline__ float4 preact4(float4 v, const float4 sc, const float4 sh, const int left) {
  v.x = left > 0 ? fmaxf(sc.x * v.x + sh.x, 0.f) : 0.f;
  v.y = left > 1 ? fmaxf(sc.y * v.y + sh.y, 0.f) : 0.f;
  v.z = left > 2 ? fmaxf(sc.z * v.z + sh.z, 0.f) : 0.f;
  v.w = left > 3 ? fmaxf(sc.w * v.w + sh.w, 0.f) : 0.f;
  return v;
}

constexpr int kBM = 128;
// 1x1 convs: CK-channel sub-chunks per LDS buffer (see conv_tile; 4: -20 % on the 1x1 layers)
constexpr int kTB1x1 = 1;

template <int KS>
struct PiecesPerTap {
  static constexpr int value = (KS == 1) ? 6 : 1;
};

// m_local (0..127) -> (ty, tx) inside a 2-D tile.  2x2 quads are 4 consecutive
// m so that a fused max-pool is a max over 4 accumulator registers of one lane.
__device__ __forceinline__ void tile_local_yx(int ml, int tw_log2, int& ty, int& tx) {
  const int qi = ml >> 2;
  const int hw_log2 = tw_log2 - 1;  // quads per tile row
  ty = ((qi >> hw_log2) << 1) + ((ml >> 1) & 1);
  tx = ((qi & ((1 << hw_log2) - 1)) << 1) + (ml & 1);
}

// NBUF = 2: the next channel chunk's halo is fetched underneath the MFMAs into a second
//           LDS buffer (2 blocks per CU).
// NBUF = 1: one halo buffer, re-filled between chunks behind a barrier; half the LDS and
//           <= 128 VGPRs, so 4 blocks share a CU and hide each other's refills
//           (occupancy instead of software pipelining).
// MF = 32-row M fragments per wave: 2 = the normal 128-pixel block tile, 1 = a 64-pixel
// half tile used only for the last, partial wave of blocks of a strip-mode launch (tail
// quantisation: see plan_conv).
// NF = 32-column N fragments per wave: 1 -> block tile 128 x 64, 2 -> 128 x 128 (wave tile
// 64 x 64).  NF = 2 halves the B (weight) and A (LDS) operand bytes per MFMA; measured, the B
// loads cost ~4.6 % of the forward and half of them ~2 %.
// XT: the residual / pre-activation instantiation (KS = 1, NBUF = 1; X != nullptr)
template <int KS, int CK, int MODE, int NBUF, int MF, int NF, bool PR = false, bool XT = false>
__device__ __forceinline__ void conv_tile(const ConvArgs& A, const ConvGroup& g, const int m0_arg,
                                          const int ntile, float* smem, const float* prelu = nullptr,
                                          const ConvX* X = nullptr) {
  static_assert(!XT || (KS == 1 && NBUF == 1 && !PR), "residual / pre-activation: the single-buffered 1x1 kernel");
  constexpr int P = KS / 2;
  constexpr int BMT = 64 * MF;  // pixels per block tile
  constexpr int CG = CK / 4;  // 16-byte channel groups per chunk
  constexpr int G = CK / 8;   // 8-deep k groups per chunk (4 MFMAs each)
  constexpr int GB = G * NF;  // B registers (float4) per tap: [n-fragment][k-group]
  constexpr int PPT = PiecesPerTap<KS>::value;
  // 1x1 convs have no spatial taps to re-use a halo over.  The tap loop can instead walk
  // the channel axis: one LDS buffer holds TB consecutive CK-channel sub-chunks of the pixel
  // tile ([TB*CG planes][pixel][4]) and tap t multiplies sub-chunk t, with the k x k
  // machinery (B/A prefetch, next buffer staged under the MFMAs) unchanged.  Measured with
  // TB = 4 (double-buffered, 2 blocks/CU): SLOWER than TB = 1 single-buffered at 4 blocks/CU
  // (VGG 1x1 layers 1.27 vs 1.04 ms, ShuffleNetV2 pointwise 13.6 vs 12.7 ms): these GEMMs
  // are short (K = 24..512), so per-block prologue/epilogue latency dominates and is hidden
  // better by occupancy than by in-block pipelining.  TB stays a knob for a future
  // multi-tile (persistent) 1x1 kernel.
  constexpr int TB = (KS == 1) ? kTB1x1 : 1;
  constexpr int CGB = CG * TB;              // channel-group planes per LDS buffer
  constexpr int TAPS = (KS == 1) ? TB : KS; // taps per "row" of the tap loop
  constexpr int ROWS = (KS == 1) ? 1 : KS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int l31 = lane & 31, kh = lane >> 5;

  const int QS = A.qs;

  // ---- block -> tile -------------------------------------------------------
  int m0 = 0, n_img = 0, y0 = 0, x0 = 0;  // MODE 0 uses m0; MODE 1 uses the rest
  int q_origin, np_pix, row_lds;
  int qc0 = 0;
  if (MODE == 0) {
    m0 = m0_arg;
    const int HW = A.H * A.W;
    const int n = m0 / HW, r = m0 - n * HW;
    const int y = r / A.W, x = r - y * A.W;
    qc0 = g.lin.lead + (n * g.lin.hs + y) * g.lin.ws + x;
    int ml = min(m0 + BMT, A.M) - 1;
    const int n2 = ml / HW, r2 = ml - n2 * HW;
    const int y2 = r2 / A.W, x2 = r2 - y2 * A.W;
    const int qcl = g.lin.lead + (n2 * g.lin.hs + y2) * g.lin.ws + x2;
    q_origin = qc0 - P * g.lin.ws - P;
    np_pix = qcl + P * g.lin.ws + P - q_origin + 1;
    row_lds = g.lin.ws;
  } else {
    int b = m0_arg;  // MODE 1: the tile index
    const int txi = b % A.tiles_x;
    b /= A.tiles_x;
    const int tyi = b % A.tiles_y;
    n_img = b / A.tiles_y;
    const int TW = 1 << A.tw_log2, TH = kBM >> A.tw_log2;
    y0 = tyi * TH;
    x0 = txi * TW;
    q_origin = g.lin.lead + (n_img * g.lin.hs + y0 - P) * g.lin.ws + x0 - P;
    np_pix = (TH + 2 * P) * A.hw_lds;
    row_lds = A.hw_lds;
  }
  const int np_total = np_pix * CGB;  // 16-byte pieces per LDS buffer

  // ---- per-lane A fragment bases (LDS pixel index of this lane's row) ------
  int abase[MF];
  int an = 0, ay = 0, ax = 0;  // strip mode: coordinates of fragment 0's row, stepped by 32 pixels
  if (MODE == 0) {
    const int m = m0 + wm * (32 * MF) + l31;
    const int HW = A.H * A.W;
    an = m / HW;
    const int r = m - an * HW;
    ay = r / A.W;
    ax = r - ay * A.W;
  }
#pragma unroll
  for (int fm = 0; fm < MF; ++fm) {
    const int ml = wm * (32 * MF) + fm * 32 + l31;
    if (MODE == 0) {
      // rows past the end of the tensor (last strip) read the last real pixel's halo
      const bool past = m0 + ml > A.M - 1;
      const int n = past ? A.N - 1 : an, y = past ? A.H - 1 : ay, x = past ? A.W - 1 : ax;
      abase[fm] = g.lin.lead + (n * g.lin.hs + y) * g.lin.ws + x - qc0;
      ax += 32;
      while (ax >= A.W) {
        ax -= A.W;
        if (++ay >= A.H) {
          ay = 0;
          ++an;
        }
      }
    } else {
      int ty, tx;
      tile_local_yx(ml, A.tw_log2, ty, tx);
      abase[fm] = ty * A.hw_lds + tx;
    }
  }

  // ---- halo staging helpers -------------------------------------------------
  // A halo is staged as 16-byte pieces: piece idx = (pixel idx/CG, channel group idx%CG);
  // thread `tid` owns pieces tid, tid+256, ... ("sets").  LDS image: [group][pixel][4].
  const int in_cstride = g.lin.cstride, in_ws = g.lin.ws;
  const float* in_base = g.in + g.lin.choff;
  constexpr int PIXSET = 256 / CGB;             // halo pixels covered by one piece set
  const int pj = tid % CGB, ppix0 = tid / CGB;  // this thread's group and first pixel
  const unsigned hw_inv = MODE == 1 ? (65536u + A.hw_lds - 1) / A.hw_lds : 0u;
  // global float offset (from the chunk's first channel) and LDS float offset of piece
  // (set, tid).  MODE 0 may run past the halo (never past the buffer: layout slack);
  // the caller masks the LDS side.
  auto piece_goff = [&](int set) -> size_t {
    int pix = set * PIXSET + ppix0;
    int q;
    if (MODE == 0) {
      q = q_origin + pix;
    } else {
      pix = min(pix, np_pix - 1);
      const int hy = (int)(((unsigned)pix * hw_inv) >> 16), hx = pix - hy * A.hw_lds;
      q = q_origin + hy * in_ws + hx;
    }
    return (size_t)q * in_cstride + pj * 4;
  };
  // LDS offsets are kept in float4 units: the compiler then knows every access is
  // 16-byte aligned and emits ds_read_b128 / ds_write_b128 (with float offsets it fell
  // back to ds_read2_b32 pairs: 2x the instructions and 4-way bank conflicts)
  float4* smem4 = reinterpret_cast<float4*>(smem);
  const int buf4 = CGB * QS;  // float4 per halo buffer
  auto piece_loff = [&](int set) -> int { return pj * QS + set * PIXSET + ppix0; };
  // a thread with nothing to park writes its stale registers to a private dummy slot
  // behind the two buffers, so the park step needs no per-thread branch
  const int dummy_loff = NBUF * buf4 + tid;
  const int nsets = (np_total + 255) / 256;  // piece sets per chunk

  // ---- B operand pointers (advance one (chunk,tap) block per tap) ---------------
  const int nchunks = A.cin / CK;
  const int ncol = ntile * (kConvBN * NF) + wn * (32 * NF) + l31;  // column of n-fragment 0
  const float4* bq[GB];
#pragma unroll
  for (int fn = 0; fn < NF; ++fn)
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
      bq[fn * G + gi] = reinterpret_cast<const float4*>(g.w) + (size_t)(2 * gi + kh) * g.cout_pad + ncol + fn * 32;
  const size_t b_it_stride = (size_t)CG * g.cout_pad;  // float4 per (chunk,tap)

  // B lives in three register sets: the tap being multiplied, the next one, and the one
  // in flight from L2 (two taps of lead: one tap was not enough to cover L2 latency
  // under load - dropping the B loads was worth +7% on the 7x7 layers)
  float4 s0[GB], s1[GB], s2[GB];
#pragma unroll
  for (int gi = 0; gi < GB; ++gi) {
    s0[gi] = gload4(bq[gi]);
    bq[gi] += b_it_stride;
    s1[gi] = gload4(bq[gi]);
  }

  // ---- halo fill used by the prologue (NBUF 2) / before every chunk (NBUF 1) ------
  auto fill_halo = [&](const float* src, int ntaps) {  // ntaps: sub-chunks that exist in this buffer
    const bool ch_ok = pj < ntaps * CG;
    constexpr int FD = (KS == 1 && kTB1x1 > 1) ? 8 : 4;  // loads in flight per thread
    // pre-activation: this thread's pieces are 4 fixed channels of the chunk, so their scale / shift are fetched once per
    // chunk and applied between the load and the LDS write.  Gap pixels of a strip become relu(shift) in LDS: no A fragment
    // of a 1x1 conv reads them (a row of the product is one real pixel).
    float4 psc = make_float4(0.f, 0.f, 0.f, 0.f), psh = psc;
    int pc0 = 0;
    bool pre = false;
    if constexpr (XT) {
      pre = X->in_scale != nullptr;
      if (pre && ch_ok) {
        pc0 = (int)(src - in_base) + pj * 4;
        psc = gload4(X->in_scale + pc0);
        psh = gload4(X->in_shift + pc0);
        pc0 = X->pre_cin - pc0;  // real channels left from this piece's first one
      }
    }
    (void)pre;
    for (int set0 = 0; set0 < nsets; set0 += FD) {
      float4 t[FD];
#pragma unroll
      for (int u = 0; u < FD; ++u)
        if (ch_ok && set0 + u < nsets && (set0 + u) * 256 + tid < np_total) t[u] = gload4(src + piece_goff(set0 + u));
#pragma unroll
      for (int u = 0; u < FD; ++u)
        if (ch_ok && set0 + u < nsets && (set0 + u) * 256 + tid < np_total) {
          if constexpr (XT) {
            if (pre) t[u] = preact4(t[u], psc, psh, pc0);
          }
          smem4[piece_loff(set0 + u)] = t[u];
        }
    }
  };
  const int nbig = (nchunks + TB - 1) / TB;  // LDS buffer fills per block
  if (NBUF == 2) {
    fill_halo(in_base, min(TB, nchunks));
    __syncthreads();
  }
  // (NBUF 1, measured and rejected: issuing chunk c+1's loads before chunk c is multiplied and
  //  parking them afterwards - "load early / write late" - made the ShuffleNetV2 pointwise layers
  //  5-15 % SLOWER than the plain refill below with 4 blocks per CU hiding each other's latency.)

  // the bias is fetched now (at the epilogue its latency would be fully exposed) and rides in
  // the accumulator: every register of a lane belongs to the lane's output channel
  floatx16 acc[MF][NF];
#pragma unroll
  for (int fn = 0; fn < NF; ++fn) {
    const float b0 = g.bias[ncol + fn * 32];  // bias is padded to cout_pad
#pragma unroll
    for (int fm = 0; fm < MF; ++fm)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[fm][fn][r] = b0;
  }
  float slope[NF];  // PReLU: fetched with the bias, for the same reason
#pragma unroll
  for (int fn = 0; fn < NF; ++fn) {
    slope[fn] = 0.f;
    if constexpr (PR) slope[fn] = ncol + fn * 32 < g.cout ? prelu[ncol + fn * 32] : 0.f;
  }

  // LDS float4 offsets of this lane's A fragments inside a halo buffer: [k-group][m-frag]
  int afrag[G][MF];
#pragma unroll
  for (int gi = 0; gi < G; ++gi)
#pragma unroll
    for (int fm = 0; fm < MF; ++fm) afrag[gi][fm] = (2 * gi + kh) * QS + abase[fm];
  // float4 between consecutive taps' A fragments: one stencil row (k x k) or CG planes (1x1)
  const int rowstep = KS == 1 ? CG * QS : row_lds;

  // One tap = 8*G MFMAs with the loads for the NEXT tap threaded between them in a
  // fixed order: B straight from L2, A fragments from LDS (running row address +
  // immediate column offset), and - in the first rows of a chunk only (STAGE) - PPT
  // 16-byte pieces per thread of the next chunk's halo, parked in LDS one tap later.
  // A wave issues MFMAs back to back on its own and the VALU port stays nearly idle:
  // measured, every VALU instruction in this loop costs MFMA issue slots once two
  // waves share a SIMD (measured by dropping one load stream at a time).
  // B register (k-group) n is fetched after MFMA pair n < GB
  // memory clobber: loads/stores may not cross (IR + DAG); sched_barrier: nothing may
  // cross in the machine scheduler
#define RTPOSE_CONV_STEP(ACUR, ANXT, BCUR, BLOAD, KX, STAGE)                                   \
  {                                                                                            \
    _Pragma("unroll") for (int n = 0; n < 4 * G; ++n) {                                        \
      const int gi_ = n >> 2, j_ = n & 3;                                                      \
      _Pragma("unroll") for (int fn = 0; fn < NF; ++fn) {                                      \
        const float bv_[4] = {BCUR[fn * G + gi_].x, BCUR[fn * G + gi_].y, BCUR[fn * G + gi_].z, \
                              BCUR[fn * G + gi_].w};                                           \
        _Pragma("unroll") for (int fm = 0; fm < MF; ++fm) {                                    \
          const float av_[4] = {ACUR[gi_][fm].x, ACUR[gi_][fm].y, ACUR[gi_][fm].z, ACUR[gi_][fm].w}; \
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av_[j_], bv_[j_], acc[fm][fn], 0, 0, 0); \
        }                                                                                      \
      }                                                                                        \
      RTPOSE_PIN();                                                                            \
      if (n < GB) {                                                                            \
        bq[n] += b_it_stride;                                                                  \
        BLOAD[n] = gload4(bq[n]);                                                              \
      }                                                                                        \
      if (n == 1) {                                                                            \
        if (KS == 1 || (KX) == KS - 1) { /* next tap: next sub-chunk (1x1) / next stencil row */ \
          _Pragma("unroll") for (int g2 = 0; g2 < G; ++g2)                                     \
            _Pragma("unroll") for (int fm = 0; fm < MF; ++fm) arow[g2][fm] += rowstep;         \
        }                                                                                      \
        if (STAGE) {                                                                           \
          _Pragma("unroll") for (int p = 0; p < PPT; ++p) {                                    \
            smem4[hl[p]] = hv[p];                                                              \
            const int set = ps * PPT + p;                                                      \
            if (set < nsets) { /* uniform: sets past the halo are not fetched at all */        \
              hv[p] = gload4(next_base + piece_goff(set));                                     \
              hl[p] = (next_ch_ok && tid < np_total - set * 256) ? hn_off + piece_loff(set) : dummy_loff; \
            } else {                                                                           \
              hv[p] = make_float4(0.f, 0.f, 0.f, 0.f);                                         \
              hl[p] = dummy_loff;                                                              \
            }                                                                                  \
          }                                                                                    \
          ++ps;                                                                                \
        }                                                                                      \
      }                                                                                        \
      if (n >= 2 && n - 2 < G) {                                                               \
        _Pragma("unroll") for (int fm = 0; fm < MF; ++fm)                                      \
          ANXT[n - 2][fm] = smem4[arow[n - 2][fm] + ((KS > 1 && (KX) + 1 < KS) ? (KX) + 1 : 0)];   \
      }                                                                                        \
      RTPOSE_PIN();                                                                            \
    }                                                                                          \
  }
#define RTPOSE_CONV_ROW(STAGE)                                                  \
  {                                                                             \
    _Pragma("unroll") for (int kx = 0; kx < TAPS; ++kx) {                       \
      /* A sets alternate (kx & 1); B sets rotate (kx % 3): multiply s[kx%3],  */ \
      /* fill s[(kx+2)%3] with the tap two ahead                               */ \
      if (KS == 1 && kx >= nt) { /* short last buffer of a 1x1 conv */          \
      } else if (kx % 6 == 0) {                                                 \
        RTPOSE_CONV_STEP(a0, a1, s0, s2, kx, STAGE)                             \
      } else if (kx % 6 == 1) {                                                 \
        RTPOSE_CONV_STEP(a1, a0, s1, s0, kx, STAGE)                             \
      } else if (kx % 6 == 2) {                                                 \
        RTPOSE_CONV_STEP(a0, a1, s2, s1, kx, STAGE)                             \
      } else if (kx % 6 == 3) {                                                 \
        RTPOSE_CONV_STEP(a1, a0, s0, s2, kx, STAGE)                             \
      } else if (kx % 6 == 4) {                                                 \
        RTPOSE_CONV_STEP(a0, a1, s1, s0, kx, STAGE)                             \
      } else {                                                                  \
        RTPOSE_CONV_STEP(a1, a0, s2, s1, kx, STAGE)                             \
      }                                                                         \
    }                                                                           \
    /* re-normalise the register roles for the next row (a few v_mov per row) */ \
    if (TAPS & 1) {                                                             \
      _Pragma("unroll") for (int gi = 0; gi < G; ++gi)                          \
        _Pragma("unroll") for (int fm = 0; fm < MF; ++fm) a0[gi][fm] = a1[gi][fm]; \
    }                                                                           \
    _Pragma("unroll") for (int gi = 0; gi < GB; ++gi) {                         \
      if (TAPS % 3 == 1) {                                                      \
        const float4 t_ = s0[gi];                                               \
        s0[gi] = s1[gi];                                                        \
        s1[gi] = s2[gi];                                                        \
        s2[gi] = t_;                                                            \
      } else if (TAPS % 3 == 2) {                                               \
        const float4 t_ = s2[gi];                                               \
        s2[gi] = s1[gi];                                                        \
        s1[gi] = s0[gi];                                                        \
        s0[gi] = t_;                                                            \
      }                                                                         \
    }                                                                           \
  }

  // rows of a chunk whose taps carry the staging code: set s is fetched at tap s and
  // parked at tap s+1, so nsets+1 taps are needed (the host guarantees they exist)
  const int stage_rows = min(ROWS, (nsets + 1 + PPT * TAPS - 1) / (PPT * TAPS));
  float4 hv[PPT];
  int hl[PPT];
  for (int chunk = 0; chunk < nbig; ++chunk) {   // one LDS buffer (TB sub-chunks of CK channels) per turn
    const int nt = min(TB, nchunks - chunk * TB);  // taps that exist in this buffer (1x1 only: < TB at the end)
    (void)nt;
    if (NBUF == 1) {  // every wave is past the previous chunk (barrier at the loop end)
      fill_halo(in_base + (size_t)chunk * TB * CK, nt);
      __syncthreads();
    }
    const int hb_off = NBUF == 2 ? (chunk & 1) * buf4 : 0;
    const int hn_off = NBUF == 2 ? ((chunk + 1) & 1) * buf4 : 0;
    // the last chunk re-stages itself into the idle buffer (never read): no branch
    const int chunk_next = min(chunk + 1, nbig - 1);
    const float* next_base = in_base + (size_t)chunk_next * TB * CK;
    const bool next_ch_ok = pj < min(TB, nchunks - chunk_next * TB) * CG;
    (void)next_ch_ok;
    int ps = 0;
#pragma unroll
    for (int p = 0; p < PPT; ++p) {
      hv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      hl[p] = dummy_loff;
    }
    // running LDS addresses (float4 units) of this lane's fragments on the current stencil row
    int arow[G][MF];
    float4 a0[G][MF], a1[G][MF];
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
#pragma unroll
      for (int fm = 0; fm < MF; ++fm) {
        arow[gi][fm] = hb_off + afrag[gi][fm];
        a0[gi][fm] = smem4[arow[gi][fm]];  // tap (0,0)
      }
    int ky = 0;
    if (NBUF == 2)
      for (; ky < stage_rows; ++ky) RTPOSE_CONV_ROW(1)
    for (; ky < ROWS; ++ky) RTPOSE_CONV_ROW(0)
    if (NBUF == 2) {  // park whatever is still in flight, then publish the buffer
#pragma unroll
      for (int p = 0; p < PPT; ++p) smem4[hl[p]] = hv[p];
    }
    __syncthreads();
  }
#undef RTPOSE_CONV_ROW
#undef RTPOSE_CONV_STEP

  // ---- epilogue: bias (+ReLU) (+2x2 max-pool), masked stores -----------------
#pragma unroll
  for (int fn = 0; fn < NF; ++fn) {
  const int ncolf = ncol + fn * 32;
  const bool col_ok = ncolf < g.cout;
  float* out_base = g.out + ((g.out_cmap && col_ok) ? g.out_cmap[ncolf] : g.lout.choff + ncolf);
  if (!A.pool) {
    // strip mode: the lane's rows are m0 + wm*32*MF + 4*kh + {0,1,2,3, 8,9,10,11, 16,...}: pixel
    // coordinates by ONE division pair, then stepped (+1,+1,+1,+5 repeating).  An integer division
    // is ~40 VALU instructions; 32 of them per lane were longer than the whole tap loop of a
    // short-K 1x1 conv (ShuffleNetV2 pointwise: 8k MFMA cycles per block).
    int sn = 0, sy = 0, sx = 0;
    if (MODE == 0) {
      const int m = m0 + wm * (32 * MF) + 4 * kh;
      const int HW = A.H * A.W;
      sn = m / HW;
      const int r = m - sn * HW;
      sy = r / A.W;
      sx = r - sy * A.W;
    }
    auto step = [&](int d) {
      sx += d;
      while (sx >= A.W) {
        sx -= A.W;
        if (++sy >= A.H) {
          sy = 0;
          ++sn;
        }
      }
    };
    (void)step;
#pragma unroll
    for (int fm = 0; fm < MF; ++fm) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        // rows rg*8 + 4*kh + {0,1,2,3}
        const int ml0 = wm * (32 * MF) + fm * 32 + rg * 8 + 4 * kh;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int ml = ml0 + rr;
          int n, y, x;
          bool ok;
          if (MODE == 0) {
            ok = m0 + ml < A.M;
            n = sn;
            y = sy;
            x = sx;
            step(rr == 3 ? 5 : 1);  // (the walk restarts with every n-fragment)
          } else {
            int ty, tx;
            tile_local_yx(ml, A.tw_log2, ty, tx);
            n = n_img;
            y = y0 + ty;
            x = x0 + tx;
            ok = (y < A.H) && (x < A.W);
          }
          float v = acc[fm][fn][rg * 4 + rr];
          if (A.relu) v = relu_of(v, A.relu);
          if constexpr (PR) v = prelu1(v, slope[fn]);
          if (ok && col_ok) {
            if constexpr (XT) {
              // the residual element of this output element alone (it may be the element about to be overwritten)
              if (X->res)
                v += X->res[((size_t)X->lres.lead + (size_t)(n * X->lres.hs + y) * X->lres.ws + x) * X->lres.cstride +
                            X->lres.choff + ncolf];
            }
            const size_t q = (size_t)g.lout.lead + (size_t)(n * g.lout.hs + y) * g.lout.ws + x;
            out_base[q * g.lout.cstride] = v;
          }
        }
      }
    }
  } else {
    // MODE 1 only: quad = 4 consecutive m = 4 consecutive accumulator registers
    const int Ho = A.H >> 1, Wo = A.W >> 1;
    const int hw_log2 = A.tw_log2 - 1;
#pragma unroll
    for (int fm = 0; fm < MF; ++fm) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int ml0 = wm * (32 * MF) + fm * 32 + rg * 8 + 4 * kh;
        const int qi = ml0 >> 2;
        const int py = (y0 >> 1) + (qi >> hw_log2);
        const int px = (x0 >> 1) + (qi & ((1 << hw_log2) - 1));
        float v = fmaxf(fmaxf(acc[fm][fn][rg * 4 + 0], acc[fm][fn][rg * 4 + 1]),
                        fmaxf(acc[fm][fn][rg * 4 + 2], acc[fm][fn][rg * 4 + 3]));
        if (A.relu) v = relu_of(v, A.relu);
        if (py < Ho && px < Wo && col_ok) {
          const size_t q = (size_t)g.lout.lead + (size_t)(n_img * g.lout.hs + py) * g.lout.ws + px;
          out_base[q * g.lout.cstride] = v;
        }
      }
    }
  }
  }  // fn
}

// Kernel: 1-D grid, block id -> (group, N tile, M tile).
//  * XCD-aware order (xcd_remap): the dispatcher places block b on XCD b % 8 (observed; used
//    for speed only).  Ids are laid out so that the (group, N tile) combinations of ONE M tile
//    are consecutive slots of ONE XCD: they run together and share that tile's input halo in
//    the XCD's L2 instead of each re-reading it from MALL/HBM (8 N tiles x 1.75 halo overlap
//    = 14 reads of every input pixel of conv4_2 before this).
//  * MODE 0 (strip) tail: ids [0, nbig) are 128-pixel tiles; the rest are pairs of 64-pixel
//    halves of the remaining tiles, dispatched last (see plan in conv2d_launch).
template <int KS, int CK, int MODE, int NBUF, int NF, bool PR = false>
__global__ __launch_bounds__(256, NBUF == 1 ? 4 : 2) void conv_mfma_f32(const ConvArgsT<PR> A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int L = blockIdx.x;
  // Equal tiles keep the two co-resident blocks of a CU in lock step, so their prologues
  // (first halo fill, ~2 us of exposed latency) and epilogues coincide instead of hiding
  // under each other's MFMAs.  Half of the first wave of blocks starts half a tile late.
  if (A.dephase_mode && L < 2 * A.n_cu &&
      (A.dephase_mode == 1 ? L >= A.n_cu : (L & 1))) {
    const long long t0 = __builtin_readcyclecounter();
    while (__builtin_readcyclecounter() - t0 < A.dephase_cycles) __builtin_amdgcn_s_sleep(32);
  }
  const bool small = MODE == 0 && L >= A.nbig;
  const int bi = small ? A.nbig + ((L - A.nbig) >> 1) : L;
  int mt, c;
  if (A.xcd_remap) {
    const int xcd = bi & 7, j = bi >> 3;
    c = j % A.ncombo;
    mt = (j / A.ncombo) * 8 + xcd;
  } else {
    mt = bi % A.mtiles;
    c = bi / A.mtiles;
  }
  if (mt >= A.mtiles) return;  // padding ids of the remapped order
  const int nt = c % A.ntiles, grp = c / A.ntiles;
  const float* prelu = nullptr;
  if constexpr (PR) prelu = grp ? A.prelu[1] : A.prelu[0];
  if (MODE == 1) {
    conv_tile<KS, CK, MODE, NBUF, 2, NF, PR>(A, A.g[grp], mt, nt, smem, prelu);
  } else if (!small) {
    conv_tile<KS, CK, MODE, NBUF, 2, NF, PR>(A, A.g[grp], mt * kBM, nt, smem, prelu);
  } else {
    const int m0 = mt * kBM + ((L - A.nbig) & 1) * (kBM / 2);
    if (m0 < A.M) conv_tile<KS, CK, MODE, NBUF, 1, NF, PR>(A, A.g[grp], m0, nt, smem, prelu);
  }
}

// The residual / pre-activation 1x1 kernel: one group, no dephasing, the same id order as conv_mfma_f32.
template <int CK, int MODE>
__global__ __launch_bounds__(256, 4) void conv_mfma_f32_x(const ConvArgsX A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int L = blockIdx.x;
  const bool small = MODE == 0 && L >= A.nbig;
  const int bi = small ? A.nbig + ((L - A.nbig) >> 1) : L;
  int mt, nt;
  if (A.xcd_remap) {
    const int xcd = bi & 7, j = bi >> 3;
    nt = j % A.ncombo;
    mt = (j / A.ncombo) * 8 + xcd;
  } else {
    mt = bi % A.mtiles;
    nt = bi / A.mtiles;
  }
  if (mt >= A.mtiles) return;  // padding ids of the remapped order
  if (MODE == 1) {
    conv_tile<1, CK, MODE, 1, 2, 1, false, true>(A, A.g[0], mt, nt, smem, nullptr, &A.x);
  } else if (!small) {
    conv_tile<1, CK, MODE, 1, 2, 1, false, true>(A, A.g[0], mt * kBM, nt, smem, nullptr, &A.x);
  } else {
    const int m0 = mt * kBM + ((L - A.nbig) & 1) * (kBM / 2);
    if (m0 < A.M) conv_tile<1, CK, MODE, 1, 1, 1, false, true>(A, A.g[0], m0, nt, smem, nullptr, &A.x);
  }
}

// ---- weight packing -------------------------------------------------------------
// packed[chunk][tap][cg][cout_pad][4]  <-  w[cout][cin_src][k][k]
__global__ void pack_weights_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                    int cout, int cin_src, int k, const int32_t* __restrict__ cin_map,
                                    int cin_packed, int ck, int coutp, float* __restrict__ wp,
                                    float* __restrict__ bp) {
  const int T = k * k;
  const size_t total = (size_t)T * cin_packed * coutp;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)coutp) bp[i] = (i < (size_t)cout && bias) ? bias[i] : 0.f;
  if (i >= total) return;
  const int e = i & 3;
  size_t r = i >> 2;
  const int n = r % coutp;
  r /= coutp;
  const int cg = r % (ck / 4);
  r /= (ck / 4);
  const int tap = r % T;
  const int chunk = r / T;
  const int c = chunk * ck + cg * 4 + e;
  int src = cin_map ? cin_map[c] : (c < cin_src ? c : -1);
  float v = 0.f;
  if (n < cout && src >= 0 && src < cin_src) {
    const int ky = tap / k, kx = tap - ky * k;
    v = w[(((size_t)n * cin_src + src) * k + ky) * k + kx];
  }
  wp[i] = v;
}

// ---- host side --------------------------------------------------------------------
static int conv_ck(int cin) { return (cin % 16 == 0) ? 16 : 8; }

struct ConvPlan {
  int mode, ck, qs, hw_lds, tw_log2, tiles_x, tiles_y, grid_x, nbuf;
  size_t lds_bytes;
};

static int plan_conv(const rtpose_conv_desc& d, int N, int H, int W, ConvPlan* pl) {
  const int P = d.k / 2;
  pl->ck = conv_ck(d.cin);
  const int M = N * H * W;
  // piece sets per thread that fit the staging schedule (set s fetched at tap s, parked at s+1)
  const int max_pieces = (d.k == 1) ? PiecesPerTap<1>::value : d.k * d.k - 1;
  const int cg = (pl->ck / 4) * (d.k == 1 ? kTB1x1 : 1);  // channel-group planes per LDS buffer
  // 1x1 layers: single halo buffer, 4 blocks per CU (occupancy hides the refill latency of
  // these short-K GEMMs better than a second buffer: 42.7 vs 32.6 TF/s); k x k: double buffer
  pl->nbuf = d.k == 1 ? 1 : 2;
  // strips waste no MFMA work on tile edges but stage a longer halo than 2-D tiles on wide maps
  // (3x3 at W = 92: 2.4x the tile vs 1.4x, against 8.9 % edge waste); widest map that still strips:
  constexpr int strip_maxw = 128;  // measured: conv3_1..3 (92 x 92) 6.70 -> 6.33 ms as strips; 184 x 184: no change
  bool strip = (W <= strip_maxw) && !d.pool;
  if (strip) {
    const rtpose_layout& l = d.lin;
    const int lb = (kBM - 1) + ((kBM - 1) / W + 1) * (l.ws - W) +
                   ((kBM - 1) / (H * W) + 1) * (l.hs - H) * l.ws + 2 * P * l.ws + 2 * P + 1;
    const int qs = round_qs(lb);
    const size_t lds = (size_t)pl->nbuf * cg * qs * 16 + 256 * 16;  // + one dummy park slot per thread
    if ((pl->nbuf == 2 && ceil_div(qs * cg, 256) > max_pieces) || lds > 80 * 1024) strip = false;
    if (strip) {
      pl->mode = 0;
      pl->qs = qs;
      pl->hw_lds = 0;
      pl->tw_log2 = 0;
      pl->tiles_x = pl->tiles_y = 0;
      pl->grid_x = ceil_div(M, kBM);
      pl->lds_bytes = lds;
      return 0;
    }
  }
  // 2-D tiles: pick the tile width with the least padded work
  int best_tw = 0;
  long best_cost = -1;
  for (int twl = 2; twl <= 6; ++twl) {
    const int tw = 1 << twl, th = kBM >> twl;
    if (th < 2) continue;
    const long cost = (long)ceil_div(W, tw) * ceil_div(H, th);
    const long halo = (long)(th + 2 * P) * halo_row_lds(tw, P);
    // tie-break on the smaller halo
    const long key = cost * 100000 + halo;
    if (best_cost < 0 || key < best_cost) {
      best_cost = key;
      best_tw = twl;
    }
  }
  const int tw = 1 << best_tw, th = kBM >> best_tw;
  pl->mode = 1;
  pl->tw_log2 = best_tw;
  pl->hw_lds = halo_row_lds(tw, P);
  const int npix = (th + 2 * P) * pl->hw_lds;
  pl->qs = round_qs(npix);
  pl->tiles_x = ceil_div(W, tw);
  pl->tiles_y = ceil_div(H, th);
  pl->grid_x = N * pl->tiles_x * pl->tiles_y;
  pl->lds_bytes = (size_t)pl->nbuf * cg * pl->qs * 16 + 256 * 16;
  if (pl->nbuf == 2 && ceil_div(pl->qs * cg, 256) > max_pieces)
    return fail(RTPOSE_E_INVAL, "conv halo too large for the staging schedule");
  return 0;
}

template <int KS, int CK, int MODE, int NBUF, int NF, bool PR = false>
static int launch_inst(const ConvArgsT<PR>& a, dim3 grid, size_t lds, hipStream_t s) {
  return launch_kernel<conv_mfma_f32<KS, CK, MODE, NBUF, NF, PR>>(grid, dim3(256), lds, 150 * 1024, s, a);
}

int conv2d_launch(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, hipStream_t s, bool relu_max) {
  const ConvSpec spec = {"conv2d", 4, 1, true, false, true, true, true, true};
  if (int rc = check_conv_features(d, ngroups, spec)) return rc;
  const rtpose_conv_desc& d0 = d[0];
  if (d0.k != 1 && d0.k != 3 && d0.k != 7) return fail(RTPOSE_E_INVAL, "conv2d: k must be 1, 3 or 7");
  if (d0.prelu && (d0.k == 7 || d[0].out_cmap || (ngroups > 1 && d[1].out_cmap)))
    return fail(RTPOSE_E_INVAL, "conv2d: the PReLU epilogue exists for k = 1 and 3 without out_cmap");
  const bool has_res = desc_has_residual(d, ngroups), has_pre = desc_has_preact(d, ngroups);
  if (has_res || has_pre) {
    const char* what = has_res ? "residual epilogue (rtpose_conv_desc.residual)"
                               : "input pre-activation (rtpose_conv_desc.in_scale / in_shift)";
    if (d0.k != 1)
      return fail(RTPOSE_E_INVAL, "conv2d: the %s exists for k = 1 only (a halo's zero padding would become relu(shift); "
                                  "a k x k residual has no kernel)", what);
    if (ngroups != 1 || d0.pool || d0.out_cmap || d0.prelu)
      return fail(RTPOSE_E_INVAL, "conv2d: the %s takes one group without fused pool, out_cmap or PReLU", what);
    if (has_res) {
      if (d0.relu) return fail(RTPOSE_E_INVAL, "conv2d: the residual epilogue has no activation after the sum (relu must be 0)");
      if (!slice_inside(d0.lres, d0.cout) || d0.lres.cstride <= 0 || d0.lres.choff < 0 || H > d0.lres.hs || W > d0.lres.ws)
        return fail(RTPOSE_E_INVAL, "conv2d: residual slice (lres) exceeds cstride or is smaller than the map");
    }
    if (has_pre) {
      if (!d0.in_scale || !d0.in_shift)
        return fail(RTPOSE_E_INVAL, "conv2d: the input pre-activation needs both in_scale and in_shift");
      if ((reinterpret_cast<uintptr_t>(d0.in_scale) | reinterpret_cast<uintptr_t>(d0.in_shift)) % 16)
        return fail(RTPOSE_E_INVAL, "conv2d: in_scale and in_shift (input pre-activation) must be 16-byte aligned");
      if (d0.preact_cin < 0 || d0.preact_cin > d0.cin)
        return fail(RTPOSE_E_INVAL, "conv2d: preact_cin (input pre-activation) must lie in 0 .. cin");
    }
  }
  if (d0.cin % 8 != 0 || d0.cin <= 0) return fail(RTPOSE_E_INVAL, "conv2d: cin must be a multiple of 8");
  if (int rc = check_conv_layouts(d, ngroups, N, H, W, spec)) return rc;
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < ngroups; ++i) fill_group(a.g[i], d[i]);
  ConvPlan pl;
  int rc = plan_conv(d0, N, H, W, &pl);
  if (rc) return rc;
  a.N = N;
  a.H = H;
  a.W = W;
  a.M = N * H * W;
  a.cin = d0.cin;
  a.relu = d0.relu ? (relu_max ? kReluMax : kReluKeepsNan) : 0;
  a.pool = d0.pool;
  a.qs = pl.qs;
  a.hw_lds = pl.hw_lds;
  a.tw_log2 = pl.tw_log2;
  a.tiles_x = pl.tiles_x;
  a.tiles_y = pl.tiles_y;
  // ---- 1-D grid: id order, XCD-aware remap, half-tile tail ------------------------------
  const int n_cu = device_cu_count();  // of the device this launch goes to
  a.mtiles = pl.grid_x;
  // 64-wide N tiles (NF = 1).  128-wide ones (wave tile 64 x 64, NF = 2), measured on the 32 x 368 x 368 workload, help
  // the 8-N-tile 3x3 layers by ~3 % (conv4_1/4_2) and lose 11 % on the 7x7 stage convs (fewer, longer blocks: worse
  // tail, and 32 MFMAs between filler slots) - 427 vs 464 img/s overall.
  a.ntiles = cout_pad(d0.cout) / kConvBN;
  a.ncombo = a.ntiles * ngroups;
  long ids;
  if (int rc = grid_ids(a.mtiles, a.ncombo, a.xcd_remap, ids, "conv2d")) return rc;
  a.nbig = (int)ids;
  if (pl.mode == 0) {
    // Tail quantisation: equal tiles on `slots` co-resident block slots run in lock-step
    // rounds; a last round with few blocks leaves most CUs idle for a whole tile time.  When
    // that remainder is small, its tiles are split into two 64-pixel halves (twice the blocks,
    // half the time).  32x46x46, cout 128 x 2 branches: 2116 tiles = 4 x 512 + 68 -> the last
    // 68 become 136 halves.
    const int slots = n_cu * (pl.nbuf == 1 ? 4 : 2);
    const int total = (int)ids;
    const int rem = total % slots;
    if (total > slots && rem > 0 && 2 * rem <= n_cu) a.nbig = total - rem;
    // small batches (e.g. the reference's own one-image-at-a-time flow): fewer tiles than
    // CUs -> every tile is split, doubling the number of busy CUs
    if (total <= n_cu) a.nbig = 0;
  }
  dim3 grid((unsigned)(a.nbig + 2 * (ids - a.nbig)), 1, 1);
  if (has_res || has_pre) {
    ConvArgsX ax;
    static_cast<ConvArgs&>(ax) = a;
    memset(&ax.x, 0, sizeof(ax.x));
    if (has_res) {
      ax.x.res = d0.residual;
      ax.x.lres = to_lay(d0.lres);
    }
    if (has_pre) {
      ax.x.in_scale = d0.in_scale;
      ax.x.in_shift = d0.in_shift;
      ax.x.pre_cin = d0.preact_cin ? d0.preact_cin : d0.cin;
    }
#define RTPOSE_CONV_CASE_X(CK_, MODE_)    \
  if (pl.ck == CK_ && pl.mode == MODE_) \
    return launch_kernel<conv_mfma_f32_x<CK_, MODE_>>(grid, dim3(256), pl.lds_bytes, 150 * 1024, s, ax);
    RTPOSE_CONV_CASE_X(16, 0)
    RTPOSE_CONV_CASE_X(16, 1)
    RTPOSE_CONV_CASE_X(8, 0)
    RTPOSE_CONV_CASE_X(8, 1)
#undef RTPOSE_CONV_CASE_X
    return fail(RTPOSE_E_INVAL, "conv2d: no residual / pre-activation kernel instance for ck=%d mode=%d", pl.ck, pl.mode);
  }
  if (d0.prelu) {
    ConvArgsP ap;
    static_cast<ConvArgs&>(ap) = a;
    set_prelu(ap, d, ngroups);
#define RTPOSE_CONV_CASE_P(KS_, CK_, MODE_)            \
  if (d0.k == KS_ && pl.ck == CK_ && pl.mode == MODE_) \
    return launch_inst<KS_, CK_, MODE_, KS_ == 1 ? 1 : 2, 1, true>(ap, grid, pl.lds_bytes, s);
    RTPOSE_CONV_CASE_P(3, 8, 0)
    RTPOSE_CONV_CASE_P(3, 8, 1)
    RTPOSE_CONV_CASE_P(3, 16, 0)
    RTPOSE_CONV_CASE_P(3, 16, 1)
    RTPOSE_CONV_CASE_P(1, 16, 0)
    RTPOSE_CONV_CASE_P(1, 16, 1)
    RTPOSE_CONV_CASE_P(1, 8, 0)
    RTPOSE_CONV_CASE_P(1, 8, 1)
#undef RTPOSE_CONV_CASE_P
    return fail(RTPOSE_E_INVAL, "conv2d: no PReLU kernel instance for k=%d ck=%d mode=%d", d0.k, pl.ck, pl.mode);
  }
#define RTPOSE_CONV_CASE(KS_, CK_, MODE_)                \
  if (d0.k == KS_ && pl.ck == CK_ && pl.mode == MODE_) \
    return launch_inst<KS_, CK_, MODE_, KS_ == 1 ? 1 : 2, 1>(a, grid, pl.lds_bytes, s);
  RTPOSE_CONV_CASE(3, 8, 0)
  RTPOSE_CONV_CASE(3, 8, 1)
  RTPOSE_CONV_CASE(3, 16, 0)
  RTPOSE_CONV_CASE(3, 16, 1)
  RTPOSE_CONV_CASE(7, 16, 0)
  RTPOSE_CONV_CASE(7, 16, 1)
  RTPOSE_CONV_CASE(1, 16, 0)
  RTPOSE_CONV_CASE(1, 16, 1)
  RTPOSE_CONV_CASE(1, 8, 0)
  RTPOSE_CONV_CASE(1, 8, 1)
  RTPOSE_CONV_CASE(7, 8, 0)
  RTPOSE_CONV_CASE(7, 8, 1)
#undef RTPOSE_CONV_CASE
  return fail(RTPOSE_E_INVAL, "conv2d: no kernel instance for k=%d ck=%d mode=%d", d0.k, pl.ck, pl.mode);
}

int pack_weights_launch(const float* w, const float* bias, int cout, int cin_src, int k,
                        const int32_t* cin_map, int cin_packed, float* wp, float* bp, hipStream_t s) {
  if (cin_packed % 8 || (cin_packed < cin_src && !cin_map))
    return fail(RTPOSE_E_INVAL, "pack: cin_packed must be a multiple of 8 and >= cin_src");
  if (k != 1 && k != 3 && k != 7) return fail(RTPOSE_E_INVAL, "pack: k must be 1, 3 or 7");
  const int coutp = cout_pad(cout);
  const size_t total = (size_t)k * k * cin_packed * coutp;
  const int threads = 256;
  const unsigned blocks = (unsigned)((total + threads - 1) / threads);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(threads), 0, s, w, bias, cout, cin_src, k,
                     cin_map, cin_packed, conv_ck(cin_packed), coutp, wp, bp);
  RTPOSE_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace rtpose

extern "C" {

size_t rtpose_packed_weight_floats(int cout, int cin, int k) {
  const int cinp = rtpose::ceil_div(cin, 8) * 8;
  // + two (chunk, tap) blocks of slack: the kernel's B prefetch runs two taps ahead
  return (size_t)(k * k * cinp + 32) * rtpose::cout_pad(cout);
}
size_t rtpose_packed_bias_floats(int cout) { return (size_t)rtpose::cout_pad(cout); }

int rtpose_pack_conv_weights(const float* w_oihw, const float* bias, int cout, int cin_src, int k,
                             const int32_t* cin_map, int cin_packed, float* w_packed,
                             float* bias_packed, void* stream) {
  return rtpose::pack_weights_launch(w_oihw, bias, cout, cin_src, k, cin_map, cin_packed, w_packed,
                                     bias_packed, rtpose::as_stream(stream));
}

int rtpose_conv2d(const rtpose_conv_desc* d, int ngroups, int N, int H, int W, void* stream) {
  return rtpose::conv2d_launch(d, ngroups, N, H, W, rtpose::as_stream(stream), false);
}

}  // extern "C"
