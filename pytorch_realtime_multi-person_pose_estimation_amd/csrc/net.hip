// Native executor for the rtpose_vgg network (lib/network/rtpose_vgg.py:60-225):
// builds the launch plan for a given (N, H, W), carves the caller-provided
// workspace into shared-gap padded NHWC activation buffers, packs weights into
// the caller-provided weight arena and enqueues the forward
// (rtpose_model.forward, rtpose_vgg.py:158-198) as a fixed list of launches on
// one HIP stream.
//
// What differs from the reference module graph (same arithmetic, other layout):
//  * torch.cat([L1, L2, out1], 1) (rtpose_vgg.py:165,171,177,183,189) never
//    runs: the two branch heads of stage s write straight into channel slices
//    of one 192-channel buffer laid out [out1 0..127 | PAF 128..165 | heat
//    166..184 | 7 zero], and the 185-input-channel filters are permuted to that
//    order when packed.  Two such buffers ping-pong between stages.
//  * the two branches of a stage (independent, rtpose_vgg.py:163-164) run as
//    one grouped grid per layer.
//  * MaxPool2d is fused into the epilogue of the conv in front of it when the
//    map has even height and width.
//
// A second topology, OpenPose_Model (lib/network/openpose.py:114-177), shares the
// executor (rtpose_openpose_create, build_plan_openpose): the same trunk with PReLU
// epilogues on its last three convs, dense-block stages whose three convs write
// slices of one 3 x inner buffer, and stage heads that write the next stage's
// input buffer in place.
//
// A third topology, the stacked hourglass (lib/network/rtpose_hourglass.py; rtpose_hourglass_create,
// build_plan_hourglass): a 7x7 stride-2 stem, pre-activation Bottlenecks whose `bn1` + ReLU is applied while the 1x1
// conv1 stages its input and whose `out += residual` is the epilogue of the 1x1 conv3 (csrc/conv_mfma.hip), 2x2 max-pools
// and `up1 + upsample(low3)` launches (csrc/hourglass_ops.hip).  Every other BatchNorm follows a conv and reaches the
// plan folded into that conv's filters and bias by the host.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "launchers.h"

using namespace rtpose;

namespace {

struct Buf {
  size_t off_floats = 0;  // offset in the workspace
  size_t floats = 0;
  rtpose_layout lay{};
  int C = 0, H = 0, W = 0;
  // fp32 plans: the buffer is stored as 8-channel planes of `plane_px` pixel slots (mark_plane_bufs) - what the forms of
  // its producer and consumers allow; `stale`: its bytes were written in the other storage and must be cleared first
  // (the gaps of either storage are data positions of the other)
  int plane_px = 0;
  bool stale = false;
};

// The forms a conv can run in, in the order their packings follow each other in the weight arena.  Everything that
// depends on the form is read from kForm: the code the ABI reports (rtpose_net_conv_numerics,
// rtpose_net_launch_executed_flops), the kernel size the form applies to, the m of F(m x m,3x3) / F(m,7) as the
// descriptor's wino_m and the launchers' fm take it, the slot of its amplification estimate in the arena's amp[4]
// (ABI too: rtpose_net_conv_numerics hands the four out in that order) and its rank among the forms of its kernel
// size - direct, which sums in the reference's order, is the most conservative.
// F(8,7) is the exception to "every arena holds every packing": only a plan created with winograd7 = 8 has it, BEHIND
// the standard layout (add_f87_packings), so every other plan keeps its arena byte for byte.  It has no slot in amp[4]
// (which is ABI) - nothing chooses it by its estimate; rtpose_winograd_amplification(.., 7, 8, ..) computes one on demand.
enum Form { F_DIRECT, F_W3_2X2, F_W3_4X4, F_W7_4, F_W7_6, F_W7_8, kForms };
constexpr int kStdForms = F_W7_8;  // the forms of the standard arena layout
struct FormInfo {
  int code, k, fm, amp_slot, rank;
};
constexpr FormInfo kForm[kForms] = {
    {0, 0, 0, -1, 0},  // direct (any kernel size)
    {3, 3, 0, 0, 1},   // F(2x2,3x3)
    {43, 3, 4, 3, 2},  // F(4x4,3x3)
    {4, 7, 4, 1, 1},   // F(4,7)
    {6, 7, 6, 2, 2},   // F(6,7)
    {8, 7, 8, -1, 3},  // F(8,7): opt-in only
};
constexpr size_t kNotPacked = ~(size_t)0;

struct ConvW {
  std::string name;
  int cout = 0, cin_src = 0, cin_packed = 0, k = 0;
  bool cat_perm = false;   // input channels follow the cat([L1,L2,out1]) order
  // Float offsets in the weight arena.  An fp32 arena holds EVERY packing a plan may run the conv in (it is shared by
  // all plans of a module, whatever their geometry and options): the direct one, and every Winograd form that has a
  // kernel for these channel counts; kNotPacked where it has none.  bf16 arenas hold the direct packing only.
  size_t w_off[kForms] = {kNotPacked, kNotPacked, kNotPacked, kNotPacked, kNotPacked, kNotPacked};
  size_t b_off = 0;
  bool first = false;      // conv1_1 (3 -> 64, 3x3): its own kernel, packing at w_off_first (csrc/conv_first.hip)
  size_t w_off_first = 0;
  size_t amp_off = 0;      // 4 floats in the arena: the amplification estimate of each Winograd form at its amp_slot (0 = n/a)
  float amp[4] = {0.f, 0.f, 0.f, 0.f};  // host copy (rtpose_net_finalize_weights)
  Form form = F_DIRECT;    // what THIS plan runs the conv in
  int H = 0, W = 0;        // map size the conv runs at in this plan
  // OpenPose_Model: nn.PReLU after the conv (slopes at pr_off, cout_pad floats; state_dict prefix prelu_name)
  bool has_prelu = false;
  size_t pr_off = 0;
  std::string prelu_name;
  // stacked hourglass: the 7x7 stride-2 stem (its own kernel, packing at w_off_first, csrc/hourglass_ops.hip), and the
  // BatchNorm2d + ReLU in FRONT of a 1x1 conv (scale at pa_off, shift round_up(cin_packed, 64) floats behind it;
  // state_dict prefix of the BatchNorm preact_name)
  bool stem = false;
  bool has_preact = false;
  size_t pa_off = 0;
  std::string preact_name;
  bool packed(Form f) const { return w_off[f] != kNotPacked; }
};

// OP_SAVE: the copy of a stage's maps into its record, run only under keep_intermediates
// OP_UPADD: out_buf[0] = in_buf[0] + upsample2(in_buf[1]) (stacked hourglass)
enum OpKind { OP_INPUT, OP_CONV, OP_POOL, OP_COPY, OP_SAVE, OP_TAIL, OP_UPADD };

struct Op {
  OpKind kind;
  std::string name;
  int H = 0, W = 0;         // spatial size the op runs at
  // conv
  int ngroups = 0;
  int conv_idx[2] = {-1, -1};
  int conv2_idx[2] = {-1, -1};  // OP_TAIL: the second conv of the back-to-back pair
  int in_buf[2] = {-1, -1}, out_buf[2] = {-1, -1};
  int in_choff[2] = {0, 0}, out_choff[2] = {0, 0};
  int relu = 0, pool = 0;
  int res_buf = -1, res_choff = 0;  // conv: the residual its epilogue adds (rtpose_conv_desc.residual)
  int out_f32 = 0;          // bf16 plans: this conv writes fp32 (the final stage heads)
  // pool / copy
  int C = 0;
  double flops = 0.0;
  int ks = 0;
};

}  // namespace

struct rtpose_net {
  int N = 0, H = 0, W = 0;       // input
  int bf16 = 0;                  // 1: bf16 activations/weights, fp32 accumulate (BASELINE config 3)
  int split = 0;                 // bf16 plans only: 1 = "bf16x3" split operands (hi + lo bf16 per value)
  int w3 = RTPOSE_WINO3_AUTO;    // fp32 plans, 3x3 convs: 0 direct, 1 = F(2x2,3x3), 4 = F(4x4,3x3), RTPOSE_WINO3_AUTO = per layer by amp_limit (the default)
  int w7 = RTPOSE_WINO7_AUTO;    // fp32 plans: 0 direct, 4 / 6 / 8 = F(4,7) / F(6,7) / F(8,7), RTPOSE_WINO7_AUTO = per layer by amp_limit (the default)
  float amp_limit = 256.f;
  bool forms_final = false;      // forms chosen (AUTO: after the amplification estimates were read back)
  bool amps_read = false;
  uint64_t seen_gen = ~0ull;     // generation of the weight arena the estimates / forms above were taken from
  int n_cu = 0;                  // CUs of the device the plan was created for (sizes the hand-over scratch)
  hipEvent_t out_guard = nullptr;  // rtpose_net_set_output_guard: waited for before the first launch that writes the buffer
  int guard_op = -1;               // the stage-6 maps are read from (index of that launch)
  int persist7 = 1;              // 1: 7x7 launches whose tiles are not whole rounds run as persistent blocks with split tiles
                                 // (rtpose_net_set_persistent7; cleared by a hand-over that timed out)
  int device = -1;               // HIP device that owns the bound arenas: the only device this plan launches on
  CheckedPtr in_checked;         // last input pointer verified to live on that device
  size_t scratch_off = 0, scratch_bytes = 0;  // persistent 7x7 launches: hand-over scratch inside the workspace
  int x0f_buf = -1;              // bf16 plans: fp32 NHWC8 staging buffer for rtpose_preprocess_u8
  int H3 = 0, W3 = 0;            // stride-8 map
  std::vector<Buf> bufs;
  std::vector<ConvW> convs;
  std::vector<Op> ops;
  size_t ws_floats = 0, wt_floats = 0;
  size_t catmap_off = 0;         // int32[192] inside the weight arena
  float* ws = nullptr;
  float* wt = nullptr;
  bool bound = false;
  int keep = 0;
  int save_buf[6] = {-1, -1, -1, -1, -1, -1};
  int cat_buf[2] = {-1, -1};
  // topology: 0 = rtpose_vgg, 1 = OpenPose_Model (rtpose_openpose_create).  OpenPose plans keep their stage outputs in
  // cat_buf[0] = the stage input buffer [features 128 | PAF | pad to 16 | heat | pad to 16] (heat at op_heat_off) and
  // copy each stage's output to op_save[stage] when keep_intermediates is set.  catmap_host, uploaded at bind: packed
  // input channel -> source channel of the filters that read a concat buffer (rtpose_vgg: cat([L1, L2, out1]);
  // OpenPose_Model: cat([features, heat, paf]) of the l1 stages 1..), -1 = zero taps.
  // 2 = stacked hourglass (rtpose_hourglass_create): the score maps of the stack that ran last live in cat_buf[0] = [PAF |
  // pad to 8 | heat at hg_heat_off | pad to 8] (the pads are never written: the 1x1 convs that read the maps back read them
  // as zero taps), every stack's are copied to op_save[stack] under keep_intermediates.  H3 x W3 is the stride-4 map.
  int topo = 0;
  int hg_stacks = 0, hg_blocks = 0, hg_paf = 0, hg_heat = 0, hg_heat_off = 0;
  int op_l2 = 0, op_l1 = 0, op_paf = 0, op_heat = 0, op_heat_off = 0;
  std::vector<int> op_save;
  std::vector<int32_t> catmap_host;
  int x0_buf = -1;
  int conv1_op = -1;             // the launch that runs conv1_1 in its own kernel (-1: the split plan has none)
  // hipGraph replay of the launch list (ops after the input conversion have fixed arguments):
  // captured once per keep_intermediates setting on a private non-blocking stream that is
  // joined to the caller's stream by events, so it also works under the legacy NULL stream
  int graph_mode = -1;             // -1 unread, 0 off (default), 1 on (RTPOSE_GRAPH=1)
  bool zeroed_at_bind = false;     // rtpose_net_bind cleared the workspace (nothing to clear before the first forward)
  int forwards = 0;                // the first forward runs directly (lazy statics, attributes)
  hipStream_t gstream = nullptr;
  hipEvent_t gev_in = nullptr, gev_out = nullptr;
  hipGraphExec_t gexec[2] = {nullptr, nullptr};
  // profiling
  int profiling = 0;
  std::vector<hipEvent_t> ev;
  bool ev_valid = false;
};

namespace {

// Plans of one module share ONE weight arena, and any of them may be the one a reload is issued through
// (rtpose_net_load_conv).  The forms of an AUTO plan depend on the filters, so every plan must notice a reload made
// through a sibling: the arena's generation - a host-side counter keyed by the arena's base address, bumped by every
// fp32 rtpose_net_load_conv - is compared with the one the plan's estimates were read at (rtpose_net.seen_gen) before
// every forward / finalize / conv_numerics.  (An arena freed and another allocated at the same address just continues
// the count; rtpose_net_bind forgets the plan's generation.)
std::mutex g_arena_mu;
std::unordered_map<const void*, uint64_t> g_arena_gen;

uint64_t arena_generation(const void* wt) {
  std::lock_guard<std::mutex> lk(g_arena_mu);
  auto it = g_arena_gen.find(wt);
  return it == g_arena_gen.end() ? 0 : it->second;
}

void arena_bump(const void* wt) {
  std::lock_guard<std::mutex> lk(g_arena_mu);
  ++g_arena_gen[wt];
}

constexpr int kCatC = 192;      // [out1 128 | PAF 38 | heat 19 | pad 7]
constexpr int kCatPaf = 128, kCatHeat = 166;

int add_buf(rtpose_net* n, int C, int P, int H, int W, bool f32 = false) {
  Buf b;
  b.C = C;
  b.H = H;
  b.W = W;
  b.lay.cstride = C;
  b.lay.choff = 0;
  b.lay.ws = W + P;
  b.lay.hs = H + P;
  b.lay.lead = P * (W + P) + P;
  // bf16 plans keep activations as 2-byte elements (C is even for every such buffer)
  // (split plans: two 2-byte elements per channel = the fp32 footprint)
  const size_t per_px = (n->bf16 && !n->split && !f32) ? (size_t)C / 2 : (size_t)C;
  b.floats = round_up(rtpose_layout_pixels(&b.lay, n->N, H, W) * per_px, 64);
  b.off_floats = n->ws_floats;
  n->ws_floats += b.floats;
  n->bufs.push_back(b);
  return (int)n->bufs.size() - 1;
}

int add_conv_w(rtpose_net* n, const std::string& name, int cout, int cin, int k, bool cat_perm, int H = 0, int W = 0,
               int cin_packed = 0) {
  ConvW c;
  c.name = name;
  c.cout = cout;
  c.cin_src = cin;
  c.cin_packed = cin_packed > 0 ? cin_packed : cat_perm ? kCatC : (n->bf16 ? ceil_div(cin, 16) * 16 : ceil_div(cin, 8) * 8);
  c.k = k;
  c.cat_perm = cat_perm;
  c.H = H;
  c.W = W;
  auto take = [&](size_t floats) {
    const size_t off = n->wt_floats;
    n->wt_floats += round_up(floats, 64);
    return off;
  };
  // conv1_1 has its own kernel in fp32 and bf16 plans (conv_first.hip; bf16: MODE 2 reads the fp32 image, rounds it and the
  // filters to bf16, writes bf16; not the split plans) - the generic packing stays in the arena for rtpose_net_conv introspection
  c.first = !n->split && k == 3 && cin == 3 && cout == 64;
  if (n->bf16) {
    c.w_off[F_DIRECT] = take(n->split ? rtpose_packed_weight_bytes_bf16x3(cout, c.cin_packed, k) / 4
                                      : rtpose_packed_weight_bytes_bf16(cout, c.cin_packed, k) / 4);
  } else {
    // The weight arena is shared by every plan of a module (any N x H x W, any rtpose_net_options), so its layout
    // depends on the channel counts only: the direct packing, plus every Winograd packing that has a kernel.
    // (3x3 with < 32 input channels stays direct: nothing to amortise the transforms over - conv1_1, 3 -> 64 on 8
    //  padded channels, takes 0.71 ms in Winograd form and 0.50 ms in the direct kernel)
    c.w_off[F_DIRECT] = take(rtpose_packed_weight_floats(cout, c.cin_packed, k));
    const bool w3 = k == 3 && c.cin_packed >= 32 && conv2d_winograd_fits(3, c.cin_packed, cout, 0, 1, 8, 8, 9, 0);
    const bool w7 = k == 7 && c.cin_packed % 8 == 0 && cout_pad(cout) % 128 == 0;
    for (int f = F_DIRECT + 1; f < kStdForms; ++f) {
      const int fm = kForm[f].fm;
      if (kForm[f].k == 3 && w3 && (f == F_W3_2X2 || conv2d_winograd_fits(3, c.cin_packed, cout, 0, 1, 8, 8, 9, fm)))
        c.w_off[f] = take(rtpose_packed_weight_floats_winograd3(cout, c.cin_packed, fm));
      if (kForm[f].k == 7 && w7) c.w_off[f] = take(packed_weight_floats_wino7(cout, c.cin_packed, fm));
    }
    c.amp_off = take(4);
  }
  if (c.first) c.w_off_first = take(conv_first_packed_floats());
  c.b_off = take(rtpose_packed_bias_floats(cout));
  n->convs.push_back(c);
  return (int)n->convs.size() - 1;
}

// A plan created with winograd7 = 8: the F(8,7) packing of every 7x7 conv that has Winograd packings, behind everything
// the standard layout holds (called last by build_plan).
void add_f87_packings(rtpose_net* n) {
  if (n->bf16 || n->w7 != 8) return;
  for (ConvW& c : n->convs) {
    if (!c.packed(F_W7_6)) continue;
    c.w_off[F_W7_8] = n->wt_floats;
    n->wt_floats += round_up(packed_weight_floats_wino7(c.cout, c.cin_packed, 8), 64);
  }
}

// The form plan `n` runs conv `c` in.  (It is NOT chosen by batch size: the direct kernel sums in another order, and
// an image's maps would depend on the batch it is evaluated in.  Small grids get the frequency-split launch of the
// same arithmetic instead, conv_wino7.hip: wino7s_f32.)  A form without a kernel instance at the plan's geometry -
// F(m,7) on maps so wide that the transformed rows of a block do not fit the LDS - falls back to the next one.
Form pick_form(const rtpose_net* n, const ConvW& c) {
  if (n->bf16) return F_DIRECT;
  auto tame = [&](Form f) { return c.amp[kForm[f].amp_slot] <= n->amp_limit; };
  if (c.k == 3) {
    if (!c.packed(F_W3_2X2) || !n->w3) return F_DIRECT;
    if (c.packed(F_W3_4X4) && (n->w3 == 4 || (n->w3 == RTPOSE_WINO3_AUTO && tame(F_W3_4X4)))) return F_W3_4X4;
    return F_W3_2X2;
  }
  if (c.k != 7 || !c.packed(F_W7_4) || !n->w7) return F_DIRECT;
  auto fits = [&](Form f) {
    return conv2d_winograd_fits(7, c.cin_packed, c.cout, 0, n->N, c.H, c.W, c.H + 3, kForm[f].fm) != 0;
  };
  if (n->w7 == RTPOSE_WINO7_AUTO) {
    if (tame(F_W7_6) && fits(F_W7_6)) return F_W7_6;
    if (tame(F_W7_4) && fits(F_W7_4)) return F_W7_4;
    return F_DIRECT;
  }
  if (n->w7 == 8 && c.packed(F_W7_8) && fits(F_W7_8)) return F_W7_8;
  if (n->w7 >= 6 && fits(F_W7_6)) return F_W7_6;
  return fits(F_W7_4) ? F_W7_4 : F_DIRECT;
}

bool forms_need_amps(const rtpose_net* n) {
  return !n->bf16 && (n->w7 == RTPOSE_WINO7_AUTO || n->w3 == RTPOSE_WINO3_AUTO);
}

// the filters in the arena changed since this plan last looked (through this plan or a sibling): estimates and AUTO
// forms are stale
void sync_arena_generation(rtpose_net* n) {
  if (n->bf16 || !n->bound) return;
  const uint64_t g = arena_generation(n->wt);
  if (g == n->seen_gen) return;
  n->seen_gen = g;
  n->amps_read = false;
  if (forms_need_amps(n)) n->forms_final = false;
}

void pick_forms(rtpose_net* n) {
  for (ConvW& c : n->convs) c.form = pick_form(n, c);
  // the two branches of a grouped launch run one kernel: the more conservative form of the two
  for (Op& o : n->ops) {
    if (o.kind != OP_CONV || o.ngroups < 2) continue;
    ConvW &a = n->convs[o.conv_idx[0]], &b = n->convs[o.conv_idx[1]];
    a.form = b.form = kForm[a.form].rank < kForm[b.form].rank ? a.form : b.form;
  }
}

// Channel-plane storage (conv_wino4.hip) for every buffer that only F(4x4,3x3) launches - and conv1_1 - touch: written by
// ONE conv (conv1_1's own kernel or a conv in that form; a branch of a grouped launch counts) as a whole, read only by convs
// in that form as a whole.  Depends on the forms, so it is re-derived whenever they are; a buffer that changes storage is
// cleared before the next forward.
void mark_plane_bufs(rtpose_net* n) {
  const int nb = (int)n->bufs.size();
  std::vector<int> writers(nb, 0), readers(nb, 0);
  std::vector<char> ok(nb, 1);
  for (const Op& o : n->ops) {
    const bool conv = o.kind == OP_CONV;
    for (int g = 0; g < (o.ngroups > 0 ? o.ngroups : 1); ++g) {
      const int bi = o.in_buf[g], bo = o.out_buf[g];
      const ConvW* c = conv ? &n->convs[o.conv_idx[g]] : nullptr;
      if (bi >= 0) {
        ++readers[bi];
        if (!(conv && c->form == F_W3_4X4 && o.in_choff[g] == 0 && c->cin_packed == n->bufs[bi].C)) ok[bi] = 0;
      }
      if (bo >= 0) {
        ++writers[bo];
        if (!(conv && (c->form == F_W3_4X4 || c->first) && o.out_choff[g] == 0 && c->cout == n->bufs[bo].C))
          ok[bo] = 0;
      }
    }
  }
  for (int b = 0; b < nb; ++b) {
    Buf& bf = n->bufs[b];
    const size_t px = bf.C > 0 ? bf.floats / (size_t)bf.C : 0;  // pixel slots of the buffer (>= the layout's pixels)
    const bool planes = !n->bf16 && ok[b] && writers[b] == 1 && readers[b] >= 1 && bf.C % 8 == 0 &&
                        px * (size_t)bf.C * sizeof(float) < 0x7ffffffeull && px <= 0x7fffffffull;
    const int want = planes ? (int)px : 0;
    if (want != bf.plane_px) {
      bf.plane_px = want;
      bf.stale = true;
    }
  }
}

void add_conv_op(rtpose_net* n, int H, int W, int ngroups, const int* conv_idx, const int* in_buf,
                 const int* in_choff, const int* out_buf, const int* out_choff, int relu, int pool) {
  Op o;
  o.kind = OP_CONV;
  o.H = H;
  o.W = W;
  o.ngroups = ngroups;
  o.relu = relu;
  o.pool = pool;
  double fl = 0;
  for (int i = 0; i < ngroups; ++i) {
    o.conv_idx[i] = conv_idx[i];
    o.in_buf[i] = in_buf[i];
    o.in_choff[i] = in_choff[i];
    o.out_buf[i] = out_buf[i];
    o.out_choff[i] = out_choff[i];
    const ConvW& c = n->convs[conv_idx[i]];
    // algorithmic flops: direct-convolution count of the reference nn.Conv2d
    fl += 2.0 * n->N * H * W * (double)c.cout * c.cin_src * c.k * c.k;
    o.name += (i ? "+" : "") + c.name;
  }
  o.flops = fl;
  o.ks = n->convs[conv_idx[0]].k;
  if (n->convs[conv_idx[0]].first || n->convs[conv_idx[0]].stem) n->conv1_op = (int)n->ops.size();
  n->ops.push_back(o);
}

// The trailing 1x1 pair of a stage, c1 (ReLU) -> c2 (linear), of both branches as ONE back-to-back launch (conv_tail.hip /
// conv_tail_bf16.hip): the intermediate never leaves the CU
void add_tail_op(rtpose_net* n, int H, int W, const int* c1, const int* c2, const int* in_buf, const int* out_buf,
                 const int* out_choff, int out_f32) {
  Op o;
  o.kind = OP_TAIL;
  o.H = H;
  o.W = W;
  o.ngroups = 2;
  o.out_f32 = out_f32;
  o.ks = 1;
  for (int b = 0; b < 2; ++b) {
    o.conv_idx[b] = c1[b];
    o.conv2_idx[b] = c2[b];
    o.in_buf[b] = in_buf[b];
    o.out_buf[b] = out_buf[b];
    o.out_choff[b] = out_choff[b];
    const ConvW &w1 = n->convs[c1[b]], &w2 = n->convs[c2[b]];
    o.flops += 2.0 * n->N * H * W * ((double)w1.cout * w1.cin_src + (double)w2.cout * w2.cin_src);
    o.name += (b ? "|" : "") + w1.name + "+" + w2.name;
  }
  n->ops.push_back(o);
}

void add_simple_op(rtpose_net* n, OpKind kind, const std::string& name, int H, int W, int in_buf,
                   int in_choff, int out_buf, int out_choff, int C) {
  Op o;
  o.kind = kind;
  o.name = name;
  o.H = H;
  o.W = W;
  o.in_buf[0] = in_buf;
  o.in_choff[0] = in_choff;
  o.out_buf[0] = out_buf;
  o.out_choff[0] = out_choff;
  o.C = C;
  n->ops.push_back(o);
}

// conv (+pool) writing into a buffer at the pooled or the same resolution
void plan_vgg_conv(rtpose_net* n, int conv, int H, int W, int in_buf, int out_buf_same,
                   int out_buf_pooled) {
  const int zero = 0;
  if (out_buf_pooled < 0) {
    // (OpenPose_Model: conv4_2 .. conv4_4_CPM end in a PReLU instead of the ReLU; never in front of a pool)
    add_conv_op(n, H, W, 1, &conv, &in_buf, &zero, &out_buf_same, &zero, n->convs[conv].has_prelu ? 0 : 1, 0);
  } else if (!((H | W) & 1)) {
    add_conv_op(n, H, W, 1, &conv, &in_buf, &zero, &out_buf_pooled, &zero, 1, 1);
  } else {
    add_conv_op(n, H, W, 1, &conv, &in_buf, &zero, &out_buf_same, &zero, 1, 0);
    add_simple_op(n, OP_POOL, "pool", H, W, out_buf_same, 0, out_buf_pooled, 0,
                  n->bufs[out_buf_same].C);
  }
}

// the nn.PReLU that follows conv `conv`: slopes in the arena, padded like the bias
void add_prelu(rtpose_net* n, int conv, const std::string& name) {
  ConvW& c = n->convs[conv];
  c.has_prelu = true;
  c.prelu_name = name;
  c.pr_off = n->wt_floats;
  n->wt_floats += round_up(rtpose_packed_bias_floats(c.cout), 64);
}

// The trunk both topologies start with: VGG19's first 10 convs + 2 CPM convs (rtpose_vgg.py:69-83, openpose.py:28-44) as
// convs `prefix`0 .. `prefix`25 in state_dict order, the input and trunk buffers, the input conversion and the launches of
// convs 0..10.  Sets H3 / W3.  The last conv, cw[11] (conv4_4_CPM), reads D3; what it writes is the caller's.
// `prelu_tail` (openpose.py:40-44): the last three convs end in an nn.PReLU, named by the index after the conv's.
struct Trunk {
  int cw[12];
  int D3;
};

Trunk add_trunk(rtpose_net* n, const std::string& prefix, bool prelu_tail) {
  const int H0 = n->H, W0 = n->W;
  const int H1 = H0 / 2, W1 = W0 / 2, H2 = H1 / 2, W2 = W1 / 2, H3 = H2 / 2, W3 = W2 / 2;
  n->H3 = H3;
  n->W3 = W3;
  const int vgg_idx[12] = {0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25};
  const int vgg_cin[12] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 256};
  const int vgg_cout[12] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 256, 128};
  Trunk t;
  for (int i = 0; i < 12; ++i) {
    t.cw[i] = add_conv_w(n, prefix + std::to_string(vgg_idx[i]), vgg_cout[i], vgg_cin[i], 3, false);
    if (prelu_tail && i >= 9) add_prelu(n, t.cw[i], prefix + std::to_string(vgg_idx[i] + 1));
  }

  const int X0 = add_buf(n, n->bf16 ? 16 : 8, 1, H0, W0);
  n->x0_buf = X0;
  if (n->bf16) n->x0f_buf = add_buf(n, 8, 1, H0, W0, true);
  const int A1 = add_buf(n, 64, 1, H0, W0);
  // (A2 / B2 / C4: the un-pooled map of a conv whose pool cannot be fused, odd height or width)
  const bool even0 = !((H0 | W0) & 1), even1 = !((H1 | W1) & 1), even2 = !((H2 | W2) & 1);
  const int A2 = even0 ? -1 : add_buf(n, 64, 0, H0, W0);
  const int B0 = add_buf(n, 64, 1, H1, W1);
  const int B1 = add_buf(n, 128, 1, H1, W1);
  const int B2 = even1 ? -1 : add_buf(n, 128, 0, H1, W1);
  const int C0 = add_buf(n, 128, 1, H2, W2);
  const int C1 = add_buf(n, 256, 1, H2, W2);
  const int C2 = add_buf(n, 256, 1, H2, W2);
  const int C3 = add_buf(n, 256, 1, H2, W2);
  const int C4 = even2 ? -1 : add_buf(n, 256, 0, H2, W2);
  const int D0 = add_buf(n, 256, 1, H3, W3);
  const int D1 = add_buf(n, 512, 1, H3, W3);
  const int D2 = add_buf(n, 512, 1, H3, W3);
  t.D3 = add_buf(n, 256, 1, H3, W3);

  add_simple_op(n, OP_INPUT, "nchw_to_nhwc8", H0, W0, -1, 0, X0, 0, 3);
  plan_vgg_conv(n, t.cw[0], H0, W0, X0, A1, -1);
  plan_vgg_conv(n, t.cw[1], H0, W0, A1, A2, B0);
  plan_vgg_conv(n, t.cw[2], H1, W1, B0, B1, -1);
  plan_vgg_conv(n, t.cw[3], H1, W1, B1, B2, C0);
  plan_vgg_conv(n, t.cw[4], H2, W2, C0, C1, -1);
  plan_vgg_conv(n, t.cw[5], H2, W2, C1, C2, -1);
  plan_vgg_conv(n, t.cw[6], H2, W2, C2, C3, -1);
  plan_vgg_conv(n, t.cw[7], H2, W2, C3, C4, D0);
  plan_vgg_conv(n, t.cw[8], H3, W3, D0, D1, -1);
  plan_vgg_conv(n, t.cw[9], H3, W3, D1, D2, -1);
  plan_vgg_conv(n, t.cw[10], H3, W3, D2, t.D3, -1);
  return t;
}

// rtpose_vgg.  Weights in the reference's state_dict order (rtpose_vgg.py:141-155); the order of the add_conv_w / add_buf /
// add_*_op calls IS the layout of the weight arena and of the workspace and the launch list.
void build_plan(rtpose_net* n) {
  const Trunk tr = add_trunk(n, "model0.", false);
  const int H3 = n->H3, W3 = n->W3;

  // ---- stage weights: branch 1 (PAF, 38) for stages 1..6, then branch 2 (heat, 19); [layer][branch] ----
  int cw1[5][2], cws[5][7][2];
  for (int b = 0; b < 2; ++b) {
    const int last = b == 0 ? 38 : 19;
    const std::string sfx = "_" + std::to_string(b + 1) + ".";
    // stage 1 (rtpose_vgg.py:95-105)
    for (int i = 0; i < 5; ++i) {
      const int cin = i < 4 ? 128 : 512;
      const int cout = i < 3 ? 128 : (i == 3 ? 512 : last);
      const int k = i < 3 ? 3 : 1;
      cw1[i][b] = add_conv_w(n, "model1" + sfx + std::to_string(2 * i), cout, cin, k, false);
    }
    // stages 2..6 (rtpose_vgg.py:108-127)
    for (int s = 2; s <= 6; ++s)
      for (int i = 0; i < 7; ++i) {
        const int cin = i == 0 ? 185 : 128;
        const int cout = i < 6 ? 128 : last;
        const int k = i < 5 ? 7 : 1;
        cws[s - 2][i][b] = add_conv_w(n, "model" + std::to_string(s) + sfx + std::to_string(2 * i),
                                      cout, cin, k, i == 0, H3, W3);
      }
  }
  n->catmap_off = n->wt_floats;
  n->wt_floats += 256;  // int32[192]
  add_f87_packings(n);
  n->catmap_host.assign(kCatC, -1);  // channel map of the concat input: packed c -> source channel of cat([L1,L2,out1])
  for (int c = 0; c < 185; ++c)
    n->catmap_host[c] = c < 128 ? 57 + c : c < kCatHeat ? c - kCatPaf : 38 + (c - kCatHeat);

  // ---- activation buffers ------------------------------------------------------
  const int CATa = add_buf(n, kCatC, 3, H3, W3);
  const int CATb = add_buf(n, kCatC, 3, H3, W3);
  n->cat_buf[0] = CATa;
  n->cat_buf[1] = CATb;
  int T1[2], T2[2], T3[2], T4[2], U[6][2];
  for (int b = 0; b < 2; ++b) {
    T1[b] = add_buf(n, 128, 1, H3, W3);
    T2[b] = add_buf(n, 128, 1, H3, W3);
    T3[b] = add_buf(n, 128, 0, H3, W3);
    // (fp32 and bf16 plans run the trailing 1x1 pairs back to back, conv_tail.hip / conv_tail_bf16.hip: their intermediates
    //  never reach HBM; the split plan keeps them)
    T4[b] = n->split ? add_buf(n, 512, 0, H3, W3) : -1;
    for (int i = 0; i < 4; ++i) U[i][b] = add_buf(n, 128, 3, H3, W3);
    U[4][b] = add_buf(n, 128, 0, H3, W3);
    U[5][b] = n->split ? add_buf(n, 128, 0, H3, W3) : -1;
  }
  for (int s = 0; s < 6; ++s) n->save_buf[s] = add_buf(n, 57, 0, H3, W3, true);  // always fp32
  if (!n->bf16) {
    // hand-over scratch of the persistent 7x7 launches (conv_wino7.hip): part of the workspace, so that the
    // forward allocates nothing, rtpose_net_workspace_bytes tells the whole truth and the launch list can be
    // stream-captured.  One scratch: the launches of a plan are serialised on one stream.
    n->scratch_off = round_up(n->ws_floats, 64);
    n->scratch_bytes = conv2d_wino7_scratch_bytes(n->n_cu, n->w7 == 8 ? 8 : 6);
    n->ws_floats = n->scratch_off + round_up(n->scratch_bytes / 4, 64);
  }

  // ---- launches ------------------------------------------------------------------
  // conv4_4_CPM -> out1, written once into each concat buffer
  plan_vgg_conv(n, tr.cw[11], H3, W3, tr.D3, CATa, -1);
  add_simple_op(n, OP_COPY, "out1->cat_b", H3, W3, CATa, 0, CATb, 0, 128);
  const int zz[2] = {0, 0};
  const int head_off[2] = {kCatPaf, kCatHeat};
  {  // stage 1: reads out1 = CATa[0:128]; heads write CATb
    const int in0[2] = {CATa, CATa}, outb[2] = {CATb, CATb};
    add_conv_op(n, H3, W3, 2, cw1[0], in0, zz, T1, zz, 1, 0);
    add_conv_op(n, H3, W3, 2, cw1[1], T1, zz, T2, zz, 1, 0);
    add_conv_op(n, H3, W3, 2, cw1[2], T2, zz, T3, zz, 1, 0);
    if (!n->split) {
      // fp32 and bf16: conv5_4_CPM (128 -> 512, ReLU) + conv5_5_CPM (512 -> 38 | 19) as one back-to-back launch;
      // the split (bf16x3) plan keeps two launches of its generic kernel
      add_tail_op(n, H3, W3, cw1[3], cw1[4], T3, outb, head_off, 0);
    } else {
      add_conv_op(n, H3, W3, 2, cw1[3], T3, zz, T4, zz, 1, 0);
      add_conv_op(n, H3, W3, 2, cw1[4], T4, zz, outb, head_off, 0, 0);
    }
    add_simple_op(n, OP_SAVE, "save1", H3, W3, CATb, kCatPaf, n->save_buf[0], 0, 57);
  }
  for (int s = 2; s <= 6; ++s) {
    const int(*cw)[2] = cws[s - 2];
    const int cin_buf = (s % 2 == 0) ? CATb : CATa;
    const int cout_buf = (s % 2 == 0) ? CATa : CATb;
    const int in0[2] = {cin_buf, cin_buf};
    add_conv_op(n, H3, W3, 2, cw[0], in0, zz, U[0], zz, 1, 0);
    for (int i = 1; i < (n->split ? 6 : 5); ++i) add_conv_op(n, H3, W3, 2, cw[i], U[i - 1], zz, U[i], zz, 1, 0);
    // The decoder and the TTA merge read fp32: the last heads of a bf16 plan write the fp32 stage-6 record (no bf16
    // concat slice, no save copy).
    const bool last_bf16 = n->bf16 && s == 6;
    const int dst = last_bf16 ? n->save_buf[5] : cout_buf;
    const int outb[2] = {dst, dst};
    const int off57[2] = {0, 38};
    const int* out_off = last_bf16 ? off57 : head_off;
    if (!n->split) {
      // fp32 and bf16: Mconv6 (128 -> 128, ReLU) + Mconv7 (128 -> 38 | 19) of both branches as ONE back-to-back launch
      add_tail_op(n, H3, W3, cw[5], cw[6], U[4], outb, out_off, last_bf16);
    } else {
      add_conv_op(n, H3, W3, 2, cw[6], U[5], zz, outb, out_off, 0, 0);
      n->ops.back().out_f32 = last_bf16;
    }
    if (!last_bf16)
      add_simple_op(n, OP_SAVE, "save" + std::to_string(s), H3, W3, cout_buf, kCatPaf, n->save_buf[s - 1], 0, 57);
  }
}

// OpenPose_Model (openpose.py:114-177).  Stage input buffer IN = [features 0..127 | PAF 128.. | pad | heat R.. | pad], R =
// the PAF end rounded up to 16, S = the heat end rounded up to 16.  The l2 stages 1.. and the l1 stage 0 read IN[0:R]
// (cat([features, paf]) is its natural order, the pad gets zero taps), the l1 stages 1.. read IN[0:S] through a channel map
// (cat([features, heat, paf]), openpose.py:174).  Nothing a stage reads is left over from an earlier forward: the PAF and
// heat slices are written before they are read in every forward and the pads are never written.  Every 3x3 stage conv is
// a dense-block conv: Mconv{b}_0 reads the whole 3 x inner buffer of block b - 1 (or IN) and writes slice 0 of block b's,
// Mconv{b}_1 / _2 read slice 0 / 1 and write slice 1 / 2 (the torch.cat of openpose.py:86-105 never runs); two buffers
// per inner width ping-pong between blocks.  The head (Mconv6 1x1 + PReLU into HEAD, Mconv7 1x1 linear) writes the stage's
// output into its IN slice, from where the next stage reads it.
void build_plan_openpose(rtpose_net* n) {
  const int P = n->op_paf, Hc = n->op_heat;
  const int R = (128 + P + 15) / 16 * 16;
  const int S = (R + Hc + 15) / 16 * 16;
  n->op_heat_off = R;

  // ---- weights, in the reference's state_dict order ----
  const Trunk tr = add_trunk(n, "feature_extractor.", true);
  const int H3 = n->H3, W3 = n->W3;
  struct StageW {
    int br, inner, cw[5][3], m6, m7;
  };
  std::vector<StageW> st;
  for (int br = 0; br < 2; ++br)
    for (int s = 0; s < (br == 0 ? n->op_l2 : n->op_l1); ++s) {
      StageW w;
      w.br = br;
      w.inner = s == 0 ? 96 : 128;
      const int n1 = s == 0 ? 256 : 512, cout = br == 0 ? P : Hc;
      const int cin0 = br == 0 ? (s == 0 ? 128 : 128 + P) : (s == 0 ? 128 + P : 128 + P + Hc);
      const int cinp0 = br == 0 ? (s == 0 ? 128 : R) : (s == 0 ? R : S);
      const std::string pre = (br == 0 ? "l2_stages." : "l1_stages.") + std::to_string(s) + ".";
      for (int b = 0; b < 5; ++b)
        for (int j = 0; j < 3; ++j) {
          const std::string blk = pre + "Mconv" + std::to_string(b + 1) + "_" + std::to_string(j);
          const bool in0 = b == 0 && j == 0;
          const int cin = j ? w.inner : (b ? 3 * w.inner : cin0);
          w.cw[b][j] = add_conv_w(n, blk + ".Mconv", w.inner, cin, 3, in0 && br == 1 && s > 0, H3, W3, in0 ? cinp0 : 0);
          add_prelu(n, w.cw[b][j], blk + ".MPrelu");
        }
      w.m6 = add_conv_w(n, pre + "Mconv6.Mconv", n1, 3 * w.inner, 1, false, H3, W3);
      add_prelu(n, w.m6, pre + "Mconv6.MPrelu");
      w.m7 = add_conv_w(n, pre + "Mconv7", cout, n1, 1, false, H3, W3);
      st.push_back(w);
    }
  n->catmap_off = n->wt_floats;
  n->wt_floats += 256;  // int32[S <= 256]
  n->catmap_host.assign(S, -1);
  for (int c = 0; c < S; ++c) {
    if (c < 128) n->catmap_host[c] = c;
    else if (c < 128 + P) n->catmap_host[c] = 128 + Hc + (c - 128);
    else if (c >= R && c < R + Hc) n->catmap_host[c] = 128 + (c - R);
  }

  // ---- activation buffers: after the trunk's, IN, the dense-block pairs, HEAD and the stage records ----
  const int IN = add_buf(n, S, 1, H3, W3);
  n->cat_buf[0] = IN;
  const int DB96[2] = {add_buf(n, 288, 1, H3, W3), add_buf(n, 288, 1, H3, W3)};
  const int DB128[2] = {add_buf(n, 384, 1, H3, W3), add_buf(n, 384, 1, H3, W3)};
  const int HEAD = add_buf(n, 512, 0, H3, W3);
  for (const StageW& w : st) n->op_save.push_back(add_buf(n, w.br == 0 ? P : Hc, 0, H3, W3));

  // ---- launches ----
  plan_vgg_conv(n, tr.cw[11], H3, W3, tr.D3, IN, -1);  // conv4_4_CPM + PReLU -> features
  const int zero = 0;
  for (size_t si = 0; si < st.size(); ++si) {
    const StageW& w = st[si];
    const int* db = w.inner == 96 ? DB96 : DB128;
    for (int b = 0; b < 5; ++b) {
      const int dst = db[b & 1];
      const int src0 = b ? db[(b + 1) & 1] : IN;
      const int off1 = w.inner, off2 = 2 * w.inner;
      add_conv_op(n, H3, W3, 1, &w.cw[b][0], &src0, &zero, &dst, &zero, 0, 0);
      add_conv_op(n, H3, W3, 1, &w.cw[b][1], &dst, &zero, &dst, &off1, 0, 0);
      add_conv_op(n, H3, W3, 1, &w.cw[b][2], &dst, &off1, &dst, &off2, 0, 0);
    }
    const int last = db[0];  // block 5 (b = 4) wrote db[0]
    const int out_off = w.br == 0 ? 128 : R;
    add_conv_op(n, H3, W3, 1, &w.m6, &last, &zero, &HEAD, &zero, 0, 0);
    add_conv_op(n, H3, W3, 1, &w.m7, &HEAD, &zero, &IN, &out_off, 0, 0);
    add_simple_op(n, OP_SAVE, "save" + std::to_string(si), H3, W3, IN, out_off, n->op_save[si], 0,
                  w.br == 0 ? P : Hc);
  }
}

// The stacked hourglass, hg(num_stacks, num_blocks, paf_classes, ht_classes) of rtpose_hourglass.py:201.  Weights in the
// reference's state_dict order: conv1, layer1..3, hg (every stack), res, fc, score_ht, score_paf, fc_, paf_score_,
// ht_score_ (the order HourglassNet.__init__ registers them in, :126-133); inside a Bottleneck conv1, conv2, conv3,
// downsample.0.
//
// Buffers.  X (256 channels, stride 4) is the running `x` of the stacks: layer2 writes it, layer3 and every hand-over add
// into it in place.  Depth level n of an hourglass (4 at stride 4 .. 1 at stride 32) owns UP[n], where hg[n-1][0] writes
// up1 and the upsample-add leaves the level's result in place, and L[n-1], where the pooled input becomes low1 in place;
// a level's input (X, or L[n] of the level above) is last read by its pool, so up1 survives until its add and nothing
// else has to.  A Bottleneck without downsample whose input nobody else needs runs in place (conv3 adds into the buffer
// its input lives in); one with downsample runs it first and conv3 on top.  T1[r] / T2[r] hold conv1's and conv2's
// output per resolution.  Nothing is read through taps an earlier forward may have left non-finite: every channel count
// but the score maps' is a multiple of 8, the score buffer's pad channels are never written, and the gap of T1 (the only
// buffer a 3x3 conv reads) is never written either.
//
// The hand-over x + fc_(y) + paf_score_(score_paf) + ht_score_(score_ht) is three residual-accumulating 1x1 launches into
// X: each conv keeps its own index, filters and bias as the state_dict has them (one K = 320 conv would need a packing
// over three state_dict entries), and the two small ones are 4 % of fc_'s work.
struct Bneck {
  int c1, c2, c3, ds;
};

void add_preact(rtpose_net* n, int conv, const std::string& name) {
  ConvW& c = n->convs[conv];
  c.has_preact = true;
  c.preact_name = name;
  c.pa_off = n->wt_floats;
  n->wt_floats += 2 * round_up((size_t)c.cin_packed, 64);
}

Bneck add_bneck_w(rtpose_net* n, const std::string& pre, int cin, int planes, bool ds) {
  Bneck b;
  b.c1 = add_conv_w(n, pre + ".conv1", planes, cin, 1, false);
  add_preact(n, b.c1, pre + ".bn1");
  b.c2 = add_conv_w(n, pre + ".conv2", planes, planes, 3, false);
  b.c3 = add_conv_w(n, pre + ".conv3", 2 * planes, planes, 1, false);
  b.ds = ds ? add_conv_w(n, pre + ".downsample.0", 2 * planes, cin, 1, false) : -1;
  return b;
}

// the num_blocks Bottlenecks of one nn.Sequential (_make_residual): 2 * planes -> 2 * planes
std::vector<Bneck> add_seq_w(rtpose_net* n, const std::string& pre, int blocks) {
  std::vector<Bneck> v;
  for (int b = 0; b < blocks; ++b) v.push_back(add_bneck_w(n, pre + "." + std::to_string(b), 256, 128, false));
  return v;
}

void add_conv1(rtpose_net* n, int H, int W, int conv, int in_buf, int in_choff, int out_buf, int out_choff, int relu,
               int res_buf = -1) {
  add_conv_op(n, H, W, 1, &conv, &in_buf, &in_choff, &out_buf, &out_choff, relu, 0);
  n->ops.back().res_buf = res_buf;
}

// one Bottleneck at H x W: in -> out (out == in: in place)
void plan_bneck(rtpose_net* n, const Bneck& b, int H, int W, int in, int out, int t1, int t2) {
  add_conv1(n, H, W, b.c1, in, 0, t1, 0, 1);  // relu(bn2(conv1(relu(bn1(x)))))
  add_conv1(n, H, W, b.c2, t1, 0, t2, 0, 1);  // relu(bn3(conv2(.)))
  if (b.ds >= 0) {
    add_conv1(n, H, W, b.ds, in, 0, out, 0, 0);
    add_conv1(n, H, W, b.c3, t2, 0, out, 0, 0, out);
  } else {
    add_conv1(n, H, W, b.c3, t2, 0, out, 0, 0, in);
  }
}

void plan_seq(rtpose_net* n, const std::vector<Bneck>& v, int H, int W, int in, int out, int t1, int t2) {
  for (size_t i = 0; i < v.size(); ++i) plan_bneck(n, v[i], H, W, i ? out : in, out, t1, t2);
}

void build_plan_hourglass(rtpose_net* n) {
  const int S = n->hg_stacks, NB = n->hg_blocks, P = n->hg_paf, Hc = n->hg_heat;
  const int hoff = ceil_div(P, 8) * 8, sc_c = hoff + ceil_div(Hc, 8) * 8;
  n->hg_heat_off = hoff;
  const int H0 = n->H, W0 = n->W, H1 = H0 / 2, W1 = W0 / 2;
  int RH[5], RW[5];  // depth level 4 (stride 4) .. 0 (stride 64)
  for (int l = 4; l >= 0; --l) {
    RH[l] = H0 >> (6 - l);
    RW[l] = W0 >> (6 - l);
  }
  n->H3 = RH[4];
  n->W3 = RW[4];

  // ---- weights, in the reference's state_dict order ----
  const int stem = add_conv_w(n, "conv1", 64, 3, 7, false);
  // (as for conv1_1: the generic 7x7 packing of add_conv_w stays in the arena - packed on every load, read by no launch -
  //  so that the conv is an ordinary entry of the conv table; the launch reads the packing below)
  n->convs[stem].stem = true;
  n->convs[stem].w_off_first = n->wt_floats;
  n->wt_floats += round_up(conv7x7_s2_packed_floats(), 64);
  const Bneck l1 = add_bneck_w(n, "layer1.0", 64, 64, true);
  const Bneck l2 = add_bneck_w(n, "layer2.0", 128, 128, true);
  const Bneck l3 = add_bneck_w(n, "layer3.0", 256, 128, false);
  std::vector<std::vector<std::vector<std::vector<Bneck>>>> hgw(S);  // [stack][level index 0..3][j]
  for (int s = 0; s < S; ++s) {
    hgw[s].resize(4);
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < (i == 0 ? 4 : 3); ++j)
        hgw[s][i].push_back(add_seq_w(n, "hg." + std::to_string(s) + ".hg." + std::to_string(i) + "." + std::to_string(j), NB));
  }
  std::vector<std::vector<Bneck>> resw;
  for (int s = 0; s < S; ++s) resw.push_back(add_seq_w(n, "res." + std::to_string(s), NB));
  std::vector<int> fc(S), sht(S), spaf(S), fc_(S, -1), pafb(S, -1), htb(S, -1);
  for (int s = 0; s < S; ++s) fc[s] = add_conv_w(n, "fc." + std::to_string(s) + ".0", 256, 256, 1, false);
  for (int s = 0; s < S; ++s) sht[s] = add_conv_w(n, "score_ht." + std::to_string(s), Hc, 256, 1, false);
  for (int s = 0; s < S; ++s) spaf[s] = add_conv_w(n, "score_paf." + std::to_string(s), P, 256, 1, false);
  for (int s = 0; s + 1 < S; ++s) fc_[s] = add_conv_w(n, "fc_." + std::to_string(s), 256, 256, 1, false);
  for (int s = 0; s + 1 < S; ++s) pafb[s] = add_conv_w(n, "paf_score_." + std::to_string(s), 256, P, 1, false);
  for (int s = 0; s + 1 < S; ++s) htb[s] = add_conv_w(n, "ht_score_." + std::to_string(s), 256, Hc, 1, false);

  // ---- activation buffers ----
  const int X0 = add_buf(n, 8, 1, H0, W0);
  n->x0_buf = X0;
  const int S1 = add_buf(n, 64, 0, H1, W1);
  const int T1a = add_buf(n, 64, 1, H1, W1), T2a = add_buf(n, 64, 0, H1, W1);
  const int A = add_buf(n, 128, 0, H1, W1);
  const int B0 = add_buf(n, 128, 0, RH[4], RW[4]);
  const int X = add_buf(n, 256, 0, RH[4], RW[4]);
  int T1[5], T2[5], UP[5], L[5];
  for (int l = 4; l >= 0; --l) {
    T1[l] = add_buf(n, 128, 1, RH[l], RW[l]);
    T2[l] = add_buf(n, 128, 0, RH[l], RW[l]);
    UP[l] = l ? add_buf(n, 256, 0, RH[l], RW[l]) : -1;
    L[l] = l < 4 ? add_buf(n, 256, 0, RH[l], RW[l]) : -1;
  }
  const int Y = add_buf(n, 256, 0, RH[4], RW[4]);
  const int SC = add_buf(n, sc_c, 0, RH[4], RW[4]);
  n->cat_buf[0] = SC;
  for (int s = 0; s < S; ++s) n->op_save.push_back(add_buf(n, hoff + Hc, 0, RH[4], RW[4]));

  // ---- launches ----
  add_simple_op(n, OP_INPUT, "nchw_to_nhwc8", H0, W0, -1, 0, X0, 0, 3);
  add_conv1(n, H0, W0, stem, X0, 0, S1, 0, 1);  // (H0 x W0 is the INPUT size of the strided conv)
  n->ops.back().flops /= 4.0;
  plan_bneck(n, l1, H1, W1, S1, A, T1a, T2a);
  add_simple_op(n, OP_POOL, "maxpool", H1, W1, A, 0, B0, 0, 128);
  plan_bneck(n, l2, RH[4], RW[4], B0, X, T1[4], T2[4]);
  plan_bneck(n, l3, RH[4], RW[4], X, X, T1[4], T2[4]);
  for (int s = 0; s < S; ++s) {
    const std::string tag = "hg." + std::to_string(s);
    // _hour_glass_forward(lv, in), rtpose_hourglass.py:74-86; the level's result is left in UP[lv]
    struct Rec {
      rtpose_net* n;
      const std::vector<std::vector<std::vector<Bneck>>>& w;
      const int *RH, *RW, *T1, *T2, *UP, *L;
      const std::string& tag;
      void run(int lv, int in) const {
        const int H = RH[lv], W = RW[lv], Hl = RH[lv - 1], Wl = RW[lv - 1];
        plan_seq(n, w[lv - 1][0], H, W, in, UP[lv], T1[lv], T2[lv]);                                     // up1
        add_simple_op(n, OP_POOL, tag + ".pool" + std::to_string(lv), H, W, in, 0, L[lv - 1], 0, 256);
        plan_seq(n, w[lv - 1][1], Hl, Wl, L[lv - 1], L[lv - 1], T1[lv - 1], T2[lv - 1]);                 // low1
        int low = L[lv - 1];
        if (lv > 1) {
          run(lv - 1, L[lv - 1]);
          low = UP[lv - 1];
        } else {
          plan_seq(n, w[0][3], Hl, Wl, low, low, T1[0], T2[0]);                                          // low2
        }
        plan_seq(n, w[lv - 1][2], Hl, Wl, low, low, T1[lv - 1], T2[lv - 1]);                             // low3
        add_simple_op(n, OP_UPADD, tag + ".up" + std::to_string(lv), H, W, UP[lv], 0, UP[lv], 0, 256);   // up1 + up2
        n->ops.back().in_buf[1] = low;
      }
    };
    const Rec rec = {n, hgw[s], RH, RW, T1, T2, UP, L, tag};
    rec.run(4, X);
    const int H = RH[4], W = RW[4];
    plan_seq(n, resw[s], H, W, UP[4], UP[4], T1[4], T2[4]);
    add_conv1(n, H, W, fc[s], UP[4], 0, Y, 0, 1);  // fc: conv + folded bn + relu
    {
      const int cw[2] = {spaf[s], sht[s]}, in2[2] = {Y, Y}, zz[2] = {0, 0}, out2[2] = {SC, SC}, off2[2] = {0, hoff};
      add_conv_op(n, H, W, 2, cw, in2, zz, out2, off2, 0, 0);
    }
    add_simple_op(n, OP_SAVE, "save" + std::to_string(s), H, W, SC, 0, n->op_save[s], 0, hoff + Hc);
    if (s + 1 < S) {
      add_conv1(n, H, W, fc_[s], Y, 0, X, 0, 0, X);
      add_conv1(n, H, W, pafb[s], SC, 0, X, 0, 0, X);
      add_conv1(n, H, W, htb[s], SC, hoff, X, 0, 0, X);
    }
  }
}

// RTPOSE_WINOGRAD in the environment of the process: 1 (unset) = both kernel sizes in Winograd form, 0 = none,
// 3 / 7 = only that kernel size
int winograd_env() {
  const char* e = getenv("RTPOSE_WINOGRAD");
  return !e ? 1 : e[0] == '0' ? 0 : e[0] == '3' ? 3 : e[0] == '7' ? 7 : 1;
}

// the default form of the fp32 3x3 convs (RTPOSE_WINO_DEFAULT): AUTO, unless the environment says otherwise
// (RTPOSE_WINOGRAD=0|7: direct; RTPOSE_WINOGRAD3_M=2: F(2x2,3x3), =4: F(4x4,3x3) forced)
int default_winograd3() {
  const int env = winograd_env();
  const char* e3 = getenv("RTPOSE_WINOGRAD3_M");
  return (env == 1 || env == 3) ? ((e3 && e3[0] == '2') ? 1 : (e3 && e3[0] == '4') ? 4 : RTPOSE_WINO3_AUTO) : 0;
}

// channels choff.. of buffer b.  `per_channel` = 2: the split plan's buffers, whose layouts count elements, 2 per channel
rtpose_layout slice(const Buf& b, int choff, int per_channel = 1) {
  rtpose_layout l = b.lay;
  l.cstride *= per_channel;
  l.choff = choff * per_channel;
  return l;
}

// the fp32 NHWC8 buffer rtpose_net_input_view hands out and conv1_1 reads (bf16 plans: a staging buffer, converted by
// forward_prepared's input launch in the split plan)
const Buf& fp32_input_buf(const rtpose_net* net) { return net->bufs[net->bf16 ? net->x0f_buf : net->x0_buf]; }

// ---- what the two create calls share ----
int check_winograd3(const char* who, int w3) {
  if (w3 == RTPOSE_WINO_DEFAULT || w3 == 0 || w3 == 1 || w3 == 4 || w3 == RTPOSE_WINO3_AUTO) return 0;
  return fail(RTPOSE_E_INVAL, "%s: winograd3 must be RTPOSE_WINO_DEFAULT, 0, 1, 4 or RTPOSE_WINO3_AUTO", who);
}

rtpose_net* new_plan(int N, int H, int W, int winograd3, float amp_limit) {
  rtpose_net* n = new rtpose_net();
  n->N = N;
  n->H = H;
  n->W = W;
  n->n_cu = device_cu_count();
  n->w3 = winograd3 != RTPOSE_WINO_DEFAULT ? winograd3 : default_winograd3();
  n->amp_limit = amp_limit > 0.f ? amp_limit : 256.f;
  return n;
}

void decide_forms(rtpose_net* n) {
  pick_forms(n);
  mark_plane_bufs(n);
  n->forms_final = true;
}

int finish_plan(rtpose_net* n, rtpose_net** out) {
  if (!forms_need_amps(n)) decide_forms(n);  // AUTO waits for the filters (rtpose_net_finalize_weights)
  *out = n;
  return 0;
}

// a captured launch list holds the arenas' pointers, the forms and the 7x7 grids: dropped when one of them may change
void drop_graphs(rtpose_net* net) {
  for (hipGraphExec_t& g : net->gexec) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
}

}  // namespace

extern "C" {

int rtpose_net_create_opts(int N, int H, int W, const rtpose_net_options* opt, rtpose_net** out) {
  if (!out) return fail(RTPOSE_E_INVAL, "net_create: out is NULL");
  if (!opt || opt->struct_bytes < sizeof(rtpose_net_options))
    return fail(RTPOSE_E_INVAL, "net_create: options missing or struct_bytes smaller than this library's rtpose_net_options");
  const int dtype = opt->dtype;
  if (N <= 0 || H < 8 || W < 8) return fail(RTPOSE_E_INVAL, "net_create: need N>=1 and H,W>=8");
  if (dtype != RTPOSE_DTYPE_F32 && dtype != RTPOSE_DTYPE_BF16 && dtype != RTPOSE_DTYPE_BF16X3)
    return fail(RTPOSE_E_INVAL, "net_create: dtype must be RTPOSE_DTYPE_F32, _BF16 or _BF16X3");
  if (dtype != RTPOSE_DTYPE_F32 && ((H | W) & 7))
    return fail(RTPOSE_E_INVAL, "net_create: the bf16 plan needs H and W to be multiples of 8 "
                                "(crop_with_factor pads to that, im_transform.py:128-132)");
  if (int rc = check_winograd3("net_create", opt->winograd3)) return rc;
  if (opt->winograd7 != RTPOSE_WINO_DEFAULT && opt->winograd7 != 0 && opt->winograd7 != 4 && opt->winograd7 != 6 &&
      opt->winograd7 != 8 && opt->winograd7 != RTPOSE_WINO7_AUTO)
    return fail(RTPOSE_E_INVAL, "net_create: winograd7 must be RTPOSE_WINO_DEFAULT, 0, 4, 6, 8 or RTPOSE_WINO7_AUTO");
  rtpose_net* n = new_plan(N, H, W, opt->winograd3, opt->amp_limit);
  n->bf16 = dtype != RTPOSE_DTYPE_F32;
  n->split = dtype == RTPOSE_DTYPE_BF16X3;
  {
    // defaults of winograd3 (default_winograd3) and winograd7: on, unless the environment of the process says otherwise
    // (RTPOSE_WINOGRAD = 0: direct kernels everywhere, 3 / 7: only that kernel size in Winograd form; RTPOSE_WINOGRAD7_M=4: F(4,7), =8: F(8,7))
    const int env = winograd_env();
    // Round 4: the default is the GUARDED choice - per layer, the fastest form whose amplification estimate for the
    // filters actually loaded stays under amp_limit (256): nobody here has seen pose_model.pth (README.md:19), and a
    // forced F(6,7) / F(4x4,3x3) would run whatever it holds.  He-init / N(0, 0.01) filters estimate 115-120 and
    // 42-43, so the bench plan keeps its forms bit for bit; RTPOSE_WINOGRAD3_M / RTPOSE_WINOGRAD7_M force a form.
    const char* e7 = getenv("RTPOSE_WINOGRAD7_M");
    n->w7 = opt->winograd7 != RTPOSE_WINO_DEFAULT ? opt->winograd7
            : (env == 1 || env == 7)              ? ((e7 && e7[0] == '8')                     ? 8
                                                     : (e7 && (e7[0] == '4' || e7[0] == '6')) ? wino7_default_fm()
                                                                                              : RTPOSE_WINO7_AUTO)
                                                  : 0;
    // RTPOSE_W7_PERSIST=0 in the environment of the process: plans start with the split-tile launches off
    // (rtpose_net_set_persistent7 changes it per plan)
    const char* ep = getenv("RTPOSE_W7_PERSIST");
    n->persist7 = (ep && ep[0] == '0') ? 0 : 1;
  }
  build_plan(n);
  return finish_plan(n, out);
}

int rtpose_openpose_create(int N, int H, int W, const rtpose_openpose_options* opt, rtpose_net** out) {
  if (!out) return fail(RTPOSE_E_INVAL, "openpose_create: out is NULL");
  if (!opt || opt->struct_bytes < sizeof(rtpose_openpose_options))
    return fail(RTPOSE_E_INVAL, "openpose_create: options missing or struct_bytes smaller than this library's "
                                "rtpose_openpose_options");
  if (N <= 0 || H < 8 || W < 8) return fail(RTPOSE_E_INVAL, "openpose_create: need N>=1 and H,W>=8");
  if (opt->l2_stages < 2 || opt->l1_stages < 2 || opt->l2_stages > 64 || opt->l1_stages > 64)
    return fail(RTPOSE_E_INVAL, "openpose_create: l2_stages and l1_stages must be 2..64 (the forward returns the last two "
                                "stages of each, openpose.py:177)");
  if (opt->paf_channels < 1 || opt->paf_channels > 64 || opt->heat_channels < 1 || opt->heat_channels > 64)
    return fail(RTPOSE_E_INVAL, "openpose_create: paf_channels and heat_channels must be 1..64");
  if (int rc = check_winograd3("openpose_create", opt->winograd3)) return rc;
  rtpose_net* n = new_plan(N, H, W, opt->winograd3, opt->amp_limit);
  n->topo = 1;
  n->op_l2 = opt->l2_stages;
  n->op_l1 = opt->l1_stages;
  n->op_paf = opt->paf_channels;
  n->op_heat = opt->heat_channels;
  n->w7 = 0;  // no 7x7 convs
  build_plan_openpose(n);
  return finish_plan(n, out);
}

int rtpose_hourglass_create(int N, int H, int W, const rtpose_hourglass_options* opt, rtpose_net** out) {
  if (!out) return fail(RTPOSE_E_INVAL, "hourglass_create: out is NULL");
  if (!opt || opt->struct_bytes < sizeof(rtpose_hourglass_options))
    return fail(RTPOSE_E_INVAL, "hourglass_create: options missing or struct_bytes smaller than this library's "
                                "rtpose_hourglass_options");
  if (N <= 0) return fail(RTPOSE_E_INVAL, "hourglass_create: need N>=1");
  if (H < 64 || W < 64 || (H % 64) || (W % 64))
    return fail(RTPOSE_E_INVAL, "hourglass_create: H and W must be a multiple of 64 (got %d x %d): the depth-4 hourglass "
                                "halves the stride-4 map four times and adds the upsampled maps back, `out = up1 + up2` "
                                "(rtpose_hourglass.py:85), which fails in the reference too for any other size", H, W);
  if (opt->num_stacks < 1 || opt->num_stacks > 64)
    return fail(RTPOSE_E_INVAL, "hourglass_create: num_stacks must be 1..64 (forward returns the last stack's maps)");
  if (opt->num_blocks < 1 || opt->num_blocks > 16)
    return fail(RTPOSE_E_INVAL, "hourglass_create: num_blocks must be 1..16 (Bottlenecks per residual module)");
  if (opt->paf_classes < 1 || opt->paf_classes > 64 || opt->ht_classes < 1 || opt->ht_classes > 64)
    return fail(RTPOSE_E_INVAL, "hourglass_create: paf_classes and ht_classes must be 1..64");
  if (int rc = check_winograd3("hourglass_create", opt->winograd3)) return rc;
  rtpose_net* n = new_plan(N, H, W, opt->winograd3, opt->amp_limit);
  n->topo = 2;
  n->hg_stacks = opt->num_stacks;
  n->hg_blocks = opt->num_blocks;
  n->hg_paf = opt->paf_classes;
  n->hg_heat = opt->ht_classes;
  n->w7 = 0;  // the 7x7 stem has its own kernel
  build_plan_hourglass(n);
  return finish_plan(n, out);
}

int rtpose_net_create_ex(int N, int H, int W, int dtype, rtpose_net** out) {
  rtpose_net_options o;
  o.struct_bytes = sizeof(o);
  o.dtype = dtype;
  o.winograd3 = RTPOSE_WINO_DEFAULT;
  o.winograd7 = RTPOSE_WINO_DEFAULT;
  o.amp_limit = 0.f;
  return rtpose_net_create_opts(N, H, W, &o, out);
}

int rtpose_net_create(int N, int H, int W, rtpose_net** out) {
  return rtpose_net_create_ex(N, H, W, RTPOSE_DTYPE_F32, out);
}

int rtpose_net_dtype(const rtpose_net* net) {
  return !net || !net->bf16 ? RTPOSE_DTYPE_F32 : (net->split ? RTPOSE_DTYPE_BF16X3 : RTPOSE_DTYPE_BF16);
}

void rtpose_net_destroy(rtpose_net* net) {
  if (!net) return;
  for (hipEvent_t e : net->ev) (void)hipEventDestroy(e);
  drop_graphs(net);
  if (net->gev_in) (void)hipEventDestroy(net->gev_in);
  if (net->gev_out) (void)hipEventDestroy(net->gev_out);
  if (net->gstream) (void)hipStreamDestroy(net->gstream);
  delete net;
}

size_t rtpose_net_workspace_bytes(const rtpose_net* net) { return net->ws_floats * sizeof(float); }
size_t rtpose_net_weight_bytes(const rtpose_net* net) { return net->wt_floats * sizeof(float); }

int rtpose_net_bind(rtpose_net* net, void* workspace, size_t workspace_bytes, void* weights,
                    size_t weight_bytes, int zero_workspace, void* stream) {
  if (!net || !workspace || !weights) return fail(RTPOSE_E_INVAL, "net_bind: NULL argument");
  if (workspace_bytes < rtpose_net_workspace_bytes(net) || weight_bytes < rtpose_net_weight_bytes(net))
    return fail(RTPOSE_E_INVAL, "net_bind: arena too small");
  if (((uintptr_t)workspace | (uintptr_t)weights) & 255)
    return fail(RTPOSE_E_INVAL, "net_bind: arenas must be 256-byte aligned");
  const int dev = current_device();
  int rcd = check_device_ptr(workspace, dev, "net_bind", "the workspace");
  if (!rcd) rcd = check_device_ptr(weights, dev, "net_bind", "the weight arena");
  if (rcd) return rcd;
  if (device_cu_count() != net->n_cu)
    return fail(RTPOSE_E_STATE, "net_bind: the plan was created for a device of %d CUs, the current device %d has %d "
                                "(create the plan with that device current)", net->n_cu, dev, device_cu_count());
  net->device = dev;
  net->in_checked = CheckedPtr();
  drop_graphs(net);  // captured pointers are about to change
  net->forwards = 0;
  // a zeroed workspace suits either storage of a buffer; a caller-kept one is taken to hold pixel-major data with clean gaps
  net->zeroed_at_bind = zero_workspace != 0;
  for (Buf& b : net->bufs) b.stale = !zero_workspace && b.plane_px != 0;
  net->amps_read = false;
  net->seen_gen = ~0ull;
  if (forms_need_amps(net)) net->forms_final = false;
  net->ws = static_cast<float*>(workspace);
  net->wt = static_cast<float*>(weights);
  hipStream_t s = as_stream(stream);
  if (zero_workspace) RTPOSE_HIP_CHECK(hipMemsetAsync(workspace, 0, rtpose_net_workspace_bytes(net), s));
  // the hand-over flags and the device error word of the persistent 7x7 launches must start at zero whatever the
  // caller says about the rest of the workspace
  else if (!net->bf16 && net->scratch_bytes)
    RTPOSE_HIP_CHECK(hipMemsetAsync(net->ws + net->scratch_off, 0,
                                    (size_t)((char*)(conv2d_wino7_scratch_err(net->ws + net->scratch_off, net->n_cu) + 1) -
                                             (char*)(net->ws + net->scratch_off)), s));
  // channel map of the filters that read a concat buffer
  if (!net->catmap_host.empty())
    RTPOSE_HIP_CHECK(hipMemcpyAsync(net->wt + net->catmap_off, net->catmap_host.data(),
                                    net->catmap_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  RTPOSE_HIP_CHECK(hipStreamSynchronize(s));
  net->bound = true;
  return 0;
}

int rtpose_net_num_convs(const rtpose_net* net) { return (int)net->convs.size(); }

int rtpose_net_conv_info(const rtpose_net* net, int idx, char* name, int name_cap, int* cout, int* cin,
                         int* k) {
  if (!net || idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "conv_info: bad index");
  const ConvW& c = net->convs[idx];
  if (name && name_cap > 0) snprintf(name, name_cap, "%s", c.name.c_str());
  if (cout) *cout = c.cout;
  if (cin) *cin = c.cin_src;
  if (k) *k = c.k;
  return 0;
}

static int net_on_its_device(const rtpose_net* net, const char* who);

int rtpose_net_prelu_info(const rtpose_net* net, int idx, char* name, int name_cap) {
  if (!net || idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "prelu_info: bad index");
  const ConvW& c = net->convs[idx];
  if (name && name_cap > 0) snprintf(name, name_cap, "%s", c.prelu_name.c_str());
  return c.has_prelu ? 1 : 0;
}

int rtpose_net_load_prelu(rtpose_net* net, int idx, const float* slope, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_load_prelu: net not bound");
  if (idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "net_load_prelu: bad index");
  const ConvW& c = net->convs[idx];
  if (!c.has_prelu) return fail(RTPOSE_E_INVAL, "net_load_prelu: conv %d (%s) has no PReLU", idx, c.name.c_str());
  int rc = net_on_its_device(net, "net_load_prelu");
  if (!rc) rc = check_device_ptr(slope, net->device, "net_load_prelu", "the slope tensor");
  if (rc) return rc;
  RTPOSE_HIP_CHECK(hipMemcpyAsync(net->wt + c.pr_off, slope, (size_t)c.cout * sizeof(float), hipMemcpyDeviceToDevice,
                                  as_stream(stream)));
  return 0;
}

int rtpose_net_preact_info(const rtpose_net* net, int idx, char* name, int name_cap) {
  if (!net || idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "preact_info: bad index");
  const ConvW& c = net->convs[idx];
  if (name && name_cap > 0) snprintf(name, name_cap, "%s", c.preact_name.c_str());
  return c.has_preact ? 1 : 0;
}

int rtpose_net_load_preact(rtpose_net* net, int idx, const float* scale, const float* shift, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_load_preact: net not bound");
  if (idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "net_load_preact: bad index");
  const ConvW& c = net->convs[idx];
  if (!c.has_preact)
    return fail(RTPOSE_E_INVAL, "net_load_preact: conv %d (%s) has no pre-activation", idx, c.name.c_str());
  int rc = net_on_its_device(net, "net_load_preact");
  if (!rc) rc = check_device_ptr(scale, net->device, "net_load_preact", "the scale tensor");
  if (!rc) rc = check_device_ptr(shift, net->device, "net_load_preact", "the shift tensor");
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  float* dst = net->wt + c.pa_off;
  RTPOSE_HIP_CHECK(hipMemcpyAsync(dst, scale, (size_t)c.cin_src * sizeof(float), hipMemcpyDeviceToDevice, s));
  RTPOSE_HIP_CHECK(hipMemcpyAsync(dst + round_up((size_t)c.cin_packed, 64), shift, (size_t)c.cin_src * sizeof(float),
                                  hipMemcpyDeviceToDevice, s));
  return 0;
}

int rtpose_net_load_conv(rtpose_net* net, int idx, const float* w_oihw, const float* bias, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_load_conv: net not bound");
  if (idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "net_load_conv: bad index");
  int rcd = net_on_its_device(net, "net_load_conv");
  if (!rcd) rcd = check_device_ptr(w_oihw, net->device, "net_load_conv", "the filter tensor");
  if (!rcd && bias) rcd = check_device_ptr(bias, net->device, "net_load_conv", "the bias tensor");
  if (rcd) return rcd;
  const ConvW& c = net->convs[idx];
  const int32_t* map = c.cat_perm ? reinterpret_cast<const int32_t*>(net->wt + net->catmap_off) : nullptr;
  hipStream_t s = as_stream(stream);
  if (net->bf16) {
    if (c.first) {
      const int rcf = conv_first_pack_launch(w_oihw, bias, net->wt + c.w_off_first, s, 1);
      if (rcf) return rcf;
    }
    return pack_weights_bf16_launch(w_oihw, bias, c.cout, c.cin_src, c.k, map, c.cin_packed,
                                    net->wt + c.w_off[F_DIRECT], net->wt + c.b_off, net->split, s);
  }
  // every packing the arena holds for this conv (the plans that share the arena choose among them), and the
  // amplification estimate of each Winograd form; every plan on this arena re-reads them (sync_arena_generation)
  arena_bump(net->wt);
  net->amps_read = false;
  if (forms_need_amps(net)) net->forms_final = false;
  int rc = pack_weights_launch(w_oihw, bias, c.cout, c.cin_src, c.k, map, c.cin_packed, net->wt + c.w_off[F_DIRECT],
                               net->wt + c.b_off, s);
  if (rc) return rc;
  if (c.first) {
    rc = conv_first_pack_launch(w_oihw, bias, net->wt + c.w_off_first, s, 0);
    if (rc) return rc;
  }
  if (c.stem) {
    rc = conv7x7_s2_pack_launch(w_oihw, bias, net->wt + c.w_off_first, s);
    if (rc) return rc;
  }
  float* amp = net->wt + c.amp_off;
  RTPOSE_HIP_CHECK(hipMemsetAsync(amp, 0, 4 * sizeof(float), s));
  for (int f = F_DIRECT + 1; f < kForms; ++f) {
    if (!c.packed((Form)f)) continue;
    const FormInfo& fi = kForm[f];
    float* wp = net->wt + c.w_off[f];
    rc = fi.k == 3 ? rtpose_pack_conv_weights_winograd3(w_oihw, bias, c.cout, c.cin_src, fi.fm, map, c.cin_packed, wp,
                                                        net->wt + c.b_off, stream)
                   : pack_weights_wino7_launch(w_oihw, bias, c.cout, c.cin_src, map, c.cin_packed, fi.fm, wp,
                                               net->wt + c.b_off, s);
    if (!rc && fi.amp_slot >= 0)
      rc = rtpose_winograd_amplification(w_oihw, c.cout, c.cin_src, fi.k, fi.fm, amp + fi.amp_slot, stream);
    if (rc) return rc;
  }
  return 0;
}

static int read_amps(rtpose_net* net, hipStream_t s) {
  if (net->amps_read || net->bf16) return 0;
  // the estimates are written by the pack kernels of rtpose_net_load_conv on whatever stream THAT call was given -
  // possibly a sibling plan's, another stream than `s` (the arena is shared by the plans of a module).  Once per
  // weight load, so the whole device is drained rather than an event kept per arena.
  RTPOSE_HIP_CHECK(hipDeviceSynchronize());
  // one contiguous read-back of the arena span that holds the estimates would drag the packed filters along;
  // 92 small copies once per weight load are cheaper
  for (ConvW& c : net->convs)
    RTPOSE_HIP_CHECK(hipMemcpyAsync(c.amp, net->wt + c.amp_off, 4 * sizeof(float), hipMemcpyDeviceToHost, s));
  RTPOSE_HIP_CHECK(hipStreamSynchronize(s));
  net->amps_read = true;
  return 0;
}

int rtpose_net_finalize_weights(rtpose_net* net, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_finalize_weights: net not bound");
  sync_arena_generation(net);
  if (net->forms_final) return 0;
  const int rc = read_amps(net, as_stream(stream));
  if (rc) return rc;
  decide_forms(net);
  drop_graphs(net);  // a captured launch list may hold other forms
  return 0;
}

int rtpose_net_conv_numerics(rtpose_net* net, int idx, int* form, float* amp, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_conv_numerics: net not bound");
  if (idx < 0 || idx >= (int)net->convs.size()) return fail(RTPOSE_E_INVAL, "net_conv_numerics: bad index");
  int rc = rtpose_net_finalize_weights(net, stream);  // (notices a reload made through a sibling plan)
  if (!rc && amp) rc = read_amps(net, as_stream(stream));
  if (rc) return rc;
  const ConvW& c = net->convs[idx];
  if (form) *form = kForm[c.form].code;
  if (amp)
    for (int i = 0; i < 4; ++i) amp[i] = c.amp[i];
  return 0;
}

int rtpose_net_graph_active(const rtpose_net* net) {
  return net && net->graph_mode == 1 && (net->gexec[0] || net->gexec[1]) ? 1 : 0;
}

int rtpose_net_device_status(rtpose_net* net, int* error_word, void* stream) {
  if (!net || !net->bound || !error_word) return fail(RTPOSE_E_STATE, "net_device_status: net not bound / NULL argument");
  *error_word = 0;
  if (net->bf16 || !net->scratch_bytes) return 0;
  hipStream_t s = as_stream(stream);
  int* err = conv2d_wino7_scratch_err(net->ws + net->scratch_off, net->n_cu);
  RTPOSE_HIP_CHECK(hipMemcpyAsync(error_word, err, sizeof(int), hipMemcpyDeviceToHost, s));
  RTPOSE_HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int), s));
  RTPOSE_HIP_CHECK(hipStreamSynchronize(s));
  // a hand-over wait ran out: this device does not dispatch the grid the way the split tiles assume (a CU mask, a
  // co-tenant that starves it).  The maps of that forward are invalid - the caller is told - and the plan stops
  // splitting tiles: every later forward runs one block per tile (same results, bit for bit, a few per cent slower).
  if (*error_word & 1) return rtpose_net_set_persistent7(net, 0);  // (also drops captured launch lists: they hold the split-tile grids)
  return 0;
}

static void decide_guard_launch(rtpose_net* net);

int rtpose_net_output_guard_launch(rtpose_net* net) {
  if (!net) return fail(RTPOSE_E_INVAL, "net_output_guard_launch: NULL net");
  decide_guard_launch(net);
  return net->guard_op;
}

int rtpose_net_set_output_guard(rtpose_net* net, void* hip_event) {
  if (!net) return fail(RTPOSE_E_INVAL, "net_set_output_guard: NULL net");
  decide_guard_launch(net);
  net->out_guard = static_cast<hipEvent_t>(hip_event);
  return 0;
}

static void decide_guard_launch(rtpose_net* net) {
  if (net->guard_op < 0) {
    // Where a forward waits for the reader of its previous maps (the decoder of the batch before on a second stream,
    // pipeline.SideDecoder).  Default, every arithmetic: in front of the FIRST launch that writes the buffer
    // rtpose_net_output_view hands out - fp32: CATa, first written by conv4_4_CPM (its out1 channels), so the reader runs beside
    // the trunk's ~8 ms; bf16 / bf16x3: the stage-6 record, written by the last launch only.  RTPOSE_GUARD_WHOLE_FORWARD=1 (or
    // RTPOSE_GUARD_FINE=0): in FRONT of the launch list - the reader never runs beside this plan's kernels (costs 0.9 % of an
    // fp32 step, 1.1 % of a bf16 one).  History: in round 5 a decoder beside the bf16 plan's kernels returned a
    // limb score one sample off in ~1 % of the batches and bf16 plans waited in front; round 6 traced it to the packed-fp32
    // VALU instructions clang's SLP vectoriser had put into limb_assign_kernel's sample loop (wrong values in lanes 48..63
    // when the wave shares a CU with those kernels), the decoder is built without them (csrc/Makefile) and gave 0 differing
    // records in 240,000 decodes beside the bf16 forward on the box where the old build gave 342 in 48,000.
    const int target = net->bf16 ? net->save_buf[5] : net->cat_buf[0];
    net->guard_op = 0;
    for (size_t i = 0, found = 0; i < net->ops.size() && !found; ++i)
      for (int g = 0; g < 2; ++g)
        if (net->ops[i].out_buf[g] == target) {
          net->guard_op = (int)i;
          found = 1;
        }
    const char* e = getenv("RTPOSE_GUARD_WHOLE_FORWARD");
    const char* f = getenv("RTPOSE_GUARD_FINE");
    if ((e && e[0] == '1') || (f && f[0] == '0')) net->guard_op = 0;
  }
}

int rtpose_net_set_persistent7(rtpose_net* net, int enable) {
  if (!net) return fail(RTPOSE_E_INVAL, "net_set_persistent7: NULL net");
  net->persist7 = enable ? 1 : 0;
  drop_graphs(net);  // a captured launch list holds the other grids
  return 0;
}

int rtpose_net_persistent7(const rtpose_net* net) { return net && net->persist7 ? 1 : 0; }

int rtpose_net_device_status_async(rtpose_net* net, int* host_word, void* stream) {
  if (!net || !net->bound || !host_word) return fail(RTPOSE_E_STATE, "net_device_status_async: net not bound / NULL argument");
  if (net->bf16 || !net->scratch_bytes) {
    *host_word = 0;
    return 0;
  }
  hipStream_t s = as_stream(stream);
  int* err = conv2d_wino7_scratch_err(net->ws + net->scratch_off, net->n_cu);
  RTPOSE_HIP_CHECK(hipMemcpyAsync(host_word, err, sizeof(int), hipMemcpyDeviceToHost, s));
  RTPOSE_HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int), s));
  return 0;
}

int rtpose_net_set_keep_intermediates(rtpose_net* net, int keep) {
  if (!net) return fail(RTPOSE_E_INVAL, "NULL net");
  net->keep = keep ? 1 : 0;
  return 0;
}

int rtpose_net_set_profiling(rtpose_net* net, int enable) {
  if (!net) return fail(RTPOSE_E_INVAL, "NULL net");
  net->profiling = enable ? 1 : 0;
  if (enable && net->ev.empty()) {
    net->ev.resize(net->ops.size() + 1);
    for (auto& e : net->ev) RTPOSE_HIP_CHECK(hipEventCreate(&e));
  }
  net->ev_valid = false;
  return 0;
}

int rtpose_net_num_launches(const rtpose_net* net) { return (int)net->ops.size(); }

int rtpose_net_launch_executed_flops(const rtpose_net* net, int i, double* flops, int* winograd) {
  if (!net || i < 0 || i >= (int)net->ops.size()) return fail(RTPOSE_E_INVAL, "launch_executed_flops: bad index");
  const Op& o = net->ops[i];
  double fl = 0.0;
  int wino = 0;
  if (o.kind == OP_TAIL)
    for (int g = 0; g < o.ngroups; ++g)
      for (int ci : {o.conv_idx[g], o.conv2_idx[g]}) {
        const ConvW& c = net->convs[ci];
        fl += 2.0 * net->N * o.H * o.W * (double)c.cin_packed * cout_pad(c.cout);
      }
  if (o.kind == OP_CONV)
    for (int g = 0; g < o.ngroups; ++g) {
      // what the matrix pipe is issued (SQ_INSTS_MFMA x 4096 of a launch): whole tiles, padded channels and columns
      const ConvW& c = net->convs[o.conv_idx[g]];
      wino = kForm[c.form].code;
      if (c.stem) continue;  // conv7x7_s2_kernel issues no matrix instruction (v_fma_f32 only)
      if (c.first)  // conv_first_kernel (fp32 and bf16 plans: the fp32 matrix instruction either way): 8 x 32 pixel tiles, K = 28 (27 taps + a zero row), 64 columns
        fl += 2.0 * net->N * ceil_div(o.H, 8) * ceil_div(o.W, 32) * 256.0 * 28.0 * 64.0;
      else if (c.form == F_W3_2X2)  // 16 frequencies per 2 x 2 wtile
        fl += conv2d_wino_issued_flops(c.cin_packed, c.cout, net->N, o.H, o.W);
      else if (c.form == F_W3_4X4)  // 36 frequencies per 4 x 4 wtile
        fl += conv2d_wino4_issued_flops(c.cin_packed, c.cout, net->N, o.H, o.W);
      else if (c.form != F_DIRECT)  // FM + 6 frequencies x 7 rows per group of FM pixels, 32-position strips per image
        fl += conv2d_wino7_issued_flops(c.cin_packed, c.cout, net->N, o.H, o.W, o.H + 3, kForm[c.form].fm);
      else
        fl += 2.0 * net->N * o.H * o.W * (double)c.k * c.k * (double)c.cin_packed * cout_pad(c.cout);
    }
  if (flops) *flops = fl;
  if (winograd) *winograd = wino;
  return 0;
}

int rtpose_net_launch_info(rtpose_net* net, int i, float* ms, int* k, double* flops, char* name,
                           int name_cap) {
  if (!net || i < 0 || i >= (int)net->ops.size()) return fail(RTPOSE_E_INVAL, "launch_info: bad index");
  const Op& o = net->ops[i];
  if (k) *k = (o.kind == OP_CONV || o.kind == OP_TAIL) ? o.ks : 0;
  if (flops) *flops = o.flops;
  if (name && name_cap > 0) snprintf(name, name_cap, "%s", o.name.c_str());
  if (ms) {
    *ms = -1.f;
    if (net->profiling && net->ev_valid) {
      float t = 0.f;
      hipError_t e = hipEventElapsedTime(&t, net->ev[i], net->ev[i + 1]);
      if (e == hipSuccess) *ms = t;
    }
  }
  return 0;
}

static int net_forward_impl(rtpose_net* net, const float* x_nchw, void* stream);

int rtpose_net_forward(rtpose_net* net, const float* x_nchw, void* stream) {
  if (!x_nchw) return fail(RTPOSE_E_INVAL, "net_forward: x is NULL");
  return net_forward_impl(net, x_nchw, stream);
}

int rtpose_net_forward_prepared(rtpose_net* net, void* stream) { return net_forward_impl(net, nullptr, stream); }

int rtpose_net_input_view(const rtpose_net* net, float** base, rtpose_layout* layout) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_input_view: net not bound");
  const Buf& b = fp32_input_buf(net);
  if (base) *base = net->ws + b.off_floats;
  if (layout) *layout = b.lay;
  return 0;
}

static int net_run_ops(rtpose_net* net, size_t first, size_t last, const float* x_nchw, void* stream, bool prof);

// the plan's kernels go to the CURRENT device with pointers into the arenas bound on net->device
static int net_on_its_device(const rtpose_net* net, const char* who) {
  const int cur = current_device();
  if (cur == net->device) return 0;
  return fail(RTPOSE_E_STATE, "%s: the plan's arenas live on HIP device %d but the current device is %d", who,
              net->device, cur);
}

static int net_forward_impl(rtpose_net* net, const float* x_nchw, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_forward: net not bound");
  hipStream_t s = as_stream(stream);
  int rcd = net_on_its_device(net, "net_forward");
  if (!rcd && x_nchw) rcd = net->in_checked.check(x_nchw, net->device, "net_forward", "the input tensor");
  if (rcd) return rcd;
  sync_arena_generation(net);
  bool stale = false;
  for (const Buf& b : net->bufs) stale |= b.stale;
  if (!net->forms_final || stale) {
    // deciding AUTO forms reads the amplification estimates back (92 small D2H copies + a stream synchronise) and a
    // buffer that changed storage is cleared: neither may happen inside a stream capture, where the first is illegal
    // and the second would be baked into the graph
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(RTPOSE_E_STATE, "net_forward: the stream is capturing but the plan's forms are not final (weights were "
                                  "loaded since the last forward): call rtpose_net_finalize_weights and run one forward "
                                  "outside the capture first");
  }
  if (!net->forms_final) {  // AUTO forms, and the host did not call rtpose_net_finalize_weights since the last load
    const int rcf = rtpose_net_finalize_weights(net, stream);
    if (rcf) return rcf;
  }
  for (Buf& b : net->bufs) {  // buffers that changed between pixel-major and channel-plane storage (forms re-derived)
    if (!b.stale) continue;
    if (net->forwards > 0 || !net->zeroed_at_bind)
      RTPOSE_HIP_CHECK(hipMemsetAsync(net->ws + b.off_floats, 0, b.floats * sizeof(float), s));
    b.stale = false;
  }
  const bool prof = net->profiling && !net->ev.empty();
  const size_t nops = net->ops.size();
  if (net->graph_mode < 0) {
    const char* e = getenv("RTPOSE_GRAPH");
    // measured on MI355X / ROCm 7.2: replay is not faster than the 49 direct launches (batch-1 bf16
    // forward 1.16 ms vs 1.08 ms direct; batch 32 identical) - the launches are asynchronous and
    // the GPU-side dispatch cost is the same - so the graph path is opt-in (RTPOSE_GRAPH=1)
    net->graph_mode = (e && e[0] == '1') ? 1 : 0;
  }
  int rc = 0;
  if (net->graph_mode == 1 && !prof && net->forwards > 0 && nops > 1) {
    // op 0 (input conversion: its source pointer changes per call) runs on the caller's stream
    rc = net_run_ops(net, 0, 1, x_nchw, stream, false);
    if (rc) return rc;
    if (!net->gstream) {
      if (hipStreamCreateWithFlags(&net->gstream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&net->gev_in, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&net->gev_out, hipEventDisableTiming) != hipSuccess) {
        net->graph_mode = 0;
        (void)hipGetLastError();
        return net_run_ops(net, 1, nops, x_nchw, stream, false);
      }
    }
    const int slot = net->keep ? 1 : 0;
    if (!net->gexec[slot]) {
      hipGraph_t g = nullptr;
      hipError_t e = hipStreamBeginCapture(net->gstream, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        hipEvent_t guard = net->out_guard;  // not part of the captured list (see the replay below)
        net->out_guard = nullptr;
        rc = net_run_ops(net, 1, nops, nullptr, net->gstream, false);
        net->out_guard = guard;
        e = hipStreamEndCapture(net->gstream, &g);
        if (e == hipSuccess && !rc && g) e = hipGraphInstantiate(&net->gexec[slot], g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
      }
      if (e != hipSuccess || rc || !net->gexec[slot]) {  // no graphs on this runtime: direct launches from now on
        net->graph_mode = 0;
        net->gexec[slot] = nullptr;
        (void)hipGetLastError();
        return net_run_ops(net, 1, nops, x_nchw, stream, false);
      }
    }
    if (net->out_guard) RTPOSE_HIP_CHECK(hipStreamWaitEvent(s, net->out_guard, 0));  // (a replay cannot wait mid-list)
    RTPOSE_HIP_CHECK(hipEventRecord(net->gev_in, s));
    RTPOSE_HIP_CHECK(hipStreamWaitEvent(net->gstream, net->gev_in, 0));
    RTPOSE_HIP_CHECK(hipGraphLaunch(net->gexec[slot], net->gstream));
    RTPOSE_HIP_CHECK(hipEventRecord(net->gev_out, net->gstream));
    RTPOSE_HIP_CHECK(hipStreamWaitEvent(s, net->gev_out, 0));
    ++net->forwards;
    return 0;
  }
  rc = net_run_ops(net, 0, nops, x_nchw, stream, prof);
  if (rc) return rc;
  ++net->forwards;
  if (prof) {
    RTPOSE_HIP_CHECK(hipEventRecord(net->ev[nops], s));
    net->ev_valid = true;
  }
  return 0;
}

// Descriptor of group g of launch `o`.  OP_CONV: the whole conv.  OP_TAIL: what conv_tail_launch / conv_tail_bf16_launch
// take for the first and the `second` conv of the pair - the input side / the output side only, ReLU by position and
// nothing else (the launchers check what they are given, csrc/conv_desc.h).
static rtpose_conv_desc conv_desc(const rtpose_net* net, const Op& o, int g, bool second = false) {
  const bool pair = o.kind == OP_TAIL;
  const ConvW& c = net->convs[second ? o.conv2_idx[g] : o.conv_idx[g]];
  rtpose_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.w_packed = net->wt + c.w_off[c.form];
  d.bias_packed = net->wt + c.b_off;
  d.cin = c.cin_packed;
  d.cout = c.cout;
  d.k = c.k;
  if (!pair || !second) {
    const Buf& bi = net->bufs[o.in_buf[g]];
    d.in = net->ws + bi.off_floats;
    d.lin = slice(bi, o.in_choff[g], net->split ? 2 : 1);
    if (!pair) d.in_plane_pixels = bi.plane_px;
  }
  if (!pair || second) {
    const Buf& bo = net->bufs[o.out_buf[g]];
    d.out = net->ws + bo.off_floats;
    d.lout = slice(bo, o.out_choff[g], net->split && !o.out_f32 ? 2 : 1);
    if (!pair) d.out_plane_pixels = bo.plane_px;
  }
  if (pair) {
    d.relu = !second;
    return d;
  }
  d.wino_m = kForm[c.form].fm;
  d.relu = o.relu;
  d.pool = o.pool;
  d.prelu = c.has_prelu ? net->wt + c.pr_off : nullptr;
  if (c.has_preact) {
    d.in_scale = net->wt + c.pa_off;
    d.in_shift = net->wt + c.pa_off + round_up((size_t)c.cin_packed, 64);
    d.preact_cin = c.cin_src;
  }
  if (o.res_buf >= 0) {
    const Buf& br = net->bufs[o.res_buf];
    d.residual = net->ws + br.off_floats;
    d.lres = slice(br, o.res_choff);
  }
  return d;
}

static int net_run_ops(rtpose_net* net, size_t first, size_t last, const float* x_nchw, void* stream, bool prof) {
  hipStream_t s = as_stream(stream);
  const int N = net->N;
  // conv1_1 of the fp32 and bf16 plans reads fp32 itself (conv_first.hip): the NCHW image where the caller left it when
  // the image and the launch belong to the same call, else the plan's fp32 NHWC8 input buffer - filled by the caller
  // (forward_prepared) or by OP_INPUT (graph replay: the captured launch list reads the plan's own buffer)
  const bool conv1_reads_image = x_nchw && first == 0 && net->conv1_op >= 0 && (size_t)net->conv1_op < last;
  for (size_t i = first; i < last; ++i) {
    const Op& o = net->ops[i];
    if (prof) RTPOSE_HIP_CHECK(hipEventRecord(net->ev[i], s));
    if (net->out_guard && (int)i == net->guard_op) {
      RTPOSE_HIP_CHECK(hipStreamWaitEvent(s, net->out_guard, 0));
    }
    int rc = 0;
    switch (o.kind) {
      case OP_INPUT: {
        const Buf& bs = fp32_input_buf(net);
        if (net->split) {  // no conv1_1 kernel: the image, or what the caller left in the fp32 buffer, becomes hi + lo bf16
          const Buf& b = net->bufs[o.out_buf[0]];
          const rtpose_layout lb = slice(b, 0, 2);
          rc = x_nchw ? rtpose_nchw_to_layout_split(x_nchw, net->ws + b.off_floats, &lb, 3, 16, N, o.H, o.W, stream)
                      : rtpose_layout_f32_to_split(net->ws + bs.off_floats, &bs.lay, net->ws + b.off_floats, &lb, 3, 16,
                                                   N, o.H, o.W, stream);
        } else if (x_nchw && !conv1_reads_image) {
          rc = rtpose_nchw_to_layout(x_nchw, net->ws + bs.off_floats, &bs.lay, 3, 8, N, o.H, o.W, stream);
        }
        break;
      }
      case OP_CONV: {
        rtpose_conv_desc d[2] = {};
        for (int g = 0; g < o.ngroups; ++g) d[g] = conv_desc(net, o, g);
        const ConvW& c = net->convs[o.conv_idx[0]];  // grouped convs run one form (pick_forms)
        if (c.stem) {
          const Buf& bs = fp32_input_buf(net);
          rc = conv7x7_s2_launch(conv1_reads_image ? x_nchw : nullptr, net->ws + bs.off_floats, &bs.lay,
                                 net->wt + c.w_off_first, d[0].out, &d[0].lout, o.relu, N, o.H, o.W, s);
          break;
        }
        if (c.first) {
          const Buf& bs = fp32_input_buf(net);
          rc = conv_first_launch(conv1_reads_image ? x_nchw : nullptr, net->ws + bs.off_floats, &bs.lay,
                                 net->wt + c.w_off_first, d[0].out, &d[0].lout, d[0].out_plane_pixels, o.relu, N, o.H, o.W,
                                 s, net->bf16);
          break;
        }
        rc = net->bf16           ? conv2d_bf16_launch(d, o.ngroups, N, o.H, o.W, o.out_f32, net->split, s)
             : c.form == F_W3_2X2 ? conv2d_wino_launch(d, o.ngroups, N, o.H, o.W, s)
             : c.form == F_W3_4X4 ? conv2d_wino4_launch(d, o.ngroups, N, o.H, o.W, s)
             : c.form != F_DIRECT ? conv2d_wino7_launch(d, o.ngroups, N, o.H, o.W, kForm[c.form].fm,
                                                        net->persist7 ? net->ws + net->scratch_off : nullptr,  // (no scratch:
                                                        net->persist7 ? net->scratch_bytes : 0, s)             //  one block per tile)
                                  : conv2d_launch(d, o.ngroups, N, o.H, o.W, s, true);
        break;
      }
      case OP_TAIL: {
        rtpose_conv_desc d1[2], d2[2];
        for (int g = 0; g < o.ngroups; ++g) {
          d1[g] = conv_desc(net, o, g, false);
          d2[g] = conv_desc(net, o, g, true);
        }
        rc = net->bf16 ? conv_tail_bf16_launch(d1, d2, o.ngroups, N, o.H, o.W, o.out_f32, s)
                       : conv_tail_launch(d1, d2, o.ngroups, N, o.H, o.W, s);
        break;
      }
      case OP_POOL: {
        const Buf& bi = net->bufs[o.in_buf[0]];
        const Buf& bo = net->bufs[o.out_buf[0]];
        rc = rtpose_maxpool2x2(net->ws + bi.off_floats, &bi.lay, net->ws + bo.off_floats, &bo.lay, o.C,
                               N, o.H, o.W, stream);
        break;
      }
      case OP_UPADD: {
        const Buf &bu = net->bufs[o.in_buf[0]], &bl = net->bufs[o.in_buf[1]], &bo = net->bufs[o.out_buf[0]];
        rc = upsample2_add_launch(net->ws + bu.off_floats, &bu.lay, net->ws + bl.off_floats, &bl.lay,
                                  net->ws + bo.off_floats, &bo.lay, o.C, N, o.H, o.W, s);
        break;
      }
      case OP_SAVE:  // a concat slice -> the fp32 record of the stage outputs
      case OP_COPY: {
        const bool save = o.kind == OP_SAVE;
        if (save && !net->keep) break;
        const Buf& bi = net->bufs[o.in_buf[0]];
        const Buf& bo = net->bufs[o.out_buf[0]];
        rtpose_layout li = slice(bi, o.in_choff[0], save && net->split ? 2 : 1), lo = slice(bo, o.out_choff[0]);
        if (save && net->split) {
          rc = rtpose_layout_split_to_f32(net->ws + bi.off_floats, &li, net->ws + bo.off_floats, &lo, o.C, N,
                                          o.H, o.W, stream);
          break;
        }
        if (save && net->bf16) {
          rc = rtpose_layout_bf16_to_f32(net->ws + bi.off_floats, &li, net->ws + bo.off_floats, &lo, o.C, N,
                                         o.H, o.W, stream);
          break;
        }
        int words = o.C;
        if (net->bf16 && !net->split) {  // bf16 -> bf16: move channel pairs as 4-byte words
          li.cstride /= 2; li.choff /= 2; lo.cstride /= 2; lo.choff /= 2;
          words /= 2;
        }
        rc = rtpose_layout_copy(net->ws + bi.off_floats, &li, net->ws + bo.off_floats, &lo, words, N, o.H,
                                o.W, stream);
        break;
      }
    }
    if (rc) return rc;
  }
  return 0;
}

// Where the maps of stage output `which` (numbered as rtpose_net_read_output numbers them) are: in the stage records
// when `records` (keep_intermediates; a bf16 plan's last stage always), else where the stage's last launch left them -
// which only the last stages' are still there.
static int stage_output_slice(const rtpose_net* net, int which, bool records, const float** base, rtpose_layout* lay,
                              int* C) {
  int buf, choff;
  if (net->topo == 2) {  // 0 / 1: PAF / heat of the last stack; 2 + 2 s / 3 + 2 s: of stack s (records)
    const bool paf = which % 2 == 0;
    *C = paf ? net->hg_paf : net->hg_heat;
    choff = paf ? 0 : net->hg_heat_off;
    if (which < 2) {
      buf = net->cat_buf[0];  // the score buffer: the last stack wrote it last
    } else {
      if (!records) return fail(RTPOSE_E_STATE, "net_read_output: the maps of stack %d are not kept (set keep_intermediates)", which / 2 - 1);
      buf = net->op_save[which / 2 - 1];
    }
  } else if (net->topo == 1) {  // saved_for_loss flattened: the PAF stages, then the heat-map stages
    const bool paf = which < net->op_l2;
    *C = paf ? net->op_paf : net->op_heat;
    if (records) {
      buf = net->op_save[which];
      choff = 0;
    } else {
      if (which != net->op_l2 - 1 && which != net->op_l2 + net->op_l1 - 1)
        return fail(RTPOSE_E_STATE, "net_read_output: stage output %d not kept (set keep_intermediates)", which);
      buf = net->cat_buf[0];  // the stage input buffer
      choff = paf ? 128 : net->op_heat_off;
    }
  } else {
    const int stage = which / 2 + 1, br = which % 2;
    *C = br == 0 ? 38 : 19;
    if (records || (net->bf16 && stage == 6)) {
      buf = net->save_buf[stage - 1];
      choff = br == 0 ? 0 : 38;
    } else {
      if (net->bf16)
        return fail(RTPOSE_E_STATE, "net_read_output: bf16 plan keeps only stage 6 (set keep_intermediates)");
      if (stage < 5) return fail(RTPOSE_E_STATE, "net_read_output: stage %d not kept (set keep_intermediates)", stage);
      buf = (stage % 2 == 0) ? net->cat_buf[0] : net->cat_buf[1];  // (stage 6 writes CATa)
      choff = br == 0 ? kCatPaf : kCatHeat;
    }
  }
  const Buf& b = net->bufs[buf];
  *base = net->ws + b.off_floats;
  *lay = slice(b, choff);
  return 0;
}

int rtpose_net_read_output(rtpose_net* net, int which, float* dst_nchw, void* stream) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_read_output: net not bound");
  if (which < 0 || which >= (net->topo == 2 ? 2 + 2 * net->hg_stacks : net->topo == 1 ? net->op_l2 + net->op_l1 : 12) ||
      !dst_nchw)
    return fail(RTPOSE_E_INVAL, "net_read_output: bad argument");
  int rcd = net_on_its_device(net, "net_read_output");
  if (!rcd) rcd = check_device_ptr(dst_nchw, net->device, "net_read_output", "the destination tensor");
  if (rcd) return rcd;
  const float* src;
  rtpose_layout l;
  int C;
  if (int rc = stage_output_slice(net, which, net->keep != 0, &src, &l, &C)) return rc;
  return rtpose_layout_to_nchw(src, &l, dst_nchw, C, net->N, net->H3, net->W3, stream);
}

int rtpose_net_output_view(const rtpose_net* net, int which, const float** base, rtpose_layout* layout,
                           int* C, int* H, int* W) {
  if (!net || !net->bound || which < 0 || which > 1) return fail(RTPOSE_E_INVAL, "output_view: bad argument");
  // the last PAF / heat maps, where the last stage's launch writes them whether records are kept or not
  const int last = net->topo == 2   ? which
                   : net->topo == 1 ? (which == 0 ? net->op_l2 : net->op_l2 + net->op_l1) - 1
                                    : 10 + which;
  const float* b;
  rtpose_layout l;
  int c;
  if (int rc = stage_output_slice(net, last, false, &b, &l, &c)) return rc;
  if (base) *base = b;
  if (layout) *layout = l;
  if (C) *C = c;
  if (H) *H = net->H3;
  if (W) *W = net->W3;
  return 0;
}

int rtpose_net_stage_view(const rtpose_net* net, int which, const float** base, rtpose_layout* layout, int* C, int* H,
                          int* W) {
  if (!net || !net->bound) return fail(RTPOSE_E_STATE, "net_stage_view: net not bound");
  if (which < 0 || which >= (net->topo == 2 ? 2 + 2 * net->hg_stacks : net->topo == 1 ? net->op_l2 + net->op_l1 : 12))
    return fail(RTPOSE_E_INVAL, "net_stage_view: bad argument");
  const float* b;
  rtpose_layout l;
  int c;
  if (int rc = stage_output_slice(net, which, net->keep != 0, &b, &l, &c)) return rc;
  if (base) *base = b;
  if (layout) *layout = l;
  if (C) *C = c;
  if (H) *H = net->H3;
  if (W) *W = net->W3;
  return 0;
}

}  // extern "C"
