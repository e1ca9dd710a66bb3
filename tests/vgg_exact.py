"""The exact whole-net cases of the rtpose_vgg plans (csrc/net.hip: add_trunk, build_plan): a float64 restatement of the
network over {state_dict prefix: (w, b)}, under the names rtpose_net_conv_info reports (model0.0 .. model6_2.12), the operand
family 'tracer' whose every stored activation is a small integer, the conditions under which == is legitimate, a table of
mutations of the restatement and the shapes with the edges they reach.  torch CPU only: no GPU, no library call (the layer
table is derived from the tables of network.py, which are plain lists).  tests/test_vgg_exact_cpu.py asserts the conditions,
the tags and the mutations, tests/test_vgg_exact_gpu.py runs the cases through network.get_model('vgg19').

What the plan composes differently from the module graph, and what the restatement therefore does the module's way: the
185-channel torch.cat([L1, L2, out1], 1) never runs - the heads write slices of two ping-pong 192-channel buffers laid out
[out1 0..127 | PAF 128..165 | heat 166..184 | 7 zero], and the 185 -> 128 filters are permuted into that order in every
packing (direct, F(2x2,3x3) / F(4x4,3x3), F(4,7) / F(6,7) / F(8,7), bf16, bf16x3); both branches of a stage run as one
grouped grid; the trailing 1x1 pair is one fused launch (two through T4 / U[5] in the bf16x3 plan); pools are fused on even
maps and separate launches through A2 / B2 / C4 on odd ones; the bf16 plan's stage-6 heads write the fp32 record at
offsets {0, 38}; the records are made by OP_SAVE.

Why == holds.  Every operand of a tracer case is a small integer and a bf16 value; every stored activation and every one of
the 12 outputs is an integer of magnitude <= 256 (8 significant bits: an fp32 AND a bf16 value), and S = sum |x| |w| + |b| of
every output stays below 2^24.
* direct fp32, bf16, bf16x3: the argument of tests/conv_forward_exact.py - exact products, fp32 accumulation of integers
  below 2^24 is exact in any order, over any split of K, with any number of zero-weight K rows.  The split of bf16x3 has
  lo = 0 for these integers, so hi * hi is the product.  The bf16 stores of the activations and of the stage 1..5 heads, and
  the in-CU intermediate of the fused 1x1 pair, round nothing.  A max-pool rounds nothing.
* F(2x2,3x3) is admitted layer by layer by conv_forward_exact.wino_proof (imported, not restated) with the layer's cin, the
  largest |input| the case really has, |t| <= 1 and |b| <= 2: `conditions` runs it for every 3x3 conv.
So the fp32 plan with winograd3 = 0 / winograd7 = 0, the one with winograd3 = 1 / winograd7 = 0, the bf16 and the bf16x3 plan
must give THE integers: the bits of the restatement cast to fp32.
* F(4x4,3x3), F(4,7), F(6,7) and F(8,7) are not exact (conv_forward_exact.py: non-dyadic tables, or multipliers that pass
  2^24 quanta).  For them the check is the project's contract, |out - integers| <= 1e-3 * max(1, max |ref|) - and
  `conditions` asserts 1e-3 * max(1, max |out|) < 0.5: a wrong integer term moves an output by >= 1 and fails that bound.

What a differing bit then means: a concat channel taken from its neighbour, the PAF / heat slices swapped in one packing, a
pad channel that is not zero under a tap that is, heads read from the buffer of two stages ago, a branch run with the other
branch's filters, a pool window or a tap off by one, a bias lost, a head stored at the other's offset.  `mutations` shows on
the CPU that each of these changes of the restatement moves at least one of the 12 outputs at every shape.

The family is sparse on purpose (a row has one +1 tap and, every second time, one -1 tap): sums stay small over 47 layers in
sequence.  At the first draw the +1 taps of a layer cover all its input channels where it has at least as many rows as
inputs; the 185 -> 128 convs cover the 57 head channels first.  Taps are drawn only among offsets that can reach a pixel of
the layer's map (|dy| < H, |dx| < W): at H3 <= 3 most of the 49 offsets of a 7x7 filter see nothing but gaps."""
import importlib
from collections import OrderedDict, namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import conv_forward_exact as cfx
from conftest import PKG_NAME

LIMIT = cfx.LIMIT            # 2^24
ACT_MAX = 256                # integers up to 2^8 are bf16 values
TOL = 1e-3                   # the contract of the non-exact forms: |out - ref| <= TOL * max(1, max |ref|)
N_PAF, N_HEAT, N_OUT1 = 38, 19, 128
N_HEADS = N_PAF + N_HEAT     # 57
N_CAT = N_HEADS + N_OUT1     # 185

# ---- tiles of the kernels the plans launch on the stage map, with the place they are stated at --------------------------------
BM = cfx.BM                  # 128: csrc/conv_mfma.hip, conv_mfma_bf16.hip kBM, pixels of a strip tile
PAIR_BM = cfx.PAIR_BM        # 64: csrc/conv_tail.hip, conv_tail_bf16.hip BM, pixels of a block of the fused 1x1 pair
FIRST_TILE = cfx.FIRST_TILE  # (8, 32): csrc/conv_first.hip TH, TW
WINO_M = (2, 4)              # F(2x2,3x3), F(4x4,3x3): output tiles of m x m
WINO7_M = (4, 6, 8)          # F(m,7): runs of m output pixels along x


# ---- the layer table ------------------------------------------------------------------------------------------------------------
Layer = namedtuple("Layer", "name cout cin k relu pool")


def _sequential(prefix, table, relu_after_last):
    """the convs of network._sequential(table, relu_after_last), named by their index in the nn.Sequential"""
    out, idx = [], 0
    for i, e in enumerate(table):
        if e == 'P':
            out[-1] = out[-1]._replace(pool=True)
            idx += 1
            continue
        cin, cout, k = e
        relu = relu_after_last or i + 1 < len(table)
        out.append(Layer("%s.%d" % (prefix, idx), cout, cin, k, relu, False))
        idx += 2 if relu else 1
    return out


@lru_cache(maxsize=None)
def net():
    """SimpleNamespace(trunk = [Layer], stage = {(s, b): [Layer]}, table = OrderedDict name -> Layer in the order of
    rtpose_net_conv_info: model0, model1_1 .. model6_1, model1_2 .. model6_2), from network._VGG / _stage1 / _stage_t"""
    nw = importlib.import_module(PKG_NAME + ".network")
    r = SimpleNamespace(trunk=_sequential("model0", nw._VGG, True), stage={})
    for b, nout in ((1, N_PAF), (2, N_HEAT)):
        for s in range(1, 7):
            r.stage[(s, b)] = _sequential("model%d_%d" % (s, b), nw._stage1(nout) if s == 1 else nw._stage_t(nout), False)
    order = r.trunk + [l for b in (1, 2) for s in range(1, 7) for l in r.stage[(s, b)]]
    r.table = OrderedDict((l.name, l) for l in order)
    return r


def layer_table():
    """[(name, cout, cin, k)] in the order of the plan's convs"""
    return [(l.name, l.cout, l.cin, l.k) for l in net().table.values()]


def output_names():
    """the 12 outputs in the order of saved_for_loss: out1_1, out1_2, out2_1 .."""
    return [net().stage[(s, b)][-1].name for s in range(1, 7) for b in (1, 2)]


# ---- the shape chain and the edges a shape reaches ---------------------------------------------------------------------------
def chain(n, h0, w0):
    """csrc/net.hip, add_trunk: three floor-mode 2x2 pools; M: the pixels of the stage map over the batch; sg: what
    conv_forward_exact.geometry makes of a 7x7 stage conv (strip tiles or 2-D tiles, tile count)"""
    g = SimpleNamespace(n=n, H0=h0, W0=w0)
    g.H1, g.W1 = h0 // 2, w0 // 2
    g.H2, g.W2 = g.H1 // 2, g.W1 // 2
    g.H3, g.W3 = g.H2 // 2, g.W2 // 2
    g.M = n * g.H3 * g.W3
    g.fused = tuple(not ((h | w) & 1) for h, w in ((g.H0, g.W0), (g.H1, g.W1), (g.H2, g.W2)))    # plan_vgg_conv
    g.sg = cfx.geometry(cfx._c("conv2d", "stage", n, g.H3, g.W3, 128, 128, k=7, relu=1))
    g.sg3 = cfx.geometry(cfx._c("conv2d", "stage", n, g.H3, g.W3, 128, 128, k=3, relu=1))
    return g


def _spans(n, per_image, tile):
    """a tile of `tile` consecutive pixels holds pixels of two images"""
    return any((i * per_image) % tile for i in range(1, n))


EDGES = {
    # tag -> predicate(chain)
    "minimum": lambda g: g.H0 == 8 and g.W0 == 8,                             # rtpose_net_create_opts: H, W >= 8
    "one image": lambda g: g.n == 1,
    "7x7: every tap but the centre lies in gaps": lambda g: g.H3 == 1 and g.W3 == 1,
    "7x7 wider than the map": lambda g: 1 < g.H3 <= 3 and 1 < g.W3 <= 3,
    "multiple of 8": lambda g: not ((g.H0 | g.W0) & 7),                       # what the bf16 plans take
    "no multiple of 8": lambda g: bool((g.H0 | g.W0) & 7),
    "every pool fused": lambda g: g.fused == (True, True, True),
    "every pool unfused (A2, B2, C4)": lambda g: g.fused == (False, False, False),
    "pool 1 fused, 2 and 3 unfused (B2, C4 without A2)": lambda g: g.fused == (True, False, False),
    "only pool 3 unfused (C4 alone)": lambda g: g.fused == (True, True, False),
    "H0 odd": lambda g: g.H0 % 2 == 1, "W0 odd": lambda g: g.W0 % 2 == 1,
    "W0 even under an odd H0": lambda g: g.H0 % 2 == 1 and g.W0 % 2 == 0,
    "H1 odd": lambda g: g.H1 % 2 == 1, "W1 odd": lambda g: g.W1 % 2 == 1,
    "H1 even under an odd W1": lambda g: g.H1 % 2 == 0 and g.W1 % 2 == 1,
    "H2 odd": lambda g: g.H2 % 2 == 1, "W2 odd": lambda g: g.W2 % 2 == 1,
    "H3 odd": lambda g: g.H3 % 2 == 1, "W3 odd": lambda g: g.W3 % 2 == 1,
    "image ragged for the conv1_1 tile": lambda g: g.H0 % FIRST_TILE[0] != 0 and g.W0 % FIRST_TILE[1] != 0,
    # the stage map against every tile that runs on it: strip tiles and the pair's blocks (pixels of N H3 W3), the Winograd
    # output tiles m x m (3x3) and the runs of m along x (7x7)
    "stage map ragged for every tile": lambda g: (g.M % BM != 0 and g.M % PAIR_BM != 0
                                                  and all(g.H3 % m and g.W3 % m for m in WINO_M) and all(g.W3 % m for m in WINO7_M)),
    "stage convs run as strips": lambda g: g.sg.strip and g.sg3.strip,
    "stage convs run as 2-D tiles": lambda g: not g.sg.strip and not g.sg3.strip,
    "one strip tile holds every image": lambda g: g.n > 1 and g.sg.strip and g.sg.mtiles == 1,
    "a full strip tile and a tail": lambda g: g.sg.strip and g.M > BM and g.M % BM != 0,
    "image boundaries inside strip tiles": lambda g: g.n > 1 and g.sg.strip and _spans(g.n, g.H3 * g.W3, BM),
    "image boundaries inside the pair's blocks": lambda g: g.n > 1 and _spans(g.n, g.H3 * g.W3, PAIR_BM),
    "several blocks of the pair": lambda g: g.M > PAIR_BM,
    "PAIR_BM - 1 pixels": lambda g: g.M == PAIR_BM - 1,
}

# what the cases must reach between them
REQUIRED = ("minimum", "7x7: every tap but the centre lies in gaps", "7x7 wider than the map", "every pool fused",
            "every pool unfused (A2, B2, C4)", "pool 1 fused, 2 and 3 unfused (B2, C4 without A2)", "only pool 3 unfused (C4 alone)",
            "H0 odd", "W0 odd", "W0 even under an odd H0", "H1 odd", "W1 odd", "H1 even under an odd W1", "H2 odd", "W2 odd",
            "H3 odd", "W3 odd", "image ragged for the conv1_1 tile", "stage map ragged for every tile",
            "one strip tile holds every image", "a full strip tile and a tail", "image boundaries inside strip tiles",
            "image boundaries inside the pair's blocks", "several blocks of the pair")

Case = namedtuple("Case", "n h w tags seed")

CASES = (
    Case(4, 8, 8, ("minimum", "multiple of 8", "every pool fused", "7x7: every tap but the centre lies in gaps",
                   "H3 odd", "W3 odd", "stage map ragged for every tile", "stage convs run as 2-D tiles",
                   "image boundaries inside the pair's blocks"), 1),
    Case(5, 24, 24, ("multiple of 8", "every pool fused", "7x7 wider than the map", "H3 odd", "W3 odd",
                     "stage map ragged for every tile", "stage convs run as strips", "one strip tile holds every image",
                     "image boundaries inside strip tiles", "image boundaries inside the pair's blocks"), 2),
    Case(2, 64, 72, ("multiple of 8", "every pool fused", "W3 odd", "stage convs run as strips", "a full strip tile and a tail",
                     "image boundaries inside strip tiles", "image boundaries inside the pair's blocks",
                     "several blocks of the pair"), 3),
    Case(3, 40, 88, ("multiple of 8", "every pool fused", "H3 odd", "W3 odd", "stage map ragged for every tile",
                     "stage convs run as strips", "a full strip tile and a tail", "image boundaries inside strip tiles",
                     "image boundaries inside the pair's blocks", "several blocks of the pair"), 4),
    Case(1, 56, 40, ("one image", "multiple of 8", "every pool fused", "H3 odd", "W3 odd", "stage map ragged for every tile",
                     "stage convs run as strips"), 5),
    # fp32 only from here: the bf16 plans refuse sizes that are no multiples of 8
    Case(1, 61, 75, ("one image", "no multiple of 8", "every pool unfused (A2, B2, C4)", "H0 odd", "W0 odd", "W1 odd", "H2 odd",
                     "H3 odd", "W3 odd", "H1 even under an odd W1", "image ragged for the conv1_1 tile", "stage convs run as strips",
                     "stage map ragged for every tile", "PAIR_BM - 1 pixels"), 6),
    Case(2, 47, 50, ("no multiple of 8", "every pool unfused (A2, B2, C4)", "H0 odd", "W0 even under an odd H0", "H1 odd", "W1 odd",
                     "H2 odd", "H3 odd", "image ragged for the conv1_1 tile", "stage convs run as strips",
                     "one strip tile holds every image", "image boundaries inside strip tiles",
                     "image boundaries inside the pair's blocks"), 7),
    # (added: in every shape above the three pools are fused together or unfused together, so a plan that holds B2 / C4
    # without A2, or C4 alone - other buffer numbers behind the first unfused pool, a fused launch in front of an OP_POOL
    # one - is never built.  50 x 44 -> 25 x 22 -> 12 x 11 -> 6 x 5;  36 x 52 -> 18 x 26 -> 9 x 13 -> 4 x 6)
    Case(1, 50, 44, ("one image", "no multiple of 8", "pool 1 fused, 2 and 3 unfused (B2, C4 without A2)", "H1 odd", "W2 odd",
                     "W3 odd", "image ragged for the conv1_1 tile", "stage convs run as strips"), 8),
    Case(2, 36, 52, ("no multiple of 8", "only pool 3 unfused (C4 alone)", "H2 odd", "W2 odd", "image ragged for the conv1_1 tile",
                     "stage convs run as strips", "one strip tile holds every image", "image boundaries inside strip tiles",
                     "image boundaries inside the pair's blocks"), 9),
)
BASE_SHAPES = ((4, 8, 8), (5, 24, 24), (2, 64, 72), (3, 40, 88), (1, 56, 40), (1, 61, 75), (2, 47, 50))


def case_id(c):
    return "%dx%dx%d" % (c.n, c.h, c.w)


def by_shape(n, h, w):
    return next(c for c in CASES if (c.n, c.h, c.w) == (n, h, w))


def admits(c, dtype):
    """rtpose_net_create_opts: the bf16 and bf16x3 plans take multiples of 8 only"""
    return dtype == "fp32" or not ((c.h | c.w) & 7)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------
def apply_layer(l, x, w, b):
    y = F.conv2d(x, w.to(x.dtype), b.to(x.dtype), 1, l.k // 2)
    return F.relu(y) if l.relu else y


def _pool(x, shift):
    """max_pool2d(2), floor mode.  `shift`: the windows start at row / column 1 wherever the map's height / width is odd (an
    odd map has room for that: the output keeps its size)"""
    if shift:
        x = x[:, :, x.shape[2] % 2:, x.shape[3] % 2:]
    return F.max_pool2d(x, 2)


def _walk(x, layer, mut=None, trunk=None, resume=None):
    """The network (reference lib/network/rtpose_vgg.py:158-198, as oracle/net_oracle.py restates it) over a per-layer
    callback layer(Layer, x, post) -> y.  Returns (acts, outs): acts holds every activation a plan stores in some form - every
    conv's output after its ReLU, every pooled map as '<conv>.pool' - by name, outs the 12 stage outputs in the order of
    saved_for_loss.  `mut`: one site of `mutations`, applied.  `trunk`: the acts of an earlier walk of the same image and
    operands - the trunk is then taken from them; `resume` = (first stage to compute, the outs of that walk): the stages
    below it are taken from them too (their activations are then not in acts)."""
    m = mut or {}
    nt = net()
    acts = OrderedDict()

    def L(l, z, post=None):
        y = layer(l, z, post)
        if m.get("bump", (None,))[0] == l.name:                 # the probe of `observable`: one channel raised by 1
            y = y.clone()
            y[:, m["bump"][1]] += 1
        acts[l.name] = y
        return y

    if trunk is None:
        h = x
        npool = 0
        for l in nt.trunk:
            if l.pool:
                npool += 1
                post = (lambda t, k=npool: _pool(t, m.get("pool_shift") == k))
                h = acts[l.name + ".pool"] = post(L(l, h, post))
            else:
                h = L(l, h)
        out1 = h
    else:
        for k, v in trunk.items():
            if k.startswith("model0."):
                acts[k] = v
        out1 = acts[nt.trunk[-1].name]
    zero = torch.zeros_like(out1[:, :1])
    heads = {0: (zero.expand(-1, N_PAF, -1, -1), zero.expand(-1, N_HEAT, -1, -1))}    # what a buffer holds before stage 1
    outs = []
    for s in range(1, 7):
        if resume is not None and s < resume[0]:
            heads[s] = (resume[1][2 * s - 2], resume[1][2 * s - 1])
            outs += heads[s]
            continue
        if s == 1:
            inp = out1
        else:
            l1, l2 = heads[s - 2 if m.get("stale_heads") == s else s - 1]
            # (stage s reads CATb for even s, CATa for odd s: csrc/net.hip, build_plan)
            o1 = torch.zeros_like(out1) if (m.get("no_out1_in_cat_b") and s % 2 == 0) else out1
            inp = torch.cat([l2, l1, o1] if m.get("heads_swapped") == s else [l1, l2, o1], 1)
            if m.get("cat_neighbour", (None,))[0] in (0, s):    # (0: in every stage - the channel map is one for all)
                ch = m["cat_neighbour"][1]
                inp = inp.clone()
                inp[:, ch] = torch.cat([l1, l2, o1], 1)[:, ch + 1]
            if m.get("cat_bump", (None,))[0] in (0, s):         # the probe of `most_observable`: one channel raised by 1
                inp = inp.clone()
                inp[:, m["cat_bump"][1]] += 1
        pair = []
        for b in (1, 2):
            t = inp
            for l in nt.stage[(s, b)]:
                t = L(l, t)
            pair.append(t)
        heads[s] = tuple(pair)
        outs += pair
    if m.get("stage6_offsets_swapped"):                     # a 57-channel record [PAF 0..37 | heat 38..56] written at {38, 0}
        rec = torch.cat([outs[11], outs[10]], 1)
        outs[10], outs[11] = rec[:, :N_PAF], rec[:, N_PAF:]
    return acts, outs


def forward(ops, x, mut=None, stats=None, trunk=None, resume=None, dtype=torch.float64):
    """ops: {state_dict prefix: (w, b)} (float32 or float64, OIHW), x the NCHW image -> (acts, outs) in float64.  `stats`, a
    dict: filled with name -> (S max, max |y|, all integers, pre-activations below zero, max |input|) per layer."""
    m = mut or {}
    if "ops" in m:
        ops = m["ops"](ops)
    src = m.get("filters_from", {})

    def layer(l, z, post):
        w, b = ops[src.get(l.name, l.name)]
        if stats is None:
            return apply_layer(l, z, w, b)
        pre = apply_layer(l._replace(relu=False), z, w, b)
        y = F.relu(pre) if l.relu else pre
        s = F.conv2d(z.abs(), w.to(z.dtype).abs(), b.to(z.dtype).abs(), 1, l.k // 2)
        stats[l.name] = (s.max().item(), y.abs().max().item(), bool(torch.equal(y, y.round())), int((pre < 0).sum()),
                         z.abs().max().item())
        return y
    with torch.no_grad():
        return _walk(x.to(dtype), layer, m, trunk, resume)


# ---- the operand family 'tracer' -------------------------------------------------------------------------------------------------
IMAGE_MAX = 8               # pixels in 1 .. 8
BIAS_MAX = 2                # biases in {0, 1, 2}
REDRAWS = 400
LIVE_PART = 4               # a channel differs from its witness in at least a quarter of its elements
WITNESS = 50                # seed offset of the witness images


def _dead(y):
    """[C] bool: the channel is constant over the batch"""
    f = y.transpose(0, 1).reshape(y.shape[1], -1)
    return f.max(1).values == f.min(1).values


def reach(k, h, w):
    """(ky list, kx list): the taps of a k x k filter that reach a pixel of an h x w map from some pixel of it"""
    p = k // 2
    return [t for t in range(k) if abs(t - p) < h], [t for t in range(k) if abs(t - p) < w]


def _draw_rows(g, l, rows, first, hw, keep=None):
    """Sparse integer rows of layer `l` for the output channels `rows` (a LongTensor) on an hw map -> (w rows, b rows): one +1
    tap and, every second time, one -1 tap at another (cin, ky, kx).  `first`: the first draw of the layer - the +1 taps then
    cover its input channels (all of them where cout >= cin; of a 185 -> 128 conv the 57 head channels first).  `keep`: the
    input channels the +1 taps of the rows stay at (a redraw that moves the taps, draws the -1 tap and the bias again)."""
    r = rows.numel()
    kys, kxs = reach(l.k, *hw)
    nt = len(kys) * len(kxs)
    total = l.cin * nt
    b = torch.randint(0, BIAS_MAX + 1, (r,), generator=g).float()
    ch = torch.randint(0, l.cin, (r,), generator=g)
    if first:
        assert r == l.cout
        if l.cin == N_CAT:
            cover = torch.cat([torch.randperm(N_HEADS, generator=g), N_HEADS + torch.randperm(N_OUT1, generator=g)])[:l.cout]
        else:
            more = torch.randint(0, l.cin, (max(l.cout - l.cin, 0),), generator=g)
            cover = torch.cat([torch.randperm(l.cin, generator=g), more])[:l.cout]
        ch = cover[torch.randperm(l.cout, generator=g)]
    if keep is not None:
        ch = keep
    p0 = ch * nt + torch.randint(0, nt, (r,), generator=g)
    p1 = (p0 + torch.randint(1, total, (r,), generator=g)) % total                   # another tap
    minus = -1.0 * torch.randint(0, 2, (r,), generator=g).float()
    w = torch.zeros(r, l.cin, l.k, l.k)
    ar = torch.arange(r)
    for p, v in ((p1, minus), (p0, torch.ones(r))):
        t = p % nt
        w[ar, p // nt, torch.tensor(kys)[t // len(kxs)], torch.tensor(kxs)[t % len(kxs)]] = v
    return w, b


def image(c, seed_offset=0):
    g = torch.Generator().manual_seed(7100 + c.seed + 1000 * seed_offset)
    return torch.randint(1, IMAGE_MAX + 1, (c.n, 3, c.h, c.w), generator=g).float()


def _blind(y, n):
    """[C] bool: the channel does not see the image - fewer than 1 / LIVE_PART of its elements differ between the case's
    batch, y[:n], and the same operands on the witness images, y[n:]"""
    d = (y[:n] != y[n:]).transpose(0, 1).flatten(1).sum(1)
    return d * LIVE_PART < y[0, 0].numel() * n


def tracer(c, family=0):
    """the operands of a case, drawn once: see _tracer"""
    return _tracer(c, family)


@lru_cache(maxsize=None)
def _tracer(c, family):
    """The operands of a case: SimpleNamespace(x = image [n, 3, h, w] float32, ops = {name: (w, b)} float32, acts, outs = the
    float64 restatement's results, stats = what `forward` records of that run, drawn = the 12 outputs as the fp32 draw saw them).  Rows are drawn again, on the CPU, until every channel of every stored activation, of
    every pooled map and each of the 12 x (38 | 19) outputs (a) is non-constant over the case's batch and (b) sees the image:
    no channel is exempt.  (b): with the zero border and the biases alone a channel is non-constant, and a net of such
    channels would give nearly the same outputs for every image - a kernel that reads a wrong pixel of them would show
    nowhere.  So the walk carries a second batch of witness images along, and a channel must differ from its witness in
    at least 1 / LIVE_PART of its elements.
    `family`: another seed of both the filters and the image (tracer B of the A-B-A test)."""
    g = torch.Generator().manual_seed(9100 + c.seed + 1000 * family)
    x = image(c, family)
    ops = {}
    n = c.n

    def layer(l, z, post):
        hw = tuple(z.shape[2:])
        w, b = _draw_rows(g, l, torch.arange(l.cout), True, hw)
        y = apply_layer(l, z, w, b)
        plus = (w == 1).flatten(2).any(2).double().argmax(1)            # the input channel of each row's +1 tap
        for i in range(REDRAWS):
            seen = post(y) if post else y
            dead = (_dead(seen[:n]) | _blind(seen, n)).nonzero().flatten()
            if dead.numel() == 0:
                break
            # (the cover of the first draw is kept while that works: the row keeps its +1 channel)
            w[dead], b[dead] = _draw_rows(g, l, dead, False, hw, keep=plus[dead] if i < REDRAWS // 2 else None)
            y[:, dead] = apply_layer(l, z, w[dead], b[dead])
        else:
            raise AssertionError("%s: %d channels stay constant or blind at %s" % (l.name, dead.numel(), case_id(c)))
        ops[l.name] = (w, b)
        return y
    # (the draw itself runs in fp32, which is quick and exact for these integers; what is recorded is the float64 restatement
    # of the operands it found, and `conditions` asserts again that every channel of THAT is alive)
    with torch.no_grad():
        _, drawn = _walk(torch.cat([x, image(c, WITNESS + family)]), layer)
    stats = {}
    acts, outs = forward(ops, x, stats=stats)
    return SimpleNamespace(x=x, ops=ops, acts=acts, outs=outs, stats=stats, drawn=[o[:n] for o in drawn])


def expected(c, family=0):
    """the 12 outputs the exact plans must give, bit for bit: the float64 restatement cast to fp32 (exactly: asserted)"""
    out = []
    for y in tracer(c, family).outs:
        f = y.float()
        assert torch.equal(f.double(), y)
        out.append(f)
    return out


def expected_of(c, x, family=0):
    """the 12 outputs for another image `x` under the operands of the case, cast to fp32 (exactly: asserted)"""
    _, outs = forward(tracer(c, family).ops, x)
    assert all(torch.equal(y.float().double(), y) for y in outs)
    return [y.float() for y in outs]


def conditions(c):
    """What tests/test_vgg_exact_cpu.py asserts of a case, from the restatement alone."""
    t = tracer(c)
    stats, acts, outs = t.stats, t.acts, t.outs
    r = SimpleNamespace(stats=stats)
    r.same = all(torch.equal(a.double(), b) for a, b in zip(t.drawn, outs))      # the fp32 draw saw the float64 outputs
    r.S = max(v[0] for v in stats.values())
    r.act_max = max(max(a.abs().max().item() for a in acts.values()), float(t.x.abs().max()))
    r.out_max = max(o.abs().max().item() for o in outs)
    r.integers = all(v[2] for v in stats.values()) and all(torch.equal(a, a.round()) for a in acts.values())
    r.dead = [k for k, a in acts.items() if _dead(a).any()]
    r.bf16_operands = (all(torch.equal(v.to(torch.bfloat16).float(), v) for wb in t.ops.values() for v in wb)
                       and torch.equal(t.x.to(torch.bfloat16).float(), t.x))
    r.clipped = sum(v[3] for k, v in stats.items() if net().table[k].relu)
    # F(2x2,3x3): conv_forward_exact.wino_proof per 3x3 conv, with the layer's cin and the largest |input| the case has
    m_, r_, points, two_d, _, rows = cfx.WINO_FORMS["F(2x2,3x3)"]
    r.wino = {}
    for l in net().table.values():
        if l.k != 3:
            continue
        mult, stages, dyadic = cfx.wino_proof(m_, r_, points, two_d, (l.cin + 7) // 8 * 8, rows, x_max=stats[l.name][4], t_max=1,
                                              b_max=BIAS_MAX)
        r.wino[l.name] = mult == cfx.WINO2_C and dyadic and all(ok for _, _, _, ok in stages)
    r.tol_below_half = TOL * max(1.0, r.out_max) < 0.5
    return r


def state_dict(ops):
    """the operands under the 184 keys of network.RtposeVGG"""
    sd = OrderedDict()
    for name in net().table:
        sd[name + ".weight"], sd[name + ".bias"] = ops[name][0].clone(), ops[name][1].clone()
    return sd


def ops_of(sd):
    """a state dict of the network -> {prefix: (w, b)} in float64"""
    f = lambda key: sd[key].detach().double().cpu()     # noqa: E731
    return {name: (f(name + ".weight"), f(name + ".bias")) for name in net().table}


# ---- mutations of the restatement -------------------------------------------------------------------------------------------------
def _with(ops, name, w=None, b=None):
    ops = dict(ops)
    ops[name] = (ops[name][0] if w is None else w, ops[name][1] if b is None else b)
    return ops


def _move_tap(name, ch):
    """the +1 tap of row `ch` moved by one pixel along x"""
    def fn(ops):
        w = ops[name][0].clone()
        k = w.shape[3]
        ci, ky, kx = [int(v) for v in (w[ch] == 1).nonzero()[0]]
        w[ch, ci, ky, kx] -= 1
        w[ch, ci, ky, kx + 1 if kx + 1 < k else kx - 1] += 1
        return _with(ops, name, w=w)
    return fn


def _drop_bias(name, ch):
    def fn(ops):
        b = ops[name][1].clone()
        b[ch] = 0
        return _with(ops, name, b=b)
    return fn


def read_rows(c, name):
    """{output channel of layer `name`} that some tap of the rest of its branch leads from to the branch's head: a change of
    any other channel cannot show (structurally; a ReLU or a gap may still hide one of these)"""
    t = tracer(c)
    branch = next(ls for ls in net().stage.values() if any(l.name == name for l in ls))
    need = None
    for l in reversed(branch):
        if l.name == name:
            break
        w = t.ops[l.name][0]
        rows = w if need is None else w[sorted(need)]
        need = set((rows != 0).flatten(2).any(2).any(0).nonzero().flatten().tolist())
    return sorted(need) if need is not None else list(range(net().table[name].cout))


def read_cat_channels(c, s):
    """concat channels that a first conv of stage s reads in a row that leads on to its head"""
    t = tracer(c)
    out = set()
    for b in (1, 2):
        l = net().stage[(s, b)][0]
        w = t.ops[l.name][0][read_rows(c, l.name)]
        out |= set((w != 0).flatten(2).any(2).any(0).nonzero().flatten().tolist())
    return sorted(out)


def most_observable(c, candidates, probe, tries=8):
    """[the one of the first `tries` candidates whose probes move the most output elements], [] if none moves any"""
    score = [(min(moved_elements(c, p) for p in probe(ch)), -ch) for ch in candidates[:tries]]
    return [-max(score)[1]] if score and max(score)[0] > 0 else []


def observable(c, candidates, probe, want=6, tries=64):
    """The first `want` of `candidates` (channels) at which the probe - the channel raised by 1 at every pixel, probe(ch) says
    where - moves one of the 12 outputs.  A change of one channel shows only if some chain of taps leads from it to a head
    without leaving the map (on a 3 x 3 map a 7x7 tap shifts most pixels out) and no ReLU clips it on the way; whether it
    does is a property of the operands, and a mutation at a channel that nothing observes says nothing about the outputs."""
    out = []
    for ch in candidates[:tries]:
        if all(moves_an_output(c, p) for p in probe(ch)):
            out.append(ch)
            if len(out) == want:
                break
    return out


@lru_cache(maxsize=None)
def mutations(c):
    """[(what, [mut, ...])]: mutations of the restatement, each as the list of sites it is tried at.  A mutation of ONE channel
    (a concat channel, a tap, a bias) is tried at channels that `read_rows` admits and `observable` / `most_observable` find:
    tests/test_vgg_exact_cpu.py asserts that the first site of every list moves an output, and at least half of the sites
    of a list."""
    t = tracer(c)
    g = chain(c.n, c.h, c.w)
    cat = []
    # The channel map of the concat is one for all 185 -> 128 convs (csrc/net.hip: catmap_host), so a wrong entry shows in
    # every stage (stage 0 below); a wrong channel in ONE packing of one stage's filters in that stage alone.  Channels: PAF,
    # the PAF / heat border, heat, the heat / out1 border, out1.
    for s, lo, hi in ((0, 0, N_PAF - 1), (0, N_PAF - 1, N_PAF), (0, N_PAF, N_HEADS - 1), (0, N_HEADS - 1, N_HEADS),
                      (0, N_HEADS, N_CAT - 1), (2, 0, N_HEADS - 1), (4, 0, N_HEADS - 1), (6, 0, N_HEADS - 1)):
        read = sorted(set().union(*(read_cat_channels(c, k) for k in (range(2, 7) if s == 0 else (s,)))))
        ch = most_observable(c, [k for k in read if lo <= k < hi], lambda k, s=s: [{"cat_bump": (s, k)}])
        assert ch, "%s: no observable concat channel in %d .. %d of stage %d (0: all)" % (case_id(c), lo, hi - 1, s)
        cat += [{"cat_neighbour": (s, k)} for k in ch]

    def sites(name, want=lambda ch: True):
        return observable(c, [ch for ch in read_rows(c, name) if want(ch)], lambda ch: [{"bump": (name, ch)}])
    table = [
        ("stage t's first conv reads heat where PAF is and PAF where heat is", [{"heads_swapped": s} for s in (2, 5)]),
        ("one concat channel read from its neighbour", cat),
        ("stage s reads the heads of stage s - 2 (the stale ping-pong buffer)", [{"stale_heads": s} for s in (2, 3, 6)]),
        ("out1 missing from the second concat buffer", [{"no_out1_in_cat_b": True}]),
        ("the branch-2 filters of one layer applied in branch 1",
         [{"filters_from": {"model%d_1.%d" % (s, i): "model%d_2.%d" % (s, i)}} for s, i in ((1, 2), (2, 0), (4, 6), (6, 10))]),
        ("a 3x3 tap moved by one pixel", [{"ops": _move_tap("model1_2.4", ch), "stage": 1} for ch in sites("model1_2.4")]),
        ("a 7x7 tap moved by one pixel", [{"ops": _move_tap("model3_1.8", ch), "stage": 3} for ch in sites("model3_1.8")]),
        ("a bias dropped", [{"ops": _drop_bias("model4_2.10", ch), "stage": 4}
                            for ch in sites("model4_2.10", lambda ch: t.ops["model4_2.10"][1][ch] != 0)]),
        ("the stage-6 heads stored at each other's offset", [{"stage6_offsets_swapped": True}]),
    ]
    odd = [k + 1 for k, f in enumerate(g.fused) if not f]
    if odd:
        table.append(("a pool window shifted by one on an odd map", [{"pool_shift": k} for k in odd]))
    return table


def first_stage(mut):
    """the first stage whose outputs a mutation can move (None: the trunk)"""
    stage_of = lambda name: int(name[5])     # noqa: E731  'model<s>_<b>.<i>'
    for key, fn in (("heads_swapped", lambda v: v), ("cat_neighbour", lambda v: v[0] or 2), ("cat_bump", lambda v: v[0] or 2),
                    ("stale_heads", lambda v: v), ("no_out1_in_cat_b", lambda v: 2), ("filters_from", lambda v: min(map(stage_of, v))),
                    ("bump", lambda v: stage_of(v[0])), ("stage", lambda v: v), ("stage6_offsets_swapped", lambda v: 6)):
        if key in mut:
            return fn(mut[key])
    return None


@lru_cache(maxsize=None)
def _tracer32(c):
    t = tracer(c)
    return SimpleNamespace(acts={k: v.float() for k, v in t.acts.items() if k.startswith("model0.")},
                           outs=[o.float() for o in t.outs])


def moves_an_output(c, mut):
    return moved_elements(c, mut) > 0


def moved_elements(c, mut):
    """How many elements of the 12 outputs a mutation moves.  (Computed in fp32, from the fp32 copies of the recorded trunk
    and of the stages below the first one the mutation can reach: exact for these integers, as `conditions` shows of the
    unmutated case - S < 2^24 -, and no mutation moves an S by more than a few units.)"""
    t, t32 = tracer(c), _tracer32(c)
    s = first_stage(mut)
    _, outs = forward(t.ops, t.x, mut=mut, trunk=None if s is None else t32.acts, resume=None if s is None else (s, t32.outs),
                      dtype=torch.float32)
    return sum(int((a != b).sum()) for a, b in zip(outs, t32.outs))
