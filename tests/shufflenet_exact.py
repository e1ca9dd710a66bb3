"""The exact whole-net cases of the ShuffleNetV2 plans (csrc/shufflenet.hip: zc_plan, zc_columns, build): a float64
restatement of the network on FOLDED operands - the (w, b) per layer that rtpose_shufflenet_load receives, under the names
and kinds rtpose_shufflenet_layer_info reports -, the operand family 'tracer' whose every activation is a small integer, the
conditions under which == is legitimate, a table of mutations of the restatement and the shapes with the edges they reach.
torch CPU only: no GPU, no library call.  tests/test_shufflenet_exact_cpu.py asserts the conditions, the tags and the
mutations, tests/test_shufflenet_exact_gpu.py runs the cases through shufflenet.Network.

Why == holds.  Every stored activation of a tracer case is an integer of magnitude <= 256: an fp32 value and a bf16 value
(8 significant bits), so the bf16 plan's stores round nothing and its fp32 accumulation of exact products is exact while
S = sum |x| |w| + |b| of an output stays below 2^24 - in any order, over any split of K, with any number of zero-weight K
rows.  All weights and biases are bf16 values too.  Then both plans must give THE integers: the bits of the float64
restatement cast to fp32.

What a differing bit then means: a bias lost on a folded layer, a column of a slot group stored as its neighbour's, a
class-padding slot that is not zero under a weight that is, a ceil-mode window or stride-2 row taken at the wrong place, a
pixel tile that leaks across an image boundary, a stale buffer.  Every depthwise layer of the family is a SHIFT by one of
the nine taps, which pulls the zero border in: a pixel taken from the neighbouring image or from a gap that is not zero
changes the integers.  `mutations` shows on the CPU that such changes of the restatement move at least one output.

The family is sparse on purpose (a row of a pointwise layer has one +1 and, every second time, one -1): sums stay small
over 56 layers.  The +1 entries of a layer cover all its input channels where it has at least as many rows as inputs, so
that a channel is not dropped on its way; the 57 head rows take up to four of conv5's 1024 channels each."""
from collections import OrderedDict, namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LIMIT = 2 ** 24
ACT_MAX = 256                # integers up to 2^8 are bf16 values

# ---- pixel tiles of the kernels the plans launch, with the place they are stated at ----------------------------------------
PWF_BM = 64                  # csrc/pw_fused.hip:62 kPwBM, csrc/pw_fused_bf16.hip:48 kBM: 64 consecutive pixels of N*H*W per
#                              block where no depthwise conv runs in front (pw_fused.hip:109, pw_fused_bf16.hip:87: nwork)
PWF_TILE = 8                 # pw_fused.hip:67 kPwTile, pw_fused_bf16.hip:53 kTile: with a depthwise conv in front the 64
#                              pixels are an 8 x 8 tile of ONE image
UNIT_TILE = 8                # csrc/unit_bf16.hip:42 kTile: 8 x 8 output tiles per image (:502 nitems = N tiles_x tiles_y)
HEAD_PX = 32                 # csrc/pw_head.hip:41 PX: 32 consecutive pixels per work item (:357 nitems)
HEAD_PXB = 128               # csrc/pw_head_bf16.hip:46 PXB: 128 consecutive pixels per block item (:410 nitems)
LINEAR_TILES = (HEAD_PX, PWF_BM, HEAD_PXB)

WIDTH = (116, 232, 464, 1024)
STAGES = ((4, 2), (8, 1), (4, 1))          # blocks, stride of the first block
K_AFFINE, K_STEM, K_DW, K_PW = 0, 1, 2, 3  # rtpose_shufflenet_layer_info: kind


def layer_table():
    """[(name, kind, cout, cin)] in the order of the plan's layers (csrc/shufflenet.hip, build)."""
    t = [("network.0", K_AFFINE, 3, 3), ("network.1", K_STEM, 24, 3)]
    cin = 24
    for si, (nblocks, _) in enumerate(STAGES):
        h = WIDTH[si] // 2
        for b in range(nblocks):
            p = "network.%d.%d." % (3 + si, b)
            if b == 0:
                t += [(p + "conv0.0", K_DW, cin, cin), (p + "conv0.1", K_PW, h, cin), (p + "conv.0", K_PW, h, cin)]
            else:
                t += [(p + "conv.0", K_PW, h, h)]
            t += [(p + "conv.1", K_DW, h, h), (p + "conv.2", K_PW, h, h)]
        cin = WIDTH[si]
    return t + [("network.6", K_PW, 1024, 464), ("paf", K_PW, 38, 1024), ("heatmap", K_PW, 19, 1024)]


TABLE = OrderedDict((name, (kind, cout, cin)) for name, kind, cout, cin in layer_table())


def weight_shape(name):
    kind, cout, cin = TABLE[name]
    return {K_AFFINE: (3,), K_STEM: (cout, cin, 3, 3), K_DW: (cout, 1, 3, 3), K_PW: (cout, cin, 1, 1)}[kind]


# ---- the shape chain and the edges a shape reaches ---------------------------------------------------------------------------
def chain(h0, w0):
    """csrc/shufflenet.hip, build(): H0 -> stem 3x3 s2 p1 -> max-pool 3/2 ceil -> stride-2 depthwise of stage 2"""
    g = SimpleNamespace(H0=h0, W0=w0)
    g.H1, g.W1 = (h0 - 1) // 2 + 1, (w0 - 1) // 2 + 1
    g.H2, g.W2 = (g.H1 - 3 + 1) // 2 + 1, (g.W1 - 3 + 1) // 2 + 1
    g.H3, g.W3 = (g.H2 - 1) // 2 + 1, (g.W2 - 1) // 2 + 1
    return g


def _spans(n, per_image, tile):
    """a tile of `tile` consecutive pixels holds pixels of two images"""
    return any((i * per_image) % tile for i in range(1, n))


EDGES = {
    # tag -> predicate(n, chain)
    "minimum": lambda n, g: g.H0 == 32 and g.W0 == 32,
    "one image": lambda n, g: n == 1,
    "H1 odd": lambda n, g: g.H1 % 2 == 1, "H1 even": lambda n, g: g.H1 % 2 == 0,
    "W1 odd": lambda n, g: g.W1 % 2 == 1, "W1 even": lambda n, g: g.W1 % 2 == 0,
    "H2 odd": lambda n, g: g.H2 % 2 == 1, "H2 even": lambda n, g: g.H2 % 2 == 0,
    "W2 odd": lambda n, g: g.W2 % 2 == 1, "W2 even": lambda n, g: g.W2 % 2 == 0,
    # the last ceil-mode window, rows 2 (H2 - 1) .. 2 (H2 - 1) + 2, ends past the conv map
    "pool window overhangs H": lambda n, g: 2 * (g.H2 - 1) + 3 > g.H1,
    "pool window overhangs W": lambda n, g: 2 * (g.W2 - 1) + 3 > g.W1,
    "pool windows fit H": lambda n, g: 2 * (g.H2 - 1) + 3 == g.H1,
    "pool windows fit W": lambda n, g: 2 * (g.W2 - 1) + 3 == g.W1,
    # the stride-2 depthwise convs of stage 2 on an odd map: the last output row / column has no row / column below it
    "stride-2 depthwise on odd H": lambda n, g: g.H2 % 2 == 1,
    "stride-2 depthwise on odd W": lambda n, g: g.W2 % 2 == 1,
    # N H3 W3 is no multiple of any linear pixel tile (pw_fused* 64, pw_head 32, pw_head_bf16 128) ...
    "stage map ragged for the linear tiles": lambda n, g: all((n * g.H3 * g.W3) % t for t in LINEAR_TILES),
    # ... and H3, W3 no multiples of the 8 x 8 tile of unit_bf16 and of pw_fused* behind a depthwise conv
    "stage map ragged for the 8 x 8 tile": lambda n, g: g.H3 % UNIT_TILE != 0 and g.W3 % PWF_TILE != 0,
    "stage-2 input map ragged": lambda n, g: (n * g.H2 * g.W2) % PWF_BM != 0,     # block 0's conv.0 runs at H2 x W2
    "a linear tile spans two images": lambda n, g: all(_spans(n, g.H3 * g.W3, t) for t in LINEAR_TILES),
    "several linear tiles": lambda n, g: n * g.H3 * g.W3 > 2 * HEAD_PXB,
    "several 8 x 8 tiles per image": lambda n, g: g.H3 > UNIT_TILE and g.W3 > UNIT_TILE,
}

# what the cases must reach between them
REQUIRED = ("minimum", "H1 odd", "H1 even", "W1 odd", "W1 even", "H2 odd", "H2 even", "W2 odd", "W2 even",
            "pool window overhangs H", "pool window overhangs W", "stride-2 depthwise on odd H", "stride-2 depthwise on odd W",
            "stage map ragged for the linear tiles", "stage map ragged for the 8 x 8 tile", "a linear tile spans two images",
            "several linear tiles", "several 8 x 8 tiles per image")

Case = namedtuple("Case", "n h w tags seed")

CASES = (
    Case(1, 32, 32, ("minimum", "one image", "H1 even", "W1 even", "H2 even", "W2 even", "pool window overhangs H",
                     "pool window overhangs W", "stage map ragged for the linear tiles", "stage map ragged for the 8 x 8 tile"), 1),
    Case(2, 33, 47, ("H1 odd", "W1 even", "H2 even", "W2 even", "pool windows fit H", "pool window overhangs W",
                     "stage map ragged for the linear tiles", "stage map ragged for the 8 x 8 tile",
                     "a linear tile spans two images"), 2),
    Case(3, 61, 75, ("H1 odd", "W1 even", "H2 odd", "W2 odd", "pool windows fit H", "pool window overhangs W",
                     "stride-2 depthwise on odd H", "stride-2 depthwise on odd W", "stage map ragged for the linear tiles",
                     "stage-2 input map ragged", "a linear tile spans two images"), 3),
    Case(2, 97, 131, ("H1 odd", "W1 even", "H2 even", "W2 odd", "pool windows fit H", "pool window overhangs W",
                      "stride-2 depthwise on odd W", "stage map ragged for the linear tiles", "stage map ragged for the 8 x 8 tile",
                      "a linear tile spans two images", "several linear tiles", "several 8 x 8 tiles per image"), 4),
    Case(5, 40, 88, ("H1 even", "W1 even", "H2 even", "W2 even", "pool window overhangs H", "pool window overhangs W",
                     "stage map ragged for the linear tiles", "stage map ragged for the 8 x 8 tile", "stage-2 input map ragged",
                     "a linear tile spans two images", "several linear tiles"), 5),
    # (none of the five sizes above has an odd W1: that takes W0 = 4 k + 1 or 4 k + 2)
    Case(2, 47, 50, ("H1 even", "W1 odd", "H2 even", "W2 even", "pool window overhangs H", "pool windows fit W",
                     "stage map ragged for the linear tiles", "stage map ragged for the 8 x 8 tile", "stage-2 input map ragged",
                     "a linear tile spans two images"), 6),
)


def case_id(c):
    return "%dx%dx%d" % (c.n, c.h, c.w)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------
def _shuffle(x, groups=2):
    n, c, h, w = x.shape
    return x.view(n, groups, c // groups, h, w).permute(0, 2, 1, 3, 4).reshape(n, c, h, w)


def apply_layer(name, x, w, b, stride=1, relu=False):
    """one folded layer in float64"""
    kind = TABLE[name][0]
    w, b = w.double(), b.double()
    if kind == K_AFFINE:
        y = x * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    elif kind == K_STEM:
        y = F.conv2d(x, w, b, 2, 1)
    elif kind == K_DW:
        y = F.conv2d(x, w, b, stride, 1, 1, x.shape[1])
    else:
        y = F.conv2d(x, w, b)
    return F.relu(y) if relu else y


def _walk(x, layer, mut=None):
    """The network (reference rtpose_shufflenetV2.py: BasicBlock :22-63, Network :80-148, the slim helpers as
    oracle/shufflenet_oracle.py infers them) over a per-layer callback layer(name, x, stride, relu, post) -> y.
    Returns (acts, paf, heat): acts holds every activation a plan stores in some form - the pooled stem, the outputs of all
    convs of a block, the block outputs after cat + shuffle, conv5 - by name.  `mut`: one site of `mutations`, applied."""
    m = mut or {}
    acts = OrderedDict()

    def L(name, z, stride=1, relu=False, post=None):
        y = layer(name, z, stride, relu, post)
        acts[name] = y
        return y

    def pool(t):
        return F.max_pool2d(t, 3, 2, 0, ceil_mode=not m.get("pool_floor"))

    def dw(name, z, stride):
        if stride == 2 and m.get("s2_odd_rows"):          # rows 1, 3, 5 .. of the stride-1 result (the last one repeated)
            y = layer(name, z, 1, False, None)
            rows = torch.clamp(2 * torch.arange((z.shape[2] - 1) // 2 + 1) + 1, max=z.shape[2] - 1)
            y = y[:, :, rows][:, :, :, ::2]
            acts[name] = y
            return y
        return L(name, z, stride)

    x = L("network.0", x.double())
    x = L("network.1", x, 2, True, pool)
    x = acts["pool"] = pool(x)
    for si, (nblocks, stride) in enumerate(STAGES):
        for b in range(nblocks):
            p = "network.%d.%d" % (3 + si, b)
            st = stride if b == 0 else 1

            def conv(z):
                z = L(p + ".conv.0", z, 1, True)
                z = dw(p + ".conv.1", z, st)
                return L(p + ".conv.2", z, 1, True)
            if b == 0:
                x1 = L(p + ".conv0.1", dw(p + ".conv0.0", x, st), 1, True)
                y = conv(x)
            else:
                half = x.shape[1] // 2
                x1 = x[:, half:] if m.get("pass_from_x2") == p else x[:, :half]
                y = conv(x[:, half:])
            if m.get("y_swap", (None,))[0] == p:
                _, i, j = m["y_swap"]
                perm = list(range(y.shape[1]))
                perm[i], perm[j] = j, i
                y = y[:, perm]
            x = torch.cat((x1, y), 1)
            if m.get("no_shuffle") != p:
                x = _shuffle(x)
            acts[p] = x
    x = L("network.6", x, 1, not m.get("conv5_no_relu"))
    paf, heat = L("paf", x), L("heatmap", x)
    if "head_col_shift" in m:                             # PAF column j stored from column j + 1
        j = m["head_col_shift"]
        paf = paf.clone()
        paf[:, j] = acts["paf"][:, j + 1]
    del acts["paf"], acts["heatmap"]
    return acts, paf, heat


def forward(ops, x, mut=None, stats=None):
    """ops: {layer name: (w, b)} folded operands (float32 or float64 tensors of the shapes weight_shape gives), x the NCHW
    image -> (acts, paf, heat) in float64.  `stats`, a dict: filled with name -> (S max, max |y|, all integers) per layer."""
    m = mut or {}
    if "ops" in m:
        ops = m["ops"](ops)

    def layer(name, z, stride, relu, post):
        w, b = ops[name]
        y = apply_layer(name, z, w, b, stride, relu)
        if stats is not None:
            s = apply_layer(name, z.abs(), w.abs(), b.abs(), stride, False)
            stats[name] = (s.max().item(), y.abs().max().item(), bool(torch.equal(y, y.round())))
        return y
    with torch.no_grad():
        return _walk(x, layer, m)


# ---- the operand family 'tracer' -------------------------------------------------------------------------------------------------
IMAGE_MAX = 8               # pixels in 1 .. 8
SHIFT_MAX = 3               # input affine: scale in {1, 2}, shift in -3 .. 3
BIAS_MAX = 2                # biases in {0, 1, 2}
HEAD_TERMS = 4
REDRAWS = 200


def _dead(y):
    """[C] bool: the channel is constant over the batch"""
    f = y.transpose(0, 1).reshape(y.shape[1], -1)
    return f.max(1).values == f.min(1).values


def _draw_rows(g, name, rows, first):
    """Sparse integer rows of layer `name` for the output channels `rows` (a LongTensor) -> (w rows, b rows).  `first`: the
    first draw of the layer - the +1 entries of a pointwise layer then cover its inputs."""
    kind, cout, cin = TABLE[name]
    r = rows.numel()
    b = torch.randint(0, BIAS_MAX + 1, (r,), generator=g).double()
    if kind == K_STEM:                                   # at most three taps of the 27, each -1 or 1
        w = torch.zeros(r, 27, dtype=torch.float64)
        pos = torch.rand(r, 27, generator=g).argsort(1)[:, :3]
        val = (2 * torch.randint(0, 2, (r, 3), generator=g) - 1).double()
        cnt = torch.randint(1, 4, (r,), generator=g)
        val = val * (torch.arange(3).view(1, 3) < cnt.view(-1, 1))
        w.scatter_(1, pos, val)
        return w.view(r, 3, 3, 3), b
    if kind == K_DW:                                     # one tap, 1: a shift by (ky - 1, kx - 1) that pulls the zero border in
        w = torch.zeros(r, 9, dtype=torch.float64)
        w.scatter_(1, torch.randint(0, 9, (r, 1), generator=g), 1.0)
        return w.view(r, 1, 3, 3), b
    head = name in ("paf", "heatmap")
    terms = HEAD_TERMS if head else 2
    pos = torch.rand(r, cin, generator=g).argsort(1)[:, :terms]          # distinct input channels
    if first and not head:
        cover = torch.cat([torch.randperm(cin, generator=g), torch.randint(0, cin, (max(cout - cin, 0),), generator=g)])[:cout]
        cover = cover[torch.randperm(cout, generator=g)]
        clash = pos[:, 1] == cover
        pos[:, 1] = torch.where(clash, pos[:, 0], pos[:, 1])
        pos[:, 0] = cover
    val = (2 * torch.randint(0, 2, (r, terms), generator=g) - 1).double()
    val[:, 0] = 1.0
    if head:
        cnt = torch.randint(1, terms + 1, (r,), generator=g)
        val = val * (torch.arange(terms).view(1, terms) < cnt.view(-1, 1))
    else:
        val[:, 1] = -1.0 * torch.randint(0, 2, (r,), generator=g)
    w = torch.zeros(r, cin, dtype=torch.float64)
    w.scatter_(1, pos, val)
    return w.view(r, cin, 1, 1), b


def image(c, seed_offset=0):
    g = torch.Generator().manual_seed(7000 + c.seed + 1000 * seed_offset)
    return torch.randint(1, IMAGE_MAX + 1, (c.n, 3, c.h, c.w), generator=g).float()


@lru_cache(maxsize=None)
def tracer(c):
    """The operands of a case: SimpleNamespace(x = image [n, 3, h, w] float32, ops = {name: (w, b)} float32, acts, paf, heat
    = the float64 restatement's results).  Rows are drawn again, on the CPU, until every channel of every activation, the pool's
    output and each of the 57 outputs is non-constant over the case's batch: no channel is exempt."""
    g = torch.Generator().manual_seed(9000 + c.seed)
    x = image(c)
    ops = {}

    def layer(name, z, stride, relu, post):
        kind, cout, cin = TABLE[name]
        if kind == K_AFFINE:
            w = torch.randint(1, 3, (3,), generator=g).double()
            b = torch.randint(-SHIFT_MAX, SHIFT_MAX + 1, (3,), generator=g).double()
            ops[name] = (w.float(), b.float())
            return apply_layer(name, z, w, b)
        w, b = _draw_rows(g, name, torch.arange(cout), True)
        for _ in range(REDRAWS):
            y = apply_layer(name, z, w, b, stride, relu)
            dead = _dead(post(y) if post else y).nonzero().flatten()
            if dead.numel() == 0:
                break
            w[dead], b[dead] = _draw_rows(g, name, dead, False)
        else:
            raise AssertionError("%s: %d channels stay constant at %s" % (name, dead.numel(), case_id(c)))
        ops[name] = (w.float(), b.float())
        return y
    with torch.no_grad():
        acts, paf, heat = _walk(x, layer)
    return SimpleNamespace(x=x, ops=ops, acts=acts, paf=paf, heat=heat)


def expected(c):
    """(PAF, heat) the plans must give, bit for bit: the float64 restatement cast to fp32 (exactly: asserted)"""
    t = tracer(c)
    out = []
    for y in (t.paf, t.heat):
        f = y.float()
        assert torch.equal(f.double(), y)
        out.append(f)
    return out


def conditions(c):
    """What tests/test_shufflenet_exact_cpu.py asserts of a case, from the restatement alone."""
    t = tracer(c)
    stats = {}
    acts, paf, heat = forward(t.ops, t.x, stats=stats)
    r = SimpleNamespace(stats=stats)
    r.same = all(torch.equal(acts[k], t.acts[k]) for k in t.acts) and torch.equal(paf, t.paf) and torch.equal(heat, t.heat)
    r.S = max(s for s, _, _ in stats.values())
    r.act_max = max(a for k, (_, a, _) in stats.items() if k not in ("paf", "heatmap", "network.0"))
    r.integers = all(i for _, _, i in stats.values()) and all(torch.equal(a, a.round()) for a in acts.values())
    r.dead = [k for k, a in list(acts.items()) + [("paf", paf), ("heatmap", heat)] if _dead(a).any()]
    r.bf16_operands = all(torch.equal(v.to(torch.bfloat16).float(), v) for k, wb in t.ops.items() if k != "network.0" for v in wb)
    r.clipped = sum(int((a == 0).sum()) for k, a in acts.items() if k.endswith(("conv.0", "conv.2", "conv0.1", "network.6")))
    return r


# ---- the door: a state dict of shufflenet.Network that folds to the operands exactly ------------------------------------------------
def state_dict(ops, template):
    """The operands as a state dict of shufflenet.Network (`template`: its state_dict(), for the keys): the integers in the
    conv weights and the BatchNorm biases; BatchNorm weight 1, running_mean 0, running_var 1 - with eps = 0 on the instance
    the fold gives s = 1 / sqrt(1 + 0) = 1, w * 1 and b - 0 * 1: the operands, bit for bit (the input BatchNorm: weight =
    the scale)."""
    sd = {}
    for name, (w, b) in ops.items():
        kind = TABLE[name][0]
        if kind == K_AFFINE:
            bn = name
            sd[bn + ".weight"] = w.clone()
        elif name in ("paf", "heatmap"):
            sd[name + ".weight"], sd[name + ".bias"] = w.clone(), b.clone()
            continue
        else:
            bn = name + ".1"
            sd[name + ".0.weight"] = w.clone()
            sd[bn + ".weight"] = torch.ones_like(b)
        sd[bn + ".bias"] = b.clone()
        sd[bn + ".running_mean"] = torch.zeros_like(b)
        sd[bn + ".running_var"] = torch.ones_like(b)
        sd[bn + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    assert set(sd) == set(template), set(sd) ^ set(template)
    assert all(sd[k].shape == template[k].shape for k in sd)
    return sd


def fold_state_dict(sd, eps):
    """Any state dict of the network -> folded operands in float64 (eval-mode BatchNorm into the conv in front of it)."""
    sd = {k: v.detach().double().cpu() for k, v in sd.items()}
    ops = {}
    for name, (kind, _, _) in TABLE.items():
        if name in ("paf", "heatmap"):
            ops[name] = (sd[name + ".weight"], sd[name + ".bias"])
            continue
        bn = name if kind == K_AFFINE else name + ".1"
        s = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + eps)
        b = sd[bn + ".bias"] - sd[bn + ".running_mean"] * s
        ops[name] = (s, b) if kind == K_AFFINE else (sd[name + ".0.weight"] * s.view(-1, 1, 1, 1), b)
    return ops


# ---- mutations of the restatement -------------------------------------------------------------------------------------------------
def _with(ops, name, w=None, b=None):
    ops = dict(ops)
    ops[name] = (ops[name][0] if w is None else w, ops[name][1] if b is None else b)
    return ops


def _move_tap(name, ch):
    def fn(ops):
        w = ops[name][0].clone()
        t = int(w[ch].flatten().argmax())
        w[ch] = 0
        w[ch].view(-1)[(t + 1) % 9] = 1.0
        return _with(ops, name, w=w)
    return fn


def _drop_bias(name, ch):
    def fn(ops):
        b = ops[name][1].clone()
        b[ch] = 0
        return _with(ops, name, b=b)
    return fn


def _sites(c, name, want):
    """channels of layer `name` to try a one-channel mutation at, from the operands of the case: `want(w row, b)`"""
    w, b = tracer(c).ops[name]
    return [ch for ch in range(w.shape[0]) if want(w[ch], b[ch])]


def mutations(c):
    """[(what, [mut, ...])]: mutations of the restatement, each as the list of sites it is tried at.  A mutation of ONE channel
    (a swap, a tap, a bias) shows at the outputs only if the channel reaches one of the at most 228 channels of conv5 that the
    heads read and is not clipped on its way, so these are tried at six sites: tests/test_shufflenet_exact_cpu.py asserts that
    the first site of every list moves an output, and at least half of the sites of a list."""
    u, v = "network.4.3", "network.5.2"                  # a unit of the 116-wide stage, a unit of the 232-wide stage
    return [
        ("two channels of a unit's y swapped inside a group of 8", [{"y_swap": (p, i, i + 1)} for p in (u, v) for i in (0, 8, 50)]),
        ("the shuffle of one unit omitted", [{"no_shuffle": u}]),
        ("the pass-through half taken from x2", [{"pass_from_x2": v}]),
        ("one depthwise tap moved by one", [{"ops": _move_tap(u + ".conv.1", ch)} for ch in range(6)]),
        ("one bias dropped in a mid-stage conv.2",
         [{"ops": _drop_bias(u + ".conv.2", ch)} for ch in _sites(c, u + ".conv.2", lambda w, b: b != 0)[:6]]),
        ("the pool with ceil_mode=False", [{"pool_floor": True}]),
        ("the stride-2 depthwise sampling odd rows", [{"s2_odd_rows": True}]),
        ("one head column shifted by one", [{"head_col_shift": 17}]),
        ("conv5's ReLU omitted", [{"conv5_no_relu": True}]),
    ]


def moves_an_output(c, mut):
    t = tracer(c)
    _, paf, heat = forward(t.ops, t.x, mut=mut)
    return paf.shape != t.paf.shape or not torch.equal(paf, t.paf) or not torch.equal(heat, t.heat)
