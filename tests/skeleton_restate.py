"""Host restatement of the table-driven decoder (csrc/decode.hip): PAF scoring, greedy assignment and grouping in
plain numpy / np.float32 with the skeleton's tables as arguments - what oracle/post_oracle.c states for COCO-18, generalised
to P parts and a limb list - plus the scene sets the skeleton tests share (rendered by the package's
synth.render_skeleton: Gaussians and limb fields the way synth.render draws them, + U(0, noise) noise).

Not product code: tests/test_skeleton_cpu.py checks it against the C oracle (COCO-18 tables) and checks, on the CPU, that
every scene set has something to get wrong (humans, row merges, refused seeds, overflow at small capacities);
tests/test_skeleton_gpu.py compares the device records with it bit for bit.

NMS is oracle.post_oracle.nms (generic in the part count).  Exact score ties inside a limb's candidate list raise TieError:
the order the reference's std::sort leaves them in is covered by the COCO-18 equality test of the two entry points, where
the compiled oracle replays it - not here.

Float arithmetic: every operation below is a single IEEE float32 (or float64) numpy operation in the order of
pafprocess.cpp / post_oracle.c; numpy does not contract a * b + c.
"""
import numpy as np

F = np.float32


class TieError(RuntimeError):
    pass


def _synth():
    import importlib
    return importlib.import_module("pytorch_realtime_multi-person_pose_estimation_amd.synth")


# ---- tables ---------------------------------------------------------------------------------------------------------
class Table(object):
    """A skeleton as plain data: P, limbs [(A, B, PAF x, PAF y)], seed mask, channel counts of the maps."""

    def __init__(self, name, num_parts, limbs, seed_mask=None, background=True, template=None):
        self.name, self.P = name, int(num_parts)
        self.num_parts = self.P
        self.limbs = [tuple(int(v) for v in l) for l in limbs]
        self.L = len(self.limbs)
        self.seed_mask = (1 << self.L) - 1 if seed_mask is None else int(seed_mask)
        self.heat_channels = self.P + (1 if background else 0)
        self.paf_channels = 1 + max(max(l[2], l[3]) for l in self.limbs)
        self.template = template

    def skeleton(self, pkg_skeleton):
        """The product's Skeleton for this table (pkg_skeleton = the package's skeleton module)."""
        return pkg_skeleton.Skeleton.from_mask(self.name, ["p%d" % i for i in range(self.P)], self.limbs, self.seed_mask,
                                               background=self.heat_channels > self.P)


COCO18_LIMBS = [(1, 2, 12, 13), (1, 5, 20, 21), (2, 3, 14, 15), (3, 4, 16, 17), (5, 6, 22, 23), (6, 7, 24, 25), (1, 8, 0, 1),
                (8, 9, 2, 3), (9, 10, 4, 5), (1, 11, 6, 7), (11, 12, 8, 9), (12, 13, 10, 11), (1, 0, 28, 29), (0, 14, 30, 31),
                (14, 16, 34, 35), (0, 15, 32, 33), (15, 17, 36, 37), (2, 16, 18, 19), (5, 17, 26, 27)]
BODY25_LIMBS = [(1, 8, 0, 1), (1, 2, 14, 15), (1, 5, 22, 23), (2, 3, 16, 17), (3, 4, 18, 19), (5, 6, 24, 25), (6, 7, 26, 27),
                (8, 9, 6, 7), (9, 10, 2, 3), (10, 11, 4, 5), (8, 12, 8, 9), (12, 13, 10, 11), (13, 14, 12, 13),
                (1, 0, 30, 31), (0, 15, 32, 33), (15, 17, 36, 37), (0, 16, 34, 35), (16, 18, 38, 39), (2, 17, 20, 21),
                (5, 18, 28, 29), (14, 19, 40, 41), (19, 20, 42, 43), (14, 21, 44, 45), (11, 22, 46, 47), (22, 23, 48, 49),
                (11, 24, 50, 51)]

# standing figures in unit coordinates (x right, y down); only used to put peaks somewhere plausible
_COCO_TEMPLATE = np.array([[0.00, -0.80], [0.00, -0.60], [-0.18, -0.58], [-0.26, -0.32], [-0.28, -0.08], [0.18, -0.58],
                           [0.26, -0.32], [0.28, -0.08], [-0.11, -0.05], [-0.12, 0.35], [-0.12, 0.75], [0.11, -0.05],
                           [0.12, 0.35], [0.12, 0.75], [-0.04, -0.84], [0.04, -0.84], [-0.09, -0.80], [0.09, -0.80]])
_BODY25_TEMPLATE = np.array([[0.00, -0.80], [0.00, -0.60], [-0.18, -0.58], [-0.26, -0.32], [-0.28, -0.08], [0.18, -0.58],
                             [0.26, -0.32], [0.28, -0.08], [0.00, -0.05], [-0.11, -0.03], [-0.12, 0.35], [-0.12, 0.72],
                             [0.11, -0.03], [0.12, 0.35], [0.12, 0.72], [-0.04, -0.84], [0.04, -0.84], [-0.09, -0.80],
                             [0.09, -0.80], [0.20, 0.82], [0.26, 0.78], [0.10, 0.80], [-0.20, 0.82], [-0.26, 0.78],
                             [-0.10, 0.80]])


def _grid_template(P, seed):
    """P points scattered over a standing figure's box, at least 0.12 apart (distinct peaks at every scale used)."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < P:
        c = np.array([rng.uniform(-0.32, 0.32), rng.uniform(-0.85, 0.8)])
        if all(np.hypot(*(c - q)) >= 0.12 for q in pts):
            pts.append(c)
    return np.array(pts)


def _full32_limbs():
    """32 limbs over 32 parts: a chain i -> i + 1 in a shuffled order (many partial rows that later limbs merge), PAF
    channel pairs neither adjacent nor ordered: x = 63 - l, y = l."""
    order = np.random.default_rng(32).permutation(31)
    limbs = [(int(i), int(i) + 1) for i in order] + [(0, 31)]
    return [(a, b, 63 - l, l) for l, (a, b) in enumerate(limbs)]


TABLES = {
    "coco18": Table("coco18", 18, COCO18_LIMBS, 0x3FFFF, template=_COCO_TEMPLATE),
    "body25": Table("body25", 25, BODY25_LIMBS, template=_BODY25_TEMPLATE),
    "pair2": Table("pair2", 2, [(0, 1, 0, 1)], template=np.array([[0.0, -0.5], [0.05, 0.4]])),
    "full32": Table("full32", 32, _full32_limbs(), template=_grid_template(32, 7)),
    # COCO-18's limbs walked backwards, every other limb allowed to seed: other rows are started, other rows merge
    "coco18rev": Table("coco18rev", 18, COCO18_LIMBS[::-1], 0x15555, template=_COCO_TEMPLATE),
}


# ---- scenes ---------------------------------------------------------------------------------------------------------
def random_people(rng, template, n_people, height, width, drop_prob=0.1):
    return _synth().spaced_people(rng, template, n_people, height, width, drop_prob)


def render(table, people, height, width, stride=8, noise=0.02, rng=None):
    """The package's synth.render_skeleton (synth.render's formulas for any table, + U(0, noise) noise)."""
    return _synth().render_skeleton(table, people, height, width, stride, noise, rng)


def make_scenes(table, people_counts, h, w, up, seed, drop_prob=0.1):
    """Seeded scenes on h x w maps decoded at `up`: heat [N, h, w, heat_channels], paf [N, h, w, paf_channels]."""
    rng = np.random.default_rng(seed)
    heats, pafs = [], []
    for n_people in people_counts:
        people = random_people(rng, table.template, n_people, h * up, w * up, drop_prob)
        hm, pf = render(table, people, h * up, w * up, stride=up, rng=rng)
        heats.append(hm)
        pafs.append(pf)
    return np.stack(heats), np.stack(pafs)


# The scene sets of the GPU tests: (table, people per image, map h, map w, up, seed).  46 x 46 and 23 x 31 maps, N <= 4,
# up 8 / 4 (the power-of-two path, stride-8 and stride-4 models) and 6 (the other path).  Every set has an image with more
# than 4 people, so a 4-peak table overflows.
SCENE_SETS = {
    "body25": ("body25", (6, 2, 7), 46, 46, 8, 6),
    "pair2": ("pair2", (7, 3), 23, 31, 4, 12),
    "full32": ("full32", (5, 7, 1, 6), 46, 46, 6, 5),
    "coco18rev": ("coco18rev", (6, 3, 7), 46, 46, 8, 14),
}

_scene_cache = {}


def scene_set(name):
    """-> (table, heat, paf, up), computed once and handed out read-only."""
    if name not in _scene_cache:
        tname, counts, h, w, up, seed = SCENE_SETS[name]
        heat, paf = make_scenes(TABLES[tname], counts, h, w, up, seed)
        heat.setflags(write=False)
        paf.setflags(write=False)
        _scene_cache[name] = (TABLES[tname], heat, paf, up)
    return _scene_cache[name]


# ---- the decoder ----------------------------------------------------------------------------------------------------
def truncate_peaks(jl, P, pcap):
    """What a device table of pcap peaks per part keeps of a joint list (x, y, score, id, part): the first pcap of every part
    in scan order, ids renumbered over what is kept.  -> (joint list, overflowed)."""
    rows, over = [], False
    for p in range(P):
        blk = jl[jl[:, 4] == p]
        over |= len(blk) > pcap
        rows.append(blk[:pcap])
    out = np.concatenate(rows, 0).astype(np.float32) if rows else np.zeros((0, 5), np.float32)
    out[:, 3] = np.arange(len(out), dtype=np.float32)
    return out, over


def limb_candidates(A, B, paf, chx, chy, up, h1):
    """pafprocess.cpp:56-94 for every (a, b) of one limb at once.  A, B: int arrays [nA, 2], [nB, 2] of (x, y).
    -> crit2 float32 [nA, nB], 0 where the pair is no candidate."""
    h, w, _ = paf.shape
    ax, ay = A[:, 0][:, None], A[:, 1][:, None]
    bx, by = B[:, 0][None, :], B[:, 1][None, :]
    dx, dy = (bx - ax).astype(F), (by - ay).astype(F)
    norm = np.sqrt(dx * dx + dy * dy)
    ok = norm > 0
    safe = np.where(ok, norm, F(1))
    vx, vy = dx / safe, dy / safe
    step_x, step_y = dx / F(10), dy / F(10)
    scores = np.zeros(norm.shape, F)
    crit1 = np.zeros(norm.shape, np.int32)
    inv_up = 1.0 / float(up)
    axf, ayf = ax.astype(F), ay.astype(F)
    for i in range(10):
        fx, fy = axf + F(i) * step_x, ayf + F(i) * step_y
        lx = (fx.astype(np.float64) + 0.5).astype(np.int64)        # (int)(v + 0.5) on a double; v >= 0
        ly = (fy.astype(np.float64) + 0.5).astype(np.int64)
        sx = np.clip(np.floor(lx * inv_up).astype(np.int64), 0, w - 1)
        sy = np.clip(np.floor(ly * inv_up).astype(np.int64), 0, h - 1)
        px, py = paf[sy, sx, chx], paf[sy, sx, chy]
        s = vx * px + vy * py
        scores = scores + s
        crit1 += s > F(0.05)
    pen = np.minimum(0.5 * float(h1) / safe.astype(np.float64) - 1.0, 0.0)
    crit2 = ((scores / F(10)).astype(np.float64) + pen).astype(F)
    return np.where(ok & (crit1 > 6) & (crit2 > 0), crit2, F(0))


def process(jl, paf, table, up, hcap=None, ties="raise"):
    """Assignment + grouping of the joint list `jl` (float32 [n, 5]: x, y, score, id, part; ids = row numbers) over `paf`
    [h, w, C] with `table`.  hcap: the device's human capacity - rows are created up to max(64, 2 hcap) (rows merged away
    are not reused), humans emitted up to hcap; None = unbounded.  ties: "raise" (TieError on two candidates of one limb with
    exactly the same score) or "keep" (they stay in (a, b) order: post_oracle.process_paf(libstdcxx_sort=False)).
    -> dict(parts int32 [H, P], score float32 [H], overflow, merges, refused_seeds, rows, connections)."""
    P = table.P
    h1 = paf.shape[0] * up
    xy = jl[:, :2].astype(np.int64)            # (int) of the joint-list columns
    pscore = jl[:, 2].astype(F)
    part = jl[:, 4].astype(np.int64)
    ids = [np.flatnonzero(part == p) for p in range(P)]
    row_cap = None if hcap is None else max(64, 2 * hcap)

    conns = []
    for a, b, chx, chy in table.limbs:
        ia, ib = ids[a], ids[b]
        out = []
        if len(ia) and len(ib):
            c = limb_candidates(xy[ia], xy[ib], paf, chx, chy, up, h1)
            cand = [(c[i, j], i, j) for i in range(len(ia)) for j in range(len(ib)) if c[i, j] > 0]
            vals = [v for v, _, _ in cand]
            if ties == "raise" and len(set(np.array(vals, F).view(np.uint32).tolist())) != len(vals):
                raise TieError("limb %d-%d: two candidates with exactly the same score" % (a, b))
            cand.sort(key=lambda t: -float(t[0]))
            used_a, used_b = set(), set()
            for v, i, j in cand:
                if i in used_a or j in used_b:
                    continue
                used_a.add(i)
                used_b.add(j)
                out.append((int(ia[i]), int(ib[j]), F(v)))
        conns.append(out)

    rows, alive = [], []
    merges = refused = 0
    overflow = False
    kS, kC = P, P + 1
    for l, (p1, p2, _, _) in enumerate(table.limbs):
        for cid1, cid2, cs in conns[l]:
            f1, f2 = F(cid1), F(cid2)
            hit = [r for r in range(len(rows)) if alive[r] and (rows[r][p1] == f1 or rows[r][p2] == f2)]
            found = len(hit)
            if found == 1:
                row = rows[hit[0]]
                if row[p2] != f2:
                    row[p2] = f2
                    row[kC] = row[kC] + F(1)
                    row[kS] = row[kS] + (pscore[cid2] + cs)
            elif found == 2:
                r1, r2 = rows[hit[0]], rows[hit[1]]
                if not np.any((r1[:P] > 0) & (r2[:P] > 0)):          # cid 0 reads as absent
                    r1[:P] = r1[:P] + (r2[:P] + F(1))
                    r1[kC] = r1[kC] + r2[kC]
                    r1[kS] = r1[kS] + r2[kS]
                    r1[kS] = r1[kS] + cs
                    alive[hit[1]] = False
                    merges += 1
                else:
                    r1[p2] = f2
                    r1[kC] = r1[kC] + F(1)
                    r1[kS] = r1[kS] + (pscore[cid2] + cs)
            elif found == 0 and (table.seed_mask >> l) & 1:
                if row_cap is not None and len(rows) >= row_cap:
                    overflow = True
                    continue
                row = np.full(P + 2, -1, F)
                row[p1], row[p2] = f1, f2
                row[kC] = F(2)
                row[kS] = (pscore[cid1] + pscore[cid2]) + cs
                rows.append(row)
                alive.append(True)
            elif found == 0:
                refused += 1
    parts, score = [], []
    for r, row in enumerate(rows):
        if not alive[r] or row[kC] < F(4) or row[kS] / row[kC] < F(0.3):
            continue
        if hcap is not None and len(parts) >= hcap:
            overflow = True
            continue
        parts.append(row[:P].astype(np.int32))
        score.append(row[kS] / row[kC])
    return {"parts": np.array(parts, np.int32).reshape(-1, P), "score": np.array(score, F), "overflow": overflow,
            "merges": merges, "refused_seeds": refused, "rows": len(rows), "connections": sum(len(c) for c in conns)}


def peaks_word(P):
    return max(32, (8 + P + 3) & ~3)


def result_words(P, pcap, hcap):
    return (peaks_word(P) + 4 * P * pcap + (P + 1) * hcap + 3) & ~3


def pack_record(jl, res, table, pcap, hcap, peak_overflow, nms_only=False):
    """The record a `_skel` entry point writes for one image (header section 4a), words behind the counts left 0."""
    P = table.P
    rec = np.zeros(result_words(P, pcap, hcap), np.int32)
    flags = (1 if peak_overflow else 0) | (2 if (res is not None and res["overflow"]) else 0)
    nh = 0 if res is None else len(res["parts"])
    rec[0:7] = [len(jl), nh, flags, pcap, hcap, P, table.L]
    pk0 = peaks_word(P)
    for p in range(P):
        blk = jl[jl[:, 4] == p]
        rec[8 + p] = len(blk)
        o = pk0 + 4 * p * pcap
        words = np.stack([blk[:, 0].astype(np.int32), blk[:, 1].astype(np.int32),
                          np.ascontiguousarray(blk[:, 2], dtype=F).view(np.int32), blk[:, 3].astype(np.int32)], axis=1)
        rec[o:o + 4 * len(blk)] = words.reshape(-1)
    if not nms_only and nh:
        off = pk0 + 4 * P * pcap
        rec[off:off + P * nh] = res["parts"].reshape(-1)
        rec[off + P * hcap:off + P * hcap + nh] = res["score"].view(np.int32)
    return rec


_nms_cache = {}


def expected_block(name, pcap, hcap, nms_only=False, num_keypoints=None):
    """The record block [N, words] the device must write for scene set `name` at these capacities, + the per-image
    restatement results.  NMS once per set, shared."""
    from oracle import post_oracle
    table, heat, paf, up = scene_set(name)
    nk = table.P if num_keypoints is None else num_keypoints
    key = (name, nk)
    if key not in _nms_cache:
        _nms_cache[key] = [post_oracle.nms(heat[i], num_keypoints=nk, thr=0.1, up=up) for i in range(len(heat))]
    recs, results = [], []
    for i, full in enumerate(_nms_cache[key]):
        jl, over = truncate_peaks(full, table.P, pcap)
        res = None if nms_only else process(jl, paf[i], table, up, hcap)
        recs.append(pack_record(jl, res, table, pcap, hcap, over, nms_only))
        results.append(res)
    return np.stack(recs), results
