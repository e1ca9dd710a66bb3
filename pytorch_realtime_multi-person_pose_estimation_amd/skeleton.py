"""Skeletons for the table-driven decoder (csrc/decode.hip, header section 4a).

A ``Skeleton`` is the data the `_skel` decode entry points take: the parts, the limbs as
(part A, part B, PAF x channel, PAF y channel) in the order the grouping walks them, and which
limbs may start a new person.  ``decode.decode_maps(..., skeleton=s)``,
``pipeline.PoseEstimator(model, skeleton=s)`` and ``common.draw_humans(..., skeleton=s)`` take one.

Flip merge and multi-scale TTA take one too: ``preprocess.handle_paf_and_heat``, ``get_multiscale_outputs`` and
``get_multiscale_outputs_batch`` with ``skeleton=s`` run ``rtpose_flip_merge_skel`` / ``rtpose_tta_accumulate_skel``
(csrc/tta.hip, header section 5a) over ``s.flip_tables()``: which channel of the mirrored pass every output channel
reads, and with which sign.  The tables follow from the part names (a leading ``L`` / ``R``) or an explicit ``mirror``
and from the limbs.  The TTA paths resize with ``crop_with_factor(factor=stride)``; hourglass models, whose input size
must be a multiple of 64, are out of their scope.

The way back takes one as well: ``encode.encode_targets(people, skeleton=s)`` renders people into the heat-map / PAF
targets of ``s`` on the device (csrc/encode.hip, header section 4b: the reference's get_ground_truth, fp64 operation for
operation).  ``encode.COCO18_TRAIN`` is the reference's training table, which joins shoulder to eye where ``COCO18`` below
(the decoder's, pafprocess.h) joins shoulder to ear on the same PAF channels; encode with the table the maps are for.

What a skeleton does NOT reach (COCO-18 only): the legacy ``pafprocess.process_paf`` API and its getters,
``append_result`` / the OKS evaluation (COCO-18 -> COCO-17 mapping), ``run_eval_batched``'s TTA mode, and any
reduced-precision plan.
"""
import ctypes as C

MAX_PARTS, MAX_LIMBS = 32, 32


class Skeleton(object):
    """name; part_names: one string per part; limbs: sequence of (part A, part B, PAF x channel, PAF y channel);
    seed: the limbs (indices into ``limbs``) whose unmatched connections may start a person - None = every limb;
    background: the heat map carries one more channel behind the parts; mirror: for every part the part it becomes in
    the x-mirrored image (a permutation that is its own inverse) - None derives it from the names: a leading ``L`` / ``R``
    followed by an upper-case letter is swapped, any other name mirrors to itself.

    Validates like ``rtpose_skeleton_check``: 1..32 parts and limbs, part indices inside the parts, no limb from a
    part to itself, no (A, B) pair twice, x channel != y channel, channels >= 0, seed limbs inside the table."""

    def __init__(self, name, part_names, limbs, seed=None, background=True, mirror=None):
        self.name = str(name)
        self.part_names = tuple(str(p) for p in part_names)
        self.limbs = tuple(tuple(int(v) for v in l) for l in limbs)
        self.background = bool(background)
        P, L = len(self.part_names), len(self.limbs)
        if not 1 <= P <= MAX_PARTS:
            raise ValueError("Skeleton %s: %d parts, outside 1..%d" % (self.name, P, MAX_PARTS))
        if not 1 <= L <= MAX_LIMBS:
            raise ValueError("Skeleton %s: %d limbs, outside 1..%d" % (self.name, L, MAX_LIMBS))
        seen = {}
        for i, l in enumerate(self.limbs):
            if len(l) != 4:
                raise ValueError("Skeleton %s: limb %d is not (part A, part B, PAF x, PAF y)" % (self.name, i))
            a, b, cx, cy = l
            if not (0 <= a < P and 0 <= b < P):
                raise ValueError("Skeleton %s: limb %d joins parts %d and %d, outside [0,%d)" % (self.name, i, a, b, P))
            if a == b:
                raise ValueError("Skeleton %s: limb %d joins part %d with itself" % (self.name, i, a))
            if cx < 0 or cy < 0:
                raise ValueError("Skeleton %s: limb %d reads PAF channels %d and %d" % (self.name, i, cx, cy))
            if cx == cy:
                raise ValueError("Skeleton %s: limb %d has the same PAF channel %d for x and y" % (self.name, i, cx))
            if (a, b) in seen:
                raise ValueError("Skeleton %s: limb %d repeats limb %d (parts %d -> %d)" % (self.name, i, seen[(a, b)], a, b))
            seen[(a, b)] = i
        seed = range(L) if seed is None else [int(s) for s in seed]
        mask = 0
        for s in seed:
            if not 0 <= s < L:
                raise ValueError("Skeleton %s: seed limb %d outside [0,%d)" % (self.name, s, L))
            mask |= 1 << s
        self.seed_mask = mask
        # an explicit mirror is checked here; the one the names give is derived on first use, so that a skeleton whose
        # names do not follow the L / R convention still decodes (it only cannot be flipped)
        self._mirror = None if mirror is None else self._checked_mirror(tuple(int(m) for m in mirror))

    @property
    def mirror(self):
        """For every part the part it becomes in the x-mirrored image."""
        if self._mirror is None:
            self._mirror = self._checked_mirror(self._mirror_from_names())
        return self._mirror

    def _checked_mirror(self, mirror):
        P = len(self.part_names)
        if len(mirror) != P:
            raise ValueError("Skeleton %s: mirror has %d entries for %d parts" % (self.name, len(mirror), P))
        for i, m in enumerate(mirror):
            if not 0 <= m < P:
                raise ValueError("Skeleton %s: part %d mirrors to %d, outside [0,%d)" % (self.name, i, m, P))
            if mirror[m] != i:
                raise ValueError("Skeleton %s: part %d mirrors to %d but %d mirrors to %d: the mirror is not an involution"
                                 % (self.name, i, m, m, mirror[m]))
        return mirror

    def _mirror_from_names(self):
        index = {n: i for i, n in enumerate(self.part_names)}
        out = []
        for n in self.part_names:
            if len(n) > 1 and n[0] in "LR" and n[1].isupper():
                other = ("R" if n[0] == "L" else "L") + n[1:]
                if other not in index:
                    raise ValueError("Skeleton %s: part %s has no counterpart %s (pass mirror= for names that do not "
                                     "follow the L / R convention)" % (self.name, n, other))
                out.append(index[other])
            else:
                out.append(index[n])
        return tuple(out)

    @classmethod
    def from_mask(cls, name, part_names, limbs, seed_mask, background=True, mirror=None):
        """The same with the seed limbs as a bit mask (bit l = limb l); bits at or above the limb count are refused."""
        n = len(tuple(limbs))
        if int(seed_mask) >> n:
            raise ValueError("Skeleton %s: seed mask 0x%x has bits at or above the %d limbs" % (name, int(seed_mask), n))
        return cls(name, part_names, limbs, [l for l in range(n) if (int(seed_mask) >> l) & 1], background, mirror)

    num_parts = property(lambda self: len(self.part_names))
    num_limbs = property(lambda self: len(self.limbs))

    @property
    def heat_channels(self):
        """Channels of the heat map the model must write: the parts (+ background)."""
        return self.num_parts + (1 if self.background else 0)

    @property
    def paf_channels(self):
        """Channels of the PAF map the model must write: the highest channel a limb reads, + 1."""
        return 1 + max(max(l[2], l[3]) for l in self.limbs)

    @property
    def pairs(self):
        """[(part A, part B)] in limb order (what draw_humans connects)."""
        return [(l[0], l[1]) for l in self.limbs]

    def flip_tables(self):
        """(heat_src, paf_src, paf_sign) of the flip merge: output heat-map channel c averages with channel heat_src[c] of
        the x-mirrored pass, PAF channel c with paf_sign[c] * channel paf_src[c].  A limb A -> B reads the limb
        mirror[A] -> mirror[B] as (-x, +y); where the table holds that limb only as mirror[B] -> mirror[A], as (+x, -y).
        Raises if a limb has no mirror in the table, or if limbs that share a channel disagree about it."""
        m, P, CP = self.mirror, self.num_parts, self.paf_channels
        heat_src = list(m) + ([P] if self.background else [])
        by_parts = {(l[0], l[1]): l for l in self.limbs}
        got = {}
        for i, (a, b, cx, cy) in enumerate(self.limbs):
            same, rev = by_parts.get((m[a], m[b])), by_parts.get((m[b], m[a]))
            if same is not None:
                pairs = ((cx, same[2], -1), (cy, same[3], 1))
            elif rev is not None:
                pairs = ((cx, rev[2], 1), (cy, rev[3], -1))
            else:
                raise ValueError("Skeleton %s: limb %d (%s -> %s) has no mirror: no limb joins %s and %s"
                                 % (self.name, i, self.part_names[a], self.part_names[b], self.part_names[m[a]],
                                    self.part_names[m[b]]))
            for c, s, sign in pairs:
                if got.setdefault(c, (s, sign)) != (s, sign):
                    raise ValueError("Skeleton %s: limb %d gives PAF channel %d the source %+d * channel %d, another limb gave "
                                     "it %+d * channel %d" % (self.name, i, c, sign, s, got[c][1], got[c][0]))
        paf_src = [got.get(c, (c, 1))[0] for c in range(CP)]
        paf_sign = [got.get(c, (c, 1))[1] for c in range(CP)]
        for c in range(CP):
            if paf_src[paf_src[c]] != c or paf_sign[c] != paf_sign[paf_src[c]]:
                raise ValueError("Skeleton %s: PAF channels %d and %d do not read each other: flipping twice is not the "
                                 "identity" % (self.name, c, paf_src[c]))
        return heat_src, paf_src, paf_sign

    def native_flip_table(self):
        """The ctypes mirror of rtpose_flip_table holding flip_tables(), checked by the library."""
        from . import _capi
        heat_src, paf_src, paf_sign = self.flip_tables()
        if len(heat_src) > _capi.FLIP_MAX_HEAT or len(paf_src) > _capi.FLIP_MAX_PAF:
            raise ValueError("Skeleton %s: %d heat-map / %d PAF channels, a flip table holds at most %d / %d"
                             % (self.name, len(heat_src), len(paf_src), _capi.FLIP_MAX_HEAT, _capi.FLIP_MAX_PAF))
        t = _capi.FlipTable()
        t.struct_bytes = C.sizeof(_capi.FlipTable)
        t.heat_channels, t.paf_channels = len(heat_src), len(paf_src)
        for c, s in enumerate(heat_src):
            t.heat_src[c] = s
        mask = 0
        for c, (s, sign) in enumerate(zip(paf_src, paf_sign)):
            t.paf_src[c] = s
            mask |= (sign < 0) << c
        t.paf_neg_mask = mask
        _capi.check(_capi.lib.rtpose_flip_table_check(C.byref(t)), "rtpose_flip_table_check")
        return t

    def native(self):
        """The ctypes mirror of rtpose_skeleton, checked by the library against this skeleton's channel counts."""
        from . import _capi
        s = _capi.SkeletonStruct()
        s.struct_bytes = C.sizeof(_capi.SkeletonStruct)
        s.num_parts, s.num_limbs = self.num_parts, self.num_limbs
        for i, (a, b, cx, cy) in enumerate(self.limbs):
            s.limb_part[i][0], s.limb_part[i][1] = a, b
            s.limb_paf[i][0], s.limb_paf[i][1] = cx, cy
        s.seed_mask = self.seed_mask
        _capi.check(_capi.lib.rtpose_skeleton_check(C.byref(s), self.heat_channels, self.paf_channels),
                    "rtpose_skeleton_check")
        return s

    def __repr__(self):
        return "Skeleton(%s: %d parts, %d limbs, %d PAF / %d heat-map channels)" % (
            self.name, self.num_parts, self.num_limbs, self.paf_channels, self.heat_channels)


# lib/utils/common.py:5-24 and lib/pafprocess/pafprocess.h:16-24; the reference's `pair_id < 18`: the last limb never seeds
COCO18 = Skeleton(
    "COCO18",
    ["Nose", "Neck", "RShoulder", "RElbow", "RWrist", "LShoulder", "LElbow", "LWrist", "RHip", "RKnee", "RAnkle", "LHip",
     "LKnee", "LAnkle", "REye", "LEye", "REar", "LEar"],
    [(1, 2, 12, 13), (1, 5, 20, 21), (2, 3, 14, 15), (3, 4, 16, 17), (5, 6, 22, 23), (6, 7, 24, 25), (1, 8, 0, 1),
     (8, 9, 2, 3), (9, 10, 4, 5), (1, 11, 6, 7), (11, 12, 8, 9), (12, 13, 10, 11), (1, 0, 28, 29), (0, 14, 30, 31),
     (14, 16, 34, 35), (0, 15, 32, 33), (15, 17, 36, 37), (2, 16, 18, 19), (5, 17, 26, 27)],
    seed=range(18))

# BODY_25: 25 parts (heat-map channel 25 is background), 26 limbs over 52 PAF channels, every limb may seed a person.
# Written from memory of upstream OpenPose's poseParameters.cpp: NOT VERIFIED against CMU's weights (neither that file
# nor the weights were at hand).  The grouping run over these tables is this project's - the tf-pose pafprocess algorithm
# the decoder implements - not OpenPose's own.
BODY_25 = Skeleton(
    "BODY_25",
    ["Nose", "Neck", "RShoulder", "RElbow", "RWrist", "LShoulder", "LElbow", "LWrist", "MidHip", "RHip", "RKnee", "RAnkle",
     "LHip", "LKnee", "LAnkle", "REye", "LEye", "REar", "LEar", "LBigToe", "LSmallToe", "LHeel", "RBigToe", "RSmallToe",
     "RHeel"],
    [(1, 8, 0, 1), (1, 2, 14, 15), (1, 5, 22, 23), (2, 3, 16, 17), (3, 4, 18, 19), (5, 6, 24, 25), (6, 7, 26, 27),
     (8, 9, 6, 7), (9, 10, 2, 3), (10, 11, 4, 5), (8, 12, 8, 9), (12, 13, 10, 11), (13, 14, 12, 13), (1, 0, 30, 31),
     (0, 15, 32, 33), (15, 17, 36, 37), (0, 16, 34, 35), (16, 18, 38, 39), (2, 17, 20, 21), (5, 18, 28, 29),
     (14, 19, 40, 41), (19, 20, 42, 43), (14, 21, 44, 45), (11, 22, 46, 47), (22, 23, 48, 49), (11, 24, 50, 51)])
BODY_25.__doc__ = ("OpenPose BODY_25 as a 25-part, 26-limb table written from memory of poseParameters.cpp: NOT VERIFIED "
                   "against CMU's weights; grouped by this project's (tf-pose pafprocess) algorithm, not OpenPose's own.")
