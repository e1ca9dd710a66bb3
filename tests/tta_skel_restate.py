"""Host restatement of the flip merge with the left / right permutation as data (csrc/tta.hip), and the tables
tests/test_skeleton_flip_cpu.py and tests/test_tta_skel_gpu.py share.  numpy + torch CPU float64, no GPU, no library call;
extends tests/layout_restate.py (which stays as it is) and follows its convention: an arithmetic reference returns
(value, S), the float64 result and the float64 sum of the absolute values of the terms that were added.
"""
import numpy as np
import torch

import layout_restate as lr

BODY_25_HEAT = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21, 25]


def flip_merge(normal, flipped, src, sign):
    """One map, NHWC: the average of `normal` with the x-mirrored `flipped` gathered through src and multiplied by sign
    (+1 / -1 per output channel).  -> (value, S) in float64; S is the magnitude sum lr.flip_merge returns."""
    a, f = lr._t64(normal), lr._t64(flipped)
    g = torch.flip(f, dims=[2])[..., torch.as_tensor(np.asarray(src, dtype=np.int64))]
    g = g * torch.as_tensor(np.asarray(sign, dtype=np.float64))
    return (a + g) / 2, (a.abs() + g.abs()) / 2


def flip_merge_f32(normal, flipped, src, sign):
    """The kernel's own arithmetic in fp32: (a + s * g) / 2 - the sign change and the halving are exact, the add rounds
    once - as uint32 bit patterns."""
    a = np.ascontiguousarray(normal, dtype=np.float32)
    g = np.ascontiguousarray(flipped, dtype=np.float32)[:, :, ::-1][..., np.asarray(src, dtype=np.int64)]
    g = g * np.asarray(sign, dtype=np.float32)
    return np.ascontiguousarray((a + g) / np.float32(2)).view(np.uint32)


def mirror_maps(heat, paf, tables):
    """What the maps of the x-mirrored image should be: HWC maps mirrored in x and gathered through the tables."""
    heat_src, paf_src, paf_sign = tables
    return (heat[:, ::-1][:, :, np.asarray(heat_src)],
            paf[:, ::-1][:, :, np.asarray(paf_src)] * np.asarray(paf_sign, dtype=paf.dtype))


# ---- the skeletons under test: (part names, limbs, background, mirror or None) -----------------------------------------
def reversed3():
    """Neck -> LHand mirrors to Neck -> RHand, which the table holds only as RHand -> Neck."""
    return ["Neck", "LHand", "RHand"], [(0, 1, 0, 1), (2, 0, 2, 3)], True, None


def pair2():
    """2 parts, 1 limb, no background: the limb LHip -> RHip mirrors to itself walked backwards."""
    return ["LHip", "RHip"], [(0, 1, 1, 0)], False, None


def full32():
    """32 parts, 32 limbs, 64 scattered PAF channels, an explicit mirror: a ring p0 -> p1 -> ... -> p31 -> p0 mirrored by
    i -> (5 - i) mod 32 (two fixed points would need 2 i = 5: none, so every part moves), which maps limb i -> i + 1 onto the
    limb (4 - i) -> (5 - i) walked backwards; the channels are a fixed shuffle of 0..63."""
    P = 32
    chans = np.random.default_rng(32).permutation(64)
    limbs = [(i, (i + 1) % P, int(chans[2 * i]), int(chans[2 * i + 1])) for i in range(P)]
    return ["p%d" % i for i in range(P)], limbs, True, [(5 - i) % P for i in range(P)]


def make(skm, name):
    """The product's Skeleton for one of: coco18, body25, reversed3, full32, pair2."""
    if name == "coco18":
        return skm.COCO18
    if name == "body25":
        return skm.BODY_25
    names, limbs, bg, mirror = {"reversed3": reversed3, "full32": full32, "pair2": pair2}[name]()
    return skm.Skeleton(name, names, limbs, background=bg, mirror=mirror)


TABLE_NAMES = ["coco18", "body25", "reversed3", "full32", "pair2"]
