"""Float64 restatement of the target encoder (header section 4b; csrc/encode.hip mirrors it): the reference's
get_ground_truth / putGaussianMaps / putVecMaps (lib/datasets/datasets.py:259-308, heatmap.py:20-36, paf.py:18-68) for any
skeleton table, operation for operation in the reference's order.  Whole maps are numpy arrays, but every array
operation is element-wise IEEE float64, so each cell sees the scalar sequence the kernel executes; people are walked in
order.  The one deliberate difference from the reference: the limb norm is the unfused sqrt(vx * vx + vy * vy), where
np.linalg.norm goes through BLAS's dot (which may fuse the multiply-add).

Also the float64 restatement of rtpose_stage_mse.  Not a test module."""
import numpy as np


def present(kp, input_h, input_w):
    """kp [..., 3] -> bool [...]: v > 0.5 and inside the input (remove_illegal_joint + the `> 0.5` tests)."""
    x, y, v = kp[..., 0], kp[..., 1], kp[..., 2]
    with np.errstate(invalid="ignore"):
        return (v > 0.5) & (x >= 0) & (x < input_w) & (y >= 0) & (y < input_h)


def encode(people, table, input_h, input_w, stride=8, sigma=7.0, heat_channels=None, paf_channels=None, background=None,
           return_counts=False):
    """people: (K, P, 3) float64 (x, y, v); table: num_parts, limbs [(A, B, chx, chy)], heat_channels, paf_channels,
    background (a skeleton.Skeleton has them; the keyword arguments override).
    -> heat [h, w, heat_channels], paf [h, w, paf_channels] float64; with return_counts also the limbs' final counts
    [h, w, num_limbs] (how many people's masks cover a cell)."""
    CH = table.heat_channels if heat_channels is None else heat_channels
    CP = table.paf_channels if paf_channels is None else paf_channels
    bg = table.background if background is None else background
    P = table.num_parts
    people = np.asarray(people, np.float64).reshape(-1, P, 3)
    h, w = input_h // stride, input_w // stride
    ok = present(people, input_h, input_w)
    start = stride / 2.0 - 0.5
    ys, xs = np.mgrid[0:h, 0:w]
    gx, gy = (xs * stride).astype(np.float64) + start, (ys * stride).astype(np.float64) + start
    fx, fy = xs.astype(np.float64), ys.astype(np.float64)
    heat = np.zeros((h, w, CH), np.float64)
    for j in range(P):
        acc = np.zeros((h, w), np.float64)
        for k in range(people.shape[0]):
            if not ok[k, j]:
                continue
            dx, dy = gx - people[k, j, 0], gy - people[k, j, 1]
            e = (dx * dx + dy * dy) / 2.0 / sigma / sigma
            acc = acc + np.where(e <= 4.6052, np.exp(-e), 0.0)
            acc = np.where(acc > 1.0, 1.0, acc)
        heat[:, :, j] = acc
    if bg:
        heat[:, :, P] = np.maximum(1.0 - heat[:, :, :P].max(axis=2), 0.0)
    paf = np.zeros((h, w, CP), np.float64)
    owned = set()
    counts = []
    for A, B, chx, chy in table.limbs:
        accx, accy = np.zeros((h, w), np.float64), np.zeros((h, w), np.float64)
        count = np.zeros((h, w), np.int64)
        for k in range(people.shape[0]):
            if not (ok[k, A] and ok[k, B]):
                continue
            ax, ay = people[k, A, 0] / stride, people[k, A, 1] / stride
            bx, by = people[k, B, 0] / stride, people[k, B, 1] / stride
            vx, vy = bx - ax, by - ay
            n = np.sqrt(vx * vx + vy * vy)
            if n == 0.0:
                continue
            ux, uy = vx / n, vy / n
            x0, x1 = max(int(np.rint(min(ax, bx) - 1.0)), 0), min(int(np.rint(max(ax, bx) + 1.0)), w)
            y0, y1 = max(int(np.rint(min(ay, by) - 1.0)), 0), min(int(np.rint(max(ay, by) + 1.0)), h)
            m = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
            m &= np.abs((fx - ax) * uy - (fy - ay) * ux) < 1.0
            m &= bool(abs(ux) > 0.0 or abs(uy) > 0.0)
            cd = count.astype(np.float64)
            accx, accy = accx * cd, accy * cd
            accx = np.where(m, accx + ux, accx)
            accy = np.where(m, accy + uy, accy)
            count = count + m
            div = np.maximum(count, 1).astype(np.float64)
            accx, accy = accx / div, accy / div
        # a channel two limbs name belongs to the first of them
        if chx not in owned:
            paf[:, :, chx] = accx
        if chy not in owned:
            paf[:, :, chy] = accy
        owned.update((chx, chy))
        counts.append(count)
    if return_counts:
        return heat, paf, np.stack(counts, axis=2)
    return heat, paf


def encode_batch(people_list, table, input_h, input_w, **kw):
    """[(k_i, P, 3)] per image -> heat [N, h, w, CH], paf [N, h, w, CP] float64."""
    hs, ps = zip(*[encode(p, table, input_h, input_w, **kw) for p in people_list])
    return np.stack(hs), np.stack(ps)


def ulp_distance(a, b):
    """Element-wise distance of two float32 arrays in units in the last place (ordered-integer trick)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def stage_mse(pred, target):
    """float64 mean of (pred - target)^2 over equal-shaped float32 arrays."""
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    return float(np.sum(d * d) / d.size)
