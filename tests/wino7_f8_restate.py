"""F(8,7) - the 14-frequency form of csrc/conv_wino7.hip (struct WT<8>) - restated on the host for the tests.

The point set is the F(6,7) one plus the pair +-5/4 (of the candidates +-5/4, +-3, +-1/4, +-1/3, +-3/4 the one with the
smallest element-wise error in an fp32 emulation of the kernel's arithmetic).  The exact tables come from
oracle/winograd_tables.toom_cook; `conv_rows_f87` is an fp32 numpy restatement of what the kernel does to one row of
outputs: the input transform BT (rows scaled by N_f, rounded to fp32 as the kernel's constants are) in fp32, the filter
transform G in float64 rounded once to fp32 (the pack kernel), the products summed over channels and ky in fp32, and the
output transform AT in fp32."""
from fractions import Fraction as Fr

import numpy as np

from oracle.winograd_tables import toom_cook, POINTS_F6_7

POINTS_F8_7 = POINTS_F6_7 + [Fr(5, 4), Fr(-5, 4)]
FM, NFQ = 8, 14


def tables_f87():
    """(AT [8][14], G [14][7], BT [14][14]) as float64 arrays of the exact rationals."""
    f = lambda M: np.array([[float(v) for v in row] for row in M])   # noqa: E731
    return tuple(map(f, toom_cook(FM, 7, POINTS_F8_7)))


def amp_exact(wts, m):
    """The amplification estimate's definition (include/rtpose_mi355x.h: rtpose_winograd_amplification) for a 7x7 filter
    bank [cout][cin][7][7] in F(m,7), m = 4 / 6 / 8, from the exact tables."""
    from oracle.winograd_tables import POINTS_F4_7
    pts = {4: POINTS_F4_7, 6: POINTS_F6_7, 8: POINTS_F8_7}[m]
    f = lambda M: np.array([[float(v) for v in row] for row in M])   # noqa: E731
    AT, G, BT = map(f, toom_cook(m, 7, pts))
    wd = np.asarray(wts, dtype=np.float64)
    Uf = np.einsum('fk,ocyk->ocyf', G, wd)
    a, b = np.abs(AT), np.abs(BT).sum(1)
    sfreq = np.abs(Uf).sum((1, 2))
    num = (a[None] * (b * sfreq)[:, None, :]).sum(2).max(1)
    return float((num / np.abs(wd).sum((1, 2, 3))).max())


def conv_rows_f87(x, w, bias):
    """x [cin][H][W], w [cout][cin][7][7], bias [cout] (float32) -> [cout][H][W] float32: stride 1, 'same' padding,
    F(8,7) along x and a direct sum along y, every step rounded to fp32 where the kernel rounds."""
    AT, G, BT = tables_f87()
    AT32, BT32 = AT.astype(np.float32), BT.astype(np.float32)
    cin, H, W = x.shape
    cout = w.shape[0]
    gx = (W + FM - 1) // FM
    xp = np.zeros((cin, H + 6, FM * gx + 6), np.float32)
    xp[:, 3:3 + H, 3:3 + W] = x
    # U[ky][f][c][o]: float64 sum, one rounding
    U = np.einsum('fk,ocyk->yfco', G, w.astype(np.float64)).astype(np.float32)
    # V[r][g][f][c] = sum_n BT[f][n] x[c][r][8 g + n], accumulated term by term in fp32
    V = np.zeros((H + 6, gx, NFQ, cin), np.float32)
    for g in range(gx):
        d = xp[:, :, FM * g:FM * g + NFQ]                       # [c][r][n]
        for n in range(NFQ):
            V[:, g] += BT32[None, :, n, None] * d[:, :, n].T[:, None, :]
    out = np.zeros((cout, H, FM * gx), np.float32)
    for y in range(H):
        m = np.zeros((gx, NFQ, cout), np.float32)
        m[:, 1, :] = bias[None, :]                              # the bias rides in the point 1 (its AT column is ones)
        for ky in range(7):
            m += np.einsum('gfc,fco->gfo', V[y + ky], U[ky]).astype(np.float32)
        o = np.zeros((gx, FM, cout), np.float32)
        for f in range(NFQ):
            o += AT32[None, :, f, None] * m[:, f, None, :]
        out[:, y, :] = o.reshape(gx * FM, cout).T
    return out[:, :, :W]
