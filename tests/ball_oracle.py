"""CPU oracle of the ball's points and of the exact sampler (lgs_ball_points, lgs_exact_table,
lgs_exact_sample): a transcription, in pure Python floats (IEEE fp64, one rounding per
operation), of the fixed-radius traversal that include/lgs.h defines -- lgs_gaussian_mass's
loop, writing every point instead of summing it -- of the blocked running sum, and of the
draw rule.  Run on the c' a library call reports, the rows, D, nodes and status compare bit
for bit."""
import math

import numpy as np

from cvp_oracle import qr, refdist, setup  # noqa: F401  (the tests take bases and targets from there)

BLOCK = 256


def points(R, cp, radius2, max_nodes=1 << 40):
    """The traversal of lgs.h with A = radius2: (z, D, nodes, status) with z the (N, d) int64
    rows and D the (N,) distances in traversal order.  status 1: the budget ran out (the
    rows visited so far are returned; the library lists none)."""
    Rl, cpl = np.asarray(R).tolist(), np.asarray(cp).tolist()
    d = len(cpl)
    z, base, P, nxt, stp = [0] * d, [0.0] * d, [0.0] * (d + 1), [0] * d, [0] * d
    A = float(radius2)

    def enter(i):
        cs = 0.0
        Ri = Rl[i]
        for j in range(i + 1, d):
            cs = cs + Ri[j] * z[j]
        b = cpl[i] - cs
        m = b / Ri[i]
        z0 = round(m)  # round-half-even
        base[i] = b
        z[i] = z0
        stp[i] = 1 if m >= z0 else -1
        nxt[i] = 0

    rows, D, nodes, status = [], [], 0, 0
    i = d - 1
    enter(i)
    while True:
        if nodes == max_nodes:
            status = 1
            break
        nodes += 1
        r = base[i] - Rl[i][i] * z[i]
        Pi = P[i + 1] + r * r
        if Pi < A:
            if i == 0:
                rows.append(list(z))
                D.append(Pi)
            else:
                P[i] = Pi
                i -= 1
                enter(i)
                continue
        else:
            i += 1
            if i == d:
                break
        nxt[i] += 1
        z[i] += stp[i] * nxt[i]
        stp[i] = -stp[i]
    return (np.array(rows, dtype=np.int64).reshape(len(rows), d), np.array(D, dtype=np.float64), nodes, status)


def weights(D, sigma, shift=0.0):
    """w_m = exp((shift - D_m) / two_s2), each step a single operation (math.exp per row: the
    library's exp is within 1 ulp of it, not equal)."""
    two_s2 = 2.0 * sigma * sigma
    return np.array([math.exp((float(shift) - float(x)) / two_s2) for x in D], dtype=np.float64)


def blocked_cumsum(w):
    """S of lgs.h for one target's weights, by its written definition in Python floats:
    sequential inside each block of 256 rows, sequential over the block totals."""
    w = [float(x) for x in w]
    S, Pb = [], 0.0
    for b0 in range(0, len(w), BLOCK):
        c = 0.0
        for x in w[b0:b0 + BLOCK]:
            c = c + x
            S.append(Pb + c)
        Pb = Pb + c
    return np.array(S, dtype=np.float64)


def blocked_cumsum_np(w):
    """The same in NumPy terms: np.cumsum along the rows of the zero-padded (blocks, 256)
    array, then np.cumsum of the block totals (both accumulate sequentially)."""
    w = np.asarray(w, dtype=np.float64)
    N = len(w)
    if N == 0:
        return np.zeros(0)
    nb = (N + BLOCK - 1) // BLOCK
    pad = np.zeros(nb * BLOCK)
    pad[:N] = w
    c = np.cumsum(pad.reshape(nb, BLOCK), axis=1)
    Pnext = np.cumsum(c[:, -1])
    Pb = np.concatenate(([0.0], Pnext[:-1]))
    return (Pb[:, None] + c).reshape(-1)[:N]


def draw(S, u):
    """The row (within the target) a uniform u selects: the smallest m with S_m > u * M, M =
    S of the last row; the last row if there is none."""
    S = np.asarray(S, dtype=np.float64)
    tau = float(u) * float(S[-1])
    return min(int(np.searchsorted(S, tau, side="right")), len(S) - 1)
