"""CPU oracle of lgs_klein_bases, the whole definition of include/lgs.h for one basis: QR(p) from
tests/qr_oracle.py, the draws from the C oracle (oracle/lgs_oracle.py klein: the reference-order
conditional means, the reference's SampleZ and lgs_set_basis's sigma_i rule, on the Philox counters
of Klein sample s), D in the defined order in IEEE fp64 with one rounding per operation, the select
and the lattice point.  Every output of the device call compares bit for bit.  Also the batches and
widths the host and device tests share."""
import math

import numpy as np

import lgs_oracle
import qr_oracle

KEYS = ("qr_status", "R", "cprime", "z_draws", "dist2_draws", "best_draw", "dist2", "z", "v", "status")
SIGMAS = (3.0, 300.0, 3000.0)
SEED = 20240607
# (d, T) -> the K of the parity test: one lane and a ragged wave; two lanes and six; fifteen lanes
# and a basis spanning two blocks with a ragged tail; 320 lanes twice (the largest LDS image last)
PARITY_K = {(2, 1): (1, 70), (3, 2): (1, 3), (17, 5): (3, 70), (33, 64): (5,), (64, 64): (5,)}


def sigma_for(v):
    """The width of distinct pair v: a kernel that reads sigma[0] for every basis fails."""
    return SIGMAS[v % 3]


def distances(R, cp, z):
    """D of the draws z (n, d) around c' = cp ((d,), or (n, d): one centre per draw), all at once:
    for i = d-1 .. 0, cs the sequential sum over ascending j > i of R[i][j] * z[j] from 0.0,
    r = (c'_i - cs) - R[i][i] * z[i] with the product rounded first, D = D + r * r.  NumPy's
    elementwise fp64 operations round once each."""
    R, zf = np.asarray(R, dtype=np.float64), np.asarray(z).astype(np.float64)
    cp = np.broadcast_to(np.asarray(cp, dtype=np.float64), zf.shape)
    d = R.shape[0]
    D = np.zeros(zf.shape[0])
    for i in range(d - 1, -1, -1):
        cs = np.zeros(zf.shape[0])
        for j in range(i + 1, d):
            cs = cs + R[i, j] * zf[:, j]
        q = R[i, i] * zf[:, i]
        r = (cp[:, i] - cs) - q
        D = D + r * r
    return D


def points(B, z):
    """qr_oracle.point for every row of z (n, d) at once (the same operations in the same order)."""
    B, zf = np.asarray(B, dtype=np.float64), np.asarray(z).astype(np.float64)
    out = np.zeros(zf.shape)
    for j in range(B.shape[1]):
        out = out + B[None, :, j] * zf[:, j, None]
    return out


_qr = {}


def qr_of(d, T, v):
    """QR(p) of distinct pair v, computed once per process."""
    if (d, T, v) not in _qr:
        _qr[(d, T, v)] = qr_oracle.qr(*qr_oracle.pair(d, T, v))
    return _qr[(d, T, v)]


def solve(B, targets, sigma, K, seed, first, precision=10, qr=None):
    """One basis: the dict of the C-ABI's outputs for it (z int64), `first` the Klein sample index
    of its draw (0, 0), plus "fallbacks" (the C oracle's count) and "s" (the sigma_i used)."""
    targets = np.asarray(targets, dtype=np.float64)
    T, d = targets.shape
    qs, R, cp = qr if qr is not None else qr_oracle.qr(B, targets)
    out = {"qr_status": np.int32(qs), "R": R, "cprime": cp, "z_draws": np.zeros((T, K, d), dtype=np.int64),
           "dist2_draws": np.full((T, K), math.inf), "best_draw": np.full(T, -1, dtype=np.int64),
           "dist2": np.full(T, math.inf), "z": np.zeros((T, d), dtype=np.int64), "v": np.zeros((T, d)),
           "status": np.full(T, 3 if qs else 0, dtype=np.int32), "fallbacks": 0, "s": np.zeros(d)}
    if qs:
        return out
    out["s"] = float(sigma) / np.diag(R)
    for k in range(T):
        r = lgs_oracle.klein(R, cp[k], float(sigma), K, seed=seed, first_sample=(first + k * K) % (1 << 64),
                             precision=precision)
        out["fallbacks"] += r["fallbacks"]
        out["z_draws"][k] = r["z"]
    out["dist2_draws"] = distances(R, np.repeat(cp, K, axis=0), out["z_draws"].reshape(T * K, d)).reshape(T, K)
    for k in range(T):
        D = out["dist2_draws"][k]
        j = int(np.argmin(D))  # (the first of equal minima: ties to the smallest j)
        out["best_draw"][k], out["dist2"][k], out["z"][k] = j, D[j], out["z_draws"][k, j]
    out["v"] = points(B, out["z"])
    return out


_expected = {}


def expected(d, T, n, K, seed=SEED, first_sample=0):
    """The outputs of the parity batch qr_oracle.batch(d, T, n) with sigma_for and K draws, stacked
    in the C-ABI's shapes; the 130-basis batch is computed once per process and shorter ones are its
    head (a problem's outputs do not depend on the batch).  Also "sigma" (n,) and "fallbacks"."""
    key = (d, T, K, seed, first_sample)
    if key not in _expected or _expected[key][0] < n:
        m = 3 if n <= 3 else max(n, max(qr_oracle.BATCHES))
        Bs, Ts, idx = qr_oracle.batch(d, T, m)
        per = [solve(Bs[p], Ts[p], sigma_for(idx[p]), K, seed, (first_sample + p * T * K) % (1 << 64),
                     qr=qr_of(d, T, idx[p])) for p in range(m)]
        e = {k: np.stack([q[k] for q in per]) for k in KEYS + ("s",)}
        e["sigma"] = np.array([sigma_for(v) for v in idx])
        e["fallbacks"] = sum(q["fallbacks"] for q in per)
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[key] = (m, e)
    e = _expected[key][1]
    return {k: (a[:n] if isinstance(a, np.ndarray) else a) for k, a in e.items()}
