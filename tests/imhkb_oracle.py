"""CPU oracle of lgs_imhk_bases, the whole definition of include/lgs.h for one basis: QR(p) from
tests/qr_oracle.py; draw t of chain c is the C oracle's Klein sample c + t 2^32 around the target's
c' (oracle/lgs_oracle.py klein: the reference-order means, the reference's SampleZ, lgs_set_basis's
sigma_i rule); its weight is the C oracle's Wang-Ling log weight (log_weight, IMHK_WANG_LING); the
accept uniform is philox_u(seed, 0, t, c, 1); the scan, the kept states and the lattice point are
written out here.  tests/test_imhk_bases_host.py checks that this composition is lgs_oracle.imhk
bit for bit.  Also the shapes, batches and widths the host and device tests share, and which
chains are settled: chains none of whose decisions lies within the weight tolerance of its
threshold, so that a weight evaluated another way (the device's SampleZ normaliser against the
oracle's logsumexp, 1e-9 relative) cannot decide otherwise."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import kleinb_oracle
import lgs_oracle
import qr_oracle

KEYS = ("qr_status", "R", "cprime", "z_draws", "logw_draws", "accepted", "accepts", "final_step", "logw", "z", "v",
        "z_samples", "status")
SEED = 20240607
FIRST_CHAIN = 1000
# (d, T) -> the (C, S) of the parity test: one ragged wave and no steps; 42 lanes; 465 lanes, two
# blocks of 256 with chains straddling the boundary and a ragged tail; 448 lanes, 3.5 blocks of 128
PARITY_CS = {(2, 1): ((1, 69), (5, 0)), (3, 2): ((3, 6),), (17, 5): ((3, 30),), (33, 64): ((1, 6),),
             (64, 64): ((1, 6),)}
SETTLE = 2e-9  # twice the 1e-9 relative weight tolerance of tests/test_gpu_imhk_targets.py


def ratio(lw_y, lw_x):
    """min(1, exp(lw_y - lw_x)); 1 from lw_x = -inf, and a NaN ratio is taken as 1."""
    if lw_x == -math.inf:
        return 1.0
    diff = lw_y - lw_x
    if diff != diff or diff >= 0.0:
        return 1.0
    return math.exp(diff)


def scan(lw, u, thin=1):
    """The accept scan of one chain over its S + 1 weights lw with the uniforms u[1 .. S] (u[0]
    unused).  Returns (accepted (S,) uint8, accepts, final_step, logw, kept: the state's draw index
    after steps thin, 2 thin, .., settled)."""
    S = len(lw) - 1
    cur, lw_x, acc, settled = 0, float(lw[0]), 0, True
    accepted, kept = np.zeros(S, dtype=np.uint8), []
    for t in range(1, S + 1):
        lw_y, ut = float(lw[t]), float(u[t])
        lnu = math.log(ut) if ut > 0.0 else -math.inf
        thr = min(0.0, lw_y - lw_x) if lw_x != -math.inf else 0.0
        if not abs(lnu - thr) >= SETTLE * max(abs(lw_y), abs(lw_x)):
            settled = False
        if ut < ratio(lw_y, lw_x):
            cur, lw_x, acc = t, lw_y, acc + 1
            accepted[t - 1] = 1
        if t % thin == 0:
            kept.append(cur)
    return accepted, acc, cur, lw_x, np.array(kept, dtype=np.int64), settled


def solve(B, targets, sigma, C, S, seed, first, thin=1, precision=10, qr=None):
    """One basis: the dict of the C-ABI's outputs for it (z int64), `first` the id of its chain
    (0, 0), plus "settled" (T, C) and "fallbacks" (the C oracle's count)."""
    targets = np.asarray(targets, dtype=np.float64)
    T, d = targets.shape
    nk = S // thin
    qs, R, cp = qr if qr is not None else qr_oracle.qr(B, targets)
    out = {"qr_status": np.int32(qs), "R": R, "cprime": cp, "z_draws": np.zeros((T, C, S + 1, d), dtype=np.int64),
           "logw_draws": np.full((T, C, S + 1), -math.inf), "accepted": np.zeros((T, C, S), dtype=np.uint8),
           "accepts": np.zeros((T, C), dtype=np.int64), "final_step": np.full((T, C), -1, dtype=np.int64),
           "logw": np.full((T, C), -math.inf), "z": np.zeros((T, C, d), dtype=np.int64), "v": np.zeros((T, C, d)),
           "z_samples": np.zeros((T, C, nk, d), dtype=np.int64), "status": np.full(T, 3 if qs else 0, dtype=np.int32),
           "settled": np.ones((T, C), dtype=bool), "fallbacks": 0}
    if qs:
        return out
    Bc = np.ascontiguousarray(B, dtype=np.float64)
    for k in range(T):
        c0 = first + k * C
        for t in range(S + 1):  # chains c0 .. c0 + C - 1 at step t are consecutive Klein samples
            r = lgs_oracle.klein(R, cp[k], float(sigma), C, seed=seed, first_sample=c0 + (t << 32), precision=precision)
            out["fallbacks"] += r["fallbacks"]
            out["z_draws"][k, :, t] = r["z"]
            for j in range(C):
                out["logw_draws"][k, j, t] = lgs_oracle.log_weight(R, cp[k], Bc, float(sigma), r["z"][j],
                                                                   mode=lgs_oracle.IMHK_WANG_LING, precision=precision)
        for j in range(C):
            u = [0.0] + [lgs_oracle.philox_u(seed, 0, t, c0 + j, 1) for t in range(1, S + 1)]
            a, acc, fin, lw, kept, ok = scan(out["logw_draws"][k, j], u, thin)
            out["accepted"][k, j], out["accepts"][k, j], out["final_step"][k, j], out["logw"][k, j] = a, acc, fin, lw
            out["settled"][k, j] = ok
            out["z"][k, j] = out["z_draws"][k, j, fin]
            out["z_samples"][k, j] = out["z_draws"][k, j, kept]
    out["v"] = kleinb_oracle.points(B, out["z"].reshape(T * C, d)).reshape(T, C, d)
    return out


_expected = {}


def expected(d, T, n, C, S, thin=1, seed=SEED, first_chain=FIRST_CHAIN):
    """The outputs of the parity batch qr_oracle.batch(d, T, n) with kleinb_oracle.sigma_for, stacked
    in the C-ABI's shapes; the 130-basis batch is computed once per process and shorter ones are its
    head (a chain's outputs do not depend on the batch).  Also "sigma" (n,), "settled" (n, T, C) and
    "fallbacks"."""
    key = (d, T, C, S, thin, seed, first_chain)
    if key not in _expected or _expected[key][0] < n:
        m = 3 if n <= 3 else max(n, max(qr_oracle.BATCHES))
        Bs, Ts, idx = qr_oracle.batch(d, T, m)
        qrs = [kleinb_oracle.qr_of(d, T, v) for v in idx]
        lgs_oracle.lib()
        # (the C oracle runs outside the interpreter lock: the bases in parallel)
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            per = list(pool.map(lambda p: solve(Bs[p], Ts[p], kleinb_oracle.sigma_for(idx[p]), C, S, seed,
                                                first_chain + p * T * C, thin, qr=qrs[p]), range(m)))
        e = {k: np.stack([q[k] for q in per]) for k in KEYS + ("settled",)}
        e["sigma"] = np.array([kleinb_oracle.sigma_for(v) for v in idx])
        e["fallbacks"] = sum(q["fallbacks"] for q in per)
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[key] = (m, e)
    e = _expected[key][1]
    return {k: (a[:n] if isinstance(a, np.ndarray) else a) for k, a in e.items()}
