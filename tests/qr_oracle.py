"""CPU oracle of lgs_closest_vector_bases' factorisation: QR(p) of include/lgs.h transcribed
into Python floats (IEEE fp64, one rounding per operation, math.sqrt correctly rounded), and
the lattice point v = B z in the defined order.  With the search of tests/cvp_oracle.py run on
its R and c', every output of the device call compares bit for bit.  Also the batches the host
and device tests share."""
import math

import numpy as np


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def qr(B, targets):
    """QR(p) on W = [B | t_0 .. t_{T-1}].  B: d x d, the columns generate the lattice; targets:
    T x d.  Returns (qr_status, R, cprime): R d x d and cprime T x d float64 arrays, zeros with
    qr_status 3."""
    B, targets = np.asarray(B, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    d, T = B.shape[0], targets.shape[0]
    W = [B[i].tolist() + targets[:, i].tolist() for i in range(d)]
    for k in range(d):
        s = 0.0
        for i in range(k, d):
            s = s + W[i][k] * W[i][k]
        nrm = math.sqrt(s) if s >= 0.0 else math.nan
        if not 0.0 < nrm < math.inf:
            return 3, np.zeros((d, d)), np.zeros((T, d))
        alpha = -nrm if W[k][k] >= 0.0 else nrm
        v = [0.0] * d
        v[k] = W[k][k] - alpha
        for i in range(k + 1, d):
            v[i] = W[i][k]
        vv = 0.0
        for i in range(k, d):
            vv = vv + v[i] * v[i]
        for c in range(k + 1, d + T):
            dot = 0.0
            for i in range(k, d):
                dot = dot + v[i] * W[i][c]
            f = _div(dot + dot, vv)
            for i in range(k, d):
                W[i][c] = W[i][c] - f * v[i]
        W[k][k] = alpha
        for i in range(k + 1, d):
            W[i][k] = 0.0
    for k in range(d):
        if W[k][k] < 0.0:
            for c in range(k, d + T):
                W[k][c] = -W[k][c]
    Wa = np.array(W, dtype=np.float64)
    return 0, np.ascontiguousarray(Wa[:, :d]), np.ascontiguousarray(Wa[:, d:].T)


def point(B, z):
    """v[i] = the sequential sum over ascending j of B[i][j] * float(z[j]), from 0.0."""
    Bl, zl = np.asarray(B, dtype=np.float64).tolist(), [float(int(x)) for x in z]
    out = []
    for row in Bl:
        acc = 0.0
        for bij, zj in zip(row, zl):
            acc = acc + bij * zj
        out.append(acc)
    return np.array(out, dtype=np.float64)


def solve(B, targets, max_nodes=1 << 40, radius2=None):
    """The whole definition for one basis: QR(p), then cvp_oracle.se per target, then v.  Returns
    a dict of the C-ABI's outputs for that basis (z int64)."""
    import cvp_oracle
    targets = np.asarray(targets, dtype=np.float64)
    T, d = targets.shape
    qs, R, cp = qr(B, targets)
    out = {"qr_status": np.int32(qs), "R": R, "cprime": cp, "z": np.zeros((T, d), dtype=np.int64),
           "v": np.zeros((T, d)), "dist2": np.full(T, math.inf), "nodes": np.zeros(T, dtype=np.int64),
           "status": np.full(T, 3 if qs else 0, dtype=np.int32)}
    if qs:
        return out
    for k in range(T):
        z, D, nodes, st = cvp_oracle.se(R, cp[k], max_nodes=max_nodes,
                                        radius2=math.inf if radius2 is None else float(radius2[k]))
        out["z"][k], out["dist2"][k], out["nodes"][k], out["status"][k] = z, D, nodes, st
        out["v"][k] = point(B, z)
    return out


KEYS = ("qr_status", "R", "cprime", "z", "v", "dist2", "nodes", "status")

# ---------------------------------------------------------------- the parity batches
# (d, T), the smallest at which each mechanism can go wrong: one lane; a ragged pair; an odd d
# beside a ragged T; the second column pass of the QR (d + T > 64); both LDS budgets.
SHAPES = ((2, 1), (3, 2), (17, 5), (33, 64), (64, 64))
BATCHES = (1, 3, 130)
PARITY_NODES = 1 << 16  # max_nodes of the parity tests: test_cvp_bases_host.py shows every problem ends below it
# Distinct (basis, targets) pairs of a shape; a longer batch repeats them in turn (the outputs of a
# problem do not depend on its place in the batch).  The transcription costs 0.3 s per basis at d = 64.
DISTINCT = {2: 130, 3: 130, 17: 130, 33: 3, 64: 3}
RATIO = 64.0


def basis_for(d, variant=0):
    """Basis `variant` of a parity shape: float64 d x d, integral, the vectors in columns, built
    from the bases of lll_oracle.  d = 2: the raw d2; d = 3: the reduced d3; both times a
    unimodular matrix that depends on the variant.  d = 17, 33, 64: reduced qary16 blocks
    (delta 0.99 and 0.75 in turn, then 1 x 1 blocks up to d) on the diagonal, block k scaled by
    64^k, with random integers above the diagonal blocks.  The exact search is exponential in d
    for targets of this spread; the growing scale lets the search settle the later blocks first,
    which keeps every problem at a few thousand nodes, and the transcription affordable, while R
    stays a full upper triangle."""
    import lll_oracle
    rng = np.random.default_rng(9000 + 100 * d + variant)
    if d <= 3:
        B = (lll_oracle.bases()["d2"] if d == 2 else np.array(lll_oracle.reduced("d3", 0.99)["basis_out"]))
        B = B.astype(np.float64)
        for _ in range(variant % 4 + (variant > 0)):
            a = int(rng.integers(d))
            b = (a + 1 + int(rng.integers(d - 1))) % d
            B[:, a] = B[:, a] + float(rng.integers(-2, 3)) * B[:, b]
        return B
    q16 = [np.array(lll_oracle.reduced("qary16", dl)["basis_out"], dtype=np.float64) for dl in (0.99, 0.75)]
    blocks = [q16[k % 2] for k in range(d // 16)] + [np.array([[5.0 + e]]) for e in range(d % 16)]
    B, o, scale = np.zeros((d, d)), 0, 1.0
    for blk in blocks:
        k = blk.shape[0]
        B[o:o + k, o:o + k] = blk * scale
        B[:o, o:o + k] = np.rint(rng.standard_normal((o, k)) * 3.0) * scale
        o += k
        scale *= RATIO
    return B


_pairs, _solved = {}, {}


def pair(d, T, v):
    """Distinct pair v of a shape: (basis, targets), read-only, built once per process."""
    if (d, T, v) not in _pairs:
        B = basis_for(d, v)
        t = np.random.default_rng(7000 + 131 * d + v).standard_normal((T, d)) * 2500.0
        B.setflags(write=False)
        t.setflags(write=False)
        _pairs[(d, T, v)] = (B, t)
    return _pairs[(d, T, v)]


def batch(d, T, n):
    """bases (n, d, d), targets (n, T, d) and the index of each basis's distinct pair."""
    idx = [p % DISTINCT[d] for p in range(n)]
    return (np.stack([pair(d, T, v)[0] for v in idx]), np.stack([pair(d, T, v)[1] for v in idx]), idx)


def solved(d, T, v, max_nodes=PARITY_NODES):
    """solve() of distinct pair v, computed once per process and not to be modified."""
    if (d, T, v, max_nodes) not in _solved:
        _solved[(d, T, v, max_nodes)] = solve(*pair(d, T, v), max_nodes=max_nodes)
    return _solved[(d, T, v, max_nodes)]


def expected(d, T, n, max_nodes=PARITY_NODES):
    """The outputs of the whole batch, stacked in the C-ABI's shapes."""
    idx = batch(d, T, n)[2]
    return {k: np.stack([solved(d, T, v, max_nodes)[k] for v in idx]) for k in KEYS}
