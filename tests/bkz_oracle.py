"""CPU oracle of lgs_bkz_reduce: the operational definition of include/lgs.h transcribed into
Python ints (exact) and floats (IEEE fp64, one rounding per operation, round() = half-even).

The LLL loop is lgs_lll_reduce's, stated here in resumable form (``_State.lll(k0)`` enters the
``while k < d`` loop at k0 on the current state); ENUM and INSERT follow the header line by
line.  ``plain=True`` replaces ENUM by the textbook search -- entered at the block's top level,
zigzag on every level, no ``top`` rule, so that it meets v and -v alike -- and is the
independent check that a status-0 output holds no block vector below delta r[kb][kb].

Conventions are the C-ABI's: ``basis`` is d x d, vector b_i is COLUMN i, basis_out = basis @ U.
The bases are lll_oracle.bases(); results are computed once per process and not to be modified.
"""
import numpy as np

import lll_oracle

B_LIMIT = 1 << 28
U_LIMIT = 1 << 40
X_LIMIT = float(1 << 22)
C_LIMIT = float(1 << 22)
BKZ_SLICE = 64  # enumeration nodes per launch that the device slice test forces
LLL_SLICE = 16  # ... and LLL main-loop iterations

FIELDS = ("basis_out", "U_out", "swaps", "iters", "passes", "tours", "blocks", "insertions", "nodes", "truncated",
          "status", "gs_norm2")


class _Stop(Exception):
    def __init__(self, status, where="lll"):
        self.status, self.where = status, where


def _good(x):
    return x > 0.0 and x != float("inf")


class _State:
    """b, U, exact G, mu, r of lgs_lll_reduce, and the counters of lgs_bkz_outputs."""

    def __init__(self, basis, delta, eta, max_iters):
        d = self.d = len(basis)
        self.delta, self.eta, self.max_iters = delta, eta, max_iters
        self.b = [[int(basis[c][i]) for c in range(d)] for i in range(d)]  # b[i] = column i
        self.U = [[int(i == c) for c in range(d)] for i in range(d)]
        b = self.b
        self.G = [[sum(x * y for x, y in zip(b[i], b[j])) for j in range(d)] for i in range(d)]
        self.mu = [[0.0] * d for _ in range(d)]
        self.r = [[0.0] * d for _ in range(d)]
        self.swaps = self.iters = self.passes = 0
        self.tours = self.blocks = self.insertions = self.nodes = self.truncated = 0
        self.steps = 0  # Euclid steps of INSERT applied
        self.log = []  # per block: (kb, e, nodes_b, trunc, best or None)
        self.trace = []  # in order: ("lll", main-loop iterations of one run) and ("enum", nodes of one block)

    def chol(self, k):
        mu, r = self.mu, self.r
        rk, Gk = r[k], self.G[k]
        for j in range(k + 1):
            s, muj = float(Gk[j]), mu[j]
            for i in range(j):
                s = s - muj[i] * rk[i]
            rk[j] = s
            if j < k:
                mu[k][j] = s / r[j][j]

    def lll(self, k):
        """The main loop of lgs_lll_reduce entered at k; returns when k reaches d."""
        start = self.iters
        try:
            self._lll(k)
        finally:
            self.trace.append(("lll", self.iters - start))

    def _lll(self, k):
        d, b, U, G, mu, r, eta = self.d, self.b, self.U, self.G, self.mu, self.r, self.eta
        while k < d:
            if self.iters == self.max_iters:
                raise _Stop(1)
            self.iters += 1
            while True:
                self.passes += 1
                self.chol(k)
                applied = False
                for j in range(k - 1, -1, -1):
                    if abs(mu[k][j]) > eta:
                        X = float(round(mu[k][j]))
                        if not abs(X) < X_LIMIT:
                            raise _Stop(2)
                        Xi = int(X)
                        nb = [x - Xi * y for x, y in zip(b[k], b[j])]
                        nU = [x - Xi * y for x, y in zip(U[k], U[j])]
                        if any(abs(x) >= B_LIMIT for x in nb) or any(abs(x) >= U_LIMIT for x in nU):
                            raise _Stop(2)
                        b[k], U[k] = nb, nU
                        for i in range(j):
                            mu[k][i] = mu[k][i] - X * mu[j][i]
                        mu[k][j] = mu[k][j] - X
                        applied = True
                if not applied:
                    break
                for j in range(d):
                    G[k][j] = G[j][k] = sum(x * y for x, y in zip(b[k], b[j]))
            if not _good(r[k][k]):
                raise _Stop(3)
            t = mu[k][k - 1] * mu[k][k - 1]
            t = self.delta - t
            t = t * r[k - 1][k - 1]
            if r[k][k] >= t:
                k += 1
            else:
                b[k], b[k - 1] = b[k - 1], b[k]
                U[k], U[k - 1] = U[k - 1], U[k]
                G[k], G[k - 1] = G[k - 1], G[k]
                for row in G:
                    row[k], row[k - 1] = row[k - 1], row[k]
                self.swaps += 1
                if k == 1:
                    r[0][0] = float(G[0][0])
                    if not _good(r[0][0]):
                        raise _Stop(3)
                k = max(k - 1, 1)

    def enum(self, kb, e, enum_nodes, plain=False):
        """ENUM(kb, e): (best, trunc, nodes_b); best is the list x[kb..e] or None."""
        mu, r = self.mu, self.r
        A = self.delta * r[kb][kb]
        x = [0] * (e + 2)
        c = [0.0] * (e + 2)
        P = [0.0] * (e + 2)
        stp = [1] * (e + 2)
        nxt = [0] * (e + 2)
        best = None
        nodes_b = 0

        def enter(i):
            cs = 0.0
            for j in range(e, i, -1):
                cs = cs + mu[j][i] * float(x[j])
            c[i] = 0.0 - cs
            if not abs(c[i]) < C_LIMIT:
                raise _Stop(2, "enum")
            x[i] = int(round(c[i]))
            stp[i] = 1 if c[i] >= x[i] else -1
            nxt[i] = 0

        if plain:
            top, i = None, e
            enter(e)
        else:
            top = i = kb
        while True:
            if nodes_b == enum_nodes:
                return best, 1, nodes_b
            nodes_b += 1
            self.nodes += 1
            t = float(x[i]) - c[i]
            t = t * t
            t = t * r[i][i]
            Pi = P[i + 1] + t
            if Pi < A:
                if i == kb:
                    zero = nodes_b == 1 if not plain else not any(x[kb:e + 1])
                    if not zero:
                        A = Pi
                        best = x[kb:e + 1]
                else:
                    P[i] = Pi
                    i -= 1
                    enter(i)
                    continue
            else:
                i += 1
                if i > e:
                    return best, 0, nodes_b
                if not plain and i > top:
                    top = i
            if not plain and i == top:
                x[i] += 1
            else:
                nxt[i] += 1
                x[i] += stp[i] * nxt[i]
                stp[i] = -stp[i]

    def insert(self, kb, e, best):
        d, b, U, G = self.d, self.b, self.U, self.G
        x = {kb + l: int(v) for l, v in enumerate(best)}
        for j in range(e, kb, -1):
            i = j - 1
            while x[j] != 0:
                q = abs(x[i]) // abs(x[j])
                if (x[i] < 0) != (x[j] < 0):
                    q = -q
                nb = [u + q * v for u, v in zip(b[j], b[i])]
                nU = [u + q * v for u, v in zip(U[j], U[i])]
                if any(abs(v) >= B_LIMIT for v in nb) or any(abs(v) >= U_LIMIT for v in nU):
                    raise _Stop(2, "insert")
                b[j], U[j] = nb, nU
                self.steps += 1
                x[i] -= q * x[j]
                b[i], b[j] = b[j], b[i]
                U[i], U[j] = U[j], U[i]
                x[i], x[j] = x[j], x[i]
        for k in range(kb, e + 1):
            for j in range(d):
                G[k][j] = G[j][k] = sum(u * v for u, v in zip(b[k], b[j]))

    def tour(self, block_size, enum_nodes, plain=False):
        """One tour; returns its insertions."""
        d, r = self.d, self.r
        ins = 0
        for kb in range(d - 1):
            e = min(kb + block_size, d) - 1
            before = self.nodes
            try:
                best, trunc, nodes_b = self.enum(kb, e, enum_nodes, plain)
            finally:
                self.trace.append(("enum", self.nodes - before))
            self.blocks += 1
            self.truncated += trunc
            self.log.append((kb, e, nodes_b, trunc, best))
            if best is not None:
                self.insert(kb, e, best)
                self.insertions += 1
                ins += 1
                if kb == 0:
                    r[0][0] = float(self.G[0][0])
                    if not _good(r[0][0]):
                        raise _Stop(3)
                self.lll(max(kb, 1))
        return ins

    def result(self, status, where=None):
        d, b, U = self.d, self.b, self.U
        return {"where": where, "steps": self.steps,
                "basis_out": [[b[i][c] for i in range(d)] for c in range(d)],
                "U_out": [[U[i][c] for i in range(d)] for c in range(d)],
                "swaps": self.swaps, "iters": self.iters, "passes": self.passes, "tours": self.tours,
                "blocks": self.blocks, "insertions": self.insertions, "nodes": self.nodes,
                "truncated": self.truncated, "status": status, "gs_norm2": [self.r[i][i] for i in range(d)],
                "log": self.log, "trace": self.trace}


def bkz(basis, block_size, delta=0.99, eta=0.51, max_tours=1 << 40, max_iters=1 << 40, enum_nodes=1 << 40,
        plain=False):
    """lgs_bkz_reduce of one basis.  Returns a dict with the fields of FIELDS and ``log``, the
    list of (kb, e, nodes_b, trunc, best) per block enumeration, ``where`` (the part of the definition
    that stopped the call: "lll", "enum", "insert" or "tour"), ``steps`` (Euclid steps applied) and
    ``trace``, the LLL runs and block enumerations in order with what each spent (for schedule())."""
    s = _State(basis, delta, eta, max_iters)
    try:
        s.chol(0)
        if not _good(s.r[0][0]):
            raise _Stop(3)
        s.lll(1)
        while True:
            if s.tours == max_tours:
                raise _Stop(4, "tour")
            s.tours += 1
            if s.tour(block_size, enum_nodes, plain) == 0:
                raise _Stop(0, "tour")
    except _Stop as stop:
        return s.result(stop.status, stop.where)


def plain_tour_insertions(basis, block_size, delta=0.99, eta=0.51):
    """Insertions of one tour of the plain enumeration on ``basis`` (0: every block's first
    vector is the shortest of its projected block up to delta)."""
    return bkz(basis, block_size, delta, eta, max_tours=1, plain=True)["insertions"]


# ---------------------------------------------------------------- the parity cases
# (name, block_size, delta); "lll64" is the LLL-reduced qary64 (delta 0.75) of lll_oracle, run for
# two tours only: the oracle needs 2 s for those and minutes for the whole reduction.
CASES = (("d2", 2, 0.99), ("d3", 3, 0.99), ("qary8", 4, 0.99), ("qary12", 6, 0.99), ("qary12", 12, 0.99),
         ("qary16", 8, 0.99), ("ntru24", 10, 0.99), ("ntru24", 24, 0.99), ("qary32", 12, 0.99),
         ("qary32", 32, 0.99), ("qary40", 16, 0.99), ("qary40", 16, 0.75), ("lll64", 12, 0.75))
SLICE_CASES = (("qary16", 8), ("ntru24", 10), ("qary32", 12))
_cache = {}


def basis(name):
    if name == "lll64":
        return np.array(lll_oracle.reduced("qary64", 0.75)["basis_out"], dtype=np.int64)
    return lll_oracle.bases()[name]


def reduced(name, block_size, delta=0.99, **kw):
    """bkz() of a test basis, computed once per process and not to be modified."""
    if name == "lll64":
        kw.setdefault("max_tours", 2)
    key = (name, block_size, delta, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = bkz(basis(name).tolist(), block_size, delta, 0.51, **kw)
    return _cache[key]


# (name, block_size, max_tours), all at (0.99, 0.51): the dense signed bases of lll_oracle at the
# d where the ownership of lanes changes, and the two rounding ties that half-even and half-away
# resolve differently (lll_loop is shared).  dense63 runs one tour: the oracle needs 0.8 s for it.
DENSE_CASES = (("dense7", 4, 1 << 40), ("dense17", 6, 1 << 40), ("dense33", 10, 1 << 40), ("dense63", 8, 1),
               ("tie2.5", 2, 1 << 40), ("tie-2.5", 2, 1 << 40))


def schedule(o, lll_slice=LLL_SLICE, node_slice=BKZ_SLICE):
    """What the kernel's state machine makes of one oracle result under forced slices: (reduction
    launches, suspensions inside an LLL run, suspensions inside an enumeration).  A launch has
    lll_slice main-loop iterations and node_slice nodes to spend on whatever comes, in the order of
    o["trace"]; it suspends the basis when a run or a block needs one more than is left (both
    loops test their own end -- k = d, max_iters, enum_nodes, the block exhausted -- before the
    budget, so spending the last of a budget on the last step suspends nothing)."""
    launches, in_lll, in_enum = 1, 0, 0
    left = {"lll": lll_slice, "enum": node_slice}
    for kind, n in o["trace"]:
        while n > left[kind]:
            n -= left[kind]
            launches += 1
            in_lll += kind == "lll"
            in_enum += kind == "enum"
            left = {"lll": lll_slice, "enum": node_slice}
        left[kind] -= n
    return launches, in_lll, in_enum


MIXED_D, MIXED_BETA = 17, 6
MIXED_DENSE = ((500, 3), (500, 1000), (501, 1000), (502, 3), (503, 30), (504, 1000))  # (seed, amp)
_mixed = {}


def mixed_batch():
    """The d = 17 batch of the scheduling test, (n, 17, 17) int64: six dense bases, and among them
    the entries that leave the live list early -- the identity, a BKZ-reduced basis (the oracle's
    output for the first entry), a singular matrix -- and a repeat.  Not to be modified."""
    if "bases" not in _mixed:
        d = MIXED_D
        ds = [lll_oracle.dense(d, s, amp) for s, amp in MIXED_DENSE]
        red = np.array(bkz(ds[0].tolist(), MIXED_BETA)["basis_out"], dtype=np.int64)
        sing = lll_oracle.dense(d, 7002, 30).copy()
        sing[:, 9] = sing[:, 3] + sing[:, 6]
        _mixed["bases"] = np.ascontiguousarray(
            np.stack([ds[0], np.eye(d, dtype=np.int64), ds[1], ds[2], sing, ds[3], red, ds[4], ds[1], ds[5]]))
    return _mixed["bases"]


MIXED_MAX_TOURS = 2  # the budget of the run in which status 4 and status 0 meet


def mixed_reduced(max_tours=1 << 40):
    """bkz() of every entry of mixed_batch() at beta = MIXED_BETA, (0.99, 0.51), once per process."""
    if max_tours not in _mixed:
        _mixed[max_tours] = [bkz(x.tolist(), MIXED_BETA, max_tours=max_tours) for x in mixed_batch()]
    return _mixed[max_tours]


def chunk_reduced():
    """index of lll_oracle.chunk_batch() -> bkz() at beta = 2, (0.99, 0.51), once per process."""
    if "chunk" not in _mixed:
        B, idx = lll_oracle.chunk_batch()
        _mixed["chunk"] = {v: bkz(B[idx.index(v)].tolist(), 2) for v in sorted(set(idx))}
    return _mixed["chunk"]


GUARD_SCALE = 25600000


def guard_basis():
    """The LLL-reduced qary12 times GUARD_SCALE (largest |entry| 0.86 * 2^28): the initial LLL has
    nothing to do, the first block (beta = 12) finds the vector of norm 125 s^2, and the second
    step of Euclid in its INSERT would carry a coordinate past 2^28."""
    return [[v * GUARD_SCALE for v in row] for row in lll_oracle.reduced("qary12", 0.99)["basis_out"]]


def as_arrays(o):
    """The oracle's result in the dtypes of the C-ABI's outputs."""
    out = {f: np.int64(o[f]) for f in FIELDS}
    out["basis_out"] = np.array(o["basis_out"], dtype=np.int64)
    out["U_out"] = np.array(o["U_out"], dtype=np.int64)
    out["status"] = np.int32(o["status"])
    out["gs_norm2"] = np.array(o["gs_norm2"], dtype=np.float64)
    return out
