"""CPU oracle of lgs_lll_reduce: the operational definition of include/lgs.h transcribed into
Python ints (exact) and floats (IEEE fp64, one rounding per operation, round() = half-even),
and an exact-rational Gram-Schmidt checker of what it returns.

Conventions are the C-ABI's: ``basis`` is d x d, vector b_i is COLUMN i, and the result
satisfies basis_out = basis @ U.  The test bases live here too, so the host test (premises on
the oracle) and the device test (parity) use the same ones, reduced once per process.
"""
import math
from fractions import Fraction

import numpy as np

B_LIMIT = 1 << 28
U_LIMIT = 1 << 40
X_LIMIT = float(1 << 22)
SLICE = 16  # main-loop iterations per launch that the device slice test forces


def lll(basis, delta=0.99, eta=0.51, max_iters=1 << 40, rnd=round):
    """lgs_lll_reduce of one basis.  Returns a dict: basis_out, U_out (d x d lists of ints, vectors
    in columns), swaps, iters, passes, status, gs_norm2 (d floats).  ``rnd`` is the rounding of
    the size reduction: the definition's is round(), half-even; the host test passes half_away to
    show which inputs tell the two apart."""
    d = len(basis)
    b = [[int(basis[c][i]) for c in range(d)] for i in range(d)]  # b[i] = column i
    U = [[int(i == c) for c in range(d)] for i in range(d)]
    G = [[sum(x * y for x, y in zip(b[i], b[j])) for j in range(d)] for i in range(d)]
    mu = [[0.0] * d for _ in range(d)]
    r = [[0.0] * d for _ in range(d)]
    swaps = iters = passes = 0

    def chol(k):
        rk, Gk = r[k], G[k]
        for j in range(k + 1):
            s, muj = float(Gk[j]), mu[j]
            for i in range(j):
                s = s - muj[i] * rk[i]
            rk[j] = s
            if j < k:
                mu[k][j] = s / r[j][j]

    def good(x):
        return x > 0.0 and x != float("inf")

    def result(status):
        return {"basis_out": [[b[i][c] for i in range(d)] for c in range(d)],
                "U_out": [[U[i][c] for i in range(d)] for c in range(d)],
                "swaps": swaps, "iters": iters, "passes": passes, "status": status,
                "gs_norm2": [r[i][i] for i in range(d)]}

    chol(0)
    if not good(r[0][0]):
        return result(3)
    k = 1
    while k < d:
        if iters == max_iters:
            return result(1)
        iters += 1
        while True:
            passes += 1
            chol(k)
            applied = False
            for j in range(k - 1, -1, -1):
                if abs(mu[k][j]) > eta:
                    X = float(rnd(mu[k][j]))
                    if not abs(X) < X_LIMIT:
                        return result(2)
                    Xi = int(X)
                    nb = [x - Xi * y for x, y in zip(b[k], b[j])]
                    nU = [x - Xi * y for x, y in zip(U[k], U[j])]
                    if any(abs(x) >= B_LIMIT for x in nb) or any(abs(x) >= U_LIMIT for x in nU):
                        return result(2)
                    b[k], U[k] = nb, nU
                    for i in range(j):
                        mu[k][i] = mu[k][i] - X * mu[j][i]
                    mu[k][j] = mu[k][j] - X
                    applied = True
            if not applied:
                break
            for j in range(d):
                G[k][j] = G[j][k] = sum(x * y for x, y in zip(b[k], b[j]))
        if not good(r[k][k]):
            return result(3)
        t = mu[k][k - 1] * mu[k][k - 1]
        t = delta - t
        t = t * r[k - 1][k - 1]
        if r[k][k] >= t:
            k += 1
        else:
            b[k], b[k - 1] = b[k - 1], b[k]
            U[k], U[k - 1] = U[k - 1], U[k]
            G[k], G[k - 1] = G[k - 1], G[k]
            for row in G:
                row[k], row[k - 1] = row[k - 1], row[k]
            swaps += 1
            if k == 1:
                r[0][0] = float(G[0][0])
                if not good(r[0][0]):
                    return result(3)
            k = max(k - 1, 1)
    return result(0)


def half_away(x):
    """Round to nearest, ties away from zero: what the definition does NOT do."""
    whole = math.floor(abs(x))
    return int(math.copysign(whole + (abs(x) - whole >= 0.5), x))  # (the difference is exact)


def matmul(A, B):
    """Exact integer product of two d x d lists."""
    d = len(A)
    Bt = list(zip(*B))
    return [[sum(x * y for x, y in zip(A[i], Bt[j])) for j in range(d)] for i in range(d)]


def det_bareiss(M):
    """Exact integer determinant (fraction-free elimination)."""
    A = [[int(x) for x in row] for row in M]
    n = len(A)
    sign, prev = 1, 1
    for k in range(n - 1):
        if A[k][k] == 0:
            p = next((i for i in range(k + 1, n) if A[i][k] != 0), None)
            if p is None:
                return 0
            A[k], A[p] = A[p], A[k]
            sign = -sign
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                A[i][j] = (A[i][j] * A[k][k] - A[i][k] * A[k][j]) // prev
        prev = A[k][k]
    return sign * A[n - 1][n - 1]


def gso_excess(basis_out, delta, eta):
    """Exact-rational Gram-Schmidt of the columns of basis_out.  Returns (mu_excess,
    lovasz_deficit): the largest |mu_kj| - eta and the largest delta - (|b*_k|^2 / |b*_{k-1}|^2
    + mu_{k,k-1}^2) over the basis, as Fractions (negative: the condition holds with room)."""
    d = len(basis_out)
    b = [[int(basis_out[c][i]) for c in range(d)] for i in range(d)]
    G = [[sum(x * y for x, y in zip(b[i], b[j])) for j in range(d)] for i in range(d)]
    mu = [[Fraction(0)] * d for _ in range(d)]
    r = [[Fraction(0)] * d for _ in range(d)]
    for k in range(d):
        for j in range(k + 1):
            s = Fraction(G[k][j])
            for i in range(j):
                s -= mu[j][i] * r[k][i]
            r[k][j] = s
            if j < k:
                mu[k][j] = s / r[j][j]
    fe, fd = Fraction(eta), Fraction(delta)
    mu_excess = max(abs(mu[k][j]) - fe for k in range(1, d) for j in range(k))
    deficit = max(fd - (r[k][k] / r[k - 1][k - 1] + mu[k][k - 1] ** 2) for k in range(1, d))
    return mu_excess, deficit


# ---------------------------------------------------------------- the test bases
def bases():
    """name -> d x d int64 array, vectors in columns: the smallest at which each mechanism of
    the kernel can go wrong (one lane pair, an odd d, a q-ary block, ragged against 16 and 32,
    half a wave, a whole wave)."""
    from lgs_amd import lattices
    rows = {"qary8": lattices.qary_basis(4, 4, 97), "qary12": lattices.qary_basis(6, 6, 97),
            "qary16": lattices.qary_basis(8, 8, 3329), "ntru24": lattices.ntru_basis(12, 12289),
            "qary32": lattices.qary_basis(16, 16, 3329), "qary40": lattices.qary_basis(20, 20, 3329),
            "qary64": lattices.qary_basis(32, 32, 3329)}
    # the builders return row bases [[q I, 0], [A, I]]: their rows become the columns here
    out = {k: np.ascontiguousarray(np.asarray(v).T).astype(np.int64) for k, v in rows.items()}
    out["d2"] = np.array([[1, 0], [7, 1]], dtype=np.int64)
    out["d3"] = np.array([[1, 0, 0], [11, 1, 0], [5, 3, 29]], dtype=np.int64)
    for name, d, amp in DENSE:
        out[name] = dense(d, 100 + d, amp)
    out.update(TIES)
    out.update(big_bases())
    return out


_dense = {}


def dense(d, seed, amp):
    """A dense signed basis: entries uniform on -amp..amp, redrawn until the determinant is not
    zero.  Computed once per process and not to be modified."""
    if (d, seed, amp) not in _dense:
        rng = np.random.default_rng(seed)
        while True:
            M = rng.integers(-amp, amp + 1, (d, d)).astype(np.int64)
            if det_bareiss(M.tolist()) != 0:
                break
        _dense[(d, seed, amp)] = M
    return _dense[(d, seed, amp)]


# Dense signed bases at the d where the ownership of lanes changes (act = lane < d, the pitch
# d | 1, the 8-wide Cholesky wavefront and its tail): (name, d, amp), seed 100 + d.
DENSE = (("dense5", 5, 50), ("dense7", 7, 1000), ("dense17", 17, 1000), ("dense33", 33, 100), ("dense63", 63, 20),
         ("dense64", 64, 20))
DENSE_NAMES = tuple(n for n, _, _ in DENSE)
# (delta, eta): the usual pair, a lax one, and one at the edge of both ranges
DENSE_PARAMS = ((0.99, 0.51), (0.3, 0.95), (0.999999, 0.500001))
DENSE_CASES = tuple((n, dl, et) for n in DENSE_NAMES for dl, et in DENSE_PARAMS)

# 2 x 2 bases whose first mu[1][0] = G[1][0] / G[0][0] is a tie of the rounding: 2.5, -2.5, 3.5,
# 1.5 and 1.5 (as 6/4).  Half-even and half-away differ on the first two and agree on the rest.
TIES = {"tie2.5": np.array([[2, 5], [0, 1]], dtype=np.int64), "tie-2.5": np.array([[2, -5], [0, 1]], dtype=np.int64),
        "tie3.5": np.array([[2, 7], [0, 1]], dtype=np.int64), "tie1.5": np.array([[2, 3], [0, 1]], dtype=np.int64),
        "tie6/4": np.array([[4, 6], [0, 1]], dtype=np.int64)}
TIE_NAMES = tuple(TIES)


def big_bases():
    """big4 and big9, drawn in this order from one generator: entries up to 2^27 + 12345 in
    magnitude, so that Gram entries pass 2^53 and (double)G rounds."""
    if "big" not in _dense:
        rng, M = np.random.default_rng(5), 2 ** 27 + 12345
        _dense["big"] = {f"big{d}": rng.integers(-M, M, (d, d)).astype(np.int64) for d in (4, 9)}
    return _dense["big"]


BIG_NAMES = ("big4", "big9")


def gram(basis):
    """The exact Gram matrix of the columns of ``basis``, as Python ints."""
    d = len(basis)
    b = [[int(basis[c][i]) for c in range(d)] for i in range(d)]
    return [[sum(x * y for x, y in zip(b[i], b[j])) for j in range(d)] for i in range(d)]


def launches(o, slice_=None):
    """Reduction launches one basis needs at ``slice_`` main-loop iterations per launch.  lll_loop
    tests k >= d and iters == max_iters before the launch's budget, so a launch that completes
    the last iteration also ends the basis; a basis that stops before its first iteration (status
    3 from chol(0)) still takes the one launch that writes its outputs."""
    s = SLICE if slice_ is None else slice_
    return max(1, -(-o["iters"] // s))


_mixed = {}


def mixed_batch():
    """The d = 17 batch of the scheduling test: (bases (n, 17, 17) int64, oracle results).  Dense
    bases of three amplitudes, so that the iteration counts spread, and between them the entries
    that leave the live list at once: the identity (16 iterations, exactly one slice), a reduced
    basis, two singular matrices (equal columns 0 and 1; column 9 the sum of columns 3 and 6) and a
    repeat.  Computed once per process and not to be modified."""
    if "bases" not in _mixed:
        d = 17
        ds = [dense(d, s, amp) for s in MIXED_SEEDS for amp in (3, 30, 1000)]
        eq = dense(d, 7001, 30).copy()
        eq[:, 1] = eq[:, 0]
        dep = dense(d, 7002, 30).copy()
        dep[:, 9] = dep[:, 3] + dep[:, 6]
        red = np.array(reduced("dense17", 0.99)["basis_out"], dtype=np.int64)
        batch = ds[:3] + [np.eye(d, dtype=np.int64)] + ds[3:9] + [eq] + ds[9:14] + [red, ds[1]] + ds[14:20] + \
            [dep] + ds[20:]
        _mixed["bases"] = np.ascontiguousarray(np.stack(batch))
    return _mixed["bases"]


MIXED_SEEDS = tuple(range(500, 508))  # each at the three amplitudes
MIXED_MAX_ITERS = 250  # the budget of the run in which status 1 and status 0 meet


def mixed_reduced(max_iters=1 << 40):
    """lll() of every entry of mixed_batch() at (0.99, 0.51), once per process."""
    if max_iters not in _mixed:
        _mixed[max_iters] = [lll(x.tolist(), 0.99, 0.51, max_iters) for x in mixed_batch()]
    return _mixed[max_iters]


CHUNK_D, CHUNK_DISTINCT, CHUNK_N = 3, 130, 1024 + 6  # kLllChunk = 1024 (test_lll_host.py reads it)
CHUNK_SINGULAR = (1023, 1024)  # the last basis of the first chunk and the first of the second


def chunk_batch():
    """(bases (CHUNK_N, 3, 3), index of each entry's distinct basis; -1 - s for singular s): 130
    dense bases cycled over more than one chunk of the scheduler, a singular one on either side
    of the chunk boundary."""
    if "chunk" not in _mixed:
        idx = [p % CHUNK_DISTINCT for p in range(CHUNK_N)]
        idx[CHUNK_SINGULAR[0]], idx[CHUNK_SINGULAR[1]] = -1, -2
        sing = (np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.int64),
                np.array([[2, -4, 1], [3, -6, 5], [-1, 2, 7]], dtype=np.int64))
        B = np.stack([sing[-1 - v] if v < 0 else dense(CHUNK_D, 900 + v, 200) for v in idx])
        _mixed["chunk"] = (B, tuple(idx))
    return _mixed["chunk"]


def chunk_reduced():
    """index of chunk_batch() -> lll() at (0.99, 0.51), once per process."""
    if "chunk_lll" not in _mixed:
        B, idx = chunk_batch()
        _mixed["chunk_lll"] = {v: lll(B[idx.index(v)].tolist()) for v in sorted(set(idx))}
    return _mixed["chunk_lll"]


# The parity cases.  qary64 fills the wave and the LDS budget; the oracle needs 3 s for it at
# delta = 0.75 and 9 s at 0.99, so it runs at 0.75 only and qary40 covers 0.99 above half a wave.
# qary12 is the end-to-end basis.
NAMES = ("d2", "d3", "qary8", "qary16", "ntru24", "qary32", "qary40", "qary64")
CASES = tuple((n, dl) for n in NAMES for dl in (0.75, 0.99) if (n, dl) != ("qary64", 0.99))
_cache = {}


def reduced(name, delta, max_iters=1 << 40, eta=0.51):
    """lll() of a test basis, computed once per process and not to be modified."""
    key = (name, delta, max_iters, eta)
    if key not in _cache:
        _cache[key] = lll(bases()[name].tolist(), delta, eta, max_iters)
    return _cache[key]


def as_arrays(o):
    """The oracle's result in the dtypes of the C-ABI's outputs."""
    return {"basis_out": np.array(o["basis_out"], dtype=np.int64), "U_out": np.array(o["U_out"], dtype=np.int64),
            "swaps": np.int64(o["swaps"]), "iters": np.int64(o["iters"]), "passes": np.int64(o["passes"]),
            "status": np.int32(o["status"]), "gs_norm2": np.array(o["gs_norm2"], dtype=np.float64)}
