"""CPU oracle of lgs_lll_reduce: the operational definition of include/lgs.h transcribed into
Python ints (exact) and floats (IEEE fp64, one rounding per operation, round() = half-even),
and an exact-rational Gram-Schmidt checker of what it returns.

Conventions are the C-ABI's: ``basis`` is d x d, vector b_i is COLUMN i, and the result
satisfies basis_out = basis @ U.  The test bases live here too, so the host test (premises on
the oracle) and the device test (parity) use the same ones, reduced once per process.
"""
from fractions import Fraction

import numpy as np

B_LIMIT = 1 << 28
U_LIMIT = 1 << 40
X_LIMIT = float(1 << 22)
SLICE = 16  # main-loop iterations per launch that the device slice test forces


def lll(basis, delta=0.99, eta=0.51, max_iters=1 << 40):
    """lgs_lll_reduce of one basis.  Returns a dict: basis_out, U_out (d x d lists of ints, vectors
    in columns), swaps, iters, passes, status, gs_norm2 (d floats)."""
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
                    X = float(round(mu[k][j]))
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
    return out


# The parity cases.  qary64 fills the wave and the LDS budget; the oracle needs 3 s for it at
# delta = 0.75 and 9 s at 0.99, so it runs at 0.75 only and qary40 covers 0.99 above half a wave.
# qary12 is the end-to-end basis.
NAMES = ("d2", "d3", "qary8", "qary16", "ntru24", "qary32", "qary40", "qary64")
CASES = tuple((n, dl) for n in NAMES for dl in (0.75, 0.99) if (n, dl) != ("qary64", 0.99))
_cache = {}


def reduced(name, delta, max_iters=1 << 40):
    """lll() of a test basis, computed once per process and not to be modified."""
    key = (name, delta, max_iters)
    if key not in _cache:
        _cache[key] = lll(bases()[name].tolist(), delta, 0.51, max_iters)
    return _cache[key]


def as_arrays(o):
    """The oracle's result in the dtypes of the C-ABI's outputs."""
    return {"basis_out": np.array(o["basis_out"], dtype=np.int64), "U_out": np.array(o["U_out"], dtype=np.int64),
            "swaps": np.int64(o["swaps"]), "iters": np.int64(o["iters"]), "passes": np.int64(o["passes"]),
            "status": np.int32(o["status"]), "gs_norm2": np.array(o["gs_norm2"], dtype=np.float64)}
