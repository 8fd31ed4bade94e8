"""GPU: the Babai decoders (nearest_plane_kernel<ZT, 16 | 32>, round_kernel, the fp64 MFMA
frame GEMM and run_decode's copies) where test_gpu_decode.py cannot see a wrong answer.

Exact frames.  With Q = I the GEMM returns c' = t exactly, and with small dyadic inputs
every sum and the subtraction of include/lgs.h's rule

    z_i = round-half-even((c'_i - sum_{j>i} R_ij z_j) / R_ii)

are exact in fp64 in any order, so only the division rounds, the device has exactly one
correct answer and targets can sit ON the rounding boundary (k + 1/2) and one step beside
it.  Round-half-away for rint, a multiplication by 1 / R_ii for the division, or a far
field that loses low bits turn these tests red.  The rounding decoder gets the same with
B = U D (U unit upper bidiagonal, D powers of two): B^-1 is dyadic and w = B^-1 t is exact
in any summation order.  Non-dyadic B^-1 is left out on purpose: round(B^-1 t) with a
rounded B^-1 differs legitimately from solve-then-round at one ulp of w.

General frames.  Real Q at d = 1 .. 100 around the 16- and 32-row panel edges and batch
sizes around the 64-sample tile and the 256-lane block, against the extended-precision
walk of oracle/lgs_decode_oracle.py: a decision whose distance from the rounding boundary
exceeds the fp64 error bound of the rule must equal the reference; at most 1 % of the
targets of a case may hold a decision inside the bound (the recipe gives none: the
smallest margin is above 1e3 bounds).

Also here: every buffer layout of run_decode, its chunk loop (hooks build,
LGS_TEST_DECODE_CHUNK), the int32 edge at +-2^31, one non-finite target in a batch, and
lgs_set_basis discarding the decoding frame."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import lgs_decode_oracle as DO

pytestmark = pytest.mark.gpu

N = 321          # targets per case: two 256-lane blocks, six 64-sample tiles, both ragged
S = 2.0 ** -20   # the grid every exact-frame quantity lies on
SMALL_K = (-2, -1, 0, 1)  # ties at -1.5, -0.5, 0.5, 1.5: half-even and half-away differ on each


def _context(R, B, Q, Binv=None, *, panel=32, hooks=False, sigma=1.0):
    from lgs_amd import _capi
    ctx = _capi.Context(0, panel=panel, hooks=hooks)
    ctx.set_basis(R, np.zeros(R.shape[0]), B, sigma)
    ctx.set_decoder(Q, Binv)
    return ctx


def _tie_classes(rng, n):
    """k (integers in [-1000, 1000], SMALL_K forced), e (0, +-2^-20, each forced beside each
    small k) and the mask of the quarter of entries that take a generic grid point instead,
    scattered over the n targets."""
    k = rng.integers(-1000, 1001, n).astype(np.float64)
    e = rng.choice([0.0, S, -S], n)
    generic = rng.random(n) < 0.25
    f = len(SMALL_K)
    for a, ev in enumerate((0.0, S, -S)):
        k[a * f:(a + 1) * f] = SMALL_K
        e[a * f:(a + 1) * f] = ev
    generic[:3 * f] = False
    p = rng.permutation(n)
    return k[p], e[p], generic[p]


# ---------------------------------------------------------------- nearest plane, coupled walk
DIAG = (1.0, 2.0, 3.0, 4.0, 5.0, 8.0)  # 3 and 5: the division really rounds


@functools.lru_cache(maxsize=None)
def _coupled_case(d):
    """(U, T, Z): an integer upper-triangular frame, targets built backwards so that the
    walk's mean x_i / U_ii is a tie, 2^-20 / U_ii beside one, or a generic grid point, and
    the coefficients the rule gives.  Every quantity is a multiple of 2^-20 below 2^20."""
    rng = np.random.default_rng(7100 + d)
    U = np.triu(rng.integers(-3, 4, (d, d)).astype(np.float64), 1)
    dg = rng.choice(DIAG, d)
    dg[:min(d, 2)] = (3.0, 5.0)[:min(d, 2)]
    if d >= len(DIAG):
        dg[-len(DIAG):] = DIAG
    U[np.diag_indices(d)] = dg
    X, Z, T = np.zeros((N, d)), np.zeros((N, d)), np.zeros((N, d))
    for i in range(d - 1, -1, -1):
        k, e, generic = _tie_classes(rng, N)
        x = U[i, i] * (k + 0.5) + e
        x[generic] = rng.integers(-1000 << 20, (1000 << 20) + 1, int(generic.sum())) * S
        X[:, i] = x
        Z[:, i] = np.rint(x / U[i, i])  # one IEEE division
        T[:, i] = x + Z[:, i + 1:] @ U[i, i + 1:]
    assert np.abs(T).max() < 2.0 ** 20 and np.array_equal(T, np.rint(T / S) * S)
    ties = np.abs(X / dg - np.floor(X / dg) - 0.5) == 0.0
    assert ties.sum() >= N * d // 8 and ties.any(axis=0).all()
    # the construction is exact: redone in rationals on a few targets, where the rule's
    # exact value rounds (half to even) to the same coefficients as the fp64 division
    for r in range(0, N, 40):
        for i in range(d - 1, -1, -1):
            x = Fraction(T[r, i]) - sum(Fraction(U[i, j]) * int(Z[r, j]) for j in range(i + 1, d))
            assert x == Fraction(X[r, i]) and round(x / Fraction(U[i, i])) == int(Z[r, i])
    return U, T, Z.astype(np.int64)


@pytest.mark.parametrize("panel", [32, 16])
@pytest.mark.parametrize("d", [1, 2, 16, 17, 32, 33, 65])
def test_nearest_plane_coupled_walk_decides_ties(d, panel):
    U, T, Z = _coupled_case(d)
    ctx = _context(U, U, np.eye(d), panel=panel)
    z, v = ctx.decode_host(T, "plane")
    bad = np.argwhere(z != Z)
    assert bad.size == 0, (f"{len(bad)} of {Z.size} coefficients differ, first (target, i) = {bad[0]}: "
                           f"device {z[tuple(bad[0])]}, rule {Z[tuple(bad[0])]}")
    np.testing.assert_array_equal(v, (Z @ U.T.astype(np.int64)).astype(np.float64))


# ---------------------------------------------------------------- diagonal frames, one ulp from the tie
POW2 = tuple(2.0 ** e for e in range(-3, 4))


def _one_ulp_targets(rii, m, seed):
    """(3 m, d) targets fl(R_ii (k + 1/2)) and their two fp64 neighbours, k of both signs up
    to 2^20 and small (-1 and 0 forced)."""
    rng = np.random.default_rng(seed)
    d = len(rii)
    k = np.where(rng.random((m, d)) < 0.3, rng.integers(-4, 4, (m, d)), rng.integers(-(1 << 20), 1 << 20, (m, d)))
    k[0], k[1] = -1, 0
    t = rii * (k + 0.5)
    return np.concatenate([t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)])


@functools.lru_cache(maxsize=None)
def _one_ulp_case(name):
    if name == "d33":
        rii = np.array((POW2 + (3.0, 5.0)) * 4)[:33]
        T = _one_ulp_targets(rii, N // 3, 7200)
    else:  # d = 1: one frame per diagonal value
        rii = np.array([float(name[2:])])
        T = _one_ulp_targets(rii, 1000, 7201)
    want = np.rint(T / rii)
    # the inputs tell the division from a multiplication by the reciprocal
    recip = np.rint(T * (1.0 / rii))
    for c in np.flatnonzero((rii == 3.0) | (rii == 5.0)):
        assert (recip[:, c] != want[:, c]).any(), f"column {c} (R_ii = {rii[c]}) cannot tell / from * (1 / R_ii)"
    assert np.array_equal(recip[:, (rii != 3.0) & (rii != 5.0)], want[:, (rii != 3.0) & (rii != 5.0)])
    return rii, T, want.astype(np.int64)


@pytest.mark.parametrize("name", ["d33", "r=3", "r=5", "r=0.125", "r=8"])
def test_nearest_plane_one_ulp_from_the_tie(name):
    rii, T, want = _one_ulp_case(name)
    R = np.diag(rii)
    ctx = _context(R, R, np.eye(len(rii)))
    z, v = ctx.decode_host(T, "plane")
    bad = np.argwhere(z != want)
    assert bad.size == 0, (f"{len(bad)} of {want.size} differ, first (target, i) = {bad[0]}: t = "
                           f"{T[tuple(bad[0])].hex()}, R_ii = {rii[bad[0][1]]}, device {z[tuple(bad[0])]}, "
                           f"rint(t / R_ii) {want[tuple(bad[0])]}")
    np.testing.assert_array_equal(v, want * rii)


@pytest.mark.parametrize("d", [1, 33])
def test_round_decode_one_ulp_from_the_tie(d):
    """B = diag(powers of two): w = t / B_ii is exact, t one ulp beside B_ii (k + 1/2)."""
    bii = np.array(POW2 * 5)[2:2 + d]
    T = _one_ulp_targets(bii, N // 3 if d > 1 else 1000, 7300 + d)
    want = np.rint(T / bii).astype(np.int64)
    B = np.diag(bii)
    ctx = _context(B, B, np.eye(d), np.diag(1.0 / bii))
    z, v = ctx.decode_host(T, "round")
    np.testing.assert_array_equal(z, want)
    np.testing.assert_array_equal(v, want * bii)


# ---------------------------------------------------------------- rounding decode, dyadic frames
@functools.lru_cache(maxsize=None)
def _round_case(d):
    """(B, Binv, T, Z): B = U D with U unit upper bidiagonal (superdiagonal in {-1, 0, 1}) and
    D powers of two, its exact dyadic inverse, targets t = B w with w a tie, 2^-20 beside
    one, or a generic grid point."""
    rng = np.random.default_rng(7400 + d)
    u = rng.integers(-1, 2, max(d - 1, 0))
    u[:3] = (-1, 1, 0)[:len(u[:3])]
    D = 2.0 ** rng.integers(-2, 4, d)
    U = np.eye(d) + np.diag(u.astype(np.float64), 1)
    B = U * D[None, :]
    Ui = [[int(i == j) for j in range(d)] for i in range(d)]  # U^-1 in Python integers
    for i in range(d - 2, -1, -1):
        for j in range(i + 1, d):
            Ui[i][j] = -int(u[i]) * Ui[i + 1][j]
    Binv = np.array(Ui, dtype=np.float64) / D[:, None]
    # B Binv = I exactly, in integers: 4 B and 8 Binv are integral
    Bi, Vi = (4 * B).astype(np.int64), (8 * Binv).astype(np.int64)
    assert np.array_equal(Bi, 4 * B) and np.array_equal(Vi, 8 * Binv)
    assert np.array_equal(Bi @ Vi, 32 * np.eye(d, dtype=np.int64)) and set(np.unique(Ui)) <= {-1, 0, 1}
    W = np.zeros((N, d))
    for i in range(d):
        k, e, generic = _tie_classes(rng, N)
        W[:, i] = k + 0.5 + e
        W[generic, i] = rng.integers(-1000 << 20, (1000 << 20) + 1, int(generic.sum())) * S
    T = W @ B.T  # two non-zero terms per row, multiples of 2^-22: exact
    for r in range(0, N, 40):  # B^-1 t is w, exactly
        tf = [Fraction(x) for x in T[r]]
        for i in range(d):
            assert sum(Fraction(Binv[i, j]) * tf[j] for j in range(d)) == Fraction(W[r, i])
    assert (np.abs(W - np.floor(W) - 0.5) == 0.0).any(axis=0).all()
    return B, Binv, T, np.rint(W).astype(np.int64)


@pytest.mark.parametrize("d", [1, 2, 17, 33, 65])
def test_round_decode_decides_ties(d):
    B, Binv, T, Z = _round_case(d)
    ctx = _context(B, B, np.eye(d), Binv)  # B is upper triangular with a positive diagonal: its own R
    z, v = ctx.decode_host(T, "round")
    bad = np.argwhere(z != Z)
    assert bad.size == 0, (f"{len(bad)} of {Z.size} coefficients differ, first (target, i) = {bad[0]}: "
                           f"device {z[tuple(bad[0])]}, rint(w) {Z[tuple(bad[0])]}")
    np.testing.assert_array_equal(v, Z.astype(np.float64) @ B.T)


# ---------------------------------------------------------------- integer edges
EDGES = (2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1, 2 ** 52 + 1, -(2 ** 52 + 1))


@pytest.mark.parametrize("frame", ["identity", "triangular"])
def test_coefficients_at_the_int32_edge(frame):
    """+-2^31 is where int32 output ends: the last values inside are stored, the first
    outside raise LGS_ERR_OVERFLOW, LGS_Z64 holds all of them exactly and decode_host
    reruns with it.  (|z| >= 2^63 is outside int64 and outside the ABI: include/lgs.h.)"""
    from lgs_amd import _capi
    U = np.eye(2) if frame == "identity" else np.array([[1.0, 1.0], [0.0, 1.0]])
    Ui = np.eye(2) if frame == "identity" else np.array([[1.0, -1.0], [0.0, 1.0]])
    ctx = _context(U, U, np.eye(2), Ui)
    Uint = U.astype(np.int64)
    for val in EDGES:
        for pos in (0, 1):
            Z = np.array([[3, -4], [val, 5] if pos == 0 else [7, val], [-6, 2]], dtype=np.int64)
            V = Z @ Uint.T
            assert np.abs(V).max() < 2 ** 53
            T = V.astype(np.float64)
            for method in ("plane", "round"):
                z32, v = np.full((3, 2), 99, dtype=np.int32), np.empty((3, 2))
                if -2 ** 31 <= val < 2 ** 31:
                    ctx.decode(T, method, z32, v, 0)
                    np.testing.assert_array_equal(z32, Z)
                    np.testing.assert_array_equal(v, T)
                else:
                    with pytest.raises(_capi.LgsError) as err:
                        ctx.decode(T, method, z32, v, 0)
                    assert err.value.code == _capi.LGS_ERR_OVERFLOW
                z64, v = np.empty((3, 2), dtype=np.int64), np.empty((3, 2))
                ctx.decode(T, method, z64, v, _capi.LGS_Z64)
                np.testing.assert_array_equal(z64, Z)
                np.testing.assert_array_equal(v, T)
                z, v = ctx.decode_host(T, method)
                np.testing.assert_array_equal(z, Z)
                np.testing.assert_array_equal(v, T)


# ---------------------------------------------------------------- general frames, with a margin
DIMS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100)
GENERAL = [(k, d) for k in ("gauss", "int") for d in DIMS] + [("qary", 40), ("ntru", 40)]


@functools.lru_cache(maxsize=None)
def _general_case(kind, d):
    from lgs_amd import lattices
    rng = np.random.default_rng(7500 + 7 * d + len(kind))
    if kind == "gauss":
        B = 4.0 * rng.standard_normal((d, d)) + 12.0 * np.eye(d)
    elif kind == "int":
        B = np.rint(4.0 * rng.standard_normal((d, d))) + 40.0 * np.eye(d)
    else:
        B = lattices.qary_basis(20, 20, 3329, 5) if kind == "qary" else lattices.ntru_basis(20, 12289, 2)
    assert B.shape == (d, d)
    Q, R = DO.qr_frame(B)
    Binv = np.linalg.inv(B)
    T = 2500.0 * rng.standard_normal((N, d))
    s = {"B": B, "Q": Q, "R": R, "Binv": Binv, "T": T, "integral": kind != "gauss",
         "plane": DO.nearest_plane_margins(Q, R, T), "round": DO.round_decode_margins(Binv, T)}
    # the reference alone: the recipe leaves (almost) every target decided
    for m in ("plane", "round"):
        rows, zr, marg, bound = s[m]
        assert DO.undecided(zr, zr, marg, bound, "walk" if m == "plane" else "each")[1] <= len(rows) // 100
    return s


def _check_general(s, method, z, v, n=N, label=""):
    """Device z of the first n targets against the margin reference; v = B z."""
    rows, zr, marg, bound = s[method]
    keep = rows < n
    rows, zr, marg, bound = rows[keep], zr[keep], marg[keep], bound[keep]
    bad, und = DO.undecided(z[rows], zr, marg, bound, "walk" if method == "plane" else "each")
    d = s["B"].shape[0]
    print(f"  {label} d={d} n={n} {method}: undecided targets {und} of {len(rows)}, "
          f"smallest margin / bound {float((marg / bound).min()):.3g}")
    assert bad == 0, f"{bad} decisions outside the error bound differ from the reference"
    assert und <= len(rows) / 100.0, f"{und} of {len(rows)} targets undecided"
    if s["integral"]:
        np.testing.assert_array_equal(v, (z @ s["B"].T.astype(np.int64)).astype(np.float64))
    else:  # real basis: two fp64 sums of d products
        zf = z.astype(np.float64)
        assert (np.abs(v - zf @ s["B"].T) <= 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(zf) @ np.abs(s["B"]).T)).all()


@pytest.mark.parametrize("kind,d", GENERAL)
def test_general_frames_decide_outside_the_error_bound(kind, d):
    s = _general_case(kind, d)
    ctx = _context(s["R"], s["B"], s["Q"], s["Binv"])
    for method in ("plane", "round"):
        z, v = ctx.decode_host(s["T"], method)
        _check_general(s, method, z, v, label=kind)


@pytest.mark.parametrize("d", [17, 33])
def test_general_frames_batch_sizes_at_tile_and_block_edges(d):
    s = _general_case("gauss", d)
    ctx = _context(s["R"], s["B"], s["Q"], s["Binv"])
    for n in (1, 63, 64, 65, 255, 256, 257):
        for method in ("plane", "round"):
            z, v = ctx.decode_host(s["T"][:n], method)
            assert z.shape == (n, d) and v.shape == (n, d)
            _check_general(s, method, z, v, n=n, label="gauss")


@pytest.mark.parametrize("panel", [32, 16])
@pytest.mark.parametrize("d", [17, 65])
def test_decode_buffer_layouts(d, panel):
    """Every way run_decode reads targets and writes z / v gives the host int64 result."""
    import torch
    from lgs_amd import _capi
    Z64, CM, DEV = _capi.LGS_Z64, _capi.LGS_COORD_MAJOR, _capi.LGS_DEVICE_PTRS
    s = _general_case("gauss", d)
    T = s["T"]
    ctx = _context(s["R"], s["B"], s["Q"], s["Binv"], panel=panel)
    Td = torch.as_tensor(T, device="cuda")
    Tc = torch.as_tensor(np.ascontiguousarray(T.T), device="cuda")

    def dev(shape, dtype):  # poisoned: an element the call leaves unwritten shows
        return torch.full(shape, -77, dtype=dtype, device="cuda")

    for method in ("plane", "round") if panel == 32 else ("plane",):
        zr, vr = np.empty((N, d), dtype=np.int64), np.empty((N, d))
        ctx.decode(T, method, zr, vr, Z64)
        _check_general(s, method, zr, vr, label=f"panel={panel}")
        # host int32 row-major
        z, v = np.full((N, d), -77, dtype=np.int32), np.full((N, d), -77.0)
        ctx.decode(T, method, z, v, 0)
        np.testing.assert_array_equal(z, zr)
        np.testing.assert_array_equal(v, vr)
        # host, z_out = NULL and v_out = NULL
        v = np.full((N, d), -77.0)
        ctx.decode(T, method, None, v, 0)
        np.testing.assert_array_equal(v, vr)
        z = np.full((N, d), -77, dtype=np.int64)
        ctx.decode(T, method, z, None, Z64)
        np.testing.assert_array_equal(z, zr)
        # device: int32 row-major, int32 and int64 coordinate-major
        for zt, cm in ((torch.int32, False), (torch.int32, True), (torch.int64, True)):
            f = DEV | (CM if cm else 0) | (Z64 if zt == torch.int64 else 0)
            z, v = dev((d, N) if cm else (N, d), zt), dev((N, d), torch.float64)
            ctx.decode(Tc if cm else Td, method, z, v, f)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(z.cpu().numpy().T if cm else z.cpu().numpy(), zr)
            np.testing.assert_array_equal(v.cpu().numpy(), vr)
        # device, z_out = NULL (v only) and v_out = NULL
        v = dev((N, d), torch.float64)
        ctx.decode(Tc, method, None, v, DEV | CM)
        z = dev((N, d), torch.int32)
        ctx.decode(Td, method, z, None, DEV)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(v.cpu().numpy(), vr)
        np.testing.assert_array_equal(z.cpu().numpy(), zr)


# ---------------------------------------------------------------- the chunk loop
def test_decode_chunk_loop_matches_one_chunk(monkeypatch):
    """run_decode's chunk is max(256, 2^27 / d) targets, so its second chunk needs 1 GiB of
    them; the hooks build's LGS_TEST_DECODE_CHUNK=100 cuts 321 targets into 100/100/100/21
    and every per-chunk offset (targets, z, v; host and device; both layouts) is used.
    Reference: one unchunked call of the product library."""
    import torch
    from lgs_amd import _capi
    Z64, CM, DEV = _capi.LGS_Z64, _capi.LGS_COORD_MAJOR, _capi.LGS_DEVICE_PTRS
    d = 17
    s = _general_case("gauss", d)
    T = s["T"]
    Tt = np.ascontiguousarray(T.T)
    prod = _context(s["R"], s["B"], s["Q"], s["Binv"])
    want = {}
    for method in ("plane", "round"):
        zr, vr = np.empty((N, d), dtype=np.int64), np.empty((N, d))
        prod.decode(T, method, zr, vr, Z64)
        want[method] = (zr, vr)
    hk = _context(s["R"], s["B"], s["Q"], s["Binv"], hooks=True)
    monkeypatch.setenv("LGS_TEST_DECODE_CHUNK", "100")
    for method in ("plane", "round"):
        zr, vr = want[method]
        # host row-major int32, host coordinate-major int64
        z, v = np.full((N, d), -77, dtype=np.int32), np.full((N, d), -77.0)
        hk.decode(T, method, z, v, 0)
        np.testing.assert_array_equal(z, zr)
        np.testing.assert_array_equal(v, vr)
        z, v = np.full((d, N), -77, dtype=np.int64), np.full((N, d), -77.0)
        hk.decode(Tt, method, z, v, CM | Z64)
        np.testing.assert_array_equal(z.T, zr)
        np.testing.assert_array_equal(v, vr)
        # device row-major int64, device coordinate-major int32
        z = torch.full((N, d), -77, dtype=torch.int64, device="cuda")
        v = torch.full((N, d), -77.0, dtype=torch.float64, device="cuda")
        hk.decode(torch.as_tensor(T, device="cuda"), method, z, v, DEV | Z64)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(z.cpu().numpy(), zr)
        np.testing.assert_array_equal(v.cpu().numpy(), vr)
        z = torch.full((d, N), -77, dtype=torch.int32, device="cuda")
        v = torch.full((N, d), -77.0, dtype=torch.float64, device="cuda")
        hk.decode(torch.as_tensor(Tt, device="cuda"), method, z, v, DEV | CM)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(z.cpu().numpy().T, zr)
        np.testing.assert_array_equal(v.cpu().numpy(), vr)
    # the product library has no such switch: the variable changes nothing there
    zr, vr = want["plane"]
    z, v = prod.decode_host(T, "plane")
    np.testing.assert_array_equal(z, zr)
    np.testing.assert_array_equal(v, vr)


# ---------------------------------------------------------------- non-finite targets
def test_one_non_finite_target_in_a_batch():
    """A NaN or an infinity in one target, at the ends of the two 256-lane blocks, fails the
    call with LGS_ERR_NONFINITE; the context is usable afterwards."""
    from lgs_amd import _capi
    s = _general_case("gauss", 17)
    ctx = _context(s["R"], s["B"], s["Q"], s["Binv"])
    fresh = _context(s["R"], s["B"], s["Q"], s["Binv"])
    bads = (np.nan, np.inf, -np.inf)
    for a, row in enumerate((0, 255, 256, 320)):
        for method in ("plane", "round"):
            T = s["T"].copy()
            T[row, (5 * a + 3) % 17] = bads[a % 3]
            with pytest.raises(_capi.LgsError) as err:
                ctx.decode_host(T, method)
            assert err.value.code == _capi.LGS_ERR_NONFINITE
    for method in ("plane", "round"):
        z, v = ctx.decode_host(s["T"], method)
        zf, vf = fresh.decode_host(s["T"], method)
        np.testing.assert_array_equal(z, zf)
        np.testing.assert_array_equal(v, vf)
        _check_general(s, method, z, v, label="after non-finite")


# ---------------------------------------------------------------- lgs_set_basis discards the decoding frame
def _frame(B):
    Q, R = DO.qr_frame(B)
    return np.ascontiguousarray(R), np.ascontiguousarray(Q), np.linalg.inv(B)


def _set_basis_discards_decoder(B1, B2):
    from lgs_amd import _capi
    SIGMA, SEED, K = 4.0, 11, 4
    R1, Q1, Bi1 = _frame(B1)
    R2, Q2, Bi2 = _frame(B2)
    d1, d2 = B1.shape[0], B2.shape[0]
    rng = np.random.default_rng(7600 + d2)
    T = 50.0 * rng.standard_normal((33, d2))
    ctx = _capi.Context(0)
    ctx.set_basis(R1, np.zeros(d1), B1, SIGMA)
    ctx.set_decoder(Q1, Bi1)
    ctx.decode_host(50.0 * rng.standard_normal((5, d1)), "plane")  # the first frame is in use
    ctx.set_basis(R2, np.zeros(d2), B2, SIGMA)
    stale = (lambda: ctx.decode_host(T, "plane"), lambda: ctx.decode_host(T, "round"),
             lambda: ctx.klein_targets_host(SEED, 0, T), lambda: ctx.klein_decode_host(SEED, 0, T, K))
    for call in stale:  # the frame of the first basis must not be read: not its size, not its values
        with pytest.raises(_capi.LgsError) as err:
            call()
        assert err.value.code == _capi.LGS_ERR_STATE
    fresh = _capi.Context(0)
    fresh.set_basis(R2, np.zeros(d2), B2, SIGMA)
    fresh.set_decoder(Q2, Bi2)
    # targets already in the Q frame need no decoding frame
    CP = T @ Q2
    a = ctx.klein_targets_host(SEED, 0, CP, want_cprime=True, flags=_capi.LGS_TARGETS_QFRAME)
    b = fresh.klein_targets_host(SEED, 0, CP, want_cprime=True, flags=_capi.LGS_TARGETS_QFRAME)
    for key in ("z", "v", "cprime"):
        np.testing.assert_array_equal(a[key], b[key])
    ctx.set_decoder(Q2, None)
    with pytest.raises(_capi.LgsError) as err:  # Q came back, B^-1 did not
        ctx.decode_host(T, "round")
    assert err.value.code == _capi.LGS_ERR_STATE
    ctx.set_decoder(None, Bi2)
    for method in ("plane", "round"):
        z, v = ctx.decode_host(T, method)
        zf, vf = fresh.decode_host(T, method)
        np.testing.assert_array_equal(z, zf)
        np.testing.assert_array_equal(v, vf)
    a, b = ctx.klein_targets_host(SEED, 0, T, want_cprime=True), fresh.klein_targets_host(SEED, 0, T, want_cprime=True)
    for key in ("z", "v", "cprime"):
        np.testing.assert_array_equal(a[key], b[key])
    a, b = ctx.klein_decode_host(SEED, 0, T, K), fresh.klein_decode_host(SEED, 0, T, K)
    for key in ("z", "v", "best_draw", "dist2"):
        np.testing.assert_array_equal(a[key], b[key])


def test_set_basis_discards_decoder_same_d():
    """A second basis of the same d: without the discard the decoders silently work in the
    first basis's frame."""
    from lgs_amd import lattices
    B1, B2 = lattices.qary_basis(8, 8, 17, 1), lattices.qary_basis(8, 8, 17, 2)
    assert B1.shape == B2.shape and not np.array_equal(B1, B2)
    _set_basis_discards_decoder(B1, B2)


def test_set_basis_discards_decoder_grown_d():
    """d grows from 8 to 64: without the discard the frame GEMM reads 32 KiB of a 512-byte
    Q.  Every stale call must fail before any launch."""
    from lgs_amd import lattices
    B1, B2 = lattices.qary_basis(4, 4, 17, 1), lattices.qary_basis(32, 32, 17, 2)
    assert B1.shape == (8, 8) and B2.shape == (64, 64)
    _set_basis_discards_decoder(B1, B2)
