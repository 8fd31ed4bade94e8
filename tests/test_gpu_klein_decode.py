"""Decoding by sampling (lgs_klein_decode, KleinSampler.decode_around,
Decoder.sampling_decode): the closest of K Klein draws per target.

Oracle.  The z of all n K draws come from klein_targets_host(LGS_TARGETS_QFRAME |
LGS_EXACT_ORDER) on the call's own cprime repeated K times (that path is checked
against the CPU oracle in test_gpu_targets.py); on the bases with d <= 40 every 5th
draw is also taken from the CPU oracle.  The reference-order distance D is restated in
NumPy (two Python loops over i and j, vectorised over draws; NumPy does not fuse), the
expected winner is argmin D with the first index on ties, and z, best_draw and dist2
are compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 4242
CASES = ((1, 1, 0), (5, 3, 7), (4, 64, 1000), (9, 100, 77), (64, 16, 5))  # (n, K, first)


def _qr(B):
    Q, R = np.linalg.qr(np.asarray(B, dtype=np.float64), mode="full")
    for i in range(R.shape[0]):
        if R[i, i] < 0:
            R[i, :] *= -1
            Q[:, i] *= -1
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


def _bases():
    from lgs_amd import lattices
    rng = np.random.default_rng(12)
    g37 = rng.standard_normal((37, 37)) * 6.0 + 25.0 * np.eye(37)
    i12 = np.rint(rng.standard_normal((12, 12)) * 4.0) + 40.0 * np.eye(12)
    return {
        "qary40": (lattices.qary_basis(20, 20, 3329, 5), 165.7, True),
        "ntru64": (lattices.ntru_basis(32, 12289, 2), 165.7, True),
        "qary128": (lattices.qary_basis(64, 64, 3329, 1), 165.7, True),
        "gauss37": (g37, 30.0, False),
        "d2": (np.array([[4.0, 1.0], [1.0, 3.0]]), 3.0, True),
        "int12": (i12, 45.0, True),
    }


BASES = ("qary40", "ntru64", "qary128", "gauss37", "d2", "int12")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


def _setup(B, sigma, integral, n_targets=64):
    Q, R = _qr(B)
    d = B.shape[0]
    T = np.random.default_rng(1000 + d).standard_normal((n_targets, d)) * 2500.0
    for a in (B, Q, R, T):
        a.setflags(write=False)
    return dict(B=B, sigma=sigma, integral=integral, Q=Q, R=R, T=T, d=d)


@pytest.fixture(scope="module")
def setups():
    """Per basis: B, sigma, Q, R and 64 targets = 2500 N(0, 1) (shared, read-only)."""
    return {name: _setup(*v) for name, v in _bases().items()}


def _context(capi, s, sigma=None, **kw):
    ctx = capi.Context(0, **kw)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], s["sigma"] if sigma is None else sigma)
    ctx.set_decoder(Q=s["Q"])
    return ctx


def ref_dist(R, cprime, z):
    """The reference-order squared distance of each draw (rows of z, centres rows of
    cprime), exactly as lgs.h defines it: unfused fp64, i descending, j ascending."""
    d = R.shape[0]
    zf = z.astype(np.float64)
    D = np.zeros(zf.shape[0])
    for i in range(d - 1, -1, -1):
        cs = np.zeros(zf.shape[0])
        for j in range(i + 1, d):
            cs = cs + R[i, j] * zf[:, j]
        r = (cprime[:, i] - cs) - R[i, i] * zf[:, i]
        D = D + r * r
    return D


def all_draws(capi, ctx, s, cprime, K, first, oracle=None, sigma=None):
    """(z, D) of all n K draws, shaped (n, K, d) and (n, K): the exact-order
    per-target path on cprime repeated K times; every 5th draw also from the CPU
    oracle when one is given and d <= 40."""
    n, d = cprime.shape
    rep = np.repeat(cprime, K, axis=0)
    z = ctx.klein_targets_host(SEED, first, rep, want_v=False,
                               flags=capi.LGS_TARGETS_QFRAME | capi.LGS_EXACT_ORDER)["z"]
    if oracle is not None and d <= 40:
        sg = s["sigma"] if sigma is None else sigma
        for p in range(0, n * K, 5):
            want = oracle.klein(s["R"], rep[p], sg, 1, seed=SEED, first_sample=first + p)["z"][0]
            assert np.array_equal(z[p], want), f"draw {p} differs from the CPU oracle"
    return z.reshape(n, K, d), ref_dist(s["R"], rep, z).reshape(n, K)


def check_winners(s, r, zall, Dall):
    """z, best_draw and dist2 bit for bit; v as test_gpu_targets.py checks it."""
    n, d = r["z"].shape
    want = np.argmin(Dall, axis=1)  # the first index on ties
    assert np.array_equal(r["best_draw"], want), (r["best_draw"], want)
    assert np.array_equal(r["dist2"], Dall[np.arange(n), want])
    assert np.array_equal(r["z"], zall[np.arange(n), want])
    if r.get("v") is not None:
        zf = r["z"].astype(np.float64)
        if s["integral"]:
            assert np.array_equal(r["v"], zf @ s["B"].T)
        else:  # real basis: two fp64 sums of d products
            assert (np.abs(r["v"] - zf @ s["B"].T)
                    <= 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(zf) @ np.abs(s["B"]).T)).all()


@pytest.fixture(scope="module")
def runs(capi, oracle, setups):
    """The runs of cases 1 and 2, made once per (basis, mode): per (n, K, first) the
    call's result with the per-draw arrays, and the oracle's z and D of every draw."""
    memo = {}

    def get(name, exact):
        if (name, exact) not in memo:
            s = setups[name]
            ctx = _context(capi, s)
            out = []
            for n, K, first in CASES:
                r = ctx.klein_decode_host(SEED, first, s["T"][:n], K, want_cprime=True, want_draws=True,
                                          flags=capi.LGS_EXACT_ORDER if exact else 0)
                zall, Dall = all_draws(capi, ctx, s, r["cprime"], K, first, oracle)
                out.append((n, K, first, r, zall, Dall))
            memo[name, exact] = out
        return memo[name, exact]
    return get


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", BASES)
def test_oracle_parity(setups, runs, name, exact):
    s = setups[name]
    for n, K, first, r, zall, Dall in runs(name, exact):
        d = s["d"]
        ref = s["T"][:n] @ s["Q"]  # c' = Q^T t, as test_gpu_targets.py bounds it
        assert (np.abs(r["cprime"] - ref)
                <= 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(s["T"][:n]) @ np.abs(s["Q"]))).all()
        check_winners(s, r, zall, Dall)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", BASES)
def test_bound_is_sound(runs, name, exact):
    worst = 0.0
    for n, K, first, r, zall, Dall in runs(name, exact):
        Dt, E = r["dist2_draws"], r["bound_draws"]
        assert Dt.shape == (n, K) and E.shape == (n, K)
        if exact:
            assert np.array_equal(Dt, Dall) and not E.any()
        else:
            assert (E >= 0).all() and np.isfinite(E).all()
            assert (np.abs(Dt - Dall) <= E).all()
            worst = max(worst, float((np.abs(Dt - Dall) / E).max()))
            print(f"  {name} n={n} K={K}: max E/D = {float((E / Dall).max()):.3e}, "
                  f"max |D~ - D| / E = {float((np.abs(Dt - Dall) / E).max()):.3e}")


def test_exact_ties_first_index_wins(capi, oracle):
    """B = 2 I_8, every target (1, ..., 1): all arithmetic is exact and every draw in
    {0, 1}^8 is at D = 8, so distinct z tie exactly; the first tied draw wins."""
    s = _setup(2.0 * np.eye(8), 1.6, True)
    T = np.ones((32, 8))
    ctx = _context(capi, s)
    res = {}
    for exact in (False, True):
        ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED, reset=True)
        r = ctx.klein_decode_host(SEED, 0, T, 16, want_cprime=True,
                                  flags=capi.LGS_EXACT_ORDER if exact else 0)
        res[exact] = (r, ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED))
    r = res[False][0]
    zall, Dall = all_draws(capi, ctx, s, r["cprime"], 16, 0, oracle)
    tied = (Dall == Dall.min(axis=1, keepdims=True)).sum(axis=1)
    distinct = [len({tuple(z) for z, D in zip(zall[t], Dall[t]) if D == Dall[t].min()}) for t in range(32)]
    print(f"  targets with tied minima: {(tied > 1).sum()} of 32, up to {tied.max()} draws, "
          f"winners {sorted(set(r['best_draw']))}, resolved {res[False][1]}")
    assert (tied > 1).sum() >= 16 and max(distinct) > 1
    for exact in (False, True):
        check_winners(s, res[exact][0], zall, Dall)
    assert res[False][1] > 0


def test_near_ties_that_rounding_separates(capi, oracle, setups):
    """Targets half way between two lattice points along b_0: draws with z_0 = z0_0 and
    z0_0 + 1 are at distances that agree to rounding; the default path must fall back
    to the reference order and agree with the exact path and NumPy bit for bit."""
    s = setups["int12"]
    sigma = 0.25 * np.diag(s["R"]).min()
    n, K = 64, 32
    T = np.empty((n, 12))
    for k in range(n):
        z0 = np.random.default_rng(500 + k).integers(-50, 50, 12).astype(np.float64)
        z0[0] += 0.5
        T[k] = s["B"] @ z0
    ctx = _context(capi, s, sigma=sigma)
    ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED, reset=True)
    a = ctx.klein_decode_host(SEED, 0, T, K, want_cprime=True)
    grew = ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED)
    b = ctx.klein_decode_host(SEED, 0, T, K, want_cprime=True, flags=capi.LGS_EXACT_ORDER)
    zall, Dall = all_draws(capi, ctx, s, a["cprime"], K, 0, oracle, sigma=sigma)
    Dmin = Dall.min(axis=1, keepdims=True)
    near = [len({tuple(z) for z, D in zip(zall[t], Dall[t]) if D <= Dmin[t] * (1 + 1e-9)}) for t in range(n)]
    print(f"  targets with >= 2 distinct z within 1e-9 of the minimum: {sum(c > 1 for c in near)} of {n}; "
          f"resolved in the reference order: {grew}")
    assert np.array_equal(a["cprime"], b["cprime"])
    check_winners(s, a, zall, Dall)
    check_winners(s, b, zall, Dall)
    assert grew >= 32


def test_random_targets_are_certified(capi, setups):
    """Random targets: the gap between the best and the second-best draw (4e-4 relative
    at the least on these inputs) is far above the bound (about 1e-10 relative), so the
    intervals decide every target."""
    s = setups["gauss37"]
    ctx = _context(capi, s)
    ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED, reset=True)
    r = ctx.klein_decode_host(SEED, 0, s["T"][:40], 16, want_cprime=True, want_draws=True)
    resolved = ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED)
    zall, Dall = all_draws(capi, ctx, s, r["cprime"], 16, 0)
    srt = np.sort(Dall, axis=1)
    print(f"  max E/D = {float((r['bound_draws'] / Dall).max()):.3e}, smallest relative gap "
          f"{float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min()):.3e}, resolved {resolved} of 40")
    check_winners(s, r, zall, Dall)
    assert resolved <= 0.01 * 40


def test_forced_fallback(capi, setups, monkeypatch):
    """The hooks library widens every certificate bound, and with it every distance
    bound, by 1 / LGS_TEST_Z1CAP_SCALE (each stays a bound): decisions and selections
    go through their reference-order paths and the outputs must not change."""
    s = setups["qary128"]
    T = s["T"][:32]
    want = _context(capi, s).klein_decode_host(SEED, 3, T, 16, want_draws=True, flags=capi.LGS_EXACT_ORDER)
    monkeypatch.setenv("LGS_TEST_Z1CAP_SCALE", "1e-9")
    ctx = _context(capi, s, hooks=True)
    ctx.resolved(reset=True)
    ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED, reset=True)
    got = ctx.klein_decode_host(SEED, 3, T, 16, want_draws=True)
    redone, sel = ctx.resolved(), ctx.counter(capi.LGS_COUNTER_DECODE_RESOLVED)
    print(f"  {redone} decisions and {sel} of 32 selections redone in the reference order")
    for k in ("z", "v", "best_draw", "dist2"):
        assert np.array_equal(got[k], want[k]), k
    assert (np.abs(got["dist2_draws"] - want["dist2_draws"]) <= got["bound_draws"]).all()
    assert redone > 0 and sel > 0


def test_select_without_lds_staging(capi, setups, monkeypatch):
    """The select kernel's path of d > 8192 (the draw's coefficients read from the store
    instead of the wave's LDS row), taken through the hooks library: same results, with
    one candidate (random targets) and with several (exact ties)."""
    ties = _setup(2.0 * np.eye(8), 1.6, True)
    jobs = ((setups["qary128"], setups["qary128"]["T"][:9], 20), (ties, np.ones((32, 8)), 16))
    want = [_context(capi, s).klein_decode_host(SEED, 2, T, K) for s, T, K in jobs]
    monkeypatch.setenv("LGS_TEST_DECODE_NOSTAGE", "1")
    for (s, T, K), w in zip(jobs, want):
        got = _context(capi, s, hooks=True).klein_decode_host(SEED, 2, T, K)
        for k in ("z", "v", "best_draw", "dist2"):
            assert np.array_equal(got[k], w[k]), k


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_batch_invariance(capi, setups, exact):
    """max_proposals = 256, K = 48: 5 targets per chunk (240 lanes padded to 256), n = 13
    in three chunks; equal to one chunk, and to two calls split at target 6."""
    s = setups["qary40"]
    f = capi.LGS_EXACT_ORDER if exact else 0
    T, K = s["T"][:13], 48
    keys = ("z", "v", "cprime", "best_draw", "dist2", "dist2_draws", "bound_draws")
    small = _context(capi, s, max_proposals=256)
    r = small.klein_decode_host(SEED, 11, T, K, want_cprime=True, want_draws=True, flags=f)
    one = _context(capi, s).klein_decode_host(SEED, 11, T, K, want_cprime=True, want_draws=True, flags=f)
    for k in keys:
        assert np.array_equal(r[k], one[k]), k
    a = small.klein_decode_host(SEED, 11, T[:6], K, want_cprime=True, want_draws=True, flags=f)
    b = small.klein_decode_host(SEED, 11 + 6 * K, T[6:], K, want_cprime=True, want_draws=True, flags=f)
    for k in keys:
        assert np.array_equal(r[k], np.concatenate([a[k], b[k]])), k


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", ["qary40", "gauss37", "qary128"])
def test_one_draw_is_klein_targets(capi, setups, name, exact):
    s = setups[name]
    f = capi.LGS_EXACT_ORDER if exact else 0
    ctx = _context(capi, s)
    T = s["T"][:50]
    want = ctx.klein_targets_host(SEED, 9, T, want_cprime=True, flags=f)
    got = ctx.klein_decode_host(SEED, 9, T, 1, want_cprime=True, flags=f)
    for k in ("z", "v", "cprime"):
        assert np.array_equal(got[k], want[k]), k
    assert not got["best_draw"].any()


def test_device_pointers_coordinate_major_and_qframe(capi, setups):
    import torch
    s = setups["qary40"]
    n, K, d = 21, 12, s["d"]
    T = s["T"][:n]
    ctx = _context(capi, s)
    host = ctx.klein_decode_host(SEED, 21, T, K, want_cprime=True, want_draws=True)
    z64 = ctx.klein_decode_host(SEED, 21, T, K, flags=capi.LGS_Z64)
    for k in ("z", "v", "best_draw", "dist2"):
        assert np.array_equal(z64[k], host[k]), k
    f = capi.LGS_DEVICE_PTRS | capi.LGS_COORD_MAJOR
    dev = dict(device="cuda")
    t = torch.as_tensor(np.ascontiguousarray(T.T), **dev)
    z = torch.empty((d, n), dtype=torch.int32, **dev)
    v = torch.empty((n, d), dtype=torch.float64, **dev)
    cp = torch.empty((n, d), dtype=torch.float64, **dev)
    best = torch.empty(n, dtype=torch.int64, **dev)
    d2 = torch.empty(n, dtype=torch.float64, **dev)
    dd = torch.empty((n, K), dtype=torch.float64, **dev)
    bd = torch.empty((n, K), dtype=torch.float64, **dev)
    ctx.klein_decode(SEED, 21, t, K, z, v, cp, best, d2, dd, bd, f)
    torch.cuda.synchronize()
    for got, k in ((z.T, "z"), (v, "v"), (cp, "cprime"), (best, "best_draw"), (d2, "dist2"),
                   (dd, "dist2_draws"), (bd, "bound_draws")):
        assert np.array_equal(got.cpu().numpy(), host[k]), k
    # the Q frame, coordinate-major on the device and row-major on the host: c' verbatim
    zq = torch.empty((d, n), dtype=torch.int64, **dev)
    ctx.klein_decode(SEED, 21, cp.T.contiguous(), K, zq, None, None, best, None, None, None,
                     f | capi.LGS_TARGETS_QFRAME | capi.LGS_Z64)
    torch.cuda.synchronize()
    assert np.array_equal(zq.T.cpu().numpy(), host["z"])
    q = ctx.klein_decode_host(SEED, 21, host["cprime"], K, want_cprime=True, flags=capi.LGS_TARGETS_QFRAME)
    assert np.array_equal(q["cprime"], host["cprime"]) and np.array_equal(q["z"], host["z"])
    assert np.array_equal(q["dist2"], host["dist2"])
    # row-major device buffers
    zr = torch.empty((n, d), dtype=torch.int32, **dev)
    ctx.klein_decode(SEED, 21, torch.as_tensor(np.array(T), **dev), K, zr, flags=capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    assert np.array_equal(zr.cpu().numpy(), host["z"])


def test_large_coefficients_and_overflow(capi, setups):
    import torch
    s = setups["int12"]
    d, n, K = s["d"], 24, 8
    ctx = _context(capi, s)
    T = s["T"][:n] * 4000.0  # |t| ~ 1e7: |z| beyond the 16-bit range
    for exact in (False, True):
        r = ctx.klein_decode_host(SEED, 3, T, K, want_cprime=True, flags=capi.LGS_EXACT_ORDER if exact else 0)
        assert np.abs(r["z"]).max() > 32767
        zall, Dall = all_draws(capi, ctx, s, r["cprime"], K, 3)
        check_winners(s, r, zall, Dall)
    z = torch.empty((d, n), dtype=torch.int32, device="cuda")
    best = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.klein_decode(SEED, 3, torch.as_tensor(np.ascontiguousarray(T.T), device="cuda"), K, z, best_draw=best,
                     flags=capi.LGS_DEVICE_PTRS | capi.LGS_COORD_MAJOR)
    torch.cuda.synchronize()
    assert np.array_equal(best.cpu().numpy(), r["best_draw"]) and np.array_equal(z.T.cpu().numpy(), r["z"])
    # |z| >= 2^31: int32 buffers overflow, int64 succeed
    T = s["T"][:10] * 1e9
    z32 = np.empty((10, d), dtype=np.int32)
    for f in (0, capi.LGS_EXACT_ORDER):
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_decode(SEED, 0, T, K, z32, flags=f)
        assert e.value.code == capi.LGS_ERR_OVERFLOW
    r = ctx.klein_decode_host(SEED, 0, T, K, want_cprime=True)  # reruns with LGS_Z64
    assert np.abs(r["z"]).max() >= 2 ** 31
    zall, Dall = all_draws(capi, ctx, s, r["cprime"], K, 0)
    check_winners(s, r, zall, Dall)


def test_errors(capi, setups):
    s = setups["qary40"]
    d = s["d"]
    T = np.array(s["T"][:10])
    ctx = capi.Context(0, max_proposals=512)
    ctx.set_basis(s["R"], np.zeros(d), None, s["sigma"])  # no B
    z = np.empty((10, d), dtype=np.int32)
    with pytest.raises(capi.LgsError) as e:  # no Q uploaded, targets in the lattice frame
        ctx.klein_decode(SEED, 0, T, 4, z)
    assert e.value.code == capi.LGS_ERR_STATE
    ctx.klein_decode(SEED, 0, T, 4, z, flags=capi.LGS_TARGETS_QFRAME)  # needs no Q; null out accepted
    with pytest.raises(capi.LgsError) as e:  # v_out without B
        ctx.klein_decode(SEED, 0, T, 4, z, np.empty((10, d)), flags=capi.LGS_TARGETS_QFRAME)
    assert e.value.code == capi.LGS_ERR_STATE
    ctx.set_decoder(Q=s["Q"])
    ctx.klein_decode(SEED, 0, T[:0], 4)  # n == 0
    for K in (0, -3, 513):
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_decode(SEED, 0, T, K, z)
        assert e.value.code == capi.LGS_ERR_INVALID
    ctx.klein_decode(SEED, 0, T[:1], 512, z[:1])  # all of max_proposals on one target
    for f in (capi.LGS_WANG_LING, capi.LGS_LOGW_BOUND, capi.LGS_SAMPLEZ_TABLE):
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_decode(SEED, 0, T, 4, z, flags=f)
        assert e.value.code == capi.LGS_ERR_INVALID
    for f in (0, capi.LGS_EXACT_ORDER, capi.LGS_TARGETS_QFRAME):
        bad = T.copy()
        bad[4, 7] = np.nan
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_decode(SEED, 0, bad, 4, z, flags=f)
        assert e.value.code == capi.LGS_ERR_NONFINITE
    ctx.klein_decode(SEED, 0, T, 4, z)  # the context is usable after an error


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_sampler_decode_around(setups, exact):
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import KleinSampler
    s = setups["qary40"]
    lat = SimpleLattice(s["B"])
    T, K = s["T"][:17], 6
    smp = KleinSampler(lat, s["sigma"], seed=11, exact_order=exact)
    smp.sample(3)  # counters 0..2
    pts, z = smp.decode_around(T, K, coefficients=True)
    assert pts.shape == (17, s["d"]) and z.shape == (17, s["d"]) and smp._next_sample == 3 + 17 * K
    twin = KleinSampler(lat, s["sigma"], seed=11, exact_order=exact)
    twin.sample(3)
    cand = twin.sample_around(np.repeat(T, K, axis=0)).reshape(17, K, -1)  # the same 17 K draws
    dist = np.linalg.norm(cand - T[:, None, :], axis=2)
    for t in range(17):
        hit = [k for k in range(K) if np.array_equal(cand[t, k], pts[t])]
        assert hit, f"target {t}: the point is none of its {K} draws"
        assert dist[t, hit[0]] <= dist[t].min() * (1 + 1e-12)
    assert np.array_equal(pts, z.astype(np.float64) @ s["B"].T)
    one = smp.decode_around(T[0], 4)
    assert one.shape == (s["d"],) and smp._next_sample == 3 + 17 * K + 4
    assert np.array_equal(smp.sample(2), twin.sample(6)[4:])


def test_decoder_sampling_decode(setups):
    from lgs_amd.decode import Decoder
    s = setups["qary40"]
    dec = Decoder(s["B"])
    zt = np.random.default_rng(5).integers(-40, 40, (9, s["d"])).astype(np.float64)
    T = zt @ s["B"].T + np.random.default_rng(6).standard_normal((9, s["d"])) * 0.05
    want = dec.nearest_plane(T, coefficients=True)
    assert np.array_equal(want, zt)
    sigma = 0.2 * np.diag(s["R"]).min()
    z = dec.sampling_decode(T, 8, sigma, seed=3, coefficients=True)
    v = dec.sampling_decode(T, 8, sigma, seed=3)
    assert z.shape == (9, s["d"]) and np.array_equal(v, z.astype(np.float64) @ s["B"].T)
    assert np.array_equal(dec.sampling_decode(T[0], 8, sigma, seed=3), v[0])
    # a narrow sampler around a target 0.05 from a lattice point finds that point
    assert np.array_equal(z, zt)
    assert np.array_equal(dec.nearest_plane(T, coefficients=True), want)  # still works after the reload
    assert np.array_equal(dec.round_decode(T, coefficients=True), want)
