"""The exact sampler (lgs_exact_table, lgs_exact_sample, ExactSampler) against its operational
definition: the weights within 4 * 2^-53 relative of np.exp (both exps are within 1 ulp, the
argument is identical), cum and mass equal to the blocked running sum of the RETURNED weights
bit for bit, every draw equal to the inverse CDF at the Philox uniform of tag 2, bit for bit."""
import math

import numpy as np
import pytest

import ball_oracle
import cvp_oracle

pytestmark = pytest.mark.gpu

MAX_NODES = 1 << 22
NATS = 12.0


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def setups():
    return {name: cvp_oracle.setup(name) for name in ("d2", "int12")}


def _context(capi, s, **kw):
    ctx = capi.Context(0, **kw)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], 1.0)
    ctx.set_decoder(Q=s["Q"])
    return ctx


def _radius_for(s, t, counts, extra):
    """Squared radii (one per entry of counts) whose balls around t hold exactly counts[k]
    points, and D_min: from the CPU oracle's list of the ball of squared radius D_min + extra."""
    cp = t @ s["Q"]
    _, Dmin, _, st0 = cvp_oracle.se(s["R"], cp)
    _, D, _, st = ball_oracle.points(s["R"], cp, Dmin + extra)
    assert st0 == 0
    D = np.sort(D)
    assert st == 0 and len(D) > max(counts) and len(np.unique(D[:max(counts) + 1])) >= 2
    out = []
    for N in counts:
        assert D[N - 1] < D[N]
        out.append(0.5 * (D[N - 1] + D[N]))
    return out, D[0]


_TABLES = {}


def _table(capi, s, key):
    """A context holding a table of the named layout, with its host record (shared, read-only).
    The targets are passed as c' = t Q in the QR frame (LGS_TARGETS_QFRAME), so that the library
    and the CPU oracle, which chooses the radii, work on the same bits."""
    if key in _TABLES:
        return _TABLES[key]
    QF = capi.LGS_TARGETS_QFRAME
    if key == "sizes":  # int12: 1, 300, 777 points and a natural ball; sigma 12
        sigma = 12.0
        (r1, r300), d0 = _radius_for(s, s["T"][0], (1, 300), 2.0 * 144.0 * NATS)
        (r777,), d1 = _radius_for(s, s["T"][1], (777,), 2.0 * 144.0 * NATS)
        T = np.stack([s["T"][k] @ s["Q"] for k in (0, 0, 1, 2)])  # (row by row, as the oracle forms c')
        cv = _context(capi, s).closest_vector_host(T, 1 << 20, want_z=False, want_v=False, flags=QF)
        assert cv["dist2"][0] == d0 and cv["dist2"][2] == d1
        r2 = np.array([r1, r300, r777, cv["dist2"][3] + 2.0 * sigma * sigma * NATS])
        shift = cv["dist2"].copy()
    elif key == "d2":  # d2: 16 points and 1; sigma 0.8
        sigma = 0.8
        t = np.array([1.7, -0.6])
        (r1, r16), d0 = _radius_for(s, t, (1, 16), 80.0)
        T, r2, shift = np.stack([t @ s["Q"], t @ s["Q"]]), np.array([r16, r1]), np.array([d0, d0])
    else:  # "many": int12, the first 130 targets, 12 nats
        sigma = 12.0
        T = s["T"][:130] @ s["Q"]
        cv = _context(capi, s).closest_vector_host(T, 1 << 20, want_z=False, want_v=False, flags=QF)
        shift = cv["dist2"].copy()
        r2 = shift + 2.0 * sigma * sigma * NATS
    ctx = _context(capi, s)
    T = np.ascontiguousarray(T)
    rows = ctx.ball_points_host(T, r2, MAX_NODES, flags=QF)
    t = ctx.exact_table_host(T, sigma, r2, shift, MAX_NODES, want_weights=True, flags=QF)
    rec = dict(T=T, r2=r2, shift=shift, sigma=sigma, rows=rows, **t)
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _TABLES[key] = (ctx, rec)
    return _TABLES[key]


# ------------------------------------------------------------------ 1. table contents
@pytest.mark.parametrize("key,base,sizes", [("sizes", "int12", (1, 300, 777, None)), ("d2", "d2", (16, 1))])
def test_table_contents(capi, setups, key, base, sizes):
    s = setups[base]
    ctx, t = _table(capi, s, key)
    off, n = t["offsets"], len(sizes)
    assert np.array_equal(off, t["rows"]["offsets"]) and not t["status"].any()
    for k, N in enumerate(sizes):
        got = off[k + 1] - off[k]
        if N is None:
            assert got > 512 and got % 256 != 0
        else:
            assert got == N
        assert got == 1 or got % 256 != 0
        D = t["rows"]["dist2"][off[k]:off[k + 1]]
        W, S = t["weights"][off[k]:off[k + 1]], t["cum"][off[k]:off[k + 1]]
        ref = np.exp((t["shift"][k] - D) / (2.0 * t["sigma"] * t["sigma"]))
        assert (np.abs(W - ref) <= 4.0 * 2.0 ** -53 * ref).all()
        want = ball_oracle.blocked_cumsum_np(W)
        assert np.array_equal(S, want) and np.array_equal(S, ball_oracle.blocked_cumsum(W))
        assert t["mass"][k] == S[-1] and (np.diff(S) >= 0).all()
    assert len(t["weights"]) == off[n]


# ------------------------------------------------------------------ 2. draws
def _expected_index(oracle, t, seed, first, K, n):
    off, S = t["offsets"], t["cum"]
    idx = np.empty(n * K, dtype=np.int64)
    for j in range(n * K):
        k = j // K
        s = (first + j) % (1 << 64)
        u = oracle.philox_u(seed, 0, s >> 32, s & 0xffffffff, 2)
        Sk = S[off[k]:off[k + 1]]
        idx[j] = off[k] + min(int(np.searchsorted(Sk, u * Sk[-1], side="right")), len(Sk) - 1)
    return idx


def _check_draws(s, t, r, idx):
    assert np.array_equal(r["index"], idx)
    assert np.array_equal(r["z"], t["rows"]["z"][idx]) and np.array_equal(r["dist2"], t["rows"]["dist2"][idx])
    assert np.array_equal(r["v"], (r["z"] @ s["B"].T.astype(np.int64)).astype(np.float64))


@pytest.mark.parametrize("key,base,K,first,seed", [("sizes", "int12", 7, (1 << 32) - 3, 11),
                                                   ("sizes", "int12", 64, 0, 12),
                                                   ("many", "int12", 7, (1 << 32) - 3, 13),
                                                   ("d2", "d2", 33, (1 << 64) - 5, 14)])
def test_draws_are_the_inverse_cdf(capi, setups, oracle, key, base, K, first, seed):
    """(n = 130 targets x K = 7: a target's lanes straddle waves, the last wave is padded;
    first = 2^32 - 3 crosses the step counter.)"""
    s = setups[base]
    ctx, t = _table(capi, s, key)
    n = len(t["mass"])
    r = ctx.exact_sample_host(seed, first, K, n)
    _check_draws(s, t, r, _expected_index(oracle, t, seed, first, K, n))
    z64 = ctx.exact_sample_host(seed, first, K, n, flags=capi.LGS_Z64)
    assert all(np.array_equal(r[k], z64[k]) for k in r)


def test_single_centre_split_over_calls_and_device_pointers(capi, setups, oracle):
    import torch
    s = setups["int12"]
    one = _context(capi, s)
    _, big = _table(capi, s, "sizes")
    T, r2, sh = big["T"][3:4], big["r2"][3:4], big["shift"][3:4]
    QF = capi.LGS_TARGETS_QFRAME
    T = np.ascontiguousarray(T)
    t = one.exact_table_host(T, 12.0, r2, sh, MAX_NODES, want_weights=True, flags=QF)
    t["rows"] = one.ball_points_host(T, r2, MAX_NODES, flags=QF)
    one.exact_table(T, 12.0, np.ascontiguousarray(r2), np.ascontiguousarray(sh), MAX_NODES, len(t["weights"]),
                    flags=QF)
    seed, first = 21, (1 << 32) - 400
    whole = one.exact_sample_host(seed, first, 1000, 1)
    _check_draws(s, t, whole, _expected_index(oracle, t, seed, first, 1000, 1))
    a = one.exact_sample_host(seed, first, 600, 1)
    b = one.exact_sample_host(seed, first + 600, 400, 1)
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]]))
    chunked = capi.Context(0, max_proposals=64)  # 16 chunks of draws
    chunked.set_basis(s["R"], np.zeros(s["d"]), s["B"], 1.0)
    chunked.set_decoder(Q=s["Q"])
    chunked.exact_table(T, 12.0, np.ascontiguousarray(r2), np.ascontiguousarray(sh), MAX_NODES, len(t["weights"]),
                        flags=QF)
    c = chunked.exact_sample_host(seed, first, 1000, 1)
    assert all(np.array_equal(whole[k], c[k]) for k in whole)
    dev = dict(device="cuda:0")
    z = torch.full((1000, s["d"]), -7, dtype=torch.int32, **dev)
    v = torch.zeros((1000, s["d"]), dtype=torch.float64, **dev)
    ix = torch.zeros(1000, dtype=torch.int64, **dev)
    d2 = torch.zeros(1000, dtype=torch.float64, **dev)
    one.exact_sample(seed, first, 1000, 1, z, v, ix, d2, capi.LGS_DEVICE_PTRS)
    assert np.array_equal(z.cpu().numpy(), whole["z"]) and np.array_equal(v.cpu().numpy(), whole["v"])
    assert np.array_equal(ix.cpu().numpy(), whole["index"]) and np.array_equal(d2.cpu().numpy(), whole["dist2"])


def test_table_over_several_chunks(capi, setups):
    """lgs_exact_table over three chunks of targets (d2, 130 targets, max_proposals = 64): the
    listing pass writes into the context's table with recomputed centres.  Host and device
    pointers; everything equals the one-chunk table of a default context, byte for byte."""
    import torch
    s = setups["d2"]
    sigma, n = 0.8, 130
    T = np.array(s["T"][:n])  # (a writable copy: it also goes to the device through torch)
    cv = _context(capi, s).closest_vector_host(T, 1 << 20, want_z=False, want_v=False)
    assert not cv["status"].any()
    shift = cv["dist2"].copy()
    r2 = shift + 2.0 * sigma * sigma * NATS
    one = _context(capi, s)
    want = one.exact_table_host(T, sigma, r2, shift, MAX_NODES, want_weights=True)
    total = int(want["offsets"][n])
    assert not want["status"].any() and total >= 2 * n
    seed, first = 31, (1 << 32) - 100
    draws = one.exact_sample_host(seed, first, 3, n)

    def check(ctx, got):
        for k in ("offsets", "nodes", "status", "mass", "weights", "cum"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        r = ctx.exact_sample_host(seed, first, 3, n)
        for k in ("z", "index", "dist2"):
            assert r[k].dtype == draws[k].dtype and r[k].tobytes() == draws[k].tobytes(), k

    host = _context(capi, s, max_proposals=64)
    check(host, host.exact_table_host(T, sigma, r2, shift, MAX_NODES, want_weights=True))
    dev = dict(device="cuda:0")
    out = dict(offsets=torch.full((n + 1,), -1, dtype=torch.int64, **dev),
               nodes=torch.full((n,), -1, dtype=torch.int64, **dev),
               status=torch.full((n,), -1, dtype=torch.int32, **dev),
               mass=torch.zeros(n, dtype=torch.float64, **dev),
               weights=torch.zeros(total, dtype=torch.float64, **dev),
               cum=torch.zeros(total, dtype=torch.float64, **dev))
    device = _context(capi, s, max_proposals=64)
    device.exact_table(torch.as_tensor(T, **dev), sigma, torch.as_tensor(r2, **dev), torch.as_tensor(shift, **dev),
                       MAX_NODES, total, flags=capi.LGS_DEVICE_PTRS, **out)
    check(device, {k: v.cpu().numpy() for k, v in out.items()})


# ------------------------------------------------------------------ 3. statistics
def _d2_exact_pmf(B, sigma, t, half=12):
    """D_{Lambda,sigma,t} over coefficients z in [-half, half]^2, by enumeration (the host box
    sum of tests/test_imhk_targets_host.py)."""
    g = np.arange(-half, half + 1)
    zz = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    r2 = ((zz @ B.T - t) ** 2).sum(axis=1)
    p = np.exp(-r2 / (2.0 * sigma * sigma))
    return zz, p / p.sum()


def _tv(z, p, half=12):
    inside = (np.abs(z) <= half).all(axis=1)
    idx = (z[inside, 0] + half) * (2 * half + 1) + (z[inside, 1] + half)
    emp = np.bincount(idx, minlength=p.size) / z.shape[0]
    return 0.5 * (np.abs(emp - p).sum() + (1.0 - inside.mean()))


def test_d2_total_variation():
    """d2, sigma 0.8, target (1.7, -0.6), seed 7, 2^14 draws: TV from the exact pmf <= 0.02
    (the project's threshold for "unbiased"), where Klein's draw gives >= 0.15."""
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import ExactSampler, KleinSampler
    B = np.array([[4.0, 1.0], [1.0, 3.0]])
    sigma, t, n = 0.8, np.array([1.7, -0.6]), 1 << 14
    zz, p = _d2_exact_pmf(B, sigma, t)
    ex = ExactSampler(SimpleLattice(B), sigma, t, seed=7)
    tv_exact = _tv(ex.sample_coefficients(n), p)
    tv_klein = _tv(KleinSampler(SimpleLattice(B), sigma, t, seed=7).sample_coefficients(n), p)
    print(f"  TV(exact) {tv_exact:.4f}, TV(Klein) {tv_klein:.4f}")
    assert tv_exact <= 0.02 and tv_klein >= 0.15


# ------------------------------------------------------------------ 4. state
def test_state_and_failed_tables(capi, setups):
    s = setups["int12"]
    ctx = _context(capi, s)
    with pytest.raises(capi.LgsError) as e:
        ctx.exact_sample_host(1, 0, 4, 1)
    assert e.value.code == capi.LGS_ERR_STATE
    _, big = _table(capi, s, "sizes")
    T, r2, sh = big["T"], np.ascontiguousarray(big["r2"]), np.ascontiguousarray(big["shift"])
    total, QF = int(big["offsets"][-1]), capi.LGS_TARGETS_QFRAME

    def attempt(r2_, max_nodes, max_points, match):
        out = dict(offsets=np.full(5, -1, dtype=np.int64), nodes=np.full(4, -1, dtype=np.int64),
                   status=np.full(4, -1, dtype=np.int32))
        with pytest.raises(capi.LgsError, match=match) as e:
            ctx.exact_table(T, 12.0, r2_, sh, max_nodes, max_points, flags=QF, **out)
        assert e.value.code == capi.LGS_ERR_INVALID
        with pytest.raises(capi.LgsError) as e2:  # no table is kept, a previous one is discarded
            ctx.exact_sample_host(1, 0, 4, 4)
        assert e2.value.code == capi.LGS_ERR_STATE
        return out

    ctx.exact_table(T, 12.0, r2, sh, MAX_NODES, total, flags=QF)
    assert ctx.exact_sample_host(1, 0, 4, 4)["z"].shape == (16, 12)
    out = attempt(r2, MAX_NODES, total - 1, "max_points")
    assert np.array_equal(out["offsets"], big["offsets"]) and np.array_equal(out["nodes"], big["nodes"])
    budget = int(big["nodes"].max()) - 1
    out = attempt(r2, budget, total, "status 1")
    assert out["status"].tolist() == (big["nodes"] > budget).astype(int).tolist() and out["status"].sum() == 1
    empty = r2.copy()
    empty[1] = 0.0
    out = attempt(empty, MAX_NODES, total, "no lattice point")
    assert out["offsets"][2] == out["offsets"][1] and not out["status"].any()
    ctx.exact_table(T, 12.0, r2, sh, MAX_NODES, total, flags=QF)  # the context is usable
    assert ctx.exact_sample_host(1, 0, 4, 4)["z"].shape == (16, 12)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], 1.0)
    with pytest.raises(capi.LgsError) as e:
        ctx.exact_sample_host(1, 0, 4, 4)
    assert e.value.code == capi.LGS_ERR_STATE


# ------------------------------------------------------------------ 5. Python
def test_exact_sampler_class(setups):
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import ExactSampler
    s = setups["int12"]
    lat = SimpleLattice(s["B"])
    c = s["T"][0]
    a = ExactSampler(lat, 12.0, c, nats=NATS, max_nodes=MAX_NODES, seed=3)
    b = ExactSampler(lat, 12.0, c, nats=NATS, max_nodes=MAX_NODES, seed=3)
    va, za = a.sample_with_coefficients(100)
    assert va.shape == (100, 12) and za.shape == (100, 12) and np.array_equal(va, za @ s["B"].T)
    assert np.array_equal(b.sample(60), va[:60]) and np.array_equal(b.sample(40), va[60:])  # the counter advances
    assert a.sample(1).shape == (1, 12) and a._next_sample == 101
    z, p = a.pmf()
    assert z.shape == (len(p), 12) and abs(p.sum() - 1.0) <= len(p) * 2.0 ** -52 and len(p) > 1000
    m = lat.__class__(s["B"].T).gaussian_mass(12.0, c, nats=NATS, max_nodes=MAX_NODES)
    assert a.log_mass == pytest.approx(float(m["log_mass"]), rel=1e-12) and m["points"] == len(p)
    pts, zs = a.sample_around(s["T"][1:4], 5, coefficients=True)
    assert pts.shape == (3, 5, 12) and np.array_equal(pts, zs @ s["B"].T) and a._next_sample == 116
    near = np.sum((pts - s["T"][1:4, None, :]) ** 2, axis=2)
    assert (near < np.sum(s["T"][1:4] ** 2, axis=1)[:, None]).all()
    assert math.isfinite(a.log_mass) and a.sample(3).shape == (3, 12)  # the centre table is rebuilt
