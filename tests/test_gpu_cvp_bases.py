"""Exact closest vectors over a batch of bases (lgs_closest_vector_bases,
lgs_amd.decode.closest_vector_bases) against the CPU transcription: tests/qr_oracle.py for QR(p)
and the lattice point, tests/cvp_oracle.py (unchanged) for the search.  Every output -- R, c', z, v,
dist2, nodes, status, qr_status -- compares bit for bit, with no tolerance.
tests/test_cvp_bases_host.py holds the premises: the transcription agrees with NumPy's QR, and
every parity problem ends with status 0 far below the budget used here."""
import math

import numpy as np
import pytest

import cvp_oracle
import lll_oracle
import qr_oracle

pytestmark = pytest.mark.gpu

MAX_NODES = qr_oracle.PARITY_NODES
KEYS = qr_oracle.KEYS


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


def _run(capi, ctx, Bs, Ts, max_nodes=MAX_NODES, radius2=None, z64=False, dev=False):
    """The raw call on host arrays or device tensors, every output prefilled with a sentinel;
    returns host arrays, z as int64."""
    n, T, d = Ts.shape
    zdt = np.int64 if z64 else np.int32
    host = {"z": np.full((n, T, d), -77, dtype=zdt), "v": np.full((n, T, d), np.nan),
            "dist2": np.full((n, T), np.nan), "nodes": np.full((n, T), -1, dtype=np.int64),
            "status": np.full((n, T), -1, dtype=np.int32), "qr_status": np.full(n, -1, dtype=np.int32),
            "R": np.full((n, d, d), np.nan), "cprime": np.full((n, T, d), np.nan)}
    b, t = np.ascontiguousarray(Bs, dtype=np.float64), np.ascontiguousarray(Ts, dtype=np.float64)
    r2 = None if radius2 is None else np.ascontiguousarray(radius2, dtype=np.float64)
    flags = capi.LGS_Z64 if z64 else 0
    if dev:
        import torch
        up = lambda a: None if a is None else torch.from_numpy(a).cuda()
        bufs = {k: up(a) for k, a in host.items()}
        b, t, r2 = up(b), up(t), up(r2)
        flags |= capi.LGS_DEVICE_PTRS
    else:
        bufs = host
    out = {k: bufs[k] for k in ("dist2", "nodes", "status", "qr_status", "R", "cprime")}
    try:
        ctx.closest_vector_bases(b, t, max_nodes, r2, bufs["z"], bufs["v"], flags=flags, **out)
    finally:
        if dev:
            torch.cuda.synchronize()
            host = {k: a.cpu().numpy() for k, a in bufs.items()}
        _run.last = host
    host["z"] = host["z"].astype(np.int64)
    return host


def _same(got, want, keys=KEYS):
    """Bit for bit: the bytes of every array (so -0.0 differs from +0.0 and +inf equals +inf)."""
    for k in keys:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(np.asarray(want[k], dtype=got[k].dtype))
        if g.shape != w.shape or g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w) if g.shape == w.shape else None
            raise AssertionError(f"{k} differs: first at {None if bad is None or not len(bad) else bad[0].tolist()}, "
                                 f"{0 if bad is None else len(bad)} elements")


# ------------------------------------------------------------------ 1. parity with the transcription
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("z64", [False, True], ids=["z32", "z64"])
@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_parity_with_the_transcription(capi, d, T, z64, dev):
    """n_bases = 1, 3, 130 of every shape; max_nodes = 2^16.  The transcription's node counts
    (minimum / median / maximum over the distinct problems): (2, 1) 4 / 14 / 95; (3, 2) 6 / 8 / 179;
    (17, 5) 42 / 366 / 923; (33, 64) 262 / 1729 / 5100; (64, 64) 294 / 1639 / 4318 -- it reports
    status 0 for every one (asserted on the CPU in test_cvp_bases_host.py), and every problem of
    every batch is compared."""
    ctx = capi.Context(0)
    for n in qr_oracle.BATCHES:
        Bs, Ts, _ = qr_oracle.batch(d, T, n)
        want = qr_oracle.expected(d, T, n)
        assert not want["status"].any()
        _same(_run(capi, ctx, Bs, Ts, z64=z64, dev=dev), want)


def test_130_bases_in_chunks_of_64(capi, monkeypatch):
    """The hooks library with 64 bases per chunk: chunks of 64, 64 and 2 bases."""
    d, T = 17, 5
    Bs, Ts, _ = qr_oracle.batch(d, T, 130)
    monkeypatch.setenv("LGS_TEST_CVPB_SLOTS", "64")
    ctx = capi.Context(0, hooks=True)
    ctx.timing_enable(True)
    _same(_run(capi, ctx, Bs, Ts), qr_oracle.expected(d, T, 130))
    assert ctx.timing_get(capi.KERNEL_CPRIME)[1] == 3  # one QR launch per chunk
    prod = capi.Context(0)  # the product library reads no environment: one chunk
    prod.timing_enable(True)
    _same(_run(capi, prod, Bs, Ts), qr_oracle.expected(d, T, 130))
    assert prod.timing_get(capi.KERNEL_CPRIME)[1] == 1


def test_host_wrappers_agree_with_the_raw_call(capi):
    from lgs_amd.decode import closest_vector_bases
    d, T = 17, 5
    Bs, Ts, _ = qr_oracle.batch(d, T, 3)
    want = qr_oracle.expected(d, T, 3)
    r = capi.Context(0).closest_vector_bases_host(Bs, Ts, MAX_NODES, want_cprime=True)
    _same(r, want)
    v, z, info = closest_vector_bases(Bs, Ts, max_nodes=MAX_NODES, coefficients=True)
    _same({"v": v, "z": z, **info}, want, ("v", "z", "dist2", "nodes", "status", "qr_status", "R"))
    v1, info1 = closest_vector_bases(np.swapaxes(Bs, 1, 2), Ts[:, 0], max_nodes=MAX_NODES, rows=True)
    assert np.array_equal(v1, want["v"][:, 0]) and np.array_equal(info1["nodes"], want["nodes"][:, 0])


# ------------------------------------------------------------------ 2. the single-basis path
@pytest.mark.parametrize("d,T", [(3, 2), (17, 5), (33, 64)])
def test_same_search_as_closest_vector_on_the_returned_frame(capi, d, T):
    """lgs_set_basis(R_out[p]) and lgs_closest_vector with LGS_TARGETS_QFRAME on cprime_out[p] visit
    the same nodes: z, dist2, nodes and status are identical."""
    Bs, Ts, _ = qr_oracle.batch(d, T, 3)
    got = _run(capi, capi.Context(0), Bs, Ts)
    one = capi.Context(0)
    for p in range(3):
        one.set_basis(np.ascontiguousarray(got["R"][p]), np.zeros(d), np.ascontiguousarray(Bs[p]), 1.0)
        r = one.closest_vector_host(got["cprime"][p], MAX_NODES, flags=capi.LGS_TARGETS_QFRAME, want_v=False)
        for k in ("z", "dist2", "nodes", "status"):
            assert np.array_equal(r[k], got[k][p]), (p, k)


# ------------------------------------------------------------------ 3. independence
def _deep_batch(n):
    """d = 32, T = 4: in turn the LLL-reduced qary32 (230 000 to 600 000 nodes per problem: beyond the
    default slice of 2^16) and the scaled sum of two reduced qary16 (about a thousand)."""
    deep = np.array(lll_oracle.reduced("qary32", 0.99)["basis_out"], dtype=np.float64)
    pair = [deep, qr_oracle.basis_for(32, 0)]
    Bs = np.stack([pair[p % 2] for p in range(n)])
    Ts = np.random.default_rng(7032).standard_normal((n, 4, 32)) * 2500.0
    return Bs, Ts


def test_slices_slots_and_split_calls_give_the_same_outputs(capi, monkeypatch):
    Bs, Ts = _deep_batch(6)
    budget = 1 << 22
    prod = capi.Context(0)
    prod.timing_enable(True)
    want = _run(capi, prod, Bs, Ts, max_nodes=budget)
    nodes = want["nodes"]
    print(f"  nodes {nodes.min()} .. {nodes.max()}, {prod.timing_get(capi.KERNEL_CVP_ENUM)[1]} launches")
    assert not want["status"].any()
    assert (nodes > 1 << 16).any() and (nodes <= 1 << 16).any()  # some cross the default slice, some do not
    assert prod.timing_get(capi.KERNEL_CVP_ENUM)[1] == -(-int(nodes.max()) // (1 << 16))
    # bases split over two calls
    a, b = _run(capi, prod, Bs[:1], Ts[:1], max_nodes=budget), _run(capi, prod, Bs[1:], Ts[1:], max_nodes=budget)
    _same({k: np.concatenate([a[k], b[k]]) for k in KEYS}, want)
    # few slots: two bases per chunk, the others wait
    monkeypatch.setenv("LGS_TEST_CVPB_SLOTS", "2")
    hooks = capi.Context(0, hooks=True)
    hooks.timing_enable(True)
    _same(_run(capi, hooks, Bs, Ts, max_nodes=budget, z64=True), want)
    assert hooks.timing_get(capi.KERNEL_CPRIME)[1] == 3
    monkeypatch.delenv("LGS_TEST_CVPB_SLOTS")
    # a slice of 64 nodes: the short problems (the second basis of the pair, and one deep one cut
    # short by its budget) are suspended and resumed many times
    monkeypatch.setenv("LGS_TEST_CVPB_SLICE", "64")
    short = 4000
    w2 = _run(capi, prod, Bs, Ts, max_nodes=short)
    sliced = capi.Context(0, hooks=True)
    sliced.timing_enable(True)
    _same(_run(capi, sliced, Bs, Ts, max_nodes=short), w2)
    launches = sliced.timing_get(capi.KERNEL_CVP_ENUM)[1]
    assert (w2["status"] == 0).any() and (w2["status"] == 1).any()
    assert launches == -(-int(w2["nodes"].max()) // 64)


# ------------------------------------------------------------------ 4. per-basis failure
def test_a_refused_basis_leaves_the_others_alone(capi):
    """Five bases of d = 17: basis 1 has a repeated column and basis 3 a zero column.  Both repeated
    columns are multiples of e_0, so that the dependence is exact in fp64 -- column 3 of W is
    exactly zero below row 0 when its turn comes -- and not a residue of rounding size."""
    d, T = 17, 5
    good, Ts, _ = qr_oracle.batch(d, T, 5)
    Bs = good.copy()
    Bs[1][:, 0] = 0.0
    Bs[1][0, 0] = 3.0
    Bs[1][:, 3] = Bs[1][:, 0]
    Bs[3][:, 7] = 0.0
    want = {k: np.stack([qr_oracle.solve(Bs[p], Ts[p], MAX_NODES)[k] for p in range(5)]) for k in KEYS}
    assert want["qr_status"].tolist() == [0, 3, 0, 3, 0]
    for dev in (False, True):
        got = _run(capi, capi.Context(0), Bs, Ts, dev=dev)
        _same(got, want)
        for p in (1, 3):
            assert (got["status"][p] == 3).all() and not got["z"][p].any() and not got["v"][p].any()
            assert np.isinf(got["dist2"][p]).all() and not got["nodes"][p].any()
            assert not got["R"][p].any() and not got["cprime"][p].any()
        clean = _run(capi, capi.Context(0), good[[0, 2, 4]], Ts[[0, 2, 4]], dev=dev)
        _same({k: got[k][[0, 2, 4]] for k in KEYS}, clean)


# ------------------------------------------------------------------ 5. budget and radius
def test_budget_and_radius_beside_finished_problems(capi):
    d, T = 17, 5
    Bs, Ts, _ = qr_oracle.batch(d, T, 3)
    full = qr_oracle.expected(d, T, 3)
    small = 480  # the 15 problems take 174 .. 923 nodes, on both sides of it in every basis
    want = {k: np.stack([qr_oracle.solve(Bs[p], Ts[p], small)[k] for p in range(3)]) for k in KEYS}
    got = _run(capi, capi.Context(0), Bs, Ts, max_nodes=small)
    _same(got, want)
    assert ((got["status"] == 1) == (full["nodes"] > small)).all() and (got["nodes"][got["status"] == 1] == small).all()
    assert all(set(got["status"][p]) == {0, 1} for p in range(3)), got["status"]  # both in every wave
    r2 = np.where(np.arange(3 * T).reshape(3, T) % 2 == 0, full["dist2"] * 0.999, np.inf)
    want = {k: np.stack([qr_oracle.solve(Bs[p], Ts[p], MAX_NODES, r2[p])[k] for p in range(3)]) for k in KEYS}
    for dev in (False, True):
        got = _run(capi, capi.Context(0), Bs, Ts, radius2=r2, dev=dev)
        _same(got, want)
        assert ((got["status"] == 2) == np.isfinite(r2)).all() and not got["z"][got["status"] == 2].any()
        assert np.isinf(got["dist2"][got["status"] == 2]).all()
    with pytest.raises(capi.LgsError) as e:
        _run(capi, capi.Context(0), Bs, Ts, radius2=np.where(r2 < np.inf, -1.0, r2))
    assert e.value.code == capi.LGS_ERR_INVALID


# ------------------------------------------------------------------ 6. ground truth
@pytest.mark.parametrize("d,T,half", [(2, 1, 12), (3, 2, 8)])
def test_returned_point_is_the_closest_in_a_box(capi, d, T, half):
    """Brute force in NumPy over the coefficient box returned z + [-half, half]^d: no point of it is
    closer to the target than the returned one (distances as ||t - B z|| in fp64; the margin is the
    rounding of that sum, 4 d ulps of the larger squared norm involved)."""
    n = 40
    Bs, Ts, _ = qr_oracle.batch(d, T, n)
    got = _run(capi, capi.Context(0), Bs, Ts)
    assert not got["status"].any()
    grid = np.stack(np.meshgrid(*[np.arange(-half, half + 1)] * d, indexing="ij"), axis=-1).reshape(-1, d)
    for p in range(n):
        for k in range(T):
            zz = got["z"][p, k][None, :] + grid
            D = ((Ts[p, k][None, :] - zz.astype(np.float64) @ Bs[p].T) ** 2).sum(axis=1)
            mine = ((Ts[p, k] - got["v"][p, k]) ** 2).sum()
            tol = 4 * d * 2.0 ** -52 * ((Ts[p, k] ** 2).sum() + (got["v"][p, k] ** 2).sum())
            assert mine <= D.min() + tol, (p, k, mine, D.min())
            assert abs(mine - got["dist2"][p, k]) <= tol


# ------------------------------------------------------------------ 7. reduce=True
def test_reduce_decodes_the_same_points_in_fewer_nodes(capi):
    """Raw qary_basis(16, 16, 3329) of three seeds, two random targets each, decoded in the caller's
    bases and in their LLL-reduced ones.  The targets are bounded-distance instances, a random
    lattice point plus uniform noise below 0.45 per coordinate: at the spread of the parity targets
    the raw basis -- Gram-Schmidt norms q, ..., q, 1, ..., 1 -- needs more than 2^27 nodes per
    problem, which no test can wait for.  On the CPU transcription the raw bases take 1634 to 7722
    nodes for these targets and the reduced ones 64 each, the minimum at d = 32."""
    from lgs_amd import lattices
    from lgs_amd.decode import closest_vector_bases
    d = 32
    Bs = np.stack([np.asarray(lattices.qary_basis(16, 16, 3329, seed)).T for seed in (1, 2, 3)]).astype(np.int64)
    rng = np.random.default_rng(50)
    z0 = rng.integers(-50, 51, size=(3, 2, d))
    Ts = np.einsum("nij,ntj->nti", Bs, z0).astype(np.float64) + rng.uniform(-0.45, 0.45, size=(3, 2, d))
    budget = 1 << 20
    v_raw, z_raw, i_raw = closest_vector_bases(Bs, Ts, max_nodes=budget, coefficients=True)
    v_red, z_red, i_red = closest_vector_bases(Bs, Ts, max_nodes=budget, reduce=True, coefficients=True)
    ratio = i_raw["nodes"] / i_red["nodes"]
    print(f"  nodes raw {i_raw['nodes'].tolist()} reduced {i_red['nodes'].tolist()} ratio {ratio.min():.1f} .. {ratio.max():.1f}")
    assert not i_raw["status"].any() and not i_red["status"].any() and not i_red["lll_status"].any()
    assert np.array_equal(v_raw, v_red)  # the same lattice points, exactly
    assert np.array_equal(z_raw, z0) and np.array_equal(z_red, z0)
    for p in range(3):
        for k in range(2):  # and the mapped coefficients are those points in the caller's basis
            assert np.array_equal(Bs[p] @ z_red[p, k], v_red[p, k].astype(np.int64))
    # dist2 = ||c' - R z||^2 from two factorisations: each c' carries an absolute error of order
    # d 2^-53 ||t|| (test_cvp_bases_host.py), so the two dist2 differ by that times 2 sqrt(dist2).
    # For targets as far from the lattice as they are long this is the relative 64 d 2^-53 on dist2
    # itself; these targets are 10^6 long and 1.5 away, and the bound has to say so.
    tnorm = np.linalg.norm(Ts, axis=2)
    diff = np.abs(i_raw["dist2"] - i_red["dist2"])
    print(f"  |dist2 raw - reduced| {diff.max():.3g}, bound {(64 * d * 2.0 ** -53 * np.sqrt(i_raw['dist2']) * tnorm).min():.3g}")
    assert (diff <= 64 * d * 2.0 ** -53 * np.sqrt(i_raw["dist2"]) * tnorm).all()
    assert (i_red["nodes"] < i_raw["nodes"]).all()


# ------------------------------------------------------------------ 8. errors
def _raw_rc(capi, ctx, n, d, T, flags, z=None):
    """lgs_closest_vector_bases itself, past the Python checks; returns its code."""
    b = np.tile(np.eye(max(d, 1)) * 3.0, (max(n, 1), 1, 1))
    t = np.zeros((max(n, 1), max(T, 1), max(d, 1)))
    return ctx._L.lgs_closest_vector_bases(ctx._h, n, d, T, capi._ptr(b), capi._ptr(t), None, 100,
                                           None if z is None else capi._ptr(z), None, None, flags)


def test_errors_leave_outputs_and_context_alone(capi):
    d, T = 3, 2
    Bs, Ts, _ = qr_oracle.batch(d, T, 3)
    want = qr_oracle.expected(d, T, 3)
    ctx = capi.Context(0)
    # a loaded basis and an exact table, to be found unchanged at the end
    s = cvp_oracle.setup("d3")
    ctx.set_basis(s["R"], np.zeros(3), s["B"], 1.0)
    ctx.set_decoder(Q=s["Q"])
    cv0 = ctx.closest_vector_host(s["T"][:8], 1 << 20)
    ctx.exact_table_host(s["T"][:4], 2.0, cv0["dist2"][:4] + 80.0)
    draws0 = ctx.exact_sample_host(11, 0, 16, 4)
    for dev in (False, True):
        for which in ("bases", "targets"):
            b, t = Bs.copy(), Ts.copy()
            (b if which == "bases" else t)[2, 1, 0] = np.nan if dev else np.inf
            with pytest.raises(capi.LgsError) as e:
                _run(capi, ctx, b, t, dev=dev)
            assert e.value.code == capi.LGS_ERR_NONFINITE
            out = _run.last  # every output still holds its sentinel
            assert (out["z"] == -77).all() and np.isnan(out["v"]).all() and np.isnan(out["R"]).all()
            assert (out["status"] == -1).all() and (out["qr_status"] == -1).all() and (out["nodes"] == -1).all()
            assert np.isnan(out["dist2"]).all() and np.isnan(out["cprime"]).all()
    for flags in (capi.LGS_EXACT_ORDER, capi.LGS_COORD_MAJOR, capi.LGS_TARGETS_QFRAME, 0x1000):
        assert _raw_rc(capi, ctx, 2, 3, 2, flags) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 65, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 65, 2, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 1, 2, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 0, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, -1, 3, 2, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 0, 3, 2, 0) == capi.LGS_OK and _raw_rc(capi, ctx, 2, 3, 2, 0) == capi.LGS_OK
    # |z| = 3 * 10^9 in a returned point
    big_b = np.array([[[1e-6, 0.0], [0.0, 1.0]]])
    big_t = np.array([[[3000.0, 0.25]]])
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, big_b, big_t)
    assert e.value.code == capi.LGS_ERR_OVERFLOW and (_run.last["z"] == -77).all() and np.isnan(_run.last["v"]).all()
    r = _run(capi, ctx, big_b, big_t, z64=True)
    assert r["z"].tolist() == [[[3000000000, 0]]] and r["status"].tolist() == [[0]]
    assert ctx.closest_vector_bases_host(big_b, big_t, 100)["z"].tolist() == [[[3000000000, 0]]]  # the wrapper retries
    # a conditional mean beyond 2^52
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, np.array([[[1e-14, 0.0], [0.0, 1.0]]]), big_t, z64=True)
    assert e.value.code == capi.LGS_ERR_NONFINITE and (_run.last["z"] == -77).all()
    # the context is still usable, its basis and its table are what they were
    _same(_run(capi, ctx, Bs, Ts), want)
    cv1 = ctx.closest_vector_host(s["T"][:8], 1 << 20)
    draws1 = ctx.exact_sample_host(11, 0, 16, 4)
    for k in ("z", "v", "dist2", "nodes", "status"):
        assert np.array_equal(cv0[k], cv1[k]), k
    for k in ("z", "v", "index", "dist2"):
        assert np.array_equal(draws0[k], draws1[k]), k
