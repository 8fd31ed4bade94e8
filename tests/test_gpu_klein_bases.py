"""Klein sampling and best-of-K decoding over a batch of bases (lgs_klein_bases,
lgs_amd.samplers.klein_bases, lgs_amd.decode.sampling_decode_bases) against the CPU transcription
tests/kleinb_oracle.py: QR(p) from tests/qr_oracle.py, the draws from the C oracle, D, the select
and the lattice point in the defined order.  Every output -- qr_status, R, c', every draw and its
distance, best_draw, dist2, z, v, status -- compares bit for bit, with no tolerance.
tests/test_klein_bases_host.py holds the premises of the inputs."""
import numpy as np
import pytest

import kleinb_oracle
import qr_oracle

pytestmark = pytest.mark.gpu

KEYS = kleinb_oracle.KEYS
SEED = kleinb_oracle.SEED
OUTS = ("best_draw", "dist2", "status", "qr_status", "R", "cprime", "z_draws", "dist2_draws")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


def _run(capi, ctx, Bs, Ts, sigma, K, seed=SEED, first=0, z64=False, dev=False, precision=10):
    """The raw call on host arrays or device tensors, every output prefilled with a sentinel;
    returns host arrays, z and z_draws as int64."""
    n, T, d = Ts.shape
    zdt = np.int64 if z64 else np.int32
    host = {"z": np.full((n, T, d), -77, dtype=zdt), "v": np.full((n, T, d), np.nan),
            "best_draw": np.full((n, T), -5, dtype=np.int64), "dist2": np.full((n, T), np.nan),
            "status": np.full((n, T), -1, dtype=np.int32), "qr_status": np.full(n, -1, dtype=np.int32),
            "R": np.full((n, d, d), np.nan), "cprime": np.full((n, T, d), np.nan),
            "z_draws": np.full((n, T, K, d), -77, dtype=zdt), "dist2_draws": np.full((n, T, K), np.nan)}
    b, t = np.ascontiguousarray(Bs, dtype=np.float64), np.ascontiguousarray(Ts, dtype=np.float64)
    s = np.ascontiguousarray(sigma, dtype=np.float64)
    flags = capi.LGS_Z64 if z64 else 0
    if dev:
        import torch
        up = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: the oracle's arrays are read-only)
        bufs = {k: up(a) for k, a in host.items()}
        b, t, s = up(b), up(t), up(s)
        flags |= capi.LGS_DEVICE_PTRS
    else:
        bufs = host
    try:
        ctx.klein_bases(seed, first, b, t, s, K, precision, bufs["z"], bufs["v"], flags=flags,
                        **{k: bufs[k] for k in OUTS})
    finally:
        if dev:
            torch.cuda.synchronize()
            host = {k: a.cpu().numpy() for k, a in bufs.items()}
        _run.last = host
    host["z"], host["z_draws"] = host["z"].astype(np.int64), host["z_draws"].astype(np.int64)
    return host


def _same(got, want, keys=KEYS):
    """Bit for bit: the bytes of every array (so -0.0 differs from +0.0 and +inf equals +inf)."""
    for k in keys:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(np.asarray(want[k], dtype=got[k].dtype))
        if g.shape != w.shape or g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w) if g.shape == w.shape else None
            raise AssertionError(f"{k} differs: first at {None if bad is None or not len(bad) else bad[0].tolist()}, "
                                 f"{0 if bad is None else len(bad)} elements")


def _sentinels_intact(out):
    assert (out["z"] == -77).all() and (out["z_draws"] == -77).all() and np.isnan(out["v"]).all()
    assert np.isnan(out["R"]).all() and np.isnan(out["cprime"]).all() and np.isnan(out["dist2"]).all()
    assert np.isnan(out["dist2_draws"]).all() and (out["best_draw"] == -5).all()
    assert (out["status"] == -1).all() and (out["qr_status"] == -1).all()


# ------------------------------------------------------------------ 1. parity with the transcription
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("z64", [False, True], ids=["z32", "z64"])
@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_parity_with_the_transcription(capi, d, T, z64, dev):
    """n_bases = 1, 3, 130 of every shape, widths 3 / 300 / 3000 in turn, K from
    kleinb_oracle.PARITY_K: 1 to 350 lanes per basis, blocks of 256 lanes (d <= 32) and 128."""
    ctx = capi.Context(0)
    for K in kleinb_oracle.PARITY_K[(d, T)]:
        for n in qr_oracle.BATCHES:
            Bs, Ts, _ = qr_oracle.batch(d, T, n)
            want = kleinb_oracle.expected(d, T, n, K)
            _same(_run(capi, ctx, Bs, Ts, want["sigma"], K, z64=z64, dev=dev), want)


# ------------------------------------------------------------------ 2. the single-basis path
@pytest.mark.parametrize("libm", [False, True], ids=["table", "libm"])
@pytest.mark.parametrize("d,T", [(3, 2), (17, 5), (33, 64)])
def test_same_draws_as_klein_decode_on_the_returned_frame(capi, d, T, libm):
    """lgs_set_basis(R_out[p], sigma_p), then lgs_klein_decode with LGS_EXACT_ORDER |
    LGS_TARGETS_QFRAME on cprime_out[p] from first_sample + p T K: the same winners, draw indices
    and distances; lgs_klein_targets on the c' rows repeated K times: the same draws."""
    K, n, first = 5, 3, 11
    Bs, Ts, idx = qr_oracle.batch(d, T, n)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    got = _run(capi, capi.Context(0, samplez_libm=libm), Bs, Ts, sigma, K, first=first)
    one = capi.Context(0, samplez_libm=libm)
    fl = capi.LGS_EXACT_ORDER | capi.LGS_TARGETS_QFRAME
    for p in range(n):
        one.set_basis(np.ascontiguousarray(got["R"][p]), np.zeros(d), np.ascontiguousarray(Bs[p]), float(sigma[p]))
        cp = np.ascontiguousarray(got["cprime"][p])
        r = one.klein_decode_host(SEED, first + p * T * K, cp, K, want_z=True, want_v=False, flags=fl)
        assert np.array_equal(r["z"], got["z"][p]), p
        assert np.array_equal(r["best_draw"], got["best_draw"][p]), p
        assert r["dist2"].tobytes() == got["dist2"][p].tobytes(), p
        rows = np.ascontiguousarray(np.repeat(cp, K, axis=0))
        rt = one.klein_targets_host(SEED, first + p * T * K, rows, want_z=True, want_v=False, flags=fl)
        assert np.array_equal(rt["z"].reshape(T, K, d), got["z_draws"][p]), p


# ------------------------------------------------------------------ 3. independence
def test_split_calls_and_chunks_give_the_same_bytes(capi, monkeypatch):
    d, T, K = 17, 5, 3
    Bs, Ts, _ = qr_oracle.batch(d, T, 130)
    want = kleinb_oracle.expected(d, T, 130, K)
    sg = want["sigma"]
    prod = capi.Context(0)
    prod.timing_enable(True)
    whole = _run(capi, prod, Bs, Ts, sg, K)
    _same(whole, want)
    assert prod.timing_get(capi.KERNEL_CPRIME)[1] == 1 and prod.timing_get(capi.KERNEL_KLEIN)[1] == 1
    assert prod.timing_get(capi.KERNEL_DECODE_SELECT)[1] == 1
    a = _run(capi, prod, Bs[:57], Ts[:57], sg[:57], K)
    b = _run(capi, prod, Bs[57:], Ts[57:], sg[57:], K, first=57 * T * K)
    _same({k: np.concatenate([a[k], b[k]]) for k in KEYS}, whole)
    monkeypatch.setenv("LGS_TEST_KLEINB_SLOTS", "64")
    hooks = capi.Context(0, hooks=True)
    hooks.timing_enable(True)
    _same(_run(capi, hooks, Bs, Ts, sg, K), whole)
    assert hooks.timing_get(capi.KERNEL_CPRIME)[1] == 3  # one QR launch per chunk: 64, 64 and 2 bases
    again = capi.Context(0)  # the product library reads no environment: one chunk
    again.timing_enable(True)
    _same(_run(capi, again, Bs, Ts, sg, K), whole)
    assert again.timing_get(capi.KERNEL_CPRIME)[1] == 1


def test_the_step_counter_changes_inside_the_batch(capi):
    """first_sample = 2^32 - 7: sample 7 of the batch is the first with step 1."""
    d, T, K, n = 17, 5, 3, 3
    first = (1 << 32) - 7
    Bs, Ts, _ = qr_oracle.batch(d, T, n)
    want = kleinb_oracle.expected(d, T, n, K, first_sample=first)
    got = _run(capi, capi.Context(0), Bs, Ts, want["sigma"], K, first=first)
    _same(got, want)
    low = kleinb_oracle.expected(d, T, n, K)
    assert not np.array_equal(got["z_draws"], low["z_draws"])


# ------------------------------------------------------------------ 4. rounded coordinates
def test_rounded_coordinates_are_not_drawn(capi):
    d, T, K, n = 17, 5, 3, 3
    Bs, Ts, idx = qr_oracle.batch(d, T, n)
    sigma = np.full(n, 1e-9)
    want = {k: np.stack([kleinb_oracle.solve(Bs[p], Ts[p], 1e-9, K, SEED, p * T * K,
                                             qr=kleinb_oracle.qr_of(d, T, idx[p]))[k] for p in range(n)]) for k in KEYS}
    assert (1e-9 / np.diagonal(want["R"], axis1=1, axis2=2) < 1e-10).all()
    for dev in (False, True):
        got = _run(capi, capi.Context(0), Bs, Ts, sigma, K, dev=dev)
        _same(got, want)
        assert (got["z_draws"] == got["z_draws"][:, :, :1]).all() and not got["best_draw"].any()


# ------------------------------------------------------------------ 5. per-basis failure
def test_a_refused_basis_leaves_the_others_alone(capi):
    d, T, K = 17, 5, 3
    good, Ts, idx = qr_oracle.batch(d, T, 3)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    Bs = good.copy()
    Bs[1][:, 7] = 0.0
    want = {k: np.stack([kleinb_oracle.solve(Bs[p], Ts[p], sigma[p], K, SEED, p * T * K)[k] for p in range(3)])
            for k in KEYS}
    assert want["qr_status"].tolist() == [0, 3, 0]
    for dev in (False, True):
        got = _run(capi, capi.Context(0), Bs, Ts, sigma, K, dev=dev)
        _same(got, want)
        assert (got["status"][1] == 3).all() and not got["z"][1].any() and not got["v"][1].any()
        assert np.isinf(got["dist2"][1]).all() and (got["best_draw"][1] == -1).all()
        assert not got["R"][1].any() and not got["cprime"][1].any()
        for p in (0, 2):
            alone = _run(capi, capi.Context(0), good[p:p + 1], Ts[p:p + 1], sigma[p:p + 1], K, first=p * T * K, dev=dev)
            _same({k: got[k][p:p + 1] for k in KEYS}, alone)


# ------------------------------------------------------------------ 6. errors
def _raw_rc(capi, ctx, n, d, T, K, flags, precision=10):
    """lgs_klein_bases itself, past the Python checks; returns its code."""
    b = np.tile(np.eye(max(d, 1)) * 3.0, (max(n, 1), 1, 1))
    t = np.zeros((max(n, 1), max(T, 1), max(d, 1)))
    s = np.ones(max(n, 1))
    return ctx._L.lgs_klein_bases(ctx._h, 0, 0, n, d, T, K, capi._ptr(b), capi._ptr(t), capi._ptr(s), precision,
                                  None, None, None, flags)


def test_errors_leave_outputs_alone(capi):
    d, T, K = 3, 2, 3
    Bs, Ts, idx = qr_oracle.batch(d, T, 3)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    ctx = capi.Context(0)
    for dev in (False, True):
        t = Ts.copy()
        t[2, 1, 0] = np.nan
        with pytest.raises(capi.LgsError) as e:
            _run(capi, ctx, Bs, t, sigma, K, dev=dev)
        assert e.value.code == capi.LGS_ERR_NONFINITE
        _sentinels_intact(_run.last)
        b = Bs.copy()
        b[1, 0, 2] = np.inf
        with pytest.raises(capi.LgsError) as e:
            _run(capi, ctx, b, Ts, sigma, K, dev=dev)
        assert e.value.code == capi.LGS_ERR_NONFINITE
        _sentinels_intact(_run.last)
        for bad in (0.0, -1.0, np.nan):
            s = sigma.copy()
            s[1] = bad
            with pytest.raises(capi.LgsError) as e:
                _run(capi, ctx, Bs, Ts, s, K, dev=dev)
            assert e.value.code == capi.LGS_ERR_INVALID
            _sentinels_intact(_run.last)
    for flags in (capi.LGS_EXACT_ORDER, capi.LGS_COORD_MAJOR, capi.LGS_TARGETS_QFRAME, 0x1000):
        assert _raw_rc(capi, ctx, 2, 3, 2, 3, flags) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 1, 2, 3, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 65, 2, 3, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 65, 3, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 0, 3, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 0, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, (1 << 21) + 1, 0) == capi.LGS_ERR_INVALID  # T K > 2^22
    assert _raw_rc(capi, ctx, 2, 3, 2, 3, 0, precision=0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, -1, 3, 2, 3, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 0, 3, 2, 3, 0) == capi.LGS_OK and _raw_rc(capi, ctx, 2, 3, 2, 3, 0) == capi.LGS_OK
    # |z| near 10^12 / 3 in every draw
    big_b = np.array([[[3.0, 1.0], [0.0, 2.0]]])
    big_t = np.array([[[1e12, 0.25]]])
    big_s = np.array([2.0])
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, big_b, big_t, big_s, K)
    assert e.value.code == capi.LGS_ERR_OVERFLOW
    _sentinels_intact(_run.last)
    want = kleinb_oracle.solve(big_b[0], big_t[0], 2.0, K, SEED, 0)
    assert np.abs(want["z_draws"]).max() > 1 << 31
    for dev in (False, True):
        _same(_run(capi, ctx, big_b, big_t, big_s, K, z64=True, dev=dev), {k: want[k][None] for k in KEYS})
    r = ctx.klein_bases_host(SEED, 0, big_b, big_t, big_s, K, want_draws=True)  # the wrapper retries
    assert np.array_equal(r["z_draws"], want["z_draws"][None])
    # the context is still usable
    good = kleinb_oracle.expected(d, T, 3, K)
    _same(_run(capi, ctx, Bs, Ts, sigma, K), good)


# ------------------------------------------------------------------ 7. wrappers
def test_wrappers_agree_with_the_raw_call(capi):
    from lgs_amd.decode import sampling_decode_bases
    from lgs_amd.samplers import klein_bases
    d, T, K = 17, 5, 3
    Bs, Ts, _ = qr_oracle.batch(d, T, 3)
    want = kleinb_oracle.expected(d, T, 3, K)
    sg = want["sigma"]
    r = capi.Context(0).klein_bases_host(SEED, 0, Bs, Ts, sg, K, want_cprime=True, want_draws=True)
    _same(r, want)
    v, z, info = sampling_decode_bases(Bs, Ts, K, sg, seed=SEED, coefficients=True)
    _same({"v": v, "z": z, **info}, want, ("v", "z", "best_draw", "dist2", "status", "qr_status", "R"))
    v1, info1 = sampling_decode_bases(np.swapaxes(Bs, 1, 2), Ts, K, sg, seed=SEED, rows=True)
    assert v1.tobytes() == want["v"].tobytes() and np.array_equal(info1["best_draw"], want["best_draw"])
    pts, zd = klein_bases(Bs, sg, Ts, n_draws=K, seed=SEED, coefficients=True)
    assert pts.shape == (3, T, K, d) and np.array_equal(zd, want["z_draws"])
    assert np.array_equal(pts, np.einsum("nij,ntkj->ntki", Bs, want["z_draws"].astype(np.float64)))
    pts1, zd1 = klein_bases(np.swapaxes(Bs, 1, 2), sg, Ts, n_draws=K, seed=SEED, rows=True, coefficients=True)
    assert np.array_equal(zd1, zd) and np.array_equal(pts1, pts)
    # one zero target per basis, a scalar width, later sample indices: the T axis is dropped
    p0, z0 = klein_bases(Bs, 300.0, n_draws=4, seed=SEED, first_sample=9, coefficients=True)
    raw = capi.Context(0).klein_bases_host(SEED, 9, Bs, np.zeros((3, 1, d)), np.full(3, 300.0), 4, want_draws=True)
    assert p0.shape == (3, 4, d) and np.array_equal(z0, raw["z_draws"][:, 0])


def test_reduce_draws_on_the_reduced_bases_and_maps_back(capi):
    """Raw qary_basis(16, 16, 3329) of three seeds: z = U z_reduced exactly, v = qr_oracle.point(B, z)
    bit for bit, dist2 the minimum of the target's dist2_draws row on the reduced basis."""
    from lgs_amd import lattices
    from lgs_amd.decode import sampling_decode_bases
    d, T, K, sigma = 32, 2, 8, 20.0
    Bs = np.stack([np.asarray(lattices.qary_basis(16, 16, 3329, seed)).T for seed in (1, 2, 3)]).astype(np.int64)
    rng = np.random.default_rng(51)
    z0 = rng.integers(-50, 51, size=(3, T, d))
    Ts = np.einsum("nij,ntj->nti", Bs, z0).astype(np.float64) + rng.uniform(-0.45, 0.45, size=(3, T, d))
    v, z, info = sampling_decode_bases(Bs, Ts, K, sigma, seed=SEED, reduce=True, coefficients=True)
    assert not info["lll_status"].any() and not info["status"].any()
    ctx = capi.Context(0)
    lr = ctx.lll_reduce_host(Bs)
    assert not lr["status"].any()
    red = ctx.klein_bases_host(SEED, 0, lr["basis"].astype(np.float64), Ts, np.full(3, sigma), K, want_draws=True)
    for p in range(3):
        for k in range(T):
            zz = [int(x) for x in (lr["U"][p].astype(object) @ red["z"][p, k].astype(object))]
            assert z[p, k].tolist() == zz
            assert v[p, k].tobytes() == qr_oracle.point(Bs[p], z[p, k]).tobytes()
    assert info["dist2"].tobytes() == red["dist2_draws"].min(axis=2).tobytes()
    assert np.array_equal(info["best_draw"], red["best_draw"])
