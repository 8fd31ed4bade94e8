"""Klein sampling around per-sample targets (lgs_klein_targets, KleinSampler.sample_around)
against the CPU oracle.

Sample k of a call is the draw of klein.py:181-220 with the centre c'_k = Q^T t_k, on the
Philox counters of Klein sample first + k.  The oracle is fed the c' the library reports
having used (cprime_out), one sample at a time, so the comparison is bit-exact; c' itself
is checked against T @ Q with the fp64 bound for sums of d products."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 4242


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


@pytest.fixture(scope="module")
def setups():
    """Per basis: B, sigma, Q, R and 700 targets (shared, read-only)."""
    out = {}
    for name, (B, sigma, integral) in _bases().items():
        Q, R = _qr(B)
        d = B.shape[0]
        T = np.random.default_rng(1000 + d).standard_normal((700, d)) * 2500.0
        for a in (B, Q, R, T):
            a.setflags(write=False)
        out[name] = dict(B=B, sigma=sigma, integral=integral, Q=Q, R=R, T=T, d=d)
    return out


def _context(capi, s, center=None, **kw):
    ctx = capi.Context(0, **kw)
    cp = np.zeros(s["d"]) if center is None else s["Q"].T @ center
    ctx.set_basis(s["R"], cp, s["B"], s["sigma"])
    ctx.set_decoder(Q=s["Q"])
    return ctx


def _oracle_rows(oracle, s, cprime, first, rows):
    return {k: oracle.klein(s["R"], cprime[k], s["sigma"], 1, seed=SEED, first_sample=first + k)["z"][0]
            for k in rows}


def _check_against_oracle(oracle, s, r, T, first):
    n, d = T.shape
    z, v, cp = r["z"], r["v"], r["cprime"]
    # c' = Q^T t: both sides are fp64 sums of d products in some order
    ref = T @ s["Q"]
    bound = 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(T) @ np.abs(s["Q"]))
    err = np.abs(cp - ref)
    print(f"  d={d} n={n}: max |c' - T Q| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    rows = range(n) if d <= 40 else range(0, n, 7)
    want = _oracle_rows(oracle, s, cp, first, rows)
    bad = [k for k in rows if not np.array_equal(z[k], want[k])]
    assert not bad, f"{len(bad)} of {len(want)} samples differ from the oracle, first {bad[:5]}"
    if s["integral"]:
        assert np.array_equal(v, z.astype(np.float64) @ s["B"].T)
    else:
        zf = z.astype(np.float64)  # real basis: two fp64 sums of d products
        assert (np.abs(v - zf @ s["B"].T) <= 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(zf) @ np.abs(s["B"]).T)).all()


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", BASES)
def test_oracle_parity(capi, oracle, setups, name, exact):
    s = setups[name]
    ctx = _context(capi, s)
    f = capi.LGS_EXACT_ORDER if exact else 0
    for n, first in ((1, 0), (63, 5), (64, 1000), (300, 77)):
        T = s["T"][:n]
        r = ctx.klein_targets_host(SEED, first, T, want_cprime=True, flags=f)
        _check_against_oracle(oracle, s, r, T, first)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_three_chunks_and_batch_invariance(capi, oracle, setups, exact):
    """n = 700 on max_proposals = 256: chunks of 256, 256 and 188 (padded to 192)
    lanes; and [0, 700) in one call equals [0, 300) followed by [300, 700)."""
    s = setups["qary40"]
    f = capi.LGS_EXACT_ORDER if exact else 0
    T = s["T"]
    ctx = _context(capi, s, max_proposals=256)
    r = ctx.klein_targets_host(SEED, 0, T, want_cprime=True, flags=f)
    _check_against_oracle(oracle, s, r, T, 0)
    a = ctx.klein_targets_host(SEED, 0, T[:300], want_cprime=True, flags=f)
    b = ctx.klein_targets_host(SEED, 300, T[300:], want_cprime=True, flags=f)
    for k in ("z", "v", "cprime"):
        assert np.array_equal(r[k], np.concatenate([a[k], b[k]])), k
    one = _context(capi, s).klein_targets_host(SEED, 0, T, flags=f)  # one chunk
    assert np.array_equal(one["z"], r["z"]) and np.array_equal(one["v"], r["v"])


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", ["qary40", "qary128"])
def test_fixed_centre_gives_lgs_klein(capi, setups, name, exact):
    """Every row equal to the context's c' (non-zero centre), passed in the Q frame:
    the z of lgs_klein for the same sample indices, across the roll-over of the
    counter's step word."""
    s = setups[name]
    center = np.random.default_rng(3).uniform(-4000.0, 4000.0, s["d"])
    ctx = _context(capi, s, center=center)
    cp = s["Q"].T @ center
    n, first = 300, 2 ** 32 - 5
    f = capi.LGS_EXACT_ORDER if exact else 0
    want = ctx.klein_host(SEED, first, n, want_v=False, flags=f)["z"]
    r = ctx.klein_targets_host(SEED, first, np.tile(cp, (n, 1)), want_cprime=True,
                               flags=f | capi.LGS_TARGETS_QFRAME)
    assert np.array_equal(r["cprime"], np.tile(cp, (n, 1)))  # verbatim
    assert np.array_equal(r["z"], want)


def test_default_equals_exact_order_d128(capi, setups):
    s = setups["qary128"]
    T = np.random.default_rng(8).standard_normal((4096, s["d"])) * 2500.0
    ctx = _context(capi, s)
    a = ctx.klein_targets_host(SEED, 0, T, want_v=False)["z"]
    b = ctx.klein_targets_host(SEED, 0, T, want_v=False, flags=capi.LGS_EXACT_ORDER)["z"]
    bad = int((a != b).any(axis=1).sum())
    print(f"  {bad} of 4096 samples differ, {ctx.resolved()} decisions redone in the reference's order")
    assert bad == 0


def test_widened_certificate_bound_forces_reference_order_decisions(capi, setups, monkeypatch):
    """The blocked kernel redoes a decision its certificate does not cover at the
    reference-order mean with the lane's own centre.  The hooks library widens every
    bound by 1 / LGS_TEST_Z1CAP_SCALE (still a bound): the decisions take that path,
    the output must not change, and LGS_COUNTER_RESOLVED must grow."""
    s = setups["qary128"]
    T = s["T"][:512]
    want = _context(capi, s).klein_targets_host(SEED, 9, T, want_v=False, flags=capi.LGS_EXACT_ORDER)["z"]
    monkeypatch.setenv("LGS_TEST_Z1CAP_SCALE", "1e-9")
    ctx = _context(capi, s, hooks=True)
    ctx.resolved(reset=True)
    got = ctx.klein_targets_host(SEED, 9, T, want_v=False)["z"]
    redone = ctx.resolved()
    print(f"  {redone} decisions redone of {T.size}")
    assert redone > T.shape[0]
    assert np.array_equal(got, want)


def test_large_coefficients(capi, oracle, setups):
    s = setups["int12"]
    d = s["d"]
    ctx = _context(capi, s)
    T = s["T"][:96] * 4000.0  # |t| ~ 1e7: |z| beyond the 16-bit range
    r = ctx.klein_targets_host(SEED, 3, T, want_cprime=True, flags=capi.LGS_Z64)
    assert np.abs(r["z"]).max() > 32767
    want = _oracle_rows(oracle, s, r["cprime"], 3, range(96))
    assert all(np.array_equal(r["z"][k], want[k]) for k in range(96))
    assert np.array_equal(r["v"], r["z"].astype(np.float64) @ s["B"].T)
    for f in (0, capi.LGS_EXACT_ORDER):
        assert np.array_equal(ctx.klein_targets_host(SEED, 3, T, want_v=False, flags=f)["z"], r["z"])
    # |z| >= 2^31: int32 buffers overflow, int64 succeed
    T = s["T"][:70] * 1e9
    z32 = np.empty((70, d), dtype=np.int32)
    for f in (0, capi.LGS_EXACT_ORDER):
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_targets(SEED, 0, T, z32, None, None, f)
        assert e.value.code == capi.LGS_ERR_OVERFLOW
    z64 = np.empty((70, d), dtype=np.int64)
    cp = np.empty((70, d))
    ctx.klein_targets(SEED, 0, T, z64, None, cp, capi.LGS_Z64)
    assert np.abs(z64).max() >= 2 ** 31
    want = _oracle_rows(oracle, s, cp, 0, range(0, 70, 7))
    assert all(np.array_equal(z64[k], want[k]) for k in want)


@pytest.mark.parametrize("name", ["qary40", "ntru64"])
def test_device_pointers_coordinate_major(capi, setups, name):
    import torch
    s = setups[name]
    n, d = 300, s["d"]
    T = s["T"][:n]
    ctx = _context(capi, s)
    host = ctx.klein_targets_host(SEED, 21, T, want_cprime=True, flags=capi.LGS_Z64)
    f = capi.LGS_DEVICE_PTRS | capi.LGS_COORD_MAJOR | capi.LGS_Z64
    t = torch.as_tensor(np.ascontiguousarray(T.T), device="cuda")
    z = torch.empty((d, n), dtype=torch.int64, device="cuda")
    v = torch.empty((n, d), dtype=torch.float64, device="cuda")
    cp = torch.empty((n, d), dtype=torch.float64, device="cuda")
    ctx.klein_targets(SEED, 21, t, z, v, cp, f)
    torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy().T, host["z"])
    assert np.array_equal(v.cpu().numpy(), host["v"])
    assert np.array_equal(cp.cpu().numpy(), host["cprime"])
    # the Q frame, coordinate-major on the device: c' taken verbatim
    z2 = torch.empty_like(z)
    ctx.klein_targets(SEED, 21, cp.T.contiguous(), z2, None, None, f | capi.LGS_TARGETS_QFRAME)
    torch.cuda.synchronize()
    assert torch.equal(z2, z)


def test_errors(capi, setups):
    s = setups["qary40"]
    d = s["d"]
    T = np.array(s["T"][:10])
    ctx = capi.Context(0)
    ctx.set_basis(s["R"], np.zeros(d), s["B"], s["sigma"])
    z = np.empty((10, d), dtype=np.int32)
    with pytest.raises(capi.LgsError) as e:  # no Q uploaded, targets in the lattice frame
        ctx.klein_targets(SEED, 0, T, z)
    assert e.value.code == capi.LGS_ERR_STATE
    ctx.klein_targets(SEED, 0, T, z, None, None, capi.LGS_TARGETS_QFRAME)  # needs no Q
    ctx.klein_targets(SEED, 0, T[:0], None)  # n == 0
    ctx.set_decoder(Q=s["Q"])
    for f in (capi.LGS_WANG_LING, capi.LGS_LOGW_BOUND, capi.LGS_SAMPLEZ_TABLE):
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_targets(SEED, 0, T, z, None, None, f)
        assert e.value.code == capi.LGS_ERR_INVALID
    for f in (0, capi.LGS_EXACT_ORDER, capi.LGS_TARGETS_QFRAME):
        bad = T.copy()
        bad[4, 7] = np.nan
        with pytest.raises(capi.LgsError) as e:
            ctx.klein_targets(SEED, 0, bad, z, None, None, f)
        assert e.value.code == capi.LGS_ERR_NONFINITE
    ctx.klein_targets(SEED, 0, T, z)  # the context is usable after an error


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_sampler_sample_around(setups, exact):
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import KleinSampler
    s = setups["qary40"]
    lat = SimpleLattice(s["B"])
    T = s["T"][:130]
    smp = KleinSampler(lat, s["sigma"], seed=11, exact_order=exact)
    pts, z = smp.sample_around(T, coefficients=True)
    ref = smp.context.klein_targets_host(11, 0, T, flags=smp._flags())
    assert np.array_equal(pts, ref["v"]) and np.array_equal(z, ref["z"])
    assert np.array_equal(pts, z.astype(np.float64) @ s["B"].T)
    # the points are near their targets: ||v - t||^2 = sum_i (R_ii (z_i - mu_i))^2 and every
    # draw lies in its support window, |z_i - mu_i| <= precision * sigma / R_ii + 1 (klein.py:113-128)
    assert np.linalg.norm(pts - T, axis=1).max() <= np.linalg.norm(10.0 * s["sigma"] + np.diag(s["R"])) * (1 + 1e-9)
    one = smp.sample_around(T[0])  # sample 130
    assert one.shape == (s["d"],)
    assert np.array_equal(one, smp.context.klein_targets_host(11, 130, T[:1], flags=smp._flags())["v"][0])
    nxt = smp.sample(5)  # samples 131..135
    fresh = KleinSampler(lat, s["sigma"], seed=11, exact_order=exact)
    assert np.array_equal(nxt, fresh.sample(136)[131:])
