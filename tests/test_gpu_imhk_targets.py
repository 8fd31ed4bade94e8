"""IMHK chains around per-target centres (lgs_imhk_targets, IMHKSampler.sample_around)
against the CPU oracle.

Target k of a call is chain first_chain + k: its draw t = 0 .. n_steps is Klein's draw
around c'_k = Q^T t_k on the Philox counters (chain, step t) with the Wang-Ling log weight,
and the state after the Metropolis scan over those draws is returned.  The oracle runs one
chain per target with the c' the library reports having used (cprime_out), so coefficients
and accept counts compare bit for bit; log weights compare to rtol 1e-9, the tolerance
tests/test_gpu_parity.py uses for lgs_imhk's weights (the device SampleZ normaliser and the
oracle's logsumexp are different evaluations of the same sum)."""
import numpy as np
import pytest

from test_imhk_targets_host import d2_exact_pmf, tv_distance

pytestmark = pytest.mark.gpu

SEED = 4242
# LGS_TEST_WL_BOUND_SCALE values of test_default_equals_exact_order.  The weight bounds of
# qary128 are 7e-4 .. 6e-3 per draw (the actual differences stay below 3e-11) and leave no
# decision of the 7936 open at scale 1; 3e3, the value of tests/test_gpu_wl_accept.py,
# sends 55 of them through the recomputation, and 1e8 every one.  Each must leave every
# output unchanged.
BOUND_SCALES = (3e3, 1e8)


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
    """Per basis: B, sigma, Q, R and 256 targets (shared, read-only)."""
    out = {}
    for name, (B, sigma, integral) in _bases().items():
        Q, R = _qr(B)
        d = B.shape[0]
        T = np.random.default_rng(1000 + d).standard_normal((256, d)) * 2500.0
        for a in (B, Q, R, T):
            a.setflags(write=False)
        out[name] = dict(B=B, sigma=sigma, integral=integral, Q=Q, R=R, T=T, d=d)
    return out


def _context(capi, s, center=None, sigma=None, **kw):
    ctx = capi.Context(0, **kw)
    cp = np.zeros(s["d"]) if center is None else s["Q"].T @ center
    ctx.set_basis(s["R"], cp, s["B"], s["sigma"] if sigma is None else sigma)
    ctx.set_decoder(Q=s["Q"])
    return ctx


def _check_against_oracle(oracle, s, r, T, first_chain, n_steps):
    """z, accepts, logw against one oracle chain per target; c' and v as
    tests/test_gpu_targets.py checks them."""
    n, d = T.shape
    z, v, cp = r["z"], r["v"], r["cprime"]
    ref = T @ s["Q"]  # c' = Q^T t: both sides are fp64 sums of d products in some order
    bound = 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(T) @ np.abs(s["Q"]))
    assert (np.abs(cp - ref) <= bound).all()
    rows = range(n) if d <= 40 else range(0, n, 7)
    bad_z, bad_a, worst = [], [], 0.0
    for k in rows:
        o = oracle.imhk(s["R"], cp[k], s["B"], s["sigma"], 1, n_steps, seed=SEED, first_chain=first_chain + k,
                        mode=oracle.IMHK_WANG_LING)
        if not np.array_equal(z[k], o["z"][0]):
            bad_z.append(k)
        if r["accepts"][k] != o["accepts"][0]:
            bad_a.append(k)
        worst = max(worst, abs(r["logw"][k] - o["lw"][0]) / abs(o["lw"][0]))
    print(f"  d={d} n={n} first_chain={first_chain} steps={n_steps}: max rel logw err {worst:.2e}, "
          f"accepted {int(r['accepts'].sum())} of {n * n_steps}")
    assert not bad_z, f"{len(bad_z)} of {len(rows)} final states differ from the oracle, first {bad_z[:5]}"
    assert not bad_a, f"{len(bad_a)} of {len(rows)} accept counts differ from the oracle, first {bad_a[:5]}"
    assert worst <= 1e-9
    if s["integral"]:
        assert np.array_equal(v, z.astype(np.float64) @ s["B"].T)
    else:
        zf = z.astype(np.float64)  # real basis: two fp64 sums of d products
        assert (np.abs(v - zf @ s["B"].T) <= 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(zf) @ np.abs(s["B"]).T)).all()
    assert ((r["final_step"] >= 0) & (r["final_step"] <= n_steps)).all()
    assert np.array_equal(r["final_step"] > 0, r["accepts"] > 0)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("n_steps", [31, 6])
@pytest.mark.parametrize("name", BASES)
def test_oracle_parity(capi, oracle, setups, name, n_steps, exact):
    """K = 32 draws per chain (whole chains per wave) and K = 7 (a chain's lanes straddle
    waves, the last wave is padded)."""
    s = setups[name]
    ctx = _context(capi, s)
    f = capi.LGS_EXACT_ORDER if exact else 0
    acc = tot = 0
    for n in (1, 63, 64, 130):
        for first_chain in (0, 1000):
            T = s["T"][:n]
            r = ctx.imhk_targets_host(SEED, first_chain, T, n_steps, want_cprime=True, flags=f)
            _check_against_oracle(oracle, s, r, T, first_chain, n_steps)
            acc += int(r["accepts"].sum())
            tot += n * n_steps
    assert ctx.counter(capi.LGS_COUNTER_WL_MISMATCH) == 0
    if n_steps == 31 and name in ("qary40", "ntru64", "qary128"):  # (the oracle: about 0.10 on each)
        assert 0 < acc < tot


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", BASES)
def test_zero_steps_is_klein_targets(capi, setups, name, exact):
    s = setups[name]
    ctx = _context(capi, s)
    f = capi.LGS_EXACT_ORDER if exact else 0
    for n, first_chain in ((130, 0), (64, 1000)):
        T = s["T"][:n]
        want = ctx.klein_targets_host(SEED, first_chain, T, want_cprime=True, flags=f)
        r = ctx.imhk_targets_host(SEED, first_chain, T, 0, want_cprime=True, want_trace=True, flags=f)
        for k in ("z", "v", "cprime"):
            assert np.array_equal(r[k], want[k]), k
        assert not r["accepts"].any() and not r["final_step"].any()
        assert r["accepted"].shape == (n, 0) and np.array_equal(r["logw_draws"][:, 0], r["logw"])


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("name", ["qary40", "qary128"])
def test_fixed_centre_gives_lgs_imhk(capi, setups, name, exact):
    """Every row equal to the context's c' (non-zero centre), passed in the Q frame: the
    chains of lgs_imhk_trace(LGS_WANG_LING) from uninitialised states, first_step 1."""
    s = setups[name]
    d = s["d"]
    center = np.random.default_rng(3).uniform(-4000.0, 4000.0, d)
    ctx = _context(capi, s, center=center)
    cp = s["Q"].T @ center
    n, first_chain, n_steps = 130, 1000, 31
    f = capi.LGS_EXACT_ORDER if exact else 0
    z = np.zeros((n, d), dtype=np.int32)
    lw, init, acc = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    trace = np.zeros((n, n_steps), dtype=np.uint8)
    ctx.imhk(SEED, first_chain, n, 1, n_steps, 1, z, lw, init, acc, flags=f | capi.LGS_WANG_LING, accepted=trace)
    r = ctx.imhk_targets_host(SEED, first_chain, np.tile(cp, (n, 1)), n_steps, want_cprime=True, want_trace=True,
                              flags=f | capi.LGS_TARGETS_QFRAME)
    assert np.array_equal(r["cprime"], np.tile(cp, (n, 1)))  # verbatim
    assert np.array_equal(r["z"], z)
    assert np.array_equal(r["accepts"], acc)
    assert np.array_equal(r["accepted"], trace)
    if exact:
        assert np.array_equal(r["logw"], lw)
    else:
        assert np.allclose(r["logw"], lw, rtol=1e-9, atol=0.0)


def _same_chains(a, b):
    for k in ("z", "v", "accepted", "final_step", "accepts"):
        assert np.array_equal(a[k], b[k]), k


def test_default_equals_exact_order(capi, setups, monkeypatch):
    """The default path's decisions are certified: z, accepted, final_step and accepts are
    those of LGS_EXACT_ORDER, each draw's weight is within its bound of the exact one, and
    logw is within the final draw's bound.  With the bounds widened by the hooks library
    (still bounds) decisions go through the reference-order recomputation and nothing but
    logw -- then the reference-order value itself where it was recomputed -- may move."""
    s = setups["qary128"]
    T, n_steps = s["T"], 31
    n = T.shape[0]
    ctx = _context(capi, s)
    ex = ctx.imhk_targets_host(SEED, 0, T, n_steps, want_trace=True, flags=capi.LGS_EXACT_ORDER)
    assert not ex["bound_draws"].any()
    de = ctx.imhk_targets_host(SEED, 0, T, n_steps, want_trace=True)
    _same_chains(de, ex)
    err = np.abs(de["logw_draws"] - ex["logw_draws"])
    print(f"  max |logw_draws - exact| {err.max():.3e}, bounds {de['bound_draws'].min():.3e} .. "
          f"{de['bound_draws'].max():.3e}, {ctx.counter(capi.LGS_COUNTER_ACCEPT_RESOLVED)} decisions redone")
    assert (err <= de["bound_draws"]).all()
    fin = de["bound_draws"][np.arange(n), de["final_step"]]
    assert (np.abs(de["logw"] - ex["logw"]) <= fin).all()
    assert ctx.counter(capi.LGS_COUNTER_WL_MISMATCH) == 0
    redone = {}
    for scale in BOUND_SCALES:
        monkeypatch.setenv("LGS_TEST_WL_BOUND_SCALE", repr(scale))
        hk = _context(capi, s, hooks=True)
        hk.counter(capi.LGS_COUNTER_ACCEPT_RESOLVED, reset=True)
        r = hk.imhk_targets_host(SEED, 0, T, n_steps, want_trace=True)
        redone[scale] = hk.counter(capi.LGS_COUNTER_ACCEPT_RESOLVED)
        print(f"  bound scale {scale:g}: {redone[scale]} of {n * n_steps} decisions redone")
        _same_chains(r, ex)
        assert np.array_equal(r["logw_draws"], de["logw_draws"]) and np.array_equal(r["bound_draws"], de["bound_draws"])
        assert (np.abs(r["logw"] - ex["logw"]) <= fin).all()
        assert hk.counter(capi.LGS_COUNTER_WL_MISMATCH) == 0
    assert redone[BOUND_SCALES[-1]] > 0


def test_widened_certificate_keeps_the_chains(capi, setups, monkeypatch):
    """LGS_TEST_Z1CAP_SCALE widens every certificate bound (as in lgs_klein_decode): the
    draws' decisions go through the reference-order path, whose Wang-Ling term is added at
    the reference-order mean, and the chains must not change."""
    s = setups["qary128"]
    T = s["T"][:130]
    ex = _context(capi, s).imhk_targets_host(SEED, 9, T, 31, want_trace=True, flags=capi.LGS_EXACT_ORDER)
    monkeypatch.setenv("LGS_TEST_Z1CAP_SCALE", "1e-9")
    hk = _context(capi, s, hooks=True)
    hk.resolved(reset=True)
    r = hk.imhk_targets_host(SEED, 9, T, 31, want_trace=True)
    print(f"  {hk.resolved()} coordinate decisions redone in the reference's order")
    assert hk.resolved() > T.shape[0]
    _same_chains(r, ex)
    assert (np.abs(r["logw_draws"] - ex["logw_draws"]) <= r["bound_draws"]).all()
    assert hk.counter(capi.LGS_COUNTER_WL_MISMATCH) == 0


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_chunking_splits_and_prefixes(capi, setups, exact):
    s = setups["qary40"]
    f = capi.LGS_EXACT_ORDER if exact else 0
    T = s["T"][:100]
    keys = ("z", "v", "cprime", "logw", "accepts", "final_step", "accepted", "logw_draws", "bound_draws")
    one = _context(capi, s).imhk_targets_host(SEED, 0, T, 31, want_cprime=True, want_trace=True, flags=f)
    ctx = _context(capi, s, max_proposals=256)  # 8 chains of 32 draws per chunk: 13 chunks
    r = ctx.imhk_targets_host(SEED, 0, T, 31, want_cprime=True, want_trace=True, flags=f)
    for k in keys:
        assert np.array_equal(r[k], one[k]), k
    a = ctx.imhk_targets_host(SEED, 0, T[:40], 31, want_cprime=True, want_trace=True, flags=f)
    b = ctx.imhk_targets_host(SEED, 40, T[40:], 31, want_cprime=True, want_trace=True, flags=f)
    for k in keys:
        assert np.array_equal(r[k], np.concatenate([a[k], b[k]])), k
    short = ctx.imhk_targets_host(SEED, 0, T, 15, want_trace=True, flags=f)  # 16 chains per chunk
    assert np.array_equal(r["accepted"][:, :15], short["accepted"])
    assert np.array_equal(r["logw_draws"][:, :16], short["logw_draws"])
    assert np.array_equal(short["accepts"], short["accepted"].sum(axis=1))


@pytest.mark.parametrize("name", ["qary40", "ntru64"])
def test_device_pointers_coordinate_major(capi, setups, name):
    import torch
    s = setups[name]
    n, d, n_steps = 130, s["d"], 31
    T = s["T"][:n]
    ctx = _context(capi, s)
    host = ctx.imhk_targets_host(SEED, 21, T, n_steps, want_cprime=True, want_trace=True, flags=capi.LGS_Z64)
    f = capi.LGS_DEVICE_PTRS | capi.LGS_COORD_MAJOR | capi.LGS_Z64

    def dev(shape, dtype):
        return torch.empty(shape, dtype=dtype, device="cuda")
    t = torch.as_tensor(np.ascontiguousarray(T.T), device="cuda")
    z, v, cp = dev((d, n), torch.int64), dev((n, d), torch.float64), dev((n, d), torch.float64)
    out = dict(logw=dev(n, torch.float64), accepts=dev(n, torch.int64), final_step=dev(n, torch.int64),
               accepted=dev((n, n_steps), torch.uint8), logw_draws=dev((n, n_steps + 1), torch.float64),
               bound_draws=dev((n, n_steps + 1), torch.float64))
    ctx.imhk_targets(SEED, 21, t, n_steps, z, v, cp, flags=f, **out)
    torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy().T, host["z"])
    assert np.array_equal(v.cpu().numpy(), host["v"])
    assert np.array_equal(cp.cpu().numpy(), host["cprime"])
    for k, a in out.items():
        assert np.array_equal(a.cpu().numpy(), host[k]), k
    # the Q frame, coordinate-major on the device: c' taken verbatim; every output optional
    z2 = torch.empty_like(z)
    ctx.imhk_targets(SEED, 21, cp.T.contiguous(), n_steps, z2, flags=f | capi.LGS_TARGETS_QFRAME)
    torch.cuda.synchronize()
    assert torch.equal(z2, z)


def test_errors(capi, setups):
    s = setups["qary40"]
    d = s["d"]
    T = np.array(s["T"][:10])
    ctx = capi.Context(0, max_proposals=4096)
    ctx.set_basis(s["R"], np.zeros(d), None, s["sigma"])
    z = np.empty((10, d), dtype=np.int32)

    def code(*a, **kw):
        with pytest.raises(capi.LgsError) as e:
            ctx.imhk_targets(*a, **kw)
        return e.value.code
    assert code(SEED, 0, T, 4, z) == capi.LGS_ERR_STATE  # lattice frame without Q
    ctx.imhk_targets(SEED, 0, T, 4, z, flags=capi.LGS_TARGETS_QFRAME)  # needs no Q
    ctx.imhk_targets(SEED, 0, T[:0], 4)  # n == 0
    ctx.set_decoder(Q=s["Q"])
    assert code(SEED, 0, T, 4, z, np.empty((10, d))) == capi.LGS_ERR_STATE  # v_out without B
    ctx.set_basis(s["R"], np.zeros(d), s["B"], s["sigma"])
    ctx.set_decoder(Q=s["Q"])
    for f in (capi.LGS_WANG_LING, capi.LGS_LOGW_BOUND, capi.LGS_SAMPLEZ_TABLE):
        assert code(SEED, 0, T, 4, z, flags=f) == capi.LGS_ERR_INVALID
    assert code(SEED, 0, T, -1, z) == capi.LGS_ERR_INVALID
    assert code(SEED, 0, T, 4096, z) == capi.LGS_ERR_INVALID  # n_steps < max_proposals
    ctx.imhk_targets(SEED, 0, T[:1], 4095, z[:1])  # one chain fills the launch
    assert code(SEED, 2 ** 32 - 9, T, 4, z) == capi.LGS_ERR_INVALID  # the chain counter has 32 bits
    assert code(SEED, 2 ** 32 + 1, T[:0], 4) == capi.LGS_ERR_INVALID
    last = np.empty((10, d), dtype=np.int32)
    ctx.imhk_targets(SEED, 2 ** 32 - 10, T, 4, last)  # chains up to 2^32 - 1
    for f in (0, capi.LGS_EXACT_ORDER, capi.LGS_TARGETS_QFRAME):
        bad = T.copy()
        bad[4, 7] = np.nan
        assert code(SEED, 0, bad, 4, z, flags=f) == capi.LGS_ERR_NONFINITE
    ctx.imhk_targets(SEED, 0, T, 4, z)  # the context is usable after an error
    # |z| >= 2^31: int32 buffers overflow, int64 succeed
    s = setups["int12"]
    ctx = _context(capi, s)
    T = s["T"][:70] * 1e9
    z32 = np.empty((70, s["d"]), dtype=np.int32)
    for f in (0, capi.LGS_EXACT_ORDER):
        with pytest.raises(capi.LgsError) as e:
            ctx.imhk_targets(SEED, 0, T, 6, z32, flags=f)
        assert e.value.code == capi.LGS_ERR_OVERFLOW
    z64 = np.empty((70, s["d"]), dtype=np.int64)
    ctx.imhk_targets(SEED, 0, T, 6, z64, flags=capi.LGS_Z64)
    assert np.abs(z64).max() >= 2 ** 31
    assert np.array_equal(ctx.imhk_targets_host(SEED, 0, T, 6, want_v=False)["z"], z64)  # int64 on overflow


def test_exact_where_klein_is_biased(capi, oracle, setups):
    """B = [[4,1],[1,3]] at sigma = 0.8, below the smoothing bound, 2^14 chains on the one
    target (1.7, -0.6), seed 7: against the exact D_{Lambda,sigma,t} (enumerated over
    z in [-12,12]^2) Klein's draws are 0.218 away in total variation and the states after 32
    steps 0.0035 (2^14 exact samples: 0.003-0.005), acceptance 0.787 -- the oracle's figures,
    and the library reproduces the oracle's integers."""
    s = setups["d2"]
    sigma, t, n = 0.8, np.array([1.7, -0.6]), 1 << 14
    ctx = _context(capi, s, sigma=sigma)
    T = np.tile(t, (n, 1))
    zz, p = d2_exact_pmf(s["B"], sigma, t)
    r0 = ctx.imhk_targets_host(7, 0, T, 0, want_cprime=True)
    r32 = ctx.imhk_targets_host(7, 0, T, 32)
    cp = r0["cprime"][0]
    assert (r0["cprime"] == cp).all()
    o0, _, _ = oracle.imhk_parallel(s["R"], cp, s["B"], sigma, n, 0, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    o32, _, oa = oracle.imhk_parallel(s["R"], cp, s["B"], sigma, n, 32, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    tv0, tv32 = tv_distance(r0["z"], zz, p), tv_distance(r32["z"], zz, p)
    rate = r32["accepts"].sum() / (32.0 * n)
    print(f"  TV(Klein) {tv0:.4f}, TV(32 steps) {tv32:.4f}, acceptance {rate:.3f}")
    assert np.array_equal(r0["z"], o0) and np.array_equal(r32["z"], o32) and np.array_equal(r32["accepts"], oa)
    assert tv32 <= 0.02
    assert tv0 >= 0.15
    assert 0.7 <= rate <= 0.9


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_sampler_sample_around(setups, exact):
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import IMHKSampler
    s = setups["qary40"]
    lat = SimpleLattice(s["B"])
    T = s["T"][:130]
    smp = IMHKSampler(lat, s["sigma"], seed=11, burn_in=0, wang_ling=True, exact_order=exact, chain_id=3)
    own = smp.sample(5)  # the sampler's own chain 3, steps 1..5
    pts, z = smp.sample_around(T, 31, coefficients=True)  # chains 4..133
    ctx, f = smp.context, smp.proposal_sampler._flags()
    ref = ctx.imhk_targets_host(11, 4, T, 31, flags=f)
    assert pts.shape == (130, s["d"]) and z.shape == (130, s["d"])
    assert np.array_equal(pts, ref["v"]) and np.array_equal(z, ref["z"])
    assert np.array_equal(pts, z.astype(np.float64) @ s["B"].T)
    assert smp.stats.acceptance_rate == ref["accepts"].sum() / (130 * 31)
    one = smp.sample_around(T[0], 31)  # chain 134
    assert one.shape == (s["d"],)
    assert np.array_equal(one, ctx.imhk_targets_host(11, 134, T[:1], 31, flags=f)["v"][0])
    assert not np.array_equal(one, pts[0])  # the same target on another chain
    assert np.array_equal(smp.sample_around(T[:2], 31, first_chain=4), pts[:2])
    own2 = smp.sample(5)  # steps 6..10 of chain 3, as if nothing had happened in between
    fresh = IMHKSampler(lat, s["sigma"], seed=11, burn_in=0, wang_ling=True, exact_order=exact, chain_id=3)
    assert np.array_equal(np.concatenate([own, own2]), fresh.sample(10))
