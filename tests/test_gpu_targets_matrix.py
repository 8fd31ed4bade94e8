"""Every kernel of the per-target entry points against the oracle, in every context option,
at ragged d.

lgs_klein_targets, lgs_klein_decode and lgs_imhk_targets run kernels of their own
(csrc/lgs_kernels.hip): the launcher klein_targets_zt / klein_targets_any picks one from the
context's panel height (Context(panel=16): LGS_CTX_PANEL16), the store width (LGS_Z64), the
entry point's trailing lanes argument and LGS_EXACT_ORDER, and their SampleZ (decide_coord)
branches on the context's SampleZ path (Context(samplez_libm=True): a.szc is null) and on
the basis's precision and LGS_BASIS_LINEAR_PROBS.  The launch has no counter of its own; it
is a function of exactly these settings, and tests/test_targets_matrix_host.py holds the case
table (tests/targets_matrix_cases.py) against the launcher's source.  A case whose store is
z32 also asserts that no coefficient left the int32 range, so the int32 call was not rerun
with LGS_Z64 by the *_host wrapper.

Instantiations the launcher can launch, and the case that launches each (the ids read
[basis-p<panel>-<table|libm>-<z32|z64>-<default|exact>]; every basis runs every one, each
with tabulated and with libm SampleZ):

  klein_targets_kernel<int32_t, 32>               test_klein_targets_vs_oracle[*-p32-*-z32-default]
  klein_targets_kernel<int64_t, 32>               test_klein_targets_vs_oracle[*-p32-*-z64-default]
  klein_targets_kernel<int32_t, 16>               test_klein_targets_vs_oracle[*-p16-*-z32-default]
  klein_targets_kernel<int64_t, 16>               test_klein_targets_vs_oracle[*-p16-*-z64-default]
  klein_targets_kernel<int32_t, 32, DecodeLanes>  test_klein_decode_winners_and_bounds[*-p32-*-z32-default]
  klein_targets_kernel<int64_t, 32, DecodeLanes>  test_klein_decode_winners_and_bounds[*-p32-*-z64-default]
  klein_targets_kernel<int32_t, 16, DecodeLanes>  test_klein_decode_winners_and_bounds[*-p16-*-z32-default]
  klein_targets_kernel<int64_t, 16, DecodeLanes>  test_klein_decode_winners_and_bounds[*-p16-*-z64-default]
  klein_targets_kernel<int32_t, 32, WeightLanes>  test_imhk_targets_vs_oracle[*-p32-*-z32-default]
  klein_targets_kernel<int64_t, 32, WeightLanes>  test_imhk_targets_vs_oracle[*-p32-*-z64-default]
  klein_targets_kernel<int32_t, 16, WeightLanes>  test_imhk_targets_vs_oracle[*-p16-*-z32-default]
  klein_targets_kernel<int64_t, 16, WeightLanes>  test_imhk_targets_vs_oracle[*-p16-*-z64-default]
  klein_targets_exact_kernel<int32_t>             test_klein_targets_vs_oracle[*-z32-exact]
  klein_targets_exact_kernel<int64_t>             test_klein_targets_vs_oracle[*-z64-exact]
  klein_decode_exact_kernel<int32_t>              test_klein_decode_winners_and_bounds[*-z32-exact]
  klein_decode_exact_kernel<int64_t>              test_klein_decode_winners_and_bounds[*-z64-exact]
  klein_imhk_exact_kernel<int32_t>                test_imhk_targets_vs_oracle[*-z32-exact]
  klein_imhk_exact_kernel<int64_t>                test_imhk_targets_vs_oracle[*-z64-exact]

The reference-order kernels have no panels: their panel 16 cases run the same instantiation
on a context whose RP / RC are laid out for 16 rows, which they must not read.

Bases (targets_matrix_cases.BASES): q130 = qary_basis(65, 65, 3329, 3), d = 130 (32-row panels:
4 full and a 2-row bottom panel; 16-row: 8 full and 2 rows; the far-field loop runs more than
once above a ragged bottom and the packed-panel offset passes pk = 2); gauss37 (real, bottom
panel of 5 rows); qary40 (8 rows); gauss17 (real, one row below a 16-row panel); int12 (one
panel, no far field).  Oracle rows: every one for d <= 40, every 7th at d = 130.

Tolerances are the borrowed modules' own: z, accepts, accepted, final_step, best_draw, dist2
and v of integer bases exact; c' and v of real bases within 2.02 (d + 2) 2^-53 |T| |Q| resp.
|z| |B|^T (test_gpu_targets: both sides are fp64 sums of d products in some order); logw
against the oracle and tabulated against libm relative 1e-9 (test_gpu_imhk_targets); per-draw
distances and weights within the kernel's own bound of the reference-order kernel's, whose
bound is 0."""
import numpy as np
import pytest

import targets_matrix_cases as C
import test_gpu_imhk_targets as it
import test_gpu_klein_decode as kd
import test_gpu_targets as tg

pytestmark = pytest.mark.gpu

SEED = tg.SEED
assert SEED == kd.SEED == it.SEED  # the borrowed helpers draw on their module's seed


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def setups():
    s = C.make_setups()
    s["kinds"] = C.make_kinds_setup()
    return s


class _Memo:
    """The oracle with klein / imhk memoised on their arguments: the variants of a case feed
    it the same c' rows.  (R is keyed by identity: the setups outlive the memo.)"""

    def __init__(self, oracle):
        self._o, self._memo = oracle, {}
        self.IMHK_WANG_LING = oracle.IMHK_WANG_LING

    def _get(self, fn, R, cprime, rest, kw, call):
        key = (fn, id(R), np.asarray(cprime).tobytes(), rest, tuple(sorted(kw.items())))
        if key not in self._memo:
            self._memo[key] = call()
        return self._memo[key]

    def klein(self, R, cprime, sigma, n, **kw):
        return self._get("klein", R, cprime, (sigma, n), kw, lambda: self._o.klein(R, cprime, sigma, n, **kw))

    def imhk(self, R, cprime, B, sigma, n_chains, n_steps, **kw):
        return self._get("imhk", R, cprime, (sigma, n_chains, n_steps), kw,
                         lambda: self._o.imhk(R, cprime, B, sigma, n_chains, n_steps, **kw))


@pytest.fixture(scope="module")
def memo(oracle):
    return _Memo(oracle)


@pytest.fixture(scope="module")
def ctxs(capi):
    """Contexts by their options, created on first use and closed with the module."""
    made = {}

    def get(**opts):
        key = tuple(sorted(opts.items()))
        if key not in made:
            made[key] = capi.Context(0, **opts)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _load(c, s, precision=10, linear=False):
    """The setup's basis (and Q) on context c, unless it is what c holds."""
    key = (s["name"], precision, linear)
    if getattr(c, "_matrix_basis", None) != key:
        c.set_basis(s["R"], s["cp0"], s["B"], s["sigma"], precision=precision, linear_probs=linear)
        if s["Q"] is not None:
            c.set_decoder(Q=s["Q"])
        c._matrix_basis = key
    return c


def _ctx(ctxs, s, panel, samplez, **basis):
    return _load(ctxs(panel=panel, samplez_libm=samplez == "libm"), s, **basis)


def _flags(capi, store, order):
    return (capi.LGS_Z64 if store == "z64" else 0) | (capi.LGS_EXACT_ORDER if order == "exact" else 0)


def _fits_store(r, store):
    """An int32 call that overflowed would have been rerun with LGS_Z64 by the wrapper."""
    return store == "z64" or np.abs(r["z"]).max() < 2 ** 31


def _cprime_ok(s, cp, T):
    """c' = Q^T t as test_gpu_targets bounds it: both sides are fp64 sums of d products in
    some order, so they differ by at most 2.02 (d + 2) 2^-53 |T| |Q|."""
    d = s["d"]
    return (np.abs(cp - T @ s["Q"]) <= 2.02 * (d + 2) * 2.0 ** -53 * (np.abs(T) @ np.abs(s["Q"]))).all()


def _rows(n, d):
    return range(n) if d <= 40 else range(0, n, 7)


def _cross(fn):
    """The cross of one entry point, ids [basis-p<panel>-<samplez>-<store>-<order>]."""
    for mark in (pytest.mark.parametrize("name", list(C.BASES)),
                 pytest.mark.parametrize("panel,samplez,store", C.VARIANTS, ids=C.VARIANT_IDS),
                 pytest.mark.parametrize("order", C.ORDERS)):
        fn = mark(fn)
    return fn


# ------------------------------------------------------------------ 1. lgs_klein_targets
_kt_runs = {}


def _kt_run(capi, ctxs, setups, name, panel, samplez, store, order):
    """The four calls of one cell of the cross (made once, read-only)."""
    key = (name, panel, samplez, store, order)
    if key not in _kt_runs:
        s = setups[name]
        c = _ctx(ctxs, s, panel, samplez)
        out = []
        for n, first in C.N_FIRST:
            r = c.klein_targets_host(SEED, first, s["T"][:n], want_cprime=True, flags=_flags(capi, store, order))
            assert _fits_store(r, store)
            out.append(r)
        _kt_runs[key] = out
    return _kt_runs[key]


@_cross
def test_klein_targets_vs_oracle(capi, ctxs, memo, setups, name, panel, samplez, store, order):
    """z bit for bit the oracle's on the call's own c', row by row; c' and v within the bounds
    of test_gpu_targets (v exact on integer bases)."""
    s = setups[name]
    for (n, first), r in zip(C.N_FIRST, _kt_run(capi, ctxs, setups, name, panel, samplez, store, order)):
        tg._check_against_oracle(memo, s, r, s["T"][:n], first)


@pytest.mark.parametrize("store", C.STORES)
@pytest.mark.parametrize("name", list(C.BASES))
def test_klein_targets_every_variant_gives_the_same_bits(capi, ctxs, setups, name, store):
    """Every row, not only the oracle's: the default and the exact flag give the same z, the
    two panel heights the same z, v and c', and so do the two SampleZ paths."""
    want = _kt_run(capi, ctxs, setups, name, 32, "table", store, "exact")
    for panel in C.PANELS:
        for samplez in C.SAMPLEZ:
            for order in C.ORDERS:
                got = _kt_run(capi, ctxs, setups, name, panel, samplez, store, order)
                for g, w in zip(got, want):
                    for k in ("z", "v", "cprime"):
                        assert np.array_equal(g[k], w[k]), (panel, samplez, order, k)


# ------------------------------------------------------------------ 2. precision, linear probabilities
@pytest.mark.parametrize("linear", C.LINEAR, ids=["log", "linear"])
@pytest.mark.parametrize("precision", C.PRECISIONS)
@pytest.mark.parametrize("panel", C.PANELS, ids=["p32", "p16"])
@pytest.mark.parametrize("name", C.PRECISION_BASES)
def test_precision_and_linear_probs(capi, ctxs, memo, setups, name, panel, precision, linear):
    """The basis's precision and LGS_BASIS_LINEAR_PROBS reach the per-target kernels: with the
    same precision / use_log_space the oracle gives the same z (lgs_klein_targets) and the
    same chains (lgs_imhk_targets), with tabulated and libm SampleZ, default and exact."""
    s = setups[name]
    d = s["d"]
    kw = dict(precision=precision, use_log_space=not linear)
    Bo = s["B"] if s["B"] is not None else np.zeros_like(s["R"])  # (Wang-Ling weights do not read B)
    nc, n_steps, chain0 = C.PRECISION_CHAINS
    for samplez in C.SAMPLEZ:
        c = _ctx(ctxs, s, panel, samplez, precision=precision, linear=linear)
        for order in C.ORDERS:
            f = _flags(capi, "z32", order) | (capi.LGS_TARGETS_QFRAME if s["qframe"] else 0)
            for n, first in C.PRECISION_N_FIRST:
                r = c.klein_targets_host(SEED, first, s["T"][:n], want_v=False, want_cprime=True, flags=f)
                assert _fits_store(r, "z32")
                if s["qframe"]:
                    assert np.array_equal(r["cprime"], s["T"][:n])  # verbatim
                bad = [k for k in _rows(n, d)
                       if not np.array_equal(r["z"][k], memo.klein(s["R"], r["cprime"][k], s["sigma"], 1, seed=SEED,
                                                                   first_sample=first + k, **kw)["z"][0])]
                assert not bad, f"{samplez} {order} n={n}: {len(bad)} rows differ from the oracle, first {bad[:5]}"
            r = c.imhk_targets_host(SEED, chain0, s["T"][:nc], n_steps, want_v=False, want_cprime=True, flags=f)
            worst = 0.0
            for k in range(nc):
                o = memo.imhk(s["R"], r["cprime"][k], Bo, s["sigma"], 1, n_steps, seed=SEED, first_chain=chain0 + k,
                              mode=memo.IMHK_WANG_LING, **kw)
                assert np.array_equal(r["z"][k], o["z"][0]), (samplez, order, k)
                assert r["accepts"][k] == o["accepts"][0], (samplez, order, k)
                worst = max(worst, abs(r["logw"][k] - o["lw"][0]) / abs(o["lw"][0]))
            print(f"  {samplez} {order}: max rel logw err {worst:.2e}")
            assert worst <= 1e-9


# ------------------------------------------------------------------ 3. lgs_klein_decode
@_cross
def test_klein_decode_winners_and_bounds(capi, ctxs, memo, setups, name, panel, samplez, store, order):
    """best_draw, dist2 and z are those of the reference-order distance of every draw
    (check_winners on ref_dist); each draw's distance is within its bound of it, and with
    LGS_EXACT_ORDER the bounds are zero and the distances equal."""
    s = setups[name]
    c = _ctx(ctxs, s, panel, samplez)
    for n, K, first in C.decode_cases(s["d"]):
        T = s["T"][:n]
        r = c.klein_decode_host(SEED, first, T, K, want_cprime=True, want_draws=True, flags=_flags(capi, store, order))
        assert _fits_store(r, store)
        assert _cprime_ok(s, r["cprime"], T)
        zall, Dall = kd.all_draws(capi, c, s, r["cprime"], K, first, memo)
        kd.check_winners(s, r, zall, Dall)
        Dt, E = r["dist2_draws"], r["bound_draws"]
        assert Dt.shape == (n, K) and E.shape == (n, K)
        if order == "exact":
            assert np.array_equal(Dt, Dall) and not E.any()
        else:
            assert (E >= 0).all() and np.isfinite(E).all()
            assert (np.abs(Dt - Dall) <= E).all()


# ------------------------------------------------------------------ 4. lgs_imhk_targets
_it_runs = {}


def _it_run(capi, ctxs, setups, name, panel, samplez, store, order):
    key = (name, panel, samplez, store, order)
    if key not in _it_runs:
        s = setups[name]
        c = _ctx(ctxs, s, panel, samplez)
        out = []
        for n, n_steps, chain0 in C.imhk_cases(s["d"]):
            r = c.imhk_targets_host(SEED, chain0, s["T"][:n], n_steps, want_cprime=True, want_trace=True,
                                    flags=_flags(capi, store, order))
            assert _fits_store(r, store)
            out.append(r)
        assert c.counter(capi.LGS_COUNTER_WL_MISMATCH) == 0
        _it_runs[key] = out
    return _it_runs[key]


def _check_trace(memo, s, r, chain0, n_steps):
    """accepted and final_step against the oracle's states: chain k starts from the oracle's
    0-step state, and step t was accepted where the state after it differs from the one before."""
    n, d = r["z"].shape
    for k in _rows(n, d):
        kw = dict(seed=SEED, first_chain=chain0 + k, mode=memo.IMHK_WANG_LING)
        start = memo.imhk(s["R"], r["cprime"][k], s["B"], s["sigma"], 1, 0, **kw)["z"]
        o = memo.imhk(s["R"], r["cprime"][k], s["B"], s["sigma"], 1, n_steps, trace=True, **kw)
        states = np.concatenate([start, o["trace"][0]])
        moved = (states[1:] != states[:-1]).any(axis=1)
        assert moved.sum() == o["accepts"][0]  # (a condition on the oracle: no accepted draw equals its state)
        assert np.array_equal(r["accepted"][k], moved), k
        assert r["final_step"][k] == (np.flatnonzero(moved)[-1] + 1 if moved.any() else 0), k


@_cross
def test_imhk_targets_vs_oracle(capi, ctxs, memo, setups, name, panel, samplez, store, order):
    """One oracle chain per target on the call's own c': z, accepts, accepted and final_step
    equal, logw relative 1e-9, c' and v as test_gpu_targets bounds them."""
    s = setups[name]
    runs = _it_run(capi, ctxs, setups, name, panel, samplez, store, order)
    for (n, n_steps, chain0), r in zip(C.imhk_cases(s["d"]), runs):
        it._check_against_oracle(memo, s, r, s["T"][:n], chain0, n_steps)
        _check_trace(memo, s, r, chain0, n_steps)
        assert np.array_equal(r["accepts"], r["accepted"].sum(axis=1))


@pytest.mark.parametrize("store", C.STORES)
@pytest.mark.parametrize("name", list(C.BASES))
def test_imhk_targets_bounds_and_variants(capi, ctxs, setups, name, store):
    """Every chain, not only the oracle's: each variant's chains are the reference-order
    kernel's; each draw's weight is within its bound of that kernel's (whose bounds are 0);
    tabulated and libm weights agree to the relative 1e-9 of test_gpu_imhk_targets."""
    s = setups[name]
    cases = C.imhk_cases(s["d"])
    ex = {z: _it_run(capi, ctxs, setups, name, 32, z, store, "exact") for z in C.SAMPLEZ}
    worst = 0.0
    for j in range(len(cases)):
        assert not ex["table"][j]["bound_draws"].any() and not ex["libm"][j]["bound_draws"].any()
        for panel in C.PANELS:
            got = {}
            for samplez in C.SAMPLEZ:
                for order in C.ORDERS:
                    r = got[samplez, order] = _it_run(capi, ctxs, setups, name, panel, samplez, store, order)[j]
                    it._same_chains(r, ex["table"][j])
                    assert np.array_equal(r["cprime"], ex["table"][j]["cprime"])
                    err = np.abs(r["logw_draws"] - ex[samplez][j]["logw_draws"])
                    assert (err <= r["bound_draws"]).all(), (panel, samplez, order, float((err - r["bound_draws"]).max()))
                    fin = r["bound_draws"][np.arange(len(r["logw"])), r["final_step"]]
                    assert (np.abs(r["logw"] - ex[samplez][j]["logw"]) <= fin).all()
                    if order == "exact":  # the reference-order kernel does not read the panels
                        assert np.array_equal(r["logw_draws"], ex[samplez][j]["logw_draws"])
            for order in C.ORDERS:
                a, b = got["table", order]["logw"], got["libm", order]["logw"]
                worst = max(worst, float((np.abs(a - b) / np.abs(b)).max()))
                assert np.allclose(a, b, rtol=1e-9, atol=0.0), (panel, order)
    print(f"  {name}: max rel |logw tabulated - libm| = {worst:.2e}")


@pytest.mark.parametrize("order", C.ORDERS)
@pytest.mark.parametrize("panel", C.PANELS, ids=["p32", "p16"])
@pytest.mark.parametrize("name", ["qary40", "q130"])
def test_fixed_centre_gives_lgs_imhk(capi, setups, name, panel, order):
    """Every row equal to the context's c' (non-zero centre), passed in the Q frame: the
    chains of lgs_imhk_trace(LGS_WANG_LING) from uninitialised states, first_step 1."""
    s = setups[name]
    d = s["d"]
    n, n_steps, chain0 = C.FIXED_CENTRE
    cp = s["Q"].T @ np.random.default_rng(3).uniform(-4000.0, 4000.0, d)
    ctx = capi.Context(0, panel=panel)
    try:
        ctx.set_basis(s["R"], cp, s["B"], s["sigma"])
        f = _flags(capi, "z32", order)
        z = np.zeros((n, d), dtype=np.int32)
        lw, init, acc = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
        trace = np.zeros((n, n_steps), dtype=np.uint8)
        ctx.imhk(SEED, chain0, n, 1, n_steps, 1, z, lw, init, acc, flags=f | capi.LGS_WANG_LING, accepted=trace)
        r = ctx.imhk_targets_host(SEED, chain0, np.tile(cp, (n, 1)), n_steps, want_cprime=True, want_trace=True,
                                  flags=f | capi.LGS_TARGETS_QFRAME)
    finally:
        ctx.close()
    assert np.array_equal(r["cprime"], np.tile(cp, (n, 1)))  # verbatim
    assert np.array_equal(r["z"], z)
    assert np.array_equal(r["accepts"], acc)
    assert np.array_equal(r["accepted"], trace)
    if order == "exact":
        assert np.array_equal(r["logw"], lw)
    else:
        assert np.allclose(r["logw"], lw, rtol=1e-9, atol=0.0)


# ------------------------------------------------------------------ 5. forced resolution, 16-row panels
def _fresh(capi, s, **opts):
    c = capi.Context(0, **opts)
    c.set_basis(s["R"], s["cp0"], s["B"], s["sigma"])
    c.set_decoder(Q=s["Q"])
    return c


def _forced_call(capi, c, s, entry, flags=0):
    T = s["T"][:C.FORCED[entry][0]]
    if entry == "klein_targets":
        n, first = C.FORCED[entry]
        return c.klein_targets_host(SEED, first, T, flags=flags)
    if entry == "klein_decode":
        n, K, first = C.FORCED[entry]
        return c.klein_decode_host(SEED, first, T, K, want_draws=True, flags=flags)
    n, n_steps, chain0 = C.FORCED[entry]
    return c.imhk_targets_host(SEED, chain0, T, n_steps, want_trace=True, flags=flags)


@pytest.mark.parametrize("entry", list(C.FORCED))
def test_forced_resolution_panel16(capi, setups, monkeypatch, entry):
    """The hooks library widens every certificate bound by 1 / LGS_TEST_Z1CAP_SCALE (each stays
    a bound): under 16-row panels decisions, selections and accept decisions go through their
    reference-order paths, the counters grow and the outputs are those of the unwidened run."""
    s = setups["qary40"]
    n = C.FORCED[entry][0]
    plain = _fresh(capi, s, panel=16)
    try:
        want = _forced_call(capi, plain, s, entry)
        ex = _forced_call(capi, plain, s, entry, capi.LGS_EXACT_ORDER)
    finally:
        plain.close()
    monkeypatch.setenv("LGS_TEST_Z1CAP_SCALE", "1e-9")
    hk = _fresh(capi, s, panel=16, hooks=True)
    try:
        for k in (capi.LGS_COUNTER_RESOLVED, capi.LGS_COUNTER_DECODE_RESOLVED, capi.LGS_COUNTER_ACCEPT_RESOLVED):
            hk.counter(k, reset=True)
        got = _forced_call(capi, hk, s, entry)
        redone = hk.counter(capi.LGS_COUNTER_RESOLVED)
        sel = hk.counter(capi.LGS_COUNTER_DECODE_RESOLVED)
        acc = hk.counter(capi.LGS_COUNTER_ACCEPT_RESOLVED)
        mismatch = hk.counter(capi.LGS_COUNTER_WL_MISMATCH)
    finally:
        hk.close()
    print(f"  {redone} coordinate decisions, {sel} selections and {acc} accept decisions redone in the reference order")
    assert redone > 0
    if entry == "klein_targets":
        for k in ("z", "v"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["z"], ex["z"])
    elif entry == "klein_decode":
        # (a redone decision changes z_i, not how the draw's distance was formed)
        for k in ("z", "v", "best_draw", "dist2", "dist2_draws"):
            assert np.array_equal(got[k], want[k]), k
        assert (got["bound_draws"] >= want["bound_draws"]).all()
        assert (np.abs(got["dist2_draws"] - ex["dist2_draws"]) <= got["bound_draws"]).all()
        assert sel > 0
    else:
        it._same_chains(got, want)
        assert (np.abs(got["logw_draws"] - ex["logw_draws"]) <= got["bound_draws"]).all()
        fin = got["bound_draws"][np.arange(n), got["final_step"]]
        assert (np.abs(got["logw"] - ex["logw"]) <= fin).all()
        assert acc > 0
        assert mismatch == 0
