"""Exact Gaussian mass by fixed-radius enumeration (lgs_gaussian_mass, Decoder.gaussian_mass,
SimpleLattice.gaussian_mass, IMHKSampler.compute_delta(exact=True)) against the CPU oracle of
tests/mass_oracle.py.

The oracle is the operational definition of include/lgs.h in Python floats, run on the c' the
library reports having used (cprime_out): points, nodes, status and dist2_min compare bit for
bit; mass, energy and sum_z, which are defined up to the order of summation, within the
tolerances derived in mass_oracle.tolerances.  tests/test_mass_host.py holds the premises: the
oracle equals brute force at d = 2, 3, and the host's split emits the oracle's prefixes.

Cases (nodes and points per target from the oracle): A int12, sigma 12, 12 nats: 8 633 to
10 082 nodes, 1 070 to 1 249 points for the first three targets (3 114 to 19 297 nodes, 293 to
2 968 points over the first 130); B int12, sigma 16, 12 nats: about 75 000 nodes (beyond
one launch slice of 2^16); C gauss16, sigma 9, 12 nats: about 118 000 nodes, a real basis."""
import math

import numpy as np
import pytest

import cvp_oracle
import mass_oracle

pytestmark = pytest.mark.gpu

MAX_NODES = 1 << 22
NATS = 12.0
CASES = {"d2": ("d2", 0.8), "d3": ("d3", 1.1), "A": ("int12", 12.0), "B": ("int12", 16.0), "C": ("gauss16", 9.0)}
INT_KEYS = ("points", "nodes", "status", "dist2_min")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def setups():
    return {name: cvp_oracle.setup(name) for name in ("d2", "d3", "int12", "gauss16")}


_ORACLE = {}  # shared by every test, never modified


def _oracle(s, cp, sigma, radius2, shift, max_nodes=MAX_NODES):
    key = (s["name"], cp.tobytes(), float(sigma), float(radius2), float(shift), max_nodes)
    if key not in _ORACLE:
        _ORACLE[key] = mass_oracle.enum(s["R"], cp, sigma, radius2, shift, max_nodes=max_nodes)
    return _ORACLE[key]


def _context(capi, s, decoder=True, **kw):
    ctx = capi.Context(0, **kw)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], 1.0)
    if decoder:
        ctx.set_decoder(Q=s["Q"])
    return ctx


_BALLS = {}


def _ball(capi, s, n, sigma, nats=NATS):
    """(radius2, shift) = (D_min + 2 sigma^2 nats, D_min) of the first n targets, D_min from
    lgs_closest_vector (tests/test_gpu_cvp.py checks it against its oracle)."""
    key = (s["name"], float(sigma), float(nats))
    if key not in _BALLS or len(_BALLS[key][0]) < n:
        cv = _context(capi, s).closest_vector_host(s["T"][:max(n, 3)], 1 << 20, want_z=False, want_v=False)
        assert not cv["status"].any()
        D = cv["dist2"]
        r2 = D + 2.0 * sigma * sigma * nats
        for a in (r2, D):
            a.setflags(write=False)
        _BALLS[key] = (r2, D)
    r2, D = _BALLS[key]
    return r2[:n], D[:n]


def _run(capi, ctx, T, sigma, radius2, shift, max_nodes=MAX_NODES, mode="host", moments=True, flags=0):
    """The raw call in one of the layouts: host row-major, host coordinate-major, device
    tensors.  Every output comes back as a host array."""
    n, d = T.shape
    cm = mode == "coordmajor"
    f = flags | (capi.LGS_COORD_MAJOR if cm else 0)
    t = np.ascontiguousarray(T.T if cm else T)
    out = {"cprime": np.full((n, d), np.nan), "mass": np.full(n, np.nan), "energy": np.full(n, np.nan),
           "points": np.full(n, -1, dtype=np.int64), "dist2_min": np.full(n, np.nan),
           "sum_z": np.full((n, d), np.nan) if moments else None, "nodes": np.full(n, -1, dtype=np.int64),
           "status": np.full(n, -1, dtype=np.int32)}
    r2 = np.ascontiguousarray(radius2, dtype=np.float64)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    if mode == "device":
        import torch
        dev = torch.device("cuda:0")
        f |= capi.LGS_DEVICE_PTRS
        up = lambda a: None if a is None else torch.as_tensor(a.copy(), device=dev)  # noqa: E731
        t, r2, sh = up(t), up(r2), up(sh)
        bufs = {k: up(v) for k, v in out.items()}
    else:
        bufs = out
    ctx.gaussian_mass(t, sigma, r2, sh, max_nodes, bufs["cprime"], bufs["mass"], bufs["energy"], bufs["points"],
                      bufs["dist2_min"], bufs["sum_z"], bufs["nodes"], bufs["status"], f)
    if mode == "device":
        out = {k: None if v is None else v.cpu().numpy() for k, v in bufs.items()}
    return out


def _check_cprime(s, T, cp):
    ref = T @ s["Q"]
    bound = 2.02 * (s["d"] + 2) * 2.0 ** -53 * (np.abs(T) @ np.abs(s["Q"]))
    assert (np.abs(cp - ref) <= bound).all()


def _check_against_oracle(s, r, sigma, radius2, shift, max_nodes=MAX_NODES, status=0):
    """Integers and dist2_min bit for bit, sums within the derived tolerances; returns the
    largest |difference| / tolerance."""
    n = len(r["mass"])
    bad, worst = [], 0.0
    for k in range(n):
        o = _oracle(s, r["cprime"][k], sigma, radius2[k], 0.0 if shift is None else shift[k], max_nodes)
        same = all(np.array_equal(r[key][k], o[key]) for key in INT_KEYS) and o["status"] == status
        if not same:
            bad.append((k, [(r[key][k], o[key]) for key in INT_KEYS]))
            continue
        got = {"mass": r["mass"][k], "energy": r["energy"][k],
               "sum_z": None if r["sum_z"] is None else r["sum_z"][k]}
        worst = max(worst, mass_oracle.close(got, o, o["points"]))
    assert not bad, f"{len(bad)} of {n} targets differ from the oracle (k, (got, want) per output): {bad[:3]}"
    assert worst <= 1.0, f"a sum is {worst:.2f} times its tolerance away from the oracle's"
    return worst


def _same_integers(a, b):
    for k in INT_KEYS + ("cprime",):
        assert np.array_equal(a[k], b[k]), k


def _sums_agree(s, a, b, sigma, radius2, shift):
    """Two runs of the same targets agree pairwise within the derived tolerances: the bound
    covers two sums of the same N terms in any two orders."""
    for k in range(len(a["mass"])):
        o = _oracle(s, a["cprime"][k], sigma, radius2[k], shift[k])
        tm, te, tz = mass_oracle.tolerances(o["points"], o["mass"], o["energy"], o["abs_z"])
        assert abs(a["mass"][k] - b["mass"][k]) <= tm and abs(a["energy"][k] - b["energy"][k]) <= te
        if a["sum_z"] is not None and b["sum_z"] is not None:
            assert (np.abs(a["sum_z"][k] - b["sum_z"][k]) <= np.array(tz)).all()


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("mode,moments,qframe", [("host", True, False), ("coordmajor", False, False),
                                                 ("device", True, False), ("host", False, True),
                                                 ("device", False, True), ("coordmajor", True, True)],
                         ids=["host-sumz", "coordmajor", "device-sumz", "qframe", "device-qframe",
                              "coordmajor-qframe-sumz"])
@pytest.mark.parametrize("case", ["d2", "d3", "A"])
def test_oracle_parity(capi, setups, case, mode, moments, qframe):
    """n = 1, 63, 64, 130: a partly filled wave, a whole wave, two waves and two lanes.  The
    product library splits these trees as it would for a user."""
    name, sigma = CASES[case]
    s = setups[name]
    ctx = _context(capi, s)
    for n in (1, 63, 64, 130):
        T = s["T"][:n]
        r2, D = _ball(capi, s, 130, sigma)
        r2, D = r2[:n], D[:n]
        if qframe:  # c' itself, as a lattice-frame call reports it
            cp = _run(capi, ctx, T, sigma, r2, D, moments=False)["cprime"]
            r = _run(capi, ctx, cp, sigma, r2, D, mode=mode, moments=moments, flags=capi.LGS_TARGETS_QFRAME)
            assert np.array_equal(r["cprime"], cp)
        else:
            r = _run(capi, ctx, T, sigma, r2, D, mode=mode, moments=moments)
            _check_cprime(s, T, r["cprime"])
        worst = _check_against_oracle(s, r, sigma, r2, D)
        assert np.array_equal(r["dist2_min"], D)  # the closest point is the ball's nearest
        print(f"  {case} n={n}: nodes {int(r['nodes'].min())}..{int(r['nodes'].max())}, points "
              f"{int(r['points'].min())}..{int(r['points'].max())}, difference / tolerance {worst:.3f}")


@pytest.mark.parametrize("mode,moments", [("host", True), ("device", False)], ids=["host-sumz", "device"])
@pytest.mark.parametrize("case", ["B", "C"])
def test_oracle_parity_deep(capi, setups, case, mode, moments):
    name, sigma = CASES[case]
    s = setups[name]
    T = s["T"][:2]
    r2, D = _ball(capi, s, 2, sigma)
    r = _run(capi, _context(capi, s), T, sigma, r2, D, mode=mode, moments=moments)
    _check_cprime(s, T, r["cprime"])
    worst = _check_against_oracle(s, r, sigma, r2, D)
    assert (r["nodes"] > 1 << 16).all()
    print(f"  {case}: nodes {r['nodes'].tolist()}, points {r['points'].tolist()}, difference / tolerance {worst:.3f}")


def test_no_shift_and_far_targets(capi, setups):
    """shift = NULL is 0; at these distances (D_min ~ 10^2 .. 10^3 at sigma = 12) the unshifted
    weights are small but representable, and shift = D_min only rescales them."""
    s = setups["int12"]
    T = s["T"][:5]
    r2, D = _ball(capi, s, 5, 12.0)
    ctx = _context(capi, s)
    plain = _run(capi, ctx, T, 12.0, r2, None)
    _check_against_oracle(s, plain, 12.0, r2, None)
    shifted = _run(capi, ctx, T, 12.0, r2, D)
    _same_integers(plain, shifted)
    assert np.allclose(np.log(plain["mass"]), np.log(shifted["mass"]) - D / 288.0, rtol=0, atol=1e-9)


# ------------------------------------------------------------------ 2. split invariance
def test_split_depth_does_not_change_the_result(capi, setups, monkeypatch):
    s = setups["int12"]
    sigma = 12.0
    T = s["T"][:3]
    r2, D = _ball(capi, s, 3, sigma)
    runs = {}
    for k in ("0", "1", "2", "5", "11", None):
        if k is None:
            monkeypatch.delenv("LGS_TEST_MASS_SPLIT", raising=False)
        else:
            monkeypatch.setenv("LGS_TEST_MASS_SPLIT", k)
        runs[k] = _run(capi, _context(capi, s, hooks=True), T, sigma, r2, D)
        _check_against_oracle(s, runs[k], sigma, r2, D)
    runs["product"] = _run(capi, _context(capi, s), T, sigma, r2, D)
    keys = list(runs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            _same_integers(runs[a], runs[b])
            _sums_agree(s, runs[a], runs[b], sigma, r2, D)
    for k in ("mass", "energy", "sum_z"):  # the hooks library without a switch is the product library
        assert np.array_equal(runs[None][k], runs["product"][k]), k


def test_one_target_is_split_by_default(capi, setups, monkeypatch):
    """At 64 nodes per launch an unsplit tree of m nodes takes ceil(m / 64) launches one after
    another; the default split hands the same nodes to many lanes."""
    s = setups["int12"]
    sigma = 12.0
    T = s["T"][:1]
    r2, D = _ball(capi, s, 1, sigma)
    monkeypatch.setenv("LGS_TEST_CVP_SLICE", "64")
    launches = {}
    for k in ("0", None):
        if k is not None:
            monkeypatch.setenv("LGS_TEST_MASS_SPLIT", k)
        else:
            monkeypatch.delenv("LGS_TEST_MASS_SPLIT", raising=False)
        ctx = _context(capi, s, hooks=True)
        ctx.timing_enable(True)
        r = _run(capi, ctx, T, sigma, r2, D)
        _check_against_oracle(s, r, sigma, r2, D)
        launches[k] = ctx.timing_get(capi.KERNEL_CVP_ENUM)[1]
        assert ctx.timing_get(capi.KERNEL_CPRIME)[1] == 1
    need = -(-int(r["nodes"][0]) // 64)
    print(f"  enumeration launches: {launches['0']} unsplit ({need} needed), {launches[None]} with the default split")
    assert need <= launches["0"] <= need + 1
    assert launches[None] * 8 <= launches["0"]


# ------------------------------------------------------------------ 3. suspend and resume
@pytest.mark.parametrize("split", ["0", None], ids=["unsplit", "default"])
def test_slices_slots_and_chunks(capi, setups, monkeypatch, split):
    """Case A, 130 targets, 64 nodes per launch, 64 lanes, chunks of 64 targets: every item is
    suspended and resumed, items wait for a lane, unfinished ones are compacted."""
    s = setups["int12"]
    sigma = 12.0
    T = s["T"][:130]
    r2, D = _ball(capi, s, 130, sigma)
    want = _run(capi, _context(capi, s), T, sigma, r2, D)
    _check_against_oracle(s, want, sigma, r2, D)
    monkeypatch.setenv("LGS_TEST_CVP_SLICE", "64")
    monkeypatch.setenv("LGS_TEST_CVP_SLOTS", "64")
    if split is not None:
        monkeypatch.setenv("LGS_TEST_MASS_SPLIT", split)
    ctx = _context(capi, s, hooks=True, max_proposals=64)
    ctx.timing_enable(True)
    got = _run(capi, ctx, T, sigma, r2, D)
    _same_integers(got, want)
    _check_against_oracle(s, got, sigma, r2, D)
    assert ctx.timing_get(capi.KERNEL_CPRIME)[1] == 3  # three chunks
    assert ctx.timing_get(capi.KERNEL_CVP_ENUM)[1] > 3
    # more lanes than a wave, 1000 nodes per launch: the compaction of unfinished items runs
    monkeypatch.setenv("LGS_TEST_CVP_SLICE", "1000")
    monkeypatch.setenv("LGS_TEST_CVP_SLOTS", "4096")
    ctx = _context(capi, s, hooks=True)
    ctx.timing_enable(True)
    got = _run(capi, ctx, T, sigma, r2, D, mode="device")
    _same_integers(got, want)
    _check_against_oracle(s, got, sigma, r2, D)
    if split == "0":
        assert ctx.timing_get(capi.KERNEL_DECODE_SELECT)[1] >= 1  # a compaction ran


# ------------------------------------------------------------------ 4. budget
def test_budget(capi, setups, monkeypatch):
    s = setups["int12"]
    sigma = 16.0
    T = s["T"][:2]
    r2, D = _ball(capi, s, 2, sigma)
    full = _run(capi, _context(capi, s), T, sigma, r2, D)
    _check_against_oracle(s, full, sigma, r2, D)
    monkeypatch.setenv("LGS_TEST_MASS_SPLIT", "0")
    unsplit = _run(capi, _context(capi, s, hooks=True), T, sigma, r2, D, max_nodes=10000)
    _check_against_oracle(s, unsplit, sigma, r2, D, max_nodes=10000, status=1)  # the unsplit search is the oracle's
    monkeypatch.delenv("LGS_TEST_MASS_SPLIT", raising=False)
    for cut in (unsplit, _run(capi, _context(capi, s), T, sigma, r2, D, max_nodes=10000)):
        assert (cut["status"] == 1).all() and (cut["nodes"] == 10000).all()
        assert (cut["mass"] <= full["mass"]).all() and (cut["points"] <= full["points"]).all()
        assert (cut["energy"] <= full["energy"]).all() and (cut["dist2_min"] >= full["dist2_min"]).all()
    # a budget of exactly the traversal's node count is enough
    for k in range(2):
        exact = int(full["nodes"][k])
        for ctx in (_context(capi, s), _context(capi, s, hooks=True)):  # (the second one unsplit)
            monkeypatch.setenv("LGS_TEST_MASS_SPLIT", "0")
            r = _run(capi, ctx, T[k:k + 1], sigma, r2[k:k + 1], D[k:k + 1], max_nodes=exact)
            assert r["status"][0] == 0 and r["nodes"][0] == exact and r["points"][0] == full["points"][k]
            r = _run(capi, ctx, T[k:k + 1], sigma, r2[k:k + 1], D[k:k + 1], max_nodes=exact - 1)
            assert r["status"][0] == 1 and r["nodes"][0] == exact - 1


# ------------------------------------------------------------------ 5. sigma is an argument
def test_sigma_is_an_argument(capi, setups):
    s = setups["int12"]
    T = s["T"][:5]
    r2, D = _ball(capi, s, 5, 12.0)
    ctx = _context(capi, s)
    a = _run(capi, ctx, T, 12.0, r2, D)
    b = _run(capi, ctx, T, 7.5, r2, D)  # no lgs_set_basis in between
    for sigma, got in ((12.0, a), (7.5, b)):
        fresh = _run(capi, _context(capi, s), T, sigma, r2, D)
        for k in got:
            assert np.array_equal(got[k], fresh[k]), k
        _check_against_oracle(s, got, sigma, r2, D)
    assert (b["mass"] < a["mass"]).all() and np.array_equal(a["points"], b["points"])


# ------------------------------------------------------------------ 6. errors
def _raw(capi, ctx, T, sigma, radius2, max_nodes=1000, flags=0, sum_z=False, shift=None):
    n, d = T.shape
    mass = np.zeros(n)
    sz = np.zeros((n, d)) if sum_z else None
    r2 = None if radius2 is None else np.ascontiguousarray(radius2, dtype=np.float64)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    return ctx._L.lgs_gaussian_mass(ctx._h, n, capi._ptr(np.ascontiguousarray(T)), float(sigma), capi._ptr(r2),
                                    capi._ptr(sh), max_nodes, None, capi._outputs(capi.MassOutputs, mass, None, None,
                                                                                 None, sz, None, None), flags)


def test_non_finite_target_in_an_unsplit_tree(capi, setups, monkeypatch):
    """With whole trees the lane, not the host's walk, meets the target."""
    s = setups["int12"]
    T = s["T"][:70].copy()
    r2, D = _ball(capi, s, 70, 12.0)
    monkeypatch.setenv("LGS_TEST_MASS_SPLIT", "0")
    ctx = _context(capi, s, hooks=True)
    want = _run(capi, ctx, T, 12.0, r2, D)
    T[66, 5] = np.nan
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, T, 12.0, r2, D)
    assert e.value.code == capi.LGS_ERR_NONFINITE
    T[66] = s["T"][66]
    got = _run(capi, ctx, T, 12.0, r2, D)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_errors_leave_the_context_usable(capi, setups):
    s = setups["int12"]
    T = s["T"][:70]
    r2, D = _ball(capi, s, 70, 12.0)
    ctx = _context(capi, s)
    want = _run(capi, ctx, T, 12.0, r2, D)

    def still_works():
        got = _run(capi, ctx, T, 12.0, r2, D)
        for k in want:
            assert np.array_equal(got[k], want[k]), k

    INVALID = capi.LGS_ERR_INVALID
    assert _raw(capi, ctx, T, 12.0, None) == INVALID
    for bad_r in (-1.0, np.nan, np.inf):
        r = r2.copy()
        r[69] = bad_r
        assert _raw(capi, ctx, T, 12.0, r) == INVALID
    for bad_sigma in (0.0, -3.0, np.nan, np.inf):
        assert _raw(capi, ctx, T, bad_sigma, r2) == INVALID
    sh = D.copy()
    sh[3] = np.nan
    assert _raw(capi, ctx, T, 12.0, r2, shift=sh) == INVALID
    for flags in (capi.LGS_Z64, capi.LGS_EXACT_ORDER, capi.LGS_WANG_LING, 0x1000):
        assert _raw(capi, ctx, T, 12.0, r2, flags=flags) == INVALID
    for max_nodes in (0, -5, (1 << 40) + 1):
        assert _raw(capi, ctx, T, 12.0, r2, max_nodes=max_nodes) == INVALID
    assert _raw(capi, ctx, T[:0], 12.0, r2[:0]) == capi.LGS_OK
    still_works()
    for bad_value in (np.nan, np.inf):
        for rows in (70, 1):  # 70 targets; one target (whose tree the host walks first)
            Tb = T[:rows].copy()
            Tb[rows - 1, 5] = bad_value
            with pytest.raises(capi.LgsError) as e:
                _run(capi, ctx, Tb, 12.0, r2[:rows], D[:rows])
            assert e.value.code == capi.LGS_ERR_NONFINITE
            still_works()
    # a device radius2 is read back for its check
    import torch
    dev = torch.device("cuda:0")
    bad = r2.copy()
    bad[0] = -2.0
    with pytest.raises(capi.LgsError) as e:
        ctx.gaussian_mass(torch.as_tensor(T.copy(), device=dev), 12.0, torch.as_tensor(bad, device=dev),
                          mass=torch.empty(70, dtype=torch.float64, device=dev), flags=capi.LGS_DEVICE_PTRS)
    assert e.value.code == INVALID
    still_works()


def test_needs_the_decoder_frame_unless_qframe(capi, setups):
    s = setups["int12"]
    T = s["T"][:5]
    r2, D = _ball(capi, s, 5, 12.0)
    ctx = _context(capi, s, decoder=False)
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, T, 12.0, r2, D)
    assert e.value.code == capi.LGS_ERR_STATE
    cp = _run(capi, _context(capi, s), T, 12.0, r2, D)["cprime"]
    q = _run(capi, ctx, cp, 12.0, r2, D, flags=capi.LGS_TARGETS_QFRAME)
    assert np.array_equal(q["cprime"], cp)
    _check_against_oracle(s, q, 12.0, r2, D)


def test_dimension_limits(capi):
    def ctx_of(d):
        ctx = capi.Context(0)
        B = np.eye(d) * 3.0 + np.triu(np.ones((d, d)), 1) * 0.25
        ctx.set_basis(B, np.zeros(d), B, 1.0)  # upper triangular, positive diagonal: R = B, Q = I
        ctx.set_decoder(Q=np.eye(d))
        return ctx, B
    ctx, _ = ctx_of(65)
    assert _raw(capi, ctx, np.zeros((2, 65)), 1.0, np.ones(2)) == capi.LGS_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.gaussian_mass_host(np.zeros((2, 65)), 1.0, np.ones(2))
    ctx, B = ctx_of(41)
    T = np.random.default_rng(41).uniform(-0.4, 0.4, (3, 41))
    assert _raw(capi, ctx, T, 1.0, np.ones(3), sum_z=True) == capi.LGS_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.gaussian_mass_host(T, 1.0, np.ones(3), moments=True)
    r = ctx.gaussian_mass_host(T, 1.0, np.full(3, 12.0), max_nodes=1 << 20, want_cprime=True)  # without sum_z: fine
    s41 = dict(name="tri41", R=B, d=41)
    _check_against_oracle(s41, dict(r, sum_z=None), 1.0, np.full(3, 12.0), None, max_nodes=1 << 20)
    # the largest shapes: d = 40 with sum_z (135 680 B of LDS), d = 64 without (160 KiB)
    for d, moments in ((40, True), (64, False)):
        ctx, B = ctx_of(d)
        T = np.random.default_rng(d).uniform(-0.4, 0.4, (3, d))
        r = ctx.gaussian_mass_host(T, 1.0, np.full(3, 12.0), max_nodes=1 << 20, moments=moments, want_cprime=True)
        assert np.array_equal(r["cprime"], T) and (r["points"] >= 1).all()
        _check_against_oracle(dict(name=f"tri{d}", R=B, d=d), r, 1.0, np.full(3, 12.0), None, max_nodes=1 << 20)


# ------------------------------------------------------------------ 7. the Python surface
def test_decoder_and_simple_lattice(capi, setups):
    from lgs_amd.decode import Decoder
    from lgs_amd.lattices import SimpleLattice
    s = setups["int12"]
    sigma = 12.0
    T = s["T"][:5]
    dec = Decoder(s["B"])
    got = dec.gaussian_mass(T, sigma, nats=NATS, max_nodes=MAX_NODES, moments=True)
    D = dec.ctx.closest_vector_host(T, MAX_NODES, want_z=False, want_v=False)["dist2"]
    r2 = D + 2.0 * sigma * sigma * NATS
    raw = dec.ctx.gaussian_mass_host(T, sigma, r2, D, MAX_NODES, moments=True)
    assert np.array_equal(got["log_mass"], np.log(raw["mass"]) - D / (2.0 * sigma * sigma))
    assert np.array_equal(got["mean_z"], raw["sum_z"] / raw["mass"][:, None])
    assert np.array_equal(got["mean_dist2"], raw["energy"] / raw["mass"])
    for k in ("points", "nodes", "status"):
        assert np.array_equal(got[k], raw[k]), k
    one = dec.gaussian_mass(T[2], sigma, nats=NATS, max_nodes=MAX_NODES)
    assert one["log_mass"] == got["log_mass"][2] and one["mean_z"] is None and one["points"] == got["points"][2]
    # the mean lattice point lies near the target: B mean_z - t is small against sigma
    assert (np.abs(got["mean_z"] @ s["B"].T - T) < 3 * sigma).all()
    with pytest.raises(RuntimeError, match="closest vector"):
        dec.gaussian_mass(T, sigma, max_nodes=20)
    # SimpleLattice works on the rows of its basis: int12's column lattice is the row lattice of B^T
    lat = SimpleLattice(s["B"].T.copy())
    r = lat.gaussian_mass(sigma, center=T, nats=NATS, max_nodes=MAX_NODES)
    assert np.array_equal(r["points"], got["points"])
    assert np.allclose(r["log_mass"], got["log_mass"], rtol=0, atol=1e-9)  # (another QR frame: c' differs in the last bits)
    origin = lat.gaussian_mass(sigma, nats=NATS)
    assert origin["points"] >= 1 and origin["status"] == 0 and origin["log_mass"] >= 0.0  # the origin weighs 1


def test_compute_delta_exact(capi):
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import IMHKSampler
    B = np.array([[4.0, 1.0], [1.0, 3.0]])
    sigma, c = 0.8, np.array([1.7, -0.6])
    s = IMHKSampler(SimpleLattice(B), sigma, center=c, burn_in=0, seed=17)
    k = np.arange(-30, 31)
    Z = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    V = Z @ B.T - c
    rho = math.fsum(np.exp(-(V * V).sum(1) / (2 * sigma * sigma)).tolist())
    want = rho / math.exp(s._log_normaliser_max())
    got = s.compute_delta(exact=True)
    print(f"  delta: exact {got!r}, box sum {want!r}")
    assert abs(got / want - 1) <= 1e-12
    assert s.spectral_gap(exact=True) == got
    assert s.mixing_time(0.25, exact=True) == int(np.ceil(np.log(0.25) / np.log1p(-got)))
    # the Monte Carlo default: bounded weights, relative standard error below 1 % at 2^16 draws
    mc = s.compute_delta(1 << 16)
    print(f"  delta: Monte Carlo {mc!r}")
    assert abs(mc / got - 1) < 0.05
