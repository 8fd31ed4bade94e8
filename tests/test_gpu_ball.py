"""The ball's points in traversal order (lgs_ball_points) against the CPU oracle of
tests/ball_oracle.py, run on the c' the library reports: z rows, D, offsets, nodes and status
compare bit for bit, whatever the split, the slices, the chunks, the pointer kind, the frame
and the coefficient width.  Bases and balls are those of tests/test_gpu_mass.py."""
import os

import numpy as np
import pytest

import ball_oracle
import cvp_oracle

pytestmark = pytest.mark.gpu

MAX_NODES = 1 << 22
NATS = 12.0
CASES = {"d2": ("d2", 0.8), "d3": ("d3", 1.1), "int12": ("int12", 12.0), "gauss16": ("gauss16", 9.0)}
HOOKS = ("LGS_TEST_MASS_SPLIT", "LGS_TEST_CVP_SLICE", "LGS_TEST_CVP_SLOTS")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def setups():
    return {name: cvp_oracle.setup(name) for name in ("d2", "d3", "int12", "gauss16")}


@pytest.fixture(autouse=True)
def _clean_env():
    saved = {k: os.environ.pop(k, None) for k in HOOKS}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


_ORACLE = {}  # shared by every test, never modified


def _oracle(s, cp, radius2, max_nodes=MAX_NODES):
    key = (s["name"], cp.tobytes(), float(radius2), max_nodes)
    if key not in _ORACLE:
        _ORACLE[key] = ball_oracle.points(s["R"], cp, radius2, max_nodes)
    return _ORACLE[key]


def _context(capi, s, **kw):
    ctx = capi.Context(0, **kw)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], 1.0)
    ctx.set_decoder(Q=s["Q"])
    return ctx


_BALLS = {}


def _ball(capi, s, n, sigma):
    key = (s["name"], float(sigma))
    if key not in _BALLS or len(_BALLS[key][0]) < n:
        cv = _context(capi, s).closest_vector_host(s["T"][:max(n, 5)], 1 << 20, want_z=False, want_v=False)
        assert not cv["status"].any()
        r2 = cv["dist2"] + 2.0 * sigma * sigma * NATS
        r2.setflags(write=False)
        _BALLS[key] = (r2, cv["dist2"])
    return _BALLS[key][0][:n], _BALLS[key][1][:n]


def _run(capi, ctx, T, radius2, capacity=None, max_nodes=MAX_NODES, device=False, z64=False, flags=0, sentinel=True):
    """The size query, then the listing call with `capacity` rows (default: the total).  Every
    output comes back as a host array; the row buffers start filled with sentinels."""
    n, d = T.shape
    f = flags | (capi.LGS_Z64 if z64 else 0)
    zdt = np.int64 if z64 else np.int32
    r2 = np.ascontiguousarray(radius2, dtype=np.float64)
    off0 = np.full(n + 1, -1, dtype=np.int64)
    ctx.ball_points(T, r2, max_nodes, 0, offsets=off0, flags=f & ~capi.LGS_DEVICE_PTRS)
    total = int(off0[n])
    cap = total if capacity is None else capacity
    out = {"z": np.full((cap, d), -77, dtype=zdt), "dist2": np.full(cap, -1.0), "cprime": np.full((n, d), np.nan),
           "offsets": np.full(n + 1, -1, dtype=np.int64), "nodes": np.full(n, -1, dtype=np.int64),
           "status": np.full(n, -1, dtype=np.int32)}
    t = T
    if device:
        import torch
        dev = torch.device("cuda:0")
        f |= capi.LGS_DEVICE_PTRS
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a).copy(), device=dev)  # noqa: E731
        t, r2 = up(T), up(r2)
        bufs = {k: up(v) for k, v in out.items()}
    else:
        bufs = out
    ctx.ball_points(t, r2, max_nodes, cap, bufs["z"] if cap else None, bufs["dist2"] if cap else None,
                    bufs["cprime"], bufs["offsets"], bufs["nodes"], bufs["status"], f)
    if device:
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
    assert np.array_equal(out["offsets"], off0)
    return out


def _check(s, r, radius2, max_nodes=MAX_NODES):
    n = len(r["nodes"])
    assert r["offsets"][0] == 0
    for k in range(n):
        z, D, nodes, st = _oracle(s, r["cprime"][k], radius2[k], max_nodes)
        a, b = r["offsets"][k], r["offsets"][k + 1]
        assert (r["nodes"][k], r["status"][k]) == (nodes, st), k
        if st:
            assert a == b
            continue
        assert b - a == len(D) and np.array_equal(r["z"][a:b], z) and np.array_equal(r["dist2"][a:b], D), k


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("case,n", [("d2", 130), ("d3", 64), ("int12", 5), ("int12", 1), ("gauss16", 1)])
@pytest.mark.parametrize("device,qframe,z64", [(False, False, False), (True, True, True), (True, False, False),
                                               (False, True, True)])
def test_rows_equal_the_oracle(capi, setups, case, n, device, qframe, z64):
    name, sigma = CASES[case]
    s = setups[name]
    r2, _ = _ball(capi, s, n, sigma)
    T = s["T"][:n]
    if qframe:
        T = np.ascontiguousarray(T @ s["Q"])
    r = _run(capi, _context(capi, s), T, r2, device=device, z64=z64,
             flags=capi.LGS_TARGETS_QFRAME if qframe else 0)
    if qframe:
        assert np.array_equal(r["cprime"], T)
    _check(s, r, r2)
    assert r["z"].dtype == (np.int64 if z64 else np.int32) and r["offsets"][n] > n


def test_int12_130_targets_against_the_counting_pass(capi, setups):
    """130 targets (more than two waves of whole trees, split into items by the host): the
    oracle on the first 5 and the last, and diff(offsets), nodes and min(D) equal
    lgs_gaussian_mass's points, nodes and dist2_min on the same call for all of them."""
    s = setups["int12"]
    n = 130
    r2, dmin = _ball(capi, s, n, 12.0)
    ctx = _context(capi, s)
    r = _run(capi, ctx, s["T"][:n], r2)
    m = ctx.gaussian_mass_host(s["T"][:n], 12.0, r2, dmin, MAX_NODES)
    assert np.array_equal(np.diff(r["offsets"]), m["points"]) and np.array_equal(r["nodes"], m["nodes"])
    assert not r["status"].any() and not m["status"].any()
    got = np.minimum.reduceat(r["dist2"], r["offsets"][:-1])
    assert np.array_equal(got, m["dist2_min"]) and np.array_equal(got, dmin)
    sub = dict(r, offsets=r["offsets"][:6], nodes=r["nodes"][:5], status=r["status"][:5])
    _check(s, sub, r2[:5])
    z, D, nodes, st = _oracle(s, r["cprime"][n - 1], r2[n - 1])
    assert np.array_equal(r["z"][r["offsets"][n - 1]:], z) and np.array_equal(r["dist2"][r["offsets"][n - 1]:], D)


# ------------------------------------------------------------------ 2. split independence
@pytest.mark.parametrize("case,n", [("int12", 5), ("gauss16", 1), ("d3", 130)])
def test_outputs_do_not_depend_on_the_split(capi, setups, case, n):
    name, sigma = CASES[case]
    s = setups[name]
    r2, _ = _ball(capi, s, n, sigma)
    T = s["T"][:n]
    base = _run(capi, _context(capi, s), T, r2)
    variants = [({"LGS_TEST_MASS_SPLIT": k}, {}) for k in ("0", "1", "3")]
    variants.append(({"LGS_TEST_CVP_SLICE": "64", "LGS_TEST_CVP_SLOTS": "64"}, {}))
    variants.append(({"LGS_TEST_MASS_SPLIT": "1", "LGS_TEST_CVP_SLICE": "64", "LGS_TEST_CVP_SLOTS": "64"}, {}))
    variants.append(({}, {"max_proposals": 64}))
    for env, kw in variants:
        for k in HOOKS:
            os.environ.pop(k, None)
        os.environ.update(env)
        r = _run(capi, _context(capi, s, hooks=True, **kw), T, r2)
        for key in base:
            assert r[key].tobytes() == base[key].tobytes(), (env, kw, key)


# ------------------------------------------------------------------ 3. capacity, budget, errors
def test_capacity(capi, setups):
    s = setups["int12"]
    n = 5
    r2, _ = _ball(capi, s, n, 12.0)
    ctx = _context(capi, s)
    full = _run(capi, ctx, s["T"][:n], r2)
    total = int(full["offsets"][n])
    assert (full["dist2"] >= 0).all()  # filled exactly: no sentinel left
    short = _run(capi, ctx, s["T"][:n], r2, capacity=total - 1)
    assert (short["z"] == -77).all() and (short["dist2"] == -1.0).all()
    for k in ("offsets", "nodes", "status"):
        assert np.array_equal(short[k], full[k])
    more = _run(capi, ctx, s["T"][:n], r2, capacity=total + 3)
    assert np.array_equal(more["z"][:total], full["z"]) and (more["z"][total:] == -77).all()
    off = np.full(n + 1, -1, dtype=np.int64)
    ctx.ball_points(s["T"][:n], np.ascontiguousarray(r2), MAX_NODES, 0, None, None, offsets=off)  # NULL buffers
    assert np.array_equal(off, full["offsets"])


def test_budget_gives_status_1_and_no_rows(capi, setups):
    s = setups["int12"]
    n = 5
    r2, _ = _ball(capi, s, n, 12.0)
    ctx = _context(capi, s)
    full = _run(capi, ctx, s["T"][:n], r2)
    budget = int(np.sort(full["nodes"])[2])  # two targets have more nodes
    r = _run(capi, ctx, s["T"][:n], r2, max_nodes=budget)
    over = full["nodes"] > budget
    assert over.sum() == 2 and np.array_equal(r["status"], over.astype(np.int32))
    assert np.array_equal(r["nodes"], np.minimum(full["nodes"], budget))
    for k in range(n):
        a, b = r["offsets"][k], r["offsets"][k + 1]
        fa, fb = full["offsets"][k], full["offsets"][k + 1]
        if over[k]:
            assert a == b
        else:
            assert np.array_equal(r["z"][a:b], full["z"][fa:fb]) and np.array_equal(r["dist2"][a:b], full["dist2"][fa:fb])
    _check(s, r, r2, budget)


def test_errors_leave_the_context_usable(capi, setups):
    s = setups["d3"]
    ctx = _context(capi, s)
    r2, _ = _ball(capi, s, 5, 1.1)
    T = s["T"][:5].copy()
    T[3, 1] = np.nan
    off = np.zeros(6, dtype=np.int64)
    with pytest.raises(capi.LgsError) as e:
        ctx.ball_points(T, np.ascontiguousarray(r2), MAX_NODES, 0, offsets=off)
    assert e.value.code == capi.LGS_ERR_NONFINITE
    _check(s, _run(capi, ctx, s["T"][:5], r2), r2)
    big = capi.Context(0)
    big.set_basis(np.eye(65), np.zeros(65), np.eye(65), 1.0)
    with pytest.raises(capi.LgsError) as e:  # (the library's own check: the binding's comes first otherwise)
        big._ck(big._L.lgs_ball_points(big._h, 1, capi._ptr(np.zeros((1, 65))), capi._ptr(np.ones(1)), 1 << 10, 0,
                                       None, None, None, None, capi.LGS_TARGETS_QFRAME))
    assert e.value.code == capi.LGS_ERR_INVALID
    big.set_basis(np.eye(3), np.zeros(3), np.eye(3), 1.0)
    off = np.zeros(2, dtype=np.int64)
    big.ball_points(np.zeros((1, 3)), np.array([1.5]), 1 << 10, 0, offsets=off, flags=capi.LGS_TARGETS_QFRAME)
    assert off[1] == 7  # the origin and the six unit vectors


def test_overflow_without_z64(capi):
    ctx = capi.Context(0)
    ctx.set_basis(np.eye(2), np.zeros(2), np.eye(2), 1.0)
    T = np.array([[2.0 ** 31 + 0.25, 0.0]])
    r2 = np.array([0.5])
    z, D = np.zeros((1, 2), dtype=np.int32), np.zeros(1)
    with pytest.raises(capi.LgsError) as e:
        ctx.ball_points(T, r2, 1 << 10, 1, z, D, flags=capi.LGS_TARGETS_QFRAME)
    assert e.value.code == capi.LGS_ERR_OVERFLOW
    r = ctx.ball_points_host(T, r2, 1 << 10, flags=capi.LGS_TARGETS_QFRAME)
    assert r["z"].tolist() == [[1 << 31, 0]] and r["dist2"][0] == 0.0625


def test_decoder_and_first_minimum(capi, setups):
    from lgs_amd.decode import Decoder
    from lgs_amd.lattices import SimpleLattice
    s = setups["int12"]
    dec = Decoder(s["B"])
    z, D = dec.ball_points(s["T"][0], sigma=12.0, nats=NATS, max_nodes=MAX_NODES)
    r2, _ = _ball(capi, s, 1, 12.0)
    flat = dec.ball_points(s["T"][:1], radius2=r2, max_nodes=MAX_NODES, flat=True)
    assert np.array_equal(z, flat["z"]) and np.array_equal(D, flat["dist2"]) and len(D) == flat["offsets"][1]
    for name in ("d2", "int12"):
        rows = setups[name]["B"].T  # SimpleLattice takes rows: the same lattice as the columns of B
        lat = SimpleLattice(rows)
        sq = float(np.min(np.sum(rows * rows, axis=1))) * (1.0 + 1e-9)
        Q, R = cvp_oracle.qr(rows.T)
        zz, DD, _, st = ball_oracle.points(R, np.zeros(len(rows)), sq)
        want = float(np.sqrt(DD[np.any(zz != 0, axis=1)].min()))
        assert st == 0 and lat.first_minimum() == want
    lat = SimpleLattice(setups["int12"]["B"].T)
    assert lat.smoothing_parameter(exact=True) >= lat.smoothing_parameter()
