"""Exact closest-vector decoding (lgs_closest_vector, Decoder.closest_vector,
SimpleLattice.decode_cvp(method="exact")) against the CPU oracle of tests/cvp_oracle.py.

The oracle is the operational definition of include/lgs.h in Python floats.  It runs on the
c' the library reports having used (cprime_out), so z, dist2, nodes and status compare bit
for bit, with no tolerance; c' itself is checked against T Q with the bound
tests/test_gpu_imhk_targets.py uses.  tests/test_cvp_host.py holds the premises: the oracle
equals brute force at d = 2, 3, and the node counts of these targets lie below the budgets
used here and on both sides of the launch slices."""
import math
import time

import numpy as np
import pytest

import cvp_oracle

pytestmark = pytest.mark.gpu

MAX_NODES = 1 << 20
SEED = 4242
NAMES = ("d2", "d3", "int12", "gauss16", "gauss20", "gauss24", "gauss37")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def setups():
    return {name: cvp_oracle.setup(name) for name in NAMES}


_ORACLE = {}  # (basis, c' bytes, max_nodes, radius2) -> (z, dist2, nodes, status), shared by every test


def _oracle(s, cp, max_nodes=MAX_NODES, radius2=math.inf):
    key = (s["name"], cp.tobytes(), max_nodes, float(radius2))
    if key not in _ORACLE:
        _ORACLE[key] = cvp_oracle.se(s["R"], cp, max_nodes=max_nodes, radius2=radius2)
    return _ORACLE[key]


def _context(capi, s, sigma=1.0, decoder=True, **kw):
    ctx = capi.Context(0, **kw)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], sigma)
    if decoder:
        ctx.set_decoder(Q=s["Q"])
    return ctx


def _run(capi, ctx, T, max_nodes=MAX_NODES, radius2=None, z64=False, cm=False, flags=0):
    """The raw call on host buffers in the layout the flags ask for; z back as (n, d) int64."""
    n, d = T.shape
    f = flags | (capi.LGS_Z64 if z64 else 0) | (capi.LGS_COORD_MAJOR if cm else 0)
    t = np.ascontiguousarray(T.T if cm else T)
    z = np.full((d, n) if cm else (n, d), -77, dtype=np.int64 if z64 else np.int32)
    v, cp = np.full((n, d), np.nan), np.full((n, d), np.nan)
    d2, nodes, status = np.full(n, np.nan), np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int32)
    r2 = None if radius2 is None else np.ascontiguousarray(radius2, dtype=np.float64)
    ctx.closest_vector(t, max_nodes, r2, z, v, cp, d2, nodes, status, f)
    return {"z": (z.T if cm else z).astype(np.int64), "v": v, "cprime": cp, "dist2": d2, "nodes": nodes,
            "status": status}


def _check_cprime(s, T, cp):
    ref = T @ s["Q"]  # c' = Q^T t: both sides are fp64 sums of d products in some order
    bound = 2.02 * (s["d"] + 2) * 2.0 ** -53 * (np.abs(T) @ np.abs(s["Q"]))
    assert (np.abs(cp - ref) <= bound).all()


def _check_v(s, r):
    zf = r["z"].astype(np.float64)
    if s["integral"]:
        assert np.array_equal(r["v"], zf @ s["B"].T)
    else:  # real basis: two fp64 sums of d products
        bound = 2.02 * (s["d"] + 2) * 2.0 ** -53 * (np.abs(zf) @ np.abs(s["B"]).T)
        assert (np.abs(r["v"] - zf @ s["B"].T) <= bound).all()


def _check_against_oracle(s, T, r, max_nodes=MAX_NODES, radius2=None, status=None):
    n = T.shape[0]
    _check_cprime(s, T, r["cprime"])
    bad = []
    for k in range(n):
        z, D, nodes, st = _oracle(s, r["cprime"][k], max_nodes, math.inf if radius2 is None else radius2[k])
        same = (np.array_equal(r["z"][k], z) and np.array_equal(r["dist2"][k], D) and r["nodes"][k] == nodes and
                r["status"][k] == st)
        if not same or (status is not None and st != status):
            bad.append((k, int(r["nodes"][k]), nodes, int(r["status"][k]), st, float(r["dist2"][k]), D))
    assert not bad, f"{len(bad)} of {n} targets differ from the oracle (k, nodes, status, dist2: got, want): {bad[:4]}"
    _check_v(s, r)


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("cm", [False, True], ids=["rowmajor", "coordmajor"])
@pytest.mark.parametrize("z64", [False, True], ids=["z32", "z64"])
@pytest.mark.parametrize("name", ["d2", "d3", "int12", "gauss16", "gauss20", "gauss24"])
def test_oracle_parity(capi, setups, name, z64, cm):
    """n = 1, 63, 64, 130: the lanes of a partly filled wave, a whole wave, two waves and
    two lanes (gauss24: 16 targets, whose node counts straddle the default launch slice)."""
    s = setups[name]
    ctx = _context(capi, s)
    for n in ((16,) if name == "gauss24" else (1, 63, 64, 130)):
        T = s["T"][:n]
        r = _run(capi, ctx, T, z64=z64, cm=cm)
        _check_against_oracle(s, T, r, status=0)
        print(f"  {name} n={n}: nodes median {int(np.median(r['nodes']))} max {int(r['nodes'].max())}")


def test_host_wrapper_and_decoder_agree_with_the_raw_call(capi, setups):
    from lgs_amd.decode import Decoder
    s = setups["int12"]
    T = s["T"][:130]
    want = _run(capi, _context(capi, s), T)
    r = _context(capi, s).closest_vector_host(T, MAX_NODES, want_cprime=True)
    for k in want:
        assert np.array_equal(r[k], want[k]), k
    dec = Decoder(s["B"])
    z, info = dec.closest_vector(T, max_nodes=MAX_NODES, coefficients=True, info=True)
    assert np.array_equal(z, want["z"]) and np.array_equal(info["dist2"], want["dist2"])
    assert np.array_equal(info["nodes"], want["nodes"]) and not info["status"].any()
    assert np.array_equal(dec.closest_vector(T[3]), want["v"][3])
    with pytest.raises(ValueError):
        Decoder(np.eye(65) * 3.0).closest_vector(np.zeros(65))


# ------------------------------------------------------------------ 2. slice independence
def _equal(a, b):
    for k in ("z", "v", "cprime", "dist2", "nodes", "status"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("max_proposals", [0, 64], ids=["onechunk", "chunks"])
def test_slice_of_64_nodes_suspends_and_resumes(capi, setups, monkeypatch, max_proposals):
    """int12, 130 targets (median 107 nodes, maximum 452): with 64 nodes per launch every
    target above 64 nodes is written back and resumed, up to 8 times.  max_proposals = 64:
    three chunks of 64, 64 and 2 targets."""
    s = setups["int12"]
    T = s["T"][:130]
    want = _run(capi, _context(capi, s), T)
    _check_against_oracle(s, T, want, status=0)
    monkeypatch.setenv("LGS_TEST_CVP_SLICE", "64")
    ctx = _context(capi, s, hooks=True, max_proposals=max_proposals)
    ctx.timing_enable(True)
    got = _run(capi, ctx, T)
    _equal(got, want)
    launches = ctx.timing_get(capi.KERNEL_CVP_ENUM)[1]
    per_chunk = [want["nodes"][o:o + (max_proposals or 130)].max() for o in range(0, 130, max_proposals or 130)]
    need = sum(-(-int(m) // 64) for m in per_chunk)  # a search of m nodes takes ceil(m / 64) launches
    print(f"  {launches} enumeration launches, at least {need} needed")
    assert need <= launches <= need + len(per_chunk)
    # the product library reads no environment: one launch per chunk of these targets
    prod = _context(capi, s, max_proposals=max_proposals)
    prod.timing_enable(True)
    _equal(_run(capi, prod, T), want)
    assert prod.timing_get(capi.KERNEL_CVP_ENUM)[1] == len(per_chunk)


def test_targets_wait_for_a_slot(capi, setups, monkeypatch):
    """64 lanes for 130 targets of one chunk: a lane whose target stops takes the next
    waiting one, inside a launch and across launches of 64 nodes."""
    s = setups["int12"]
    T = s["T"][:130]
    want = _run(capi, _context(capi, s), T)
    monkeypatch.setenv("LGS_TEST_CVP_SLOTS", "64")
    ctx = _context(capi, s, hooks=True)
    _equal(_run(capi, ctx, T), want)
    monkeypatch.setenv("LGS_TEST_CVP_SLICE", "64")
    _equal(_run(capi, ctx, T, z64=True, cm=True), want)


def test_default_slice_is_crossed_by_some_lanes(capi, setups):
    """gauss24, 16 targets, 27 430 to 84 901 nodes: ten stop within the first launch of 2^16
    nodes, six are resumed; the hooks library without a switch equals the product library."""
    s = setups["gauss24"]
    T = s["T"][:16]
    ctx = _context(capi, s)
    ctx.timing_enable(True)
    want = _run(capi, ctx, T)
    _check_against_oracle(s, T, want, status=0)
    assert (want["nodes"] <= 1 << 16).any() and (want["nodes"] > 1 << 16).any()
    assert ctx.timing_get(capi.KERNEL_CVP_ENUM)[1] == 2
    _equal(_run(capi, _context(capi, s, hooks=True), T), want)


def test_compaction_keeps_the_unfinished_searches(capi, setups, monkeypatch):
    """gauss20, 200 targets at 1000 nodes per launch (3530 to 10 160 nodes each): once at
    most half the lanes still work they are moved to the front of the other state block."""
    s = setups["gauss20"]
    T = s["T"][:200]
    want = _run(capi, _context(capi, s), T)
    _check_against_oracle(s, T, want, status=0)
    monkeypatch.setenv("LGS_TEST_CVP_SLICE", "1000")
    ctx = _context(capi, s, hooks=True)
    ctx.timing_enable(True)
    _equal(_run(capi, ctx, T), want)
    assert ctx.timing_get(capi.KERNEL_DECODE_SELECT)[1] >= 1  # a compaction ran


def test_split_calls_give_the_same_targets_the_same_results(capi, setups):
    s = setups["gauss16"]
    T = s["T"][:130]
    ctx = _context(capi, s)
    want = _run(capi, ctx, T)
    parts = [_run(capi, ctx, T[a:b]) for a, b in ((0, 1), (1, 70), (70, 130))]
    for k in ("z", "v", "cprime", "dist2", "nodes", "status"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), want[k]), k


# ------------------------------------------------------------------ 3. budget
def test_budget_returns_the_best_so_far(capi, setups):
    s = setups["gauss37"]
    T = s["T"][:8]
    r = _run(capi, _context(capi, s), T, max_nodes=1000)
    assert (r["status"] == 1).all() and (r["nodes"] == 1000).all()
    _check_against_oracle(s, T, r, max_nodes=1000, status=1)
    assert np.isfinite(r["dist2"]).all()  # (1000 nodes reach level 0 of every one of them)
    # one node cannot reach level 0: the outputs of status 2, with status 1
    r1 = _run(capi, _context(capi, s), T, max_nodes=1)
    assert (r1["status"] == 1).all() and (r1["nodes"] == 1).all() and np.isinf(r1["dist2"]).all()
    assert not r1["z"].any() and not r1["v"].any()


# ------------------------------------------------------------------ 4. radius, and the sampler's D
def test_radius_and_agreement_with_decoding_by_sampling(capi, setups):
    s = setups["int12"]
    T = s["T"][:130]
    ctx = _context(capi, s, sigma=45.0)
    sam = ctx.klein_decode_host(SEED, 0, T, 8, want_cprime=True)
    free = _run(capi, ctx, T)
    _check_against_oracle(s, T, free, status=0)
    assert np.array_equal(free["cprime"], sam["cprime"])
    assert (free["dist2"] <= sam["dist2"]).all()
    found = free["dist2"] == sam["dist2"]  # the sampler drew the closest point
    print(f"  the best of 8 draws is the closest point for {int(found.sum())} of 130 targets")
    r = _run(capi, ctx, T, radius2=sam["dist2"])
    _check_against_oracle(s, T, r, radius2=sam["dist2"])
    assert np.array_equal(r["status"] == 2, found) and np.array_equal(r["status"] == 0, ~found)
    assert np.isinf(r["dist2"][found]).all() and not r["z"][found].any() and not r["v"][found].any()
    assert np.array_equal(r["z"][~found], free["z"][~found])
    assert np.array_equal(r["dist2"][~found], free["dist2"][~found])
    assert (r["nodes"][~found] <= free["nodes"][~found]).all()
    # where the sampler found the closest point, its z is the search's (no ties on these targets)
    assert np.array_equal(sam["z"][found], free["z"][found])
    # a radius just above the closest point's distance keeps it
    above = np.nextafter(free["dist2"], np.inf)
    r = _run(capi, ctx, T, radius2=above)
    assert not r["status"].any() and np.array_equal(r["z"], free["z"]) and (r["nodes"] <= free["nodes"]).all()
    # the same from device buffers (a device radius2 is read back for its check)
    import torch
    dev = torch.device("cuda:0")
    zd = torch.empty((130, s["d"]), dtype=torch.int32, device=dev)
    nd = torch.empty(130, dtype=torch.int64, device=dev)
    sd = torch.empty(130, dtype=torch.int32, device=dev)
    ctx.closest_vector(torch.as_tensor(T.copy(), device=dev), MAX_NODES, torch.as_tensor(above, device=dev), zd,
                       None, None, None, nd, sd, capi.LGS_DEVICE_PTRS)
    assert np.array_equal(zd.cpu().numpy(), r["z"]) and np.array_equal(nd.cpu().numpy(), r["nodes"])
    assert not sd.cpu().numpy().any()
    bad = torch.as_tensor(np.where(np.arange(130) == 129, np.nan, above), device=dev)
    with pytest.raises(capi.LgsError) as e:
        ctx.closest_vector(torch.as_tensor(T.copy(), device=dev), MAX_NODES, bad, zd, None, None, None, nd, sd,
                           capi.LGS_DEVICE_PTRS)
    assert e.value.code == capi.LGS_ERR_INVALID


# ------------------------------------------------------------------ 5. device buffers, deep trees
DEEP_TARGETS = 8


def test_device_only_at_depth(capi, setups):
    """gauss37, max_nodes = 2^23, every buffer a device tensor.  The first 8 of the 256
    targets, 1.7 to 4.1 million nodes each: 3.9 s on an MI355X (the call lasts as long as its
    deepest lane, about 1 us per node; 16 targets took 6.5 s, 48 took 10.2 s, and target 56
    needs more than 2^23 nodes)."""
    import torch
    s = setups["gauss37"]
    n, d = DEEP_TARGETS, s["d"]
    T = s["T"][:n]
    ctx = _context(capi, s, sigma=30.0)
    dev = torch.device("cuda:0")
    t = torch.as_tensor(T.copy(), device=dev)
    z = torch.empty((n, d), dtype=torch.int32, device=dev)
    v = torch.empty((n, d), dtype=torch.float64, device=dev)
    cp = torch.empty((n, d), dtype=torch.float64, device=dev)
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    nodes = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.closest_vector(t, 1 << 23, None, z, v, cp, d2, nodes, status, capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    r = {"z": z.cpu().numpy().astype(np.int64), "v": v.cpu().numpy(), "cprime": cp.cpu().numpy(),
         "dist2": d2.cpu().numpy(), "nodes": nodes.cpu().numpy(), "status": status.cpu().numpy()}
    print(f"  gauss37: {n} targets, {int(r['nodes'].sum())} nodes in {dt:.2f} s "
          f"({r['nodes'].sum() / dt / 1e6:.1f} M nodes/s), per target {int(r['nodes'].min())} .. {int(r['nodes'].max())}")
    assert not r["status"].any()
    _check_cprime(s, T, r["cprime"])
    _check_v(s, r)
    for k in range(n):
        assert r["dist2"][k] == cvp_oracle.refdist(s["R"], r["cprime"][k], r["z"][k]), k
    sam = ctx.klein_decode_host(SEED, 0, T, 64, want_cprime=True)
    assert np.array_equal(sam["cprime"], r["cprime"])
    assert (r["dist2"] <= sam["dist2"]).all()


# ------------------------------------------------------------------ 6. errors
def _raw(capi, ctx, T, max_nodes, flags=0, radius2=None):
    n, d = T.shape
    z = np.zeros((n, d), dtype=np.int64 if flags & capi.LGS_Z64 else np.int32)
    r2 = None if radius2 is None else np.ascontiguousarray(radius2, dtype=np.float64)
    return ctx._L.lgs_closest_vector(ctx._h, n, capi._ptr(np.ascontiguousarray(T)), capi._ptr(r2), max_nodes,
                                     capi._ptr(z), None, None, None, flags), z


def test_errors_leave_the_context_usable(capi, setups):
    s = setups["int12"]
    T = s["T"][:70]
    ctx = _context(capi, s)
    want = _run(capi, ctx, T)

    def still_works():
        _equal(_run(capi, ctx, T), want)

    for bad_value in (np.nan, np.inf, -np.inf):
        Tb = T.copy()
        Tb[66, 5] = bad_value
        with pytest.raises(capi.LgsError) as e:
            _run(capi, ctx, Tb)
        assert e.value.code == capi.LGS_ERR_NONFINITE
        still_works()
    for flags in (capi.LGS_EXACT_ORDER, capi.LGS_WANG_LING, 0x1000):
        assert _raw(capi, ctx, T, 100, flags)[0] == capi.LGS_ERR_INVALID
    for max_nodes in (0, -5, (1 << 40) + 1):
        assert _raw(capi, ctx, T, max_nodes)[0] == capi.LGS_ERR_INVALID
    assert _raw(capi, ctx, T, 1 << 40, radius2=np.zeros(70))[0] == capi.LGS_OK  # nothing is below 0
    for bad_r in (-1.0, np.nan):
        r2 = np.full(70, 1e9)
        r2[69] = bad_r
        assert _raw(capi, ctx, T, 100, radius2=r2)[0] == capi.LGS_ERR_INVALID
    assert _raw(capi, ctx, T[:0], 100)[0] == capi.LGS_OK
    still_works()
    # |z| >= 2^31 needs LGS_Z64; the search itself is the same
    Tbig = T[:3] * 1e8
    rc, _ = _raw(capi, ctx, Tbig, MAX_NODES)
    assert rc == capi.LGS_ERR_OVERFLOW
    big = _run(capi, ctx, Tbig, z64=True)
    assert np.abs(big["z"]).max() >= 1 << 31
    _check_against_oracle(s, Tbig, big, status=0)
    assert np.array_equal(ctx.closest_vector_host(Tbig, MAX_NODES)["z"], big["z"])  # (retries in int64)
    still_works()


def test_needs_the_decoder_frame_unless_qframe(capi, setups):
    s = setups["int12"]
    T = s["T"][:64]
    ctx = _context(capi, s, decoder=False)
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, T)
    assert e.value.code == capi.LGS_ERR_STATE
    cp = np.ascontiguousarray(T @ s["Q"])
    q = _run(capi, ctx, cp, flags=capi.LGS_TARGETS_QFRAME)  # c' passed in is used verbatim
    assert np.array_equal(q["cprime"], cp)
    for k in range(64):
        z, D, nodes, st = _oracle(s, cp[k])
        assert np.array_equal(q["z"][k], z) and q["dist2"][k] == D and q["nodes"][k] == nodes and st == 0
    ctx.set_decoder(Q=s["Q"])
    want = _run(capi, ctx, T)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], 2.0)  # discards the frame, as for the other decoders
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, T)
    assert e.value.code == capi.LGS_ERR_STATE
    ctx.set_decoder(Q=s["Q"])
    _equal(_run(capi, ctx, T), want)  # (and sigma plays no part)


def test_dimension_above_64_is_invalid(capi):
    d = 65
    ctx = capi.Context(0)
    ctx.set_basis(np.eye(d) * 3.0, np.zeros(d), np.eye(d) * 3.0, 1.0)
    ctx.set_decoder(Q=np.eye(d))
    assert _raw(capi, ctx, np.zeros((2, d)), 100)[0] == capi.LGS_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.closest_vector_host(np.zeros((2, d)), 100)
    d = 64  # the largest supported: R fills 32 KB of LDS
    B = np.eye(d) * 3.0 + np.triu(np.ones((d, d)), 1)
    ctx.set_basis(B, np.zeros(d), B, 1.0)  # upper triangular with a positive diagonal: R = B, Q = I
    ctx.set_decoder(Q=np.eye(d))
    # targets within 0.3 per coordinate of a lattice point: R_ii = 3 prunes every other sibling
    rng = np.random.default_rng(64)
    T = rng.integers(-50, 51, (70, d)).astype(np.float64) @ B.T + rng.uniform(-0.3, 0.3, (70, d))
    r = ctx.closest_vector_host(T, MAX_NODES, want_cprime=True)
    assert np.array_equal(r["cprime"], T) and not r["status"].any()
    for k in range(0, 70, 9):
        z, D, nodes, st = cvp_oracle.se(B, T[k], max_nodes=MAX_NODES)
        assert np.array_equal(r["z"][k], z) and r["dist2"][k] == D and r["nodes"][k] == nodes and st == 0


# ------------------------------------------------------------------ 7. SimpleLattice.decode_cvp
def test_simple_lattice_decode_cvp_exact(capi, setups):
    from lgs_amd.lattices import SimpleLattice
    rows = setups["int12"]["B"].T.copy()  # the lattice of the ROWS of `rows` is int12's column lattice
    s = setups["int12"]
    T = s["T"][:40]
    lat = SimpleLattice(rows)
    got = lat.decode_cvp(T, method="exact")
    dec = lat._decoder()
    s = dict(s, name="int12 rows", R=dec._R, Q=dec._Q)  # the frame that decoder factorised
    cp = dec.ctx.closest_vector_host(T, 1 << 24, want_cprime=True)["cprime"]
    _check_cprime(s, T, cp)
    want = np.stack([_oracle(s, cp[k], 1 << 24)[0] for k in range(40)]).astype(np.float64) @ rows
    assert np.array_equal(got, want)
    assert np.array_equal(lat.decode_cvp(T[7], "exact"), want[7])
    babai = lat.decode_cvp(T, method="babai")
    assert np.array_equal(babai, lat.nearest_plane(T)) and np.array_equal(lat.decode_cvp(T), babai)
    closer = ((got - T) ** 2).sum(1) < ((babai - T) ** 2).sum(1) * (1 - 1e-9)
    print(f"  exact is closer than Babai on {int(closer.sum())} of 40 targets")
    assert (((got - T) ** 2).sum(1) <= ((babai - T) ** 2).sum(1) * (1 + 1e-12)).all()
    with pytest.raises(RuntimeError, match="nodes"):
        lat.decode_cvp(T, method="exact", max_nodes=20)
    with pytest.raises(ValueError):
        lat.decode_cvp(T, method="enumerate")
