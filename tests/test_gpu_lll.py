"""lgs_lll_reduce on the device against the Python transcription of its definition
(tests/lll_oracle.py): every output bit for bit, whatever the batch, the split into calls, the
pointer kind or the launch slice; the stops (max_iters, magnitude guard, not a basis, bad
input); the reduce=True paths of SimpleLattice end to end; dense signed bases at ragged d and
three (delta, eta), rounding ties and Gram entries that fp64 cannot hold; and the scheduler --
a mixed batch whose live list shrinks with holes over many launches, and more bases than one
chunk.  tests/test_lll_host.py checks the premises on the oracle (it terminates with work done
on every basis used here, its iteration counts lie on both sides of the forced slice, the
batches spread over the launches and cross the chunk the source names)."""
import itertools
import math

import numpy as np
import pytest

import lll_oracle

pytestmark = pytest.mark.gpu

FIELDS = ("basis_out", "U_out", "swaps", "iters", "passes", "status", "gs_norm2")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.Context(0)


def _run(ctx, bases, delta=0.99, eta=0.51, max_iters=1 << 40):
    """The raw call on host buffers, outputs pre-filled with values no reduction produces."""
    b = np.ascontiguousarray(bases, dtype=np.int64)
    n, d = b.shape[0], b.shape[1]
    bo, uo = np.full((n, d, d), -77, dtype=np.int64), np.full((n, d, d), -77, dtype=np.int64)
    sw, it, ps = (np.full(n, -1, dtype=np.int64) for _ in range(3))
    st, gs = np.full(n, -1, dtype=np.int32), np.full((n, d), np.nan)
    ctx.lll_reduce(b, bo, uo, delta, eta, max_iters, sw, it, ps, st, gs)
    return {"basis_out": bo, "U_out": uo, "swaps": sw, "iters": it, "passes": ps, "status": st, "gs_norm2": gs}


def _equal(got, k, want, what=""):
    """Entry k of a batched result against one oracle result, bit for bit."""
    w = lll_oracle.as_arrays(want)
    for f in FIELDS:
        g = got[f][k]
        assert g.dtype == w[f].dtype, (what, f)
        if f == "gs_norm2":
            assert g.tobytes() == w[f].tobytes(), (what, f, g, w[f])
        else:
            assert np.array_equal(g, w[f]), (what, f, g, w[f])


@pytest.mark.parametrize("name,delta", lll_oracle.CASES)
def test_parity_with_the_oracle(ctx, name, delta):
    B = lll_oracle.bases()[name]
    got = _run(ctx, B[None], delta)
    want = lll_oracle.reduced(name, delta)
    print(f"  {name} delta {delta}: iters {got['iters'][0]} (oracle {want['iters']}), swaps {got['swaps'][0]}, "
          f"status {got['status'][0]}")
    _equal(got, 0, want, (name, delta))
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])


@pytest.mark.parametrize("name", ["qary8", "ntru24", "qary32"])
def test_batch_and_split_invariance_host_and_device(capi, ctx, name):
    """Five mixed copies -- the basis, its column permutations and a negated one -- in one call,
    as five single calls, and on device buffers: every entry equals the oracle of its own input."""
    import torch
    B = lll_oracle.bases()[name]
    d = B.shape[0]
    rev, roll = B[:, ::-1], np.roll(B, 3, axis=1)
    neg = B * np.where(np.arange(d) % 2, -1, 1)[None, :]
    batch = np.ascontiguousarray(np.stack([B, rev, roll, B, neg]))
    want = [lll_oracle.lll(x.tolist(), 0.99) for x in (B, rev, roll)]
    want = [want[0], want[1], want[2], want[0], lll_oracle.lll(neg.tolist(), 0.99)]
    assert all(w["status"] == 0 for w in want) and len({w["iters"] for w in want}) >= 3
    got = _run(ctx, batch)
    for k in range(5):
        _equal(got, k, want[k], (name, "batch", k))
        _equal(_run(ctx, batch[k:k + 1]), 0, want[k], (name, "single", k))
    dev = torch.device("cuda:0")
    bd = torch.as_tensor(batch, device=dev)
    bo, uo = torch.full_like(bd, -77), torch.full_like(bd, -77)
    sw, it, ps = (torch.full((5,), -1, dtype=torch.int64, device=dev) for _ in range(3))
    st = torch.full((5,), -1, dtype=torch.int32, device=dev)
    gs = torch.full((5, d), math.nan, dtype=torch.float64, device=dev)
    ctx.lll_reduce(bd, bo, uo, 0.99, 0.51, 1 << 40, sw, it, ps, st, gs, flags=capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    gd = {"basis_out": bo.cpu().numpy(), "U_out": uo.cpu().numpy(), "swaps": sw.cpu().numpy(),
          "iters": it.cpu().numpy(), "passes": ps.cpu().numpy(), "status": st.cpu().numpy(),
          "gs_norm2": gs.cpu().numpy()}
    for k in range(5):
        _equal(gd, k, want[k], (name, "device", k))
    assert torch.equal(bd, torch.as_tensor(batch, device=dev))  # the input is not written
    bo1, uo1 = torch.full_like(bd, -77), torch.full_like(bd, -77)
    for k in range(5):  # the split into single calls, on slices of the device buffers
        ctx.lll_reduce(bd[k:k + 1], bo1[k:k + 1], uo1[k:k + 1], flags=capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    assert torch.equal(bo1, bo) and torch.equal(uo1, uo)
    # outputs are optional, singly and all together
    bo2, uo2 = np.zeros_like(batch), np.zeros_like(batch)
    ctx.lll_reduce(batch, bo2, uo2)
    assert np.array_equal(bo2, got["basis_out"]) and np.array_equal(uo2, got["U_out"])
    st2 = np.full(5, -1, dtype=np.int32)
    ctx.lll_reduce(batch, bo2, uo2, status=st2)
    assert np.array_equal(st2, got["status"])


@pytest.mark.parametrize("name", lll_oracle.NAMES)
def test_forced_slice_spans_launches(capi, monkeypatch, name):
    """lll_oracle.SLICE iterations per launch (hooks library): d2 and d3 stop inside the first
    launch, every other reduction is suspended and resumed at least twice.  Timer 9 counts the
    set-up launch and every reduction launch."""
    monkeypatch.setenv("LGS_TEST_LLL_SLICE", str(lll_oracle.SLICE))
    hctx = capi.Context(0, hooks=True)
    want = lll_oracle.reduced(name, 0.75)
    hctx.timing_enable(True)
    got = _run(hctx, lll_oracle.bases()[name][None], 0.75)
    _, launches = hctx.timing_get(capi.KERNEL_CVP_ENUM)
    _equal(got, 0, want, name)
    # a launch that completes the last iteration also sees k reach d
    assert launches == 1 + max(1, -(-want["iters"] // lll_oracle.SLICE))
    if name not in ("d2", "d3"):
        assert launches - 1 >= 3
    hctx.close()


def test_product_library_ignores_the_slice_switch(capi, monkeypatch):
    monkeypatch.setenv("LGS_TEST_LLL_SLICE", "1")
    c = capi.Context(0)
    c.timing_enable(True)
    _equal(_run(c, lll_oracle.bases()["qary8"][None], 0.75), 0, lll_oracle.reduced("qary8", 0.75))
    assert c.timing_get(capi.KERNEL_CVP_ENUM)[1] == 2  # set-up and one reduction launch
    c.close()


@pytest.mark.parametrize("name", ["qary8", "ntru24", "qary40"])
def test_max_iters_returns_the_intermediate_state(ctx, name):
    full = lll_oracle.reduced(name, 0.99)
    half = full["iters"] // 2
    want = lll_oracle.reduced(name, 0.99, half)
    assert want["status"] == 1 and want["iters"] == half
    B = lll_oracle.bases()[name]
    got = _run(ctx, np.stack([B, B]), 0.99, max_iters=half)
    _equal(got, 0, want, name)
    _equal(got, 1, want, name)
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])  # still a basis of the lattice
    _equal(_run(ctx, B[None], 0.99, max_iters=full["iters"]), 0, full, name)  # exactly enough


@pytest.mark.parametrize("d", [2, 3, 17, 64])
def test_identity_is_left_alone(ctx, d):
    got = _run(ctx, np.eye(d, dtype=np.int64)[None])
    assert got["status"][0] == 0 and got["swaps"][0] == 0 and got["iters"][0] == d - 1
    assert got["passes"][0] == d - 1
    assert np.array_equal(got["U_out"][0], np.eye(d, dtype=np.int64))
    assert np.array_equal(got["basis_out"][0], np.eye(d, dtype=np.int64))
    assert np.array_equal(got["gs_norm2"][0], np.ones(d))


def test_singular_inputs_give_status_3(ctx):
    for singular in ([[1, 1], [2, 2]], [[0, 1], [0, 5]], [[1, 2, 3], [4, 5, 6], [7, 8, 9]]):
        want = lll_oracle.lll(singular)
        assert want["status"] == 3
        B = np.array(singular, dtype=np.int64)
        got = _run(ctx, B[None])
        _equal(got, 0, want, singular)
        assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])
    # a singular basis does not disturb its neighbours in the batch
    good = np.array([[1, 0, 0], [11, 1, 0], [5, 3, 29]], dtype=np.int64)
    got = _run(ctx, np.stack([good, np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]]), good]))
    assert list(got["status"]) == [0, 3, 0]
    _equal(got, 0, lll_oracle.reduced("d3", 0.99), "neighbour")
    _equal(got, 2, lll_oracle.reduced("d3", 0.99), "neighbour")


def test_entry_of_2_to_28_is_invalid(capi, ctx):
    import torch
    B = np.stack([lll_oracle.bases()["qary8"]] * 3)
    for v in (1 << 28, -(1 << 28)):
        bad = B.copy()
        bad[2, 7, 0] = v
        bo, uo = np.full_like(bad, -77), np.full_like(bad, -77)
        with pytest.raises(capi.LgsError) as e:
            ctx.lll_reduce(bad, bo, uo)
        assert e.value.code == capi.LGS_ERR_INVALID and "2^28" in str(e.value)
        assert np.all(bo == -77) and np.all(uo == -77)
        bd = torch.as_tensor(bad, device="cuda:0")
        bod, uod = torch.full_like(bd, -77), torch.full_like(bd, -77)
        with pytest.raises(capi.LgsError) as e:
            ctx.lll_reduce(bd, bod, uod, flags=capi.LGS_DEVICE_PTRS)
        assert e.value.code == capi.LGS_ERR_INVALID and "2^28" in str(e.value)
        assert bool((bod == -77).all()) and bool((uod == -77).all())
    ok = B.copy()
    ok[2, 7, 0] = (1 << 28) - 1  # the largest entry allowed: the call runs (whatever it stops with)
    got = _run(ctx, ok)
    _equal(got, 2, lll_oracle.lll(ok[2].tolist(), 0.99), "2^28 - 1")


def test_magnitude_guard_gives_status_2(ctx):
    """Each guard, and the value just inside it: |X| = 2^23 against 2^22 - 1; an update with
    |X| < 2^22 that would carry a coordinate of b past 2^28 (b_1 = (M, M), M = 2^28 - 1, against
    b_0 = (192, -128): X = 322 638, the second coordinate would be M + 128 X); two updates of
    X = 2^21 whose product would put 2^42 into U, against 2^21 * 2^18 = 2^39.  On a hit the
    state before the offending update is returned (the oracle's, bit for bit)."""
    M = (1 << 28) - 1
    cases = ([[1, 1 << 23], [0, 1]], [[1, (1 << 22) - 1], [0, 1]], [[192, M], [-128, M]],
             [[1, 1 << 21, 0], [0, 1, 1 << 21], [0, 0, 1]], [[1, 1 << 21, 0], [0, 1, 1 << 18], [0, 0, 1]])
    want = [lll_oracle.lll(B) for B in cases]
    assert [w["status"] for w in want] == [2, 0, 2, 2, 0]
    for B, w in zip(cases, want):
        _equal(_run(ctx, np.array(B, dtype=np.int64)[None]), 0, w, B)
    assert want[0]["U_out"] == [[1, 0], [0, 1]] and want[3]["U_out"][0][1] == -(1 << 21)


def test_simple_lattice_reduce_end_to_end():
    """qary_basis(6, 6, 97), d = 12: lambda_1 with reduce=True equals brute force over the
    oracle's reduced basis; exact CVP returns the same lattice point with and without."""
    from lgs_amd import lattices
    from lgs_amd.reduction import LatticeReduction, lll_reduce
    rows = lattices.qary_basis(6, 6, 97)
    lat = lattices.SimpleLattice(rows, name="qary12")
    want = lll_oracle.reduced("qary12", 0.99)
    Bp = np.array(want["basis_out"], dtype=np.int64)  # reduced vectors in columns
    # brute force over [-1, 1]^12: z = B'^-1 v gives |z_i| <= |row i of B'^-1| |v|, and with |v| at
    # most the shortest reduced vector that bound is below 2 for every i (checked here), so no
    # point outside the box can be as short
    shortest = math.sqrt(min(int(np.sum(Bp[:, i] ** 2)) for i in range(12)))
    assert np.all(shortest * np.linalg.norm(np.linalg.inv(Bp.astype(np.float64)), axis=1) < 1.99)
    Z = np.array(list(itertools.product((-1, 0, 1), repeat=12)), dtype=np.int64)
    n2 = np.sum((Z @ Bp.T) ** 2, axis=1)
    best = int(n2[n2 > 0].min())
    # (the enumeration's squared distances are fp64 sums in the QR frame of an integer lattice:
    # the integer they round to is the squared norm, and they lie within 1e-9 of it)
    for lam in (lat.first_minimum(reduce=True), lat.lll().first_minimum()):
        assert round(lam * lam) == best and abs(lam * lam - best) < 1e-9
    # the public reduction gives the oracle's basis, in rows, with U @ basis = reduced
    red, U, info = lll_reduce(rows)
    assert info["status"] == 0 and info["iters"] == want["iters"]
    assert np.array_equal(red.T, Bp) and np.array_equal(U @ rows.astype(np.int64), red)
    assert np.array_equal(lat.lll().basis, red.astype(np.float64))
    r2, U2, diag = LatticeReduction().lll_reduce(rows)
    assert np.array_equal(U2 @ rows, r2) and diag["improvement_factor"] > 1.0
    assert diag["final_quality"]["max_gs_norm"] < diag["initial_quality"]["max_gs_norm"]
    # exact CVP: the same point where the raw basis finishes; coefficients refer to the caller's rows
    # (targets within 1 of a lattice point per coordinate: far targets cost the raw basis more
    # than 2^24 nodes each, seconds of enumeration)
    rng = np.random.default_rng(7)
    T = rng.integers(-3, 4, size=(3, 12)) @ rows + rng.uniform(-1.0, 1.0, size=(3, 12))
    fast = lat.decode_cvp(T, "exact", max_nodes=1 << 20, reduce=True)  # proven for every target, or it raises
    plain, info = lat._decoder().closest_vector(T, max_nodes=1 << 22, info=True)
    done = info["status"] == 0
    print(f"  raw basis: {int(done.sum())} of 3 targets proven, nodes {info['nodes']}")
    assert np.array_equal(plain[done], fast[done])
    dist = lambda v: np.sum((T - v) ** 2, axis=1)  # noqa: E731
    assert np.all(dist(fast) <= dist(plain) + 1e-9) and np.all(dist(fast) <= dist(lat.nearest_plane(T)) + 1e-9)
    z = lat._decoder(True).closest_vector(T, coefficients=True)
    assert z.dtype == np.int64 and np.array_equal(z @ rows.astype(np.int64), fast.astype(np.int64))
    # the Gaussian mass on the reduced frame is the reduced lattice's own; mean_z refers to `rows`
    c = rng.uniform(-5.0, 5.0, size=12)
    m1 = lat.gaussian_mass(3.0, center=c, nats=6.0, moments=True, reduce=True)
    m2 = lat.lll().gaussian_mass(3.0, center=c, nats=6.0, moments=True)
    assert m1["status"] == 0 and m1["points"] == m2["points"] >= 1 and m1["log_mass"] == m2["log_mass"]
    assert np.allclose(m1["mean_z"] @ rows, m2["mean_z"] @ red.astype(np.float64), rtol=0, atol=1e-9)


# ---------------------------------------------------------------- dense signed bases, rounding ties, large Gram
@pytest.mark.parametrize("name,delta,eta", lll_oracle.DENSE_CASES)
def test_parity_on_dense_signed_bases(ctx, name, delta, eta):
    """Dense bases with entries of both signs at the d where the ownership of lanes changes (5, 7,
    17, 33, 63, 64), at three (delta, eta) whose iteration counts differ (test_lll_host.py)."""
    B = lll_oracle.bases()[name]
    got = _run(ctx, B[None], delta, eta)
    want = lll_oracle.reduced(name, delta, eta=eta)
    print(f"  {name} ({delta}, {eta}): iters {got['iters'][0]} (oracle {want['iters']}), swaps {got['swaps'][0]}, "
          f"status {got['status'][0]}")
    _equal(got, 0, want, (name, delta, eta))
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])


@pytest.mark.parametrize("name", lll_oracle.TIE_NAMES + lll_oracle.BIG_NAMES)
def test_parity_on_rounding_ties_and_gram_entries_above_2_to_53(ctx, name):
    """mu[1][0] exactly 2.5, -2.5, 3.5, 1.5: the size reduction rounds half to even (the first two
    give another basis under half-away, test_lll_host.py).  big4, big9: Gram entries of 55 and more
    bits, whose conversion to fp64 rounds; big9 trips the magnitude guard in iteration 30."""
    B = lll_oracle.bases()[name]
    got = _run(ctx, np.stack([B, B]))
    want = lll_oracle.reduced(name, 0.99)
    print(f"  {name}: iters {got['iters'][0]} (oracle {want['iters']}), status {got['status'][0]}")
    _equal(got, 0, want, name)
    _equal(got, 1, want, name)
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])


def test_library_refuses_parameters_out_of_range_on_either_pointer_kind(capi, ctx):
    """delta, eta and d outside their ranges, straight to the library (Context.lll_reduce refuses
    them before it): LGS_ERR_INVALID, and no output is touched, with host and with device pointers."""
    import torch
    bad = [dict(delta=v) for v in (0.25, 1.0, math.nan)] + [dict(eta=v) for v in (0.5, 1.0, math.nan)] + \
        [dict(d=1), dict(d=65)]
    for kw in bad:
        d = kw.get("d", 4)
        B = np.stack([np.eye(d, dtype=np.int64) * 3] * 2)
        for dev in (False, True):
            b = torch.as_tensor(B, device="cuda:0") if dev else B
            bo, uo = (torch.full_like(b, -77) for _ in range(2)) if dev else (np.full_like(B, -77) for _ in range(2))
            st = torch.full((2,), -1, dtype=torch.int32, device="cuda:0") if dev else np.full(2, -1, dtype=np.int32)
            rc = ctx._L.lgs_lll_reduce(ctx._h, 2, d, capi._ptr(b), kw.get("delta", 0.99), kw.get("eta", 0.51), 100,
                                       capi._ptr(bo), capi._ptr(uo),
                                       capi._outputs(capi.LllOutputs, None, None, None, st, None),
                                       capi.LGS_DEVICE_PTRS if dev else 0)
            assert rc == capi.LGS_ERR_INVALID, (kw, dev)
            word = next(iter(kw))
            assert ("d = " if word == "d" else word) in ctx._L.lgs_last_error().decode(), (kw, dev)
            if dev:
                torch.cuda.synchronize()
            assert bool((bo == -77).all()) and bool((uo == -77).all()) and bool((st == -1).all()), (kw, dev)
    got = _run(ctx, np.eye(4, dtype=np.int64)[None] * 3)  # the context still works
    assert got["status"][0] == 0 and got["iters"][0] == 3


# ---------------------------------------------------------------- the scheduler: batches across launches and chunks
def _device_run(capi, c, bd, delta=0.99, eta=0.51, max_iters=1 << 40, only=FIELDS[2:]):
    """The raw call on device buffers (bd a device tensor), the optional outputs named in `only`
    requested and pre-filled like _run's; returns host arrays."""
    import torch
    n, d, dev = bd.shape[0], bd.shape[1], bd.device
    out = {"basis_out": torch.full_like(bd, -77), "U_out": torch.full_like(bd, -77)}
    for f in only:
        out[f] = (torch.full((n, d), math.nan, dtype=torch.float64, device=dev) if f == "gs_norm2" else
                  torch.full((n,), -1, dtype=torch.int32 if f == "status" else torch.int64, device=dev))
    c.lll_reduce(bd, out["basis_out"], out["U_out"], delta, eta, max_iters, flags=capi.LGS_DEVICE_PTRS,
                 **{f: out[f] for f in only})
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in out.items()}


def _host_run(c, bases, only):
    """_run with only the optional outputs named in `only`."""
    b = np.ascontiguousarray(bases, dtype=np.int64)
    n, d = b.shape[0], b.shape[1]
    out = {"basis_out": np.full((n, d, d), -77, dtype=np.int64), "U_out": np.full((n, d, d), -77, dtype=np.int64)}
    for f in only:
        out[f] = (np.full((n, d), np.nan) if f == "gs_norm2" else
                  np.full(n, -1, dtype=np.int32 if f == "status" else np.int64))
    c.lll_reduce(b, out["basis_out"], out["U_out"], **{f: out[f] for f in only})
    return out


def _equal_all(got, wants, what):
    """Every entry of a batched result against its own oracle result, whole arrays at a time."""
    conv = {id(o): lll_oracle.as_arrays(o) for o in wants}
    for f in got:
        w = np.stack([conv[id(o)][f] for o in wants])
        assert got[f].dtype == w.dtype and got[f].shape == w.shape, (what, f)
        diff = np.flatnonzero((got[f].view(np.int64) != w.view(np.int64)).reshape(len(wants), -1).any(axis=1)) \
            if f == "gs_norm2" else np.flatnonzero((got[f] != w).reshape(len(wants), -1).any(axis=1))
        assert diff.size == 0, (what, f, "entries", diff[:8], got[f][diff[0]], w[diff[0]])


def _launches(c, capi):
    return c.timing_get(capi.KERNEL_CVP_ENUM)[1]


def test_mixed_batch_spans_launches(capi, monkeypatch):
    """lll_oracle.mixed_batch() -- 29 bases of d = 17 whose reductions need 1 to 24 launches of
    SLICE iterations, the early leavers in the middle of the batch -- on the hooks library: every
    entry equals its own oracle whatever list of live bases the launches pass on, with host and
    device pointers, reversed, split into single calls, and with a budget that stops some entries
    (status 1) while others end (0) or fail (3).  Timer 9 counts the set-up launch and the
    reduction launches of the entry that needs most: max(1, ceil(iters / SLICE)) each, since
    lll_loop sees k = d, and iters = max_iters, before it looks at the launch's budget."""
    import torch
    monkeypatch.setenv("LGS_TEST_LLL_SLICE", str(lll_oracle.SLICE))
    hctx = capi.Context(0, hooks=True)
    B, want = lll_oracle.mixed_batch(), lll_oracle.mixed_reduced()
    count = 1 + max(lll_oracle.launches(w) for w in want)
    hctx.timing_enable(True)
    got = _run(hctx, B)
    assert _launches(hctx, capi) == count
    _equal_all(got, want, "host")
    for k, w in enumerate(want):
        _equal(got, k, w, ("host", k))
    hctx.timing_enable(True)
    _equal_all(_run(hctx, B[::-1]), want[::-1], "reversed")
    assert _launches(hctx, capi) == count
    bd = torch.as_tensor(B, device="cuda:0")
    hctx.timing_enable(True)
    gd = _device_run(capi, hctx, bd)
    assert _launches(hctx, capi) == count
    _equal_all(gd, want, "device")
    assert torch.equal(bd, torch.as_tensor(B, device="cuda:0"))  # the input is not written
    _equal_all(_device_run(capi, hctx, bd.flip(0).contiguous()), want[::-1], "device, reversed")
    bo1, uo1 = torch.full_like(bd, -77), torch.full_like(bd, -77)
    for k in range(len(B)):  # the split into single calls, on slices of the device buffers
        hctx.lll_reduce(bd[k:k + 1], bo1[k:k + 1], uo1[k:k + 1], flags=capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    assert np.array_equal(bo1.cpu().numpy(), gd["basis_out"]) and np.array_equal(uo1.cpu().numpy(), gd["U_out"])
    # a budget between the entries' iteration counts
    cut = lll_oracle.mixed_reduced(lll_oracle.MIXED_MAX_ITERS)
    count = 1 + max(lll_oracle.launches(w) for w in cut)
    hctx.timing_enable(True)
    _equal_all(_run(hctx, B, max_iters=lll_oracle.MIXED_MAX_ITERS), cut, "max_iters, host")
    assert _launches(hctx, capi) == count
    hctx.timing_enable(True)
    _equal_all(_device_run(capi, hctx, bd, max_iters=lll_oracle.MIXED_MAX_ITERS), cut, "max_iters, device")
    assert _launches(hctx, capi) == count
    hctx.close()


@pytest.mark.parametrize("library,dev", [("product", False), ("product", True), ("hooks", False), ("hooks", True)])
def test_more_bases_than_one_chunk(capi, monkeypatch, library, dev):
    """lll_oracle.chunk_batch(): 1030 bases of d = 3, six more than the scheduler's chunk, a
    singular one on either side of the boundary.  Every optional output at once, then status
    alone, then gs_norm2 alone (each offset is its own code); on the hooks library two iterations
    per launch, so that the second chunk's live list spans launches too.  Timer 9: per chunk the
    set-up launch and the reduction launches of the entry that needs most."""
    import torch
    slice_ = 1 << 12
    if library == "hooks":
        slice_ = 2
        monkeypatch.setenv("LGS_TEST_LLL_SLICE", "2")
    c = capi.Context(0, hooks=library == "hooks")
    B, idx = lll_oracle.chunk_batch()
    B0 = B.copy()
    R = lll_oracle.chunk_reduced()
    want = [R[v] for v in idx]
    count = sum(1 + max(lll_oracle.launches(R[v], slice_) for v in part) for part in (idx[:1024], idx[1024:]))
    assert (count == 4) if library == "product" else (count > 8)
    bd = torch.as_tensor(B, device="cuda:0") if dev else None
    for only in (FIELDS[2:], ("status",), ("gs_norm2",)):
        c.timing_enable(True)
        got = _device_run(capi, c, bd, only=only) if dev else _host_run(c, B, only)
        assert _launches(c, capi) == count, only
        assert sorted(got) == sorted(("basis_out", "U_out") + tuple(only))
        _equal_all(got, want, (library, dev, only))
    assert np.array_equal(bd.cpu().numpy() if dev else B, B0)  # the input is not written
    c.close()
