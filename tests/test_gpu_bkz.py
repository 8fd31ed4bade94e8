"""lgs_bkz_reduce on the device against the Python transcription of its definition
(tests/bkz_oracle.py): every output bit for bit, whatever the batch, the split into calls, the
pointer kind or the launch slices; the stops (enum_nodes, max_tours, max_iters, the magnitude
guard of INSERT, not a basis, bad input); the public layers end to end; dense signed bases at
ragged d and the rounding ties; and the scheduler -- a mixed batch suspended inside LLL runs and
inside enumerations over many launches, and more bases than one chunk.
tests/test_bkz_host.py checks the premises on the oracle."""
import math

import numpy as np
import pytest

import bkz_oracle
import lll_oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("swaps", "iters", "passes", "tours", "blocks", "insertions", "nodes", "truncated")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.Context(0)


def _run(ctx, bases, beta, delta=0.99, eta=0.51, max_tours=1 << 40, max_iters=1 << 40, enum_nodes=1 << 40):
    """The raw call on host buffers, outputs pre-filled with values no reduction produces."""
    b = np.ascontiguousarray(bases, dtype=np.int64)
    n, d = b.shape[0], b.shape[1]
    out = {"basis_out": np.full((n, d, d), -77, dtype=np.int64), "U_out": np.full((n, d, d), -77, dtype=np.int64),
           "status": np.full(n, -1, dtype=np.int32), "gs_norm2": np.full((n, d), np.nan)}
    out.update({f: np.full(n, -1, dtype=np.int64) for f in COUNTERS})
    ctx.bkz_reduce(b, out["basis_out"], out["U_out"], beta, delta, eta, max_tours, max_iters, enum_nodes,
                   *(out[f] for f in COUNTERS), out["status"], out["gs_norm2"])
    return out


def _equal(got, k, want, what=""):
    """Entry k of a batched result against one oracle result, bit for bit."""
    w = bkz_oracle.as_arrays(want)
    for f in bkz_oracle.FIELDS:
        g = got[f][k]
        assert g.dtype == w[f].dtype, (what, f)
        if f == "gs_norm2":
            assert g.tobytes() == w[f].tobytes(), (what, f, g, w[f])
        else:
            assert np.array_equal(g, w[f]), (what, f, g, w[f])


@pytest.mark.parametrize("name,beta,delta", bkz_oracle.CASES)
def test_parity_with_the_oracle(ctx, name, beta, delta):
    B = bkz_oracle.basis(name)
    want = bkz_oracle.reduced(name, beta, delta)
    got = _run(ctx, B[None], beta, delta, max_tours=2 if name == "lll64" else 1 << 40)
    print(f"  {name} beta {beta} delta {delta}: status {got['status'][0]}, tours {got['tours'][0]}, insertions "
          f"{got['insertions'][0]} (oracle {want['insertions']}), nodes {got['nodes'][0]} (oracle {want['nodes']}), "
          f"iters {got['iters'][0]} (oracle {want['iters']})")
    _equal(got, 0, want, (name, beta, delta))
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])


def test_no_insertion_equals_lll_on_the_device(ctx):
    B = lll_oracle.bases()["qary8"]
    got = _run(ctx, B[None], 4)
    bo, uo = np.zeros_like(B[None]), np.zeros_like(B[None])
    sw, it, ps = (np.zeros(1, dtype=np.int64) for _ in range(3))
    st, gs = np.zeros(1, dtype=np.int32), np.zeros((1, 8))
    ctx.lll_reduce(B[None], bo, uo, 0.99, 0.51, 1 << 40, sw, it, ps, st, gs)
    assert got["insertions"][0] == 0 and got["status"][0] == 0 == st[0]
    assert np.array_equal(got["basis_out"], bo) and np.array_equal(got["U_out"], uo)
    assert (got["swaps"][0], got["iters"][0], got["passes"][0]) == (sw[0], it[0], ps[0])
    assert got["gs_norm2"].tobytes() == gs.tobytes()


@pytest.mark.parametrize("name,beta", [("qary16", 8), ("ntru24", 10)])
def test_batch_and_split_invariance_host_and_device(capi, ctx, name, beta):
    """Five mixed copies -- the basis, two column permutations, a repeat and a negated one -- in one
    call, as five single calls, and on device buffers: every entry equals the oracle of its own input."""
    import torch
    B = lll_oracle.bases()[name]
    d = B.shape[0]
    rev, roll = B[:, ::-1], np.roll(B, 3, axis=1)
    neg = B * np.where(np.arange(d) % 2, -1, 1)[None, :]
    batch = np.ascontiguousarray(np.stack([B, rev, roll, B, neg]))
    want = [bkz_oracle.reduced(name, beta)] + [bkz_oracle.bkz(x.tolist(), beta) for x in (rev, roll)]
    want = [want[0], want[1], want[2], want[0], bkz_oracle.bkz(neg.tolist(), beta)]
    assert all(w["status"] == 0 for w in want) and len({w["iters"] for w in want}) >= 3
    got = _run(ctx, batch, beta)
    for k in range(5):
        _equal(got, k, want[k], (name, "batch", k))
        _equal(_run(ctx, batch[k:k + 1], beta), 0, want[k], (name, "single", k))
    dev = torch.device("cuda:0")
    bd = torch.as_tensor(batch, device=dev)
    bo, uo = torch.full_like(bd, -77), torch.full_like(bd, -77)
    ctr = [torch.full((5,), -1, dtype=torch.int64, device=dev) for _ in COUNTERS]
    st = torch.full((5,), -1, dtype=torch.int32, device=dev)
    gs = torch.full((5, d), math.nan, dtype=torch.float64, device=dev)
    ctx.bkz_reduce(bd, bo, uo, beta, 0.99, 0.51, 1 << 40, 1 << 40, 1 << 40, *ctr, st, gs, flags=capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    gd = {"basis_out": bo.cpu().numpy(), "U_out": uo.cpu().numpy(), "status": st.cpu().numpy(),
          "gs_norm2": gs.cpu().numpy()}
    gd.update({f: t.cpu().numpy() for f, t in zip(COUNTERS, ctr)})
    for k in range(5):
        _equal(gd, k, want[k], (name, "device", k))
    assert torch.equal(bd, torch.as_tensor(batch, device=dev))  # the input is not written
    bo1, uo1 = torch.full_like(bd, -77), torch.full_like(bd, -77)
    for k in range(5):  # the split into single calls, on slices of the device buffers
        ctx.bkz_reduce(bd[k:k + 1], bo1[k:k + 1], uo1[k:k + 1], beta, flags=capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    assert torch.equal(bo1, bo) and torch.equal(uo1, uo)
    # outputs are optional, singly and all together
    bo2, uo2 = np.zeros_like(batch), np.zeros_like(batch)
    ctx.bkz_reduce(batch, bo2, uo2, beta)
    assert np.array_equal(bo2, got["basis_out"]) and np.array_equal(uo2, got["U_out"])
    for f in COUNTERS:
        one = np.full(5, -1, dtype=np.int64)
        ctx.bkz_reduce(batch, bo2, uo2, beta, **{f: one})
        assert np.array_equal(one, got[f]), f
    st2 = np.full(5, -1, dtype=np.int32)
    ctx.bkz_reduce(batch, bo2, uo2, beta, status=st2)
    assert np.array_equal(st2, got["status"])


@pytest.mark.parametrize("name,beta", bkz_oracle.SLICE_CASES)
def test_forced_slices_span_launches(capi, monkeypatch, name, beta):
    """BKZ_SLICE nodes and LLL_SLICE iterations per launch (hooks library): enumerations and LLL
    runs are suspended and resumed, some blocks finish inside a launch, and nothing changes."""
    monkeypatch.setenv("LGS_TEST_BKZ_SLICE", str(bkz_oracle.BKZ_SLICE))
    monkeypatch.setenv("LGS_TEST_LLL_SLICE", str(bkz_oracle.LLL_SLICE))
    hctx = capi.Context(0, hooks=True)
    want = bkz_oracle.reduced(name, beta)
    hctx.timing_enable(True)
    got = _run(hctx, lll_oracle.bases()[name][None], beta)
    _, launches = hctx.timing_get(capi.KERNEL_CVP_ENUM)
    _equal(got, 0, want, (name, beta))
    # every launch but the last spends a whole slice of one kind; the set-up launch counts too
    most = 2 + -(-want["iters"] // bkz_oracle.LLL_SLICE) + -(-want["nodes"] // bkz_oracle.BKZ_SLICE)
    least = 1 + max(-(-want["iters"] // bkz_oracle.LLL_SLICE), -(-want["nodes"] // bkz_oracle.BKZ_SLICE))
    print(f"  {name} beta {beta}: {launches} launches (between {least} and {most})")
    assert 3 < least <= launches <= most
    hctx.close()


def test_product_library_ignores_the_slice_switches(capi, monkeypatch):
    monkeypatch.setenv("LGS_TEST_BKZ_SLICE", "1")
    monkeypatch.setenv("LGS_TEST_LLL_SLICE", "1")
    c = capi.Context(0)
    c.timing_enable(True)
    _equal(_run(c, lll_oracle.bases()["qary16"][None], 8), 0, bkz_oracle.reduced("qary16", 8))
    assert c.timing_get(capi.KERNEL_CVP_ENUM)[1] == 2  # set-up and one reduction launch
    c.close()


def test_enum_nodes_truncates_blocks(ctx):
    want = bkz_oracle.reduced("qary32", 12, enum_nodes=64)
    assert want["status"] == 0 and 0 < want["truncated"] < want["blocks"]
    got = _run(ctx, lll_oracle.bases()["qary32"][None], 12, enum_nodes=64)
    print(f"  truncated {got['truncated'][0]} of {got['blocks'][0]} blocks, {got['tours'][0]} tours")
    _equal(got, 0, want, "enum_nodes")


def test_max_tours_gives_status_4(ctx):
    want = bkz_oracle.reduced("qary32", 12, max_tours=2)
    assert (want["status"], want["tours"]) == (4, 2)
    B = lll_oracle.bases()["qary32"]
    got = _run(ctx, B[None], 12, max_tours=2)
    _equal(got, 0, want, "max_tours")
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])


def test_max_iters_trips_inside_a_later_lll(ctx):
    first_lll = lll_oracle.reduced("qary32", 0.99)["iters"]
    want = bkz_oracle.reduced("qary32", 12, max_iters=first_lll + 5)
    assert want["status"] == 1 and want["insertions"] >= 1 and want["iters"] == first_lll + 5
    B = lll_oracle.bases()["qary32"]
    got = _run(ctx, np.stack([B, B]), 12, max_iters=first_lll + 5)
    _equal(got, 0, want, "max_iters")
    _equal(got, 1, want, "max_iters")
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])  # still a basis of the lattice


def test_singular_inputs_give_status_3(ctx):
    for singular in ([[1, 1], [2, 2]], [[0, 1], [0, 5]], [[1, 2, 3], [4, 5, 6], [7, 8, 9]]):
        want = bkz_oracle.bkz(singular, 2)
        assert want["status"] == 3
        B = np.array(singular, dtype=np.int64)
        got = _run(ctx, B[None], 2)
        _equal(got, 0, want, singular)
        assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])
    # a singular basis does not disturb its neighbours in the batch
    good = lll_oracle.bases()["d3"]
    got = _run(ctx, np.stack([good, np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]]), good]), 3)
    assert list(got["status"]) == [0, 3, 0]
    _equal(got, 0, bkz_oracle.reduced("d3", 3), "neighbour")
    _equal(got, 2, bkz_oracle.reduced("d3", 3), "neighbour")


def test_entry_of_2_to_28_is_invalid(capi, ctx):
    import torch
    B = np.stack([lll_oracle.bases()["qary8"]] * 3)
    for v in (1 << 28, -(1 << 28)):
        bad = B.copy()
        bad[2, 7, 0] = v
        bo, uo = np.full_like(bad, -77), np.full_like(bad, -77)
        st = np.full(3, -1, dtype=np.int32)
        with pytest.raises(capi.LgsError) as e:
            ctx.bkz_reduce(bad, bo, uo, 4, status=st)
        assert e.value.code == capi.LGS_ERR_INVALID and "2^28" in str(e.value)
        assert np.all(bo == -77) and np.all(uo == -77) and np.all(st == -1)
        bd = torch.as_tensor(bad, device="cuda:0")
        bod, uod = torch.full_like(bd, -77), torch.full_like(bd, -77)
        with pytest.raises(capi.LgsError) as e:
            ctx.bkz_reduce(bd, bod, uod, 4, flags=capi.LGS_DEVICE_PTRS)
        assert e.value.code == capi.LGS_ERR_INVALID and "2^28" in str(e.value)
        assert bool((bod == -77).all()) and bool((uod == -77).all())


def test_insert_guard_gives_status_2_with_the_state_before_the_step(ctx):
    """bkz_oracle.guard_basis(): the first INSERT applies one step of Euclid and the second would
    carry a coordinate of b past 2^28; the result is the state in between, the oracle's."""
    G = bkz_oracle.guard_basis()
    want = bkz_oracle.bkz(G, 12)
    assert (want["status"], want["where"], want["steps"]) == (2, "insert", 1)
    B = np.array(G, dtype=np.int64)
    got = _run(ctx, B[None], 12)
    _equal(got, 0, want, "insert guard")
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0]) and not np.array_equal(got["basis_out"][0], B)


def test_public_layers_end_to_end(ctx):
    from lgs_amd import lattices
    from lgs_amd.reduction import LatticeReduction, bkz_reduce
    rows = lattices.qary_basis(6, 6, 97)
    lat = lattices.SimpleLattice(rows, name="qary12")
    red = lat.bkz(12)
    lam = lat.first_minimum(reduce=True)
    assert int(np.sum(np.asarray(red.basis[0], dtype=np.int64) ** 2)) == round(lam * lam) == 125
    r, U, info = bkz_reduce(rows, 12)
    want = bkz_oracle.reduced("qary12", 12)
    assert info["status"] == 0 and info["truncated"] == 0 and info["nodes"] == want["nodes"]
    assert np.array_equal(U @ rows.astype(np.int64), r) and np.array_equal(r.T, np.array(want["basis_out"]))
    assert np.array_equal(red.basis, r.astype(np.float64))
    rows32 = lattices.qary_basis(16, 16, 3329).astype(np.int64)
    lr = LatticeReduction()
    r6, U6, diag = lr.bkz_reduce(rows32, 6)
    assert sorted(diag) == ["bkz", "block_size", "block_sizes_used", "final_quality", "improvement_factor",
                            "initial_quality", "strategy", "time"]
    assert np.array_equal(U6 @ rows32, r6) and diag["improvement_factor"] >= 1 and diag["block_sizes_used"] == [6]
    rp, Up, dp = lr.bkz_reduce(rows32, 30, progressive=True)
    assert dp["block_sizes_used"] == [20, 30] and len(dp["bkz"]) == 2 and dp["improvement_factor"] >= 1
    assert np.array_equal(Up.astype(np.int64) @ rows32, rp.astype(np.int64))  # the U's compose exactly
    assert abs(lll_oracle.det_bareiss(Up.astype(np.int64).tolist())) == 1
    _, _, d12 = lr.bkz_reduce(rows32, 12)
    _, _, dl = lr.lll_reduce(rows32, delta=0.99)
    assert d12["final_quality"]["max_gs_norm"] <= dl["final_quality"]["max_gs_norm"]
    assert np.array_equal(np.array(bkz_oracle.reduced("qary32", 12)["gs_norm2"]), d12["bkz"][0]["gs_norm2"])


# ---------------------------------------------------------------- dense signed bases and rounding ties
@pytest.mark.parametrize("name,beta,max_tours", bkz_oracle.DENSE_CASES)
def test_parity_on_dense_signed_bases_and_ties(ctx, name, beta, max_tours):
    """Dense bases with entries of both signs at d = 7, 17, 33 and 63, and the two 2 x 2 bases whose
    first mu is +-2.5 (lll_loop is shared: half-away rounding would return another basis)."""
    B = bkz_oracle.basis(name)
    want = bkz_oracle.reduced(name, beta, max_tours=max_tours)
    got = _run(ctx, B[None], beta, max_tours=max_tours)
    print(f"  {name} beta {beta}: status {got['status'][0]}, tours {got['tours'][0]}, insertions "
          f"{got['insertions'][0]} (oracle {want['insertions']}), nodes {got['nodes'][0]} (oracle {want['nodes']}), "
          f"iters {got['iters'][0]} (oracle {want['iters']})")
    _equal(got, 0, want, (name, beta))
    assert np.array_equal(B @ got["U_out"][0], got["basis_out"][0])


def test_library_refuses_parameters_out_of_range_on_either_pointer_kind(capi, ctx):
    """delta, eta and d outside their ranges, straight to the library (Context.bkz_reduce refuses
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
            rc = ctx._L.lgs_bkz_reduce(ctx._h, 2, d, capi._ptr(b), 2, kw.get("delta", 0.99), kw.get("eta", 0.51), 4,
                                       100, 100, capi._ptr(bo), capi._ptr(uo),
                                       capi._outputs(capi.BkzOutputs, *([None] * 8), st, None),
                                       capi.LGS_DEVICE_PTRS if dev else 0)
            assert rc == capi.LGS_ERR_INVALID, (kw, dev)
            word = next(iter(kw))
            assert ("d = " if word == "d" else word) in ctx._L.lgs_last_error().decode(), (kw, dev)
            if dev:
                torch.cuda.synchronize()
            assert bool((bo == -77).all()) and bool((uo == -77).all()) and bool((st == -1).all()), (kw, dev)
    got = _run(ctx, np.eye(4, dtype=np.int64)[None] * 3, 2)  # the context still works
    assert got["status"][0] == 0 and got["iters"][0] == 3


# ---------------------------------------------------------------- the scheduler: batches across launches and chunks
OPTIONAL = COUNTERS + ("status", "gs_norm2")


def _device_run(capi, c, bd, beta, max_tours=1 << 40, only=OPTIONAL):
    """The raw call on device buffers (bd a device tensor), the optional outputs named in `only`
    requested and pre-filled like _run's; returns host arrays."""
    import torch
    n, d, dev = bd.shape[0], bd.shape[1], bd.device
    out = {"basis_out": torch.full_like(bd, -77), "U_out": torch.full_like(bd, -77)}
    for f in only:
        out[f] = (torch.full((n, d), math.nan, dtype=torch.float64, device=dev) if f == "gs_norm2" else
                  torch.full((n,), -1, dtype=torch.int32 if f == "status" else torch.int64, device=dev))
    c.bkz_reduce(bd, out["basis_out"], out["U_out"], beta, max_tours=max_tours, flags=capi.LGS_DEVICE_PTRS,
                 **{f: out[f] for f in only})
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in out.items()}


def _host_run(c, bases, beta, only):
    """_run with only the optional outputs named in `only`."""
    b = np.ascontiguousarray(bases, dtype=np.int64)
    n, d = b.shape[0], b.shape[1]
    out = {"basis_out": np.full((n, d, d), -77, dtype=np.int64), "U_out": np.full((n, d, d), -77, dtype=np.int64)}
    for f in only:
        out[f] = (np.full((n, d), np.nan) if f == "gs_norm2" else
                  np.full(n, -1, dtype=np.int32 if f == "status" else np.int64))
    c.bkz_reduce(b, out["basis_out"], out["U_out"], beta, **{f: out[f] for f in only})
    return out


def _equal_all(got, wants, what):
    """Every entry of a batched result against its own oracle result, whole arrays at a time."""
    conv = {id(o): bkz_oracle.as_arrays(o) for o in wants}
    for f in got:
        w = np.stack([conv[id(o)][f] for o in wants])
        assert got[f].dtype == w.dtype and got[f].shape == w.shape, (what, f)
        diff = np.flatnonzero((got[f].view(np.int64) != w.view(np.int64)).reshape(len(wants), -1).any(axis=1)) \
            if f == "gs_norm2" else np.flatnonzero((got[f] != w).reshape(len(wants), -1).any(axis=1))
        assert diff.size == 0, (what, f, "entries", diff[:8], got[f][diff[0]], w[diff[0]])


def _launches(c, capi):
    return c.timing_get(capi.KERNEL_CVP_ENUM)[1]


def _bounds(wants, lll_slice, node_slice):
    """least and most of test_forced_slices_span_launches, the max over the batch in place of one basis."""
    li = [-(-w["iters"] // lll_slice) for w in wants]
    ln = [-(-w["nodes"] // node_slice) for w in wants]
    return 1 + max(max(1, a, b) for a, b in zip(li, ln)), max(2 + a + b for a, b in zip(li, ln))


@pytest.mark.parametrize("max_tours", [1 << 40, bkz_oracle.MIXED_MAX_TOURS])
def test_mixed_batch_spans_launches(capi, monkeypatch, max_tours):
    """bkz_oracle.mixed_batch() -- ten bases of d = 17 at beta = 6, suspended inside LLL runs and
    inside enumerations a different number of times each, the early leavers in the middle of the
    batch -- on the hooks library at LLL_SLICE iterations and BKZ_SLICE nodes per launch: every
    field of every entry equals its own oracle, counters included, with host and device pointers;
    with max_tours = MIXED_MAX_TOURS status 4, 0 and 3 meet in one call.  Timer 9 lies within the
    bounds of the single-basis test, and equals the set-up launch plus the launches
    bkz_oracle.schedule derives from the kernel's two budgets for the entry that needs most."""
    import torch
    monkeypatch.setenv("LGS_TEST_BKZ_SLICE", str(bkz_oracle.BKZ_SLICE))
    monkeypatch.setenv("LGS_TEST_LLL_SLICE", str(bkz_oracle.LLL_SLICE))
    hctx = capi.Context(0, hooks=True)
    B, want = bkz_oracle.mixed_batch(), bkz_oracle.mixed_reduced(max_tours)
    least, most = _bounds(want, bkz_oracle.LLL_SLICE, bkz_oracle.BKZ_SLICE)
    exact = 1 + max(bkz_oracle.schedule(w)[0] for w in want)
    hctx.timing_enable(True)
    got = _run(hctx, B, bkz_oracle.MIXED_BETA, max_tours=max_tours)
    launches = _launches(hctx, capi)
    print(f"  max_tours {max_tours}: {launches} launches (between {least} and {most}, schedule {exact}), "
          f"status {list(got['status'])}")
    _equal_all(got, want, "host")
    for k, w in enumerate(want):
        _equal(got, k, w, ("host", k))
    assert 3 < least <= launches <= most and launches == exact
    bd = torch.as_tensor(B, device="cuda:0")
    hctx.timing_enable(True)
    gd = _device_run(capi, hctx, bd, bkz_oracle.MIXED_BETA, max_tours)
    assert _launches(hctx, capi) == launches
    _equal_all(gd, want, "device")
    assert torch.equal(bd, torch.as_tensor(B, device="cuda:0"))  # the input is not written
    _equal_all(_device_run(capi, hctx, bd.flip(0).contiguous(), bkz_oracle.MIXED_BETA, max_tours), want[::-1],
               "device, reversed")
    hctx.close()


@pytest.mark.parametrize("library,dev", [("product", False), ("product", True), ("hooks", False), ("hooks", True)])
def test_more_bases_than_one_chunk(capi, monkeypatch, library, dev):
    """lll_oracle.chunk_batch() at beta = 2: 1030 bases of d = 3, six more than the scheduler's
    chunk, a singular one on either side of the boundary.  Every optional output at once, then
    status alone, then gs_norm2 alone (each offset is its own code); on the hooks library two LLL
    iterations per launch, so that the second chunk's live list spans launches too.  Timer 9: per
    chunk the set-up launch and the launches of the entry that needs most."""
    import torch
    lll_slice = 1 << 12
    if library == "hooks":
        lll_slice = 2
        monkeypatch.setenv("LGS_TEST_LLL_SLICE", "2")
    c = capi.Context(0, hooks=library == "hooks")
    B, idx = lll_oracle.chunk_batch()
    B0 = B.copy()
    R = bkz_oracle.chunk_reduced()
    want = [R[v] for v in idx]
    parts = ([R[v] for v in idx[:1024]], [R[v] for v in idx[1024:]])
    least, most = (sum(x) for x in zip(*(_bounds(p, lll_slice, 1 << 16) for p in parts)))
    exact = sum(1 + max(bkz_oracle.schedule(w, lll_slice, 1 << 16)[0] for w in p) for p in parts)
    assert (least == exact == 4) if library == "product" else (exact > 8)
    bd = torch.as_tensor(B, device="cuda:0") if dev else None
    for only in (OPTIONAL, ("status",), ("gs_norm2",)):
        c.timing_enable(True)
        got = _device_run(capi, c, bd, 2, only=only) if dev else _host_run(c, B, 2, only)
        launches = _launches(c, capi)
        assert least <= launches <= most and launches == exact, (only, launches, least, most, exact)
        assert sorted(got) == sorted(("basis_out", "U_out") + tuple(only))
        _equal_all(got, want, (library, dev, only))
    assert np.array_equal(bd.cpu().numpy() if dev else B, B0)  # the input is not written
    c.close()
