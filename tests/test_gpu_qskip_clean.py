"""The q-panel skip's clean state: a wave that skips a panel whose
coefficient rows, int16 history blocks and zero flags still hold the skip's values from
its previous launch into the same buffers stores nothing.  After every launch memory must
hold what it held when every skip stored: these tests drive one store through
skip / no-skip / skip per block and through every event that takes the stored state's
validity away, and compare every output with the C oracle, with a context that skips but
has nothing to elide (a fresh store) or with a context that never skips (qskip=False), bit
for bit -- but for the log weights against the last one, which differ in the last bits with
or without this state (a skipped row's weight term).  lgs_qskip_elided shows
that the path ran.

The basis is test_gpu_kernel_matrix._skip_basis's (d = 100, rows 4..67 pinned by
R_ii = 1e4, one rare row in panel 2) with one large entry R[50, 90]: it sets panel 1's
skip bound ||z_W||^2 <= qz2 (lgs_set_basis, restated in _qz2 below) inside the range of
the free top panel's squared norms, so a 256-sample block skips panel 1 exactly when its
largest such norm stays below the bound -- some blocks of a launch do, some do not, and
which ones changes with first_sample.  The skip pattern is computed from the oracle's z;
the library's LGS_COUNTER_QSKIP must equal it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, SIGMA, RARE = 100, 3.0, 25
ROW, COL, BOUND = 50, 90, 400.0  # R[ROW, COL] chosen for qz2[panel 1] ~ BOUND
SEED = 20260
PINNED = np.delete(np.arange(4, 68), RARE - 4)
TOP = slice(68, 100)  # panel 0: the free rows whose norm the skip of panel 1 tests


def _basis(bound=BOUND):
    rng = np.random.default_rng(17)
    d = D
    R = np.zeros((d, d))
    for i in range(d):
        R[i, i] = float(rng.integers(2, 4))
        if i < d - 1:
            R[i, rng.integers(i + 1, d, 3)] += rng.choice([-1.0, 1.0], 3)
    cp = np.round(rng.normal(size=d) * 8.0) / 4.0
    pinned = np.arange(4, 68)
    R[pinned, pinned] = 1e4
    R[RARE, RARE + 1:] = 0.0
    R[RARE, RARE] = SIGMA / 0.25
    cp[pinned] = 0.0
    R[ROW, COL] = np.floor(0.4999 * 1e4 / np.sqrt(bound))
    return R, cp


def _qz2(R, cp):
    """lgs_set_basis's bound for panel 1 (rows 36..67; W = the free rows 68..99 above it)."""
    g = 1.1 * D * 2.0 ** -53
    zmin = np.inf
    for i in range(36, 68):
        Gi = np.sqrt((R[i, TOP] ** 2).sum()) * (1 + 1e-13)
        is_ = R[i, i] / SIGMA
        theta = 0.5 - 745.2 / (is_ * is_ * (1 - 1e-12)) - 1e-9
        num = theta * R[i, i] * (1 - 1e-12) - abs(cp[i])
        assert num > 0
        zmin = min(zmin, num / ((1 + g) * Gi) if Gi > 0 else np.inf)
    return zmin * zmin * (1 - 1e-12)


_cache = {}


def _oracle_run(oracle, first, n):
    """The oracle's samples [first, first + n) and, per 256-sample block, whether the block
    skips panel 1 (every sample's ||z_W||^2 below the bound, with a margin the bound's
    rounding cannot cross: the norms are integers)."""
    key = (first, n)
    if key not in _cache:
        R, cp = _basis()
        o = oracle.klein(R, cp, SIGMA, n, seed=SEED, first_sample=first, B=R)
        z = o["z"]
        assert np.abs(z).max() <= 32639 and not z[:, PINNED].any()
        q = _qz2(R, cp)
        m = (z[:, TOP].astype(np.int64) ** 2).sum(1)
        assert (np.abs(m - q) > 0.25).all()
        nb = n // 256
        skip = (m[:nb * 256].reshape(nb, 256) <= q).all(1) if n % 256 == 0 else np.zeros(0, dtype=bool)
        _cache[key] = (o, skip)
    return _cache[key]


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


def _klein(capi, c, first, n):
    z = np.empty((n, D), dtype=np.int32)
    v = np.empty((n, D))
    lw = np.empty(n)
    c.counter(capi.LGS_COUNTER_QSKIP, reset=True)
    c.qskip_elided(reset=True)
    c.klein(SEED, first, n, z, v, lw, 0)
    return z.astype(np.int64), v, lw, c.counter(capi.LGS_COUNTER_QSKIP), c.qskip_elided()


def _run_launches(capi, oracle, launches, max_proposals=0):
    """lgs_klein launches (first, n) into one context: z and v against the oracle, the log
    weights against the oracle (a sample of them) and, bit for bit, against a context that
    skips but has no state to trust (a fresh store; a skipped row's weight term differs
    from a computed one in the last bits, so the context that never skips is no reference
    for them); both counters against the skip pattern of the oracle's z, chunk by chunk
    (a chunk's panel is clean when the previous chunk had the same shape and skipped it
    too)."""
    R, cp = _basis()
    c = capi.Context(0, max_proposals=max_proposals)
    counts = []
    try:
        c.set_basis(R, cp, R, SIGMA)
        prev_m, prev_skip = None, None
        for first, n in launches:
            o, _ = _oracle_run(oracle, first, n)
            z, v, lw, nskip, nel = _klein(capi, c, first, n)
            ref = capi.Context(0, max_proposals=n)  # one chunk: nothing to elide
            try:
                ref.set_basis(R, cp, R, SIGMA)
                z0, v0, lw0, nskip0, nel0 = _klein(capi, ref, first, n)
            finally:
                ref.close()
            print(f"launch first={first} n={n}: qskip={nskip} elided={nel}")
            assert np.array_equal(z, o["z"]) and np.array_equal(v, o["v"])
            assert np.array_equal(z, z0) and np.array_equal(v, v0) and np.array_equal(lw, lw0)
            assert nskip0 == nskip and nel0 == 0
            # (B = R: the frame of R is the lattice's own, so the centre behind c' is c' itself)
            want = np.array([oracle.log_weight(R, cp, R, SIGMA, o["z"][k], center=cp)
                             for k in range(0, n, max(n // 32, 1))])
            np.testing.assert_allclose(lw[::max(n // 32, 1)], want, rtol=1e-9, atol=1e-9)
            want_skip = want_el = 0
            chunk = min(n, max_proposals or n)
            for off in range(0, n, chunk):
                m = min(chunk, n - off)
                if m % 256:  # not whole workgroups: another kernel, which drops the state
                    prev_m = None
                    continue
                skip = _oracle_run(oracle, first + off, m)[1]
                want_skip += 4 * int(skip.sum())
                if prev_m == m:
                    want_el += 4 * int((skip & prev_skip).sum())
                prev_m, prev_skip = m, skip
            assert (nskip, nel) == (want_skip, want_el)
            counts.append((nskip, nel))
    finally:
        c.close()
    return counts


def test_dirty_clean_dirty(capi, oracle):
    """Four launches of 4096 samples into one store.  Conditions on the oracle: between
    consecutive launches some block goes skip -> no skip, some no skip -> skip and some
    skips twice.  No elision in the first launch, some later."""
    firsts = (0, 4096, 8192, 0)
    skips = [_oracle_run(oracle, f, 4096)[1] for f in firsts]
    for a, b in zip(skips, skips[1:]):
        assert (a & ~b).any() and (~a & b).any() and (a & b).any()
    counts = _run_launches(capi, oracle, [(f, 4096) for f in firsts])
    assert counts[0][1] == 0 and all(nel > 0 for _, nel in counts[1:])


def test_ragged_n_and_changed_batches(capi, oracle):
    """A ragged n (the VALU kernel: no skip, and it drops the state); batch size and
    offset changed between launches (the state starts over each time); a launch split
    into chunks by max_proposals (the second chunk finds the first one's state)."""
    counts = _run_launches(capi, oracle, [(0, 4096), (0, 4000), (0, 4096), (0, 4096)])
    assert [nel > 0 for _, nel in counts] == [False, False, False, True]
    counts = _run_launches(capi, oracle, [(0, 4096), (512, 2048), (512, 2048), (4096, 4096), (4096, 4096)])
    assert [nel > 0 for _, nel in counts] == [False, False, True, False, True]
    counts = _run_launches(capi, oracle, [(0, 4096), (4096, 4096)], max_proposals=2048)
    assert all(nel > 0 for _, nel in counts)


# ------------------------------------------------------------------ lgs_imhk
NC, STEPS, TB = 256, 8, 4  # 256 chains x 8 steps per call, in blocks of 4 steps (max_proposals)
IMHK_SEED = 611


def _imhk(capi, qskip, *, pipeline=True, hooks=False, event=None, calls=4, tb=TB):
    """`calls` lgs_imhk calls (reference weights, device pointers on a caller's stream: the
    blocks of tb steps are pipelined through the buffer sets unless pipeline=False), `event`
    between the second and the third.  Returns every output of every call and the elision
    count."""
    import torch
    R, cp = _basis()
    dev = "cuda:0"
    c = capi.Context(0, max_proposals=NC * tb, pipeline=pipeline, qskip=qskip, hooks=hooks)
    outs = []
    try:
        c.set_basis(R, cp, R, SIGMA)
        z = torch.zeros((NC, D), dtype=torch.int32, device=dev)
        lw = torch.zeros(NC, dtype=torch.float64, device=dev)
        init = torch.zeros(NC, dtype=torch.int32, device=dev)
        acc = torch.zeros(NC, dtype=torch.int64, device=dev)
        mom = torch.zeros(2 * D, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=dev)
        c.set_stream(s.cuda_stream)
        f = capi.LGS_DEVICE_PTRS
        c.qskip_elided(reset=True)
        with torch.cuda.stream(s):
            first = 1
            for call in range(calls):
                nc, fl, zz = NC, f, z
                if call == 2 and event == "klein":
                    c.klein_host(SEED, 0, 1024)
                elif call == 2 and event == "set_basis":
                    R2, cp2 = _basis(300.0)
                    c.set_basis(R2, cp2, R2, SIGMA)
                elif call == 2 and event == "z64":  # this call with an int64 state and store
                    fl, zz = f | capi.LGS_Z64, z.to(torch.int64)
                elif call == 2 and event == "nc":  # this call on the first 128 chains only
                    nc = NC // 2
                elif call == 2 and event == "reinit":  # three chains start over: initial draws
                    init[:3] = 0
                zs = torch.zeros((nc, STEPS, D), dtype=zz.dtype, device=dev)
                vs = torch.zeros((nc, STEPS, D), dtype=torch.float64, device=dev)
                c.imhk(IMHK_SEED, 0, nc, first, STEPS, 1, zz[:nc], lw[:nc], init[:nc], acc[:nc], z_samples=zs,
                       v_samples=vs, moments=mom, flags=fl)
                s.synchronize()
                if zz is not z:
                    z.copy_(zz.to(torch.int32))
                first += STEPS
                outs.append({k: t.cpu().numpy().copy() for k, t in dict(z=z, lw=lw, init=init, acc=acc, mom=mom,
                                                                        zs=zs, vs=vs).items()})
        torch.cuda.synchronize()
        return outs, c.qskip_elided(), c.counter(capi.LGS_COUNTER_QSKIP)
    finally:
        c.close()


_imhk_ref = {}


def _never_skips(capi, event, tb=TB):
    if (event, tb) not in _imhk_ref:
        outs, nel, nskip = _imhk(capi, False, event=event, tb=tb)
        assert nel == 0 and nskip == 0
        _imhk_ref[event, tb] = outs
    return _imhk_ref[event, tb]


def _same(a, b):
    """Every output equal; the weights to rounding (a skipped row's weight term is taken
    at mu = 0, a computed one at the blocked mean: 1e-15 apart)."""
    assert len(a) == len(b)
    for call, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if k == "lw":
                np.testing.assert_allclose(x[k], y[k], rtol=1e-12, atol=0)
            else:
                assert np.array_equal(x[k], y[k]), (call, k)


@pytest.mark.parametrize("how", ["pipelined", "no-pipeline", "cu-split"])
def test_imhk_equals_context_that_never_skips(capi, how, monkeypatch):
    """Four calls of two blocks each: the blocks alternate between the buffer sets (or, with
    pipeline=False, share the context's store; or run on the CU-masked Klein stream the
    hooks build forces).  States, weights, accepts, moments, kept coefficients and lattice
    points equal the context that never skips; the pinned coordinates of the final states
    (read from the int16 history) and of the kept coefficients (gathered from the store) are
    the zeros that the elided panels left in place."""
    import torch
    if how == "cu-split":
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        monkeypatch.setenv("LGS_PIPE_CU_RESERVE", str(ncu // 8))
    outs, nel, nskip = _imhk(capi, True, pipeline=how != "no-pipeline", hooks=how == "cu-split")
    if how == "cu-split":
        monkeypatch.delenv("LGS_PIPE_CU_RESERVE")
    print(f"{how}: qskip={nskip} elided={nel}")
    _same(outs, _never_skips(capi, None))
    assert 0 < nel < nskip
    for o in outs:
        assert not o["z"][:, PINNED].any() and not o["zs"][:, :, PINNED].any()
        assert o["z"][:, TOP].any() and o["acc"].sum() > 0


_undisturbed = {}


@pytest.mark.parametrize("event,pipeline", [("klein", True), ("set_basis", True), ("z64", True), ("nc", True),
                                            ("klein", False), ("nc", False)])
def test_imhk_state_invalidated(capi, event, pipeline):
    """Between the second and the third call: an lgs_klein call on the context, another
    basis of the same d, a call with an int64 store, a call with another chain count.  The
    calls after it equal the context that never skips, and fewer skips are elided than in
    the undisturbed run of the same calls: the event took the state's validity away.
    Pipelined, lgs_klein writes the context's own store, which no block's launch trusts
    (the sets keep their state: the count stays); with pipeline=False it writes the very
    store the next block would have trusted."""
    if pipeline not in _undisturbed:
        _undisturbed[pipeline] = _imhk(capi, True, pipeline=pipeline)[1]
    outs, nel, nskip = _imhk(capi, True, event=event, pipeline=pipeline)
    print(f"{event}, pipeline={pipeline}: qskip={nskip} elided={nel} undisturbed={_undisturbed[pipeline]}")
    _same(outs, _never_skips(capi, event))
    assert nskip > 0
    if event == "klein" and pipeline:
        assert nel == _undisturbed[pipeline]
    else:
        assert nel < _undisturbed[pipeline]


@pytest.mark.parametrize("event", [None, "reinit"])
def test_imhk_one_block_per_call_without_pipeline(capi, event):
    """pipeline=False with one block per call: every call first enqueues the gated launch of
    the initial draws into the same store as its block.  That launch writes only if some
    chain is uninitialised, which the device alone knows: the block's launch trusts the
    state unless the gate's word is set.  Calls two to four find no chain to draw (their
    skips are elided); with three chains reset before the third call its initial draws do
    overwrite the store, and the block's launch starts over."""
    outs, nel, nskip = _imhk(capi, True, pipeline=False, event=event, tb=STEPS)
    print(f"one block per call, {event}: qskip={nskip} elided={nel}")
    _same(outs, _never_skips(capi, event, STEPS))
    assert 0 < nel < nskip
