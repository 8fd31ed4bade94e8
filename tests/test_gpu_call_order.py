"""No entry point disturbs another on a shared context.

A context's thirty compute entry points share a few dozen device buffers and several pieces of
remembered state ("What a context remembers between calls"); include/lgs.h
promises that an output "is a function of its own inputs alone".  Every other GPU test runs an
entry point on a fresh context or on one that only ever ran that entry point.  Here every probe
of tests/call_order_cases.py runs right behind every other one, between pipelined lgs_imhk
calls, between lgs_exact_table and lgs_exact_sample, behind sticky state and error exits, and
beside another context -- and must give what it gives alone.
"""
import time

import numpy as np
import pytest

import call_order_cases as C

pytestmark = pytest.mark.gpu

NAMES = [r.name for r in C.ROWS]


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    _capi.load_library()
    return _capi


def _sync():
    import torch
    torch.cuda.synchronize()


_faulted = []


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    """A case that leaves the device in an error state ends the module: no later case starts
    work on a faulted device."""
    if _faulted:
        pytest.exit(f"an earlier case left the device in an error state: {_faulted[0]}", 3)
    yield
    try:
        _sync()
    except Exception as e:  # (torch reports a HIP fault as a RuntimeError)
        _faulted.append(e)
        raise


def _counters(ctx, capi):
    """The Klein launches by kernel, the q-panel skips and the decisions redone at the
    reference-order mean so far (host getters: no device work).  Two runs of a call whose
    counters agree took the same path through the Klein kernels; where they differ -- another
    kernel, another skip pattern, or sub-panels replayed in the reference's order in one run
    and not in the other, which the certificate's cap on sum |z_j| decides (z1cap: the basis'
    estimate for the first launch after lgs_set_basis, then twice the largest sums seen) -- the
    log weights are the same sums evaluated at means that differ
    in rounding (include/lgs.h, LGS_LOGW_BOUND: the blocked kernels' weights are defined up to
    a bound), and compare to rtol 1e-12 instead of bit for bit."""
    return tuple(ctx.counter(k) for k in (capi.LGS_COUNTER_LAUNCH_EXACT, capi.LGS_COUNTER_LAUNCH_VALU,
                                          capi.LGS_COUNTER_LAUNCH_MFMA_FP64, capi.LGS_COUNTER_LAUNCH_MFMA_I8,
                                          capi.LGS_COUNTER_QSKIP, capi.LGS_COUNTER_RESOLVED))


def _delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


_solo_cache = {}


def _solo_for(capi, sname):
    """The rows valid for a subject, each on a fresh context after lgs_set_basis and
    lgs_set_decoder only (computed once, read-only): out[row, size, dev], the counters of the
    call under out["_counters", ...], the tolerances of its summation-order keys under
    out["tol", row, size]."""
    if sname in _solo_cache:
        return _solo_cache[sname]
    s = C.subject(sname)
    rows = [r for r in C.ROWS if r.valid_for(s["d"])]
    out = {}
    t0 = time.perf_counter()
    for r in rows:
        for size in C.SIZES:
            for dev in r.kinds:
                ctx = C.fresh_context(capi, s)
                c0 = _counters(ctx, capi)
                res = r(ctx, capi, size, dev)
                for a in res.values():
                    a.setflags(write=False)
                out[r.name, size, dev] = res
                out["_counters", r.name, size, dev] = _delta(c0, _counters(ctx, capi))
                ctx.close()
    abs_z = C.abs_z_sums(s, C.SIZES["large"]["nt"]) if sname == "int12" else None
    for r in rows:
        for size in C.SIZES:
            out["tol", r.name, size] = C.sum_tolerances(r.name, out[r.name, size, r.kinds[0]], abs_z)
    # the two pointer kinds of a row are the same call: they agree before anything is mixed
    for r in rows:
        for size in C.SIZES:
            if len(r.kinds) == 2:
                a, b = out[r.name, size, False], out[r.name, size, True]
                shared = {k for k in a if k in b}
                bad = C.same({k: a[k] for k in shared}, {k: b[k] for k in shared}, r, out["tol", r.name, size])
                assert not bad, f"{r.name} {size}: host and device pointers differ in {bad}"
    print(f"solo references on {sname}: {time.perf_counter() - t0:.1f} s")
    _solo_cache[sname] = out
    return out


@pytest.fixture(scope="module")
def solo(capi):
    return _solo_for(capi, "int12")


def _x_kind(X, want):
    return want if want in X.kinds else X.kinds[0]


# ---------------------------------------------------------------- (a) every pair
@pytest.mark.parametrize("xname", NAMES)
def test_every_probe_after(capi, solo, xname):
    """X, then E, on one context, for every probe E in both pointer kinds: X large before E
    small (E works in buffers X left bigger, beside X's stale tails) with the other pointer kind,
    and X small before E large (E reallocates what X used) with the same kind.  Nothing
    synchronises between the two calls beyond what they do themselves (the counters read
    between them are host variables).  E equals its run alone: bit for bit, the enumeration's
    floating-point sums within twice the header's summation-order bound, and the log weights of
    lgs_klein / lgs_imhk bit for bit when the call's counters are those of the run alone
    (_counters)."""
    _every_pair(capi, solo, xname, C.subject())


def _every_pair(capi, solo, xname, s):
    X = C.BY_NAME[xname]
    ctx = C.fresh_context(capi, s)
    failures = []
    t0 = time.perf_counter()
    for E in C.ROWS:
        if not E.valid_for(s["d"]):
            continue
        for edev in E.kinds:
            for xsize, esize in (("large", "small"), ("small", "large")):
                xdev = _x_kind(X, (not edev) if xsize == "large" else edev)
                xrun, xcollect = X.prepare(ctx, capi, xsize, xdev)
                erun, ecollect = E.prepare(ctx, capi, esize, edev)
                _sync()
                c0 = _counters(ctx, capi)
                xrun()
                c1 = _counters(ctx, capi)
                erun()
                got = ecollect()
                c2 = _counters(ctx, capi)
                bad = C.same(got, solo[E.name, esize, edev], E, solo["tol", E.name, esize],
                             logw_bitwise=_delta(c1, c2) == solo["_counters", E.name, esize, edev])
                if bad:
                    failures.append((f"{xname}[{xsize},{'dev' if xdev else 'host'}] -> "
                                     f"{E.name}[{esize},{'dev' if edev else 'host'}]", bad))
                bad = C.same(xcollect(), solo[xname, xsize, xdev], X, solo["tol", xname, xsize],
                             logw_bitwise=_delta(c0, c1) == solo["_counters", xname, xsize, xdev])
                if bad:  # (X itself ran behind the previous E)
                    failures.append((f"{E.name} -> {xname}[{xsize},{'dev' if xdev else 'host'}]", bad))
    ctx.close()
    print(f"after {xname} on {s['name']}: {time.perf_counter() - t0:.2f} s")
    for f in failures:
        print("  differs:", *f)
    assert not failures, f"{len(failures)} pairs differ (listed above), first {failures[0]}"


def test_first_launch_runs_under_the_basis_cap(capi, solo, monkeypatch):
    """The one dependence on earlier calls that the pairs above show, pinned: the certificate's
    cap on sum |z_j| (lgs_ctx::z1cap) is lgs_set_basis's loose estimate for the first Klein
    launch and twice the largest sums seen afterwards (fold_counters).  lgs_klein three times on
    one context: the first call is the run alone; the second has the same launches and skips,
    fewer decisions redone at the reference-order mean, the same z and v, and log weights equal
    to rounding; the third is the second bit for bit with the same counters.  With the cap held
    far below every sum (hooks build, LGS_TEST_Z1CAP_SCALE: every sub-panel is replayed) the
    first and the second call agree bit for bit: the cap, not what the buffers held, makes the
    difference."""
    row = C.BY_NAME["klein_blocks"]
    key = ("klein_blocks", "large", False)

    def three(ctx, n=3):
        runs, c = [], _counters(ctx, capi)
        for _ in range(n):
            r = row(ctx, capi, "large", False)
            c, d = _counters(ctx, capi), _delta(c, _counters(ctx, capi))
            runs.append((r, d))
        ctx.close()
        return runs
    (a, da), (b, db), (c, dc) = three(C.fresh_context(capi))
    assert da == solo[("_counters",) + key] and not C.same(a, solo[key], row)
    print(f"resolved: first {da[5]}, second {db[5]}, third {dc[5]}")
    assert da[:5] == db[:5] and da[5] > db[5]
    assert not C.same(b, a, row, logw_bitwise=False) and b["z"].tobytes() == a["z"].tobytes()
    assert dc == db and not C.same(c, b, row)
    monkeypatch.setenv("LGS_TEST_Z1CAP_SCALE", "1e-9")
    try:
        (ha, dha), (hb, dhb) = three(C.fresh_context(capi, hooks=True), 2)
    finally:
        monkeypatch.delenv("LGS_TEST_Z1CAP_SCALE")
    print(f"resolved under a cap of 1e-9 times the estimate: {dha[5]}, {dhb[5]}")
    assert dha == dhb and dha[5] >= da[5] and not C.same(hb, ha, row)
    assert not C.same(ha, a, row, logw_bitwise=False)


@pytest.mark.parametrize("xname", ["klein_blocks", "klein_ragged", "imhk_ref", "imhk_wl", "imhk_ex"])
def test_every_probe_after_a_klein_launch_with_history(capi, xname):
    """The same pairs on klein_ntru128 behind the entry points that launch the Klein kernels: at
    d = 128 the int8-digit far field runs and leaves an int16 history, which B z reads in place
    of the store (int12's single panel has no far field and never leaves one).  A B z that took
    the history of X's launch for E's coefficients -- the same store address, other contents --
    shows here as a wrong v of lgs_lattice_points and of the decoders."""
    _every_pair(capi, _solo_for(capi, "ntru128"), xname, C.subject("ntru128"))


# ---------------------------------------------------------------- (b) between pipelined lgs_imhk calls
NC, STEPS, CALLS = 256, 8, 4
PIPE_SEED = 777
PIPE_CONFIGS = [(wl, blocks) for wl in (False, True) for blocks in (1, 2)]


def _refusal(name):
    """The enumeration family at d = 128 > LGS_CVP_MAX_D: the library's LGS_ERR_INVALID (the
    binding's own check is bypassed; the refusal comes before any buffer is read)."""
    def call(ctx, capi):
        s = ctx.subject
        t = np.ascontiguousarray(s["T"][:3])
        r2 = np.full(3, 1.0)
        L, h, p = ctx._L, ctx._h, capi._ptr
        rc = {"closest_vector": lambda: L.lgs_closest_vector(h, 3, p(t), None, 100, None, None, None, None, 0),
              "gaussian_mass": lambda: L.lgs_gaussian_mass(h, 3, p(t), 12.0, p(r2), None, 100, None, None, 0),
              "ball_points": lambda: L.lgs_ball_points(h, 3, p(t), p(r2), 100, 0, None, None, None, None, 0),
              "exact_table": lambda: L.lgs_exact_table(h, 3, p(t), 12.0, p(r2), None, 100, 100, None, 0)}[name]()
        assert rc == capi.LGS_ERR_INVALID, (name, rc)
    return call


def _set_stream_away_and_back(ctx, capi):
    import torch
    ctx.set_stream(None)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def _timing(ctx, capi):
    ctx.timing_enable(True)


def _set_decoder(ctx, capi):
    ctx.set_decoder(Q=ctx.subject["Q"], Binv=ctx.subject["Binv"])


def _disturbers():
    """name -> (prepare(ctx, capi) -> run) for the pipelined case: every probe valid at d = 128
    in each pointer kind (device pointers: large, host pointers: small), the refusals of the
    enumeration family, and the three host-state calls."""
    out = {}
    for r in C.ROWS:
        if not r.valid_for(128):
            for n in r.symbols:
                if n != "lgs_exact_sample":
                    out[f"refused:{n[4:]}"] = (lambda ctx, capi, n=n[4:]: (lambda: _refusal(n)(ctx, capi)))
            continue
        for dev in r.kinds:
            def prep(ctx, capi, r=r, dev=dev):
                run, collect = r.prepare(ctx, capi, "large" if dev else "small", dev)

                def go():
                    run()
                    collect()  # (its own non-degeneracy; the disturber's values are checked in (a))
                return go
            out[f"{r.name}:{'dev' if dev else 'host'}"] = prep
    for name, fn in (("set_stream", _set_stream_away_and_back), ("timing_enable", _timing),
                     ("set_decoder", _set_decoder)):
        out[name] = (lambda ctx, capi, fn=fn: (lambda: fn(ctx, capi)))
    return out


DISTURBERS = _disturbers()
# documented as touching no loaded basis (and the diagnostics, which read caller data only): a
# look-ahead launch must survive them
MUST_SURVIVE = tuple(f"{n}:{k}" for n in C.NO_BASIS for k in ("host", "dev")) + ("timing_enable",)


def _pipelined(capi, wl, blocks, disturb=None, pipeline=True, lookahead=True):
    """Four lgs_imhk calls of 8 steps on 256 chains of klein_ntru128, device pointers on a
    caller's torch stream, max_proposals for `blocks` blocks per call; `disturb` right behind
    the second call (its buffers are prepared before that call, so that it runs right behind
    the call, while the look-ahead launch the second call left is pending).  Returns the outputs
    of every call, the Klein launches of the lgs_imhk calls alone, all counters and the lean
    B z tiles."""
    import torch
    s = C.subject("ntru128")
    d = s["d"]
    ctx = C.fresh_context(capi, s, max_proposals=NC * STEPS // blocks, pipeline=pipeline, lookahead=lookahead)
    dev = C.DEVICE
    st = dict(z=torch.zeros((NC, d), dtype=torch.int32, device=dev), lw=torch.zeros(NC, dtype=torch.float64, device=dev),
              init=torch.zeros(NC, dtype=torch.int32, device=dev), acc=torch.zeros(NC, dtype=torch.int64, device=dev),
              mom=torch.zeros(2 * d, dtype=torch.int64, device=dev))
    f = capi.LGS_DEVICE_PTRS | ((capi.LGS_WANG_LING | capi.LGS_EXACT_ORDER) if wl else 0)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    outs, own = [], 0
    try:
        with torch.cuda.stream(stream):
            go = None
            for call in range(CALLS):
                if call == 1 and disturb is not None:
                    go = disturb(ctx, capi)
                zs = torch.zeros((NC, STEPS, d), dtype=torch.int32, device=dev)
                vs = torch.zeros((NC, STEPS, d), dtype=torch.float64, device=dev)
                c0 = _counters(ctx, capi)
                ctx.imhk(PIPE_SEED, 0, NC, 1 + call * STEPS, STEPS, 1, st["z"], st["lw"], st["init"], st["acc"],
                         z_samples=zs, v_samples=vs, moments=st["mom"], flags=f)
                own += sum(_delta(c0, _counters(ctx, capi))[:4])
                if call == 1 and go is not None:
                    go()
                outs.append(dict({k: t.clone() for k, t in st.items()}, zs=zs, vs=vs))
        torch.cuda.synchronize()
        outs = [{k: t.cpu().numpy() for k, t in o.items()} for o in outs]
        return dict(outs=outs, launches=own, counters=_counters(ctx, capi), tiles=ctx.bz_tiles())
    finally:
        torch.cuda.synchronize()
        ctx.close()


_pipe_cache = {}


def _pipe_refs(capi, oracle, wl, blocks):
    """Per configuration, once: the four calls on Context(pipeline=False, lookahead=False), the
    undisturbed pipelined run with its liveness, and the oracle's first 16 chains after calls
    three and four."""
    key = (wl, blocks)
    if key not in _pipe_cache:
        s = C.subject("ntru128")
        plain = _pipelined(capi, wl, blocks, pipeline=False, lookahead=False)
        nolook = _pipelined(capi, wl, blocks, lookahead=False)
        pipe = _pipelined(capi, wl, blocks)
        assert plain["launches"] == nolook["launches"]
        hits = plain["launches"] + CALLS - pipe["launches"]
        # liveness: the int8-digit MFMA kernel ran (reference weights; LGS_EXACT_ORDER has its
        # own kernel), the int8-digit B z computed the lattice points, and calls two to four
        # each started from the previous call's look-ahead launch.  (Lean tiles, bz_tiles()[0],
        # cannot occur at d = 128: the one 128-row tile of B holds the block H off its
        # diagonal, lgs_bz_host.h; tests/test_gpu_bz_lean.py reaches them at d = 1024.)
        print(f"pipelined wl={wl} blocks={blocks}: counters {pipe['counters']} tiles {pipe['tiles']} hits {hits}; "
              f"plain counters {plain['counters']}")
        assert pipe["counters"][0 if wl else 3] > 0 and sum(pipe["tiles"]) > 0 and hits == CALLS - 1
        orc = {}
        for call in (2, 3):
            z, lw, acc = oracle.imhk_parallel(s["R"], s["cprime"], s["B"], s["sigma"], 16, (call + 1) * STEPS,
                                              seed=PIPE_SEED, mode=oracle.IMHK_WANG_LING if wl else oracle.IMHK_REFERENCE)
            orc[call] = (z, acc)
        _compare_pipe(pipe, plain, orc, "undisturbed")
        _pipe_cache[key] = (plain, pipe, orc)
    return _pipe_cache[key]


def _same_kernels(a, b):
    """The launch and skip counters of two runs show the same kernels and skip pattern: the
    same Klein kernels ran, q-panels were skipped in both or in neither (the counts themselves
    differ by the look-ahead launches), and neither replayed a decision in the reference's
    order."""
    return tuple(x > 0 for x in a[:5]) == tuple(x > 0 for x in b[:5]) and a[5] == b[5] == 0


def _compare_pipe(got, ref, orc, what):
    bitwise = _same_kernels(got["counters"], ref["counters"])
    for call in (2, 3):
        g, r = got["outs"][call], ref["outs"][call]
        for k in r:
            if k == "lw" and not bitwise:
                np.testing.assert_allclose(g[k], r[k], rtol=1e-12, atol=0, err_msg=f"{what}: call {call + 1} {k}")
            else:
                assert g[k].tobytes() == r[k].tobytes(), f"{what}: call {call + 1}: {k} differs"
        z, acc = orc[call]
        assert np.array_equal(g["z"][:16], z) and np.array_equal(g["acc"][:16], acc), f"{what}: call {call + 1} vs oracle"
        assert g["z"].any() and g["vs"].any()


@pytest.mark.parametrize("dname", sorted(DISTURBERS))
def test_between_pipelined_imhk_calls(capi, oracle, dname):
    """A disturber between the second and the third of four pipelined lgs_imhk calls, while the
    look-ahead Klein launch for the third is on the Klein stream: calls three and four equal the
    same calls on Context(pipeline=False, lookahead=False) with nothing in between, and the
    oracle's chains; reference weights and Wang-Ling weights (LGS_EXACT_ORDER: the certified
    Wang-Ling accept is host-checked and never pipelined, imhk_impl's `early`), one block per
    call and two.

    Look-ahead launches count when enqueued, every call enqueues one, and a call that starts
    from the previous call's launch makes one launch less, so over the four calls
    hits = launches(lookahead=False) + calls - launches(pipelined), counting the lgs_imhk
    calls' own launches only (lookahead() and imhk_impl's spec_hit branch in lgs_capi.hip);
    three on the undisturbed run.  A disturber that leaves the look-ahead alive leaves it
    three: it then ran while the look-ahead launch was pending."""
    survived = []
    for wl, blocks in PIPE_CONFIGS:
        plain, pipe, orc = _pipe_refs(capi, oracle, wl, blocks)
        got = _pipelined(capi, wl, blocks, disturb=DISTURBERS[dname])
        _compare_pipe(got, plain, orc, f"{dname} wl={wl} blocks={blocks}")
        hits = plain["launches"] + CALLS - got["launches"]
        assert CALLS - 2 <= hits <= CALLS - 1
        survived.append(hits == CALLS - 1)
    print(f"look-ahead after {dname}: {'survived' if all(survived) else 'discarded' if not any(survived) else survived}")
    if dname in MUST_SURVIVE:
        assert all(survived), f"{dname} touches no loaded basis but the look-ahead launch was discarded"


# ---------------------------------------------------------------- (c) exact_table -> X -> exact_sample
TABLE_ROW = "exact_table+exact_sample"


@pytest.mark.parametrize("xname", [n for n in NAMES if n != TABLE_ROW] + ["set_basis"])
def test_table_survives(capi, solo, xname):
    """lgs_exact_table, X, lgs_exact_sample: the draws equal the undisturbed ones for every X
    (small table under a large X, large table under a small X) -- but lgs_exact_table itself,
    which replaces the table by definition, and lgs_set_basis, after which lgs_exact_sample
    returns LGS_ERR_STATE."""
    row = C.BY_NAME[TABLE_ROW]
    ctx = C.fresh_context(capi)
    for tsize, xsize in (("small", "large"), ("large", "small")):
        for dev in row.kinds:
            b = C.Bufs(dev)
            table, sample, check = C.exact_calls(ctx, capi, C.SIZES[tsize], b, capi.LGS_DEVICE_PTRS if dev else 0)
            if xname == "set_basis":
                _sync()
                table()
                C.load_subject(ctx, ctx.subject)
                with pytest.raises(capi.LgsError) as e:
                    sample()
                assert e.value.code == capi.LGS_ERR_STATE
                continue
            X = C.BY_NAME[xname]
            xdev = _x_kind(X, not dev)
            xrun, xcollect = X.prepare(ctx, capi, xsize, xdev)
            _sync()
            table()
            xrun()
            sample()
            got = b.collect()
            check(got)
            bad = C.same(got, solo[TABLE_ROW, tsize, dev], row, solo["tol", TABLE_ROW, tsize])
            assert not bad, f"table[{tsize}] -> {xname}[{xsize}] -> sample: {bad}"
            # (X's log weights to rounding here: test_every_probe_after holds them to the counters)
            bad = C.same(xcollect(), solo[xname, xsize, xdev], X, solo["tol", xname, xsize], logw_bitwise=False)
            assert not bad, f"table[{tsize}] -> {xname}[{xsize}]: {bad}"
    ctx.close()


# ---------------------------------------------------------------- (d) sticky state and error exits
def _overflowed(capi, monkeypatch):
    """The basis of test_gpu_parity.test_int8_digit_far_field_overflow_falls_back loaded and
    sampled (|z| > 32767: the launch is redone, the wider store and the fp64 far field stay
    with the context), then the subject basis."""
    rng = np.random.default_rng(5)
    d = 96
    R = np.triu(rng.normal(size=(d, d)) * 0.01, 1)
    R[np.diag_indices(d)] = rng.uniform(0.5, 2.0, d)
    cp = rng.normal(size=d) * 4e4
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, None, 3.0)
    r = ctx.klein_host(11, 0, 256, want_z=True, want_v=False)
    assert np.abs(r["z"]).max() > 32767 and ctx.fallbacks() > 0
    C.load_subject(ctx, C.subject())
    return ctx


def _halved(capi, monkeypatch):
    """A max_props halved after LGS_ERR_NOMEM (hooks build, LGS_TEST_NOMEM_ABOVE): a 256-chain,
    64-step lgs_imhk whose block-sized buffers are refused above 64 KiB runs in smaller blocks,
    and the smaller cap stays with the context -- the same call then makes more Klein launches
    than on a fresh context."""
    import torch
    ctx = C.fresh_context(capi, hooks=True)
    d, nc, T = ctx.d, 256, 64

    def call(c):
        st = [torch.zeros((nc, d), dtype=torch.int32, device=C.DEVICE), torch.zeros(nc, dtype=torch.float64, device=C.DEVICE),
              torch.zeros(nc, dtype=torch.int32, device=C.DEVICE), torch.zeros(nc, dtype=torch.int64, device=C.DEVICE)]
        torch.cuda.synchronize()
        c0 = _counters(c, capi)
        c.imhk(21, 0, nc, 1, T, 1, *st, flags=capi.LGS_DEVICE_PTRS)
        torch.cuda.synchronize()
        return sum(_delta(c0, _counters(c, capi))[:4]), st[0].cpu().numpy()
    monkeypatch.setenv("LGS_TEST_NOMEM_ABOVE", str(64 << 10))
    try:
        call(ctx)
    finally:
        monkeypatch.delenv("LGS_TEST_NOMEM_ABOVE")
    after, z1 = call(ctx)
    ref = C.fresh_context(capi)
    fresh, z0 = call(ref)
    ref.close()
    assert after > fresh and np.array_equal(z0, z1), (after, fresh)
    return ctx


def _errors(capi, monkeypatch):
    """An API error return of each family, as the suite provokes them elsewhere: a flag the
    entry point does not take (LGS_ERR_INVALID), a NaN target (LGS_ERR_NONFINITE: the kernels
    ran and set their flag word), LGS_ERR_OVERFLOW in lgs_klein_bases (|z| near 10^12 / 3)."""
    ctx = C.fresh_context(capi)
    s = ctx.subject
    d = ctx.d
    t = np.ascontiguousarray(s["T"][:5])
    z, v = np.empty((5, d), dtype=np.int32), np.empty((5, d))
    bad = t.copy()
    bad[3, 2] = np.nan
    r2 = np.ascontiguousarray(s["radius2"][:5])
    calls = [
        (capi.LGS_ERR_INVALID, lambda: ctx.klein_targets(1, 0, t, z, v, None, capi.LGS_WANG_LING)),
        (capi.LGS_ERR_NONFINITE, lambda: ctx.klein_targets(1, 0, bad, z, v, None, 0)),
        (capi.LGS_ERR_INVALID, lambda: ctx.klein_decode(1, 0, t, 3, z, v, flags=capi.LGS_LOGW_BOUND)),
        (capi.LGS_ERR_NONFINITE, lambda: ctx.imhk_targets(1, 0, bad, 4, z, v)),
        (capi.LGS_ERR_INVALID, lambda: ctx._ck(ctx._L.lgs_closest_vector(ctx._h, 5, capi._ptr(t), None, 100, None, None,
                                                                         None, None, capi.LGS_EXACT_ORDER))),
        (capi.LGS_ERR_NONFINITE, lambda: ctx.closest_vector(bad, 100, None, z, v)),
        (capi.LGS_ERR_INVALID, lambda: ctx._ck(ctx._L.lgs_klein_bases(
            ctx._h, 1, 0, 2, 3, 2, 3, capi._ptr(np.zeros((2, 3, 3))), capi._ptr(np.zeros((2, 2, 3))),
            capi._ptr(np.ones(2)), 10, None, None, None, capi.LGS_COORD_MAJOR))),
        (capi.LGS_ERR_NONFINITE, lambda: ctx.gaussian_mass(bad, C.MASS_SIGMA, r2, None, 100, mass=np.empty(5))),
        (capi.LGS_ERR_OVERFLOW, lambda: ctx.klein_bases(
            1, 0, np.array([[[3.0, 1.0], [0.0, 2.0]]]), np.array([[[1e12, 0.25]]]), np.array([2.0]), 3,
            z_out=np.empty((1, 1, 2), dtype=np.int32))),
    ]
    turn = [0]

    def provoke():
        """The next error of the list, in turn: one right before every probe, so that each probe
        follows errors of every kind (any four in a row hold a flag-setting one)."""
        code, fn = calls[turn[0] % len(calls)]
        turn[0] += 1
        with pytest.raises(capi.LgsError) as e:
            fn()
        assert e.value.code == code, (e.value, code)
    for _ in calls:
        provoke()
    return ctx, provoke


@pytest.mark.parametrize("state", [_overflowed, _halved, _errors], ids=["overflow", "halved_max_props", "api_errors"])
def test_after_sticky_state(capi, solo, monkeypatch, state):
    """Every loaded-basis probe behind a sticky state or an error exit equals its run alone.
    Log weights are bit for bit when the probe's Klein launches and q-panel skips are those of
    the run alone, and within rtol 1e-12 where the counters show another kernel or skip pattern
    (after the overflow the context keeps the 32-bit store and the fp64 far field)."""
    ctx = state(capi, monkeypatch)
    ctx, before = ctx if isinstance(ctx, tuple) else (ctx, None)
    failures = []
    for E in C.ROWS:
        if not E.basis:
            continue
        for dev in E.kinds:
            for size in C.SIZES:
                run, collect = E.prepare(ctx, capi, size, dev)
                _sync()
                if before is not None:
                    before()
                c0 = _counters(ctx, capi)
                run()
                bitwise = _delta(c0, _counters(ctx, capi)) == solo["_counters", E.name, size, dev]
                bad = C.same(collect(), solo[E.name, size, dev], E, solo["tol", E.name, size], logw_bitwise=bitwise)
                if bad:
                    failures.append((E.name, size, "dev" if dev else "host", bad))
    ctx.close()
    for f in failures:
        print("  differs:", *f)
    assert not failures, f"{len(failures)} probes differ (listed above), first {failures[0]}"


# ---------------------------------------------------------------- (e) two contexts
def _two_contexts(capi, which):
    """Contexts on klein_qary128 and klein_ntru128, each on its own torch stream; per round one
    device-pointer lgs_imhk (pipelined, with a look-ahead) and one lgs_klein on each context of
    `which`, round robin, nothing synchronised between the contexts."""
    import torch
    dev = C.DEVICE
    runs = {}
    for name in which:
        s = C.subject(name)
        ctx = C.fresh_context(capi, s)
        stream = torch.cuda.Stream(device=dev)
        d = s["d"]
        with torch.cuda.stream(stream):
            st = [torch.zeros((NC, d), dtype=torch.int32, device=dev), torch.zeros(NC, dtype=torch.float64, device=dev),
                  torch.zeros(NC, dtype=torch.int32, device=dev), torch.zeros(NC, dtype=torch.int64, device=dev)]
            mom = torch.zeros(2 * d, dtype=torch.int64, device=dev)
        runs[name] = dict(ctx=ctx, stream=stream, st=st, mom=mom, d=d, keep=[])
    torch.cuda.synchronize()
    for r in runs.values():
        r["ctx"].set_stream(r["stream"].cuda_stream)
    for rnd in range(3):
        for name in which:
            r = runs[name]
            with torch.cuda.stream(r["stream"]):
                vs = torch.zeros((NC, STEPS, r["d"]), dtype=torch.float64, device=dev)
                r["ctx"].imhk(5, 0, NC, 1 + rnd * STEPS, STEPS, 1, *r["st"], v_samples=vs, moments=r["mom"],
                              flags=capi.LGS_DEVICE_PTRS)
                z = torch.zeros((509, r["d"]), dtype=torch.int32, device=dev)
                v = torch.zeros((509, r["d"]), dtype=torch.float64, device=dev)
                r["ctx"].klein(6, 1000 * rnd, 509, z, v, None, capi.LGS_DEVICE_PTRS)
                r["keep"] += [vs, z, v]
    torch.cuda.synchronize()
    out = {}
    for name, r in runs.items():
        out[name] = [t.cpu().numpy() for t in r["st"] + [r["mom"]] + r["keep"]]
        r["ctx"].close()
    return out


def test_two_contexts_interleaved(capi):
    both = _two_contexts(capi, ("qary128", "ntru128"))
    for name in ("qary128", "ntru128"):
        alone = _two_contexts(capi, (name,))[name]
        assert len(alone) == len(both[name])
        for k, (a, b) in enumerate(zip(both[name], alone)):
            assert a.tobytes() == b.tobytes(), f"{name}: output {k} differs beside the other context"
        assert alone[0].any() and alone[-1].any()
