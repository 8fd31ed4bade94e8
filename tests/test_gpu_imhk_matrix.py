"""lgs_imhk_trace / lgs_imhk_ex against the per-step oracle in every context option, weight
mode, store width, layout, pointer kind and call shape of tests/imhk_matrix_cases.py.

The accept pass, the Wang-Ling certificate, the moments pass, the kept-state gather, the
final-state gather and B z all read what the Klein launch left behind, and each LGS_CTX_*
option leaves something else: a 32-bit store (store32) instead of the 16-bit store that
widens, ocml weights (samplez_libm) instead of tabulated ones, bounds from the 16-row kernels
(panel16), no int16 history (far_fp64, panel16).  include/lgs.h promises the same outputs
bit for bit in each; tests/test_imhk_matrix_host.py checks the table's completeness and
the premises of its cases on the CPU.

Every case requests every output its flags allow: z_samples (row-major state only:
lgs_imhk refuses it with LGS_COORD_MAJOR), v_samples (device pointers; host calls use
lgs_lattice_points on the kept states; the R-only basis has no lattice points), moments,
logw_samples and accepted; device-pointer calls also lgs_imhk_ex's zk_samples and (with
lattice points) vnorm2_samples, so they are lgs_imhk_ex calls and the host ones lgs_imhk_trace
(lgs_imhk is lgs_imhk_trace without the two per-step outputs: one body, csrc/lgs_capi.hip).

Against the per-step oracle (imhk_matrix_cases.per_step_oracle), bit for bit: final z and
accepts; state_init = the step of the chain's last accepted proposal + 2 (2 after the initial
draw alone, 1 for a caller-set state never replaced); z_samples = the states after steps thin,
2 thin, ... counted across a split; accepted = the per-step flags; moments = the integer sums
over the kept states; v_samples = kept B^T, vnorm2_samples its squared norms, zk_samples
coefficient 0 of the kept states.  logw_state and logw_samples: rtol 1e-9
(test_gpu_parity.test_imhk_matches_oracle).  Across the variants of one (basis, weights,
chains, steps, thin, first_chain, initial state): every integer output equal to the default
context's host int32 row-major single call, log weights rtol 1e-12 (tests/test_gpu_call_order.py).

Oracle rows: every chain of every case but r130 with 256 chains, where every 4th chain (64 of
256) is compared: three of 154 cases leave out 3/4 of their rows, 576 of the table's 18 795
chains (3.1 %).  Every chain is compared across variants.

The launch counters prove the kernel: every case's Klein launches are those its block sizes
select (n % 64: VALU; n % 256: fp64-far-field MFMA; else the int8-digit kernel on 32-row
int8 contexts), no int8-digit launch under far_fp64 or panel16, no reference-order launch,
no fallback -- but the default context with wide carried states through device pointers,
which must fall back (it widens its store) where store32 must not.
"""
import time

import numpy as np
import pytest

import imhk_matrix_cases as C
from test_gpu_kernel_matrix import LAUNCH_KINDS, _launches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ZK_INDEX = 0  # (the coefficient the wide states hold 50000 in)
_t0 = time.time()
_report = {"oracle": 0.0, "variants": 0.0, "resolved": {}, "compared": 0, "cases": 0}


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctxs(capi):
    """One context per option set, created on first use and closed with the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = capi.Context(0, max_proposals=C.MAX_PROPOSALS, **C.CONTEXTS[name])
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _load(ctx, oracle, name):
    if getattr(ctx, "_matrix_basis", None) != name:
        ctx.set_basis(*C.basis(oracle, name))
        ctx._matrix_basis = name
    return ctx


def _kind(c, n):
    if n % 64:
        return "VALU"
    if n % 256 == 0 and not ("panel" in C.CONTEXTS[c.ctx] or "far" in C.CONTEXTS[c.ctx]):
        return "MFMA_I8"
    return "MFMA_FP64"


def expected_launches(c):
    """Per call: the (gated) launch of the initial draws, n_chains proposals, and one launch
    per block."""
    s = C.SHAPES[c.shape]
    T = C.block_length(s)
    want = dict.fromkeys(LAUNCH_KINDS, 0)
    for part in s.split:
        want[_kind(c, s.nc)] += 1
        for t0 in range(0, part, T):
            want[_kind(c, s.nc * min(T, part - t0))] += 1
    return tuple(want[k] for k in LAUNCH_KINDS)


def _imhk(capi, ctx, oracle, c, monkeypatch=None, bound_scale=None):
    """The case's calls on ctx (its basis loaded).  Returns the outputs in one form -- row-major
    int64 states, kept states n_chains x n_keep x d -- and the counters of these calls."""
    R, cp, B, sigma = C.basis(oracle, c.basis)
    s = C.SHAPES[c.shape]
    nc, d = s.nc, R.shape[0]
    zt = np.int64 if c.z64 else np.int32
    if c.dev:
        import torch

    def buf(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a).to(DEV) if c.dev else a

    def host(a):
        return None if a is None else (a.cpu().numpy() if c.dev else a)

    start = C.initial_state(oracle, c)
    z0 = np.zeros((nc, d), dtype=zt) if start is None else start[0].astype(zt)
    z = buf(z0.T if c.cm else z0)
    lw = buf(np.zeros(nc) if start is None else start[1])
    init = buf(np.full(nc, 0 if start is None else 1, dtype=np.int32))
    acc, mom = buf(np.zeros(nc, dtype=np.int64)), buf(np.zeros(2 * d, dtype=np.int64))
    flags = ((capi.LGS_WANG_LING if c.wl else 0) | (capi.LGS_Z64 if c.z64 else 0) |
             (capi.LGS_COORD_MAJOR if c.cm else 0) | (capi.LGS_DEVICE_PTRS if c.dev else 0))
    want_zs, want_vs = not c.cm, c.dev and B is not None
    parts = []
    stream = None
    if c.stream:
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=DEV)
        ctx.set_stream(stream.cuda_stream)
    if bound_scale is not None:
        monkeypatch.setenv("LGS_TEST_WL_BOUND_SCALE", repr(bound_scale))
    _launches(capi, ctx, reset=True)
    for k in (capi.LGS_COUNTER_ACCEPT_RESOLVED, capi.LGS_COUNTER_WL_MISMATCH, capi.LGS_COUNTER_QSKIP):
        ctx.counter(k, reset=True)
    ctx.fallbacks(reset=True)
    try:
        def calls():
            t = C.FIRST_STEP
            for n in s.split:
                k = n // s.thin
                p = dict(zs=buf(np.zeros((nc, k, d), dtype=zt)) if want_zs else None,
                         vs=buf(np.zeros((nc, k, d))) if want_vs else None,
                         lws=buf(np.zeros((nc, k))), accd=buf(np.zeros((nc, n), dtype=np.uint8)),
                         vn=buf(np.zeros((nc, k))) if want_vs else None,
                         zk=buf(np.zeros((nc, k), dtype=np.int64)) if c.dev else None)
                # (zk_samples makes the call lgs_imhk_ex; without it, it is lgs_imhk_trace)
                ctx.imhk(C.SEED, s.first_chain, nc, t, n, s.thin, z, lw, init, acc, z_samples=p["zs"],
                         v_samples=p["vs"], moments=mom, flags=flags, logw_samples=p["lws"], accepted=p["accd"],
                         vnorm2_samples=p["vn"], zk_samples=p["zk"], zk_index=ZK_INDEX)
                parts.append(p)
                t += n
        if stream is not None:
            with torch.cuda.stream(stream):
                calls()
        else:
            calls()
    finally:
        if c.dev:
            torch.cuda.synchronize()
        if stream is not None:
            ctx.set_stream(None)
        if bound_scale is not None:
            monkeypatch.delenv("LGS_TEST_WL_BOUND_SCALE")
    out = {k: (np.concatenate([host(p[k]) for p in parts], axis=1) if parts[0][k] is not None else None)
           for k in ("zs", "vs", "lws", "accd", "vn", "zk")}
    if out["zs"] is not None:
        out["zs"] = out["zs"].astype(np.int64)
        if out["vs"] is None and B is not None:  # host pointers: the kept states' lattice points
            out["vs"] = ctx.lattice_points(out["zs"].reshape(-1, d)).reshape(out["zs"].shape)
    zh = host(z)
    out.update(z=(zh.T if c.cm else zh).astype(np.int64), lw=host(lw), init=host(init), acc=host(acc), mom=host(mom),
               launches=_launches(capi, ctx), fallbacks=ctx.fallbacks(),
               resolved=ctx.counter(capi.LGS_COUNTER_ACCEPT_RESOLVED),
               mismatch=ctx.counter(capi.LGS_COUNTER_WL_MISMATCH), qskip=ctx.counter(capi.LGS_COUNTER_QSKIP))
    return out


_runs = {}


def _run(capi, ctxs, oracle, c):
    """One run per case (read-only afterwards).  The wide states make a context's store
    choice sticky, so those cases run on a context of their own."""
    if c not in _runs:
        if c.init == "wide":
            ctx = capi.Context(0, max_proposals=C.MAX_PROPOSALS, **C.CONTEXTS[c.ctx])
            try:
                ctx.set_basis(*C.basis(oracle, c.basis))
                _runs[c] = _imhk(capi, ctx, oracle, c)
            finally:
                ctx.close()
        else:
            _runs[c] = _imhk(capi, _load(ctxs(c.ctx), oracle, c.basis), oracle, c)
    return _runs[c]


def _rel(a, b):
    return float((np.abs(a - b) / np.abs(b)).max())


def _check_vs_oracle(oracle, c, r):
    """Every output of the run against the per-step oracle of the case's oracle rows.
    Returns the largest relative log-weight error."""
    rows = list(C.oracle_rows(c))
    o = C.case_oracle(oracle, c)
    e = C.expected(c, o)
    B = C.basis(oracle, c.basis)[2]
    assert np.array_equal(r["z"][rows], o["z"])
    assert np.array_equal(r["acc"][rows], o["accepts"])
    assert (r["init"] != 0).all()
    assert np.array_equal(r["init"][rows], e["init"])
    assert np.array_equal(r["accd"][rows], o["accepted"])
    assert set(np.unique(r["accd"])) <= {0, 1} and np.array_equal(r["accd"].sum(axis=1), r["acc"])
    if r["zs"] is not None:
        assert np.array_equal(r["zs"][rows], e["kept"])
    if r["vs"] is not None:
        assert np.array_equal(r["vs"][rows], e["kept"].astype(np.float64) @ B.T)
    if r["zk"] is not None:
        assert np.array_equal(r["zk"][rows], e["kept"][:, :, ZK_INDEX])
    if r["vn"] is not None:  # (integers below 2^53: exact)
        v = e["kept"].astype(np.float64) @ B.T
        assert np.array_equal(r["vn"][rows], (v * v).sum(axis=2))
    if len(rows) == len(r["acc"]):
        assert np.array_equal(r["mom"], e["moments"])
    elif r["zs"] is not None:  # (oracle rows left out: the sums over the run's own kept states)
        flat = r["zs"].reshape(-1, r["zs"].shape[2])
        assert np.array_equal(r["mom"], np.concatenate([flat.sum(0), (flat * flat).sum(0)]))
    worst = max(_rel(r["lw"][rows], o["lw_final"]), _rel(r["lws"][rows], e["lw_kept"]))
    np.testing.assert_allclose(r["lw"][rows], o["lw_final"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(r["lws"][rows], e["lw_kept"], rtol=1e-9, atol=0)
    return worst


def _check_counters(c, r):
    launches = dict(zip(LAUNCH_KINDS, r["launches"]))
    assert launches["EXACT"] == 0, launches
    assert r["mismatch"] == 0
    opts = C.CONTEXTS[c.ctx]
    if "far" in opts or "panel" in opts:
        assert launches["MFMA_I8"] == 0, launches  # the fp64 far field / the 16-row kernels
    widens = c.init == "wide" and c.dev and "store32" not in opts
    if widens:
        assert r["fallbacks"] >= 1  # the carried states did not fit the 16-bit store
    else:
        assert r["fallbacks"] == 0
    if c.stream:
        # (pipelined calls also count their look-ahead launches): the kernel of the blocks ran
        want = dict(zip(LAUNCH_KINDS, expected_launches(c)))
        assert all(launches[k] >= want[k] for k in LAUNCH_KINDS), (launches, want)
    if "qskip" in opts:
        assert r["qskip"] == 0
    elif c.ctx == "default" and c.basis == "skip100" and not c.wl and c.shape == "c256-thin1":
        assert r["qskip"] > 0  # (what the no_qskip case turns off)
    elif not widens:
        assert r["launches"] == expected_launches(c), (launches, expected_launches(c))


@pytest.mark.parametrize("c", C.CASES, ids=C.CASE_IDS)
def test_case_vs_oracle(capi, ctxs, oracle, c):
    r = _run(capi, ctxs, oracle, c)
    worst = _check_vs_oracle(oracle, c, r)
    _check_counters(c, r)
    _report["oracle"] = max(_report["oracle"], worst)
    _report["cases"] += 1
    _report["compared"] += len(C.oracle_rows(c))
    note = ""
    if c.wl and ("panel" in C.CONTEXTS[c.ctx] or "samplez_libm" in C.CONTEXTS[c.ctx]):
        _report["resolved"][c.ctx] = _report["resolved"].get(c.ctx, 0) + r["resolved"]
        note = f", {r['resolved']} accept decisions resolved in the reference order"
    print(f"  max rel logw err vs oracle {worst:.2e}{note}")


def _same_chains(r, w, rows=slice(None), what=""):
    """Integer outputs equal, log weights rtol 1e-12; returns the largest relative difference."""
    worst = 0.0
    for k in ("z", "acc", "init", "accd", "zs", "vs", "vn", "zk"):
        if r[k] is not None and w[k] is not None:
            assert np.array_equal(r[k], w[k][rows]), (what, k)
    for k in ("lw", "lws"):
        worst = max(worst, _rel(r[k], w[k][rows]))
        np.testing.assert_allclose(r[k], w[k][rows], rtol=1e-12, atol=0, err_msg=f"{what} {k}")
    return worst


@pytest.mark.parametrize("key", C.GROUPS, ids=["-".join(str(x) for x in k) for k in C.GROUPS])
def test_variants_equal_the_default_context(capi, ctxs, oracle, key):
    """Every chain, not only the oracle's: each context option, store width, layout, pointer
    kind and split of the group gives the chains of the default context's host, int32,
    row-major single call, moments included."""
    base = _run(capi, ctxs, oracle, C.base_case(key))
    worst = 0.0
    for c in C.CASES:
        if C.group_key(c) == key and c != C.base_case(key):
            r = _run(capi, ctxs, oracle, c)
            worst = max(worst, _same_chains(r, base, what=C.case_id(c)))
            assert np.array_equal(r["mom"], base["mom"]), C.case_id(c)
    _report["variants"] = max(_report["variants"], worst)
    print(f"  max rel logw difference from the default context {worst:.2e}")


@pytest.mark.parametrize("basis,wl", [("r40", False), ("r40", True), ("r100", False), ("skip100", True)])
def test_first_chain_5_is_rows_5_up_of_first_chain_0(capi, ctxs, oracle, basis, wl):
    a = _run(capi, ctxs, oracle, C._c("default", basis, wl, "c64-first5"))
    b = _run(capi, ctxs, oracle, C._c("default", basis, wl, "c69"))
    worst = _same_chains(a, b, rows=slice(5, None), what="first_chain 5")
    _report["variants"] = max(_report["variants"], worst)


def test_forced_resolution_panel16(capi, oracle, monkeypatch):
    """The hooks library widens every Wang-Ling bound by LGS_TEST_WL_BOUND_SCALE (each stays a
    bound).  At 3e3, the scale of tests/test_gpu_wl_accept.py, bounds of 1e-13 at d = 40 still
    certify nearly every decision; at 1e16 no bound certifies anything, so every decision
    with a nonzero bound is recomputed in the reference order: the chains are the oracle's."""
    c = C.FORCED
    counts = {}
    ctx = capi.Context(0, max_proposals=C.MAX_PROPOSALS, hooks=True, **C.CONTEXTS[c.ctx])
    try:
        ctx.set_basis(*C.basis(oracle, c.basis))
        for scale in C.FORCED_SCALES:
            r = _imhk(capi, ctx, oracle, c, monkeypatch, scale)
            _check_vs_oracle(oracle, c, r)
            _check_counters(c, r)
            counts[scale] = r["resolved"]
    finally:
        ctx.close()
    print(f"  accept decisions resolved in the reference order by bound scale: {counts}")
    _report["resolved"]["forced"] = counts
    assert counts[max(C.FORCED_SCALES)] > 0


def test_report():
    """The module's figures (run with -s)."""
    print(f"\n  {_report['cases']} device cases, {_report['compared']} chains against the oracle; "
          f"max rel logw err vs oracle {_report['oracle']:.2e}, across variants {_report['variants']:.2e}; "
          f"resolved decisions {_report['resolved']}; {time.time() - _t0:.1f} s since import")
