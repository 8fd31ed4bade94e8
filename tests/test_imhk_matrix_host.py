"""Host side of tests/test_gpu_imhk_matrix.py (no GPU).

1. The per-step oracle of tests/imhk_matrix_cases.py (lgs_oracle.imhk resumed one step at a
   time) gives the trace, the final state, weight and accept counts of one whole call; it is
   the reference of `accepted`, `logw_samples` and state_init.
2. The premises of every case, on the oracle alone: Wang-Ling cases accept and reject,
   reference-weight cases accept everything, a caller-set state decides its first step
   differently, the wide states leave int16, the SampleZ-kind basis has varying normalisers.
3. Completeness of the table: every LGS_CTX_* option Context.__init__ offers has a case in
   both weight modes, and the table uses every flag and shape class it is there for.
"""
import inspect

import numpy as np
import pytest

import imhk_matrix_cases as C


# ------------------------------------------------------------------ 1. the per-step oracle
@pytest.mark.parametrize("wl", [False, True], ids=["ref", "wl"])
@pytest.mark.parametrize("first_chain,first_step", [(0, 1), (2 ** 32 - 9, 1), (5, 7)])
def test_per_step_oracle_is_the_whole_call(oracle, wl, first_chain, first_step):
    R, cp, B, sigma = C.basis(oracle, "r40")
    nc, S = 9, 20
    o = C.per_step_oracle(oracle, R, cp, B, sigma, nc, S, seed=C.SEED, first_chain=first_chain,
                          first_step=first_step, wl=wl)
    w = oracle.imhk(R, cp, B, sigma, nc, S, seed=C.SEED, first_chain=first_chain, first_step=first_step,
                    mode=oracle.IMHK_WANG_LING if wl else oracle.IMHK_REFERENCE, trace=True)
    assert np.array_equal(o["states"], w["trace"])
    assert np.array_equal(o["z"], w["z"]) and np.array_equal(o["z"], o["states"][:, -1])
    assert np.array_equal(o["lw_final"], w["lw"]) and np.array_equal(o["lw_final"], o["lw"][:, -1])
    assert np.array_equal(o["accepts"], w["accepts"]) and np.array_equal(o["accepts"], o["accepted"].sum(axis=1))
    assert set(np.unique(o["accepted"])) <= {0, 1}
    if not wl:  # (the reference weight is one constant up to rounding)
        return
    # a step that accepted is a step whose weight is the proposal's: the state's weight
    # changes only there (no accepted proposal here has its state's weight bit for bit)
    start = oracle.imhk(R, cp, B, sigma, nc, 0, seed=C.SEED, first_chain=first_chain,
                        mode=oracle.IMHK_WANG_LING if wl else oracle.IMHK_REFERENCE)
    lw = np.concatenate([start["lw"][:, None], o["lw"]], axis=1)
    assert np.array_equal(lw[:, 1:] != lw[:, :-1], o["accepted"].astype(bool))


def test_per_step_oracle_resumes_a_caller_set_state(oracle):
    c = C._c("default", "r40", True, "c64", init="set")
    R, cp, B, sigma = C.basis(oracle, "r40")
    z0, lw0 = C.initial_state(oracle, c)
    s = C.SHAPES[c.shape]
    o = C.case_oracle(oracle, c)
    st = {"z": z0.copy(), "lw": lw0.copy(), "init": np.ones(s.nc, dtype=np.int32),
          "accepts": np.zeros(s.nc, dtype=np.int64)}
    w = oracle.imhk(R, cp, B, sigma, s.nc, s.steps, seed=C.SEED, first_chain=s.first_chain, first_step=C.FIRST_STEP,
                    state=st, mode=oracle.IMHK_WANG_LING, trace=True)
    assert np.array_equal(o["states"], w["trace"]) and np.array_equal(o["accepts"], w["accepts"])
    assert np.array_equal(o["lw_final"], w["lw"])


def test_oracle_rows_chain_by_chain_are_the_batch_rows(oracle):
    """At d = 130 with 256 chains the oracle runs every 4th chain on its own: the same rows."""
    c = C._c("default", "r130", True, "c256")
    rows = C.oracle_rows(c)
    assert rows.step == 4 and len(rows) == 64
    o = C.case_oracle(oracle, c)
    R, cp, B, sigma = C.basis(oracle, "r130")
    s = C.SHAPES[c.shape]
    w = C.per_step_oracle(oracle, R, cp, B, sigma, 12, s.steps, seed=C.SEED, first_chain=s.first_chain,
                          first_step=C.FIRST_STEP, wl=True)
    for k in ("states", "lw", "accepted"):
        assert np.array_equal(o[k][:3], w[k][0:12:4]), k


# ------------------------------------------------------------------ 2. premises
@pytest.mark.parametrize("key", C.GROUPS, ids=[str(k) for k in C.GROUPS])
def test_premises_of_every_case(oracle, key):
    c = C.base_case(key)
    s = C.SHAPES[c.shape]
    o = C.case_oracle(oracle, c)
    e = C.expected(c, o)
    n = len(C.oracle_rows(c))
    assert n >= 16  # no case compares fewer chains with the oracle
    assert o["states"].shape == (n, s.steps, C.basis(oracle, c.basis)[0].shape[0])
    if c.wl:
        assert 0 < o["accepts"].sum() < n * s.steps
        assert (o["accepts"] < s.steps).any()  # (a chain rejects)
        kept = e["kept"]
        assert (kept[:, 1:] != kept[:, :-1]).any()  # a kept state differs from its predecessor
    else:
        assert o["accepts"].sum() == n * s.steps  # reference-mode acceptance is exactly 1
        assert (e["init"] == C.FIRST_STEP + s.steps - 1 + 2).all()
    # int32 buffers hold every state, and (but for the wide case) so does the 16-bit store and
    # the int8-digit kernel's history
    assert np.abs(o["states"]).max() <= (70000 if c.init == "wide" else 32639)


def test_caller_set_state_decides_differently(oracle):
    c = C._c("default", "r40", True, "c64", init="set")
    z0, lw0 = C.initial_state(oracle, c)
    o = C.case_oracle(oracle, c)
    u = C.case_oracle(oracle, c._replace(init=None))
    R, cp, B, sigma = C.basis(oracle, c.basis)
    s = C.SHAPES[c.shape]
    # lattice points off the centre: their weights are neither the initial draws' nor the
    # first proposals' (the state after step 1 of a chain that accepted there)
    start = oracle.imhk(R, cp, B, sigma, s.nc, 0, seed=C.SEED, first_chain=s.first_chain, mode=oracle.IMHK_WANG_LING)
    assert (z0 != start["z"]).any(axis=1).all()
    assert (np.abs(z0 - cp @ np.linalg.inv(R).T) > 2 * sigma / np.diag(R)).any(axis=1).all()
    assert (lw0 != start["lw"]).all()
    took = o["accepted"][:, 0] == 1
    assert took.any() and (o["lw"][took, 0] != lw0[took]).all()
    # the first step is decided differently from the same chain started uninitialised
    differ = o["accepted"][:, 0] != u["accepted"][:, 0]
    assert differ.any(), "every first step decided as from the initial draw"
    # a chain that never accepts keeps state_init = 1, the others the step of their last accept
    e = C.expected(c, o)
    assert ((e["init"] == 1) == ~o["accepted"].any(axis=1)).all()


def test_wide_states_leave_int16(oracle):
    """The default store widens on the carried states of its first block (LGS_CTX_STORE32 starts
    wide); some chains keep the wide state over a kept step while others have moved."""
    for dev in (False, True):
        assert {c.ctx for c in C.CASES if c.init == "wide" and c.dev == dev} == {"default", "store32"}
    c = next(c for c in C.CASES if c.init == "wide")
    assert c.wl and c.basis == "wide40"
    o = C.case_oracle(oracle, c)
    kept = C.expected(c, o)["kept"]
    wide = (np.abs(kept) > 32767).any(axis=2)
    assert wide[:, 0].any() and not wide[:, 0].all()
    assert np.abs(kept).max() == 70000


def test_kinds_basis_normalisers_vary(oracle):
    """Tabulated and ocml normalisers can only be told apart where they are not constant: the
    oracle's Wang-Ling log weights of the proposals vary by more than 1e-6."""
    R, cp, _, sigma = C.basis(oracle, "kinds100")
    z = oracle.klein(R, cp, sigma, 64, seed=C.SEED, first_sample=0)["z"]
    lw = np.array([oracle.log_weight(R, cp, np.zeros_like(R), sigma, zk, mode=oracle.IMHK_WANG_LING) for zk in z])
    assert np.isfinite(lw).all() and lw.max() - lw.min() > 1e-6
    o = C.case_oracle(oracle, C._c("default", "kinds100", True, "c64"))
    assert o["lw"].max() - o["lw"].min() > 1e-6
    assert all(c.wl for c in C.CASES if c.basis == "kinds100")


def test_q_panel_skip_basis_skips(oracle):
    """The no_qskip case runs on a basis whose reference-mode Klein launch has a q-panel to
    skip (test_speculation_and_q_panel_skip_at_ragged_d): pinned panels stay at 0."""
    c = next(c for c in C.CASES if c.ctx == "no_qskip")
    assert c.basis == "skip100" and not c.wl and c.stream
    o = C.case_oracle(oracle, c)
    assert (o["states"][:, :, np.delete(np.arange(4, 68), 25 - 4)] == 0).all()


# ------------------------------------------------------------------ 3. completeness
def _options(c):
    return {k for k, v in C.CONTEXTS[c.ctx].items() if C.OPTION_ON[k] == v}


def test_every_context_option_has_a_case_in_both_weight_modes():
    from lgs_amd import _capi
    params = inspect.signature(_capi.Context.__init__).parameters
    options = {k for k, p in params.items() if p.kind is p.KEYWORD_ONLY} - C.NOT_OPTIONS
    assert options == set(C.OPTION_ON) | C.NOT_IN_TABLE, sorted(options ^ (set(C.OPTION_ON) | C.NOT_IN_TABLE))
    flags = {n for n in dir(_capi) if n.startswith("LGS_CTX_")}
    assert len(flags) == len(options), sorted(flags)  # one keyword per LGS_CTX_* flag
    for k, on in C.OPTION_ON.items():
        assert params[k].default != on, k  # the table's value is the one that sets the flag
    for name, kw in C.CONTEXTS.items():
        assert set(kw) <= set(C.OPTION_ON), name
    stream_only = {k for n in C.STREAM_CONTEXTS for k in C.CONTEXTS[n]}
    for opt in C.OPTION_ON:
        modes = {c.wl for c in C.CASES if opt in _options(c)}
        if opt in stream_only:
            # the early check is reference weights only (include/lgs.h lgs_set_stream), and
            # tests/test_gpu_stream.py owns this ground: one case, on a caller's stream
            cases = [c for c in C.CASES if opt in _options(c)]
            assert len(cases) == 1 and cases[0].stream and cases[0].dev and not cases[0].wl, opt
            continue
        assert modes == {False, True}, opt
        for d in ("40", "100"):  # on the d = 40 and the d = 100 bases
            assert {c.wl for c in C.CASES if opt in _options(c) and c.basis.endswith(d)} == {False, True}, (opt, d)
    for name in C.STORE_CONTEXTS:  # (the combination too)
        for d in ("40", "100"):
            assert {c.wl for c in C.CASES if c.ctx == name and c.basis.endswith(d)} == {False, True}, (name, d)
        assert any(c.ctx == name and c.basis == "kinds100" for c in C.CASES), name
        assert any(c.ctx == name and c.basis == "r130" for c in C.CASES), name


def test_table_uses_every_flag_and_shape_class():
    S = C.SHAPES
    used = {c.shape for c in C.CASES}
    assert used == set(S)
    assert any(c.z64 for c in C.CASES) and any(c.cm for c in C.CASES) and any(c.dev for c in C.CASES)
    # pairwise: every pair of (z64, cm, dev) values occurs
    for a, b in (("z64", "cm"), ("z64", "dev"), ("cm", "dev")):
        assert {(getattr(c, a), getattr(c, b)) for c in C.CASES} == {(x, y) for x in (False, True) for y in (False, True)}
    assert {S[c.shape].first_chain for c in C.CASES} == {0, 5, 2 ** 32 - 37}
    assert {S[c.shape].nc for c in C.CASES} >= {37, 64, 256}
    assert {S[c.shape].thin for c in C.CASES} == {1, 3}
    assert max(S[c.shape].steps for c in C.CASES) <= 24
    assert any(S[c.shape].steps % S[c.shape].thin for c in C.CASES)
    assert any(len(S[c.shape].split) > 1 for c in C.CASES)
    assert any(c.init == "set" for c in C.CASES) and any(c.init == "wide" for c in C.CASES)
    assert {c.basis for c in C.CASES} == set(C.BASES)
    assert len(C.CASES) <= 160 and len(set(C.CASE_IDS)) == len(C.CASES)
    for name, s in S.items():
        assert sum(s.split) == s.steps and all(p % s.thin == 0 for p in s.split[:-1]), name
        q = C.MAX_PROPOSALS // s.nc
        T = C.block_length(s)
        if s.thin > 1:
            assert q % s.thin != 0, name  # max_proposals / n_chains is not a multiple of thin
        assert T % s.thin == 0 and T <= max(q, s.thin)
        assert -(-s.split[0] // T) >= 3, name  # a call of at least three blocks
    assert C.MAX_PROPOSALS >= 64  # (lgs_create_ex raises smaller values to 64)
    # first_chain = 5 has its n + 5 chain partner
    a, b = S["c64-first5"], S["c69"]
    assert (b.nc, b.first_chain) == (a.nc + 5, 0) and a[1:3] == b[1:3]
    # every group has its base case, and every split shape its single call
    for key in C.GROUPS:
        C.base_case(key)
    # shapes that launch each Klein kernel: whole 256-proposal workgroups (int8 digits), whole
    # waves (fp64 MFMA far field), ragged (VALU)
    sizes = {s.nc * C.block_length(s) for s in S.values()}
    assert any(n % 256 == 0 for n in sizes) and any(n % 64 == 0 and n % 256 for n in sizes) and any(n % 64 for n in sizes)


def test_device_module_runs_the_table():
    import test_gpu_imhk_matrix as M
    marks = [m for m in M.test_case_vs_oracle.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and tuple(marks[0].args[1]) == C.CASES and tuple(marks[0].kwargs["ids"]) == C.CASE_IDS
    marks = [m for m in M.test_variants_equal_the_default_context.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and tuple(marks[0].args[1]) == C.GROUPS
    assert any(m.name == "gpu" for m in (M.pytestmark if isinstance(M.pytestmark, list) else [M.pytestmark]))
