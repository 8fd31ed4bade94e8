"""Every Klein kernel variant against the oracle, at ragged d and in every mode.

The library picks the Klein kernel from the launch shape (lgs_capi.hip run_klein):
n % 64 != 0 runs the VALU panel kernel, n % 64 == 0 the MFMA kernel with the fp64 far
field, n % 256 == 0 (32-row panels) the MFMA kernel with the int8-digit far field; the
launcher (lgs_kernels.hip klein_pb) then splits by Wang-Ling weights, libm SampleZ, store
width and panel height.  A test that means one of these kernels has to launch that shape,
so every case here asserts through the LGS_COUNTER_LAUNCH_* counters that the kernel it
names is the one that ran (and, for the int8-digit path, that nothing fell back).

All draws share one seed and first sample; one 512-sample oracle run per (basis,
precision, linear) is cached and every kernel's z is compared with its first n rows.

Tolerances are the project's own: z, v (integer bases), states, accept counts, moments
exact; log weights against the oracle rtol / atol 1e-9 on the first 64 samples
(test_gpu_configs.py); default kernels against the reference-order kernel relative 1e-10
in reference mode and within the kernel's own bound E (LGS_LOGW_BOUND, E == 0 for the
reference-order kernel) with Wang-Ling weights (test_gpu_certificate.py); tabulated
against libm SampleZ weights rtol 1e-12 / atol 1e-9 (test_gpu_parity.py).

Instantiations that launch::klein / klein_pb can launch, and the case that launches each
(ZT = int16: the default store; int32: Context(store32=True); int64: LGS_Z64; WL = false /
true: the case's "ref" / "wl" mode):

  klein_exact_kernel<ZT, WL>                 int16: test_ragged_d_every_kernel_vs_oracle[*-exact-*]
                                             int32 / int64: test_ragged_d_store_widths[*-exact-*]
  klein_panel_kernel<ZT, 32, WL>             ...[*-valu-*], same two tests
  klein_panel_kernel<ZT, 16, WL>             ...[*-p16-valu-*]
  klein_mfma_kernel<ZT, 32, WL>              ...[*-mfma64-*] (n = 192) and [*-far64-*] (LGS_CTX_FAR_FP64)
  klein_mfma_kernel<ZT, 16, WL>              ...[*-p16-mfma-*]
  klein_mfma_kernel<ZT, 32, WL, OZ>          ...[*-i8-*]; int32 also through
                                             test_ragged_d_int8_kernel_into_device_coordinate_major_int32
  klein_mfma_kernel<ZT, 32, WL, OZ, LIBM>    int16: test_samplez_kinds_precision_linear_every_kernel[*-i8-*]
                                             (its samplez_libm context); int32 / int64:
                                             test_samplez_libm_store_widths[*-i8-*]
  klein_mfma_kernel<ZT, 32, WL, false, LIBM> the same two tests, [*-mfma64-*] and [*-far64-*]
  klein_mfma_kernel<ZT, 16, WL, false, LIBM> the same two tests, [*-p16-mfma-*]

The exact and VALU kernels have no LIBM instantiation (they test a.szc at run time); their
libm path runs in the samplez_libm contexts of [*-exact-*] and [10-valu-*].  Not launchable:
klein_mfma_kernel<ZT, 16, WL, true, *> is compiled, but klein_pb takes the int8-digit
branch for 32-row panels only.
"""
import numpy as np
import pytest

from test_gpu_edges import _int_basis
from test_gpu_parity import _wide_sigma_basis

pytestmark = pytest.mark.gpu

SEED, FIRST, N_ORACLE = 20261, 31, 512

# name -> (Context options, n, exact order, the one launch counter that must read 1)
SELECTORS = {
    "exact": ({}, 512, True, "EXACT"),
    "valu": ({}, 200, False, "VALU"),
    "mfma64": ({}, 192, False, "MFMA_FP64"),
    "far64": ({"far": "fp64"}, 256, False, "MFMA_FP64"),
    "i8": ({}, 512, False, "MFMA_I8"),  # two workgroups
    "p16-mfma": ({"panel": 16}, 192, False, "MFMA_FP64"),
    "p16-valu": ({"panel": 16}, 200, False, "VALU"),
}
LAUNCH_KINDS = ("EXACT", "VALU", "MFMA_FP64", "MFMA_I8")
LEAN = ("i8", "mfma64", "far64", "exact")  # the cells outside the full cross
MODES = ("ref", "wl")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


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


def _launches(capi, c, reset=False):
    return tuple(c.counter(getattr(capi, "LGS_COUNTER_LAUNCH_" + k), reset=reset) for k in LAUNCH_KINDS)


def _only(kind):
    return tuple(1 if k == kind else 0 for k in LAUNCH_KINDS)


def _klein(capi, c, d, n, *, exact=False, wl=False, want_v=False, z64=False):
    """One lgs_klein call through host buffers: z, v, the log weights and (Wang-Ling) their
    bounds, with the launch counters and fallback count of exactly this call."""
    z = np.empty((n, d), dtype=np.int64 if z64 else np.int32)
    v = np.empty((n, d)) if want_v else None
    lw = np.empty(2 * n if wl else n)
    f = (capi.LGS_EXACT_ORDER if exact else 0) | (capi.LGS_Z64 if z64 else 0) | \
        (capi.LGS_WANG_LING | capi.LGS_LOGW_BOUND if wl else 0)
    _launches(capi, c, reset=True)
    c.fallbacks(reset=True)
    c.klein(SEED, FIRST, n, z, v, lw, f)
    return {"z": z.astype(np.int64), "v": v, "lw": lw[:n], "E": lw[n:] if wl else None,
            "launches": _launches(capi, c), "fallbacks": c.fallbacks()}


def _run(capi, c, d, sel, wl, want_v=False, z64=False):
    """The selector's launch, with the proof that its kernel ran."""
    _, n, exact, kind = SELECTORS[sel]
    r = _klein(capi, c, d, n, exact=exact, wl=wl, want_v=want_v, z64=z64)
    assert r["launches"] == _only(kind), (sel, dict(zip(LAUNCH_KINDS, r["launches"])))
    if kind == "MFMA_I8":
        assert r["fallbacks"] == 0  # the int8-digit path itself, not its redo
    return r


def _check_weights(oracle, basis, r, ex, wl, precision=10, linear=False, against_oracle=True):
    """Log weights of a run: against the oracle (first 64 samples) and against the
    reference-order kernel's (ex, 512 samples on the same counters)."""
    R, cp, B, sigma = basis
    n = len(r["lw"])
    assert np.isfinite(r["lw"]).all()
    if against_oracle:
        mode = oracle.IMHK_WANG_LING if wl else oracle.IMHK_REFERENCE
        Bo = B if B is not None else np.zeros_like(R)  # (Wang-Ling weights do not read B)
        want = np.array([oracle.log_weight(R, cp, Bo, sigma, r["z"][k], mode=mode, precision=precision,
                                           use_log_space=not linear) for k in range(64)])
        np.testing.assert_allclose(r["lw"][:64], want, rtol=1e-9, atol=1e-9)
    dif = np.abs(r["lw"] - ex["lw"][:n])
    if wl:
        assert not ex["E"].any()  # the reference-order kernel's bound is 0
        assert (dif <= r["E"]).all(), float((dif - r["E"]).max())
    else:
        assert float((dif / np.maximum(np.abs(ex["lw"][:n]), 1.0)).max()) < 1e-10


# ------------------------------------------------------------------ (a) ragged integer bases
RAGGED_D = (17, 33, 47, 49, 65, 100, 129)
FULL_CROSS_D = (47, 100)
_cache = {}


def _ragged(oracle, d):
    """(R, c', B, sigma) of the ragged integer basis and its 512-sample oracle run."""
    key = ("ragged", d)
    if key not in _cache:
        B = _int_basis(d, d)
        R, cp = oracle.qr_prepare(B)
        o = oracle.klein(R, cp, 8.0, N_ORACLE, seed=SEED, first_sample=FIRST, B=B)
        assert np.abs(o["z"]).max() <= 32639  # the int8-digit path does not hand over
        _cache[key] = ((R, cp, B, 8.0), o)
    return _cache[key]


def _exact_run(capi, c, key, d, wl, want_v=False):
    """The reference-order kernel's 512 samples on the basis c holds (cached by key)."""
    key = ("exact",) + key + (wl,)
    if key not in _cache:
        _cache[key] = _klein(capi, c, d, N_ORACLE, exact=True, wl=wl, want_v=want_v)
    return _cache[key]


RAGGED_CASES = [(d, s) for d in RAGGED_D for s in (SELECTORS if d in FULL_CROSS_D else LEAN)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,sel", RAGGED_CASES)
def test_ragged_d_every_kernel_vs_oracle(capi, ctxs, oracle, d, sel, mode):
    """d = 17: one partial panel, no far field; 33, 129: a bottom panel of 1 row; 47: of 15
    rows; 49: of 16 + 1 rows; 65 and above: a far field of two or more 64-column chunks
    above the ragged bottom.  At d % 16 != 0 the int8-digit kernel runs with a history
    shift, a bottom panel that starts below row 0 and no per-wave chunk bits, and B z must
    not read the Klein history: z and v = B z equal the oracle's exactly."""
    basis, o = _ragged(oracle, d)
    wl = mode == "wl"
    c = ctxs(**SELECTORS[sel][0])
    c.set_basis(*basis)
    ex = _exact_run(capi, c, ("ragged", d), d, wl)
    r = _run(capi, c, d, sel, wl, want_v=True)
    n = SELECTORS[sel][1]
    assert np.array_equal(r["z"], o["z"][:n])
    assert np.array_equal(r["v"], o["v"][:n])
    _check_weights(oracle, basis, r, ex, wl)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sel", list(SELECTORS))
@pytest.mark.parametrize("width", ["store32", "z64"])
def test_ragged_d_store_widths(capi, ctxs, oracle, sel, width, mode):
    """The 32-bit internal store (LGS_CTX_STORE32) and the 64-bit one (LGS_Z64) of every
    kernel at d = 100 (the 16-bit default is the matrix above)."""
    d = 100
    basis, o = _ragged(oracle, d)
    wl = mode == "wl"
    opts = dict(SELECTORS[sel][0], **({"store32": True} if width == "store32" else {}))
    c = ctxs(**opts)
    c.set_basis(*basis)
    r = _run(capi, c, d, sel, wl, want_v=True, z64=width == "z64")
    n = SELECTORS[sel][1]
    assert np.array_equal(r["z"], o["z"][:n])
    assert np.array_equal(r["v"], o["v"][:n])
    ex = _exact_run(capi, c, ("ragged", d), d, wl)
    _check_weights(oracle, basis, r, ex, wl, against_oracle=False)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_d_int8_kernel_into_device_coordinate_major_int32(capi, ctxs, oracle, mode):
    """A device coordinate-major int32 output is written by the kernel itself (no internal
    store): the int32 instantiation of the int8-digit kernel, d = 100, two workgroups."""
    import torch
    d, n = 100, 512
    basis, o = _ragged(oracle, d)
    wl = mode == "wl"
    c = ctxs()
    c.set_basis(*basis)
    z = torch.empty((d, n), dtype=torch.int32, device="cuda:0")
    v = torch.empty((n, d), dtype=torch.float64, device="cuda:0")
    lw = torch.empty(n, dtype=torch.float64, device="cuda:0")
    _launches(capi, c, reset=True)
    c.fallbacks(reset=True)
    c.klein(SEED, FIRST, n, z, v, lw,
            capi.LGS_DEVICE_PTRS | capi.LGS_COORD_MAJOR | (capi.LGS_WANG_LING if wl else 0))
    torch.cuda.synchronize()
    assert _launches(capi, c) == _only("MFMA_I8") and c.fallbacks() == 0
    assert np.array_equal(z.cpu().numpy().T, o["z"])
    assert np.array_equal(v.cpu().numpy(), o["v"])
    if not wl:  # (Wang-Ling: the bound needs LGS_LOGW_BOUND, checked in the matrix above)
        ex = _exact_run(capi, c, ("ragged", d), d, wl)
        _check_weights(oracle, basis, {"z": o["z"], "lw": lw.cpu().numpy()}, ex, wl, against_oracle=False)


# ------------------------------------------------------------------ (b) every SampleZ kind
KINDS_D, KINDS_SIGMA = 100, 10.0
KINDS_ROUND = 40  # the coordinate with sigma_i = 1e-11


def _kinds_basis():
    """test_gpu_parity's wide-sigma basis (tiny, small, uncapped wide, capped, clamped
    sigma_i) with one sigma_i = 1e-11 coordinate (the round kind) and the top coordinate
    pinned to a half-integer mean by a tiny sigma_i."""
    d = KINDS_D
    R, cp = _wide_sigma_basis(d, 3)
    s = (KINDS_SIGMA / 1e-11) / R[KINDS_ROUND, KINDS_ROUND]
    R[KINDS_ROUND] *= s  # (the row's mean is unchanged)
    cp[KINDS_ROUND] *= s
    R[d - 1, d - 1] = 2048.0
    cp[d - 1] = 2.5 * 2048.0
    return np.ascontiguousarray(R), cp


def _kinds(oracle, precision, linear):
    key = ("kinds", precision, linear)
    if key not in _cache:
        R, cp = _kinds_basis()
        _cache[key] = ((R, cp, None, KINDS_SIGMA),
                       oracle.klein(R, cp, KINDS_SIGMA, N_ORACLE, seed=SEED, first_sample=FIRST,
                                    precision=precision, use_log_space=not linear))
    return _cache[key]


@pytest.mark.parametrize("precision", [3, 10, 20])
def test_kinds_basis_conditions(oracle, precision):
    """Conditions on the inputs of the SampleZ-kind matrix, on the oracle alone: every kind
    is present, linear-space probabilities take the oracle's fallback and change many
    samples (a kernel that ignored linear_probs cannot pass), and no coefficient is beyond
    the int8-digit path's history range."""
    (R, _, _, sigma), o_log = _kinds(oracle, precision, False)
    _, o_lin = _kinds(oracle, precision, True)
    s = sigma / np.diag(R)
    assert (s < 1e-10).sum() == 1 and (s > 1e10).sum() == 1
    assert ((s >= 1e-10) & (s < 0.1)).sum() >= 10 and ((s >= 0.1) & (s < 4)).sum() >= 10
    assert ((s >= 4) & (s < 50)).sum() >= 10 and ((s >= 50) & (s < 360)).sum() >= 5
    assert ((s >= 360) & (s < 1e10)).sum() >= 5
    assert o_log["fallbacks"] == 0 and o_lin["fallbacks"] > 0
    differ = (o_log["z"] != o_lin["z"]).any(1).sum()
    assert differ >= N_ORACLE // 4, differ
    assert max(np.abs(o_log["z"]).max(), np.abs(o_lin["z"]).max()) <= 32639
    top = o_log["z"][:, -1]  # the half-integer mean: both neighbours drawn
    assert set(np.unique(top)) == {2, 3}


KINDS_SELECTORS = ("exact", "valu", "mfma64", "far64", "i8", "p16-mfma")
KINDS_CASES = [(p, s) for p in (3, 10, 20) for s in (KINDS_SELECTORS if p == 10 else LEAN)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("linear", [False, True], ids=["log", "linear"])
@pytest.mark.parametrize("precision,sel", KINDS_CASES)
def test_samplez_kinds_precision_linear_every_kernel(capi, ctxs, oracle, precision, sel, linear, mode):
    """A basis spanning every SampleZ kind, at precision 3 / 10 / 20, in log space and with
    linear-space probabilities (LGS_BASIS_LINEAR_PROBS, the reference's use_log_space=False),
    with the per-coordinate constants and with libm SampleZ (LGS_CTX_SAMPLEZ_LIBM): z equals
    the oracle's in every kernel.  Wang-Ling weights (B = None): against the oracle, within
    the kernel's bound of the reference-order kernel's, tabulated against libm.  Reference-
    mode weights are not compared here: their log sigma_i terms reach 1e21."""
    basis, o = _kinds(oracle, precision, linear)
    R, cp, _, sigma = basis
    wl = mode == "wl"
    n = SELECTORS[sel][1]
    out = {}
    for libm in (False, True):
        c = ctxs(**dict(SELECTORS[sel][0], **({"samplez_libm": True} if libm else {})))
        c.set_basis(R, cp, None, sigma, precision=precision, linear_probs=linear)
        ex = _exact_run(capi, c, ("kinds", precision, linear, libm), KINDS_D, wl)
        r = out[libm] = _run(capi, c, KINDS_D, sel, wl)
        assert np.array_equal(r["z"], o["z"][:n]), f"libm={libm}"
        if wl:
            _check_weights(oracle, basis, r, ex, wl, precision=precision, linear=linear)
    if wl:
        np.testing.assert_allclose(out[False]["lw"], out[True]["lw"], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sel", ["i8", "mfma64", "p16-mfma"])
@pytest.mark.parametrize("width", ["store32", "z64"])
def test_samplez_libm_store_widths(capi, ctxs, oracle, sel, width, mode):
    """The libm SampleZ instantiations of the MFMA kernels with a 32-bit and a 64-bit
    store (the 16-bit ones run in the matrix above), on the basis of every SampleZ kind."""
    basis, o = _kinds(oracle, 10, False)
    R, cp, _, sigma = basis
    wl = mode == "wl"
    opts = dict(SELECTORS[sel][0], samplez_libm=True, **({"store32": True} if width == "store32" else {}))
    c = ctxs(**opts)
    c.set_basis(R, cp, None, sigma)
    ex = _exact_run(capi, c, ("kinds", 10, False, True), KINDS_D, wl)
    r = _run(capi, c, KINDS_D, sel, wl, z64=width == "z64")
    assert np.array_equal(r["z"], o["z"][:SELECTORS[sel][1]])
    if wl:
        _check_weights(oracle, basis, r, ex, wl, against_oracle=False)


# ------------------------------------------------------------------ (c) speculation and q-panel skip
SKIP_D, SKIP_SIGMA, SKIP_N, SKIP_RARE = 100, 3.0, 4096, 25


def _skip_basis(off_zero):
    """Upper-triangular integer basis (B = R), d = 100: panel 0 (rows 68..99) and the ragged
    bottom panel (rows 0..3) are free (sigma_i = 1 .. 1.5); panels 1 and 2 (rows 4..67) are
    pinned by R_ii = 1e4 (sigma_i = 3e-4: speculative sub-panels, and panel 1 a q-panel the
    reference-mode kernel may skip), except one row of panel 2 with sigma_i = 0.25, nonzero
    in a few samples.  off_zero moves the pinned rows' means from 0 to 1: the speculation
    z = 0 fails and the sub-panels are redone in order; nothing can be skipped."""
    rng = np.random.default_rng(17)
    d = SKIP_D
    R = np.zeros((d, d))
    for i in range(d):
        R[i, i] = float(rng.integers(2, 4))
        if i < d - 1:
            R[i, rng.integers(i + 1, d, 3)] += rng.choice([-1.0, 1.0], 3)
    cp = np.round(rng.normal(size=d) * 8.0) / 4.0
    pinned = np.arange(4, 68)
    R[pinned, pinned] = 1e4
    R[SKIP_RARE, SKIP_RARE + 1:] = 0.0
    R[SKIP_RARE, SKIP_RARE] = SKIP_SIGMA / 0.25
    cp[pinned] = R[pinned, pinned] if off_zero else 0.0
    return R, cp


def _skip(oracle, off_zero):
    key = ("skip", off_zero)
    if key not in _cache:
        R, cp = _skip_basis(off_zero)
        o = oracle.klein(R, cp, SKIP_SIGMA, SKIP_N, seed=SEED, first_sample=FIRST, B=R)
        _cache[key] = ((R, cp, R, SKIP_SIGMA), o)
    return _cache[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("off_zero", [False, True], ids=["centred", "off-zero"])
def test_speculation_and_q_panel_skip_at_ragged_d(capi, oracle, off_zero, mode):
    basis, o = _skip(oracle, off_zero)
    d, n, wl = SKIP_D, SKIP_N, mode == "wl"
    zo = o["z"]
    # conditions on the oracle output
    pinned = np.delete(np.arange(4, 68), SKIP_RARE - 4)
    assert (zo[:, pinned] == (1 if off_zero else 0)).all()
    blocks = np.unique(np.flatnonzero(zo[:, SKIP_RARE] != (1 if off_zero else 0)) // 256)
    assert 0 < len(blocks) < n // 256, blocks
    assert np.abs(zo).max() <= 32639
    out = {}
    for qskip in (True, False):
        c = capi.Context(0, qskip=qskip)
        try:
            c.set_basis(*basis)
            c.counter(capi.LGS_COUNTER_QSKIP, reset=True)
            r = _klein(capi, c, d, n, wl=wl, want_v=True)
            r["qskip"] = c.counter(capi.LGS_COUNTER_QSKIP)
        finally:
            c.close()
        assert r["launches"] == _only("MFMA_I8") and r["fallbacks"] == 0
        assert np.array_equal(r["z"], zo)
        assert np.array_equal(r["v"], o["v"])
        out[qskip] = r
    assert out[False]["qskip"] == 0
    if wl or off_zero:
        assert out[True]["qskip"] == 0  # reference mode only; a mean off 0 voids the bound
    else:
        assert 0 < out[True]["qskip"] <= n // 64  # panel 1, per 64-sample wave
    assert np.array_equal(out[True]["z"], out[False]["z"])


# ------------------------------------------------------------------ (d) IMHK at ragged d, int8 path
IMHK_SEED = 611
# The ragged integer bases at sigma = 3 here: at sigma = 8 their sigma_i = 1.3 make the
# Wang-Ling normalisers constant to 1e-15 and every proposal is accepted, whatever the seed.
IMHK_SIGMA = 3.0


def _imhk_basis(oracle, name):
    if name == "skip":
        return _skip(oracle, False)[0]
    R, cp, B, _ = _ragged(oracle, int(name))[0]
    return R, cp, B, IMHK_SIGMA


def _imhk_oracle(oracle, name, nc, T):
    """Two consecutive oracle calls of T steps (the second resumes the first's state)."""
    key = ("imhk", name, nc, T)
    if key not in _cache:
        R, cp, B, sigma = _imhk_basis(oracle, name)
        calls, st = [], None
        for call in range(2):
            st = oracle.imhk(R, cp, B, sigma, nc, T, seed=IMHK_SEED, first_step=1 + call * T, state=st,
                             mode=oracle.IMHK_WANG_LING, trace=True)
            calls.append({k: np.array(v, copy=True) for k, v in st.items()})
            st = {k: st[k] for k in ("z", "lw", "init", "accepts")}
        _cache[key] = calls
    return _cache[key]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nc,T", [(64, 8), (256, 2)])
@pytest.mark.parametrize("name", ["40", "100", "skip"])
def test_imhk_ragged_d_int8_path_vs_oracle(capi, oracle, name, nc, T, dev):
    """lgs_imhk with Wang-Ling weights where d % 16 != 0 and a block is whole 256-proposal
    workgroups (nc T = 512): the int8-digit Klein kernel with a history shift feeds B z, the
    moments pass (its zero-block flags) and the final-state gather.  Two consecutive calls;
    states, accept counts, kept states, lattice points and moments equal the oracle's."""
    import torch
    R, cp, B, sigma = _imhk_basis(oracle, name)
    d = R.shape[0]
    calls = _imhk_oracle(oracle, name, nc, T)
    f = capi.LGS_WANG_LING | (capi.LGS_DEVICE_PTRS if dev else 0)

    def buf(shape, dtype):
        a = np.zeros(shape, dtype=dtype)
        return torch.from_numpy(a).to("cuda:0") if dev else a

    def host(a):
        return a.cpu().numpy() if dev else a

    z, lw, init, acc = buf((nc, d), np.int32), buf(nc, np.float64), buf(nc, np.int32), buf(nc, np.int64)
    mom = buf(2 * d, np.int64)
    want_mom = np.zeros(2 * d, dtype=np.int64)
    c = capi.Context(0)
    try:
        c.set_basis(R, cp, B, sigma)
        _launches(capi, c, reset=True)
        prev = np.zeros(nc, dtype=np.int64)
        for call, o in enumerate(calls):
            # (v_samples is a device-pointer output: through host pointers the lattice points
            # of the kept states come from lgs_lattice_points)
            zs, vs = buf((nc, T, d), np.int32), buf((nc, T, d), np.float64) if dev else None
            c.imhk(IMHK_SEED, 0, nc, 1 + call * T, T, 1, z, lw, init, acc, z_samples=zs, v_samples=vs,
                   moments=mom, flags=f)
            if dev:
                torch.cuda.synchronize()
            else:
                vs = c.lattice_points(zs.reshape(-1, d)).reshape(nc, T, d)
            step_acc = o["accepts"] - prev
            prev = o["accepts"]
            assert 0 < step_acc.sum() < nc * T  # (a condition on the oracle: the seed was picked for it)
            assert np.array_equal(host(zs), o["trace"])
            assert np.array_equal(host(vs), o["trace"].astype(np.float64) @ B.T)
            assert np.array_equal(host(acc), o["accepts"])
            assert np.array_equal(host(z), o["z"])
            assert host(init).all()
            np.testing.assert_allclose(host(lw), o["lw"], rtol=1e-9)
            flat = o["trace"].reshape(-1, d)
            want_mom[:d] += flat.sum(0)
            want_mom[d:] += (flat * flat).sum(0)
            assert np.array_equal(host(mom), want_mom)
        launches = dict(zip(LAUNCH_KINDS, _launches(capi, c)))
        assert launches["MFMA_I8"] >= 1 and launches["EXACT"] == 0, launches
        assert c.fallbacks() == 0
    finally:
        c.close()
