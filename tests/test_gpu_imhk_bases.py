"""IMHK chains over a batch of bases (lgs_imhk_bases, lgs_amd.samplers.imhk_bases) against the CPU
transcription tests/imhkb_oracle.py: QR(p) from tests/qr_oracle.py, the draws, their Wang-Ling
weights and the accept uniforms from the C oracle, the scan written out.

qr_status, R, c' and every draw compare bit for bit.  The device's weights are its SampleZ's window
normalisers, the oracle's a logsumexp over the same window: they compare to 1e-9 relative, the
tolerance of tests/test_gpu_imhk_targets.py.  A decision closer to its threshold than twice that
could go either way, so the scan's outputs compare on the settled chains only (imhkb_oracle.scan;
tests/test_imhk_bases_host.py bounds their share), and a NumPy rescan from the device's own weights
checks the scan of every chain with no tolerance."""
import numpy as np
import pytest

import imhkb_oracle
import kleinb_oracle
import qr_oracle
from test_imhk_targets_host import d2_exact_pmf, tv_distance

pytestmark = pytest.mark.gpu

SEED = imhkb_oracle.SEED
FIRST = imhkb_oracle.FIRST_CHAIN
OUTS = ("logw", "accepts", "final_step", "status", "qr_status", "R", "cprime", "accepted", "logw_draws", "z_draws",
        "z_samples")
EXACT = ("qr_status", "R", "cprime", "z_draws", "status")  # bit for bit the oracle's, every chain
SCAN = ("accepted", "accepts", "final_step", "z", "z_samples")  # equal on the settled chains
ALL = ("z", "v") + OUTS


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


def _run(capi, ctx, Bs, Ts, sigma, C, S, thin=1, seed=SEED, first=FIRST, z64=False, dev=False, precision=10):
    """The raw call on host arrays or device tensors, every output prefilled with a sentinel;
    returns host arrays, the coefficient arrays as int64."""
    n, T, d = Ts.shape
    zdt = np.int64 if z64 else np.int32
    nk = S // thin
    host = {"z": np.full((n, T, C, d), -77, dtype=zdt), "v": np.full((n, T, C, d), np.nan),
            "logw": np.full((n, T, C), np.nan), "accepts": np.full((n, T, C), -5, dtype=np.int64),
            "final_step": np.full((n, T, C), -5, dtype=np.int64), "status": np.full((n, T), -1, dtype=np.int32),
            "qr_status": np.full(n, -1, dtype=np.int32), "R": np.full((n, d, d), np.nan),
            "cprime": np.full((n, T, d), np.nan), "accepted": np.full((n, T, C, S), 9, dtype=np.uint8),
            "logw_draws": np.full((n, T, C, S + 1), np.nan), "z_draws": np.full((n, T, C, S + 1, d), -77, dtype=zdt),
            "z_samples": np.full((n, T, C, nk, d), -77, dtype=zdt)}
    b, t = np.ascontiguousarray(Bs, dtype=np.float64), np.ascontiguousarray(Ts, dtype=np.float64)
    s = np.ascontiguousarray(sigma, dtype=np.float64)
    flags = capi.LGS_Z64 if z64 else 0
    if dev:
        import torch
        up = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: the oracle's arrays are read-only)
        bufs = {k: up(a) for k, a in host.items()}
        b, t, s = up(b), up(t), up(s)
        flags |= capi.LGS_DEVICE_PTRS
    else:
        bufs = host
    try:
        ctx.imhk_bases(seed, first, b, t, s, C, S, thin, precision, bufs["z"], bufs["v"], flags=flags,
                       **{k: bufs[k] for k in OUTS})
    finally:
        if dev:
            torch.cuda.synchronize()
            host = {k: a.cpu().numpy() for k, a in bufs.items()}
        _run.last = host
    for k in ("z", "z_draws", "z_samples"):
        host[k] = host[k].astype(np.int64)
    return host


def _same(got, want, keys=ALL):
    """Bit for bit: the bytes of every array (so -0.0 differs from +0.0 and -inf equals -inf)."""
    for k in keys:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(np.asarray(want[k], dtype=got[k].dtype))
        if g.shape != w.shape or g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w) if g.shape == w.shape else None
            raise AssertionError(f"{k} differs: first at {None if bad is None or not len(bad) else bad[0].tolist()}, "
                                 f"{0 if bad is None else len(bad)} elements")


def _sentinels_intact(out):
    assert (out["z"] == -77).all() and (out["z_draws"] == -77).all() and (out["z_samples"] == -77).all()
    assert np.isnan(out["v"]).all() and np.isnan(out["R"]).all() and np.isnan(out["cprime"]).all()
    assert np.isnan(out["logw"]).all() and np.isnan(out["logw_draws"]).all() and (out["accepted"] == 9).all()
    assert (out["accepts"] == -5).all() and (out["final_step"] == -5).all()
    assert (out["status"] == -1).all() and (out["qr_status"] == -1).all()


def _close(g, w):
    """Within 1e-9 relative, elementwise (equal infinities are equal)."""
    g, w = np.asarray(g), np.asarray(w)
    fin = np.isfinite(w)
    return np.array_equal(g[~fin], w[~fin]) and bool((np.abs(g[fin] - w[fin]) <= 1e-9 * np.abs(w[fin])).all())


def _against_oracle(got, want, Bs):
    """The comparison of the module docstring; returns how many chains were left out."""
    _same(got, want, EXACT)
    assert _close(got["logw_draws"], want["logw_draws"])
    ok = want["settled"]
    for k in SCAN:
        assert np.array_equal(got[k][ok], np.asarray(want[k])[ok]), k
    assert _close(got["logw"][ok], want["logw"][ok])
    n, T, C, d = got["z"].shape
    for p in range(n):  # v of every chain, from the device's own z, in the defined order
        assert got["v"][p].tobytes() == kleinb_oracle.points(Bs[p], got["z"][p].reshape(T * C, d)).tobytes(), p
    return int((~ok).sum())


def _rescan(capi, lwd, seed, first, thin):
    """The scan in NumPy from the weights lwd (n, T, C, S + 1) with lgs_amd._philox.accept_uniform:
    (accepted, accepts, final_step, logw, kept (n, T, C, S // thin), the smallest |u - ratio| / ratio)."""
    from lgs_amd import _philox
    shape, S = lwd.shape[:-1], lwd.shape[-1] - 1
    lw = lwd.reshape(-1, S + 1)
    N = lw.shape[0]
    chain = (first + np.arange(N)).astype(np.uint32)
    cur, lw_x = np.zeros(N, dtype=np.int64), lw[:, 0].copy()
    accepted, kept, margin = np.zeros((N, S), dtype=np.uint8), [], np.inf
    for t in range(1, S + 1):
        u = _philox.accept_uniform(seed, np.uint32(t), chain)
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.exp(lw[:, t] - lw_x)
        r = np.where((lw_x == -np.inf) | ~(r < 1.0), 1.0, r)
        with np.errstate(divide="ignore"):  # (a ratio that underflowed to 0: the margin is inf)
            margin = min(margin, float((np.abs(u - r) / r).min()))
        take = u < r
        cur, lw_x = np.where(take, t, cur), np.where(take, lw[:, t], lw_x)
        accepted[:, t - 1] = take
        if t % thin == 0:
            kept.append(cur.copy())
    kept = np.stack(kept, axis=1) if kept else np.zeros((N, 0), dtype=np.int64)
    return (accepted.reshape(shape + (S,)), accepted.sum(axis=1, dtype=np.int64).reshape(shape), cur.reshape(shape),
            lw_x.reshape(shape), kept.reshape(shape + (-1,)), margin)


def _consistent(capi, got, seed, first, thin):
    """The device's scan outputs are the NumPy rescan of its own weights, exactly."""
    a, acc, fin, lw, kept, margin = _rescan(capi, got["logw_draws"], seed, first, thin)
    assert margin > 1e-14, margin  # no decision within the two exponentials' rounding of its threshold
    assert np.array_equal(got["accepted"], a) and np.array_equal(got["accepts"], acc)
    assert np.array_equal(got["final_step"], fin) and got["logw"].tobytes() == lw.tobytes()
    zd = got["z_draws"]
    assert np.array_equal(got["z"], np.take_along_axis(zd, fin[..., None, None], axis=3)[..., 0, :])
    assert np.array_equal(got["z_samples"], np.take_along_axis(zd, kept[..., None], axis=3))


# ------------------------------------------------------------------ 1. parity with the transcription
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("z64", [False, True], ids=["z32", "z64"])
@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_parity_with_the_transcription(capi, d, T, z64, dev):
    """n_bases = 1, 3, 130 of every shape, widths 3 / 300 / 3000 in turn, (C, S) from
    imhkb_oracle.PARITY_CS: 5 to 465 lanes per basis, blocks of 256 lanes (d <= 32) and 128."""
    ctx = capi.Context(0)
    for C, S in imhkb_oracle.PARITY_CS[(d, T)]:
        for n in qr_oracle.BATCHES:
            Bs, Ts, _ = qr_oracle.batch(d, T, n)
            want = imhkb_oracle.expected(d, T, n, C, S)
            got = _run(capi, ctx, Bs, Ts, want["sigma"], C, S, z64=z64, dev=dev)
            out = _against_oracle(got, want, Bs)
            print(f"  ({d}, {T}) C = {C}, S = {S}, n = {n}: {out} of {n * T * C} chains left out (unsettled)")
            # (the sigma = 3 basis, alone in the batch of one, carries most of them: 11 of 64 at d = 64)
            assert n < 130 or out <= 0.1 * n * T * C


# ------------------------------------------------------------------ 2. the scan, every chain
@pytest.mark.parametrize("d,T,C,S,thin", [(2, 1, 1, 69, 1), (2, 1, 5, 0, 1), (3, 2, 3, 6, 2), (17, 5, 3, 30, 4),
                                          (33, 64, 1, 6, 1), (64, 64, 1, 6, 3)])
def test_the_scan_is_consistent_with_the_devices_weights(capi, d, T, C, S, thin):
    """No chain left out: accepted, accepts, final_step, logw, z and z_samples are the rescan of the
    device's logw_draws, and z_samples[.., r] is the draw that is the state after step (r + 1) thin."""
    n = 130 if d <= 17 else 3
    Bs, Ts, idx = qr_oracle.batch(d, T, n)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    got = _run(capi, capi.Context(0), Bs, Ts, sigma, C, S, thin)
    _consistent(capi, got, SEED, FIRST, thin)
    assert got["z_samples"].shape[3] == S // thin


# ------------------------------------------------------------------ 3. the single-basis path
@pytest.mark.parametrize("libm", [False, True], ids=["table", "libm"])
@pytest.mark.parametrize("d,T", [(3, 2), (17, 5), (33, 64)])
def test_same_chains_as_imhk_targets_on_the_returned_frame(capi, d, T, libm):
    """lgs_set_basis(R_out[p], sigma_p), then lgs_imhk_targets with LGS_EXACT_ORDER |
    LGS_TARGETS_QFRAME on the rows of cprime_out[p] repeated C times from first_chain + p T C: the
    same states, decisions and counts; logw within 1e-9 relative."""
    (C, S), n = imhkb_oracle.PARITY_CS[(d, T)][0], 3
    Bs, Ts, idx = qr_oracle.batch(d, T, n)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    got = _run(capi, capi.Context(0, samplez_libm=libm), Bs, Ts, sigma, C, S)
    one = capi.Context(0, samplez_libm=libm)
    fl = capi.LGS_EXACT_ORDER | capi.LGS_TARGETS_QFRAME
    for p in range(n):
        one.set_basis(np.ascontiguousarray(got["R"][p]), np.zeros(d), np.ascontiguousarray(Bs[p]), float(sigma[p]))
        rows = np.ascontiguousarray(np.repeat(got["cprime"][p], C, axis=0))
        r = one.imhk_targets_host(SEED, FIRST + p * T * C, rows, S, want_v=False, want_trace=True, flags=fl)
        assert np.array_equal(r["z"].reshape(T, C, d), got["z"][p]), p
        assert np.array_equal(r["accepted"].reshape(T, C, S), got["accepted"][p]), p
        assert np.array_equal(r["accepts"].reshape(T, C), got["accepts"][p]), p
        assert np.array_equal(r["final_step"].reshape(T, C), got["final_step"][p]), p
        assert _close(got["logw"][p], r["logw"].reshape(T, C)), p


# ------------------------------------------------------------------ 4. no steps
@pytest.mark.parametrize("d,T", [(2, 1), (17, 5)])
def test_no_steps_gives_the_klein_draws(capi, d, T):
    """S = 0: chain c is Klein sample c, so z is lgs_klein_bases' z_draws for K = C from
    first_sample = first_chain."""
    C, n = 5, 3
    Bs, Ts, idx = qr_oracle.batch(d, T, n)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    ctx = capi.Context(0)
    got = _run(capi, ctx, Bs, Ts, sigma, C, 0)
    kb = ctx.klein_bases_host(SEED, FIRST, Bs, Ts, sigma, C, want_draws=True)
    assert np.array_equal(got["z"], kb["z_draws"]) and np.array_equal(got["z_draws"][:, :, :, 0], kb["z_draws"])
    assert not got["accepts"].any() and not got["final_step"].any() and got["accepted"].size == 0
    assert got["logw"].tobytes() == got["logw_draws"][..., 0].tobytes() and np.isfinite(got["logw"]).all()
    if d == 2:
        _same(got, imhkb_oracle.expected(d, T, n, C, 0), EXACT + SCAN)


# ------------------------------------------------------------------ 5. independence
def test_split_calls_chunks_and_shorter_chains_give_the_same_bytes(capi, monkeypatch):
    d, T, (C, S) = 17, 5, imhkb_oracle.PARITY_CS[(17, 5)][0]
    Bs, Ts, _ = qr_oracle.batch(d, T, 130)
    want = imhkb_oracle.expected(d, T, 130, C, S)
    sg = want["sigma"]
    prod = capi.Context(0)
    prod.timing_enable(True)
    whole = _run(capi, prod, Bs, Ts, sg, C, S)
    _against_oracle(whole, want, Bs)
    for kernel in (capi.KERNEL_CPRIME, capi.KERNEL_KLEIN, capi.KERNEL_ACCEPT, capi.KERNEL_DECODE_SELECT):
        assert prod.timing_get(kernel)[1] == 1, kernel
    a = _run(capi, prod, Bs[:57], Ts[:57], sg[:57], C, S)
    b = _run(capi, prod, Bs[57:], Ts[57:], sg[57:], C, S, first=FIRST + 57 * T * C)
    _same({k: np.concatenate([a[k], b[k]]) for k in ALL}, whole)
    monkeypatch.setenv("LGS_TEST_KLEINB_SLOTS", "64")
    hooks = capi.Context(0, hooks=True)
    hooks.timing_enable(True)
    _same(_run(capi, hooks, Bs, Ts, sg, C, S), whole)
    assert hooks.timing_get(capi.KERNEL_CPRIME)[1] == 3  # one QR launch per chunk: 64, 64 and 2 bases
    assert hooks.timing_get(capi.KERNEL_ACCEPT)[1] == 3
    again = capi.Context(0)  # the product library reads no environment: one chunk
    again.timing_enable(True)
    _same(_run(capi, again, Bs, Ts, sg, C, S), whole)
    assert again.timing_get(capi.KERNEL_CPRIME)[1] == 1
    short = _run(capi, prod, Bs, Ts, sg, C, 15)  # a shorter chain is a prefix
    assert np.array_equal(short["accepted"], whole["accepted"][..., :15])
    assert short["logw_draws"].tobytes() == np.ascontiguousarray(whole["logw_draws"][..., :16]).tobytes()
    assert np.array_equal(short["z_draws"], whole["z_draws"][..., :16, :])
    assert np.array_equal(short["accepts"], short["accepted"].sum(axis=3))


def test_the_last_chain_ids(capi):
    """first_chain = 2^32 - n T C: the batch ends at chain 2^32 - 1; the oracle's chains, and the
    same bytes from split calls."""
    d, T, (C, S), n = 17, 5, imhkb_oracle.PARITY_CS[(17, 5)][0], 3
    first = (1 << 32) - n * T * C
    Bs, Ts, _ = qr_oracle.batch(d, T, n)
    want = imhkb_oracle.expected(d, T, n, C, S, first_chain=first)
    ctx = capi.Context(0)
    got = _run(capi, ctx, Bs, Ts, want["sigma"], C, S, first=first)
    assert _against_oracle(got, want, Bs) == 0
    _consistent(capi, got, SEED, first, 1)
    a = _run(capi, ctx, Bs[:1], Ts[:1], want["sigma"][:1], C, S, first=first)
    b = _run(capi, ctx, Bs[1:], Ts[1:], want["sigma"][1:], C, S, first=first + T * C)
    _same({k: np.concatenate([a[k], b[k]]) for k in ALL}, got)
    assert not np.array_equal(got["z_draws"], imhkb_oracle.expected(d, T, n, C, S)["z_draws"])


# ------------------------------------------------------------------ 6. special bases
def test_a_refused_basis_leaves_the_others_alone(capi):
    d, T, C, S = 17, 5, 3, 6
    good, Ts, idx = qr_oracle.batch(d, T, 3)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    Bs = good.copy()
    Bs[1][:, 7] = 0.0
    for dev in (False, True):
        got = _run(capi, capi.Context(0), Bs, Ts, sigma, C, S, thin=2, dev=dev)
        assert got["qr_status"].tolist() == [0, 3, 0]
        assert (got["status"][1] == 3).all() and not got["status"][[0, 2]].any()
        for k in ("z", "v", "R", "cprime", "z_draws", "z_samples", "accepts", "accepted"):
            assert not got[k][1].any(), k
            assert not np.signbit(got[k][1]).any(), k  # (+0.0)
        assert (got["logw"][1] == -np.inf).all() and (got["logw_draws"][1] == -np.inf).all()
        assert (got["final_step"][1] == -1).all()
        for p in (0, 2):
            alone = _run(capi, capi.Context(0), good[p:p + 1], Ts[p:p + 1], sigma[p:p + 1], C, S, thin=2,
                         first=FIRST + p * T * C, dev=dev)
            _same({k: got[k][p:p + 1] for k in ALL}, alone)


def test_rounded_coordinates_are_not_drawn(capi):
    """A width of 1e-9: every s_i < 1e-10, so every coordinate is rounded, every draw is the same
    point (Babai's) and every weight is 0.0."""
    d, T, C, S, n = 17, 5, 3, 6, 3
    Bs, Ts, idx = qr_oracle.batch(d, T, n)
    sigma = np.full(n, 1e-9)
    want = kleinb_oracle.expected(d, T, n, 1)  # (R; the draws of a rounded basis do not depend on sigma below)
    assert (1e-9 / np.diagonal(want["R"], axis1=1, axis2=2) < 1e-10).all()
    babai = np.stack([kleinb_oracle.solve(Bs[p], Ts[p], 1e-9, 1, SEED, 0, qr=kleinb_oracle.qr_of(d, T, idx[p]))["z_draws"]
                      for p in range(n)])  # (n, T, 1, d)
    for dev in (False, True):
        got = _run(capi, capi.Context(0), Bs, Ts, sigma, C, S, dev=dev)
        assert (got["z_draws"] == babai[:, :, :, None, :]).all() and (got["z"] == babai).all()
        assert got["logw"].tobytes() == np.zeros((n, T, C)).tobytes()
        assert got["logw_draws"].tobytes() == np.zeros((n, T, C, S + 1)).tobytes()
        _consistent(capi, got, SEED, FIRST, 1)
        assert (got["accepts"] == S).all()  # equal weights: the ratio is 1 and u < 1


# ------------------------------------------------------------------ 7. errors
def _raw_rc(capi, ctx, n, d, T, C, S, flags, thin=1, precision=10, first=0):
    """lgs_imhk_bases itself, past the Python checks; returns its code."""
    b = np.tile(np.eye(max(d, 1)) * 3.0, (max(n, 1), 1, 1))
    t = np.zeros((max(n, 1), max(T, 1), max(d, 1)))
    s = np.ones(max(n, 1))
    return ctx._L.lgs_imhk_bases(ctx._h, 0, first, n, d, T, C, S, thin, capi._ptr(b), capi._ptr(t), capi._ptr(s),
                                 precision, None, None, None, flags)


def test_errors_leave_outputs_alone(capi):
    d, T, C, S = 3, 2, 3, 6
    Bs, Ts, idx = qr_oracle.batch(d, T, 3)
    sigma = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    ctx = capi.Context(0)
    for dev in (False, True):
        t = Ts.copy()
        t[2, 1, 0] = np.nan
        with pytest.raises(capi.LgsError) as e:
            _run(capi, ctx, Bs, t, sigma, C, S, dev=dev)
        assert e.value.code == capi.LGS_ERR_NONFINITE
        _sentinels_intact(_run.last)
        b = Bs.copy()
        b[1, 0, 2] = np.inf
        with pytest.raises(capi.LgsError) as e:
            _run(capi, ctx, b, Ts, sigma, C, S, dev=dev)
        assert e.value.code == capi.LGS_ERR_NONFINITE
        _sentinels_intact(_run.last)
        for bad in (0.0, -1.0, np.nan, np.inf):
            s = sigma.copy()
            s[1] = bad
            with pytest.raises(capi.LgsError) as e:
                _run(capi, ctx, Bs, Ts, s, C, S, dev=dev)
            assert e.value.code == capi.LGS_ERR_INVALID
            _sentinels_intact(_run.last)
    for flags in (capi.LGS_EXACT_ORDER, capi.LGS_COORD_MAJOR, capi.LGS_TARGETS_QFRAME, 0x1000):
        assert _raw_rc(capi, ctx, 2, 3, 2, 3, 6, flags) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 1, 2, 3, 6, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 65, 2, 3, 6, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 0, 3, 6, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 65, 3, 6, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 0, 6, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 3, -1, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 3, 6, 0, thin=0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 1 << 11, 1 << 10, 0) == capi.LGS_ERR_INVALID  # T C (S + 1) > 2^22
    assert _raw_rc(capi, ctx, 2, 3, 2, (1 << 21) + 1, 0, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 3, 6, 0, precision=0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, -1, 3, 2, 3, 6, 0) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 3, 6, 0, first=(1 << 32) - 11) == capi.LGS_ERR_INVALID  # 12 chains
    assert _raw_rc(capi, ctx, 0, 3, 2, 3, 6, 0, first=(1 << 32) + 1) == capi.LGS_ERR_INVALID
    assert _raw_rc(capi, ctx, 2, 3, 2, 3, 6, 0, first=(1 << 32) - 12) == capi.LGS_OK
    assert _raw_rc(capi, ctx, 0, 3, 2, 3, 6, 0) == capi.LGS_OK and _raw_rc(capi, ctx, 2, 3, 2, 3, 6, 0) == capi.LGS_OK
    # |z| near 10^12 / 3 in every draw
    big_b = np.array([[[3.0, 1.0], [0.0, 2.0]]])
    big_t = np.array([[[1e12, 0.25]]])
    big_s = np.array([2.0])
    with pytest.raises(capi.LgsError) as e:
        _run(capi, ctx, big_b, big_t, big_s, C, S)
    assert e.value.code == capi.LGS_ERR_OVERFLOW
    _sentinels_intact(_run.last)
    want = imhkb_oracle.solve(big_b[0], big_t[0], 2.0, C, S, SEED, FIRST)
    assert np.abs(want["z_draws"]).max() > 1 << 31 and want["settled"].all()
    for dev in (False, True):
        got = _run(capi, ctx, big_b, big_t, big_s, C, S, z64=True, dev=dev)
        assert _against_oracle(got, {k: np.asarray(a)[None] for k, a in want.items() if k != "fallbacks"}, big_b) == 0
    r = ctx.imhk_bases_host(SEED, FIRST, big_b, big_t, big_s, C, S, want_trace=True)  # the wrapper retries
    assert np.array_equal(r["z_draws"], want["z_draws"][None]) and np.array_equal(r["z"], want["z"][None])
    # the context is still usable
    good = imhkb_oracle.expected(d, T, 3, C, S)
    assert _against_oracle(_run(capi, ctx, Bs, Ts, sigma, C, S), good, Bs) == 0


# ------------------------------------------------------------------ 8. wrappers
def test_wrappers_agree_with_the_raw_call(capi):
    from lgs_amd.samplers import imhk_bases
    d, T, C, S, thin = 17, 5, 3, 30, 4
    Bs, Ts, idx = qr_oracle.batch(d, T, 3)
    sg = np.array([kleinb_oracle.sigma_for(v) for v in idx])
    raw = _run(capi, capi.Context(0), Bs, Ts, sg, C, S, thin)
    r = capi.Context(0).imhk_bases_host(SEED, FIRST, Bs, Ts, sg, C, S, thin, want_cprime=True, want_trace=True,
                                        want_samples=True)
    _same(r, raw)
    pts, z = imhk_bases(Bs, sg, Ts, n_chains=C, n_steps=S, seed=SEED, first_chain=FIRST, coefficients=True)
    assert pts.shape == (3, T, C, d) and np.array_equal(z, raw["z"]) and pts.tobytes() == raw["v"].tobytes()
    pts1, z1 = imhk_bases(np.swapaxes(Bs, 1, 2), sg, Ts, n_chains=C, n_steps=S, seed=SEED, first_chain=FIRST, rows=True,
                          coefficients=True)
    assert np.array_equal(z1, z) and pts1.tobytes() == pts.tobytes()
    kp, kz = imhk_bases(Bs, sg, Ts, n_chains=C, n_steps=S, thin=thin, seed=SEED, first_chain=FIRST, coefficients=True)
    assert kp.shape == (3, T, C, S // thin, d) and np.array_equal(kz, raw["z_samples"])
    for p in range(3):
        assert kp[p].tobytes() == kleinb_oracle.points(Bs[p], kz[p].reshape(-1, d)).tobytes()
    # one zero target per basis, a scalar width, the default chain ids: the T axis is dropped
    p0, z0 = imhk_bases(Bs, 300.0, n_chains=4, n_steps=5, seed=SEED, coefficients=True)
    one = capi.Context(0).imhk_bases_host(SEED, 0, Bs, np.zeros((3, 1, d)), np.full(3, 300.0), 4, 5)
    assert p0.shape == (3, 4, d) and np.array_equal(z0, one["z"][:, 0]) and p0.tobytes() == one["v"][:, 0].tobytes()


def test_reduce_runs_on_the_reduced_bases_and_maps_back(capi):
    """Raw qary_basis(16, 16, 3329) of three seeds: z = U z_reduced exactly, v = qr_oracle.point(B, z)
    bit for bit."""
    from lgs_amd import lattices
    from lgs_amd.samplers import imhk_bases
    d, T, C, S, sigma = 32, 2, 2, 8, 20.0
    Bs = np.stack([np.asarray(lattices.qary_basis(16, 16, 3329, seed)).T for seed in (1, 2, 3)]).astype(np.int64)
    rng = np.random.default_rng(51)
    z0 = rng.integers(-50, 51, size=(3, T, d))
    Ts = np.einsum("nij,ntj->nti", Bs, z0).astype(np.float64) + rng.uniform(-0.45, 0.45, size=(3, T, d))
    v, z = imhk_bases(Bs, sigma, Ts, n_chains=C, n_steps=S, seed=SEED, reduce=True, coefficients=True)
    ctx = capi.Context(0)
    lr = ctx.lll_reduce_host(Bs)
    assert not lr["status"].any()
    red = ctx.imhk_bases_host(SEED, 0, lr["basis"].astype(np.float64), Ts, np.full(3, sigma), C, S)
    assert 0 < red["accepts"].sum() < red["accepts"].size * S
    for p in range(3):
        for k in range(T):
            for j in range(C):
                zz = [int(x) for x in (lr["U"][p].astype(object) @ red["z"][p, k, j].astype(object))]
                assert z[p, k, j].tolist() == zz
                assert v[p, k, j].tobytes() == qr_oracle.point(Bs[p], z[p, k, j]).tobytes()


# ------------------------------------------------------------------ 9. the statistic
def test_exact_where_klein_is_biased(capi, oracle):
    """B = [[4,1],[1,3]] at sigma = 0.8, below the smoothing bound, 2^14 chains on the one target
    (1.7, -0.6), seed 7, through samplers.imhk_bases: the coefficients are the oracle's chains, so
    both total-variation distances from the exact D_{L,sigma,t} are the oracle's: 0.218 for Klein's
    draw, 0.0035 after 32 steps."""
    from lgs_amd.samplers import imhk_bases
    B = np.array([[4.0, 1.0], [1.0, 3.0]])
    sigma, t, n = 0.8, np.array([1.7, -0.6]), 1 << 14
    qs, R, cp = qr_oracle.qr(B, t[None])
    zz, p = d2_exact_pmf(B, sigma, t)
    _, z0 = imhk_bases(B[None], sigma, t[None], n_chains=n, n_steps=0, seed=7, coefficients=True)
    v32, z32 = imhk_bases(B[None], sigma, t[None], n_chains=n, n_steps=32, seed=7, coefficients=True)
    assert z32.shape == (1, n, 2) and np.array_equal(v32[0], z32[0].astype(np.float64) @ B.T)
    o0, _, _ = oracle.imhk_parallel(R, cp[0], B, sigma, n, 0, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    o32, _, _ = oracle.imhk_parallel(R, cp[0], B, sigma, n, 32, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    assert np.array_equal(z0[0], o0) and np.array_equal(z32[0], o32)
    tv0, tv32 = tv_distance(z0[0], zz, p), tv_distance(z32[0], zz, p)
    print(f"  TV(Klein) {tv0:.4f}, TV(32 steps) {tv32:.4f}")
    assert tv0 >= 0.15
    assert tv32 <= 0.02
