"""GPU: the diagnostics kernels (csrc/lgs_diag.hip) at the shapes where their launchers
switch kernels, tiles, chunks and grid rows -- tests/test_gpu_diag.py feeds them the
reference's goldens, which are narrow (d <= 6 for TVD, d <= 5 for histograms, one
64-tile for the VALU Gram).  The case tables live in tests/diag_shape_cases.py;
tests/test_diag_shapes_host.py pins them against the constants of the source and checks
the references and bounds used here without a GPU.

References: exact integers (NumPy int64 / Python ints) for integer input -- equality;
np.longdouble sums with the worst-case fp64 bound of ANY summation order for real input
(oracle/lgs_diag_oracle.py: gram_bounds, jump_longdouble) -- derived, not tuned; the
project's own series tolerances (test_gpu_diag.py::test_series_long_and_strided_layouts)
for autocorrelations.  The launch count of lgs_timing_get(KERNEL_GRAM) tells the int8
MFMA route (one timed scope) from the int64 replay (a second one).
"""
import functools

import numpy as np
import pytest

import diag_shape_cases as C
import lgs_diag_oracle as O

pytestmark = pytest.mark.gpu
RT = 1e-10
LD = np.longdouble


@pytest.fixture(scope="module")
def D():
    from lgs_amd import diagnostics
    return diagnostics


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    c.timing_enable(True)
    yield c
    c.close()


def _gram(ctx, capi, x, **kw):
    """ctx.gram(x, **kw); returns the number of timed Gram scopes the call opened:
    1 = pack + int8 MFMA planes only (or the fp64 kernel), 2 = the int64 replay ran too."""
    n0 = ctx.timing_get(capi.KERNEL_GRAM)[1]
    ctx.gram(x, **kw)
    return ctx.timing_get(capi.KERNEL_GRAM)[1] - n0


def _run_int(ctx, capi, z, shift=None, **kw):
    d = z.shape[1]
    s = np.zeros(d, dtype=np.int64)
    G = np.zeros((d, d), dtype=np.int64)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.int64)
    scopes = _gram(ctx, capi, np.ascontiguousarray(z), shift=sh, sum_out=s, gram_out=G, **kw)
    return scopes, s, G


def _int_ref(z, shift=None):
    y = z.astype(np.int64) - (0 if shift is None else np.asarray(shift, dtype=np.int64))
    return y.sum(0), y.T @ y


@functools.lru_cache(maxsize=None)
def _replay_data(d, n):
    z = C.rng(1, d, n).integers(-C.GRAM_INT_RANGE, C.GRAM_INT_RANGE + 1, size=(n, d))
    z[-1, -1] = C.GRAM_INT_RANGE  # beyond the digit range whatever the draw
    z.setflags(write=False)
    return z, _int_ref(z)


# ====================================================================== Gram, integer replay
@pytest.mark.parametrize("n", C.GRAM_INT_N)
@pytest.mark.parametrize("d", C.GRAM_D)
def test_gram_int_replay(ctx, capi, d, n):
    """gram_val_kernel<int, long long>: off-diagonal tiles with the mirrored add
    (d > 64), several K chunks (n > 1024), ragged tiles and chunk tails."""
    z, (s_ref, G_ref) = _replay_data(d, n)
    assert np.abs(z).max() > C.GRAM_I8_BOUND
    for dt in (np.int32, np.int64):
        scopes, s, G = _run_int(ctx, capi, z.astype(dt))
        assert scopes == 2, "the int64 replay did not run"
        np.testing.assert_array_equal(s, s_ref)
        np.testing.assert_array_equal(G, G_ref)


def test_gram_int_shift_pushes_out_of_range(ctx, capi):
    d, n = 65, 1025
    r = C.rng(2)
    z = r.integers(-C.GRAM_I8_BOUND, C.GRAM_I8_BOUND + 1, size=(n, d))
    sh = r.integers(-50, 51, size=d)
    z[7, 3], sh[3] = C.GRAM_I8_BOUND, -5
    assert np.abs(z).max() <= C.GRAM_I8_BOUND < np.abs(z - sh).max()
    s_ref, G_ref = _int_ref(z, sh)
    for dt in (np.int32, np.int64):
        scopes, s, G = _run_int(ctx, capi, z.astype(dt), sh)
        assert scopes == 2
        np.testing.assert_array_equal(s, s_ref)
        np.testing.assert_array_equal(G, G_ref)


def test_gram_int_one_value_out_of_range_in_the_last_corner(ctx, capi):
    d, n = 130, 2500
    z = C.rng(3).integers(-30000, 30001, size=(n, d))
    z[-1, -1] = C.GRAM_INT_RANGE
    assert (np.abs(z) > C.GRAM_I8_BOUND).sum() == 1
    s_ref, G_ref = _int_ref(z)
    for dt in (np.int32, np.int64):
        scopes, s, G = _run_int(ctx, capi, z.astype(dt))
        assert scopes == 2
        np.testing.assert_array_equal(s, s_ref)
        np.testing.assert_array_equal(G, G_ref)


@pytest.mark.parametrize("d,n", [(130, 1025), (65, 2500)])
def test_gram_int_digit_range_boundary(ctx, capi, d, n):
    """+-32639 everywhere stays on the MFMA planes; a single +-32640 takes the replay."""
    z = C.rng(4, d, n).choice([-C.GRAM_I8_BOUND, C.GRAM_I8_BOUND], size=(n, d))
    for dt in (np.int32, np.int64):
        scopes, s, G = _run_int(ctx, capi, z.astype(dt))
        s_ref, G_ref = _int_ref(z)
        assert scopes == 1, "values within the digit range must stay on the int8 MFMA route"
        np.testing.assert_array_equal(s, s_ref)
        np.testing.assert_array_equal(G, G_ref)
        for v, (i, j) in ((C.GRAM_I8_BOUND + 1, (n // 2, d - 1)), (-C.GRAM_I8_BOUND - 1, (n - 1, 0))):
            z1 = z.copy()
            z1[i, j] = v
            scopes, s, G = _run_int(ctx, capi, z1.astype(dt))
            s_ref1, G_ref1 = _int_ref(z1)
            assert scopes == 2, v
            np.testing.assert_array_equal(s, s_ref1)
            np.testing.assert_array_equal(G, G_ref1)


@pytest.mark.parametrize("hi", [200, C.GRAM_INT_RANGE])
def test_gram_int_accumulates_into_nonzero_outputs(ctx, capi, hi):
    d, n = 65, 1025
    r = C.rng(5, hi)
    z = r.integers(-hi, hi + 1, size=(n, d)).astype(np.int32)
    z[0, 0] = hi
    G0 = r.integers(-10 ** 9, 10 ** 9, size=(d, d))
    G0 = G0 + G0.T
    s0 = r.integers(-10 ** 9, 10 ** 9, size=d)
    s, G = s0.copy(), G0.copy()
    scopes = _gram(ctx, capi, z, sum_out=s, gram_out=G)
    assert scopes == (2 if hi > C.GRAM_I8_BOUND else 1)
    s_ref, G_ref = _int_ref(z)
    np.testing.assert_array_equal(s, s0 + s_ref)
    np.testing.assert_array_equal(G, G0 + G_ref)


@pytest.mark.parametrize("hi", [200, C.GRAM_INT_RANGE])
@pytest.mark.parametrize("d,n", [(65, 1025), (130, 2500)])
def test_gram_int_coordinate_major_padded(ctx, capi, d, n, hi):
    """Coordinate-major input at ldx = n + 37; the padding holds 2^30, so a kernel that
    read it would report a wrong (and still in-bounds) result."""
    z = C.rng(6, d, n, hi).integers(-hi, hi + 1, size=(n, d))
    z[-1, -1] = hi
    s_ref, G_ref = _int_ref(z)
    for dt in (np.int32, np.int64):
        buf = np.full((d, n + C.GRAM_PAD), 2 ** 30, dtype=dt)
        buf[:, :n] = z.T
        s = np.zeros(d, dtype=np.int64)
        G = np.zeros((d, d), dtype=np.int64)
        scopes = _gram(ctx, capi, buf, sum_out=s, gram_out=G, coord_major=True, ldx=n + C.GRAM_PAD,
                       shape=(d, n))
        assert scopes == (2 if hi > C.GRAM_I8_BOUND else 1)
        np.testing.assert_array_equal(s, s_ref)
        np.testing.assert_array_equal(G, G_ref)


@pytest.mark.parametrize("hi", [200, C.GRAM_INT_RANGE])
def test_gram_int_device_pointers_one_output(ctx, capi, hi):
    """Device pointers with only gram_out, or only sum_out: the other accumulator is the
    library's own staging buffer."""
    import torch
    d, n = 65, 1025
    z = C.rng(7, hi).integers(-hi, hi + 1, size=(n, d))
    z[-1, -1] = hi
    s_ref, G_ref = _int_ref(z)
    zt = torch.from_numpy(z).cuda()
    g = torch.zeros((d, d), dtype=torch.int64, device="cuda")
    ctx.gram(zt, gram_out=g, flags=capi.LGS_DEVICE_PTRS)
    np.testing.assert_array_equal(g.cpu().numpy(), G_ref)
    s = torch.zeros(d, dtype=torch.int64, device="cuda")
    ctx.gram(zt, sum_out=s, flags=capi.LGS_DEVICE_PTRS)
    np.testing.assert_array_equal(s.cpu().numpy(), s_ref)
    s.zero_()
    g.zero_()
    ctx.gram(zt, sum_out=s, gram_out=g, flags=capi.LGS_DEVICE_PTRS)
    np.testing.assert_array_equal(s.cpu().numpy(), s_ref)
    np.testing.assert_array_equal(g.cpu().numpy(), G_ref)


# ====================================================================== Gram, fp64
@functools.lru_cache(maxsize=None)
def _f64_data(d, n):
    r = C.rng(8, d, n)
    x = r.standard_normal((n, d)) * np.linspace(0.5, 3.0, d) + 10.0
    shift = x.mean(axis=0) + 0.125
    x.setflags(write=False)
    return x, shift, O.gram_longdouble(x, shift), O.gram_longdouble(x, None)


def _check_f64(s, G, ref, n, S0=None, G0=None, what=""):
    S_ref, G_ref, aS, aG = ref
    if S0 is not None:
        S_ref, G_ref = S_ref + S0, G_ref + G0
    bS, bG = O.gram_bounds(n, aS, aG, S0, G0)
    eS, eG = np.abs(s.astype(LD) - S_ref), np.abs(G.astype(LD) - G_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{what}: max err / bound  S {np.nanmax(eS / bS):.3g}  G {np.nanmax(eG / bG):.3g}")
    assert np.all(eS <= bS), what
    assert np.all(eG <= bG), what


@pytest.mark.parametrize("n", C.GRAM_F64_N)
@pytest.mark.parametrize("d", C.GRAM_D)
def test_gram_f64_layouts(ctx, capi, d, n):
    """gram_val_kernel<double, double>: several tiles and K chunks, row-major (through
    the transpose) and coordinate-major at ldx > n with 1e300 in the padding."""
    x, shift, ref_sh, ref_0 = _f64_data(d, n)
    xr = np.ascontiguousarray(x)
    for sh, ref, tag in ((shift, ref_sh, "shift"), (None, ref_0, "no shift")):
        s, G = np.zeros(d), np.zeros((d, d))
        assert _gram(ctx, capi, xr, shift=sh, sum_out=s, gram_out=G) == 1
        _check_f64(s, G, ref, n, what=f"row-major d={d} n={n} {tag}")
        buf = np.full((d, n + C.GRAM_PAD), 1e300)
        buf[:, :n] = x.T
        s, G = np.zeros(d), np.zeros((d, d))
        ctx.gram(buf, shift=sh, sum_out=s, gram_out=G, coord_major=True, ldx=n + C.GRAM_PAD, shape=(d, n))
        _check_f64(s, G, ref, n, what=f"coordinate-major d={d} n={n} {tag}")
    r = C.rng(9, d, n)
    G0 = r.standard_normal((d, d)) * 1e3
    G0 = G0 + G0.T
    S0 = r.standard_normal(d) * 1e3
    s, G = S0.copy(), G0.copy()
    ctx.gram(xr, shift=shift, sum_out=s, gram_out=G)
    _check_f64(s, G, ref_sh, n, S0, G0, what=f"accumulate d={d} n={n}")


def test_gram_f64_device_tensors(ctx, capi):
    import torch
    d, n = 130, 1025
    x, shift, ref_sh, _ = _f64_data(d, n)
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    st = torch.from_numpy(shift).cuda()
    s = torch.zeros(d, dtype=torch.float64, device="cuda")
    g = torch.zeros((d, d), dtype=torch.float64, device="cuda")
    ctx.gram(xt, shift=st, sum_out=s, gram_out=g, flags=capi.LGS_DEVICE_PTRS)
    _check_f64(s.cpu().numpy(), g.cpu().numpy(), ref_sh, n, what="device row-major")
    buf = torch.full((d, n + C.GRAM_PAD), 1e300, dtype=torch.float64, device="cuda")
    buf[:, :n] = xt.T
    g.zero_()
    ctx.gram(buf, shift=st, gram_out=g, coord_major=True, ldx=n + C.GRAM_PAD, shape=(d, n),
             flags=capi.LGS_DEVICE_PTRS)
    _check_f64(s.cpu().numpy(), g.cpu().numpy(), ref_sh, n, what="device coordinate-major, gram only")


# ====================================================================== jump distances
def _padded(x, ld, poison):
    """x (n, d) inside an (n, ld) buffer whose padding differs from row to row."""
    n, d = x.shape
    buf = np.empty((n, ld), dtype=x.dtype)
    buf[:, :d] = x
    buf[:, d:] = poison(np.arange(n))[:, None]
    return buf


@pytest.mark.parametrize("n", C.JUMP_N)
@pytest.mark.parametrize("d", C.JUMP_D)
def test_jump_distance_shapes(ctx, d, n):
    """jump_kernel: a second trip of the lane-strided loop with a ragged tail (d > 64),
    a ragged last block (n - 1 not a multiple of 4), row pitch ld > d."""
    for dt, amp in ((np.int32, 30000), (np.int64, 1 << 20)):
        x = C.rng(10, d, n, amp).integers(-amp, amp + 1, size=(n, d)).astype(dt)
        sq = O.jump_sq_exact(x)
        assert max(sq) < 2 ** 53
        ref = np.sqrt(np.array(sq, dtype=np.float64))
        for ld in (d, d + C.JUMP_PAD):
            buf = _padded(x, ld, lambda t: 2 ** 30 - 7919 * t)
            out = np.full(n - 1, np.nan)
            ctx.jump_distance(buf, out, ld=ld, shape=(n, d))
            assert np.all(np.abs(out - ref) <= np.spacing(ref)), (dt, ld, out, ref)
    x = C.rng(11, d, n).standard_normal((n, d)) * 100.0
    ref = O.jump_longdouble(x)
    for ld in (d, d + C.JUMP_PAD):
        buf = _padded(x, ld, lambda t: np.where(t % 2 == 0, 1e300, -1e300))
        out = np.full(n - 1, np.nan)
        ctx.jump_distance(buf, out, ld=ld, shape=(n, d))
        assert np.all(np.abs(out.astype(LD) - ref) <= (d + 2) * O.U53 * ref), (ld, out, ref)


def test_jump_distance_device_tensor(ctx, capi):
    import torch
    d, n = 200, 6
    x = C.rng(12).integers(-30000, 30001, size=(n, d))
    ref = np.sqrt(np.array(O.jump_sq_exact(x), dtype=np.float64))
    buf = torch.from_numpy(_padded(x, d + C.JUMP_PAD, lambda t: 2 ** 30 - 7919 * t)).cuda()
    out = torch.empty(n - 1, dtype=torch.float64, device="cuda")
    ctx.jump_distance(buf, out, ld=d + C.JUMP_PAD, shape=(n, d), flags=capi.LGS_DEVICE_PTRS)
    assert np.all(np.abs(out.cpu().numpy() - ref) <= np.spacing(ref))


# ====================================================================== discrete TVD
@functools.lru_cache(maxsize=None)
def _tvd_data(d, n1, n2):
    a, b = C.tvd_inputs(d, n1, n2)
    ref = np.array([O.tvd_discrete(a[:, k], b[:, k]) for k in range(d)])
    return a, b, ref


@pytest.mark.parametrize("n1,n2", C.TVD_N)
@pytest.mark.parametrize("d", C.TVD_D)
def test_marginal_tvd_shapes(ctx, d, n1, n2):
    """tvd_minmax / tvd_hist / tvd_sum with a second grid row of 256 columns, on both
    sides of the 256-row switch of the rows-per-block rule: bit-identical per column."""
    a, b, ref = _tvd_data(d, n1, n2)
    assert a.min() < 0
    for dt in (np.int32, np.int64, np.float64):
        out = np.full(d, np.nan)
        ctx.marginal_tvd(np.ascontiguousarray(a.astype(dt)), np.ascontiguousarray(b.astype(dt)), out)
        np.testing.assert_array_equal(out, ref, err_msg=str(dt))


def test_marginal_tvd_device_tensors(ctx, capi, D):
    import torch
    d, n1, n2 = 257, 500, 300
    a, b, ref = _tvd_data(d, n1, n2)
    at, bt = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.empty(d, dtype=torch.float64, device="cuda")
    ctx.marginal_tvd(at, bt, out, flags=capi.LGS_DEVICE_PTRS)
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    assert D.compute_tvd(at, bt) == O.tvd_discrete(a, b) == np.mean(list(ref))


# ====================================================================== column range, histogram
def _check_range_and_counts(ctx, D, x, bins):
    n, d = x.shape
    lo, hi = np.full(d, np.nan), np.full(d, np.nan)
    ctx.column_range(x, lo, hi)
    np.testing.assert_array_equal(lo, x.min(axis=0))
    np.testing.assert_array_equal(hi, x.max(axis=0))
    edges = np.empty((d, bins + 1))
    fd = np.empty((d, 2))
    want = np.empty((d, bins), dtype=np.int64)
    for i in range(d):
        mn, mx = x[:, i].min(), x[:, i].max()
        edges[i], fd[i] = D.convergence_diag._bin_setup(mn, mx, bins)
        want[i] = np.histogram(x[:, i], bins=bins, range=(mn, mx))[0]
    c = np.full((d, bins), -1, dtype=np.int64)
    ctx.histogram(x, edges, fd, c)
    np.testing.assert_array_equal(c, want)
    assert (c.sum(axis=1) == n).all()


@pytest.mark.parametrize("n", C.HIST_N)
@pytest.mark.parametrize("d,bins", C.HIST_CASES)
def test_column_range_and_histogram_shapes(ctx, D, d, bins, n):
    """hist_range_cols_kernel (d > 512) against hist_range_flat_kernel, hist_cols_kernel
    (d bins > 8192) against hist_flat_kernel: numpy's counts, column by column."""
    _check_range_and_counts(ctx, D, C.edge_data(d, bins, n, 0), bins)
    _check_range_and_counts(ctx, D, C.int_edge_data(d, n, 0), bins)
    _check_range_and_counts(ctx, D, C.rng(16, d, n).integers(-90, 91, size=(n, d)).astype(np.int32), bins)


@pytest.mark.parametrize("d", [513, 600])
def test_column_range_rejects_nonfinite_on_the_wide_route(ctx, capi, d):
    n = 300
    xi = C.int_edge_data(d, n, 1)
    xi[n - 1, d - 1] = 2 ** 53 + 2
    lo, hi = np.empty(d), np.empty(d)
    with pytest.raises(capi.LgsError) as e:
        ctx.column_range(xi, lo, hi)
    assert e.value.code == capi.LGS_ERR_NONFINITE
    xf = C.edge_data(d, 3, n, 1)
    xf[5, 300] = np.nan
    with pytest.raises(capi.LgsError) as e:
        ctx.column_range(xf, lo, hi)
    assert e.value.code == capi.LGS_ERR_NONFINITE
    xf[5, 300] = 0.0  # and the context goes on working
    ctx.column_range(xf, lo, hi)
    np.testing.assert_array_equal(lo, xf.min(axis=0))


@pytest.mark.parametrize("d,bins", C.HIST_TVD_CASES)
def test_binned_tvd_wide(D, d, bins):
    import torch
    r = C.rng(17, d, bins)
    a = r.standard_normal((300, d)) * np.linspace(0.1, 30.0, d) - 2.0
    b = r.standard_normal((255, d)) * np.linspace(0.1, 30.0, d) - 1.5
    want = O.tvd_binned(a, b, bins)
    assert D.compute_tvd(a, b, bins=bins) == want
    assert D.compute_tvd(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), bins=bins) == want
    ai, bi = np.round(a).astype(np.int64), np.round(b).astype(np.int64)
    assert D.compute_tvd(ai, bi, bins=bins) == O.tvd_binned(ai, bi, bins)


# ====================================================================== series statistics
@pytest.mark.parametrize("n", C.SERIES_N)
def test_series_chunk_and_lag_block_boundaries(n):
    """series_stats_kernel at n around the 4096-value staging chunk and max_lag around
    the 64-lag block, three chains x steps x d in place.  AR(0.9) closes its window near
    lag 95, in the second lag block; AR(0.5) in the first; AR(0.99) in none of the short ones."""
    from lgs_amd.diagnostics import _gpu
    nc, d = 3, 2
    x = np.ascontiguousarray(C.ar1(C.rng(18, n), np.repeat([0.5, 0.9, 0.99], d), n)
                             .reshape(nc, d, n).transpose(0, 2, 1))
    full = [[O.autocorrelation_direct(x[c, :, i], n - 1) for i in range(d)] for c in range(nc)]
    lay = dict(n_series=nc * d, n=n, group_size=d, group_stride=n * d, series_stride=1, time_stride=d)
    for L in C.series_lags(n):
        r = _gpu.series_stats(x, **lay, max_lag=L, want=("mean", "c0", "acf", "tau"))
        r2 = _gpu.series_stats(x, **lay, max_lag=L, want=("tau",))
        assert r["acf"].shape == (nc * d, L + 1)
        for c in range(nc):
            for i in range(d):
                s = c * d + i
                ref = full[c][i][:L + 1]
                np.testing.assert_allclose(r["acf"][s], ref, rtol=1e-9, atol=1e-12, err_msg=f"L={L} s={s}")
                np.testing.assert_allclose(r["tau"][s], O.tau_window(ref), rtol=1e-9)
                assert r2["tau"][s] == r["tau"][s]
                np.testing.assert_allclose(r["mean"][s], np.mean(x[c, :, i]), rtol=1e-12)
                xc = x[c, :, i] - np.mean(x[c, :, i])
                np.testing.assert_allclose(r["c0"][s], np.dot(xc, xc), rtol=1e-9)


def test_series_more_than_65536_series():
    """The second grid row of series_stats (n_series > 65536), in the layout the
    sharded driver passes: one coordinate of a chains x steps x d trace, group_size 1."""
    from lgs_amd.diagnostics import _gpu
    ns, n, L = C.SERIES_MANY
    d = 2
    X = C.rng(19).standard_normal((ns, n, d)) + 3.0
    view = _gpu.offset_view(X, 1)
    r = _gpu.series_stats(view, n_series=ns, n=n, group_size=1, group_stride=n * d, series_stride=0,
                          time_stride=d, max_lag=L, want=("mean", "c0", "acf", "tau"))
    mean, c0, acf, tau = O.series_stats_many(X[:, :, 1], L)
    np.testing.assert_allclose(r["mean"], mean, rtol=1e-12)
    np.testing.assert_allclose(r["c0"], c0, rtol=1e-9)
    np.testing.assert_allclose(r["acf"], acf, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r["tau"], tau, rtol=1e-9)
    for s in range(ns - 3, ns):
        ref = O.autocorrelation_direct(X[s, :, 1], L)
        np.testing.assert_allclose(r["acf"][s], ref, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(r["tau"][s], O.tau_window(ref), rtol=1e-9)
        np.testing.assert_allclose(r["mean"][s], np.mean(X[s, :, 1]), rtol=1e-12)


def test_series_int32_columns_of_a_row_major_matrix():
    import torch
    from lgs_amd.diagnostics import _gpu
    n, d, L = 4097, 3, 65
    x = np.round(C.ar1(C.rng(20), [0.5, 0.9, 0.0], n).T * 100).astype(np.int32)
    x = np.ascontiguousarray(x)
    for xin in (x, torch.from_numpy(x).cuda()):
        r = _gpu.series_stats(xin, **_gpu.columns(xin), max_lag=L, want=("mean", "acf", "tau"))
        for i in range(d):
            assert r["mean"][i] == float(int(x[:, i].astype(np.int64).sum())) / float(n)
            ref = O.autocorrelation_direct(x[:, i].astype(np.float64), L)
            np.testing.assert_allclose(r["acf"][i], ref, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(r["tau"][i], O.tau_window(ref), rtol=1e-9)


def test_series_int64_mean_beyond_2_53():
    """The integer sum is exact in int64 and rounded once: float(sum) / float(n).  An
    fp64 accumulation of these values rounds on the way and gives another mean (the sums
    sit one unit beside a rounding tie of float64, see int64_mean_inputs)."""
    from lgs_amd.diagnostics import _gpu
    x = C.int64_mean_inputs()
    ns, n = x.shape
    r = _gpu.series_stats(x, n_series=ns, n=n, group_size=1, group_stride=n, series_stride=0,
                          time_stride=1, want=("mean",))
    for k in range(ns):
        total = sum(int(v) for v in x[k])
        assert abs(total) > 2 ** 53
        want = float(total) / float(n)
        assert float(np.cumsum(x[k].astype(np.float64))[-1]) / float(n) != want
        assert r["mean"][k] == want, k


def test_series_batch_means_with_a_remainder():
    from lgs_amd.diagnostics import _gpu
    n = C.BATCH_N
    assert n % 7 != 0
    r = C.rng(22)
    xi = r.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int64)
    xf = r.standard_normal(n) * 100.0 + 3.0
    for b in C.batch_sizes(n):
        for x in (xi, xi.astype(np.int32)):
            bm = _gpu.series_stats(x, **_gpu.columns(x), batch_size=b, want=("bmeans",))["bmeans"]
            assert bm.shape == (1, n // b)
            np.testing.assert_array_equal(bm[0], O.batch_means_exact(x, b))
        bm = _gpu.series_stats(xf, **_gpu.columns(xf), batch_size=b, want=("bmeans",))["bmeans"]
        assert bm.shape == (1, n // b)
        ref, asum = O.batch_means_longdouble(xf, b)
        assert np.all(np.abs(bm[0].astype(LD) - ref) <= b * O.U53 * asum), b
    # several series, each with its own batches (row pitch of the output = n // b)
    X = r.integers(-10 ** 6, 10 ** 6, size=(n, 5)).astype(np.int64)
    bm = _gpu.series_stats(X, **_gpu.columns(X), batch_size=7, want=("bmeans",))["bmeans"]
    for i in range(5):
        np.testing.assert_array_equal(bm[i], O.batch_means_exact(X[:, i], 7))


def test_diagnose_chain_wide_int64(D):
    n, d = 400, 200
    x = np.round(C.ar1(C.rng(23), np.linspace(0.0, 0.9, d), n).T * 20).astype(np.int64)
    got, want = D.diagnose_chain(np.ascontiguousarray(x)), O.diagnose_chain(x)
    assert got["n_samples"] == want["n_samples"] == n
    for k in ("mean", "std", "ess", "ess_per_sample", "tau_int", "mean_jump_distance", "acf_lag_1",
              "acf_lag_10"):
        np.testing.assert_allclose(got[k], want[k], rtol=RT, atol=1e-13, err_msg=k)
