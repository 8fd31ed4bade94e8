"""Host side of tests/test_gpu_diag_shapes.py (no GPU).

1. The thresholds at which the launchers of csrc/lgs_diag.hip switch kernels, tiles,
   chunks and grid rows are read out of the source, and the case tables of
   tests/diag_shape_cases.py must have a case on each side of every one of them: a
   retune of a constant then fails here instead of silently un-covering a kernel.
2. Every reference and bound the device tests use (oracle/lgs_diag_oracle.py) is run
   against an independent NumPy computation: exact integers against object-int
   arithmetic, the longdouble sums and their worst-case bounds against honest fp64
   reorderings (NumPy's own product, a 16-row blocked sum, a reversed sum), the histogram
   against a one-value-at-a-time restatement of numpy's bin arithmetic.
"""
import functools
import os
import re

import numpy as np
import pytest

import diag_shape_cases as C
import lgs_diag_oracle as O
from conftest import PKG

LD = np.longdouble
SRC = open(os.path.join(PKG, "csrc", "lgs_diag.hip")).read()


def _one(pattern, flags=0):
    """The single integer every match of `pattern` in the source agrees on."""
    found = set(re.findall(pattern, SRC, flags))
    assert len(found) == 1, (pattern, found)
    return int(found.pop())


def _body(signature):
    """Source text of the function whose header matches `signature`, to its closing brace."""
    m = re.search(signature, SRC)
    assert m, signature
    i = SRC.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(SRC[j], 0)
        j += 1
        if depth == 0:
            return SRC[i:j]


K = {
    "hist_cols": _one(r"constexpr int kHistLdsCols = (\d+);"),
    "hist_bins": _one(r"constexpr int kHistLdsBins = (\d+);"),
    "acf_ch": _one(r"constexpr int kAcfCH = (\d+)"),
    "acf_lb": _one(r"kAcfLB = (\d+);"),
    "col_rows": _one(r"blockIdx\.y \* (\d+) \+ threadIdx\.x"),   # columns per grid row
    "i8_bound": _one(r"y > (\d+)\) \| \(y < -\d+\)"),
}


@functools.lru_cache(maxsize=None)
def _launcher_constants():
    """Each threshold is found in the launcher that applies it (so a rename or a moved
    rule fails here, rather than the regex quietly matching something else)."""
    chunk = _body(r"int64_t gram_chunk\(int64_t n, int nt\) ")
    K["kc_floor"] = int(re.search(r"if \(kc < (\d+)\) kc = \1;", chunk).group(1))
    K["kc_cap"] = int(re.search(r"if \(kc > (\d+)\) kc = \1;", chunk).group(1))
    K["kc_wgs"] = int(re.search(r"splits = \((\d+) \+ pairs - 1\) / pairs;", chunk).group(1))
    rows = re.search(r"tvd_rows\(int64_t n\) \{ return n < (\d+) \? 1 :", SRC)
    K["tvd_rows"] = int(rows.group(1))
    series = _body(r"hipError_t series_stats\(const SeriesArgs& a, hipStream_t st\) ")
    K["series_gx"] = int(re.search(r"a\.n_series < (\d+) \? a\.n_series : \1;", series).group(1))
    val = _body(r"void gram_val_kernel\(")
    m = re.search(r"constexpr int BT = (\d+), KS = (\d+);", val)
    K["val_bt"], K["val_ks"] = int(m.group(1)), int(m.group(2))
    gram = _body(r"hipError_t gram\(const void\* Z, int xtype,")
    assert re.search(rf"const int nt = \(d \+ {K['val_bt'] - 1}\) / {K['val_bt']};", gram)
    jump = _body(r"void jump_kernel\(")
    K["jump_lanes"] = int(re.search(r"for \(int i = lane; i < d; i \+= (\d+)\)", jump).group(1))
    K["jump_steps"] = int(re.search(r"blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\)", jump).group(1))
    for name in ("tvd_minmax", "tvd_hist", "hist_range", "hist_counts"):
        assert f"(d + {K['col_rows'] - 1}) / {K['col_rows']}" in _body(rf"hipError_t {name}\(const void\* x,"), name
    assert "d <= kHistLdsCols" in _body(r"hipError_t hist_range\(const void\* x,")
    assert "(int64_t)d * nb <= kHistLdsBins" in _body(r"hipError_t hist_counts\(const void\* x,")
    assert "tvd_rows(n)" in _body(r"hipError_t hist_counts\(const void\* x,")
    return K


def test_constants_are_where_the_tables_expect_them():
    _launcher_constants()
    assert K["i8_bound"] == C.GRAM_I8_BOUND
    assert all(isinstance(v, int) and v > 0 for v in K.values()), K


def _gram_chunks(n, d):
    """The launcher's K split (gram_chunk) restated: number of chunks of the VALU Gram."""
    _launcher_constants()
    nt = -(-d // K["val_bt"])
    pairs = nt * (nt + 1) // 2
    splits = -(-K["kc_wgs"] // pairs)
    kc = -(-n // splits)
    kc = -(-kc // 64) * 64
    kc = min(max(kc, K["kc_floor"]), K["kc_cap"])
    return -(-n // kc)


def test_case_tables_straddle_every_threshold():
    _launcher_constants()
    bt, ks = K["val_bt"], K["val_ks"]
    tiles = {-(-d // bt) for d in C.GRAM_D}
    assert 1 in tiles and 2 in tiles and max(tiles) >= 3        # diagonal only / one mirrored pair / several
    assert any(d % bt for d in C.GRAM_D) and any(d % bt == 0 for d in C.GRAM_D)
    for ns in (C.GRAM_INT_N, C.GRAM_F64_N):
        for d in C.GRAM_D:
            chunks = {_gram_chunks(n, d) for n in ns}
            assert 1 in chunks and max(chunks) >= 3, (d, chunks)  # one chunk, two, more
            assert 2 in chunks, (d, chunks)
        assert any(n < ks for n in ns) and any(n % ks for n in ns if n > ks)
        assert K["kc_floor"] - 1 in ns or any(n < K["kc_floor"] for n in ns)
        assert K["kc_floor"] + 1 in ns
    assert C.GRAM_INT_RANGE > K["i8_bound"]

    lanes, steps = K["jump_lanes"], K["jump_steps"]
    assert {lanes - 1, lanes, lanes + 1} <= set(C.JUMP_D) and max(C.JUMP_D) > 3 * lanes
    assert any(d > lanes and d % lanes for d in C.JUMP_D)
    assert any((n - 1) % steps for n in C.JUMP_N) and any((n - 1) % steps == 0 for n in C.JUMP_N)
    assert any(n - 1 > steps for n in C.JUMP_N) and min(C.JUMP_N) == 2

    cr, tr = K["col_rows"], K["tvd_rows"]
    assert {cr, cr + 1} <= set(C.TVD_D) and any(d % cr and d > cr + 1 for d in C.TVD_D)
    sizes = {n for pair in C.TVD_N for n in pair}
    assert {tr - 1, tr, 1} <= sizes and any(n > tr for n in sizes)

    hc, hb = K["hist_cols"], K["hist_bins"]
    ds = {d for d, _ in C.HIST_CASES}
    assert {hc, hc + 1} <= ds and any(d > hc + 1 for d in ds) and any(d < hc for d in ds)
    prods = {d * b for d, b in C.HIST_CASES}
    assert hb in prods and any(p > hb for p in prods) and any(p < hb for p in prods)
    assert min(p for p in prods if p > hb) <= hb + 64          # the first shape past the LDS store
    assert any(d > hc and d * b <= hb for d, b in C.HIST_CASES)  # wide range kernel, LDS counts
    assert any(d <= hc and d * b > hb for d, b in C.HIST_CASES)  # flat range kernel, per-column counts
    assert any(n < tr for n in C.HIST_N) and any(n >= tr for n in C.HIST_N)
    assert all(c in C.HIST_CASES for c in C.HIST_TVD_CASES)
    assert any(d > hc for d, _ in C.HIST_TVD_CASES) and any(d * b > hb for d, b in C.HIST_TVD_CASES)

    ch, lb = K["acf_ch"], K["acf_lb"]
    assert {ch - 1, ch, ch + 1, 2 * ch + 1} <= set(C.SERIES_N)
    for n in C.SERIES_N:
        assert {lb - 1, lb, lb + 1, n - 1} <= set(C.series_lags(n))
    assert C.SERIES_MANY[0] > K["series_gx"] and C.SERIES_MANY[0] % K["series_gx"]
    bs = C.batch_sizes(C.BATCH_N)
    assert 1 in bs and C.BATCH_N in bs and C.BATCH_N + 1 in bs
    assert any(1 < b < C.BATCH_N and C.BATCH_N % b for b in bs)


# ---------------------------------------------------------------- references and bounds
def _blocked_gram(y, rows=16):
    """fp64 Gram in the order of a staged kernel: partial products over blocks of rows."""
    G = np.zeros((y.shape[1], y.shape[1]))
    S = np.zeros(y.shape[1])
    for k in range(0, len(y), rows):
        G += y[k:k + rows].T @ y[k:k + rows]
        S += y[k:k + rows].sum(axis=0)
    return S, G


@pytest.mark.parametrize("d,n", [(65, 1025), (130, 3000), (64, 17), (65, 1)])
def test_f64_gram_reference_and_bound(d, n):
    r = C.rng(8, d, n)
    x = r.standard_normal((n, d)) * np.linspace(0.5, 3.0, d) + 10.0
    shift = x.mean(axis=0) + 0.125
    S_ref, G_ref, aS, aG = O.gram_longdouble(x, shift)
    bS, bG = O.gram_bounds(n, aS, aG)
    y = x - shift
    worst = 0.0
    for S, G in ((y.sum(axis=0), y.T @ y), _blocked_gram(y), _blocked_gram(y[::-1])):
        eS, eG = np.abs(S.astype(LD) - S_ref), np.abs(G.astype(LD) - G_ref)
        assert np.all(eS <= bS) and np.all(eG <= bG)
        worst = max(worst, float(np.max(eG / bG)), float(np.max(eS / bS)))
    assert worst < 0.5, worst   # honest reorderings sit well inside the worst case
    # accumulation: S0 / G0 are one more term of each sum
    G0 = r.standard_normal((d, d)) * 1e3
    S0 = r.standard_normal(d) * 1e3
    bS, bG = O.gram_bounds(n, aS, aG, S0, G0)
    S, G = _blocked_gram(y)
    assert np.all(np.abs((G0 + G).astype(LD) - (G_ref + G0)) <= bG)
    assert np.all(np.abs((S0 + S).astype(LD) - (S_ref + S0)) <= bS)
    # the longdouble sums themselves: exact on integer data
    z = r.integers(-40000, 40001, size=(min(n, 300), d))
    s_ex, G_ex = O.gram_exact(z)
    S_ld, G_ld, _, _ = O.gram_longdouble(z.astype(np.float64))
    if np.finfo(LD).nmant >= 63:
        assert all(int(a) == int(b) for a, b in zip(G_ld.ravel(), G_ex.ravel()))
        assert all(int(a) == int(b) for a, b in zip(S_ld, s_ex))


def test_int_gram_reference_is_exact():
    """The int64 product the device tests compare with equals the object-int Gram."""
    z = C.rng(1, 65, 1025).integers(-C.GRAM_INT_RANGE, C.GRAM_INT_RANGE + 1, size=(1025, 65))
    sh = C.rng(2).integers(-50, 51, size=65)
    y = z.astype(np.int64) - sh
    s_ex, G_ex = O.gram_exact(y)
    np.testing.assert_array_equal(y.T @ y, G_ex.astype(np.int64))
    np.testing.assert_array_equal(y.sum(0), s_ex)
    assert max(C.GRAM_INT_N) * C.GRAM_INT_RANGE ** 2 < 2 ** 62  # int64 cannot overflow at these sizes


@pytest.mark.parametrize("d", C.JUMP_D)
def test_jump_references(d):
    n = 6
    x = C.rng(10, d, n, 1 << 20).integers(-(1 << 20), (1 << 20) + 1, size=(n, d))
    sq = O.jump_sq_exact(x)
    assert sq == [sum(int(b - a) ** 2 for a, b in zip(x[t], x[t + 1])) for t in range(n - 1)]
    assert max(sq) < 2 ** 53
    ref = np.sqrt(np.array(sq, dtype=np.float64))
    got = O.jump_distance(x.astype(np.float64))            # fp64 throughout: exact sum, one sqrt
    assert np.all(np.abs(got - ref) <= np.spacing(ref))
    xf = C.rng(11, d, n).standard_normal((n, d)) * 100.0
    refl = O.jump_longdouble(xf)
    for got in (O.jump_distance(xf), np.sqrt((np.diff(xf, axis=0)[:, ::-1] ** 2).sum(axis=1))):
        assert np.all(np.abs(got.astype(LD) - refl) <= (d + 2) * O.U53 * refl)


def test_tvd_reference_matches_a_count_based_restatement():
    a, b = C.tvd_inputs(257, 255, 256)
    for i in (0, 1, 4, 9, 255, 256):
        lo = min(a[:, i].min(), b[:, i].min())
        c1 = np.bincount(a[:, i] - lo, minlength=1)
        c2 = np.bincount(b[:, i] - lo, minlength=1)
        m = max(len(c1), len(c2))
        c1, c2 = np.pad(c1, (0, m - len(c1))), np.pad(c2, (0, m - len(c2)))
        acc = 0.0
        for u, v in zip(c1, c2):        # ascending value order, absent values skipped
            if u or v:
                acc += abs(int(u) / len(a) - int(v) / len(b))
        assert O.tvd_discrete(a[:, i], b[:, i]) == 0.5 * acc
    assert a.min() < 0 and np.ptp(a, axis=0).max() > 100 * max(1, np.ptp(a, axis=0).min())


@pytest.mark.parametrize("d,bins", [(3, 64), (4, 3), (2, 1), (3, 16)])
def test_histogram_restatement_equals_numpy(d, bins):
    for x in (C.edge_data(d, bins, 255, 0), C.int_edge_data(d, 255, 0),
              C.rng(16, d, 255).integers(-90, 91, size=(255, d)).astype(np.int32)):
        for i in range(d):
            mn, mx = x[:, i].min(), x[:, i].max()
            want = np.histogram(x[:, i], bins=bins, range=(mn, mx))[0]
            np.testing.assert_array_equal(O.histogram_restated(x[:, i], bins, mn, mx), want)
            assert want.sum() == 255
    x = C.edge_data(2, bins, 255, 0)
    if bins > 1:  # the inputs do sit on the edges: numpy's own +-1 corrections are exercised
        e = np.linspace(x[:, 0].min(), x[:, 0].max(), bins + 1)
        assert np.isin(x[:, 0], e).sum() > 255 // 8


def test_series_references():
    ns, n, L = 200, C.SERIES_MANY[1], C.SERIES_MANY[2]
    X = C.rng(19).standard_normal((ns, n, 2))[:, :, 1] + 3.0
    mean, c0, acf, tau = O.series_stats_many(X, L)
    for s in range(ns):
        ref = O.autocorrelation_direct(X[s], L)
        np.testing.assert_allclose(acf[s], ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(tau[s], O.tau_window(ref), rtol=1e-12)
        assert mean[s] == np.mean(X[s])
    x = C.ar1(C.rng(18, 4097), [0.5, 0.9, 0.99], 4097)
    mean, c0, acf, tau = O.series_stats_many(x, 65)
    closes = []
    for s in range(3):
        ref = O.autocorrelation_direct(x[s], 65)
        np.testing.assert_allclose(acf[s], ref, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(tau[s], O.tau_window(ref), rtol=1e-9)
        t, k = 0.0, 0
        full = O.autocorrelation_direct(x[s], 4096)
        for k in range(1, len(full)):
            t += 2 * full[k]
            if k >= 5.0 * t:
                break
        closes.append(k)
    lb = 64
    assert closes[0] < lb <= closes[1] and closes[2] > lb + 1, closes  # a window per lag block


def test_integer_mean_and_batch_references():
    x = C.int64_mean_inputs()
    n = x.shape[1]
    assert len(x) == 4 and (x[:2] > 0).all() and (x[2:] < 0).all()
    for k in range(len(x)):
        total = int(x[k].astype(object).sum())
        assert total == sum(int(v) for v in x[k]) and 2 ** 61 <= abs(total) < 2 ** 62
        assert abs(total) % 512 == (257, 255)[k % 2]          # one unit beside the tie at 256
        want = float(total) / float(n)
        assert float(np.cumsum(x[k].astype(np.float64))[-1]) / float(n) != want
        # two units lost or gained on the way round the other way, and the mean shows it
        off = -2 if k % 2 == 0 else 2
        assert float(abs(total) + off) / float(n) != abs(want)
    r = C.rng(22)
    n = C.BATCH_N
    xi = r.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int64)
    xf = r.standard_normal(n) * 100.0 + 3.0
    for b in C.batch_sizes(n):
        bm = O.batch_means_exact(xi, b)
        assert bm.shape == (n // b,)
        np.testing.assert_array_equal(bm, [np.mean(xi[j * b:(j + 1) * b]) for j in range(n // b)])
        ref, asum = O.batch_means_longdouble(xf, b)
        for order in (1, -1):
            got = np.array([np.sum(xf[j * b:(j + 1) * b][::order]) / b for j in range(n // b)])
            assert got.shape == ref.shape and np.all(np.abs(got.astype(LD) - ref) <= b * O.U53 * asum)


def test_leading_dimension_arguments_reach_the_library():
    """_capi.Context.gram(ldx=, shape=) / jump_distance(ld=, shape=) pass the caller's leading
    dimension and logical shape; the defaults are the former values."""
    from lgs_amd import _capi

    class L:
        def lgs_gram(self, h, d, n, x, ldx, *rest):
            self.got = ("gram", d, n, ldx)
            return 0

        def lgs_jump_distance(self, h, n, d, x, ld, *rest):
            self.got = ("jump", n, d, ld)
            return 0

    c = object.__new__(_capi.Context)
    c._L, c._h = L(), None
    c._ck = lambda rc: None
    buf = np.zeros((5, 12))
    c.gram(buf, coord_major=True)
    assert c._L.got == ("gram", 5, 12, 12)
    c.gram(buf)
    assert c._L.got == ("gram", 12, 5, 12)
    c.gram(buf, coord_major=True, ldx=12, shape=(5, 9))
    assert c._L.got == ("gram", 5, 9, 12)
    c.jump_distance(buf, np.zeros(4))
    assert c._L.got == ("jump", 5, 12, 12)
    c.jump_distance(buf, np.zeros(4), ld=12, shape=(5, 9))
    assert c._L.got == ("jump", 5, 9, 12)
    with pytest.raises(ValueError):
        c.gram(buf, coord_major=True, ldx=13, shape=(5, 9))   # the buffer does not hold 4 * 13 + 9
    with pytest.raises(ValueError):
        c.jump_distance(buf, np.zeros(4), ld=8, shape=(5, 9))  # ld < d
    c._L = None  # nothing to destroy
