"""Case tables of the diagnostics shape tests, shared by tests/test_gpu_diag_shapes.py
(which runs them on the device) and tests/test_diag_shapes_host.py (which checks, against
the constants read out of csrc/lgs_diag.hip, that they still fall on both sides of every
threshold at which a launcher switches kernels or grid shapes).

Every shape is the smallest at which the route in question is taken: a second 64-tile
(d = 65), a third (d = 130), a second K chunk (n > 1024), a second 256-column grid row,
a second trip of a lane-strided loop, one element past a staging chunk.
"""
import numpy as np

# ---- Gram (lgs_gram): d x n; 64-wide output tiles, K chunks of >= 1024 samples
GRAM_D = (64, 65, 130)
GRAM_INT_N = (1, 1023, 1025, 2500)
GRAM_F64_N = (1, 17, 1025, 3000)
GRAM_INT_RANGE = 40000          # |x| beyond the two-digit bound: the int64 replay runs
GRAM_I8_BOUND = 32639           # largest |x - shift| the int8-digit MFMA route takes
GRAM_PAD = 37                   # ldx = n + GRAM_PAD in the coordinate-major cases

# ---- jump distances (lgs_jump_distance): 64 lanes over d, 4 steps per block
JUMP_D = (63, 64, 65, 200)
JUMP_N = (2, 5, 6)
JUMP_PAD = 3                    # ld = d + JUMP_PAD

# ---- discrete TVD (lgs_marginal_tvd): 256 columns per grid row, one row per block below 256 rows
TVD_D = (256, 257, 300)
TVD_N = ((500, 300), (255, 256), (1, 1))

# ---- column range and histogram (lgs_column_range, lgs_histogram)
HIST_CASES = ((128, 64), (129, 64), (130, 64), (600, 3), (513, 1), (512, 16))  # (d, bins)
HIST_N = (255, 300)
HIST_TVD_CASES = ((600, 3), (130, 64))

# ---- series statistics (lgs_series_stats): 4096-value staging chunks, 64-lag blocks
SERIES_N = (4095, 4096, 4097, 8193)


def series_lags(n):
    return (63, 64, 65, n - 1)


SERIES_MANY = (65536 + 3, 5, 2)  # n_series, n, max_lag


def batch_sizes(n):
    return (1, 7, n, n + 1)


BATCH_N = 300                    # 300 % 7 = 6: a remainder that no batch takes


def rng(*key):
    """The generator of one case: a fixed seed per case key."""
    return np.random.default_rng([20240611, *[int(k) for k in key]])


# ---- inputs shared by the device tests and their host-side checks
def edge_data(d, bins, n, key):
    """Float columns whose values sit on, one ulp below and one ulp above the
    np.linspace edges of their own range (and on the bin midpoints)."""
    r = rng(14, d, bins, n, key)
    x = np.empty((n, d))
    for i in range(d):
        lo, hi = -3.0 - 0.37 * i, 5.0 + 0.11 * i
        e = np.linspace(lo, hi, bins + 1)
        pool = np.concatenate([e, np.nextafter(e[1:], -np.inf), np.nextafter(e[:-1], np.inf),
                               0.5 * (e[:-1] + e[1:])])
        x[:, i] = r.choice(pool, size=n)
        x[0, i], x[1, i] = lo, hi
    return x


def int_edge_data(d, n, key):
    r = rng(15, d, n, key)
    special = np.array([2 ** 52, 2 ** 52 + 1, 2 ** 52 - 1, -(2 ** 52), -(2 ** 52) + 1, 5, 0, -7], dtype=np.int64)
    x = r.integers(-(2 ** 52), 2 ** 52, size=(n, d), dtype=np.int64)
    m = r.random((n, d)) < 0.5
    x[m] = r.choice(special, size=int(m.sum()))
    return x


def ar1(r, phi, n):
    """(len(phi), n) AR(1) series with unit innovations, offset 0.3."""
    phi = np.asarray(phi, dtype=np.float64)
    e = r.standard_normal((len(phi), n))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0]
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x + 0.3


def tvd_inputs(d, n1, n2):
    """Integer sample sets with negative values and per-column centres / widths that
    differ by orders of magnitude, so that each column's offset into the shared count
    store matters."""
    r = rng(13, d, n1, n2)
    i = np.arange(d)
    centre = (i % 7 - 3) * 1000 * (i % 3)
    width = np.array([0, 1, 5, 50, 1000])[i % 5]
    a = centre + r.integers(-width, width + 1, size=(n1, d))
    b = centre + (i % 2) + r.integers(-width, width + 1, size=(n2, d))
    return a, b


def int64_mean_inputs(n=4000):
    """Four int64 series of n values near +-2^50: |sum| is in [2^61, 2^62), where float64
    steps by 512, and the last value is set so that |sum| mod 512 is 257 (series 0, 2) or
    255 (series 1, 3): one unit beside the rounding tie.  Only an exact integer sum rounded
    once gives float(sum) / float(n); a sum that lost two units on the way, in either
    direction, rounds the other way in one of each pair."""
    x = (2 ** 50 + 2 * rng(21).integers(0, 2 ** 20, size=(4, n)) + 1).astype(np.int64)
    for k, want in enumerate((257, 255, 257, 255)):
        x[k, -1] += (want - sum(int(v) for v in x[k])) % 512
    x[2:] = -x[2:]
    return x
