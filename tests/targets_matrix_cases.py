"""Case table of tests/test_gpu_targets_matrix.py, importable without a GPU.

The per-target entry points (lgs_klein_targets, lgs_klein_decode, lgs_imhk_targets) launch
through klein_targets_zt / klein_targets_any in csrc/lgs_kernels.hip, which pick the kernel
from the panel height, the store width, the trailing lanes argument and LGS_EXACT_ORDER.
This table says which test case launches which instantiation; tests/test_targets_matrix_host.py
reads the two launchers out of the source and checks the table against them."""
import itertools

import numpy as np

PANELS = (32, 16)                 # Context(panel=...): LGS_CTX_PANEL16
SAMPLEZ = ("table", "libm")       # Context(samplez_libm=...): a.szc is null under libm
STORES = ("z32", "z64")           # LGS_Z64
ORDERS = ("default", "exact")     # LGS_EXACT_ORDER
VARIANTS = tuple(itertools.product(PANELS, SAMPLEZ, STORES))

STORE_TYPES = {"z32": "int32_t", "z64": "int64_t"}
# entry point -> (the trailing lanes argument of its certified kernel, its reference-order kernel,
#                 the test of the cross)
ENTRIES = {
    "klein_targets": (None, "klein_targets_exact_kernel", "test_klein_targets_vs_oracle"),
    "klein_decode": ("DecodeLanes", "klein_decode_exact_kernel", "test_klein_decode_winners_and_bounds"),
    "imhk_targets": ("WeightLanes", "klein_imhk_exact_kernel", "test_imhk_targets_vs_oracle"),
}


def variant_id(panel, samplez, store):
    return f"p{panel}-{samplez}-{store}"


VARIANT_IDS = tuple(variant_id(*v) for v in VARIANTS)


def instantiation(entry, panel, store, order):
    """The kernel instantiation a call of `entry` launches, spelled as the source spells it."""
    lanes, exact_kernel, _ = ENTRIES[entry]
    zt = STORE_TYPES[store]
    if order == "exact":  # (the reference-order kernels have no panels)
        return f"{exact_kernel}<{zt}>"
    return f"klein_targets_kernel<{zt}, {panel}" + (f", {lanes}>" if lanes else ">")


def launched():
    """instantiation -> the ids of the cases that launch it (every basis runs every one)."""
    out = {}
    for entry, (_, _, test) in ENTRIES.items():
        for (panel, samplez, store), order in itertools.product(VARIANTS, ORDERS):
            out.setdefault(instantiation(entry, panel, store, order), []).append(
                f"{test}[*-{variant_id(panel, samplez, store)}-{order}]")
    return out


# ------------------------------------------------------------------ bases
# name -> why it is here; d is the smallest at which the layout edge appears
BASES = {
    "q130": "d = 130: PB = 32 gives 4 full panels and a 2-row bottom panel, PB = 16 gives 8 and 2 rows",
    "gauss37": "d = 37, real: a bottom panel of 5 rows",
    "qary40": "d = 40: a bottom panel of 8 rows",
    "gauss17": "d = 17, real: one row below a 16-row panel",
    "int12": "d = 12: a single panel, no far field",
}
N_TARGETS = 300
N_FIRST = ((1, 0), (63, 5), (64, 1000), (300, 77))  # (n, first) of the lgs_klein_targets cases


def make_setups():
    """Per basis: B, sigma, Q, R and 300 targets, as test_gpu_klein_decode._setup builds them
    (shared, read-only)."""
    from lgs_amd import lattices
    from test_gpu_klein_decode import _setup
    rng = np.random.default_rng(12)  # gauss37 and int12 as the per-target modules draw them
    g37 = rng.standard_normal((37, 37)) * 6.0 + 25.0 * np.eye(37)
    i12 = np.rint(rng.standard_normal((12, 12)) * 4.0) + 40.0 * np.eye(12)
    g17 = np.random.default_rng(13).standard_normal((17, 17)) * 6.0 + 25.0 * np.eye(17)
    raw = {
        "q130": (lattices.qary_basis(65, 65, 3329, 3), 165.7, True),
        "gauss37": (g37, 30.0, False),
        "qary40": (lattices.qary_basis(20, 20, 3329, 5), 165.7, True),
        "gauss17": (g17, 30.0, False),
        "int12": (i12, 45.0, True),
    }
    out = {}
    for name in BASES:
        s = _setup(*raw[name], n_targets=N_TARGETS)
        s.update(name=name, cp0=np.zeros(s["d"]), qframe=False)
        out[name] = s
    return out


# ------------------------------------------------------------------ precision / linear probabilities
# The parameter set of test_gpu_kernel_matrix.test_samplez_kinds_precision_linear_every_kernel.
PRECISIONS = (3, 10, 20)
LINEAR = (False, True)
# qary40 and q130 are the bases the matrix is specified on.  Their sigma_i are either below
# 0.1 or so wide that the window's 500 cap decides, and no (precision, linear) setting
# changes one oracle row there (a kernel that ignored both would pass), so the matrix also
# runs on the basis of every SampleZ kind, where precision 3 changes every row and
# linear-space probabilities take the oracle's fallback and change half of them.
PRECISION_BASES = ("qary40", "q130", "kinds")
PRECISION_N_FIRST = ((300, 77), (64, 1000))
PRECISION_CHAINS = (8, 30, 1000)  # (n, n_steps, first_chain) of the lgs_imhk_targets run


def make_kinds_setup():
    """The basis of every SampleZ kind of test_gpu_kernel_matrix (d = 100, R only) with 300
    centres in the Q frame: c' + k_i R_ii with integers k_i, which shift every mean by whole
    numbers and keep the top coordinate's half-integer mean (the case linear-space
    probabilities decide by the fallback)."""
    from test_gpu_kernel_matrix import KINDS_SIGMA, _kinds_basis
    R, cp = _kinds_basis()
    d = R.shape[0]
    T = cp[None, :] + np.diag(R)[None, :] * np.random.default_rng(2100).integers(-3, 4, (N_TARGETS, d))
    for a in (R, cp, T):
        a.setflags(write=False)
    return dict(name="kinds", B=None, sigma=KINDS_SIGMA, integral=True, Q=None, R=R, T=T, d=d, cp0=cp, qframe=True)


# ------------------------------------------------------------------ lgs_klein_decode, lgs_imhk_targets
def decode_cases(d):
    """(n, K, first): CASES of test_gpu_klein_decode, cut to 256 lanes at d = 130."""
    from test_gpu_klein_decode import CASES
    return tuple(c for c in CASES if d <= 40 or c[:2] in ((1, 1), (5, 3), (4, 64)))


def imhk_cases(d):
    """(n, n_steps, first_chain): 8 to 64 chains of 30 and 6 steps (K = 31 and 7 draws: a
    chain's lanes straddle waves and the last wave is padded); at d = 130 at most 300 lanes."""
    return ((8, 30, 0), (64 if d <= 40 else 40, 6, 1000))


FIXED_CENTRE = (9, 30, 1000)      # (n, n_steps, first_chain): a row equal to the context's c'
FORCED = {                        # forced resolution under panel 16, qary40: per entry point its arguments
    "klein_targets": (128, 9),    # (n, first)
    "klein_decode": (32, 16, 3),  # (n, K, first)
    "imhk_targets": (64, 6, 9),   # (n, n_steps, first_chain)
}
