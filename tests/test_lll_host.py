"""CPU-side checks of LLL reduction (lgs_lll_reduce): the header declares the function, its
output struct and LGS_LLL_MAX_D; the ctypes mirror matches the header; both libraries export
the symbol; arguments are validated before anything reaches a device, in the library and in
Python; the product library reads no environment; and the oracle (tests/lll_oracle.py)
confirms the premises the device tests rest on -- it returns a unimodular transform of the
input, terminates on every test basis with work done, its iteration counts lie on both sides
of the slice the device test forces, and its outputs are reduced in exact arithmetic up to the
slack asserted below."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import lll_oracle
from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")


def test_header_declares_lll_reduce():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_lll_reduce\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_lll_reduce not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "int64_t n", "int64_t d", "const int64_t *basis", "double delta", "double eta",
                    "int64_t max_iters", "int64_t *basis_out", "int64_t *U_out", "const lgs_lll_outputs *out",
                    "uint32_t flags"]
    assert re.search(r"^#define LGS_LLL_MAX_D 64\s*$", txt, re.M)
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # no counter id added
    assert "lgs_lll_reduce reuses id 9" in txt  # lgs_timing_get's comment


def test_lll_outputs_struct_matches_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    m = re.search(r"typedef struct lgs_lll_outputs \{(.*?)\} lgs_lll_outputs;", txt, re.S)
    assert m, "struct lgs_lll_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int64_t *swaps", "int64_t *iters", "int64_t *passes", "int32_t *status", "double *gs_norm2"]
    assert [n for n, _ in _capi.LllOutputs._fields_] == ["swaps", "iters", "passes", "status", "gs_norm2"]
    assert all(t is ctypes.c_void_p for _, t in _capi.LllOutputs._fields_)
    assert ctypes.sizeof(_capi.LllOutputs) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_both_libraries_export_lll_reduce():
    from lgs_amd import _capi
    assert "lgs_lll_reduce" in _capi.EXPORTS and _capi.LGS_LLL_MAX_D == 64
    vp, i64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        L = _capi.load_library(path)
        fn = L.lgs_lll_reduce
        assert fn.argtypes == [vp, i64, i64, vp, f64, f64, i64, vp, vp, ctypes.POINTER(_capi.LllOutputs),
                               ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
        assert L.lgs_version() == 100
    assert callable(_capi.Context.lll_reduce) and callable(_capi.Context.lll_reduce_host)


def test_library_validates_before_any_device_call():
    """No device here and no context: the handle is a block of zeros the call must not read or
    hand to the runtime before it has rejected the arguments, each with its own message."""
    from lgs_amd import _capi
    L = _capi.load_library()
    fake = ctypes.create_string_buffer(1 << 16)
    B = np.array([[1, 0], [7, 1]], dtype=np.int64)
    Bo, Uo = np.zeros_like(B), np.zeros_like(B)

    def call(n=1, d=2, basis=B, delta=0.99, eta=0.51, max_iters=100, bo=Bo, uo=Uo, flags=0, ctx=fake):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.lgs_lll_reduce(ctx, n, d, p(basis), delta, eta, max_iters, p(bo), p(uo), None, flags)

    big = B.copy()
    big[1, 0] = 1 << 28
    neg = B.copy()
    neg[0, 1] = -(1 << 28)
    for kw, word in ((dict(ctx=None), "null context"), (dict(flags=_capi.LGS_Z64), "flags"),
                     (dict(flags=_capi.LGS_DEVICE_PTRS | _capi.LGS_COORD_MAJOR), "flags"),
                     (dict(d=1), "d = 1"), (dict(d=65), "d = 65"), (dict(delta=0.25), "delta"),
                     (dict(delta=1.0), "delta"), (dict(delta=float("nan")), "delta"), (dict(eta=0.5), "eta"),
                     (dict(eta=1.0), "eta"), (dict(max_iters=0), "max_iters"),
                     (dict(max_iters=(1 << 40) + 1), "max_iters"), (dict(n=-1), "n < 0"),
                     (dict(basis=None), "required"), (dict(bo=None), "required"), (dict(uo=None), "required"),
                     (dict(basis=big), "2^28"), (dict(basis=neg), "2^28")):
        assert call(**kw) == _capi.LGS_ERR_INVALID, kw
        assert word in L.lgs_last_error().decode(), (kw, L.lgs_last_error())
    assert call(n=0) == _capi.LGS_OK  # nothing to do: no device call either


def test_product_library_reads_no_environment():
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()
    assert 'hook("LGS_TEST_LLL_SLICE")' in src and 'getenv("LGS_TEST_LLL' not in src
    lll = open(os.path.join(CSRC, "lgs_lll.hip")).read()
    assert "getenv" not in lll and "printf" not in lll and "assert(" not in lll
    assert "csrc/lgs_lll.hip" in open(os.path.join(REPO, "lattice-gaussian-mcmc_amd", "Makefile")).read()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after bad arguments")


def _bare_context():
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = 0, 0, None, _NoLibrary()
    return c


def test_context_lll_reduce_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = _bare_context()
    B = np.zeros((3, 4, 4), dtype=np.int64)
    Bo, Uo = np.zeros_like(B), np.zeros_like(B)
    for bad in (np.zeros((4, 4), dtype=np.int64), np.zeros((3, 4, 5), dtype=np.int64),
                np.zeros((1, 1, 1), dtype=np.int64), np.zeros((1, 65, 65), dtype=np.int64)):
        with pytest.raises(ValueError):
            c.lll_reduce(bad, np.zeros_like(bad), np.zeros_like(bad))
        with pytest.raises(ValueError):
            c.lll_reduce_host(bad)
    for kw in (dict(delta=0.25), dict(delta=1.0), dict(delta="x"), dict(eta=0.5), dict(eta=1), dict(max_iters=0),
               dict(max_iters=2.5), dict(max_iters=(1 << 40) + 1), dict(max_iters=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            c.lll_reduce(B, Bo, Uo, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            c.lll_reduce_host(B, **kw)
    for bad_flags in (_capi.LGS_Z64, _capi.LGS_COORD_MAJOR, -1, 1.0, True):
        with pytest.raises(ValueError, match="flags"):
            c.lll_reduce(B, Bo, Uo, flags=bad_flags)
    with pytest.raises(ValueError, match="expected int64"):
        c.lll_reduce(B.astype(np.int32), Bo, Uo)
    with pytest.raises(ValueError, match="LGS_DEVICE_PTRS"):
        c.lll_reduce(B, Bo, Uo, flags=_capi.LGS_DEVICE_PTRS)  # host arrays with the device flag
    with pytest.raises(ValueError, match="U_out"):
        c.lll_reduce(B, Bo, np.zeros((3, 4, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="required"):
        c.lll_reduce(B, Bo, None)
    with pytest.raises(ValueError, match="status"):
        c.lll_reduce(B, Bo, Uo, status=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="gs_norm2"):
        c.lll_reduce(B, Bo, Uo, gs_norm2=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="int64"):
        c.lll_reduce_host(B.astype(np.float64))
    big = B.copy()
    big[2, 1, 3] = -(1 << 28)
    with pytest.raises(ValueError, match="2\\^28"):
        c.lll_reduce_host(big)


def test_reduction_module_validates_and_keeps_defaults():
    import inspect

    from lgs_amd import reduction
    from lgs_amd.decode import Decoder
    from lgs_amd.lattices import SimpleLattice
    for bad in (np.array([[1.5, 0], [0, 1]]), np.array([[np.nan, 0], [0, 1]]), np.array([["a", "b"], ["c", "d"]]),
                np.array([[float(1 << 28), 0], [0, 1]]), np.zeros((2, 3)), np.zeros(4), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError):
            reduction.lll_reduce(bad)
    sig = inspect.signature(reduction.lll_reduce).parameters
    assert (sig["delta"].default, sig["eta"].default, sig["rows"].default) == (0.99, 0.51, True)
    assert inspect.signature(reduction.LatticeReduction.lll_reduce).parameters["delta"].default == 0.75
    for fn in (Decoder.__init__, SimpleLattice.first_minimum, SimpleLattice.decode_cvp, SimpleLattice.gaussian_mass):
        assert inspect.signature(fn).parameters["reduce"].default is False
    assert inspect.signature(SimpleLattice.lll).parameters["delta"].default == 0.99
    # the quality measures on a basis whose values are known: rows (3, 0), (4, 5)
    lr = reduction.LatticeReduction.__new__(reduction.LatticeReduction)
    B = np.array([[3.0, 0.0], [4.0, 5.0]])
    assert lr.hermite_factor(B) == pytest.approx(3 / np.sqrt(15))
    assert lr.orthogonality_defect(B) == pytest.approx(3 * np.sqrt(41) / 15)
    prof = lr.basis_quality_profile(B)
    assert sorted(prof) == ["dimension", "gs_norms", "gs_ratio", "hermite_factor", "log_potential", "max_gs_norm",
                            "min_gs_norm", "orthogonality_defect"]
    assert prof["gs_norms"] == pytest.approx([3.0, 5.0]) and prof["gs_ratio"] == pytest.approx(5 / 3)
    assert prof["log_potential"] == pytest.approx(np.log(15))


def test_decoder_maps_coefficients_back_with_U():
    """z' on the reduced basis B U is U z' on the caller's: B (U z') = (B U) z'."""
    from lgs_amd.decode import Decoder
    dec = object.__new__(Decoder)
    B = np.array([[1, 0], [7, 1]], dtype=np.int64)
    U = np.array([[1, -3], [0, 1]], dtype=np.int64)
    dec._U = U
    zp = np.array([[2, 5], [-1, 4]], dtype=np.int64)
    z = dec._z(zp)
    assert z.dtype == np.int64 and np.array_equal(z @ B.T, zp @ (B @ U).T)
    assert np.allclose(dec._z(zp / 2.0) @ B.T, (zp / 2.0) @ (B @ U).T)
    dec._U = None
    assert dec._z(zp) is zp and dec._z(None) is None


# ---------------------------------------------------------------- premises, on the oracle
@pytest.mark.parametrize("name,delta", lll_oracle.CASES + (("qary12", 0.99),))
def test_oracle_returns_a_unimodular_transform(name, delta):
    """B U = B' exactly, |det U| = 1 (Bareiss, d <= 16), status 0 with swaps done: the parity
    cases and the end-to-end basis of the device tests."""
    B = lll_oracle.bases()[name].tolist()
    r = lll_oracle.reduced(name, delta)
    print(f"  {name} delta {delta}: iters {r['iters']}, swaps {r['swaps']}, passes {r['passes']}")
    assert r["status"] == 0 and r["swaps"] > 0 and r["passes"] >= r["iters"] >= r["swaps"]
    assert lll_oracle.matmul(B, r["U_out"]) == r["basis_out"]
    if len(B) <= 16:
        assert abs(lll_oracle.det_bareiss(r["U_out"])) == 1
        assert abs(lll_oracle.det_bareiss(r["basis_out"])) == abs(lll_oracle.det_bareiss(B))
    assert all(x > 0.0 for x in r["gs_norm2"])


def test_bareiss_determinant():
    assert lll_oracle.det_bareiss([[2, 0], [0, 3]]) == 6
    assert lll_oracle.det_bareiss([[0, 1], [1, 0]]) == -1
    assert lll_oracle.det_bareiss([[1, 2, 3], [4, 5, 6], [7, 8, 9]]) == 0
    assert lll_oracle.det_bareiss([[2, -1, 0], [1, 3, 5], [0, 4, 1]]) == -33


def test_iteration_counts_lie_on_both_sides_of_the_forced_slice():
    """The device slice test runs lll_oracle.SLICE iterations per launch: d2 and d3 stop inside
    the first launch, every other basis needs at least three."""
    it = {n: lll_oracle.reduced(n, 0.75)["iters"] for n in lll_oracle.NAMES}
    assert it["d2"] < lll_oracle.SLICE and it["d3"] < lll_oracle.SLICE
    assert all(v > 2 * lll_oracle.SLICE for n, v in it.items() if n not in ("d2", "d3"))
    kernels_h = open(os.path.join(CSRC, "lgs_kernels.h")).read()
    m = re.search(r"constexpr int64_t kLllSlice = 1 << (\d+);", kernels_h)
    assert m and int(m.group(1)) == 12
    # the default slice is straddled too: qary32 and up span launches, qary16 and below do not
    assert it["qary16"] < 1 << 12 < it["qary32"]


def test_oracle_stops_and_guards():
    o = lll_oracle.lll
    full = lll_oracle.reduced("qary8", 0.75)
    half = o(lll_oracle.bases()["qary8"].tolist(), 0.75, 0.51, full["iters"] // 2)
    assert half["status"] == 1 and half["iters"] == full["iters"] // 2 and half["swaps"] < full["swaps"]
    B = lll_oracle.bases()["qary8"].tolist()
    assert lll_oracle.matmul(B, half["U_out"]) == half["basis_out"]
    assert o(B, 0.75, 0.51, full["iters"])["status"] == 0  # the budget is checked before an iteration
    ident = o([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    assert (ident["status"], ident["swaps"], ident["iters"]) == (0, 0, 2)
    assert ident["U_out"] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for singular in ([[1, 1], [2, 2]], [[0, 1], [0, 5]], [[1, 2, 3], [4, 5, 6], [7, 8, 9]]):
        r = o(singular)
        assert r["status"] == 3, singular
        assert lll_oracle.matmul(singular, r["U_out"]) == r["basis_out"]
    r = o([[1, 1 << 23], [0, 1]])  # mu = 2^23: X beyond the guard, nothing applied
    assert r["status"] == 2 and r["basis_out"] == [[1, 1 << 23], [0, 1]] and r["U_out"] == [[1, 0], [0, 1]]
    r = o([[1, (1 << 22) - 1], [0, 1]])  # just inside
    assert r["status"] == 0 and r["basis_out"] == [[1, 0], [0, 1]]


# The excesses measured on the parity cases, in exact arithmetic on the oracle's outputs
# (DESIGN.md 6i): none.  The largest |mu| - eta is -3.6e-4 (qary32, delta 0.99) and the largest
# Lovasz deficit delta - (r_kk / r_{k-1,k-1} + mu_{k,k-1}^2) is -1.5e-4 (qary40, delta 0.99):
# every exact |mu| is below eta and every exact Lovasz condition holds, the fp64 Cholesky
# error (the only source of an excess) being orders of magnitude below the room the final
# bases leave.  16 times a measured excess of zero is zero.
MEASURED_MU_EXCESS = Fraction(0)
MEASURED_LOVASZ_DEFICIT = Fraction(0)


@pytest.mark.parametrize("name,delta", lll_oracle.CASES)
def test_oracle_output_is_reduced_in_exact_arithmetic(name, delta):
    r = lll_oracle.reduced(name, delta)
    mu_x, lov = lll_oracle.gso_excess(r["basis_out"], delta, 0.51)
    print(f"  {name} delta {delta}: max |mu| - eta = {float(mu_x):.3e}, max Lovasz deficit = {float(lov):.3e}")
    assert mu_x <= 16 * MEASURED_MU_EXCESS and lov <= 16 * MEASURED_LOVASZ_DEFICIT


# ---------------------------------------------------------------- premises of the dense, tie and large-Gram cases
@pytest.mark.parametrize("name", lll_oracle.DENSE_NAMES)
def test_dense_signed_bases_tell_the_parameters_apart(name):
    """The dense bases are dense and signed; at every pair of lll_oracle.DENSE_PARAMS the oracle
    ends with status 0 on a unimodular transform whose output is reduced in exact arithmetic (the
    slack of the q-ary cases: none); and from d = 7 on the three pairs take three different
    iteration counts, so a kernel that ignored delta or eta could not pass all three."""
    B = lll_oracle.bases()[name]
    d = B.shape[0]
    assert d == dict((n, dd) for n, dd, _ in lll_oracle.DENSE)[name] and d % 2 == (name != "dense64")
    assert np.count_nonzero(B) > 0.9 * d * d and (B < 0).sum() > d * d // 3 < (B > 0).sum()
    assert lll_oracle.det_bareiss(B.tolist()) != 0
    iters = []
    for delta, eta in lll_oracle.DENSE_PARAMS:
        r = lll_oracle.reduced(name, delta, eta=eta)
        assert r["status"] == 0 and r["passes"] >= r["iters"] >= r["swaps"]
        assert r["swaps"] > 0 or delta == 0.3  # (the lax pair leaves the small bases their order)
        assert lll_oracle.matmul(B.tolist(), r["U_out"]) == r["basis_out"]
        mu_x, lov = lll_oracle.gso_excess(r["basis_out"], delta, eta)
        print(f"  {name} ({delta}, {eta}): iters {r['iters']}, max |mu| - eta = {float(mu_x):.3e}, "
              f"max Lovasz deficit = {float(lov):.3e}")
        assert mu_x <= 16 * MEASURED_MU_EXCESS and lov <= 16 * MEASURED_LOVASZ_DEFICIT
        iters.append(r["iters"])
    if d >= 7:
        assert len(set(iters)) == 3, iters
    want = {"dense5": 16, "dense7": 36, "dense17": 391, "dense33": 873, "dense63": 2073, "dense64": 1994}
    assert iters[0] == want[name]
    if name == "dense17":
        assert iters == [391, 20, 550]


def test_rounding_ties_tell_half_even_from_half_away():
    """mu[1][0] of each tie basis is exactly the tie its name says.  With the rounding replaced by
    half-away-from-zero the oracle returns another basis for 2.5 and -2.5 (half-even rounds to
    +-2, half-away to +-3) and the same for 3.5 and 1.5 (both round to +-4 and +-2): the first two
    are the cases that can tell a kernel's rint from a round()."""
    mu = {"tie2.5": 2.5, "tie-2.5": -2.5, "tie3.5": 3.5, "tie1.5": 1.5, "tie6/4": 1.5}
    assert tuple(mu) == lll_oracle.TIE_NAMES
    for name, m in mu.items():
        B = lll_oracle.bases()[name].tolist()
        G = lll_oracle.gram(B)
        assert Fraction(G[1][0], G[0][0]) == Fraction(m) and float(G[1][0]) / float(G[0][0]) == m
        even, away = lll_oracle.lll(B), lll_oracle.lll(B, rnd=lll_oracle.half_away)
        assert even["status"] == away["status"] == 0 and even == lll_oracle.reduced(name, 0.99)
        assert (even["basis_out"] != away["basis_out"]) == (abs(m) == 2.5), name
    assert lll_oracle.reduced("tie2.5", 0.99)["basis_out"] == [[1, 1], [1, -1]]  # columns (1, 1), (1, -1)
    away = lll_oracle.lll(lll_oracle.TIES["tie2.5"].tolist(), rnd=lll_oracle.half_away)
    assert away["basis_out"] == [[-1, 1], [1, 1]]  # columns (-1, 1), (1, 1)
    assert [lll_oracle.half_away(x) for x in (2.5, -2.5, 3.5, -1.5, 0.5, 2.4999, -0.75)] == [3, -3, 4, -2, 1, 2, -1]
    assert [round(x) for x in (2.5, -2.5, 3.5, -1.5)] == [2, -2, 4, -2]


def test_gram_entries_above_2_to_53_round_on_conversion():
    """big4 ends with status 0 and big9 trips the magnitude guard late in its run; the Gram matrix
    of each holds an entry of 2^53 or more that fp64 cannot represent, so (double)G[k][j] has to
    round (to nearest even, as Python's float(int) does)."""
    bb = lll_oracle.big_bases()
    assert tuple(bb) == lll_oracle.BIG_NAMES and [bb[n].shape[0] for n in bb] == [4, 9]
    r4, r9 = (lll_oracle.reduced(n, 0.99) for n in lll_oracle.BIG_NAMES)
    assert (r4["status"], r4["iters"]) == (0, 15) and r9["status"] == 2 and r9["iters"] >= 30
    for name, r in (("big4", r4), ("big9", r9)):
        B = bb[name].tolist()
        assert np.abs(bb[name]).max() < lll_oracle.B_LIMIT and (bb[name] < 0).any()
        G = lll_oracle.gram(B)
        inexact = [g for row in G for g in row if abs(g) >= 1 << 53 and int(float(g)) != g]
        bits = max(G[i][i] for i in range(len(B))).bit_length()
        print(f"  {name}: {len(inexact)} Gram entries round, largest diagonal {bits} bits")
        assert inexact
        assert lll_oracle.matmul(B, r["U_out"]) == r["basis_out"]
    assert max(g.bit_length() for g in np.diag(np.array(lll_oracle.gram(bb["big4"].tolist()), dtype=object))) == 55


# ---------------------------------------------------------------- premises of the scheduling tests
def test_mixed_batch_spreads_over_the_launches():
    """lll_oracle.mixed_batch() under SLICE iterations per launch: the entries need many different
    numbers of launches, some leave the live list after the first and they do not all sit at the
    end (the list gets holes), one needs twenty or more; and at MIXED_MAX_ITERS status 0, 1 and 3
    meet in one call."""
    B, R = lll_oracle.mixed_batch(), lll_oracle.mixed_reduced()
    n = len(B)
    assert B.shape == (n, 17, 17) and len(R) == n == 3 * len(lll_oracle.MIXED_SEEDS) + 5
    need = [lll_oracle.launches(r) for r in R]
    print(f"  launches per entry: {need}")
    assert [lll_oracle.launches({"iters": i}, 16) for i in (0, 1, 16, 17, 32, 33)] == [1, 1, 1, 2, 2, 3]
    assert len(set(need)) >= 5 and max(need) >= 20
    first = [k for k, v in enumerate(need) if v == 1]
    assert len(first) >= 2 and any(any(need[j] > 1 for j in range(k + 1, n)) for k in first)
    assert max(first) < n - 1 and min(first) > 0
    ident = [k for k in range(n) if np.array_equal(B[k], np.eye(17, dtype=np.int64))]
    assert len(ident) == 1 and R[ident[0]]["iters"] == lll_oracle.SLICE and R[ident[0]]["swaps"] == 0
    red = [k for k in range(n) if B[k].tolist() == lll_oracle.reduced("dense17", 0.99)["basis_out"]]
    assert len(red) == 1 and R[red[0]]["swaps"] == 0 and R[red[0]]["U_out"] == R[ident[0]]["U_out"]
    sing = [k for k in range(n) if R[k]["status"] == 3]
    assert len(sing) == 2 and all(lll_oracle.det_bareiss(B[k].tolist()) == 0 for k in sing)
    assert R[sing[0]]["iters"] == 1 and R[sing[1]]["iters"] > lll_oracle.SLICE  # at once; only at k >= 2
    assert all(r["status"] == 0 for k, r in enumerate(R) if k not in sing)
    same = [(i, j) for i in range(n) for j in range(i + 1, n) if np.array_equal(B[i], B[j])]
    assert len(same) == 1 and R[same[0][0]] == R[same[0][1]]
    cut = lll_oracle.mixed_reduced(lll_oracle.MIXED_MAX_ITERS)
    st = [r["status"] for r in cut]
    assert st.count(0) >= 3 and st.count(1) >= 3 and st.count(3) == 2
    assert all(r["iters"] == lll_oracle.MIXED_MAX_ITERS for r in cut if r["status"] == 1)


def test_chunk_batch_crosses_the_scheduler_s_chunk():
    """kLllChunk is read out of the source: lll_oracle.chunk_batch() has more entries than one
    chunk holds, a singular basis is the last of the first chunk and another the first of the
    second, and the rest cycles 130 distinct bases (748 iterations in all)."""
    kernels_h = open(os.path.join(CSRC, "lgs_kernels.h")).read()
    m = re.search(r"constexpr int64_t kLllChunk = (\d+);", kernels_h)
    assert m, "kLllChunk not in lgs_kernels.h"
    chunk = int(m.group(1))
    B, idx = lll_oracle.chunk_batch()
    assert chunk < lll_oracle.CHUNK_N == len(B) == len(idx) < 2 * chunk and B.shape[1:] == (3, 3)
    assert lll_oracle.CHUNK_SINGULAR == (chunk - 1, chunk) and (idx[chunk - 1], idx[chunk]) == (-1, -2)
    R = lll_oracle.chunk_reduced()
    assert sorted(R) == [-2, -1] + list(range(lll_oracle.CHUNK_DISTINCT))
    assert R[-1]["status"] == R[-2]["status"] == 3
    good = [R[v] for v in range(lll_oracle.CHUNK_DISTINCT)]
    assert all(r["status"] == 0 for r in good) and sum(r["iters"] for r in good) == 748
    assert len({tuple(map(tuple, B[k])) for k in range(lll_oracle.CHUNK_DISTINCT)}) == lll_oracle.CHUNK_DISTINCT
    # both chunks hold entries that span launches at the slice of 2 that the device test forces
    for part in (idx[:chunk], idx[chunk:]):
        assert max(lll_oracle.launches(R[v], 2) for v in part) >= 3
        assert len({lll_oracle.launches(R[v], 2) for v in part}) >= 2
