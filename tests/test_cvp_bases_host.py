"""CPU-side checks of exact closest vectors over a batch of bases (lgs_closest_vector_bases):
the header declares the function and its output struct and the ctypes mirror matches it field
for field; the Python entry points validate their arguments before anything reaches a device;
the transcription of QR(p) (tests/qr_oracle.py) agrees with NumPy's QR; the coefficient mapping
of reduce=True is exact; and the premises of the device tests hold on the transcription -- every
parity problem ends with status 0 far below the budget used there."""
import ctypes
import os
import re

import numpy as np
import pytest

import qr_oracle
from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")
FIELDS = ["double *dist2", "int64_t *nodes", "int32_t *status", "int32_t *qr_status", "double *R", "double *cprime"]


def test_header_declares_closest_vector_bases():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_closest_vector_bases\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_closest_vector_bases not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "int64_t n_bases", "int64_t d", "int64_t T", "const double *bases",
                    "const double *targets", "const double *radius2", "int64_t max_nodes", "void *z_out",
                    "double *v_out", "const lgs_cvp_bases_outputs *out", "uint32_t flags"]
    assert re.search(r"^#define LGS_CVPB_MAX_T 64\s*$", txt, re.M)
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # the counter ids stay a closed range
    assert "lgs_closest_vector_bases: its input check and QR launches are id 7" in txt  # lgs_timing_get's list


def test_library_exports_closest_vector_bases():
    from lgs_amd import _capi
    assert "lgs_closest_vector_bases" in _capi.EXPORTS and _capi.LGS_CVPB_MAX_T == 64
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        fn = _capi.load_library(path).lgs_closest_vector_bases
        assert fn.argtypes == [vp, i64, i64, i64, vp, vp, vp, i64, vp, vp, ctypes.POINTER(_capi.CvpBasesOutputs),
                               ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
    assert callable(_capi.Context.closest_vector_bases) and callable(_capi.Context.closest_vector_bases_host)


def test_cvp_bases_outputs_struct_matches_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    m = re.search(r"typedef struct lgs_cvp_bases_outputs \{(.*?)\} lgs_cvp_bases_outputs;", txt, re.S)
    assert m, "struct lgs_cvp_bases_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == FIELDS
    assert [n for n, _ in _capi.CvpBasesOutputs._fields_] == [f.split("*")[1] for f in FIELDS]
    assert all(t is ctypes.c_void_p for _, t in _capi.CvpBasesOutputs._fields_)
    assert ctypes.sizeof(_capi.CvpBasesOutputs) == len(FIELDS) * ctypes.sizeof(ctypes.c_void_p)


def test_switches_live_in_the_hooks_library_only():
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()
    assert 'hook("LGS_TEST_CVPB_SLICE")' in src and 'hook("LGS_TEST_CVPB_SLOTS")' in src
    assert 'getenv("LGS_TEST_CVPB' not in src
    for name in ("lgs_cvpb.hip", "lgs_cvp_loop.h"):
        txt = open(os.path.join(CSRC, name)).read()
        assert "getenv" not in txt and "printf" not in txt and "assert(" not in txt
    assert "csrc/lgs_cvpb.hip" in open(os.path.join(REPO, "lattice-gaussian-mcmc_amd", "Makefile")).read()


class _NoLibrary:
    """A library handle that fails the test when anything is called on it."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after bad arguments")


def _bare_context():
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = 0, 0, None, _NoLibrary()
    return c


def test_context_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = _bare_context()
    B, T = np.zeros((3, 4, 4)), np.zeros((3, 2, 4))
    bad_pairs = [(np.zeros((3, 4, 5)), T), (np.zeros((4, 4)), T), (B, np.zeros((3, 2, 5))), (B, np.zeros((2, 2, 4))),
                 (B, np.zeros((3, 4))), (np.zeros((3, 65, 65)), np.zeros((3, 2, 65))), (B, np.zeros((3, 65, 4))),
                 (B, np.zeros((3, 0, 4))), (np.zeros((3, 1, 1)), np.zeros((3, 2, 1)))]
    for b, t in bad_pairs:
        with pytest.raises(ValueError):
            c.closest_vector_bases(b, t, 100)
        with pytest.raises(ValueError):
            c.closest_vector_bases_host(b, t, 100)
    for bad_nodes in (0, -1, (1 << 40) + 1, 2.5, None, True, "7"):
        with pytest.raises(ValueError, match="max_nodes"):
            c.closest_vector_bases(B, T, bad_nodes)
        with pytest.raises(ValueError, match="max_nodes"):
            c.closest_vector_bases_host(B, T, bad_nodes)
    for bad_flags in (_capi.LGS_EXACT_ORDER, _capi.LGS_COORD_MAJOR, _capi.LGS_TARGETS_QFRAME, 0x1000, -1, 1.0, True):
        with pytest.raises(ValueError, match="flags"):
            c.closest_vector_bases(B, T, 100, flags=bad_flags)
    with pytest.raises(ValueError):
        c.closest_vector_bases_host(B, T, 100, flags=_capi.LGS_DEVICE_PTRS)
    # dtypes, host / device, shapes of the outputs
    with pytest.raises(ValueError, match="expected float64"):
        c.closest_vector_bases(B.astype(np.float32), T, 100)
    with pytest.raises(ValueError, match="expected float64"):
        c.closest_vector_bases(B, T.astype(np.int64), 100)
    with pytest.raises(ValueError, match="expected int64"):
        c.closest_vector_bases(B, T, 100, z_out=np.zeros((3, 2, 4), dtype=np.int32), flags=_capi.LGS_Z64)
    with pytest.raises(ValueError, match="expected int32"):
        c.closest_vector_bases(B, T, 100, z_out=np.zeros((3, 2, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="host buffer"):
        c.closest_vector_bases(B, T, 100, flags=_capi.LGS_DEVICE_PTRS)
    for name, arr in (("z_out", np.zeros((3, 4, 2), dtype=np.int32)), ("v_out", np.zeros((3, 2, 5))),
                      ("dist2", np.zeros((3, 3))), ("nodes", np.zeros(6, dtype=np.int64)),
                      ("status", np.zeros((2, 3), dtype=np.int32)), ("qr_status", np.zeros((3, 2), dtype=np.int32)),
                      ("R", np.zeros((3, 4, 3))), ("cprime", np.zeros((3, 4, 2))), ("radius2", np.zeros(3))):
        with pytest.raises(ValueError, match=name):
            c.closest_vector_bases(B, T, 100, **{name: arr})
    with pytest.raises(ValueError, match="radius2"):
        c.closest_vector_bases_host(B, T, 100, radius2=np.full((3, 2), -1.0))


class _StubContext:
    """Stands in for _capi.Context: records every call that would reach the device."""

    def __init__(self):
        self.calls = []

    def lll_reduce_host(self, basis, *a, **kw):
        self.calls.append(("lll_reduce_host", basis.shape))
        n, d, _ = basis.shape
        U = np.tile(np.eye(d, dtype=np.int64), (n, 1, 1))
        U[:, 0, 1] = 2  # column 1 of the "reduced" basis is b_1 + 2 b_0
        status = np.zeros(n, dtype=np.int32)
        status[-1] = 1  # the last basis did not finish: it is decoded unreduced
        return {"basis": basis @ U, "U": U, "status": status}

    def closest_vector_bases_host(self, bases, targets, max_nodes, radius2=None, **kw):
        self.calls.append(("closest_vector_bases_host", bases.copy(), targets.shape, max_nodes,
                           None if radius2 is None else radius2.copy(), kw))
        n, T, d = targets.shape
        z = np.tile(np.arange(1, d + 1, dtype=np.int64), (n, T, 1))
        return {"z": z if kw.get("want_z", True) else None, "v": np.einsum("nij,ntj->nti", bases, z.astype(float)),
                "dist2": np.zeros((n, T)), "nodes": np.ones((n, T), dtype=np.int64),
                "status": np.zeros((n, T), dtype=np.int32), "qr_status": np.zeros(n, dtype=np.int32),
                "R": np.zeros((n, d, d)), "cprime": None}


def test_decode_entry_point_validates_before_any_device_call():
    from lgs_amd.decode import closest_vector_bases
    ctx = _StubContext()
    B = np.tile(np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 1.0, 5.0]]), (2, 1, 1))
    for bases, targets in ((B[0], np.zeros((2, 3))), (np.zeros((2, 3, 4)), np.zeros((2, 3))), (B, np.zeros(3)),
                           (B, np.zeros((3, 3))), (B, np.zeros((2, 2, 4))), (B, np.zeros((2, 65, 3))),
                           (np.zeros((2, 65, 65)), np.zeros((2, 65))), (np.zeros((2, 1, 1)), np.zeros((2, 1))),
                           (B.astype(complex), np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            closest_vector_bases(bases, targets, context=ctx)
    for bad_nodes in (0, 2.5, None, True, (1 << 40) + 1):
        with pytest.raises(ValueError, match="max_nodes"):
            closest_vector_bases(B, np.zeros((2, 3)), max_nodes=bad_nodes, context=ctx)
    with pytest.raises(ValueError, match="radius2"):
        closest_vector_bases(B, np.zeros((2, 3)), radius2=-1.0, context=ctx)
    with pytest.raises(ValueError, match="integral"):
        closest_vector_bases(B + 0.5, np.zeros((2, 3)), reduce=True, context=ctx)
    with pytest.raises(ValueError, match="2\\^28"):
        closest_vector_bases(B * float(1 << 28), np.zeros((2, 3)), reduce=True, context=ctx)
    assert ctx.calls == []
    # shapes of good calls: one target per basis, several, rows=True, a scalar radius
    v, info = closest_vector_bases(B, np.zeros((2, 3)), context=ctx)
    assert v.shape == (2, 3) and info["dist2"].shape == (2,) and info["qr_status"].shape == (2,)
    v, z, info = closest_vector_bases(B, np.zeros((2, 4, 3)), radius2=9.0, rows=True, coefficients=True, context=ctx)
    assert v.shape == (2, 4, 3) and z.shape == (2, 4, 3) and info["status"].shape == (2, 4) and "lll_status" not in info
    assert [c[0] for c in ctx.calls] == ["closest_vector_bases_host"] * 2
    assert np.array_equal(ctx.calls[1][1], np.swapaxes(B, 1, 2)) and ctx.calls[1][2] == (2, 4, 3)
    assert np.array_equal(ctx.calls[1][4], np.full((2, 4), 9.0)) and ctx.calls[1][3] == 1 << 24


def test_reduce_maps_coefficients_back_exactly():
    """A hand-made case: U = [[1, 2, 0], [0, 1, 0], [0, 0, 1]], z_red = (1, 2, 3) gives z = U z_red =
    (5, 2, 3) for the basis LLL finished on and z_red itself for the one it did not."""
    from lgs_amd.decode import closest_vector_bases, map_coefficients
    ctx = _StubContext()
    B = np.tile(np.array([[4, 1, 0], [1, 3, 0], [0, 1, 5]], dtype=np.int64), (2, 1, 1))
    v, z, info = closest_vector_bases(B, np.zeros((2, 3)), reduce=True, coefficients=True, context=ctx)
    assert [c[0] for c in ctx.calls] == ["lll_reduce_host", "closest_vector_bases_host"]
    assert np.array_equal(info["lll_status"], [0, 1])
    assert np.array_equal(z, [[5, 2, 3], [1, 2, 3]])
    decoded = ctx.calls[1][1]  # the bases the search ran in: reduced, and the caller's own where LLL failed
    assert np.array_equal(decoded[0], B[0] @ np.array([[1, 2, 0], [0, 1, 0], [0, 0, 1]])) and np.array_equal(decoded[1], B[1])
    for p in range(2):  # the same lattice point in either basis
        assert np.array_equal(B[p] @ z[p], v[p])
    # Python integers: a product beyond int64 is an error, one that fits only as a whole is exact
    big = np.array([[[1 << 40, 0], [0, 1]]], dtype=np.int64)
    assert np.array_equal(map_coefficients(big, np.array([[[1 << 22, 7]]])), [[[1 << 62, 7]]])
    with pytest.raises(ValueError, match="int64"):
        map_coefficients(big, np.array([[[1 << 23, 7]]]))
    U = np.array([[[(1 << 40) - 1, -(1 << 40)], [1, 1]]], dtype=np.int64)  # partial products cancel
    assert np.array_equal(map_coefficients(U, np.array([[[1 << 30, 1 << 30]]])), [[[-(1 << 30), 1 << 31]]])


# ---------------------------------------------------------------- the transcription against NumPy
def _numpy_qr(B):
    Q, R = np.linalg.qr(B, mode="complete")
    sgn = np.where(np.diag(R) < 0, -1.0, 1.0)  # klein.py:69-73
    return Q * sgn[None, :], R * sgn[:, None]


def _qr_cases():
    from lgs_amd import lattices
    rng = np.random.default_rng(17)
    return {"qary64": np.asarray(lattices.qary_basis(32, 32, 3329), dtype=np.float64).T,
            "ntru64": np.asarray(lattices.ntru_basis(32, 12289), dtype=np.float64).T,
            "int17": np.rint(rng.standard_normal((17, 17)) * 8.0) + 20.0 * np.eye(17),
            "d2": np.array([[4.0, 1.0], [1.0, 3.0]])}


@pytest.mark.parametrize("name", ["qary64", "ntru64", "int17", "d2"])
def test_transcription_agrees_with_numpy_qr(name):
    """Measured on these bases, in units of d 2^-53 times the scale on the right:
    max|R - R_np| 0.08 ||B||_F, max|c' - Q^T t| 1.12 ||t||, max|R^T R - B^T B| 0.30 ||B||_F^2.  The
    bounds are 8 times those: above what two correct QRs differ by, far below what a wrong sign
    or a wrong order gives (those are errors of order 1 in the same units times 2^53)."""
    B = _qr_cases()[name]
    d = B.shape[0]
    t = np.random.default_rng(1000 + d).standard_normal((4, d)) * 2500.0
    qs, R, cp = qr_oracle.qr(B, t)
    Q, Rn = _numpy_qr(B)
    assert qs == 0 and (np.diag(R) > 0).all() and not np.tril(R, -1).any()
    assert not np.signbit(np.tril(R, -1)).any()  # +0.0 below the diagonal
    u = d * 2.0 ** -53
    fro = np.linalg.norm(B)
    eR = np.abs(R - Rn).max() / (u * fro)
    ec = max(np.abs(cp[k] - Q.T @ t[k]).max() / (u * np.linalg.norm(t[k])) for k in range(4))
    eG = np.abs(R.T @ R - B.T @ B).max() / (u * fro * fro)
    print(f"  {name}: R {eR:.3f}, c' {ec:.3f}, R^T R {eG:.3f}")
    assert eR <= 8 * 0.08 and ec <= 8 * 1.12 and eG <= 8 * 0.30


def test_transcription_refuses_a_dependent_or_zero_column():
    B = np.array([[2.0, 1.0, 2.0], [0.0, 3.0, 0.0], [1.0, 1.0, 1.0]])  # column 2 repeats column 0
    t = np.ones((2, 3))
    qs, R, cp = qr_oracle.qr(B, t)
    # a repeated column leaves a last diagonal of rounding size or zero; only an exact zero is refused
    assert qs in (0, 3)
    Z = np.array([[2.0, 0.0], [1.0, 0.0]])
    qs, R, cp = qr_oracle.qr(Z, np.ones((1, 2)))
    assert qs == 3 and not R.any() and not cp.any()
    out = qr_oracle.solve(Z, np.ones((1, 2)))
    assert out["status"].tolist() == [3] and out["nodes"].tolist() == [0] and np.isinf(out["dist2"]).all()
    assert not out["z"].any() and not out["v"].any()


def test_point_is_the_sequential_sum():
    B = np.array([[1e16, 1.0, -1e16], [3.0, 4.0, 5.0]])
    assert qr_oracle.point(B, [1, 1, 1]).tolist() == [0.0, 12.0]  # (1e16 + 1) - 1e16 in fp64, in that order


# ---------------------------------------------------------------- premises of the device tests
@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_every_parity_problem_ends_with_status_0_below_the_budget(d, T):
    """Node counts of the transcription over each shape's distinct problems (minimum, median,
    maximum): (2, 1) 4 / 14 / 95; (3, 2) 6 / 8 / 179; (17, 5) 42 / 366 / 923; (33, 64) 262 / 1729 /
    5100; (64, 64) 294 / 1639 / 4318 -- all far below PARITY_NODES = 2^16, so max_nodes is never
    what ends a search there, and none reaches |z| = 2^31."""
    e = qr_oracle.expected(d, T, qr_oracle.DISTINCT[d])
    nodes = e["nodes"]
    print(f"  ({d}, {T}): nodes {nodes.min()} / {int(np.median(nodes))} / {nodes.max()}")
    assert not e["status"].any() and not e["qr_status"].any()
    assert nodes.max() < qr_oracle.PARITY_NODES // 8
    assert np.abs(e["z"]).max() < 1 << 31 and np.isfinite(e["dist2"]).all()
    assert (np.diagonal(e["R"], axis1=1, axis2=2) > 0).all()
