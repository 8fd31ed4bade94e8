"""CPU-side checks of exact closest-vector decoding (lgs_closest_vector): the header declares
the function, its output struct and LGS_CVP_MAX_D; the ctypes mirror matches the header; the
Python entry points validate their arguments before anything reaches a device; and the
oracle (tests/cvp_oracle.py) confirms the premises the device tests rest on -- it agrees with
brute force where brute force is possible, and the node counts of the test targets lie where
the device tests' budgets and the launch slice assume them."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import cvp_oracle
from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
KERNELS_H = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc", "lgs_kernels.h")
PARITY_BUDGET = 1 << 20  # max_nodes of tests/test_gpu_cvp.py's parity and slice tests
DEEP_BUDGET = 1 << 23    # of its gauss37 test
SMALL_BUDGET = 1000      # of its budget test


def test_header_declares_closest_vector():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_closest_vector\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_closest_vector not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "int64_t n", "const double *targets", "const double *radius2",
                    "int64_t max_nodes", "void *z_out", "double *v_out", "double *cprime_out",
                    "const lgs_cvp_outputs *out", "uint32_t flags"]
    assert re.search(r"^#define LGS_CVP_MAX_D 64\s*$", txt, re.M)
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # no counter id added
    assert "9 = lgs_closest_vector's enumeration launches" in txt  # lgs_timing_get's id


def test_library_exports_closest_vector():
    from lgs_amd import _capi
    assert "lgs_closest_vector" in _capi.EXPORTS
    assert _capi.LGS_CVP_MAX_D == 64 and _capi.KERNEL_CVP_ENUM == 9
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        L = _capi.load_library(path)
        fn = L.lgs_closest_vector
        assert fn.argtypes == [vp, i64, vp, vp, i64, vp, vp, vp, ctypes.POINTER(_capi.CvpOutputs), ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
        assert L.lgs_version() == 100
    assert callable(_capi.Context.closest_vector) and callable(_capi.Context.closest_vector_host)


def test_cvp_outputs_struct_matches_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    m = re.search(r"typedef struct lgs_cvp_outputs \{(.*?)\} lgs_cvp_outputs;", txt, re.S)
    assert m, "struct lgs_cvp_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["double *dist2", "int64_t *nodes", "int32_t *status"]
    assert [n for n, _ in _capi.CvpOutputs._fields_] == ["dist2", "nodes", "status"]
    assert all(t is ctypes.c_void_p for _, t in _capi.CvpOutputs._fields_)
    assert ctypes.sizeof(_capi.CvpOutputs) == 3 * ctypes.sizeof(ctypes.c_void_p)


def test_product_library_reads_no_environment():
    """The slice and slot switches exist in the hooks build only (hook() is a constant
    nullptr in the product library)."""
    src = open(os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc", "lgs_capi.hip")).read()
    assert 'hook("LGS_TEST_CVP_SLICE")' in src and 'getenv("LGS_TEST_CVP' not in src
    cvp = open(os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc", "lgs_cvp.hip")).read()
    assert "getenv" not in cvp and "printf" not in cvp and "assert(" not in cvp


class _NoLibrary:
    """A library handle that fails the test when anything is called on it."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after bad arguments")


def _bare_context(d):
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = d, 0, None, _NoLibrary()
    return c


def test_context_closest_vector_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = _bare_context(4)
    T = np.zeros((3, 4))
    for bad in (np.zeros((3, 5)), np.zeros(4), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            c.closest_vector(bad, 100)
        with pytest.raises(ValueError):
            c.closest_vector_host(bad, 100)
    with pytest.raises(ValueError):  # (3, 4) is not (d, n) = (4, n)
        c.closest_vector(T, 100, flags=_capi.LGS_COORD_MAJOR)
    for bad_nodes in (0, -1, (1 << 40) + 1, 2.5, None, True, "7"):
        with pytest.raises(ValueError, match="max_nodes"):
            c.closest_vector(T, bad_nodes)
        with pytest.raises(ValueError, match="max_nodes"):
            c.closest_vector_host(T, bad_nodes)
    for bad_flags in (_capi.LGS_EXACT_ORDER, _capi.LGS_WANG_LING, 0x1000, -1, 1.0):
        with pytest.raises(ValueError, match="flags"):
            c.closest_vector(T, 100, flags=bad_flags)
    with pytest.raises(ValueError, match="flags"):
        c.closest_vector_host(T, 100, flags=_capi.LGS_EXACT_ORDER)
    for f in (_capi.LGS_DEVICE_PTRS, _capi.LGS_COORD_MAJOR):
        with pytest.raises(ValueError):
            c.closest_vector_host(T, 100, flags=f)
    with pytest.raises(ValueError, match="expected int64"):
        c.closest_vector(T, 100, z_out=np.zeros((3, 4), dtype=np.int32), flags=_capi.LGS_Z64)
    with pytest.raises(ValueError, match="status"):
        c.closest_vector(T, 100, status=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="nodes"):
        c.closest_vector(T, 100, nodes=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="radius2"):
        c.closest_vector(T, 100, radius2=np.zeros(2))
    for bad_r in (np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]), np.zeros(2)):
        with pytest.raises(ValueError, match="radius2"):
            c.closest_vector_host(T, 100, radius2=bad_r)
    big = _bare_context(65)
    with pytest.raises(ValueError, match="d <= 64"):
        big.closest_vector(np.zeros((1, 65)), 100)
    with pytest.raises(ValueError, match="d <= 64"):
        big.closest_vector_host(np.zeros((1, 65)), 100)


class _StubContext:
    """Stands in for _capi.Context behind a Decoder: records what would reach the device."""

    def __init__(self, d, status=0):
        self.d, self.status, self.calls = d, status, []

    def closest_vector_host(self, targets, max_nodes, radius2=None, **kw):
        self.calls.append((targets.shape, max_nodes, None if radius2 is None else radius2.copy(), kw))
        n = targets.shape[0]
        return {"z": np.ones((n, self.d), dtype=np.int64), "v": np.full((n, self.d), 2.0), "cprime": None,
                "dist2": np.zeros(n), "nodes": np.full(n, max_nodes, dtype=np.int64),
                "status": np.full(n, self.status, dtype=np.int32)}


def _stub_decoder(d, status=0):
    from lgs_amd.decode import Decoder
    dec = object.__new__(Decoder)
    dec.dimension, dec.ctx = d, _StubContext(d, status)
    return dec


def test_decoder_closest_vector_validates_and_shapes():
    dec = _stub_decoder(3)
    for bad in (np.zeros(4), np.zeros((5, 2)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            dec.closest_vector(bad)
    assert dec.ctx.calls == []
    assert dec.closest_vector(np.zeros(3)).shape == (3,)
    assert dec.ctx.calls[-1][:2] == ((1, 3), 1 << 24) and dec.ctx.calls[-1][3] == {"want_z": False, "want_v": True}
    z, info = dec.closest_vector(np.zeros((5, 3)), max_nodes=77, radius2=2.5, coefficients=True, info=True)
    assert z.shape == (5, 3) and z.dtype == np.int64
    assert sorted(info) == ["dist2", "nodes", "status"] and info["nodes"].shape == (5,)
    assert np.array_equal(dec.ctx.calls[-1][2], np.full(5, 2.5)) and dec.ctx.calls[-1][1] == 77
    v, info = dec.closest_vector(np.zeros(3), info=True)
    assert v.shape == (3,) and info["status"] == 0
    with pytest.raises(ValueError, match="d <= 64"):
        _stub_decoder(65).closest_vector(np.zeros(65))


def test_decode_cvp_exact_never_returns_an_unproven_point():
    from lgs_amd.lattices import SimpleLattice
    lat = SimpleLattice(np.eye(3))
    lat._dec = _stub_decoder(3, status=0)
    assert lat.decode_cvp(np.zeros((2, 3)), "exact").shape == (2, 3)
    assert lat.decode_cvp(np.zeros(3), method="exact").shape == (3,)
    lat._dec = _stub_decoder(3, status=2)  # proven: nothing within the radius
    assert lat.decode_cvp(np.zeros(3), "exact").shape == (3,)
    lat._dec = _stub_decoder(3, status=1)
    with pytest.raises(RuntimeError, match="500 nodes"):
        lat.decode_cvp(np.zeros((2, 3)), "exact", max_nodes=500)
    with pytest.raises(ValueError):
        lat.decode_cvp(np.zeros(3), "nearest")


# ---------------------------------------------------------------- premises, on the oracle
@pytest.mark.parametrize("name", ["d2", "d3"])
def test_oracle_equals_brute_force(name):
    """64 targets: the search returns the argmin of refdist over a 13^d box around the
    rounded solution, with the same D.  No target has two minimisers in the box, so the
    tie rule is not involved."""
    s = cvp_oracle.setup(name)
    for k in range(64):
        cp = s["T"][k] @ s["Q"]
        z, D, nodes, status = cvp_oracle.se(s["R"], cp)
        centre = np.rint(np.linalg.solve(s["B"], s["T"][k])).astype(np.int64)
        zb, Db, ties = cvp_oracle.brute_force(s["R"], cp, centre)
        assert status == 0 and ties == 1
        assert np.array_equal(z, zb) and D == Db, (name, k)
        assert D == cvp_oracle.refdist(s["R"], cp, z)


def test_oracle_radius_and_budget_semantics():
    s = cvp_oracle.setup("int12")
    cp = s["T"][0] @ s["Q"]
    z, D, nodes, status = cvp_oracle.se(s["R"], cp)
    assert status == 0
    # strict radius: the closest point is excluded by radius2 = D, found just above it
    z2, D2, n2, st2 = cvp_oracle.se(s["R"], cp, radius2=D)
    assert st2 == 2 and D2 == math.inf and not z2.any() and n2 <= nodes
    z3, D3, n3, st3 = cvp_oracle.se(s["R"], cp, radius2=np.nextafter(D, math.inf))
    assert st3 == 0 and D3 == D and np.array_equal(z3, z) and n3 <= nodes
    # budget: exactly max_nodes nodes, the best so far; one node cannot reach level 0
    z4, D4, n4, st4 = cvp_oracle.se(s["R"], cp, max_nodes=nodes - 1)
    assert st4 == 1 and n4 == nodes - 1 and D4 >= D
    z5, D5, n5, st5 = cvp_oracle.se(s["R"], cp, max_nodes=1)
    assert st5 == 1 and n5 == 1 and D5 == math.inf and not z5.any()
    assert cvp_oracle.se(s["R"], cp, max_nodes=nodes)[3] == 0  # the last node ends the search


def _node_counts(name, count, max_nodes=1 << 40):
    s = cvp_oracle.setup(name)
    return [cvp_oracle.se(s["R"], s["T"][k] @ s["Q"], max_nodes=max_nodes)[2:] for k in range(count)]


def test_node_counts_fit_the_device_tests_budgets():
    """With c' = T Q formed on the host (the device's c' differs in the last bits, which
    moves single counts, not their scale): int12 median 107, maximum 452 over 64 targets;
    gauss16 maximum 930, gauss20 10 160, gauss24 median 53 957, maximum 84 901 over 16."""
    for name, count, lo, hi in (("int12", 130, 65, 1 << 12), ("gauss16", 16, 65, 1 << 12),
                                ("gauss20", 16, 1 << 10, 1 << 15), ("gauss24", 16, 1 << 14, 1 << 18)):
        r = _node_counts(name, count)
        nodes = [n for n, _ in r]
        print(f"  {name}: {count} targets, nodes median {int(np.median(nodes))}, max {max(nodes)}")
        assert all(st == 0 for _, st in r)
        assert lo < max(nodes) < hi < PARITY_BUDGET
    # the slice test runs int12 at 64 nodes per launch: targets on both sides of it
    nodes = [n for n, _ in _node_counts("int12", 130)]
    assert min(nodes) <= 64 < max(nodes) and sum(n > 64 for n in nodes) >= 32


def test_gauss24_node_counts_straddle_the_default_slice():
    """Some lanes of the 16-target launch stop within the first launch of kCvpSlice nodes and
    others are suspended and resumed."""
    txt = open(KERNELS_H).read()
    m = re.search(r"constexpr int64_t kCvpSlice = 1 << (\d+);", txt)
    assert m, "kCvpSlice not found in lgs_kernels.h"
    slice_nodes = 1 << int(m.group(1))
    assert slice_nodes == 1 << 16
    nodes = [n for n, _ in _node_counts("gauss24", 16)]
    below, above = sum(n <= slice_nodes for n in nodes), sum(n > slice_nodes for n in nodes)
    print(f"  gauss24: {below} targets within one slice, {above} beyond")
    assert below >= 2 and above >= 2


def test_gauss37_targets_exceed_the_small_budget():
    """The budget test's 8 targets all need more than 1000 nodes (each 3.1-3.4 million, which
    the device test proves by finishing them within 2^23; the first is checked here)."""
    r = _node_counts("gauss37", 8, max_nodes=SMALL_BUDGET + 1)
    assert all(n == SMALL_BUDGET + 1 and st == 1 for n, st in r)
    n0, st0 = _node_counts("gauss37", 1)[0]
    print(f"  gauss37 target 0: {n0} nodes")
    assert st0 == 0 and (1 << 21) < n0 < DEEP_BUDGET
