"""CPU-side checks of BKZ reduction (lgs_bkz_reduce): the header declares the function, its
output struct and LGS_BKZ_MAX_BLOCK without adding a counter or timer id; the ctypes mirror
matches the header; both libraries export the symbol; arguments are validated before anything
reaches a device, in the library and in Python; the product library reads no environment; and
the oracle (tests/bkz_oracle.py) confirms the premises the device tests rest on -- it returns a
unimodular transform of the input, an independent enumeration finds nothing left to insert in
what it calls reduced, it degenerates to LLL where no block holds a shorter vector, it finds
the true minimum where the block is the whole basis, and its cases exercise the mechanisms the
kernel has (insertions of several and of large coefficients, several tours, enumerations on both
sides of the forced node slice)."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import bkz_oracle
import lll_oracle
from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")
OUT_FIELDS = ["swaps", "iters", "passes", "tours", "blocks", "insertions", "nodes", "truncated", "status", "gs_norm2"]


def test_header_declares_bkz_reduce():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_bkz_reduce\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_bkz_reduce not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "int64_t n", "int64_t d", "const int64_t *basis", "int64_t block_size",
                    "double delta", "double eta", "int64_t max_tours", "int64_t max_iters", "int64_t enum_nodes",
                    "int64_t *basis_out", "int64_t *U_out", "const lgs_bkz_outputs *out", "uint32_t flags"]
    assert re.search(r"^#define LGS_BKZ_MAX_BLOCK 32\s*$", txt, re.M)
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # no counter id added
    assert "lgs_lll_reduce reuses id 9" in txt and "so does lgs_bkz_reduce" in txt  # lgs_timing_get's comment
    assert "only if truncated == 0" in txt  # what status 0 means


def test_bkz_outputs_struct_matches_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    m = re.search(r"typedef struct lgs_bkz_outputs \{(.*?)\} lgs_bkz_outputs;", txt, re.S)
    assert m, "struct lgs_bkz_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in (" ".join(f.split()) for f in body.split(";") if f.strip()):
        typ, rest = decl.split(" ", 1)
        assert typ == {"status": "int32_t", "gs_norm2": "double"}.get(rest.lstrip("*"), "int64_t"), decl
        names += [p.strip().lstrip("*") for p in rest.split(",")]
        assert all(p.strip().startswith("*") for p in rest.split(",")), decl
    assert names == OUT_FIELDS
    assert [n for n, _ in _capi.BkzOutputs._fields_] == OUT_FIELDS
    assert all(t is ctypes.c_void_p for _, t in _capi.BkzOutputs._fields_)
    assert ctypes.sizeof(_capi.BkzOutputs) == 10 * ctypes.sizeof(ctypes.c_void_p)


def test_both_libraries_export_bkz_reduce():
    from lgs_amd import _capi
    assert "lgs_bkz_reduce" in _capi.EXPORTS and _capi.LGS_BKZ_MAX_BLOCK == 32
    vp, i64, f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        L = _capi.load_library(path)
        fn = L.lgs_bkz_reduce
        assert fn.argtypes == [vp, i64, i64, vp, i64, f64, f64, i64, i64, i64, vp, vp,
                               ctypes.POINTER(_capi.BkzOutputs), ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
        assert L.lgs_version() == 100
    assert callable(_capi.Context.bkz_reduce) and callable(_capi.Context.bkz_reduce_host)


def test_library_validates_before_any_device_call():
    """No device here and no context: the handle is a block of zeros the call must not read or
    hand to the runtime before it has rejected the arguments, each with its own message."""
    from lgs_amd import _capi
    L = _capi.load_library()
    fake = ctypes.create_string_buffer(1 << 16)
    B = np.array([[1, 0], [7, 1]], dtype=np.int64)
    Bo, Uo = np.zeros_like(B), np.zeros_like(B)

    def call(n=1, d=2, basis=B, block_size=2, delta=0.99, eta=0.51, max_tours=4, max_iters=100, enum_nodes=100,
             bo=Bo, uo=Uo, flags=0, ctx=fake):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.lgs_bkz_reduce(ctx, n, d, p(basis), block_size, delta, eta, max_tours, max_iters, enum_nodes,
                                p(bo), p(uo), None, flags)

    big = B.copy()
    big[1, 0] = 1 << 28
    neg = B.copy()
    neg[0, 1] = -(1 << 28)
    for kw, word in ((dict(ctx=None), "null context"), (dict(flags=_capi.LGS_Z64), "flags"),
                     (dict(flags=_capi.LGS_DEVICE_PTRS | _capi.LGS_COORD_MAJOR), "flags"),
                     (dict(d=1), "d = 1"), (dict(d=65), "d = 65"),
                     (dict(block_size=1), "block_size = 1"), (dict(block_size=33), "block_size = 33"),
                     (dict(delta=0.25), "delta"), (dict(delta=1.0), "delta"), (dict(delta=float("nan")), "delta"),
                     (dict(eta=0.5), "eta"), (dict(eta=1.0), "eta"),
                     (dict(max_tours=0), "max_tours"), (dict(max_tours=(1 << 40) + 1), "max_tours"),
                     (dict(max_iters=0), "max_iters"), (dict(max_iters=(1 << 40) + 1), "max_iters"),
                     (dict(enum_nodes=0), "enum_nodes"), (dict(enum_nodes=(1 << 40) + 1), "enum_nodes"),
                     (dict(n=-1), "n < 0"),
                     (dict(basis=None), "required"), (dict(bo=None), "required"), (dict(uo=None), "required"),
                     (dict(basis=big), "2^28"), (dict(basis=neg), "2^28")):
        assert call(**kw) == _capi.LGS_ERR_INVALID, kw
        assert word in L.lgs_last_error().decode(), (kw, L.lgs_last_error())
    assert np.all(Bo == 0) and np.all(Uo == 0)  # nothing written on a refused call
    assert call(n=0) == _capi.LGS_OK  # nothing to do: no device call either


def test_product_library_reads_no_environment_and_the_state_fits():
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()
    assert 'hook("LGS_TEST_BKZ_SLICE")' in src and 'getenv("LGS_TEST_BKZ' not in src
    bkz = open(os.path.join(CSRC, "lgs_bkz.hip")).read()
    assert "getenv" not in bkz and "printf" not in bkz and "assert(" not in bkz
    assert "csrc/lgs_bkz.hip" in open(os.path.join(REPO, "lattice-gaussian-mcmc_amd", "Makefile")).read()
    # one LLL loop: both kernels call the header's, neither holds a copy
    lll = open(os.path.join(CSRC, "lgs_lll.hip")).read()
    loop = open(os.path.join(CSRC, "lgs_lll_loop.h")).read()
    assert loop.count("Lovasz test") == 1 and "Lovasz test" not in lll and "Lovasz test" not in bkz
    assert "lll_loop(" in lll and "lll_loop(" in bkz
    # the LDS budget: the LLL image at d = 64 and what BKZ adds, against the CU's 160 KiB
    kh = open(os.path.join(CSRC, "lgs_kernels.h")).read()
    assert "static_assert(kBkzExtWords * 8 <= 30144" in kh
    c = {k: int(v) for k, v in re.findall(r"constexpr int (kBkz\w+) = (\d+);", kh)}
    ext = c["kBkzHdr"] + 5 * c["kBkzLanes"] + c["kBkzMaxBlock"] * (c["kBkzMaxBlock"] + 1) + c["kBkzMaxBlock"]
    assert c["kBkzMaxBlock"] == 32 and 133696 + 8 * ext <= 160 * 1024 and 8 * ext <= 30144


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after bad arguments")


def _bare_context():
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = 0, 0, None, _NoLibrary()
    return c


def test_context_bkz_reduce_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = _bare_context()
    B = np.zeros((3, 4, 4), dtype=np.int64)
    Bo, Uo = np.zeros_like(B), np.zeros_like(B)
    for bad in (np.zeros((4, 4), dtype=np.int64), np.zeros((3, 4, 5), dtype=np.int64),
                np.zeros((1, 1, 1), dtype=np.int64), np.zeros((1, 65, 65), dtype=np.int64)):
        with pytest.raises(ValueError):
            c.bkz_reduce(bad, np.zeros_like(bad), np.zeros_like(bad), 2)
        with pytest.raises(ValueError):
            c.bkz_reduce_host(bad, 2)
    for kw in (dict(block_size=1), dict(block_size=33), dict(block_size=2.0), dict(block_size=True),
               dict(delta=0.25), dict(delta=1.0), dict(delta="x"), dict(eta=0.5), dict(eta=1),
               dict(max_tours=0), dict(max_tours=(1 << 40) + 1), dict(max_tours=1.5),
               dict(max_iters=0), dict(max_iters=2.5), dict(max_iters=(1 << 40) + 1), dict(max_iters=True),
               dict(enum_nodes=0), dict(enum_nodes=(1 << 40) + 1), dict(enum_nodes=None)):
        full = dict(block_size=2)
        full.update(kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            c.bkz_reduce(B, Bo, Uo, **full)
        with pytest.raises(ValueError, match=next(iter(kw))):
            c.bkz_reduce_host(B, **full)
    for bad_flags in (_capi.LGS_Z64, _capi.LGS_COORD_MAJOR, -1, 1.0, True):
        with pytest.raises(ValueError, match="flags"):
            c.bkz_reduce(B, Bo, Uo, 2, flags=bad_flags)
    with pytest.raises(ValueError, match="expected int64"):
        c.bkz_reduce(B.astype(np.int32), Bo, Uo, 2)
    with pytest.raises(ValueError, match="LGS_DEVICE_PTRS"):
        c.bkz_reduce(B, Bo, Uo, 2, flags=_capi.LGS_DEVICE_PTRS)  # host arrays with the device flag
    with pytest.raises(ValueError, match="U_out"):
        c.bkz_reduce(B, Bo, np.zeros((3, 4, 3), dtype=np.int64), 2)
    with pytest.raises(ValueError, match="required"):
        c.bkz_reduce(B, Bo, None, 2)
    with pytest.raises(ValueError, match="status"):
        c.bkz_reduce(B, Bo, Uo, 2, status=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="truncated"):
        c.bkz_reduce(B, Bo, Uo, 2, truncated=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="tours"):
        c.bkz_reduce(B, Bo, Uo, 2, tours=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="gs_norm2"):
        c.bkz_reduce(B, Bo, Uo, 2, gs_norm2=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="int64"):
        c.bkz_reduce_host(B.astype(np.float64), 2)
    big = B.copy()
    big[2, 1, 3] = -(1 << 28)
    with pytest.raises(ValueError, match="2\\^28"):
        c.bkz_reduce_host(big, 2)


def test_reduction_module_validates_and_keeps_defaults():
    from lgs_amd import reduction
    from lgs_amd.decode import Decoder
    from lgs_amd.lattices import SimpleLattice
    for bad in (np.array([[1.5, 0], [0, 1]]), np.array([[np.nan, 0], [0, 1]]), np.array([["a", "b"], ["c", "d"]]),
                np.array([[float(1 << 28), 0], [0, 1]]), np.zeros((2, 3)), np.zeros(4), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError):
            reduction.bkz_reduce(bad, 2)
    sig = inspect.signature(reduction.bkz_reduce).parameters
    assert list(sig) == ["basis", "block_size", "delta", "eta", "max_tours", "enum_nodes", "max_iters", "rows", "device"]
    assert [sig[k].default for k in list(sig)[2:]] == [0.99, 0.51, 1024, 1 << 30, 1 << 40, True, 0]
    sig = inspect.signature(reduction.LatticeReduction.bkz_reduce).parameters
    assert list(sig) == ["self", "basis", "block_size", "strategy", "progressive"]
    assert (sig["strategy"].default, sig["progressive"].default) == ("default", False)
    lr = reduction.LatticeReduction.__new__(reduction.LatticeReduction)
    for strategy in ("bkz2", "custom", None):  # refused before anything is computed
        with pytest.raises(ValueError, match="strategy"):
            lr.bkz_reduce(np.eye(3), 2, strategy=strategy)
    # the reference's schedule (src/lattices/reduction.py:302-312)
    prog = reduction.LatticeReduction._progressive_block_sizes
    assert prog(32, 30) == [20, 30] and prog(64, 45) == [20, 30, 40, 45] and prog(12, 12) == [12]
    assert prog(64, 10) == [10] and prog(16, 30) == [16, 26, 30]
    assert inspect.signature(SimpleLattice.bkz).parameters["delta"].default == 0.99
    # reduce=True stays what it was
    for fn in (Decoder.__init__, SimpleLattice.first_minimum, SimpleLattice.decode_cvp, SimpleLattice.gaussian_mass):
        assert inspect.signature(fn).parameters["reduce"].default is False
    assert inspect.signature(SimpleLattice.lll).parameters["delta"].default == 0.99


# ---------------------------------------------------------------- premises, on the oracle
@pytest.mark.parametrize("name,beta,delta", bkz_oracle.CASES)
def test_oracle_returns_a_unimodular_transform_and_a_reduced_basis(name, beta, delta):
    """Premises 1 and 2: B U = B' exactly and |det U| = 1 (Bareiss); what ends with status 0 holds
    no insertion for a tour of the plain enumeration."""
    B = bkz_oracle.basis(name).tolist()
    r = bkz_oracle.reduced(name, beta, delta)
    print(f"  {name} beta {beta} delta {delta}: status {r['status']}, tours {r['tours']}, blocks {r['blocks']}, "
          f"insertions {r['insertions']}, nodes {r['nodes']}, iters {r['iters']}")
    assert r["status"] == (4 if name == "lll64" else 0) and r["truncated"] == 0
    assert r["blocks"] == r["tours"] * (len(B) - 1) and r["passes"] >= r["iters"] >= r["swaps"]
    assert lll_oracle.matmul(B, r["U_out"]) == r["basis_out"]
    assert abs(lll_oracle.det_bareiss(r["U_out"])) == 1
    assert all(x > 0.0 for x in r["gs_norm2"])
    if r["status"] == 0:
        assert bkz_oracle.plain_tour_insertions(r["basis_out"], beta, delta) == 0


def test_no_insertion_is_lll():
    """Premise 3: qary8 with beta = 4 inserts nothing, and every LLL output is lll_oracle.lll's."""
    r, l = bkz_oracle.reduced("qary8", 4), lll_oracle.reduced("qary8", 0.99)
    assert (r["insertions"], r["tours"], r["blocks"], r["status"]) == (0, 1, 7, 0)
    for f in ("basis_out", "U_out", "swaps", "iters", "passes", "gs_norm2"):
        assert r[f] == l[f], f


def test_full_block_finds_the_first_minimum():
    """Premise 4: with beta = d the first vector is a shortest vector up to delta; on qary12 it is
    the shortest outright.  Brute force over [-1, 1]^12 on the LLL-reduced basis of the same
    lattice, where the box argument of test_gpu_lll.py holds: z = B'^-1 v gives |z_i| <= |row i
    of B'^-1| |v|, below 2 for every i when |v| is at most the shortest reduced vector."""
    Bl = np.array(lll_oracle.reduced("qary12", 0.99)["basis_out"], dtype=np.int64)
    shortest = min(int(np.sum(Bl[:, i] ** 2)) for i in range(12))
    assert np.all(np.sqrt(shortest) * np.linalg.norm(np.linalg.inv(Bl.astype(np.float64)), axis=1) < 1.99)
    Z = np.array(list(itertools.product((-1, 0, 1), repeat=12)), dtype=np.int64)
    n2 = np.sum((Z @ Bl.T) ** 2, axis=1)
    best = int(n2[n2 > 0].min())
    Bp = np.array(bkz_oracle.reduced("qary12", 12)["basis_out"], dtype=np.int64)
    assert int(np.sum(Bp[:, 0] ** 2)) == best == 125 < shortest == 127


def test_cases_exercise_every_mechanism():
    """Premise 5."""
    logs = {(n, b, dl): bkz_oracle.reduced(n, b, dl)["log"] for n, b, dl in bkz_oracle.CASES}
    inserted = [g[4] for log in logs.values() for g in log if g[4] is not None]
    assert any(sum(1 for v in x if v) >= 2 for x in inserted)  # the Euclid loop runs
    assert any(max(abs(v) for v in x) >= 2 for x in inserted)  # with a quotient other than 0 and +-1
    assert max(abs(v) for g in logs[("qary40", 16, 0.99)] if g[4] for v in g[4]) == 3
    assert all(x[max(i for i, v in enumerate(x) if v)] > 0 for x in inserted)  # highest coefficient positive
    assert any(bkz_oracle.reduced(n, b, dl)["tours"] >= 3 for n, b, dl in bkz_oracle.CASES)
    assert any(g[1] - g[0] + 1 == 32 for g in logs[("qary32", 32, 0.99)])  # a block of 32 levels
    assert any(g[0] < 32 <= g[1] for g in logs[("qary40", 16, 0.99)])  # blocks that straddle index 32
    for name, beta in bkz_oracle.SLICE_CASES:  # enumerations on both sides of the forced node slice
        per_block = [g[2] for g in logs[(name, beta, 0.99)]]
        assert min(per_block) < bkz_oracle.BKZ_SLICE < max(per_block), (name, per_block)
        assert bkz_oracle.reduced(name, beta)["insertions"] >= 3  # and LLL re-entries to suspend
    o = bkz_oracle.reduced("lll64", 12, 0.75)
    assert (o["status"], o["tours"], o["insertions"]) == (4, 2, 91)


def test_oracle_stops_and_guards():
    B = lll_oracle.bases()["qary32"].tolist()
    full = bkz_oracle.reduced("qary32", 12)
    cut = bkz_oracle.reduced("qary32", 12, enum_nodes=64)
    assert cut["status"] == 0 and 0 < cut["truncated"] < cut["blocks"] and cut["nodes"] < full["nodes"]
    assert all(g[2] <= 64 for g in cut["log"]) and all(g[2] == 64 for g in cut["log"] if g[3])
    two = bkz_oracle.reduced("qary32", 12, max_tours=2)
    assert (two["status"], two["tours"], two["blocks"]) == (4, 2, 62) and 0 < two["insertions"] < full["insertions"]
    first_lll = lll_oracle.reduced("qary32", 0.99)["iters"]
    it = bkz_oracle.reduced("qary32", 12, max_iters=first_lll + 5)
    assert (it["status"], it["iters"], it["where"]) == (1, first_lll + 5, "lll") and it["insertions"] >= 1
    for r in (cut, two, it):
        assert lll_oracle.matmul(B, r["U_out"]) == r["basis_out"]
    for singular in ([[1, 1], [2, 2]], [[0, 1], [0, 5]], [[1, 2, 3], [4, 5, 6], [7, 8, 9]]):
        r = bkz_oracle.bkz(singular, 2)
        assert r["status"] == 3 and r["blocks"] == 0, singular
        assert lll_oracle.matmul(singular, r["U_out"]) == r["basis_out"]
    # the INSERT guard: the reduced qary12 scaled until a step of Euclid would pass 2^28
    G = bkz_oracle.guard_basis()
    r = bkz_oracle.bkz(G, 12)
    assert (r["status"], r["where"], r["steps"], r["insertions"], r["blocks"]) == (2, "insert", 1, 0, 1)
    assert r["basis_out"] != G and lll_oracle.matmul(G, r["U_out"]) == r["basis_out"]
    assert abs(lll_oracle.det_bareiss(r["U_out"])) == 1


# ---------------------------------------------------------------- premises of the dense and the scheduling cases
@pytest.mark.parametrize("name,beta,max_tours", bkz_oracle.DENSE_CASES)
def test_dense_cases_return_a_unimodular_transform(name, beta, max_tours):
    B = bkz_oracle.basis(name).tolist()
    r = bkz_oracle.reduced(name, beta, max_tours=max_tours)
    print(f"  {name} beta {beta}: status {r['status']}, tours {r['tours']}, blocks {r['blocks']}, insertions "
          f"{r['insertions']}, nodes {r['nodes']}, iters {r['iters']}")
    assert r["status"] == (4 if name == "dense63" else 0) and r["truncated"] == 0
    assert r["blocks"] == r["tours"] * (len(B) - 1) and r["passes"] >= r["iters"] >= r["swaps"]
    assert lll_oracle.matmul(B, r["U_out"]) == r["basis_out"]
    if len(B) <= 33:
        assert abs(lll_oracle.det_bareiss(r["U_out"])) == 1
    if name in ("dense17", "dense33", "dense63"):
        assert r["insertions"] > 0
    if name == "dense17":
        assert (r["tours"], r["blocks"], r["insertions"], r["nodes"]) == (6, 96, 23, 2243)
    if name == "dense33":
        assert (r["tours"], r["insertions"], r["nodes"]) == (7, 50, 16064)
    if r["status"] == 0 and len(B) <= 17:
        assert bkz_oracle.plain_tour_insertions(r["basis_out"], beta) == 0
    if name.startswith("tie"):  # the LLL of the tie, which half-away rounding would change
        assert r["basis_out"] == lll_oracle.reduced(name, 0.99)["basis_out"] and r["insertions"] == 0


def test_schedule_counts_launches_and_suspensions():
    """bkz_oracle.schedule on hand-made traces, slices of 16 iterations and 64 nodes."""
    sch = lambda *trace: bkz_oracle.schedule({"trace": list(trace)}, 16, 64)  # noqa: E731
    assert sch() == (1, 0, 0)  # stopped by chol(0): the launch that writes the outputs
    assert sch(("lll", 16), ("enum", 64)) == (1, 0, 0)  # both budgets spent on the last steps
    assert sch(("lll", 17)) == (2, 1, 0) and sch(("lll", 16), ("enum", 65)) == (2, 0, 1)
    assert sch(("lll", 10), ("enum", 30), ("lll", 5), ("enum", 30), ("lll", 1), ("enum", 5)) == (2, 0, 1)
    assert sch(("lll", 10), ("enum", 30), ("lll", 7), ("enum", 30)) == (2, 1, 0)
    assert sch(("lll", 40), ("enum", 200)) == (3 + 3, 2, 3)
    # the trace of a real run accounts for every iteration and node
    r = bkz_oracle.reduced("dense17", 6)
    assert sum(n for k, n in r["trace"] if k == "lll") == r["iters"]
    assert sum(n for k, n in r["trace"] if k == "enum") == r["nodes"]
    assert [n for k, n in r["trace"] if k == "enum"] == [g[2] for g in r["log"]]
    assert sum(1 for k, _ in r["trace"] if k == "lll") == 1 + r["insertions"]


def test_mixed_batch_is_suspended_in_both_phases():
    """bkz_oracle.mixed_batch() at beta = 6 under 16 iterations and 64 nodes per launch: the
    entries need different numbers of launches, at least one is suspended inside an LLL and at
    least one inside an enumeration, and at MIXED_MAX_TOURS status 4, 0 and 3 meet in one call.
    (No block of these bases takes more than 64 nodes -- nor did one of 360 other dense bases of
    d = 17 at beta = 6 -- so an enumeration is suspended where a launch's 64 nodes run out in a
    later block of a run of blocks without insertion: schedule() follows the kernel's budgets.)"""
    B, R = bkz_oracle.mixed_batch(), bkz_oracle.mixed_reduced()
    n = len(B)
    assert B.shape == (n, 17, 17) and n == len(bkz_oracle.MIXED_DENSE) + 4
    assert len({amp for _, amp in bkz_oracle.MIXED_DENSE}) == 3
    sched = [bkz_oracle.schedule(r) for r in R]
    print(f"  (launches, suspended in LLL, suspended in ENUM) per entry: {sched}")
    assert len({s[0] for s in sched}) >= 5
    assert sum(1 for s in sched if s[1] > 0) >= 3 and sum(1 for s in sched if s[2] > 0) >= 3
    for r, s in zip(R, sched):  # the bounds the device test puts on the launch count hold entry by entry
        li, ln = -(-r["iters"] // bkz_oracle.LLL_SLICE), -(-r["nodes"] // bkz_oracle.BKZ_SLICE)
        assert max(1, li, ln) <= s[0] <= 1 + li + ln
    ident = [k for k in range(n) if np.array_equal(B[k], np.eye(17, dtype=np.int64))]
    assert len(ident) == 1 and (R[ident[0]]["insertions"], R[ident[0]]["tours"], R[ident[0]]["swaps"]) == (0, 1, 0)
    red = [k for k in range(n) if B[k].tolist() == R[0]["basis_out"]]
    assert len(red) == 1 and R[0]["insertions"] > 0
    assert (R[red[0]]["insertions"], R[red[0]]["tours"], R[red[0]]["status"], R[red[0]]["swaps"]) == (0, 1, 0, 0)
    sing = [k for k in range(n) if R[k]["status"] == 3]
    assert len(sing) == 1 and 0 < sing[0] < n - 1 and lll_oracle.det_bareiss(B[sing[0]].tolist()) == 0
    assert all(r["status"] == 0 for k, r in enumerate(R) if k not in sing)
    same = [(i, j) for i in range(n) for j in range(i + 1, n) if np.array_equal(B[i], B[j])]
    assert len(same) == 1 and R[same[0][0]] == R[same[0][1]]
    cut = bkz_oracle.mixed_reduced(bkz_oracle.MIXED_MAX_TOURS)
    st = [r["status"] for r in cut]
    assert st.count(4) >= 2 and st.count(0) >= 2 and st.count(3) == 1
    assert all(r["tours"] == bkz_oracle.MIXED_MAX_TOURS for r in cut if r["status"] == 4)


def test_chunk_batch_under_bkz():
    """lll_oracle.chunk_batch() at beta = 2: the singular entries at the chunk boundary stop with
    status 3 before any tour, every other entry ends with status 0, and the LLL of each is
    lll_oracle's (no block of two holds a shorter vector after LLL at 0.99 here)."""
    R, L = bkz_oracle.chunk_reduced(), lll_oracle.chunk_reduced()
    assert sorted(R) == sorted(L) and (R[-1]["status"], R[-2]["status"]) == (3, 3)
    assert R[-1]["tours"] == R[-2]["tours"] == 0
    for v in range(lll_oracle.CHUNK_DISTINCT):
        assert R[v]["status"] == 0 and R[v]["tours"] >= 1 and R[v]["blocks"] == 2 * R[v]["tours"]
        if R[v]["insertions"] == 0:
            assert all(R[v][f] == L[v][f] for f in ("basis_out", "U_out", "iters", "swaps", "passes", "gs_norm2"))
    for part in (lll_oracle.chunk_batch()[1][:1024], lll_oracle.chunk_batch()[1][1024:]):
        assert len({bkz_oracle.schedule(R[v], 2, 1 << 16)[0] for v in part}) >= 2
