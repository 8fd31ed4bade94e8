"""CPU-side checks of the ball's points and the exact sampler (lgs_ball_points,
lgs_exact_table, lgs_exact_sample): the oracle (tests/ball_oracle.py) equals brute force where
brute force is possible and mass_oracle everywhere; the blocked running sum equals its written
definition; the header declares the entry points and structs, the ctypes mirrors match, both
libraries export the symbols and the Python entry points validate their arguments before
anything reaches a device; ExactSampler, Decoder.ball_points and first_minimum run on stubs."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

import ball_oracle
import cvp_oracle
import mass_oracle
from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")
NATS = 12.0
CASES = [("d2", 0.8, 8), ("d3", 1.1, 8), ("int12", 12.0, 3), ("gauss16", 9.0, 1)]


def _ball(s, k, sigma, nats=NATS):
    cp = s["T"][k] @ s["Q"]
    _, D, _, st = cvp_oracle.se(s["R"], cp)
    assert st == 0
    return cp, D, D + 2.0 * sigma * sigma * nats


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name,sigma", [("d2", 0.8), ("d3", 1.1)])
def test_oracle_list_equals_box_enumeration(name, sigma):
    s = ball_oracle.setup(name)
    for k in range(8):
        cp, Dmin, A = _ball(s, k, sigma)
        z, D, nodes, st = ball_oracle.points(s["R"], cp, A)
        centre = np.rint(np.linalg.solve(s["B"], s["T"][k])).astype(np.int64)
        box = {}
        for off in itertools.product(range(-7, 8), repeat=s["d"]):
            zz = tuple(int(c) + o for c, o in zip(centre, off))
            Dz = cvp_oracle.refdist(s["R"], cp, zz)
            if Dz < A:
                box[zz] = Dz
        got = {tuple(int(v) for v in row): float(x) for row, x in zip(z, D)}
        assert st == 0 and len(got) == len(z) and got == box and len(box) > 1
        assert D.min() == Dmin == mass_oracle.enum(s["R"], cp, sigma, A, Dmin)["dist2_min"]


@pytest.mark.parametrize("name,sigma,n", CASES)
def test_oracle_counts_equal_mass_oracle(name, sigma, n):
    s = ball_oracle.setup(name)
    for k in range(n):
        cp, Dmin, A = _ball(s, k, sigma)
        z, D, nodes, st = ball_oracle.points(s["R"], cp, A)
        m = mass_oracle.enum(s["R"], cp, sigma, A, Dmin)
        assert (len(D), nodes, st) == (m["points"], m["nodes"], m["status"]) and st == 0
        assert all(cvp_oracle.refdist(s["R"], cp, row) == x for row, x in zip(z[:50], D[:50]))
    cut = ball_oracle.points(s["R"], cp, A, max_nodes=nodes - 1)
    assert cut[3] == 1 and cut[2] == nodes - 1


@pytest.mark.parametrize("N", [1, 16, 255, 256, 257, 300, 512, 777])
def test_blocked_sum_is_its_definition(N):
    w = np.random.default_rng(N).random(N) * np.exp(-np.arange(N) / 50.0)
    S = ball_oracle.blocked_cumsum(w)
    assert np.array_equal(S, ball_oracle.blocked_cumsum_np(w))
    assert (np.diff(S) >= 0).all() and S[0] == w[0]
    assert S[-1] == pytest.approx(math.fsum(w), rel=N * 2.0 ** -52)
    if N > 256:  # the first row of the second block: P_1 + c, P_1 the sequential sum of the first block
        p1 = 0.0
        for x in w[:256]:
            p1 = p1 + float(x)
        assert S[255] == p1 and S[256] == p1 + w[256]
    assert ball_oracle.draw(S, 0.0) == 0 and ball_oracle.draw(S, 1.0) == N - 1
    assert ball_oracle.draw(S, float(S[0] / S[-1]) * 0.5) == 0


# ---------------------------------------------------------------- header and bindings
DECLS = {
    "lgs_ball_points": ["lgs_ctx *ctx", "int64_t n", "const double *targets", "const double *radius2",
                        "int64_t max_nodes", "int64_t capacity", "void *z_out", "double *dist2_out",
                        "double *cprime_out", "const lgs_ball_outputs *out", "uint32_t flags"],
    "lgs_exact_table": ["lgs_ctx *ctx", "int64_t n", "const double *targets", "double sigma", "const double *radius2",
                        "const double *shift", "int64_t max_nodes", "int64_t max_points",
                        "const lgs_exact_table_outputs *out", "uint32_t flags"],
    "lgs_exact_sample": ["lgs_ctx *ctx", "uint64_t seed", "uint64_t first_sample", "int64_t n_draws", "void *z_out",
                         "double *v_out", "const lgs_exact_sample_outputs *out", "uint32_t flags"],
}
STRUCTS = {
    "lgs_ball_outputs": ("BallOutputs", ["int64_t *offsets", "int64_t *nodes", "int32_t *status"]),
    "lgs_exact_table_outputs": ("ExactTableOutputs", ["int64_t *offsets", "int64_t *nodes", "int32_t *status",
                                                      "double *mass", "double *weights", "double *cum"]),
    "lgs_exact_sample_outputs": ("ExactSampleOutputs", ["int64_t *index", "double *dist2"]),
}


def test_header_declares_the_entry_points():
    txt = open(HEADER).read()
    for fn, want in DECLS.items():
        m = re.search(r"^int " + fn + r"\s*\((.*?)\);", txt, re.M | re.S)
        assert m, f"{fn} not declared in lgs.h"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # no counter id added


def test_structs_match_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    for name, (cls, want) in STRUCTS.items():
        m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", txt, re.S)
        assert m, f"struct {name} not in lgs.h"
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
        assert fields == want
        S = getattr(_capi, cls)
        assert [n for n, _ in S._fields_] == [f.split("*")[1] for f in want]
        assert all(t is ctypes.c_void_p for _, t in S._fields_)
        assert ctypes.sizeof(S) == len(want) * ctypes.sizeof(ctypes.c_void_p)


def test_libraries_export_the_symbols():
    from lgs_amd import _capi
    vp, i64, u64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32
    want = {"lgs_ball_points": [vp, i64, vp, vp, i64, i64, vp, vp, vp, ctypes.POINTER(_capi.BallOutputs), u32],
            "lgs_exact_table": [vp, i64, vp, ctypes.c_double, vp, vp, i64, i64,
                                ctypes.POINTER(_capi.ExactTableOutputs), u32],
            "lgs_exact_sample": [vp, u64, u64, i64, vp, vp, ctypes.POINTER(_capi.ExactSampleOutputs), u32]}
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        L = _capi.load_library(path)
        for fn, args in want.items():
            assert fn in _capi.EXPORTS
            f = getattr(L, fn)
            assert f.argtypes == args and f.restype is ctypes.c_int
    for m in ("ball_points", "ball_points_host", "exact_table", "exact_table_host", "exact_sample",
              "exact_sample_host"):
        assert callable(getattr(_capi.Context, m))


def test_product_library_reads_no_environment():
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()
    body = src[src.index("EnumTuning enum_tuning("):]
    body = body[:body.index("\n}\n")]
    for h in ("LGS_TEST_MASS_SPLIT", "LGS_TEST_CVP_SLICE", "LGS_TEST_CVP_SLOTS"):
        assert f'hook("{h}")' in body
        assert src.count(h) == 1  # (the tuning is read in one place, by every enumeration)
    assert "getenv(" not in body
    txt = open(os.path.join(CSRC, "lgs_exact.hip")).read()
    assert "getenv" not in txt and "printf" not in txt and "assert(" not in txt and "asm" not in txt


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after bad arguments")


def _bare_context(d):
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = d, 0, None, _NoLibrary()
    return c


def test_context_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = _bare_context(4)
    T, r2 = np.zeros((3, 4)), np.ones(3)
    for bad in (np.zeros((3, 5)), np.zeros(4), np.zeros((2, 3, 4))):
        for call in (lambda t: c.ball_points(t, r2), lambda t: c.ball_points_host(t, r2),
                     lambda t: c.exact_table(t, 1.0, r2), lambda t: c.exact_table_host(t, 1.0, r2)):
            with pytest.raises(ValueError):
                call(bad)
    for bad_nodes in (0, -1, (1 << 40) + 1, 2.5, None, True):
        with pytest.raises(ValueError, match="max_nodes"):
            c.ball_points(T, r2, max_nodes=bad_nodes)
        with pytest.raises(ValueError, match="max_nodes"):
            c.exact_table_host(T, 1.0, r2, max_nodes=bad_nodes)
    for bad_cap in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="capacity"):
            c.ball_points(T, r2, capacity=bad_cap)
        with pytest.raises(ValueError, match="max_points"):
            c.exact_table(T, 1.0, r2, max_points=bad_cap)
    for bad_flags in (_capi.LGS_EXACT_ORDER, _capi.LGS_WANG_LING, 0x1000, -1, 1.0):
        with pytest.raises(ValueError, match="flags"):
            c.ball_points(T, r2, flags=bad_flags)
        with pytest.raises(ValueError, match="flags"):
            c.exact_table(T, 1.0, r2, flags=bad_flags)
    for f in (_capi.LGS_COORD_MAJOR, _capi.LGS_TARGETS_QFRAME, _capi.LGS_EXACT_ORDER, -1):
        with pytest.raises(ValueError, match="flags"):
            c.exact_sample(1, 0, 1, 1, flags=f)
    for f in (_capi.LGS_DEVICE_PTRS, _capi.LGS_COORD_MAJOR):
        with pytest.raises(ValueError):
            c.ball_points_host(T, r2, flags=f)
    for bad_sigma in (0.0, -1.0, math.nan, math.inf, None, "1", True):
        with pytest.raises(ValueError, match="sigma"):
            c.exact_table(T, bad_sigma, r2)
    with pytest.raises(ValueError, match="radius2"):
        c.ball_points(T, None)
    with pytest.raises(ValueError, match="radius2"):
        c.ball_points(T, np.ones(2))
    for bad_r in (None, np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]), np.zeros(2)):
        with pytest.raises(ValueError, match="radius2"):
            c.ball_points_host(T, bad_r)
        with pytest.raises(ValueError, match="radius2"):
            c.exact_table_host(T, 1.0, bad_r)
    with pytest.raises(ValueError, match="shift"):
        c.exact_table_host(T, 1.0, r2, np.array([0.0, np.inf, 0.0]))
    with pytest.raises(ValueError, match="z_out"):  # capacity without buffers
        c.ball_points(T, r2, capacity=5)
    with pytest.raises(ValueError, match="z_out"):  # int64 rows without LGS_Z64
        c.ball_points(T, r2, capacity=5, z_out=np.zeros((5, 4), dtype=np.int64), dist2_out=np.zeros(5))
    with pytest.raises(ValueError, match="z_out"):
        c.ball_points(T, r2, capacity=5, z_out=np.zeros((4, 4), dtype=np.int32), dist2_out=np.zeros(5))
    with pytest.raises(ValueError, match="offsets"):
        c.ball_points(T, r2, offsets=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError, match="weights"):
        c.exact_table(T, 1.0, r2, max_points=8, weights=np.zeros(7))
    for bad_n in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="n_draws"):
            c.exact_sample(1, 0, bad_n, 1)
    for bad_seed in (-1, 1 << 64, 1.5, None):
        with pytest.raises(ValueError, match="seed"):
            c.exact_sample(bad_seed, 0, 1, 1)
    with pytest.raises(ValueError, match="index"):
        c.exact_sample(1, 0, 3, 2, index=np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match="z_out"):
        c.exact_sample(1, 0, 3, 2, z_out=np.zeros((6, 4), dtype=np.int64))
    big = _bare_context(65)
    with pytest.raises(ValueError, match="d <= 64"):
        big.ball_points(np.zeros((1, 65)), np.ones(1))
    with pytest.raises(ValueError, match="d <= 64"):
        big.exact_table_host(np.zeros((1, 65)), 1.0, np.ones(1))


# ---------------------------------------------------------------- Decoder / SimpleLattice / ExactSampler on stubs
class _StubContext:
    """Stands in for _capi.Context with the CPU oracle behind it (targets in the lattice frame
    of the column lattice of B)."""

    def __init__(self, B, cvp_status=0, ball_status=0):
        self.B = np.asarray(B, dtype=np.float64)
        self.d = self.B.shape[0]
        self.Q, self.R = cvp_oracle.qr(self.B)
        self.cvp_status, self.ball_status, self.calls, self.table = cvp_status, ball_status, [], None

    def set_basis(self, *a, **kw):
        self.calls.append(("set_basis",))

    def set_decoder(self, **kw):
        self.calls.append(("set_decoder",))

    def closest_vector_host(self, targets, max_nodes, radius2=None, **kw):
        self.calls.append(("cvp", targets.copy(), max_nodes))
        D = np.array([cvp_oracle.se(self.R, t @ self.Q)[1] for t in targets])
        return {"z": None, "v": None, "cprime": None, "dist2": D, "nodes": np.zeros(len(D), dtype=np.int64),
                "status": np.full(len(D), self.cvp_status, dtype=np.int32)}

    def ball_points_host(self, targets, radius2, max_nodes=1 << 26, max_points=1 << 24, **kw):
        self.calls.append(("ball", targets.copy(), np.array(radius2, dtype=np.float64), max_nodes, max_points))
        zs, Ds, off, nodes = [], [], [0], []
        for t, A in zip(targets, radius2):
            z, D, nd, _ = ball_oracle.points(self.R, t @ self.Q, A)
            if self.ball_status:
                z, D = z[:0], D[:0]
            zs.append(z), Ds.append(D), off.append(off[-1] + len(D)), nodes.append(nd)
        return {"z": np.concatenate(zs), "dist2": np.concatenate(Ds), "offsets": np.array(off, dtype=np.int64),
                "nodes": np.array(nodes, dtype=np.int64), "cprime": None,
                "status": np.full(len(nodes), self.ball_status, dtype=np.int32)}

    def exact_table_host(self, targets, sigma, radius2, shift=None, max_nodes=1 << 26, max_points=1 << 24, *,
                         want_weights=False, flags=0):
        b = self.ball_points_host(targets, radius2, max_nodes, max_points)
        self.calls[-1] = ("table", targets.copy(), sigma, np.array(radius2), np.array(shift), max_nodes, max_points)
        off = b["offsets"]
        W = np.concatenate([ball_oracle.weights(b["dist2"][off[k]:off[k + 1]], sigma, shift[k])
                            for k in range(len(targets))])
        S = np.concatenate([ball_oracle.blocked_cumsum(W[off[k]:off[k + 1]]) for k in range(len(targets))])
        self.table = dict(b, W=W, S=S)
        return {"offsets": off, "nodes": b["nodes"], "status": b["status"], "mass": S[off[1:] - 1],
                "weights": W if want_weights else None, "cum": S if want_weights else None}

    def exact_sample_host(self, seed, first_sample, n_draws, n_targets, *, want_z=True, want_v=True, flags=0):
        self.calls.append(("sample", seed, first_sample, n_draws, n_targets))
        t = self.table
        assert len(t["offsets"]) - 1 == n_targets
        u = np.random.default_rng([seed, first_sample]).random(n_draws * n_targets)  # (not the library's stream)
        idx = np.array([t["offsets"][j // n_draws] +
                        ball_oracle.draw(t["S"][t["offsets"][j // n_draws]:t["offsets"][j // n_draws + 1]], u[j])
                        for j in range(len(u))], dtype=np.int64)
        z = t["z"][idx] if len(idx) else np.zeros((0, self.d), dtype=np.int64)
        return {"z": z if want_z else None, "v": z @ self.B.T if want_v else None, "index": idx,
                "dist2": t["dist2"][idx] if len(idx) else np.zeros(0)}


def _stub_decoder(B, **kw):
    from lgs_amd.decode import Decoder
    dec = object.__new__(Decoder)
    dec.basis = np.asarray(B, dtype=np.float64)
    dec.dimension, dec.ctx = dec.basis.shape[0], _StubContext(B, **kw)
    return dec


def test_decoder_ball_points_on_a_stub():
    B = cvp_oracle.bases()["d2"][0]
    dec = _stub_decoder(B)
    for bad in (np.zeros(3), np.zeros((5, 3)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            dec.ball_points(bad, radius2=1.0)
    with pytest.raises(ValueError, match="either"):
        dec.ball_points(np.zeros(2))
    with pytest.raises(ValueError, match="either"):
        dec.ball_points(np.zeros(2), radius2=1.0, sigma=1.0)
    with pytest.raises(ValueError, match="radius2"):
        dec.ball_points(np.zeros(2), radius2=-1.0)
    with pytest.raises(ValueError, match="nats"):
        dec.ball_points(np.zeros(2), sigma=1.0, nats=0.0)
    with pytest.raises(ValueError, match="sigma"):
        dec.ball_points(np.zeros(2), sigma=-1.0)
    assert dec.ctx.calls == []
    t = np.array([1.7, -0.6])
    z, D = dec.ball_points(t, sigma=0.8, nats=12.0, max_nodes=999, max_points=77)
    kind, tt, r2, mx, mp = dec.ctx.calls[-1]
    Dmin = cvp_oracle.se(dec.ctx.R, t @ dec.ctx.Q)[1]
    assert kind == "ball" and mx == 999 and mp == 77 and r2[0] == Dmin + 2.0 * 0.8 * 0.8 * 12.0
    assert z.shape == (len(D), 2) and z.dtype == np.int64 and D.min() == Dmin and len(D) > 1
    assert np.allclose(np.sum((z @ B.T - t) ** 2, axis=1), D, rtol=1e-12)
    both = dec.ball_points(np.stack([t, t + 1.0]), radius2=30.0)
    assert len(both) == 2 and all(np.all(Dk < 30.0) for _, Dk in both)
    flat = dec.ball_points(np.stack([t, t + 1.0]), radius2=30.0, flat=True)
    assert sorted(flat) == ["dist2", "nodes", "offsets", "status", "z"] and flat["offsets"][2] == len(flat["dist2"])
    assert np.array_equal(flat["z"][:flat["offsets"][1]], both[0][0])
    over = _stub_decoder(B, ball_status=1)
    with pytest.raises(RuntimeError, match="max_nodes"):
        over.ball_points(t, radius2=30.0)
    assert over.ball_points(t, radius2=30.0, flat=True)["status"][0] == 1
    with pytest.raises(RuntimeError, match="closest vector"):
        _stub_decoder(B, cvp_status=1).ball_points(t, sigma=1.0)
    big = _stub_decoder(np.eye(65))
    with pytest.raises(ValueError, match="d <= 64"):
        big.ball_points(np.zeros(65), radius2=1.0)


def _stub_lattice(rows, **kw):
    from lgs_amd.lattices import SimpleLattice
    lat = SimpleLattice(rows)
    lat._dec = _stub_decoder(np.asarray(rows, dtype=np.float64).T, **kw)  # the row lattice: columns of basis.T
    return lat


def test_first_minimum_on_a_stub():
    assert _stub_lattice(np.eye(4)).first_minimum() == 1.0
    rows = np.array([[4.0, 1.0], [1.0, 3.0]])
    lat = _stub_lattice(rows)
    box = min(float(np.sum((np.array(c) @ rows) ** 2)) for c in itertools.product(range(-9, 10), repeat=2) if any(c))
    assert box == 10.0
    assert lat.first_minimum(max_nodes=123) == pytest.approx(math.sqrt(10.0), rel=1e-14)
    kind, t, r2, mx, _ = lat._dec.ctx.calls[-1]
    assert kind == "ball" and mx == 123 and not t.any() and 10.0 < r2[0] < 10.0 + 1e-6
    # a basis whose rows are not shortest: rows (5, 4), (4, 3) generate (1, 1), of norm sqrt 2
    assert _stub_lattice(np.array([[5.0, 4.0], [4.0, 3.0]])).first_minimum() == pytest.approx(1.0, rel=1e-12)
    with pytest.raises(RuntimeError, match="max_nodes"):
        _stub_lattice(rows, ball_status=1).first_minimum()
    # the default smoothing parameter is unchanged, the exact one uses lambda_1 of the dual
    from lgs_amd.lattices import SimpleLattice
    dual = np.linalg.inv(rows @ rows.T) @ rows
    eta = math.sqrt(math.log(2 * 2 * (1 + 2.0 ** 53)) / math.pi) / float(np.min(np.linalg.norm(dual, axis=1)))
    assert SimpleLattice(rows).smoothing_parameter() == eta


def test_exact_sampler_on_a_stub():
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import ExactSampler
    B = cvp_oracle.bases()["d2"][0]
    lat = SimpleLattice(B)
    c = np.array([1.7, -0.6])
    for bad in (dict(nats=0.0), dict(nats=math.inf), dict(max_nodes=0), dict(max_points=2.5)):
        with pytest.raises(ValueError):
            ExactSampler(lat, 0.8, c, context=_StubContext(B), **bad)
    with pytest.raises(ValueError):
        ExactSampler(lat, -1.0, c, context=_StubContext(B))
    ctx = _StubContext(B)
    s = ExactSampler(lat, 0.8, c, nats=12.0, max_nodes=1 << 10, max_points=1 << 8, seed=5, context=ctx)
    assert ctx.calls == [("set_basis",), ("set_decoder",)] and s.seed == 5
    assert "NOT a bound on the omitted tail" in ExactSampler.__doc__
    v = s.sample(6)
    assert v.shape == (6, 2) and s._next_sample == 6
    kind, tt, sigma, r2, sh, mx, mp = [x for x in ctx.calls if x[0] == "table"][-1]
    Dmin = cvp_oracle.se(ctx.R, c @ ctx.Q)[1]
    assert sigma == 0.8 and sh[0] == Dmin and r2[0] == Dmin + 2.0 * 0.8 * 0.8 * 12.0 and (mx, mp) == (1 << 10, 1 << 8)
    assert ctx.calls[-1] == ("sample", 5, 0, 6, 1)
    z = s.sample_coefficients(3)
    assert z.shape == (3, 2) and ctx.calls[-1] == ("sample", 5, 6, 3, 1)
    assert sum(1 for x in ctx.calls if x[0] == "table") == 1  # the centre table is kept
    v2, z2 = s.sample_with_coefficients(4)
    assert np.array_equal(v2, z2 @ B.T) and s._next_sample == 13
    pts, zs = s.sample_around(np.stack([c, c + 0.5, c - 2.0]), 5, coefficients=True)
    assert pts.shape == (3, 5, 2) and zs.shape == (3, 5, 2) and ctx.calls[-1] == ("sample", 5, 13, 5, 3)
    assert s._next_sample == 28 and s.sample_around(c, 2).shape == (2, 2)
    s.sample(1)  # the centre table again
    assert ctx.calls[-1] == ("sample", 5, 30, 1, 1) and ctx.calls[-2][0] == "table"
    zz, p = s.pmf()
    assert zz.shape == (len(p), 2) and abs(p.sum() - 1.0) <= len(p) * 2.0 ** -52 and (p > 0).all()
    want = np.exp(-np.sum((zz @ B.T - c) ** 2, axis=1) / (2 * 0.64))
    assert np.allclose(p, want / want.sum(), rtol=1e-10)
    assert s.log_mass == pytest.approx(math.log(want.sum()), rel=1e-10)
    for bad in (np.zeros(3), np.zeros((0, 2))):
        with pytest.raises(ValueError):
            s.sample_around(bad, 1)
    with pytest.raises(ValueError, match="n_draws"):
        s.sample_around(c, 0)
    with pytest.raises(ValueError):
        s.sample(-1)
    with pytest.raises(RuntimeError, match="closest vector"):
        ExactSampler(lat, 0.8, c, context=_StubContext(B, cvp_status=1)).sample(1)
    with pytest.raises(ValueError, match="d <= 64"):
        ExactSampler(SimpleLattice(np.eye(65)), 1.0, context=_StubContext(np.eye(65)))
