"""CPU-side checks of Klein sampling over a batch of bases (lgs_klein_bases): the header declares
the function, its output struct and its constant, and the ctypes mirror matches them; the Python
entry points validate their arguments before anything reaches a device; and the premises of the
device tests (tests/test_gpu_klein_bases.py) hold on the transcription (tests/kleinb_oracle.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import kleinb_oracle
import qr_oracle
from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")
FIELDS = ["int64_t *best_draw", "double *dist2", "int32_t *status", "int32_t *qr_status", "double *R",
          "double *cprime", "void *z_draws", "double *dist2_draws"]


def test_header_declares_klein_bases():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_klein_bases\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_klein_bases not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "uint64_t seed", "uint64_t first_sample", "int64_t n_bases", "int64_t d",
                    "int64_t T", "int64_t n_draws", "const double *bases", "const double *targets",
                    "const double *sigma", "int32_t precision", "void *z_out", "double *v_out",
                    "const lgs_klein_bases_outputs *out", "uint32_t flags"]
    assert re.search(r"^#define LGS_KLEINB_MAX_T 64\s*$", txt, re.M)
    assert "lgs_klein_bases: its input check and QR launches are id 7, its draw kernel id 0" in txt
    m = re.search(r"typedef struct lgs_klein_bases_outputs \{(.*?)\} lgs_klein_bases_outputs;", txt, re.S)
    assert m, "struct lgs_klein_bases_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == FIELDS


def test_library_exports_klein_bases():
    from lgs_amd import _capi
    assert "lgs_klein_bases" in _capi.EXPORTS and _capi.LGS_KLEINB_MAX_T == 64
    vp, i64, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        fn = _capi.load_library(path).lgs_klein_bases
        assert fn.argtypes == [vp, u64, u64, i64, i64, i64, i64, vp, vp, vp, ctypes.c_int32, vp, vp,
                               ctypes.POINTER(_capi.KleinBasesOutputs), ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
    assert [n for n, _ in _capi.KleinBasesOutputs._fields_] == [f.split("*")[1] for f in FIELDS]
    assert all(t is ctypes.c_void_p for _, t in _capi.KleinBasesOutputs._fields_)
    assert ctypes.sizeof(_capi.KleinBasesOutputs) == len(FIELDS) * ctypes.sizeof(ctypes.c_void_p)
    assert callable(_capi.Context.klein_bases) and callable(_capi.Context.klein_bases_host)
    from lgs_amd import samplers
    from lgs_amd.decode import sampling_decode_bases
    assert callable(samplers.klein_bases) and "klein_bases" in samplers.__all__ and callable(sampling_decode_bases)


def test_chunk_switch_lives_in_the_hooks_library_only():
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()
    assert 'hook("LGS_TEST_KLEINB_SLOTS")' in src and 'getenv("LGS_TEST_KLEINB' not in src
    txt = open(os.path.join(CSRC, "lgs_kleinb.hip")).read()
    assert "getenv" not in txt and "printf" not in txt and "assert(" not in txt
    mk = open(os.path.join(REPO, "lattice-gaussian-mcmc_amd", "Makefile")).read()
    assert "csrc/lgs_kleinb.hip" in mk and "-ffp-contract=off" in mk


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
    B, T, S = np.zeros((3, 4, 4)), np.zeros((3, 2, 4)), np.ones(3)
    bad = [(np.zeros((3, 4, 5)), T, S), (np.zeros((4, 4)), T, S), (B, np.zeros((3, 2, 5)), S),
           (B, np.zeros((2, 2, 4)), S), (B, np.zeros((3, 4)), S), (np.zeros((3, 65, 65)), np.zeros((3, 2, 65)), S),
           (B, np.zeros((3, 65, 4)), S), (B, np.zeros((3, 0, 4)), S), (np.zeros((3, 1, 1)), np.zeros((3, 2, 1)), S),
           (B, T, np.ones(2)), (B, T, np.ones((3, 1)))]
    for b, t, s in bad:
        with pytest.raises(ValueError):
            c.klein_bases(0, 0, b, t, s, 4)
        with pytest.raises(ValueError):
            c.klein_bases_host(0, 0, b, t, s, 4)
    for bad_k in (0, -1, (1 << 21) + 1, 2.5, None, True, "7"):
        with pytest.raises(ValueError, match="n_draws"):
            c.klein_bases(0, 0, B, T, S, bad_k)
        with pytest.raises(ValueError, match="n_draws"):
            c.klein_bases_host(0, 0, B, T, S, bad_k)
    for bad_p in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match="precision"):
            c.klein_bases(0, 0, B, T, S, 4, bad_p)
    for bad_sigma in (np.array([1.0, 0.0, 1.0]), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]),
                      np.array([1.0, np.inf, 1.0])):
        with pytest.raises(ValueError, match="sigma"):
            c.klein_bases_host(0, 0, B, T, bad_sigma, 4)
    for bad_flags in (_capi.LGS_EXACT_ORDER, _capi.LGS_COORD_MAJOR, _capi.LGS_TARGETS_QFRAME, 0x1000, -1, 1.0, True):
        with pytest.raises(ValueError, match="flags"):
            c.klein_bases(0, 0, B, T, S, 4, flags=bad_flags)
    with pytest.raises(ValueError):
        c.klein_bases_host(0, 0, B, T, S, 4, flags=_capi.LGS_DEVICE_PTRS)
    with pytest.raises(ValueError, match="expected float64"):
        c.klein_bases(0, 0, B.astype(np.float32), T, S, 4)
    with pytest.raises(ValueError, match="expected float64"):
        c.klein_bases(0, 0, B, T, S.astype(np.float32), 4)
    with pytest.raises(ValueError, match="expected int64"):
        c.klein_bases(0, 0, B, T, S, 4, z_out=np.zeros((3, 2, 4), dtype=np.int32), flags=_capi.LGS_Z64)
    with pytest.raises(ValueError, match="expected int32"):
        c.klein_bases(0, 0, B, T, S, 4, z_draws=np.zeros((3, 2, 4, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="host buffer"):
        c.klein_bases(0, 0, B, T, S, 4, flags=_capi.LGS_DEVICE_PTRS)
    for name, arr in (("z_out", np.zeros((3, 4, 2), dtype=np.int32)), ("v_out", np.zeros((3, 2, 5))),
                      ("best_draw", np.zeros((3, 3), dtype=np.int64)), ("dist2", np.zeros((3, 3))),
                      ("status", np.zeros((2, 3), dtype=np.int32)), ("qr_status", np.zeros((3, 2), dtype=np.int32)),
                      ("R", np.zeros((3, 4, 3))), ("cprime", np.zeros((3, 4, 2))),
                      ("z_draws", np.zeros((3, 2, 5, 4), dtype=np.int32)), ("dist2_draws", np.zeros((3, 2, 5)))):
        with pytest.raises(ValueError, match=name):
            c.klein_bases(0, 0, B, T, S, 4, **{name: arr})


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

    def klein_bases_host(self, seed, first_sample, bases, targets, sigma, n_draws, precision=10, **kw):
        self.calls.append(("klein_bases_host", bases.copy(), targets.shape, sigma.copy(), n_draws, kw))
        n, T, d = targets.shape
        z = np.tile(np.arange(1, d + 1, dtype=np.int64), (n, T, 1))
        return {"z": z if kw.get("want_z", True) else None,
                "v": np.einsum("nij,ntj->nti", bases, z.astype(float)) if kw.get("want_v", True) else None,
                "best_draw": np.zeros((n, T), dtype=np.int64), "dist2": np.zeros((n, T)),
                "status": np.zeros((n, T), dtype=np.int32), "qr_status": np.zeros(n, dtype=np.int32),
                "R": np.zeros((n, d, d)), "cprime": None, "z_draws": None, "dist2_draws": None}


def test_entry_points_validate_before_any_device_call():
    from lgs_amd.decode import sampling_decode_bases
    from lgs_amd.samplers import klein as klein_mod
    ctx = _StubContext()
    B = np.tile(np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 1.0, 5.0]]), (2, 1, 1))
    t = np.zeros((2, 3))
    for bases, targets in ((B[0], t), (np.zeros((2, 3, 4)), t), (B, np.zeros(3)), (B, np.zeros((3, 3))),
                           (B, np.zeros((2, 2, 4))), (B, np.zeros((2, 65, 3))), (np.zeros((2, 65, 65)), np.zeros((2, 65))),
                           (np.zeros((2, 1, 1)), np.zeros((2, 1))), (B.astype(complex), t), (B, t.astype(complex)), (B, None)):
        with pytest.raises(ValueError):
            sampling_decode_bases(bases, targets, 4, 1.0, context=ctx)
    for bad_k in (0, 2.5, None, True, (1 << 22) + 1):
        with pytest.raises(ValueError, match="n_draws"):
            sampling_decode_bases(B, t, bad_k, 1.0, context=ctx)
    for bad_sigma in (0.0, -1.0, np.nan, np.inf, "3", None, [1.0, 2.0, 3.0], [1.0, 0.0], np.ones((2, 1))):
        with pytest.raises(ValueError, match="sigma"):
            sampling_decode_bases(B, t, 4, bad_sigma, context=ctx)
        with pytest.raises(ValueError, match="sigma"):
            klein_mod.klein_bases(B, bad_sigma, t, 4)
    with pytest.raises(ValueError, match="integral"):
        sampling_decode_bases(B + 0.5, t, 4, 1.0, reduce=True, context=ctx)
    for bases, targets in ((B[0], t), (B, np.zeros((2, 2, 4))), (np.zeros((2, 65, 65)), None), (B, np.zeros((2, 65, 3)))):
        with pytest.raises(ValueError):
            klein_mod.klein_bases(bases, 1.0, targets, 4)
    with pytest.raises(ValueError, match="n_draws"):
        klein_mod.klein_bases(B, 1.0, None, 0)
    assert ctx.calls == []
    # good calls: one target per basis, several with rows=True and a width per basis
    v, info = sampling_decode_bases(B, t, 4, 2.0, context=ctx)
    assert v.shape == (2, 3) and info["dist2"].shape == (2,) and info["best_draw"].shape == (2,)
    v, z, info = sampling_decode_bases(B, np.zeros((2, 4, 3)), 7, [1.0, 2.0], rows=True, coefficients=True, context=ctx)
    assert v.shape == (2, 4, 3) and z.shape == (2, 4, 3) and info["status"].shape == (2, 4) and "lll_status" not in info
    assert [c[0] for c in ctx.calls] == ["klein_bases_host"] * 2
    assert np.array_equal(ctx.calls[0][3], [2.0, 2.0]) and np.array_equal(ctx.calls[1][3], [1.0, 2.0])
    assert np.array_equal(ctx.calls[1][1], np.swapaxes(B, 1, 2)) and ctx.calls[1][2] == (2, 4, 3) and ctx.calls[1][4] == 7


def test_reduce_maps_coefficients_back_and_forms_points_in_the_callers_basis():
    """U = [[1, 2, 0], [0, 1, 0], [0, 0, 1]], z_red = (1, 2, 3): z = U z_red = (5, 2, 3) for the basis
    LLL finished on, z_red itself for the other; v is qr_oracle.point(B, z) bit for bit."""
    from lgs_amd.decode import sampling_decode_bases
    ctx = _StubContext()
    B = np.tile(np.array([[4, 1, 0], [1, 3, 0], [0, 1, 5]], dtype=np.int64), (2, 1, 1))
    v, z, info = sampling_decode_bases(B, np.zeros((2, 2, 3)), 4, 1.5, reduce=True, coefficients=True, context=ctx)
    assert [c[0] for c in ctx.calls] == ["lll_reduce_host", "klein_bases_host"]
    assert np.array_equal(info["lll_status"], [0, 1])
    assert np.array_equal(z[:, 0], [[5, 2, 3], [1, 2, 3]]) and np.array_equal(z[:, 1], z[:, 0])
    drawn = ctx.calls[1][1]  # the bases the draws ran in
    assert np.array_equal(drawn[0], B[0] @ np.array([[1, 2, 0], [0, 1, 0], [0, 0, 1]])) and np.array_equal(drawn[1], B[1])
    for p in range(2):
        for k in range(2):
            assert v[p, k].tobytes() == qr_oracle.point(B[p], z[p, k]).tobytes()


# ---------------------------------------------------------------- the transcription itself
def test_vectorised_distance_and_point_are_the_scalar_definitions():
    d, T = 17, 5
    B, t = qr_oracle.pair(d, T, 1)
    _, R, cp = kleinb_oracle.qr_of(d, T, 1)
    z = np.random.default_rng(3).integers(-3000, 3001, size=(6, d))
    Rl, cl = R.tolist(), cp[2].tolist()
    for n in range(6):
        zl, D = [float(x) for x in z[n]], 0.0
        for i in range(d - 1, -1, -1):
            cs = 0.0
            for j in range(i + 1, d):
                cs = cs + Rl[i][j] * zl[j]
            q = Rl[i][i] * zl[i]
            r = (cl[i] - cs) - q
            D = D + r * r
        assert D == kleinb_oracle.distances(R, cp[2], z)[n]
        assert kleinb_oracle.points(B, z)[n].tobytes() == qr_oracle.point(B, z[n]).tobytes()


# ---------------------------------------------------------------- premises of the device tests
def _regimes(s):
    return [bool((s < 0.1).any()), bool(((s >= 0.1) & (s < 4)).any()), bool(((s >= 4) & (s < 50)).any()),
            bool((s >= 50).any())]


@pytest.mark.parametrize("d", [17, 33, 64])
def test_the_parity_widths_reach_all_four_samplez_regimes(d):
    """The first three bases of a parity batch carry sigma = 3, 300, 3000.  Counted on the
    transcription's R, coordinates with s < 0.1 / 0.1 <= s < 4 / 4 <= s < 50 / s >= 50:
      d = 17: sigma 3: 17/0/0/0, 300: 0/1/16/0, 3000: 0/0/9/8
      d = 33: sigma 3: 33/0/0/0, 300: 16/1/16/0, 3000: 0/17/8/8
      d = 64: sigma 3: 64/0/0/0, 300: 47/1/16/0, 3000: 32/16/8/8
    so every shape meets all four over its three widths, and d = 64 with sigma = 3000 alone (d = 17
    and 33 do not: their smallest s at 3000 are 9.4 and 0.15).  With s >= 50 the window 2 * 10 * s
    exceeds 1000 and is capped."""
    T = dict(qr_oracle.SHAPES)[d]
    seen = np.zeros(4, dtype=bool)
    for v in range(3):
        _, R, _ = kleinb_oracle.qr_of(d, T, v)
        s = kleinb_oracle.sigma_for(v) / np.diag(R)
        print(f"  d = {d}, sigma {kleinb_oracle.sigma_for(v)}: s_i {s.min():.3g} .. {s.max():.3g}")
        assert (np.diag(R) > 0).all()
        seen |= np.array(_regimes(s))
        if v == 2:
            assert (2 * 10 * s.max()) > 1000 and (d != 64 or _regimes(s) == [True] * 4)
    assert seen.all()


def test_sigma_3_at_d_64_gives_repeated_points_and_exact_ties():
    d, T = 64, 64
    B, t = qr_oracle.pair(d, T, 0)
    qr = kleinb_oracle.qr_of(d, T, 0)
    assert (3.0 / np.diag(qr[1]) < 0.1).all()
    r = kleinb_oracle.solve(B, t[:1], 3.0, 70, kleinb_oracle.SEED, 0, qr=(qr[0], qr[1], qr[2][:1]))
    distinct = np.unique(r["z_draws"][0], axis=0)
    D = r["dist2_draws"][0]
    print(f"  {len(distinct)} distinct points in 70 draws, {np.sum(D == D.min())} draws at the minimum")
    assert len(distinct) == 3
    assert np.sum(D == D.min()) > 1 and r["best_draw"][0] == np.flatnonzero(D == D.min())[0]
    assert r["fallbacks"] == 0


@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_parity_inputs_stay_far_from_int32_and_need_no_fallback(d, T):
    for K in kleinb_oracle.PARITY_K[(d, T)]:
        e = kleinb_oracle.expected(d, T, 3, K)
        zmax = np.abs(e["z_draws"]).max()
        print(f"  ({d}, {T}) K = {K}: max |z| {zmax}, fallbacks {e['fallbacks']}")
        assert zmax < 1 << 20 and e["fallbacks"] == 0
        assert not e["status"].any() and not e["qr_status"].any() and np.isfinite(e["dist2_draws"]).all()
        assert e["sigma"].tolist() == list(kleinb_oracle.SIGMAS)  # a width per basis, all different
