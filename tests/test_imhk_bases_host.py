"""CPU-side checks of IMHK chains over a batch of bases (lgs_imhk_bases): the header declares the
function and its output struct, and the ctypes mirror matches them; the Python entry points validate
their arguments before anything reaches a device; the transcription (tests/imhkb_oracle.py) is the C
oracle's IMHK chain bit for bit; and the premises of the device tests
(tests/test_gpu_imhk_bases.py) hold on it."""
import ctypes
import os
import re

import numpy as np
import pytest

import imhkb_oracle
import kleinb_oracle
import qr_oracle
from conftest import REPO
from test_imhk_targets_host import d2_exact_pmf, tv_distance

HEADER = os.path.join(REPO, "include", "lgs.h")
CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")
FIELDS = ["double *logw", "int64_t *accepts", "int64_t *final_step", "int32_t *status", "int32_t *qr_status",
          "double *R", "double *cprime", "uint8_t *accepted", "double *logw_draws", "void *z_draws", "void *z_samples"]
# the batch of the premises per shape: all 130 bases where they are distinct, the 3 distinct ones else
PREMISE_N = {d: (130 if qr_oracle.DISTINCT[d] >= 130 else 3) for d, _ in qr_oracle.SHAPES}


def test_header_declares_imhk_bases():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_imhk_bases\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_imhk_bases not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "uint64_t seed", "uint64_t first_chain", "int64_t n_bases", "int64_t d",
                    "int64_t T", "int64_t n_chains", "int64_t n_steps", "int32_t thin", "const double *bases",
                    "const double *targets", "const double *sigma", "int32_t precision", "void *z_out", "double *v_out",
                    "const lgs_imhk_bases_outputs *out", "uint32_t flags"]
    assert "lgs_imhk_bases: its input check and QR launches are id 7, its draw kernel id 0, its accept" in txt
    m = re.search(r"typedef struct lgs_imhk_bases_outputs \{(.*?)\} lgs_imhk_bases_outputs;", txt, re.S)
    assert m, "struct lgs_imhk_bases_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == FIELDS


def test_library_exports_imhk_bases():
    from lgs_amd import _capi
    assert "lgs_imhk_bases" in _capi.EXPORTS
    vp, i64, u64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        fn = _capi.load_library(path).lgs_imhk_bases
        assert fn.argtypes == [vp, u64, u64, i64, i64, i64, i64, i64, i32, vp, vp, vp, i32, vp, vp,
                               ctypes.POINTER(_capi.ImhkBasesOutputs), ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
    assert [n for n, _ in _capi.ImhkBasesOutputs._fields_] == [f.split("*")[1] for f in FIELDS]
    assert all(t is ctypes.c_void_p for _, t in _capi.ImhkBasesOutputs._fields_)
    assert ctypes.sizeof(_capi.ImhkBasesOutputs) == len(FIELDS) * ctypes.sizeof(ctypes.c_void_p)
    assert callable(_capi.Context.imhk_bases) and callable(_capi.Context.imhk_bases_host)
    from lgs_amd import samplers
    assert callable(samplers.imhk_bases) and "imhk_bases" in samplers.__all__


def test_chunk_switch_lives_in_the_hooks_library_only():
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()
    body = src[src.index("int lgs_imhk_bases("):]
    body = body[:body.index("\n}\n")]
    assert 'hook("LGS_TEST_KLEINB_SLOTS")' in body and "getenv" not in body
    txt = open(os.path.join(CSRC, "lgs_kleinb.hip")).read()
    assert "getenv" not in txt and "kleinb_draw_body<true>" in txt and "kleinb_draw_body<false>" in txt


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
            c.imhk_bases(0, 0, b, t, s, 2, 4)
        with pytest.raises(ValueError):
            c.imhk_bases_host(0, 0, b, t, s, 2, 4)
    for bad_c in (0, -1, 2.5, None, True, "7"):
        with pytest.raises(ValueError, match="n_chains"):
            c.imhk_bases(0, 0, B, T, S, bad_c, 4)
        with pytest.raises(ValueError, match="n_chains"):
            c.imhk_bases_host(0, 0, B, T, S, bad_c, 4)
    for bad_s in (-1, 2.5, None, True, "7"):
        with pytest.raises(ValueError, match="n_steps"):
            c.imhk_bases(0, 0, B, T, S, 2, bad_s)
        with pytest.raises(ValueError, match="n_steps"):
            c.imhk_bases_host(0, 0, B, T, S, 2, bad_s)
    for bad_c, bad_s in (((1 << 21) + 1, 0), (1, 1 << 21), (1 << 11, (1 << 10))):  # T C (S + 1) > 2^22
        with pytest.raises(ValueError, match="2\\^22"):
            c.imhk_bases(0, 0, B, T, S, bad_c, bad_s)
    for bad_thin in (0, -2, 1.5, None, True):
        with pytest.raises(ValueError, match="thin"):
            c.imhk_bases(0, 0, B, T, S, 2, 4, bad_thin)
        with pytest.raises(ValueError, match="thin"):
            c.imhk_bases_host(0, 0, B, T, S, 2, 4, bad_thin)
    for bad_p in (0, -3, 2.5, None, True):
        with pytest.raises(ValueError, match="precision"):
            c.imhk_bases(0, 0, B, T, S, 2, 4, 1, bad_p)
    for bad_first in (-1, 1.5, True, (1 << 32) - 11, 1 << 32):  # 3 * 2 * 2 = 12 chains
        with pytest.raises(ValueError, match="first_chain"):
            c.imhk_bases(0, bad_first, B, T, S, 2, 4)
        with pytest.raises(ValueError, match="first_chain"):
            c.imhk_bases_host(0, bad_first, B, T, S, 2, 4)
    for bad_sigma in (np.array([1.0, 0.0, 1.0]), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]),
                      np.array([1.0, np.inf, 1.0])):
        with pytest.raises(ValueError, match="sigma"):
            c.imhk_bases_host(0, 0, B, T, bad_sigma, 2, 4)
    for bad_flags in (_capi.LGS_EXACT_ORDER, _capi.LGS_COORD_MAJOR, _capi.LGS_TARGETS_QFRAME, 0x1000, -1, 1.0, True):
        with pytest.raises(ValueError, match="flags"):
            c.imhk_bases(0, 0, B, T, S, 2, 4, flags=bad_flags)
    with pytest.raises(ValueError):
        c.imhk_bases_host(0, 0, B, T, S, 2, 4, flags=_capi.LGS_DEVICE_PTRS)
    with pytest.raises(ValueError, match="expected float64"):
        c.imhk_bases(0, 0, B.astype(np.float32), T, S, 2, 4)
    with pytest.raises(ValueError, match="expected int64"):
        c.imhk_bases(0, 0, B, T, S, 2, 4, z_out=np.zeros((3, 2, 2, 4), dtype=np.int32), flags=_capi.LGS_Z64)
    with pytest.raises(ValueError, match="expected int32"):
        c.imhk_bases(0, 0, B, T, S, 2, 4, z_draws=np.zeros((3, 2, 2, 5, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="expected uint8"):
        c.imhk_bases(0, 0, B, T, S, 2, 4, accepted=np.zeros((3, 2, 2, 4), dtype=np.int32))
    with pytest.raises(ValueError, match="host buffer"):
        c.imhk_bases(0, 0, B, T, S, 2, 4, flags=_capi.LGS_DEVICE_PTRS)
    for name, arr in (("z_out", np.zeros((3, 2, 4), dtype=np.int32)), ("v_out", np.zeros((3, 2, 2, 5))),
                      ("logw", np.zeros((3, 2))), ("accepts", np.zeros((3, 2, 3), dtype=np.int64)),
                      ("final_step", np.zeros((3, 2), dtype=np.int64)), ("status", np.zeros((3, 2, 2), dtype=np.int32)),
                      ("qr_status", np.zeros((3, 2), dtype=np.int32)), ("R", np.zeros((3, 4, 3))),
                      ("cprime", np.zeros((3, 2, 2, 4))), ("accepted", np.zeros((3, 2, 2, 5), dtype=np.uint8)),
                      ("logw_draws", np.zeros((3, 2, 2, 4))), ("z_draws", np.zeros((3, 2, 2, 4, 4), dtype=np.int32)),
                      ("z_samples", np.zeros((3, 2, 2, 4, 4), dtype=np.int32))):
        with pytest.raises(ValueError, match=name):
            c.imhk_bases(0, 0, B, T, S, 2, 4, 2, **{name: arr})  # (thin 2: z_samples keeps 2 states)


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
        status[-1] = 1  # the last basis did not finish: its chains run unreduced
        return {"basis": basis @ U, "U": U, "status": status}

    def imhk_bases_host(self, seed, first_chain, bases, targets, sigma, n_chains, n_steps, thin=1, precision=10, **kw):
        self.calls.append(("imhk_bases_host", seed, first_chain, bases.copy(), targets.shape, sigma.copy(), n_chains,
                           n_steps, thin, kw))
        n, T, d = targets.shape
        C, nk = n_chains, n_steps // thin
        z = np.tile(np.arange(1, d + 1, dtype=np.int64), (n, T, C, 1))
        return {"z": z if kw.get("want_z", True) else None,
                "v": np.einsum("nij,ntcj->ntci", bases, z.astype(float)) if kw.get("want_v", True) else None,
                "z_samples": np.tile(z[:, :, :, None, :], (1, 1, 1, nk, 1)) if kw.get("want_samples") else None,
                "qr_status": np.zeros(n, dtype=np.int32)}


def test_sampler_entry_point_validates_before_any_device_call():
    from lgs_amd.samplers import imhk_bases
    ctx = _StubContext()
    B = np.tile(np.array([[4, 1, 0], [1, 3, 0], [0, 1, 5]], dtype=np.int64), (2, 1, 1))
    t = np.zeros((2, 3))
    for bases, targets in ((B[0], t), (np.zeros((2, 3, 4)), t), (B, np.zeros(3)), (B, np.zeros((3, 3))),
                           (B, np.zeros((2, 2, 4))), (B, np.zeros((2, 65, 3))), (np.zeros((2, 65, 65)), None),
                           (np.zeros((2, 1, 1)), None), (B.astype(complex), t), (B, t.astype(complex))):
        with pytest.raises(ValueError):
            imhk_bases(bases, 1.0, targets, context=ctx)
    for kw in ({"n_chains": 0}, {"n_chains": 2.5}, {"n_chains": True}, {"n_steps": -1}, {"n_steps": None},
               {"n_chains": 1 << 12, "n_steps": 1 << 10}, {"thin": 0}, {"thin": 1.5}, {"thin": True},
               {"first_chain": -1}, {"first_chain": (1 << 32) - 1}, {"first_chain": 2.0}):
        with pytest.raises(ValueError, match=next(iter(kw)) if len(kw) == 1 else "2\\^22"):
            imhk_bases(B, 1.0, t, context=ctx, **kw)
    for bad_sigma in (0.0, -1.0, np.nan, np.inf, "3", None, [1.0, 2.0, 3.0], [1.0, 0.0], np.ones((2, 1))):
        with pytest.raises(ValueError, match="sigma"):
            imhk_bases(B, bad_sigma, t, context=ctx)
    with pytest.raises(ValueError, match="integral"):
        imhk_bases(B + 0.5, 1.0, t, reduce=True, context=ctx)
    assert ctx.calls == []
    # good calls: shapes, the arguments that reach the context, the dropped T axis
    v = imhk_bases(B, 2.0, context=ctx)
    assert v.shape == (2, 1, 3)
    assert ctx.calls[-1][1:3] == (0, 0) and ctx.calls[-1][6:9] == (1, 32, 1) and ctx.calls[-1][4] == (2, 1, 3)
    v, z = imhk_bases(B, [1.0, 2.0], np.zeros((2, 4, 3)), n_chains=5, n_steps=9, thin=2, seed=3, first_chain=7,
                      rows=True, coefficients=True, context=ctx)
    assert v.shape == (2, 4, 5, 4, 3) and z.shape == (2, 4, 5, 4, 3)
    last = ctx.calls[-1]
    assert last[1:3] == (3, 7) and last[6:9] == (5, 9, 2) and np.array_equal(last[5], [1.0, 2.0])
    assert np.array_equal(last[3], np.swapaxes(B, 1, 2)) and last[9]["want_samples"] and not last[9]["want_z"]
    for p in range(2):
        assert v[p, 1, 2, 3].tobytes() == qr_oracle.point(np.swapaxes(B, 1, 2)[p], z[p, 1, 2, 3]).tobytes()
    # reduce: U = [[1, 2, 0], [0, 1, 0], [0, 0, 1]], z_red = (1, 2, 3): z = (5, 2, 3) where LLL finished
    ctx.calls.clear()
    v, z = imhk_bases(B, 1.5, t, n_chains=2, n_steps=4, reduce=True, coefficients=True, context=ctx)
    assert [c[0] for c in ctx.calls] == ["lll_reduce_host", "imhk_bases_host"]
    assert v.shape == (2, 2, 3) and np.array_equal(z[:, 0], [[5, 2, 3], [1, 2, 3]]) and np.array_equal(z[:, 1], z[:, 0])
    drawn = ctx.calls[1][3]  # the bases the chains ran in
    assert np.array_equal(drawn[0], B[0] @ np.array([[1, 2, 0], [0, 1, 0], [0, 0, 1]])) and np.array_equal(drawn[1], B[1])
    for p in range(2):
        assert v[p, 1].tobytes() == qr_oracle.point(B[p], z[p, 1]).tobytes()


# ---------------------------------------------------------------- the transcription itself
@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_the_composition_is_the_c_oracles_chain(oracle, d, T):
    """Klein sample c + t 2^32, log_weight and philox_u composed by imhkb_oracle.solve against
    lgs_oracle.imhk(mode=IMHK_WANG_LING) with one call per target: z, accepts and lw bit for bit, on
    the first three bases of every parity shape (465 chains)."""
    chains = 0
    for C, S in imhkb_oracle.PARITY_CS[(d, T)]:
        Bs, _, _ = qr_oracle.batch(d, T, 3)
        e = imhkb_oracle.expected(d, T, 3, C, S)
        for p in range(3):
            for k in range(T):
                o = oracle.imhk(e["R"][p], e["cprime"][p, k], Bs[p], float(e["sigma"][p]), C, S, seed=imhkb_oracle.SEED,
                                first_chain=imhkb_oracle.FIRST_CHAIN + (p * T + k) * C, mode=oracle.IMHK_WANG_LING)
                assert np.array_equal(o["z"], e["z"][p, k]) and np.array_equal(o["accepts"], e["accepts"][p, k])
                assert o["lw"].tobytes() == e["logw"][p, k].tobytes()
                chains += C
        assert np.array_equal(e["accepts"], e["accepted"].sum(axis=3))
        assert np.array_equal(e["final_step"] > 0, e["accepts"] > 0)
    print(f"  ({d}, {T}): {chains} chains equal")


def test_kept_states_follow_the_scan():
    """thin = 4 at S = 30: seven kept states, the draws that are the state after steps 4, 8, .., 28."""
    d, T, C, S, thin = 17, 5, 3, 30, 4
    e = imhkb_oracle.expected(d, T, 3, C, S, thin)
    one = imhkb_oracle.expected(d, T, 3, C, S)
    assert e["z_samples"].shape == (3, T, C, 7, d)
    assert np.array_equal(e["z_samples"], one["z_samples"][:, :, :, thin - 1::thin][:, :, :, :7])
    for k in ("z", "accepted", "logw"):
        assert np.array_equal(e[k], one[k])
    last = np.zeros((3, T, C), dtype=np.int64)  # the last accepted step <= 28
    for t in range(1, 29):
        last = np.where(one["accepted"][..., t - 1] == 1, t, last)
    assert np.array_equal(e["z_samples"][..., 6, :], np.take_along_axis(one["z_draws"], last[..., None, None], axis=3)[..., 0, :])


# ---------------------------------------------------------------- premises of the device tests
@pytest.mark.parametrize("d,T", qr_oracle.SHAPES)
def test_acceptance_and_settled_chains(d, T):
    """On the oracle alone.  Summed acceptance of the sigma = 3 bases lies strictly inside (0, 1):
    0.892, 0.894, 0.867 over the 130 distinct bases of d = 2, 3, 17 and 0.943, 0.938 on the three of
    d = 33, 64.  Unsettled chains (a decision within 2e-9 max(|lw_t|, |lw_x|) of its threshold): 0, 0,
    0, 0, 1 of 192, 11 of 192 -- the last two from the sigma = 3 basis, whose |lw| reaches 1.8e7; at
    most 10 % per shape."""
    n = PREMISE_N[d]
    for C, S in imhkb_oracle.PARITY_CS[(d, T)]:
        e = imhkb_oracle.expected(d, T, n, C, S)
        assert e["fallbacks"] == 0 and not e["status"].any() and np.isfinite(e["logw_draws"]).all()
        assert np.abs(e["z_draws"]).max() < 1 << 20
        out = int((~e["settled"]).sum())
        print(f"  ({d}, {T}) C = {C}, S = {S}: {out} of {e['settled'].size} chains unsettled, "
              f"max |lw| {np.abs(e['logw_draws']).max():.3g}")
        assert out <= 0.1 * e["settled"].size
        if S:
            three = e["sigma"] == 3.0
            rate = e["accepts"][three].sum() / (e["accepts"][three].size * S)
            print(f"    acceptance at sigma = 3: {rate:.3f}")
            assert three.any() and 0.0 < rate < 1.0


def test_oracle_d2_klein_is_biased_and_imhk_is_not(oracle):
    """B = [[4,1],[1,3]], sigma = 0.8, target (1.7, -0.6), 2^14 chains, seed 7, on QR(p)'s frame: the
    thresholds of tests/test_imhk_targets_host.py, TV(step 0) >= 0.15 and TV(32 steps) <= 0.02."""
    B = np.array([[4.0, 1.0], [1.0, 3.0]])
    sigma, t, n = 0.8, np.array([1.7, -0.6]), 1 << 14
    qs, R, cp = qr_oracle.qr(B, t[None])
    assert qs == 0
    zz, p = d2_exact_pmf(B, sigma, t)
    z0, _, _ = oracle.imhk_parallel(R, cp[0], B, sigma, n, 0, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    z32, _, _ = oracle.imhk_parallel(R, cp[0], B, sigma, n, 32, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    tv0, tv32 = tv_distance(z0, zz, p), tv_distance(z32, zz, p)
    print(f"  TV(Klein) {tv0:.4f}, TV(32 steps) {tv32:.4f}")
    assert tv0 >= 0.15
    assert tv32 <= 0.02
