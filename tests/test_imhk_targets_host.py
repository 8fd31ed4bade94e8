"""CPU-side checks of IMHK chains around per-target centres (lgs_imhk_targets): the header
declares the function and its output struct, the ctypes mirror matches the header, the
Python entry points validate their arguments before anything reaches a device, and the CPU
oracle confirms the premises the device tests rest on (the chains neither accept nor reject
everything on the q-ary / NTRU bases, and on the d = 2 basis at sigma = 0.8 Klein's draw is
biased while 32 IMHK steps are not)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")
FIELDS = ["logw", "accepts", "final_step", "accepted", "logw_draws", "bound_draws"]


def test_header_declares_imhk_targets():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_imhk_targets\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_imhk_targets not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "uint64_t seed", "uint64_t first_chain", "int64_t n", "int64_t n_steps",
                    "const double *targets", "void *z_out", "double *v_out", "double *cprime_out",
                    "const lgs_imhk_targets_outputs *out", "uint32_t flags"]
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # decisions redone count under the existing id: none added


def test_library_exports_imhk_targets():
    from lgs_amd import _capi
    assert "lgs_imhk_targets" in _capi.EXPORTS
    vp = ctypes.c_void_p
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        fn = _capi.load_library(path).lgs_imhk_targets
        assert fn.argtypes == [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, vp,
                               ctypes.POINTER(_capi.ImhkTargetsOutputs), ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
    assert callable(_capi.Context.imhk_targets) and callable(_capi.Context.imhk_targets_host)


def test_imhk_targets_outputs_struct_matches_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    m = re.search(r"typedef struct lgs_imhk_targets_outputs \{(.*?)\} lgs_imhk_targets_outputs;", txt, re.S)
    assert m, "struct lgs_imhk_targets_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    names = [re.search(r"(\w+)$", f).group(1) for f in fields]
    assert names == [n for n, _ in _capi.ImhkTargetsOutputs._fields_]
    assert names == FIELDS
    assert all("*" in f for f in fields)  # every field a nullable pointer
    assert all(t is ctypes.c_void_p for _, t in _capi.ImhkTargetsOutputs._fields_)
    assert ctypes.sizeof(_capi.ImhkTargetsOutputs) == len(fields) * ctypes.sizeof(ctypes.c_void_p)


class _StubContext:
    """Stands in for _capi.Context: records every call that would reach the device."""

    def __init__(self):
        self.calls = []
        self.d = 0

    def set_basis(self, R, cprime, B, sigma, precision=10, linear_probs=False):
        self.d = R.shape[0]
        self.calls.append("set_basis")

    def set_decoder(self, Q=None, Binv=None):
        self.calls.append("set_decoder")

    def imhk_targets_host(self, seed, first_chain, targets, n_steps, **kw):
        self.calls.append(("imhk_targets_host", seed, first_chain, targets.shape, n_steps, kw.get("flags", 0)))
        n = targets.shape[0]
        return {"z": np.zeros((n, self.d), dtype=np.int64), "v": np.zeros((n, self.d)), "cprime": None,
                "logw": np.zeros(n), "accepts": np.full(n, n_steps // 2, dtype=np.int64),
                "final_step": np.zeros(n, dtype=np.int64)}


def test_sample_around_validates_before_any_device_call():
    from lgs_amd import _capi
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import IMHKSampler
    ctx = _StubContext()
    s = IMHKSampler(SimpleLattice(np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 1.0, 5.0]])), 3.0,
                    seed=5, context=ctx, exact_order=True, chain_id=9, burn_in=0)
    assert ctx.calls == ["set_basis"]
    for bad in (np.zeros(4), np.zeros((7, 2)), np.zeros((2, 3, 3)), 1.5):
        with pytest.raises(ValueError):
            s.sample_around(bad, 4)
    for bad_steps in (-1, 2.5, None, True, "3"):
        with pytest.raises(ValueError):
            s.sample_around(np.zeros((2, 3)), bad_steps)
    for bad_chain in (-1, 1.5, True):
        with pytest.raises(ValueError):
            s.sample_around(np.zeros((2, 3)), 4, first_chain=bad_chain)
    assert ctx.calls == ["set_basis"] and s._next_around_chain == 10
    # shapes and chain ids of good calls: Q uploaded once, the chain counter starts past the
    # sampler's own chain and advances by n; first_chain overrides it without moving it
    assert s.sample_around(np.zeros(3), 4).shape == (3,)
    v, z = s.sample_around(np.zeros((5, 3)), 8, coefficients=True)
    assert v.shape == (5, 3) and z.shape == (5, 3)
    assert s.stats.acceptance_rate == 0.5
    assert s.sample_around(np.zeros((0, 3)), 9).shape == (0, 3)
    assert s.sample_around(np.zeros((2, 3)), 0, first_chain=100).shape == (2, 3)
    assert ctx.calls[1] == "set_decoder" and ctx.calls.count("set_decoder") == 1
    assert ctx.calls[2] == ("imhk_targets_host", 5, 10, (1, 3), 4, _capi.LGS_EXACT_ORDER)
    assert ctx.calls[3] == ("imhk_targets_host", 5, 11, (5, 3), 8, _capi.LGS_EXACT_ORDER)
    assert ctx.calls[4] == ("imhk_targets_host", 5, 100, (2, 3), 0, _capi.LGS_EXACT_ORDER)
    assert len(ctx.calls) == 5 and s._next_around_chain == 16
    # the sampler's own chain is untouched
    assert s._next_step == 1 and s.total_proposals == 0 and s.current_state is None and not s._init[0]


def test_context_imhk_targets_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = 4, 0, None, None
    with pytest.raises(ValueError):
        c.imhk_targets(1, 0, np.zeros((3, 5)), 2)
    with pytest.raises(ValueError):
        c.imhk_targets(1, 0, np.zeros((3, 4)), 2, flags=_capi.LGS_COORD_MAJOR)
    with pytest.raises(ValueError):
        c.imhk_targets_host(1, 0, np.zeros((3, 5)), 2)
    with pytest.raises(ValueError):
        c.imhk_targets_host(1, 0, np.zeros((3, 4)), -1)
    with pytest.raises(ValueError):
        c.imhk_targets_host(1, 0, np.zeros((3, 4)), 2, flags=_capi.LGS_COORD_MAJOR)
    with pytest.raises(ValueError, match="expected int64"):
        c.imhk_targets(1, 0, np.zeros((3, 4)), 2, z_out=np.zeros((3, 4), dtype=np.int32), flags=_capi.LGS_Z64)
    with pytest.raises(ValueError, match="accepted"):
        c.imhk_targets(1, 0, np.zeros((3, 4)), 2, accepted=np.zeros((3, 2), dtype=np.int32))


# ---------------------------------------------------------------- premises, on the oracle
def _qr(B):
    Q, R = np.linalg.qr(np.asarray(B, dtype=np.float64), mode="full")
    for i in range(R.shape[0]):
        if R[i, i] < 0:
            R[i, :] *= -1
            Q[:, i] *= -1
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


@pytest.mark.parametrize("name,n", [("qary40", 64), ("ntru64", 64), ("qary128", 24)])
def test_oracle_acceptance_is_neither_zero_nor_one(oracle, name, n):
    """The device parity test asserts a summed acceptance strictly inside (0, 1) on these
    bases (targets default_rng(1000 + d) * 2500, seed 4242, 31 steps): 0.102 / 0.110 / 0.101."""
    from lgs_amd import lattices
    B = {"qary40": lambda: lattices.qary_basis(20, 20, 3329, 5), "ntru64": lambda: lattices.ntru_basis(32, 12289, 2),
         "qary128": lambda: lattices.qary_basis(64, 64, 3329, 1)}[name]()
    Q, R = _qr(B)
    d = B.shape[0]
    cp = (np.random.default_rng(1000 + d).standard_normal((n, d)) * 2500.0) @ Q
    acc = sum(int(oracle.imhk(R, cp[k], B, 165.7, 1, 31, seed=4242, first_chain=k,
                              mode=oracle.IMHK_WANG_LING)["accepts"][0]) for k in range(n))
    rate = acc / (31 * n)
    print(f"  {name}: oracle acceptance {rate:.3f} over {n} chains x 31 steps")
    assert 0.0 < rate < 1.0


def d2_exact_pmf(B, sigma, t, half=12):
    """D_{Lambda,sigma,t} over coefficients z in [-half, half]^2, by enumeration."""
    g = np.arange(-half, half + 1)
    zz = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    r2 = ((zz @ B.T - t) ** 2).sum(axis=1)
    p = np.exp(-r2 / (2.0 * sigma * sigma))
    return zz, p / p.sum()


def tv_distance(z, zz, p, half=12):
    """Total-variation distance of the empirical law of rows z from the pmf p on the grid zz
    (rows outside the grid count as mass the pmf does not have)."""
    inside = (np.abs(z) <= half).all(axis=1)
    idx = (z[inside, 0] + half) * (2 * half + 1) + (z[inside, 1] + half)
    emp = np.bincount(idx, minlength=p.size) / z.shape[0]
    assert np.array_equal(zz[idx[:1]], z[inside][:1])
    return 0.5 * (np.abs(emp - p).sum() + (1.0 - inside.mean()))


def test_oracle_d2_klein_is_biased_and_imhk_is_not(oracle):
    """B = [[4,1],[1,3]], sigma = 0.8, target (1.7, -0.6), 2^14 chains, seed 7: the oracle
    gives a total-variation distance of 0.218 for Klein's draw (step 0), 0.0035 after 32
    steps, acceptance 0.787; 2^14 exact samples give 0.003-0.005 by sampling noise alone."""
    B = np.array([[4.0, 1.0], [1.0, 3.0]])
    sigma, t, n = 0.8, np.array([1.7, -0.6]), 1 << 14
    Q, R = _qr(B)
    cp = t @ Q
    zz, p = d2_exact_pmf(B, sigma, t)
    z0, _, _ = oracle.imhk_parallel(R, cp, B, sigma, n, 0, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    z32, _, acc = oracle.imhk_parallel(R, cp, B, sigma, n, 32, seed=7, mode=oracle.IMHK_WANG_LING, threads=4)
    tv0, tv32, rate = tv_distance(z0, zz, p), tv_distance(z32, zz, p), acc.sum() / (32.0 * n)
    print(f"  TV(Klein) {tv0:.4f}, TV(32 steps) {tv32:.4f}, acceptance {rate:.3f}")
    assert tv0 >= 0.15
    assert tv32 <= 0.02
    assert 0.7 <= rate <= 0.9
