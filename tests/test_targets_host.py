"""CPU-side checks of Klein sampling around per-sample targets (lgs_klein_targets):
the header declares it, the ctypes binding matches the declaration, and the sampler
method validates its argument before anything reaches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")


def test_header_declares_klein_targets():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_klein_targets\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_klein_targets not declared in lgs.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["lgs_ctx *ctx", "uint64_t seed", "uint64_t first_sample", "int64_t n",
                    "const double *targets", "void *z_out", "double *v_out", "double *cprime_out",
                    "uint32_t flags"]
    f = re.search(r"^#define LGS_TARGETS_QFRAME\s+(0x[0-9a-fA-F]+)u", txt, re.M)
    assert f and int(f.group(1), 16) == 0x800
    # no other sampling-call flag shares the bit
    others = re.findall(r"^#define (LGS_(?!CTX_|TARGETS_|ERR_|OK|BASIS_|COUNTER_)\w+)\s+(0x[0-9a-fA-F]+)u", txt, re.M)
    assert all(int(v, 16) != 0x800 for _, v in others), others


def test_capi_binds_klein_targets():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    want = int(re.search(r"^#define LGS_TARGETS_QFRAME\s+(0x[0-9a-fA-F]+)u", txt, re.M).group(1), 16)
    assert _capi.LGS_TARGETS_QFRAME == want
    assert "lgs_klein_targets" in _capi.EXPORTS
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        L = _capi.load_library(path)
        fn = L.lgs_klein_targets
        vp = ctypes.c_void_p
        assert fn.argtypes == [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, vp, vp, vp, vp,
                               ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
    assert _capi.KERNEL_CPRIME == 7
    assert callable(_capi.Context.klein_targets) and callable(_capi.Context.klein_targets_host)


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

    def klein_targets_host(self, seed, first, targets, **kw):
        self.calls.append(("klein_targets_host", seed, first, targets.shape, kw.get("flags", 0)))
        n = targets.shape[0]
        return {"z": np.zeros((n, self.d), dtype=np.int64), "v": np.zeros((n, self.d)), "cprime": None}


def test_sample_around_validates_shapes_before_any_device_call():
    from lgs_amd import _capi
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import KleinSampler
    ctx = _StubContext()
    s = KleinSampler(SimpleLattice(np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 1.0, 5.0]])), 3.0,
                     seed=5, context=ctx, exact_order=True)
    assert ctx.calls == ["set_basis"]
    for bad in (np.zeros(4), np.zeros((7, 2)), np.zeros((2, 3, 3)), 1.5):
        with pytest.raises(ValueError):
            s.sample_around(bad)
    assert ctx.calls == ["set_basis"] and s._next_sample == 0
    # shapes and counters of good calls: Q uploaded once, counters advance by n
    assert s.sample_around(np.zeros(3)).shape == (3,)
    v, z = s.sample_around(np.zeros((5, 3)), coefficients=True)
    assert v.shape == (5, 3) and z.shape == (5, 3)
    assert s.sample_around(np.zeros((0, 3))).shape == (0, 3)
    assert ctx.calls[1] == "set_decoder" and ctx.calls.count("set_decoder") == 1
    assert ctx.calls[2] == ("klein_targets_host", 5, 0, (1, 3), _capi.LGS_EXACT_ORDER)
    assert ctx.calls[3] == ("klein_targets_host", 5, 1, (5, 3), _capi.LGS_EXACT_ORDER)
    assert len(ctx.calls) == 4 and s._next_sample == 6


def test_context_klein_targets_rejects_wrong_shapes_without_a_library_call():
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = 4, 0, None, None
    with pytest.raises(ValueError):
        c.klein_targets(1, 0, np.zeros((3, 5)))
    with pytest.raises(ValueError):
        c.klein_targets(1, 0, np.zeros((3, 4)), flags=_capi.LGS_COORD_MAJOR)
    with pytest.raises(ValueError):
        c.klein_targets_host(1, 0, np.zeros((3, 5)))
    with pytest.raises(ValueError, match="expected int64"):
        c.klein_targets(1, 0, np.zeros((3, 4)), z_out=np.zeros((3, 4), dtype=np.int32), flags=_capi.LGS_Z64)
