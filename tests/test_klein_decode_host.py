"""CPU-side checks of decoding by sampling (lgs_klein_decode): the header declares the
function, its output struct and counter, the library exports the symbol, the ctypes
mirror matches the header, and the Python entry points validate their arguments before
anything reaches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "lgs.h")


def test_header_declares_klein_decode():
    txt = open(HEADER).read()
    m = re.search(r"^int lgs_klein_decode\s*\((.*?)\);", txt, re.M | re.S)
    assert m, "lgs_klein_decode not declared in lgs.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lgs_ctx *ctx", "uint64_t seed", "uint64_t first_sample", "int64_t n", "int64_t n_draws",
                    "const double *targets", "void *z_out", "double *v_out", "double *cprime_out",
                    "const lgs_decode_outputs *out", "uint32_t flags"]
    c = re.search(r"^#define LGS_COUNTER_DECODE_RESOLVED\s+(\d+)", txt, re.M)
    assert c and int(c.group(1)) == 6
    ids = [int(v) for v in re.findall(r"^#define LGS_COUNTER_\w+\s+(\d+)", txt, re.M)]
    assert sorted(ids) == list(range(11))  # no id shared or skipped


def test_library_exports_klein_decode():
    from lgs_amd import _capi
    assert "lgs_klein_decode" in _capi.EXPORTS
    assert _capi.LGS_COUNTER_DECODE_RESOLVED == 6
    vp = ctypes.c_void_p
    for path in (_capi.LIB_PATH, _capi.HOOKS_LIB_PATH):
        L = _capi.load_library(path)
        fn = L.lgs_klein_decode
        assert fn.argtypes == [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, vp,
                               ctypes.POINTER(_capi.DecodeOutputs), ctypes.c_uint32]
        assert fn.restype is ctypes.c_int
    assert callable(_capi.Context.klein_decode) and callable(_capi.Context.klein_decode_host)


def test_decode_outputs_struct_matches_header():
    from lgs_amd import _capi
    txt = open(HEADER).read()
    m = re.search(r"typedef struct lgs_decode_outputs \{(.*?)\} lgs_decode_outputs;", txt, re.S)
    assert m, "struct lgs_decode_outputs not in lgs.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    names = [re.search(r"(\w+)$", f).group(1) for f in fields]
    assert names == [n for n, _ in _capi.DecodeOutputs._fields_]
    assert names == ["best_draw", "dist2", "dist2_draws", "bound_draws"]
    assert all("*" in f for f in fields)  # every field a nullable pointer
    assert all(t is ctypes.c_void_p for _, t in _capi.DecodeOutputs._fields_)
    assert ctypes.sizeof(_capi.DecodeOutputs) == len(fields) * ctypes.sizeof(ctypes.c_void_p)


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

    def klein_decode_host(self, seed, first, targets, n_draws, **kw):
        self.calls.append(("klein_decode_host", seed, first, targets.shape, n_draws, kw.get("flags", 0)))
        n = targets.shape[0]
        return {"z": np.zeros((n, self.d), dtype=np.int64), "v": np.zeros((n, self.d)), "cprime": None,
                "best_draw": np.zeros(n, dtype=np.int64), "dist2": np.zeros(n)}


def test_decode_around_validates_before_any_device_call():
    from lgs_amd import _capi
    from lgs_amd.lattices import SimpleLattice
    from lgs_amd.samplers import KleinSampler
    ctx = _StubContext()
    s = KleinSampler(SimpleLattice(np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 1.0, 5.0]])), 3.0,
                     seed=5, context=ctx, exact_order=True)
    assert ctx.calls == ["set_basis"]
    for bad in (np.zeros(4), np.zeros((7, 2)), np.zeros((2, 3, 3)), 1.5):
        with pytest.raises(ValueError):
            s.decode_around(bad, 4)
    for bad_k in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError):
            s.decode_around(np.zeros((2, 3)), bad_k)
    assert ctx.calls == ["set_basis"] and s._next_sample == 0
    # shapes and counters of good calls: Q uploaded once, counters advance by n * n_draws
    assert s.decode_around(np.zeros(3), 4).shape == (3,)
    v, z = s.decode_around(np.zeros((5, 3)), 7, coefficients=True)
    assert v.shape == (5, 3) and z.shape == (5, 3)
    assert s.decode_around(np.zeros((0, 3)), 9).shape == (0, 3)
    assert ctx.calls[1] == "set_decoder" and ctx.calls.count("set_decoder") == 1
    assert ctx.calls[2] == ("klein_decode_host", 5, 0, (1, 3), 4, _capi.LGS_EXACT_ORDER)
    assert ctx.calls[3] == ("klein_decode_host", 5, 4, (5, 3), 7, _capi.LGS_EXACT_ORDER)
    assert len(ctx.calls) == 4 and s._next_sample == 4 + 35


def test_context_klein_decode_rejects_bad_arguments_without_a_library_call():
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: only the argument checks run
    c.d, c.device, c._h, c._L = 4, 0, None, None
    with pytest.raises(ValueError):
        c.klein_decode(1, 0, np.zeros((3, 5)), 2)
    with pytest.raises(ValueError):
        c.klein_decode(1, 0, np.zeros((3, 4)), 2, flags=_capi.LGS_COORD_MAJOR)
    with pytest.raises(ValueError):
        c.klein_decode_host(1, 0, np.zeros((3, 5)), 2)
    with pytest.raises(ValueError):
        c.klein_decode_host(1, 0, np.zeros((3, 4)), 0)
    with pytest.raises(ValueError, match="expected int64"):
        c.klein_decode(1, 0, np.zeros((3, 4)), 2, z_out=np.zeros((3, 4), dtype=np.int32), flags=_capi.LGS_Z64)
    with pytest.raises(ValueError, match="best_draw"):
        c.klein_decode(1, 0, np.zeros((3, 4)), 2, best_draw=np.zeros(3, dtype=np.int32))
