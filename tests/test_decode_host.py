"""CPU-side checks of Context.decode (lgs_nearest_plane / lgs_round_decode): caller
buffers of the wrong shape, element type or memory kind are rejected before anything
reaches the library, which would write past their end."""
import numpy as np
import pytest


class _FakeLib:
    """Stands in for the loaded library: records every call that would reach the device."""

    def __init__(self):
        self.calls = []

    def lgs_nearest_plane(self, h, n, t, z, v, flags):
        self.calls.append(("plane", n, flags))
        return 0

    def lgs_round_decode(self, h, n, t, z, v, flags):
        self.calls.append(("round", n, flags))
        return 0


class _FakeDeviceTensor:
    """The attributes _capi reads of a device tensor."""
    is_cuda = True

    def __init__(self, shape, dtype, index=0):
        self.shape, self.dtype = shape, dtype

        class _Dev:
            pass
        self.device = _Dev()
        self.device.index = index

    def data_ptr(self):
        return 0x1000

    def is_contiguous(self):
        return True


def _context(d=4):
    from lgs_amd import _capi
    c = object.__new__(_capi.Context)  # no device: the argument checks and the fake library
    c.d, c.device, c._h, c._L = d, 0, None, _FakeLib()
    return c


def test_decode_rejects_wrong_shapes_before_any_library_call():
    from lgs_amd import _capi
    c = _context()
    CM = _capi.LGS_COORD_MAJOR
    for method in ("plane", "round"):
        for kw in (dict(targets=np.zeros((3, 5))),                                  # (n, d') with d' != d
                   dict(targets=np.zeros((3, 4)), flags=CM),                        # row-major with COORD_MAJOR
                   dict(targets=np.zeros(4)),
                   dict(targets=np.zeros((2, 3, 4))),
                   dict(targets=np.zeros((3, 4)), z_out=np.zeros((2, 4), dtype=np.int32)),   # too few rows
                   dict(targets=np.zeros((3, 4)), z_out=np.zeros((4, 3), dtype=np.int32)),   # wrong layout
                   dict(targets=np.zeros((4, 3)), z_out=np.zeros((3, 4), dtype=np.int32), flags=CM),
                   dict(targets=np.zeros((3, 4)), v_out=np.zeros((3, 5))),
                   dict(targets=np.zeros((4, 3)), v_out=np.zeros((4, 3)), flags=CM)):        # v is (n, d)
            with pytest.raises(ValueError):
                c.decode(kw.pop("targets"), method, **kw)
    with pytest.raises(ValueError):
        c.decode(np.zeros((3, 4)), "babai")
    assert c._L.calls == []


def test_decode_rejects_wrong_dtype_before_any_library_call():
    from lgs_amd import _capi
    c = _context()
    t = np.zeros((3, 4))
    with pytest.raises(ValueError, match="expected int64"):       # would be written 8 bytes per element
        c.decode(t, "plane", np.zeros((3, 4), dtype=np.int32), None, _capi.LGS_Z64)
    with pytest.raises(ValueError, match="expected int32"):
        c.decode(t, "round", np.zeros((3, 4), dtype=np.int64), None, 0)
    with pytest.raises(ValueError, match="expected float64"):
        c.decode(t.astype(np.float32), "plane", np.zeros((3, 4), dtype=np.int32))
    with pytest.raises(ValueError, match="expected float64"):
        c.decode(t, "plane", None, np.zeros((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="expected float64"):
        c.decode(np.zeros((3, 4), dtype=np.int64), "round", np.zeros((3, 4), dtype=np.int32))
    assert c._L.calls == []


def test_decode_rejects_wrong_memory_kind_before_any_library_call():
    from lgs_amd import _capi
    c = _context()
    DEV = _capi.LGS_DEVICE_PTRS
    t, z, v = np.zeros((3, 4)), np.zeros((3, 4), dtype=np.int32), np.zeros((3, 4))
    dt = _FakeDeviceTensor((3, 4), "torch.float64")
    dz = _FakeDeviceTensor((3, 4), "torch.int32")
    for method in ("plane", "round"):
        with pytest.raises(ValueError, match="host buffer with LGS_DEVICE_PTRS set"):
            c.decode(t, method, z, v, DEV)
        with pytest.raises(ValueError, match="host buffer with LGS_DEVICE_PTRS set"):
            c.decode(dt, method, z, None, DEV)
        with pytest.raises(ValueError, match="device buffer with LGS_DEVICE_PTRS unset"):
            c.decode(dt, method, z, v, 0)
        with pytest.raises(ValueError, match="device buffer with LGS_DEVICE_PTRS unset"):
            c.decode(t, method, dz, None, 0)
        with pytest.raises(ValueError, match="context on cuda:0"):
            c.decode(_FakeDeviceTensor((3, 4), "torch.float64", index=1), method, dz, None, DEV)
    assert c._L.calls == []


def test_decode_chunk_switch_exists_in_the_hooks_library_only():
    """LGS_TEST_DECODE_CHUNK (tests/test_gpu_decode_exact.py reaches run_decode's second
    chunk with it) is a switch of the hooks build; the product library does not know it."""
    import os
    from lgs_amd import _capi
    prod = os.path.join(os.path.dirname(_capi.__file__), "_lib", "liblgs_hip.so")
    assert b"LGS_TEST_DECODE_CHUNK" in open(_capi.HOOKS_LIB_PATH, "rb").read()
    assert b"LGS_TEST_DECODE_CHUNK" not in open(prod, "rb").read()


def test_decode_passes_good_buffers_through():
    """The checks reject nothing valid: n from the layout, flags untouched, both methods,
    optional outputs, raw addresses taken on trust."""
    from lgs_amd import _capi
    c = _context()
    Z64, CM, DEV = _capi.LGS_Z64, _capi.LGS_COORD_MAJOR, _capi.LGS_DEVICE_PTRS
    c.decode(np.zeros((3, 4)), "plane", np.zeros((3, 4), dtype=np.int32), np.zeros((3, 4)))
    c.decode(np.zeros((4, 5)), "round", np.zeros((4, 5), dtype=np.int64), np.zeros((5, 4)), Z64 | CM)
    c.decode(np.zeros((7, 4)), "plane", None, np.zeros((7, 4)))
    c.decode(np.zeros((7, 4)), "round", np.zeros((7, 4), dtype=np.int32), None)
    c.decode(_FakeDeviceTensor((4, 6), "torch.float64"), "plane", _FakeDeviceTensor((4, 6), "torch.int32"),
             _FakeDeviceTensor((6, 4), "torch.float64"), DEV | CM)
    c.decode(_FakeDeviceTensor((2, 4), "torch.float64"), "plane", 0x2000, None, DEV | Z64)
    assert c._L.calls == [("plane", 3, 0), ("round", 5, Z64 | CM), ("plane", 7, 0), ("round", 7, 0),
                          ("plane", 6, DEV | CM), ("plane", 2, DEV | Z64)]
    z, v = c.decode_host(np.zeros((5, 4)), "round")
    assert z.shape == (5, 4) and z.dtype == np.int64 and v.shape == (5, 4)
    assert c._L.calls[-1] == ("round", 5, 0)
