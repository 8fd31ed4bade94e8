"""The layout matrix of the per-target entry points: decode (plane, round), klein_targets,
klein_decode, imhk_targets and closest_vector give the same bits whatever the caller's
buffers look like.

Reference: host buffers, row-major, int64 coefficients, lattice-frame targets, one chunk (a
context with the default max_proposals).  Against it, bit for bit, every output of the
product {host, device pointers} x {row-major, LGS_COORD_MAJOR} x {int32, LGS_Z64} x
{lattice frame, LGS_TARGETS_QFRAME} (the last axis where the entry point takes the flag; its
targets are the c' the reference call reports), at a chunking of 64 + 64 + 22 targets: the
second and the ragged third chunk use every per-chunk offset of every output.  The other test
files anchor the reference layout to the oracles.

d = 40 is no multiple of the 16- and 32-row panels, 150 targets are no multiple of a wave,
and K = 3 draws per target make the lanes of a target straddle waves."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 4242
FIRST = 1000      # first sample / chain counter of the sampling entry points
N = 150
K = 3             # n_draws of klein_decode, n_steps + 1 of imhk_targets
CHUNK = 64        # targets per chunk of the matrix calls: 64 + 64 + 22
MAX_NODES = 2000  # closest_vector: most of these d = 40 searches stop on the budget (status 1)
ENTRIES = ("plane", "round", "klein_targets", "klein_decode", "imhk_targets", "closest_vector")


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


def make_setup():
    """qary40 as tests/test_gpu_imhk_targets.py sets it up; radius2 shuts every third target
    of closest_vector out (status 2), a pattern that no chunk boundary preserves."""
    from lgs_amd import lattices
    B = np.asarray(lattices.qary_basis(20, 20, 3329, 5), dtype=np.float64)
    Q, R = np.linalg.qr(B, mode="complete")
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    Q, R = np.ascontiguousarray(Q * sg), np.ascontiguousarray(R * sg[:, None])
    T = np.random.default_rng(1040).standard_normal((N, 40)) * 2500.0
    r2 = np.where(np.arange(N) % 3 == 0, 0.0, 1e300)
    s = dict(B=B, Q=Q, R=R, Binv=np.linalg.inv(B), T=T, radius2=r2, d=40, sigma=165.7)
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def setup():
    return make_setup()


def context(capi, s, **kw):
    ctx = capi.Context(0, **kw)
    ctx.set_basis(s["R"], np.zeros(s["d"]), s["B"], s["sigma"])
    ctx.set_decoder(s["Q"], s["Binv"])
    return ctx


def chunked_context(capi, s, entry):
    """The context whose calls run in chunks of CHUNK targets.  The Babai decoders' chunk does
    not depend on max_proposals: the hooks library cuts it with LGS_TEST_DECODE_CHUNK, which
    the caller sets."""
    if entry in ("plane", "round"):
        return context(capi, s, hooks=True)
    return context(capi, s, max_proposals=CHUNK * (K if entry in ("klein_decode", "imhk_targets") else 1))


def combos(capi, entry):
    """(dev, cm, z64, qframe) of the matrix."""
    qf = (False,) if entry in ("plane", "round") else (False, True)
    return list(itertools.product((False, True), (False, True), (False, True), qf))


def run(capi, ctx, s, entry, src, dev=False, cm=False, z64=True, qframe=False):
    """One raw call on pre-filled buffers of the layout asked for; every output back as a
    host array in the reference layout (z as (n, d) int64)."""
    n, d = src.shape
    f = ((capi.LGS_DEVICE_PTRS if dev else 0) | (capi.LGS_COORD_MAJOR if cm else 0) |
         (capi.LGS_Z64 if z64 else 0) | (capi.LGS_TARGETS_QFRAME if qframe else 0))
    if dev:
        import torch

    def put(a):
        a = np.ascontiguousarray(a)
        return torch.as_tensor(np.array(a), device="cuda") if dev else a  # (a writable copy: no warning)

    def buf(shape, dtype, fill):
        return put(np.full(shape, fill, dtype=dtype))

    t = put(src.T if cm else src)
    o = {"z": buf((d, n) if cm else (n, d), np.int64 if z64 else np.int32, -77), "v": buf((n, d), np.float64, np.nan)}
    if entry not in ("plane", "round"):
        o["cprime"] = buf((n, d), np.float64, np.nan)
    if entry in ("plane", "round"):
        ctx.decode(t, entry, o["z"], o["v"], f)
    elif entry == "klein_targets":
        ctx.klein_targets(SEED, FIRST, t, o["z"], o["v"], o["cprime"], f)
    elif entry == "klein_decode":
        o.update(best_draw=buf(n, np.int64, -1), dist2=buf(n, np.float64, np.nan),
                 dist2_draws=buf((n, K), np.float64, np.nan), bound_draws=buf((n, K), np.float64, np.nan))
        ctx.klein_decode(SEED, FIRST, t, K, o["z"], o["v"], o["cprime"], o["best_draw"], o["dist2"],
                         o["dist2_draws"], o["bound_draws"], f)
    elif entry == "imhk_targets":
        o.update(logw=buf(n, np.float64, np.nan), accepts=buf(n, np.int64, -1), final_step=buf(n, np.int64, -1),
                 accepted=buf((n, K - 1), np.uint8, 77), logw_draws=buf((n, K), np.float64, np.nan),
                 bound_draws=buf((n, K), np.float64, np.nan))
        ctx.imhk_targets(SEED, FIRST, t, K - 1, o["z"], o["v"], o["cprime"], o["logw"], o["accepts"],
                         o["final_step"], o["accepted"], o["logw_draws"], o["bound_draws"], f)
    else:
        o.update(dist2=buf(n, np.float64, np.nan), nodes=buf(n, np.int64, -1), status=buf(n, np.int32, -1))
        ctx.closest_vector(t, MAX_NODES, put(s["radius2"]), o["z"], o["v"], o["cprime"], o["dist2"], o["nodes"],
                           o["status"], f)
    if dev:
        torch.cuda.synchronize()
        o = {k: a.cpu().numpy() for k, a in o.items()}
    o["z"] = np.ascontiguousarray(o["z"].T if cm else o["z"]).astype(np.int64)
    return o


_REFERENCE = {}  # entry -> outputs of the reference call (computed once, read-only)


def reference(capi, s, entry):
    if entry not in _REFERENCE:
        r = run(capi, context(capi, s), s, entry, s["T"])
        for a in r.values():
            a.setflags(write=False)
        _REFERENCE[entry] = r
    return _REFERENCE[entry]


def combo_id(dev, cm, z64, qframe):
    return "-".join(("device" if dev else "host", "coordmajor" if cm else "rowmajor", "z64" if z64 else "z32",
                     "qframe" if qframe else "lattice"))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_layout_gives_the_reference_bits(capi, setup, monkeypatch, entry):
    s = setup
    want = reference(capi, s, entry)
    if entry == "closest_vector":  # radius2 is read at the offsets of its targets
        assert (want["status"][::3] == 2).all() and (want["status"].reshape(-1, 3)[:, 1:] != 2).all()
    if entry == "imhk_targets":  # the scan accepted somewhere and rejected somewhere
        assert 0 < want["accepts"].sum() < N * (K - 1)
    ctx = chunked_context(capi, s, entry)
    if entry in ("plane", "round"):
        monkeypatch.setenv("LGS_TEST_DECODE_CHUNK", str(CHUNK))
    bad = []
    for dev, cm, z64, qframe in combos(capi, entry):
        got = run(capi, ctx, s, entry, want["cprime"] if qframe else s["T"], dev, cm, z64, qframe)
        assert got.keys() == want.keys()
        for k, w in want.items():
            g = got[k]
            if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
                bad.append((combo_id(dev, cm, z64, qframe), k))
    assert not bad, f"{entry}: outputs that differ from the reference call: {bad}"
