"""B z's diagonal-only tiles (bz_lean_kernel) and the worklist form of bz_i8_kernel.

A launch that reads the last Klein launch's int16 history computes the (64 samples x 128
coordinates) tiles whose live coefficient chunks meet only diagonal blocks of B without
the digit GEMM, and hands the rest to the GEMM kernel through a device worklist.  Every
case checks v against z @ B.T exactly and asserts lgs_bz_tiles, so that none can pass on
the wrong path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NC, T = 256, 4


@pytest.fixture(scope="module")
def capi():
    from lgs_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def c3(oracle):
    from lgs_amd.lattices import build_config
    lat, sigma = build_config("C3_ntru512")
    B = lat.basis
    R, cp = oracle.qr_prepare(B)
    return B, sigma, R, cp


def _tiles(n, d):
    return ((n + 63) // 64) * ((d + 127) // 128)


def _imhk(capi, ctx, d, calls=1, flags=0, vnorm2=False, fn_chains=0, nc=NC, steps=T, thin=1):
    """`calls` lgs_imhk calls of nc chains x steps steps (every thin-th kept) with device
    pointers; per call the kept z, v, the call's moments, ||v||^2 (optional) and lgs_bz_tiles."""
    import torch
    dev = "cuda:0"
    z = torch.zeros((nc, d), dtype=torch.int32, device=dev)
    lw = torch.zeros(nc, dtype=torch.float64, device=dev)
    init = torch.zeros(nc, dtype=torch.int32, device=dev)
    acc = torch.zeros(nc, dtype=torch.int64, device=dev)
    out = []
    for call in range(calls):
        zs = torch.zeros((nc, steps // thin, d), dtype=torch.int32, device=dev)
        vs = torch.full((nc, steps // thin, d), -7.0, dtype=torch.float64, device=dev)
        mom = torch.zeros(2 * d, dtype=torch.int64, device=dev)
        vn = torch.zeros((nc, steps // thin), dtype=torch.float64, device=dev) if vnorm2 else None
        ctx.bz_tiles(reset=True)
        ctx.imhk(7, 0, nc, 1 + call * steps, steps, thin, z, lw, init, acc, z_samples=zs, v_samples=vs, moments=mom,
                 vnorm2_samples=vn, fn_chains=fn_chains, flags=capi.LGS_DEVICE_PTRS | flags)
        torch.cuda.synchronize()
        out.append({"z": zs.cpu().numpy().reshape(-1, d).astype(np.int64), "v": vs.cpu().numpy().reshape(-1, d),
                    "mom": mom.cpu().numpy(), "vn": vn.cpu().numpy() if vnorm2 else None,
                    "tiles": ctx.bz_tiles(), "acc": acc.cpu().numpy().copy(), "state": z.cpu().numpy().copy()})
    return out


def _exact(o, B):
    assert np.array_equal(o["v"], o["z"].astype(np.float64) @ B.T)


def test_all_lean(capi, c3):
    """C3, 256 chains x 4 steps: the q-coordinates' z are 0, every tile is lean; the
    moments B z sums equal the sums of the kept z and z^2."""
    B, sigma, R, cp = c3
    d = B.shape[0]
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    o, = _imhk(capi, ctx, d)
    _exact(o, B)
    assert not o["z"][:, :d // 2].any()
    assert o["tiles"] == (_tiles(NC * T, d), 0)
    assert np.array_equal(o["mom"][:d], o["z"].sum(0))
    assert np.array_equal(o["mom"][d:], (o["z"] * o["z"]).sum(0))


def test_mixed(capi, oracle, c3):
    """A centre of scale 3e4 on the q-coordinates makes z_a nonzero everywhere: the tiles
    of the lower coordinates meet the dense block H, and the GEMM kernel computes them."""
    B, sigma, _, _ = c3
    d = B.shape[0]
    center = np.concatenate([np.random.default_rng(5).uniform(-3e4, 3e4, d // 2), np.zeros(d // 2)])
    R, cp = oracle.qr_prepare(B, center)
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    o, = _imhk(capi, ctx, d)
    _exact(o, B)
    assert o["z"][:, :d // 2].any()
    lean, gemm = o["tiles"]
    assert gemm > 0 and lean + gemm == _tiles(NC * T, d)
    assert np.array_equal(o["mom"][:d], o["z"].sum(0))
    assert np.array_equal(o["mom"][d:], (o["z"] * o["z"]).sum(0))


def test_one_dirty_tile(capi, oracle, c3):
    """A centre of half a basis vector of a q-coordinate puts that coordinate's mean at
    just under 1/2: a few samples round to 1, most to 0.  The oracle alone says that the kept
    rows have 64-sample tiles with a nonzero z_a (dirty) and tiles without; a dirty tile
    sends its lower coordinate tiles (the dense block H) to the GEMM kernel through the
    worklist, every other tile is lean, in the same launch."""
    from lgs_amd import lattices
    B, sigma, nc = lattices.ntru_basis(128, 12289, 3), 165.7, 64  # (d = 256: the oracle's time)
    d = B.shape[0]
    R, cp = oracle.qr_prepare(B, 0.49 * B[5].astype(np.float64))
    st = oracle.imhk(R, cp, B, sigma, nc, T, seed=7, first_step=1, trace=True)
    tr = st["trace"].reshape(-1, d)
    dirty = (tr[:, :d // 2] != 0).any(axis=1).reshape(-1, 64).any(axis=1)
    assert 0 < dirty.sum() < dirty.size  # the oracle's own verdict: clean and dirty tiles
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    o, = _imhk(capi, ctx, d, nc=nc)
    _exact(o, B)
    assert (o["z"][:, :d // 2] != 0).any()
    lean, gemm = o["tiles"]
    print(f"dirty tiles (oracle) {int(dirty.sum())} of {dirty.size}; lean {lean}, gemm {gemm}")
    assert lean > 0 and gemm > 0 and lean + gemm == _tiles(nc * T, d)


def test_rejections_mix_history_and_store(capi, c3):
    """Wang-Ling weights over two calls: the second call's kept rows mix proposals (history)
    and carried-in states (store); a tile with a store-sourced sample is the GEMM kernel's."""
    B, sigma, R, cp = c3
    d = B.shape[0]
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    o = _imhk(capi, ctx, d, calls=2, flags=capi.LGS_WANG_LING)
    for c in o:
        _exact(c, B)
    assert 0 < o[1]["acc"].sum() < 2 * NC * T
    lean, gemm = o[1]["tiles"]
    assert gemm > 0 and lean + gemm == _tiles(NC * T, d)


@pytest.mark.parametrize("n,lean", [(448, False), (256, True)])
def test_ragged_rows_and_8_byte_output(capi, c3, n, lean):
    """lgs_klein with lattice points at n = 448 (whole 64-sample tiles, but not the whole
    256-lane blocks the int8-digit far field needs: no history, the direct grid) and at
    n = 256, the smallest launch with a history (all lean), into an output one double into
    its allocation (8-byte stores): exact, nothing written outside."""
    import torch
    B, sigma, R, cp = c3
    d = B.shape[0]
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    out = []
    for off in (0, 1):
        z = torch.zeros((n, d), dtype=torch.int32, device="cuda:0")
        lw = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        buf = torch.full((n * d + 2,), -1.0, dtype=torch.float64, device="cuda:0")
        v = buf[off:off + n * d].view(n, d)
        assert (v.data_ptr() % 16 == 0) == (off == 0)
        ctx.bz_tiles(reset=True)
        ctx.klein(5, 0, n, z, v, lw, capi.LGS_DEVICE_PTRS)
        torch.cuda.synchronize()
        assert ctx.bz_tiles() == ((_tiles(n, d), 0) if lean else (0, _tiles(n, d)))
        assert np.array_equal(v.cpu().numpy(), z.cpu().numpy().astype(np.float64) @ B.T)
        b = buf.cpu().numpy()
        assert np.all(b[:off] == -1.0) and np.all(b[off + n * d:] == -1.0)
        out.append(v.cpu().numpy())
    assert np.array_equal(out[0], out[1])


def test_thinned_block_of_half_a_tile(capi, c3):
    """8 chains x 32 steps, every 8th kept: 32 kept rows in blocks of 4 per chain -- a
    ragged sample tile, and output rows that change chain every 4 (the per-row mapping)."""
    B, sigma, R, cp = c3
    d = B.shape[0]
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    o, = _imhk(capi, ctx, d, nc=8, steps=32, thin=8)
    _exact(o, B)
    assert o["z"].shape[0] == 32 and o["z"].any()
    assert o["tiles"] == (_tiles(32, d), 0)


def test_vnorm2_of_the_leading_chains(capi, c3):
    """lgs_imhk_ex with fn_chains = 64 < nc: ||v||^2 of those chains' rows, exactly."""
    B, sigma, R, cp = c3
    d = B.shape[0]
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, sigma)
    o, = _imhk(capi, ctx, d, vnorm2=True, fn_chains=64)
    _exact(o, B)
    assert o["tiles"] == (_tiles(NC * T, d), 0)
    assert np.array_equal(o["vn"][:64].reshape(-1), (o["v"] * o["v"]).sum(-1)[:64 * T])


@pytest.mark.parametrize("d", [64, 72])
def test_dense_basis_takes_the_direct_grid(capi, oracle, d):
    """A dense integer basis has no diagonal-only tile (d = 64), and d % 16 != 0 has no
    history to read (d = 72): the lean kernel is not launched, bz_i8_kernel's direct grid
    computes every tile."""
    B = np.random.default_rng(d).integers(-40, 41, (d, d)).astype(np.float64) + 300.0 * np.eye(d)
    R, cp = oracle.qr_prepare(B)
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, 40.0)
    ctx.bz_tiles(reset=True)
    r = ctx.klein_host(11, 0, 512, want_z=True, want_v=True)
    assert np.array_equal(r["v"], r["z"].astype(np.float64) @ B.T)
    assert ctx.bz_tiles() == (0, _tiles(512, d))


@pytest.mark.parametrize("d", [256, 208])
def test_diagonal_basis_with_negative_and_zero_entries(capi, oracle, d):
    """B diagonal with entries other than 1 and q, some negative, some 0 (R from the same
    diagonal with the zeros replaced: lgs_set_basis takes R and B separately): all lean,
    v = B_jj z_j, and +0.0 where B_jj or z_j is 0."""
    rng = np.random.default_rng(2)
    diag = rng.integers(-60, 61, d).astype(np.float64)
    diag[::7] = 0.0
    B = np.diag(diag)
    R, cp = oracle.qr_prepare(np.diag(np.where(diag == 0.0, 9.0, diag)))
    ctx = capi.Context(0)
    ctx.set_basis(R, cp, B, 300.0)
    ctx.bz_tiles(reset=True)
    r = ctx.klein_host(11, 0, 512, want_z=True, want_v=True)
    assert r["z"].any()
    assert np.array_equal(r["v"], r["z"].astype(np.float64) @ B.T)
    assert not np.signbit(r["v"]).any() or np.array_equal(np.signbit(r["v"]), r["v"] < 0)
    assert ctx.bz_tiles() == (_tiles(512, d), 0)


def test_pipelined_unpipelined_and_forced_cu_split_agree(capi, c3, monkeypatch):
    """C3, three calls: every output equal between a pipelined context, LGS_CTX_NO_PIPELINE
    and a context whose CU split is forced (hooks library)."""
    B, sigma, R, cp = c3
    d = B.shape[0]
    outs = []
    for kind in ("pipe", "nopipe", "split"):
        if kind == "split":
            monkeypatch.setenv("LGS_PIPE_CU_RESERVE", "32")
        ctx = capi.Context(0, pipeline=kind != "nopipe", hooks=kind == "split")
        ctx.set_basis(R, cp, B, sigma)
        outs.append(_imhk(capi, ctx, d, calls=3, vnorm2=True, fn_chains=64))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            for k in ("z", "v", "mom", "vn", "acc", "state"):
                assert np.array_equal(a[k], b[k]), k
            assert a["tiles"] == b["tiles"] == (_tiles(NC * T, d), 0)
