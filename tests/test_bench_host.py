"""Host logic of bench.py's timed path (CPU), which lives in lgs_amd.distributed:
the lag-L autocovariance sums carried across bench steps, the exact
int64-in-fp64 packing of the single all-reduce, a gloo world-2 reduction that
equals the single-process statistics, and the counters' build-id check."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from lgs_amd import distributed as D  # noqa: E402


def _direct(x, L):
    """sum_t x_t x_{t-k} and pair counts over whole series (n_chains x T)."""
    S = [float((x[:, k:] * x[:, :x.shape[1] - k]).sum()) for k in range(L + 1)]
    N = [x.shape[0] * (x.shape[1] - k) for k in range(L + 1)]
    return np.array(S), np.array(N)


@pytest.mark.parametrize("T,L", [(64, 16), (5, 16), (16, 16), (1, 3)])
def test_lag_sums_across_blocks_equal_whole_series(T, L):
    rng = np.random.default_rng(T + L)
    x = rng.integers(-50, 50, (7, 6 * T)).astype(np.int64)
    acc = D.LagSums(torch, 7, L, torch.int64, "cpu")
    for b in range(6):
        acc.update(torch.from_numpy(x[:, b * T:(b + 1) * T]))
    S, N = _direct(x, L)
    np.testing.assert_array_equal(acc.S.numpy(), S)
    np.testing.assert_array_equal(acc.N, N)
    assert int(acc.S1) == x.sum() and int(acc.n) == x.size
    a = D.LagSums.acf(S, N, float(x.sum()), float(x.size))
    assert a[0] == pytest.approx(1.0)


def test_pack_unpack_exact_int64():
    ints = torch.tensor([0, 1, -1, 2**62 - 5, -(2**61) + 3], dtype=torch.int64)
    f = torch.tensor([1.5, -2.25])
    flat, layout = D.pack_f64(torch, [ints, f])
    a, b = D.unpack_f64(torch, flat, layout)
    assert torch.equal(a, ints) and torch.equal(b, f)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, x, out):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "lattice-gaussian-mcmc_amd"))
    import torch.distributed as dist
    from lgs_amd import distributed as bm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    half = x.shape[0] // world
    mine = x[rank * half:(rank + 1) * half]
    acc = bm.LagSums(torch, half, 8, torch.int64, "cpu")
    for b in range(4):
        acc.update(torch.from_numpy(mine[:, b * 10:(b + 1) * 10]))
    out[rank] = [t.numpy().tolist() for t in bm.allreduce_parts(acc.parts())]
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gloo_world2_lag_sums_match_single_process():
    x = np.random.default_rng(3).integers(-9, 9, (8, 40)).astype(np.int64)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.start_processes(_worker, args=(2, _free_port(), x, out), nprocs=2, join=True, start_method="spawn")
    single = D.LagSums(torch, 8, 8, torch.int64, "cpu")
    for b in range(4):
        single.update(torch.from_numpy(x[:, b * 10:(b + 1) * 10]))
    for r in (0, 1):
        S, N, S1, n = out[r]
        assert S == single.S.tolist() and N == single.N.tolist()
        assert S1 == single.S1.tolist() and n == [single.n]


def test_dump_outputs_writes_what_the_caller_received(tmp_path, monkeypatch):
    """bench.py --dump-outputs over a host stand-in for gpu_advance: float64 files of
    the last step's state and the reduced statistics; per-chain and per-step arrays at
    the seeded sample of chains / steps named by the index files (the last step always
    among them); the same sample on a second call; T = 1 works."""
    nc, T, d = 12, 5, 4
    rng = np.random.default_rng(1)
    st = {"z": torch.from_numpy(rng.integers(-9, 9, (d, nc)).astype(np.int32)),
          "lw": torch.from_numpy(rng.standard_normal(nc)),
          "v": torch.from_numpy(rng.integers(-99, 99, (nc, T, d)).astype(np.float64)),
          "zk": torch.from_numpy(rng.integers(-9, 9, (nc, T))),
          "vn2": torch.from_numpy(rng.random((nc, T)))}

    def advance(first_step, n_steps, acc, mom):
        acc += 1 + torch.arange(nc)
        return {"v": st["v"], "zk": st["zk"], "vn2": st["vn2"]}

    def gram(G, S):
        z = st["z"].long()
        G += z @ z.t()
        S += z.sum(1)

    advance.state, advance.gram = st, gram
    shard = D.StreamingShard(advance, nc, d, binv_row=np.ones(d), device="cpu", lag_chains=nc, lags=3, gram_every=1)
    shard.step(T)
    stats = shard.reduce()
    monkeypatch.setattr(bench, "DUMP_Z_ELEMS", 6 * d)
    monkeypatch.setattr(bench, "DUMP_V_ELEMS", 3 * 2 * d)
    monkeypatch.setattr(bench, "DUMP_V_STEPS", 2)
    outs = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), torch, advance, shard, stats)
        outs.append({f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = outs
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(x.dtype == np.float64 for x in a.values())
    ch, vch, steps = (a[k].astype(int) for k in ("sample_chains", "sample_chains_v", "sample_steps"))
    assert len(ch) == 6 and len(vch) == 3 and len(steps) == 2 and len(set(ch)) == 6
    np.testing.assert_array_equal(a["z_state"], st["z"].numpy().T[ch])
    np.testing.assert_array_equal(a["v_last_step"], st["v"].numpy()[vch][:, steps])
    assert steps[-1] == T - 1  # the block's last step: the chains' final state
    np.testing.assert_array_equal(a["zk_last_step"], st["zk"].numpy()[:, steps])
    np.testing.assert_array_equal(a["vnorm2_last_step"], st["vn2"].numpy()[:, steps])
    np.testing.assert_array_equal(a["log_weight"], st["lw"].numpy()[ch])
    np.testing.assert_array_equal(a["accepts_per_chain"], 1 + ch)
    z = st["z"].numpy().astype(np.int64)
    np.testing.assert_array_equal(a["gram_sum_zzT"], z @ z.T)
    assert a["accepts"].tolist() == [nc * (nc + 1) // 2] and a["gram_states"].tolist() == [nc]
    assert a["lag_z_S"].shape == (4,) and a["lag_v_N"].shape == (4,)
    for k in ("v", "zk", "vn2"):  # a one-step block: its only step is the sample
        st[k] = st[k][:, :1].contiguous()
    bench.dump_outputs(str(tmp_path / "c"), torch, advance, shard, stats)
    assert np.load(tmp_path / "c" / "sample_steps.npy").tolist() == [0]
    assert np.load(tmp_path / "c" / "v_last_step.npy").shape == (6, 1, d)  # (the element budget: more chains)


def test_counters_used_only_for_the_same_build(tmp_path):
    import json
    p = tmp_path / "x_klein_counters.json"
    p.write_text(json.dumps({"config": "C3_ntru512", "build_id": "abc", "fp64_flops": 1.0}))
    cnt, path, state = bench.load_counters(str(p), "C3_ntru512", "abc")
    assert state == "current" and cnt["fp64_flops"] == 1.0
    cnt, path, state = bench.load_counters(str(p), "C3_ntru512", "def")
    assert state == "stale" and cnt is None
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"\x7fELF...")
    assert bench.build_id(str(lib)) == bench.build_id(str(lib)) and len(bench.build_id(str(lib))) == 16
