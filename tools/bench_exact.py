"""Exact sampler: time per call of lgs_ball_points, lgs_exact_table and lgs_exact_sample beside
lgs_gaussian_mass, the comparator (the listing pass costs at least a counting pass).

usage: python tools/bench_exact.py [--cases one,many] [--warmup 2] [--reps 7] [--nats 12]

One MI355X, device buffers, the integral d = 12 basis and the two workloads of
tools/bench_mass.py:
  one    one centre at sigma = 20 (about 3.9 * 10^5 tree nodes, 1.1 * 10^5 points);
  many   2^12 targets at sigma = 12 (about 4.2 * 10^7 nodes, 5.9 * 10^6 points).
Per call: the host clock around the call and a device synchronise, and the library's timer 9
(the enumeration launches); 2 warm-up + 7 timed calls, median [min, max].
  (a) lgs_gaussian_mass   whole call and id 9
  (b) lgs_ball_points     whole call and id 9 (both passes)
  (c) lgs_exact_table     whole call
  (d) lgs_exact_sample    2^20 draws from the one table / 16 draws per target from the 2^12
                          tables, coefficients only, in draws/s
There is no threshold.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lattice-gaussian-mcmc_amd"))

CASES = {"one": (1, 20.0, 1 << 20), "many": (1 << 12, 12.0, 16)}


def stats(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one,many")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nats", type=float, default=12.0)
    ap.add_argument("--max-nodes", type=int, default=1 << 26)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgs_amd import _capi
    if not torch.cuda.is_available():
        sys.exit("bench_exact needs a GPU")
    dev = dict(device="cuda:0")
    B = np.rint(np.random.default_rng(12).standard_normal((12, 12)) * 4.0) + 40.0 * np.eye(12)
    d = B.shape[0]
    Q, R = np.linalg.qr(B)
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    R = np.ascontiguousarray(R * sg[:, None])
    Q = np.ascontiguousarray(Q * sg[None, :])
    F = _capi.LGS_DEVICE_PTRS
    for name in a.cases.split(","):
        n, sigma, K = CASES[name]
        Th = np.random.default_rng(1000 + d).standard_normal((n, d)) * 2500.0
        c = _capi.Context(0)
        c.set_basis(R, np.zeros(d), B, 1.0)
        c.set_decoder(Q=Q)
        D = c.closest_vector_host(Th, 1 << 24, want_z=False, want_v=False)["dist2"]
        T = torch.as_tensor(Th, **dev)
        r2 = torch.as_tensor(D + 2.0 * sigma * sigma * a.nats, **dev)
        sh = torch.as_tensor(D, **dev)
        mass = torch.empty(n, dtype=torch.float64, **dev)
        points = torch.empty(n, dtype=torch.int64, **dev)
        nodes = torch.empty(n, dtype=torch.int64, **dev)
        status = torch.empty(n, dtype=torch.int32, **dev)
        off = torch.empty(n + 1, dtype=torch.int64, **dev)
        c.ball_points(T, r2, a.max_nodes, 0, offsets=off, flags=F)  # the size query
        total = int(off[n])
        z = torch.empty((total, d), dtype=torch.int32, **dev)
        dist2 = torch.empty(total, dtype=torch.float64, **dev)
        zd = torch.empty((n * K, d), dtype=torch.int32, **dev)
        calls = {
            "mass": lambda: c.gaussian_mass(T, sigma, r2, sh, a.max_nodes, None, mass, None, points, None, None, nodes,
                                            status, F),
            "ball_points": lambda: c.ball_points(T, r2, a.max_nodes, total, z, dist2, None, off, nodes, status, F),
            "exact_table": lambda: c.exact_table(T, sigma, r2, sh, a.max_nodes, total, off, nodes, status, mass,
                                                 flags=F),
            "exact_sample": lambda: c.exact_sample(7, 0, K, n, zd, flags=F),
        }
        res = {"case": name, "d": d, "n": n, "sigma": sigma, "nats": a.nats, "warmup": a.warmup, "reps": a.reps,
               "device": c.device_info()["name"], "points_total": total, "draws": n * K}
        for key, call in calls.items():
            whole, enum = [], []
            for r in range(a.warmup + a.reps):
                c.timing_enable(True)  # (resets the totals)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                w = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    whole.append(w)
                    enum.append(c.timing_get(_capi.KERNEL_CVP_ENUM)[0])
            res[key + "_ms"] = stats(whole)
            if key in ("mass", "ball_points"):
                res[key + "_enumeration_ms"] = stats(enum)
        res["nodes_total"] = int(nodes.sum())
        res["status_counts"] = [int((status == k).sum()) for k in range(2)]
        res["ball_over_mass_whole"] = round(res["ball_points_ms"][0] / res["mass_ms"][0], 2)
        res["ball_over_mass_enumeration"] = round(res["ball_points_enumeration_ms"][0] /
                                                  res["mass_enumeration_ms"][0], 2)
        res["mdraws_per_s"] = round(n * K / res["exact_sample_ms"][0] / 1e3, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
