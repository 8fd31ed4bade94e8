"""Exact Gaussian mass: nodes per second and time per call of lgs_gaussian_mass.

usage: python tools/bench_mass.py [--cases one,many] [--warmup 2] [--reps 7] [--nats 12]

One MI355X, device buffers, the integral d = 12 basis rint(4 N(0,1)) + 40 I of
tests/cvp_oracle.py, row-major targets 2500 * N(0, 1) in the lattice frame
(default_rng(1012)), radius2 = D_min + 2 sigma^2 nats and shift = D_min from a
lgs_closest_vector call outside the timed region:
  one    one centre at sigma = 20 (about 3.9 * 10^5 tree nodes): the sampler's own case, where
         only the split of the tree into subtrees can use more than one lane;
  many   2^12 targets at sigma = 12 (about 10^4 nodes each).
Each is measured with the library's own split depth and with whole trees (the hooks library
with LGS_TEST_MASS_SPLIT=0, otherwise the same code).  Per call: the library timers (id 7 c'
stage, 9 enumeration launches, 8 compaction) and the host clock around the call and a device
synchronise, which includes the host's walk of the top levels; 2 warm-up + 7 timed calls,
median [min, max].  The comparators are the unsplit run and the node rate of the Python
oracle (tests/mass_oracle.py, about 0.5 M nodes/s on one CPU core); there is no threshold.
Prints one JSON line per case and split."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lattice-gaussian-mcmc_amd"))

CASES = {"one": (1, 20.0), "many": (1 << 12, 12.0)}


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
        sys.exit("bench_mass needs a GPU")
    dev = dict(device="cuda:0")
    ids = {"cprime": _capi.KERNEL_CPRIME, "enumeration": _capi.KERNEL_CVP_ENUM,
           "compaction": _capi.KERNEL_DECODE_SELECT}
    B = np.rint(np.random.default_rng(12).standard_normal((12, 12)) * 4.0) + 40.0 * np.eye(12)
    d = B.shape[0]
    Q, R = np.linalg.qr(B)
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    R = np.ascontiguousarray(R * sg[:, None])
    Q = np.ascontiguousarray(Q * sg[None, :])
    for name in a.cases.split(","):
        n, sigma = CASES[name]
        Th = np.random.default_rng(1000 + d).standard_normal((n, d)) * 2500.0
        for split in ("default", "0"):
            if split == "default":
                os.environ.pop("LGS_TEST_MASS_SPLIT", None)
            else:
                os.environ["LGS_TEST_MASS_SPLIT"] = split
            c = _capi.Context(0, hooks=True)
            c.set_basis(R, np.zeros(d), B, 1.0)
            c.set_decoder(Q=Q)
            D = c.closest_vector_host(Th, 1 << 24, want_z=False, want_v=False)["dist2"]
            T = torch.as_tensor(Th, **dev)
            r2 = torch.as_tensor(D + 2.0 * sigma * sigma * a.nats, **dev)
            sh = torch.as_tensor(D, **dev)
            mass = torch.empty(n, dtype=torch.float64, **dev)
            energy = torch.empty(n, dtype=torch.float64, **dev)
            points = torch.empty(n, dtype=torch.int64, **dev)
            nodes = torch.empty(n, dtype=torch.int64, **dev)
            status = torch.empty(n, dtype=torch.int32, **dev)
            recs = []
            for r in range(a.warmup + a.reps):
                c.timing_enable(True)  # (resets the totals)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.gaussian_mass(T, sigma, r2, sh, a.max_nodes, None, mass, energy, points, None, None, nodes,
                                status, _capi.LGS_DEVICE_PTRS)
                torch.cuda.synchronize()
                rec = {"whole": (time.perf_counter() - t0) * 1e3}
                for k, i in ids.items():
                    rec[k], rec[k + "_launches"] = c.timing_get(i)
                if r >= a.warmup:
                    recs.append(rec)
            total = int(nodes.sum())
            res = {"case": name, "split": split, "d": d, "n": n, "sigma": sigma, "nats": a.nats,
                   "warmup": a.warmup, "reps": a.reps, "device": c.device_info()["name"], "nodes_total": total,
                   "points_total": int(points.sum()), "status_counts": [int((status == k).sum()) for k in range(2)],
                   "log_mass_first": float(np.log(float(mass[0])) - D[0] / (2.0 * sigma * sigma)),
                   "enumeration_launches": int(recs[0]["enumeration_launches"]),
                   "compaction_launches": int(recs[0]["compaction_launches"])}
            for k in ("whole",) + tuple(ids):
                res[k + "_ms"] = stats([r[k] for r in recs])
            res["mnodes_per_s_call"] = round(total / res["whole_ms"][0] / 1e3, 2)
            print(json.dumps(res), flush=True)
    os.environ.pop("LGS_TEST_MASS_SPLIT", None)


if __name__ == "__main__":
    main()
