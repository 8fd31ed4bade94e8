"""Exact closest-vector decoding: nodes per second and time per call of lgs_closest_vector.

usage: python tools/bench_cvp.py [--cases int12,gauss37] [--warmup 2] [--reps 7] [--max-nodes 8388608]

One MI355X, device buffers, row-major targets 2500 * N(0, 1) in the lattice frame
(default_rng(1000 + d), the targets of tests/test_gpu_cvp.py):
  int12    2^12 targets on the integral d = 12 basis rint(4 N(0,1)) + 40 I (about 10^2 nodes
           each): many shallow trees, the launch is full of lanes;
  gauss37  64 targets on 6 N(0,1) + 25 I, d = 37 (millions of nodes each): one wave of deep
           trees, sliced into launches of 2^16 nodes per lane.
Per call: the library timers (id 7 c' stage, 9 enumeration launches, 8 compaction, 1 B z) and
the host clock around the call and a device synchronise; 2 warm-up + 7 timed calls, median
[min, max].  The reference has no exact decoder (src/lattices/base.py:136-155 raises), so
there is no baseline to compare with.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lattice-gaussian-mcmc_amd"))


def stats(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def bases(np):
    rng = np.random.default_rng(12)
    g37 = rng.standard_normal((37, 37)) * 6.0 + 25.0 * np.eye(37)
    i12 = np.rint(rng.standard_normal((12, 12)) * 4.0) + 40.0 * np.eye(12)
    return {"int12": (i12, 1 << 12), "gauss37": (g37, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="int12,gauss37")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-nodes", type=int, default=1 << 23)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgs_amd import _capi
    if not torch.cuda.is_available():
        sys.exit("bench_cvp needs a GPU")
    dev = dict(device="cuda:0")
    ids = {"cprime": _capi.KERNEL_CPRIME, "enumeration": _capi.KERNEL_CVP_ENUM,
           "compaction": _capi.KERNEL_DECODE_SELECT, "bz": _capi.KERNEL_BZ}
    for name in a.cases.split(","):
        B, n = bases(np)[name]
        d = B.shape[0]
        Q, R = np.linalg.qr(B)
        sg = np.where(np.diag(R) < 0, -1.0, 1.0)
        R = np.ascontiguousarray(R * sg[:, None])
        Q = np.ascontiguousarray(Q * sg[None, :])
        c = _capi.Context(0)
        c.set_basis(R, np.zeros(d), B, 1.0)
        c.set_decoder(Q=Q)
        Th = np.random.default_rng(1000 + d).standard_normal((n, d)) * 2500.0
        T = torch.as_tensor(Th, **dev)
        z = torch.empty((n, d), dtype=torch.int32, **dev)
        v = torch.empty((n, d), dtype=torch.float64, **dev)
        d2 = torch.empty(n, dtype=torch.float64, **dev)
        nodes = torch.empty(n, dtype=torch.int64, **dev)
        status = torch.empty(n, dtype=torch.int32, **dev)
        recs = []
        for r in range(a.warmup + a.reps):
            c.timing_enable(True)  # (resets the totals)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.closest_vector(T, a.max_nodes, None, z, v, None, d2, nodes, status, _capi.LGS_DEVICE_PTRS)
            torch.cuda.synchronize()
            rec = {"whole": (time.perf_counter() - t0) * 1e3}
            for k, i in ids.items():
                rec[k], rec[k + "_launches"] = c.timing_get(i)
            if r >= a.warmup:
                recs.append(rec)
        total = int(nodes.sum())
        res = {"case": name, "d": d, "n": n, "max_nodes": a.max_nodes, "warmup": a.warmup, "reps": a.reps,
               "device": c.device_info()["name"], "nodes_total": total,
               "nodes_per_target_median_max": [int(nodes.median()), int(nodes.max())],
               "status_counts": [int((status == k).sum()) for k in range(3)],
               "enumeration_launches": int(recs[0]["enumeration_launches"]),
               "compaction_launches": int(recs[0]["compaction_launches"])}
        for k in ("whole",) + tuple(ids):
            res[k + "_ms"] = stats([r[k] for r in recs])
        res["mnodes_per_s_call"] = round(total / res["whole_ms"][0] / 1e3, 2)
        res["mnodes_per_s_enumeration"] = round(total / res["enumeration_ms"][0] / 1e3, 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
