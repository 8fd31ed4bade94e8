"""Decoding by sampling: lgs_klein_decode against the route without it.

usage: python tools/decode_bench.py [--config C3_ntru512] [--n 4096] [--k 64] [--warmup 2] [--reps 7]

One MI355X, device buffers, coordinate-major targets uniform in [0, q)^d in the lattice
frame.  Two contexts alternate in one process:
  decode      one lgs_klein_decode call (n targets x K draws);
  comparator  the route of a library without it: the targets repeated K times in memory,
              lgs_klein_targets on the n K targets with v_out, then the distances, the
              argmin and the gather of the winners in torch.
Per call: the library timers (id 0 sampling kernel, 7 c' stage, 8 select + gather, 1 B z)
and the host clock around the call and a device synchronise.  Prints one JSON line with
median [min, max] ms of each, the counters, and whether both routes chose the same points."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3_ntru512")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--q", type=float, default=12289.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--exact", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgs_amd import _capi
    from lgs_amd.lattices import build_config
    if not torch.cuda.is_available():
        sys.exit("decode_bench needs a GPU")
    lat, sigma = build_config(a.config)
    B = lat.basis
    d = B.shape[0]
    Q, R = np.linalg.qr(B)
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    R = np.ascontiguousarray(R * sg[:, None])
    Q = np.ascontiguousarray(Q * sg[None, :])
    n, K = a.n, a.k
    ctxs = {}
    for name in ("decode", "comparator"):
        c = _capi.Context(0, max_proposals=n * K)
        c.set_basis(R, np.zeros(d), B, sigma)
        c.set_decoder(Q=Q)
        ctxs[name] = c
    dev = dict(device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(7)
    T = torch.rand((d, n), dtype=torch.float64, generator=g, **dev) * a.q  # coordinate-major
    f = _capi.LGS_DEVICE_PTRS | _capi.LGS_COORD_MAJOR | (_capi.LGS_EXACT_ORDER if a.exact else 0)
    z = torch.empty((d, n), dtype=torch.int32, **dev)
    v = torch.empty((n, d), dtype=torch.float64, **dev)
    best = torch.empty(n, dtype=torch.int64, **dev)
    d2 = torch.empty(n, dtype=torch.float64, **dev)
    zr = torch.empty((d, n * K), dtype=torch.int32, **dev)
    vr = torch.empty((n * K, d), dtype=torch.float64, **dev)
    ids = {"klein": _capi.KERNEL_KLEIN, "cprime": _capi.KERNEL_CPRIME, "select_gather": _capi.KERNEL_DECODE_SELECT,
           "bz": _capi.KERNEL_BZ}
    out = {}

    def timed(name, fn, first):
        c = ctxs[name]
        c.timing_enable(True)  # (resets the totals)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = fn(c, first)
        torch.cuda.synchronize()
        rec = {"whole": (time.perf_counter() - t0) * 1e3}
        rec.update(parts or {})
        for k, i in ids.items():
            rec[k] = c.timing_get(i)[0]
        return rec

    def run_decode(c, first):
        c.klein_decode(1, first, T, K, z, v, None, best, d2, flags=f)

    def run_comparator(c, first):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        Tr = T.repeat_interleave(K, dim=1)  # d x n K
        ev[1].record()
        c.klein_targets(1, first, Tr, zr, vr, None, f)
        ev[2].record()
        dist = ((vr.view(n, K, d) - T.t()[:, None, :]) ** 2).sum(dim=2)
        bk = dist.argmin(dim=1)
        cols = torch.arange(n, **dev) * K + bk
        out["cmp_best"], out["cmp_z"], out["cmp_v"] = bk, zr[:, cols], vr[cols]
        ev[3].record()
        torch.cuda.synchronize()
        return {"replicate": ev[0].elapsed_time(ev[1]), "torch_select": ev[2].elapsed_time(ev[3])}

    recs = {"decode": [], "comparator": []}
    for r in range(a.warmup + a.reps):
        first = 0  # the same draws every call, so the two routes can be compared
        for name, fn in (("decode", run_decode), ("comparator", run_comparator)):
            rec = timed(name, fn, first)
            if r >= a.warmup:
                recs[name].append(rec)
    calls = a.warmup + a.reps
    out["resolved"] = ctxs["decode"].counter(_capi.LGS_COUNTER_DECODE_RESOLVED) // calls
    out["decisions"] = {k: c.counter(_capi.LGS_COUNTER_RESOLVED) // calls for k, c in ctxs.items()}
    # one more call for the per-draw distances and bounds: how many draws per target the
    # intervals leave to the reference-order comparison
    dd = torch.empty((n, K), dtype=torch.float64, **dev)
    bd = torch.empty((n, K), dtype=torch.float64, **dev)
    ctxs["decode"].klein_decode(1, 0, T, K, None, None, None, best, d2, dd, bd, flags=f)
    torch.cuda.synchronize()
    cand = ((dd - bd) <= (dd + bd).min(dim=1, keepdim=True).values).sum(dim=1)
    srt = dd.sort(dim=1).values
    out["cand"] = {"max": int(cand.max()), "targets_with_more_than_one": int((cand > 1).sum()),
                   "evaluations": int(cand.sum()), "max_E_over_D": float((bd / dd).max()),
                   "median_E_over_D": float((bd / dd).median()),
                   "min_rel_gap_best_second": float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min())}
    same_best = int((out["cmp_best"] == best).sum())
    res = {"config": a.config, "d": d, "n": n, "K": K, "lanes": n * K, "exact": a.exact,
           "warmup": a.warmup, "reps": a.reps, "device": ctxs["decode"].device_info()["name"],
           "same_winner": same_best, "same_z_rows": int((out["cmp_z"] == z).all(dim=0).sum()),
           "v_equal": bool(torch.equal(out["cmp_v"][out["cmp_best"] == best], v[out["cmp_best"] == best])),
           "decode_resolved_per_call": out["resolved"], "decisions_resolved_per_call": out["decisions"],
           "dist2_min_max": [float(d2.min()), float(d2.max())], "candidates": out["cand"]}
    for name, rs in recs.items():
        res[name] = {k: stats([r[k] for r in rs]) for k in rs[0]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
