"""IMHK chains around per-target centres: lgs_imhk_targets against lgs_klein_decode's
sampling kernel and against the route without it.

usage: python tools/bench_imhk_targets.py [--config C3_ntru512] [--n 4096] [--steps 63] [--legacy 16]
                                          [--warmup 2] [--reps 7]

One MI355X, device buffers, coordinate-major targets uniform in [0, q)^d in the lattice
frame.  Two contexts alternate in one process on the same targets:
  imhk    one lgs_imhk_targets call (n chains x steps + 1 draws);
  decode  one lgs_klein_decode call with K = steps + 1 draws per target -- the same lanes,
          centres and back-substitution, so the difference of the two sampling kernels
          (timer 0) is the cost of the Wang-Ling weights and their bounds.
Per call: the library timers (id 7 c' stage, 0 sampling kernel, 8 scan / select + gather,
1 B z) and the host clock around the call and a device synchronise.
Then the only earlier route to such chains, for --legacy targets: per target one
lgs_set_basis with c' = Q^T t and one lgs_imhk(n_chains = 1, steps, LGS_WANG_LING) from an
uninitialised state, host clock, with the linear extrapolation to n targets marked as such.
--normal S draws the targets as S * N(0, 1) instead: small coefficients, hence tight weight
bounds and few recomputed decisions (the uniform targets give |z| ~ 10^6 on this basis).
Prints one JSON line: median [min, max] ms of each, the sampling kernels' ratio, the share
of timer 8 in the call, and the accept decisions redone per call (LGS_COUNTER_ACCEPT_RESOLVED)."""
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
    ap.add_argument("--steps", type=int, default=63)
    ap.add_argument("--legacy", type=int, default=16)
    ap.add_argument("--q", type=float, default=12289.0)
    ap.add_argument("--normal", type=float, default=0.0,
                    help="targets scale * N(0, 1) instead of uniform in [0, q)^d (small |z|: tight weight bounds)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--exact", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from lgs_amd import _capi
    from lgs_amd.lattices import build_config
    if not torch.cuda.is_available():
        sys.exit("bench_imhk_targets needs a GPU")
    lat, sigma = build_config(a.config)
    B = lat.basis
    d = B.shape[0]
    Q, R = np.linalg.qr(B)
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    R = np.ascontiguousarray(R * sg[:, None])
    Q = np.ascontiguousarray(Q * sg[None, :])
    n, T_steps = a.n, a.steps
    K = T_steps + 1
    ctxs = {}
    for name in ("imhk", "decode"):
        c = _capi.Context(0, max_proposals=n * K)
        c.set_basis(R, np.zeros(d), B, sigma)
        c.set_decoder(Q=Q)
        ctxs[name] = c
    dev = dict(device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(7)
    if a.normal > 0.0:
        T = torch.randn((d, n), dtype=torch.float64, generator=g, **dev) * a.normal
    else:
        T = torch.rand((d, n), dtype=torch.float64, generator=g, **dev) * a.q  # coordinate-major
    f = _capi.LGS_DEVICE_PTRS | _capi.LGS_COORD_MAJOR | (_capi.LGS_EXACT_ORDER if a.exact else 0)
    z = torch.empty((d, n), dtype=torch.int32, **dev)
    v = torch.empty((n, d), dtype=torch.float64, **dev)
    logw = torch.empty(n, dtype=torch.float64, **dev)
    acc = torch.empty(n, dtype=torch.int64, **dev)
    best = torch.empty(n, dtype=torch.int64, **dev)
    d2 = torch.empty(n, dtype=torch.float64, **dev)
    ids = {"cprime": _capi.KERNEL_CPRIME, "klein": _capi.KERNEL_KLEIN, "scan_or_select_gather": _capi.KERNEL_DECODE_SELECT,
           "bz": _capi.KERNEL_BZ}

    def timed(name, fn):
        c = ctxs[name]
        c.timing_enable(True)  # (resets the totals)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(c)
        torch.cuda.synchronize()
        rec = {"whole": (time.perf_counter() - t0) * 1e3}
        for k, i in ids.items():
            rec[k] = c.timing_get(i)[0]
        return rec

    def run_imhk(c):
        c.imhk_targets(1, 0, T, T_steps, z, v, None, logw, acc, flags=f)

    def run_decode(c):
        c.klein_decode(1, 0, T, K, z, v, None, best, d2, flags=f)

    recs = {"imhk": [], "decode": []}
    ctxs["imhk"].counter(_capi.LGS_COUNTER_ACCEPT_RESOLVED, reset=True)
    for r in range(a.warmup + a.reps):
        for name, fn in (("imhk", run_imhk), ("decode", run_decode)):
            rec = timed(name, fn)
            if r >= a.warmup:
                recs[name].append(rec)
    calls = a.warmup + a.reps
    ci = ctxs["imhk"]
    run_imhk(ci)  # (leaves the chains' results in z / acc for the figures below)
    torch.cuda.synchronize()
    bd = torch.empty((n, K), dtype=torch.float64, **dev)
    ci.imhk_targets(1, 0, T, T_steps, None, None, None, bound_draws=bd, flags=f)
    torch.cuda.synchronize()
    res = {"config": a.config, "d": d, "n": n, "steps": T_steps, "draws": n * K, "exact": a.exact,
           "targets": f"{a.normal:g} * N(0,1)" if a.normal > 0.0 else f"uniform [0, {a.q:g})",
           "max_abs_z": int(z.abs().max()), "bound_draws_median_max": [float(bd.median()), float(bd.max())],
           "warmup": a.warmup, "reps": a.reps, "device": ci.device_info()["name"],
           "acceptance": float(acc.sum()) / (n * T_steps) if T_steps else 0.0,
           "accept_resolved_per_call": ci.counter(_capi.LGS_COUNTER_ACCEPT_RESOLVED) / (calls + 2),
           "wl_mismatch": ci.counter(_capi.LGS_COUNTER_WL_MISMATCH),
           "decisions_resolved_per_call": {k: c.counter(_capi.LGS_COUNTER_RESOLVED) // (calls + 2 * (k == "imhk"))
                                           for k, c in ctxs.items()}}
    for name, rs in recs.items():
        res[name] = {k: stats([r[k] for r in rs]) for k in rs[0]}
    ki, kd = res["imhk"]["klein"][0], res["decode"]["klein"][0]
    res["klein_ratio_imhk_over_decode"] = round(ki / kd, 4) if kd else None
    res["scan_share_of_call"] = round(res["imhk"]["scan_or_select_gather"][0] / res["imhk"]["whole"][0], 4)
    res["scan_over_klein"] = round(res["imhk"]["scan_or_select_gather"][0] / ki, 4) if ki else None

    # the earlier route: a basis upload and a one-chain lgs_imhk per target
    m = min(a.legacy, n)
    if m > 0:
        Th = T[:, :m].t().contiguous().cpu().numpy()
        cps = Th @ Q
        c = _capi.Context(0)
        per = []
        zl = np.zeros((m, d), dtype=np.int64)
        for k in range(m + 1):  # target 0 once more first: warm-up, not counted
            j = max(k - 1, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.set_basis(R, cps[j], B, sigma)
            zs = np.zeros((1, d), dtype=np.int32)
            lw, init, ac = np.zeros(1), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
            c.imhk(1, j, 1, 1, T_steps, 1, zs, lw, init, ac, flags=_capi.LGS_WANG_LING)
            if k > 0:
                per.append((time.perf_counter() - t0) * 1e3)
                zl[j] = zs[0]
        same = int((torch.as_tensor(zl, **dev).t() == z[:, :m]).all(dim=0).sum())
        res["legacy"] = {"targets": m, "ms_per_target": stats(per), "same_final_states": same,
                         "extrapolated_ms_for_n": round(statistics.median(per) * n, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
