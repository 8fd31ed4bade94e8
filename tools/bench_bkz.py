"""Timing of lgs_bkz_reduce for DESIGN.md 6j (its output is profiles/bkz_measure.log): qary_basis(32, 32, 3329), seeds 1..256, d = 64, delta = 0.99,
device pointers, timer 9; beta 12 and 20, batch 1 and 256, two runs each; LLL alone on the same bases beside it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lattice-gaussian-mcmc_amd"))
from lgs_amd import _capi, lattices

dev = torch.device("cuda:0")
ctx = _capi.Context(0)
cols = np.stack([np.ascontiguousarray(lattices.qary_basis(32, 32, 3329, seed=s).T).astype(np.int64) for s in range(1, 257)])
print("device:", torch.cuda.get_device_name(0), flush=True)


def run(n, beta):
    bd = torch.as_tensor(cols[:n], device=dev)
    bo, uo = torch.empty_like(bd), torch.empty_like(bd)
    names = ("swaps", "iters", "passes", "tours", "blocks", "insertions", "nodes", "truncated")
    ctr = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in names}
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.timing_enable(True)
    if beta:
        ctx.bkz_reduce(bd, bo, uo, beta, 0.99, 0.51, 1 << 40, 1 << 40, 1 << 40, *(ctr[k] for k in names), st,
                       flags=_capi.LGS_DEVICE_PTRS)
    else:
        ctx.lll_reduce(bd, bo, uo, 0.99, 0.51, 1 << 40, ctr["swaps"], ctr["iters"], ctr["passes"], st,
                       flags=_capi.LGS_DEVICE_PTRS)
    torch.cuda.synchronize()
    ms, launches = ctx.timing_get(_capi.KERNEL_CVP_ENUM)
    c = {k: v.cpu().numpy() for k, v in ctr.items()}
    n1 = (bo.cpu().numpy()[:, :, 0].astype(object) ** 2).sum(axis=1)
    return ms, launches, c, st.cpu().numpy(), n1


for beta in (0, 12, 20):
    for n in (1, 256):
        for rep in (1, 2):
            ms, launches, c, st, n1 = run(n, beta)
            it, nd = c["iters"], c["nodes"]
            what = f"BKZ-{beta}" if beta else "LLL"
            print(f"{what} batch {n} run {rep}: timer9 {ms:.1f} ms, launches {launches}, status {sorted(set(st.tolist()))}, "
                  f"iters {it.min()}..{it.max()} (sum {it.sum()}), nodes {nd.min()}..{nd.max()} (sum {nd.sum()}), "
                  f"tours {c['tours'].min()}..{c['tours'].max()}, insertions {c['insertions'].min()}..{c['insertions'].max()}, "
                  f"truncated {c['truncated'].sum()}, |b1|^2 of basis 0 {n1[0]}", flush=True)
