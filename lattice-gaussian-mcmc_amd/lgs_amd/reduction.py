"""LLL and BKZ basis reduction on the GPU (``lgs_lll_reduce``, ``lgs_bkz_reduce``).

The enumeration entry points (``closest_vector``, ``gaussian_mass``, ``ball_points``, the exact
sampler) stop at a node budget, and on the raw q-ary / NTRU bases of ``lgs_amd.lattices`` that
budget is what they hit: their shortest row is as long as q.  ``lll_reduce`` is the remedy the
reference takes from Sage (``src/lattices/reduction.py:68-186``), here one wave per basis and
whole batches per call, with the transformation returned as exact integers.

``bkz_reduce`` goes on where LLL stops (``src/lattices/reduction.py:238-318``): the Gram-Schmidt
profile, which sets the size of those trees and the smallest sigma at which Klein and IMHK are
close to their target, improves only with block reduction.

``LatticeReduction`` restates the reference's host-side quality measures (Hermite factor,
orthogonality defect, Gram-Schmidt profile) in NumPy around that reduction.
"""
from __future__ import annotations

import math
import time

import numpy as np

from . import _capi

_ctx = {}


def _context(device: int):
    if device not in _ctx:
        _ctx[device] = _capi.Context(device)
    return _ctx[device]


def _integral(basis):
    """``basis`` as an int64 array; ValueError when an entry is not an integer below 2^28."""
    a = np.asarray(basis)
    if a.dtype.kind in "iu":
        b = a.astype(np.int64)
    elif a.dtype.kind == "f":
        if not np.all(np.isfinite(a)) or np.any(a != np.rint(a)):
            raise ValueError("lll_reduce takes an integral basis (real and rational bases are not supported)")
        if np.any(np.abs(a) >= float(1 << 28)):
            raise ValueError("basis entries must be below 2^28 in magnitude")
        b = a.astype(np.int64)
    else:
        raise ValueError(f"lll_reduce takes an integral basis, got dtype {a.dtype}")
    if np.any(np.abs(b) >= 1 << 28):
        raise ValueError("basis entries must be below 2^28 in magnitude")
    return b


def lll_reduce(basis, delta: float = 0.99, eta: float = 0.51, max_iters: int = 1 << 40, rows: bool = True,
               device: int = 0):
    """LLL-reduce one (d, d) basis or a batch (n, d, d) of integral bases, 2 <= d <= 64.

    With ``rows=True`` (the reference's convention, ``reduction.py:153-158``) the lattice vectors
    are the rows and ``reduced = U @ basis``; with ``rows=False`` they are the columns, the
    C-ABI's convention, and ``reduced = basis @ U``.  Returns ``(reduced, U, info)``: int64
    arrays of the input's shape and a dict of per-basis ``swaps``, ``iters``, ``passes``,
    ``status`` (0 = reduced, 1 = ``max_iters`` reached, 2 = a magnitude guard stopped the
    reduction, 3 = the input is not a basis) and ``gs_norm2`` (the squared Gram-Schmidt norms the
    reduction ended with); scalars, and a (d,) array, for a single basis.  With any status the
    result is a basis of the same lattice and ``U`` is consistent with it."""
    b = _integral(basis)
    single = b.ndim == 2
    if b.ndim not in (2, 3) or b.shape[-1] != b.shape[-2]:
        raise ValueError(f"basis must have shape (d, d) or (n, d, d), got {b.shape}")
    b3 = b[None] if single else b
    cols = np.ascontiguousarray(np.swapaxes(b3, 1, 2) if rows else b3)
    r = _context(device).lll_reduce_host(cols, delta, eta, max_iters)
    red, U = r["basis"], r["U"]
    if rows:
        red, U = np.ascontiguousarray(np.swapaxes(red, 1, 2)), np.ascontiguousarray(np.swapaxes(U, 1, 2))
    info = {k: r[k] for k in ("swaps", "iters", "passes", "status", "gs_norm2")}
    if single:
        return red[0], U[0], {k: (v[0] if v.ndim > 1 else v[0].item()) for k, v in info.items()}
    return red, U, info


_BKZ_INFO = ("swaps", "iters", "passes", "tours", "blocks", "insertions", "nodes", "truncated", "status", "gs_norm2")


def bkz_reduce(basis, block_size: int, delta: float = 0.99, eta: float = 0.51, max_tours: int = 1024,
               enum_nodes: int = 1 << 30, max_iters: int = 1 << 40, rows: bool = True, device: int = 0):
    """BKZ-reduce one (d, d) basis or a batch (n, d, d) of integral bases, 2 <= d <= 64, with
    blocks of ``block_size`` (2..32) vectors.

    Conventions and the shape of the result are ``lll_reduce``'s: ``(reduced, U, info)`` with
    ``reduced = U @ basis`` for ``rows=True``.  ``info`` holds the LLL counters summed over the
    call, ``tours``, ``blocks``, ``insertions``, ``nodes``, ``truncated`` (block enumerations cut
    at ``enum_nodes`` nodes), ``gs_norm2`` and ``status``: 0 = a whole tour made no insertion,
    1 = ``max_iters`` reached, 2 = a magnitude guard stopped the reduction, 3 = the input is not
    a basis, 4 = ``max_tours`` tours done.  Status 0 means BKZ-reduced only with ``truncated == 0``.
    With any status the result is a basis of the same lattice and ``U`` is consistent with it."""
    b = _integral(basis)
    single = b.ndim == 2
    if b.ndim not in (2, 3) or b.shape[-1] != b.shape[-2]:
        raise ValueError(f"basis must have shape (d, d) or (n, d, d), got {b.shape}")
    b3 = b[None] if single else b
    cols = np.ascontiguousarray(np.swapaxes(b3, 1, 2) if rows else b3)
    r = _context(device).bkz_reduce_host(cols, block_size, delta, eta, max_tours, max_iters, enum_nodes)
    red, U = r["basis"], r["U"]
    if rows:
        red, U = np.ascontiguousarray(np.swapaxes(red, 1, 2)), np.ascontiguousarray(np.swapaxes(U, 1, 2))
    info = {k: r[k] for k in _BKZ_INFO}
    if single:
        return red[0], U[0], {k: (v[0] if v.ndim > 1 else v[0].item()) for k, v in info.items()}
    return red, U, info


def _gs_norms(B):
    """Gram-Schmidt norms of the rows of B (float64)."""
    return np.abs(np.diag(np.linalg.qr(np.asarray(B, dtype=np.float64).T, mode="r")))


class LatticeReduction:
    """The reference's ``LatticeReduction`` (``src/lattices/reduction.py``) without Sage: the
    reduction runs on the GPU, the quality measures are NumPy.  Bases hold the lattice vectors
    in their rows."""

    def __init__(self, device: int = 0):
        self.device = device
        self.stats = {"reductions_performed": 0, "total_time": 0.0, "quality_improvements": []}

    def lll_reduce(self, basis, delta: float = 0.75):
        """(reduced, U, diagnostics) with reduced = U @ basis (``reduction.py:68-133``);
        diagnostics holds time, initial_quality, final_quality, improvement_factor, delta, and
        the reduction's own counters under ``lll``."""
        t0 = time.time()
        before = self.basis_quality_profile(basis)
        red, U, info = lll_reduce(basis, delta=delta, rows=True, device=self.device)
        if np.any(np.asarray(info["status"]) != 0):
            raise RuntimeError(f"LLL did not finish: status {info['status']}")
        after = self.basis_quality_profile(red)
        dt = time.time() - t0
        diag = {"time": dt, "initial_quality": before, "final_quality": after,
                "improvement_factor": before["hermite_factor"] / after["hermite_factor"], "delta": delta,
                "lll": info}
        self.stats["reductions_performed"] += 1
        self.stats["total_time"] += dt
        self.stats["quality_improvements"].append(diag["improvement_factor"])
        return red.astype(np.float64), U.astype(np.float64), diag

    @staticmethod
    def _progressive_block_sizes(n: int, target: int):
        """min(20, n), +10, ..., target (``reduction.py:302-312``)."""
        sizes, beta = [], min(20, n)
        while beta < target:
            sizes.append(beta)
            beta = min(beta + 10, target)
        sizes.append(target)
        return sizes

    def bkz_reduce(self, basis, block_size: int, strategy: str = "default", progressive: bool = False):
        """(reduced, U, diagnostics) with reduced = U @ basis (``reduction.py:238-300``);
        diagnostics holds the reference's keys -- time, block_size, block_sizes_used, strategy,
        initial_quality, final_quality, improvement_factor -- and the counters of every run under
        ``bkz``.  ``progressive`` runs the block sizes min(20, n), +10, ..., block_size in turn,
        each capped at 32, and composes the transformations exactly.  Only the default strategy
        exists; a run that does not end with status 0, or that cut an enumeration short, raises."""
        if strategy != "default":
            raise ValueError(f"bkz_reduce: unknown strategy {strategy!r} (only 'default')")
        t0 = time.time()
        before = self.basis_quality_profile(basis)
        n = np.asarray(basis).shape[0]
        sizes = self._progressive_block_sizes(n, block_size) if progressive else [block_size]
        sizes = [min(int(b), _capi.LGS_BKZ_MAX_BLOCK) for b in sizes]
        red, U, runs = basis, None, []
        for beta in sizes:
            red, Ub, info = bkz_reduce(red, beta, rows=True, device=self.device)
            if np.any(np.asarray(info["status"]) != 0) or np.any(np.asarray(info["truncated"]) != 0):
                raise RuntimeError(f"BKZ-{beta} did not finish: status {info['status']}, "
                                   f"truncated {info['truncated']}")
            # python ints: the product of two transformations may pass 2^63 where each fits
            U = Ub if U is None else np.array(Ub.astype(object) @ U.astype(object), dtype=np.int64)
            runs.append(info)
        after = self.basis_quality_profile(red)
        dt = time.time() - t0
        diag = {"time": dt, "block_size": block_size, "block_sizes_used": sizes, "strategy": strategy,
                "initial_quality": before, "final_quality": after,
                "improvement_factor": before["hermite_factor"] / after["hermite_factor"], "bkz": runs}
        self.stats["reductions_performed"] += 1
        self.stats["total_time"] += dt
        self.stats["quality_improvements"].append(diag["improvement_factor"])
        return red.astype(np.float64), U.astype(np.float64), diag

    @staticmethod
    def hermite_factor(basis) -> float:
        """||b_1|| / det(L)^(1/n) (``reduction.py:322-346``); the determinant through its log."""
        B = np.asarray(basis, dtype=np.float64)
        n = B.shape[0]
        _, logdet = np.linalg.slogdet(B)
        return float(np.linalg.norm(B[0]) / math.exp(logdet / n))

    @staticmethod
    def orthogonality_defect(basis) -> float:
        """prod ||b_i|| / |det| (``reduction.py:348-371``), formed in logs."""
        B = np.asarray(basis, dtype=np.float64)
        _, logdet = np.linalg.slogdet(B)
        return float(math.exp(float(np.sum(np.log(np.linalg.norm(B, axis=1)))) - logdet))

    def basis_quality_profile(self, basis) -> dict:
        """The keys of ``reduction.py:394-403``."""
        B = np.asarray(basis, dtype=np.float64)
        gs = _gs_norms(B)
        return {"dimension": int(B.shape[0]), "hermite_factor": self.hermite_factor(B),
                "orthogonality_defect": self.orthogonality_defect(B), "gs_norms": [float(x) for x in gs],
                "max_gs_norm": float(gs.max()), "min_gs_norm": float(gs.min()),
                "gs_ratio": float(gs.max() / gs.min()), "log_potential": float(np.sum(np.log(gs)))}
