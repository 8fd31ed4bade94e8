"""Klein sampler drop-in -- the reference's ``RefinedKleinSampler``
(``src/samplers/klein.py:21-354``), exported as ``KleinSampler``.

Host side (this file): the QR set-up of ``_precompute_qr_stable``
(klein.py:56-79, NumPy LAPACK, identical to the reference), parameter
validation and bookkeeping.  Device side (``liblgs_hip.so``): every coordinate
draw, the back-substitution, ``basis @ x`` and the log-density.  There is no CPU
sampling path; without a HIP device the constructor raises ``LgsError``.

Randomness: NumPy's global MT19937 stream is replaced by a Philox counter
stream keyed by ``seed``.  When ``seed`` is None it is drawn once from
``np.random`` at construction, so ``np.random.seed(k)`` still makes runs
reproducible, as in the reference's tests.  Sample ``s`` of a sampler always
uses counters (chain = s mod 2^32, step = s >> 32), so results do not depend
on how calls are batched.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, Optional

import numpy as np

from .. import _capi
from .base import DiscreteGaussianSampler

logger = logging.getLogger(__name__)


def _default_seed() -> int:
    return int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))


class RefinedKleinSampler(DiscreteGaussianSampler):
    """Klein's randomized nearest-plane sampler on MI355X (klein.py:21-54)."""

    def __init__(self, lattice, sigma: float, center: Optional[np.ndarray] = None,
                 precision: int = 10, use_log_space: bool = True, *, seed: Optional[int] = None,
                 device: int = 0, exact_order: bool = False, context: Optional[_capi.Context] = None):
        super().__init__(lattice, sigma, center)
        self.precision = precision
        self.use_log_space = use_log_space
        self.exact_order = exact_order
        self.seed = _default_seed() if seed is None else int(seed)
        self._next_sample = 0
        self._precompute_qr_stable()
        # the reference's approximate table cache does not exist here: every
        # draw uses the exact table of its own mean
        self._sample_cache: Dict = {}
        self._max_cache_size = 10000
        self._validate_klein_parameters()
        self._log_2pi = np.log(2 * np.pi)
        self._log_sigma = np.log(self.sigma)
        self._ctx = context if context is not None else _capi.Context(device)
        self._upload(self.precision)

    # ------------------------------------------------------------ set-up
    def _precompute_qr_stable(self):
        """klein.py:56-79: full QR, sign fix (R_ii > 0), c' = Q^T c."""
        self.Q, self.R = np.linalg.qr(self.lattice.basis, mode="full")
        self.P = np.arange(self.dimension)
        condition_number = np.linalg.cond(self.R)
        if condition_number > 1e10:
            logger.warning(f"Poorly conditioned basis: condition number = {condition_number:.2e}")
        for i in range(self.dimension):
            if self.R[i, i] < 0:
                self.R[i, :] *= -1
                self.Q[:, i] *= -1
        self.center_transformed = self.Q.T @ self.center
        self.R_diag = np.diag(self.R)
        self.log_R_diag = np.log(np.abs(self.R_diag) + 1e-300)

    def _validate_klein_parameters(self):
        """klein.py:81-99 (warnings only)."""
        min_gs_norm = self.lattice.min_gram_schmidt_norm
        klein_lower = min_gs_norm / np.sqrt(2 * np.log(self.dimension + 1))
        theoretical_optimal = min_gs_norm / (2 * np.sqrt(np.pi))
        if self.sigma < klein_lower * 0.9:
            logger.warning(f"σ={self.sigma:.4f} is below Klein's requirement "
                           f"(minimum ≈ {klein_lower:.4f}). Sampling may fail.")
        if theoretical_optimal * 0.8 <= self.sigma <= theoretical_optimal * 1.2:
            logger.info("σ is near optimal for BDD applications")

    def _upload(self, precision):
        self._ctx.set_basis(self.R, self.center_transformed, self.lattice.basis, self.sigma,
                            precision, linear_probs=not self.use_log_space)
        self._uploaded_precision = precision
        self._decoder_uploaded = False

    @property
    def context(self) -> _capi.Context:
        return self._ctx

    def _flags(self):
        return _capi.LGS_EXACT_ORDER if self.exact_order else 0

    # ------------------------------------------------------------ sampling
    def _draw(self, n: int, want_z=False, want_v=True, want_logw=False, flags=0):
        if self._uploaded_precision != self.precision:
            self._upload(self.precision)
        first = self._next_sample
        self._next_sample += n
        return self._ctx.klein_host(self.seed, first, n, want_z=want_z, want_v=want_v,
                                    want_logw=want_logw, flags=self._flags() | flags)

    def sample_single(self) -> np.ndarray:
        """One lattice point (klein.py:181-220)."""
        return self._draw(1)["v"][0]

    def sample_coefficients(self, num_samples: int = 1) -> np.ndarray:
        """Integer coefficient vectors, straight from the device (no lstsq needed)."""
        return self._draw(num_samples, want_z=True, want_v=False)["z"].astype(int)

    def sample_with_coefficients(self, num_samples: int = 1):
        """(lattice points, coefficients) of the same draws."""
        r = self._draw(num_samples, want_z=True, want_v=True)
        return r["v"], r["z"].astype(int)

    def parallel_sample_batch(self, num_samples: int, batch_size: int = 100) -> np.ndarray:
        """klein.py:304-322; the whole batch is one device launch (batch_size is moot)."""
        return self._draw(num_samples)["v"]

    def sample(self, num_samples: int = 1) -> np.ndarray:
        """(num_samples, dimension) lattice points (klein.py:324-337)."""
        if num_samples == 1:
            return self.sample_single().reshape(1, -1)
        return self.parallel_sample_batch(num_samples)

    def sample_around(self, targets, coefficients: bool = False):
        """One lattice point near each target: sample k is a draw of D_{L,sigma,t_k}
        (klein.py:181-220 with the centre of base.py taken per sample instead of per
        sampler) -- GPV preimage batches, randomized decoding.  A (d,) target gives a
        (d,) point, (n, d) targets give (n, d); with coefficients=True returns
        (points, z).  The draws use the sampler's next n sample counters, so they
        never share one with sample()."""
        t = np.asarray(targets, dtype=np.float64)
        single = t.ndim == 1
        if single:
            t = t[None, :]
        if t.ndim != 2 or t.shape[1] != self.dimension:
            raise ValueError(f"targets must be ({self.dimension},) or (n, {self.dimension}), got {np.shape(targets)}")
        n = t.shape[0]
        if n == 0:
            z0 = np.zeros((0, self.dimension), dtype=int)
            return (np.zeros((0, self.dimension)), z0) if coefficients else np.zeros((0, self.dimension))
        if self._uploaded_precision != self.precision:
            self._upload(self.precision)
        if not self._decoder_uploaded:
            self._ctx.set_decoder(Q=self.Q)
            self._decoder_uploaded = True
        first = self._next_sample
        self._next_sample += n
        r = self._ctx.klein_targets_host(self.seed, first, t, want_z=coefficients, want_v=True,
                                         flags=self._flags())
        v = r["v"][0] if single else r["v"]
        if not coefficients:
            return v
        z = r["z"].astype(int)
        return v, (z[0] if single else z)

    def decode_around(self, targets, n_draws: int, coefficients: bool = False):
        """Decoding by sampling (Klein 2000): for each target the closest of ``n_draws``
        draws of D_{L,sigma,t} -- the draws ``sample_around`` would return for the target
        repeated ``n_draws`` times, selected on the device (``lgs_klein_decode``: c' once
        per target, only the winners leave the device).  A (d,) target gives a (d,)
        point, (n, d) targets give (n, d); with coefficients=True returns (points, z).
        Consumes the sampler's next n * n_draws sample counters."""
        t = np.asarray(targets, dtype=np.float64)
        single = t.ndim == 1
        if single:
            t = t[None, :]
        if t.ndim != 2 or t.shape[1] != self.dimension:
            raise ValueError(f"targets must be ({self.dimension},) or (n, {self.dimension}), got {np.shape(targets)}")
        if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or n_draws < 1:
            raise ValueError(f"n_draws must be a positive integer, got {n_draws!r}")
        n, K = t.shape[0], int(n_draws)
        if n == 0:
            z0 = np.zeros((0, self.dimension), dtype=int)
            return (np.zeros((0, self.dimension)), z0) if coefficients else np.zeros((0, self.dimension))
        if self._uploaded_precision != self.precision:
            self._upload(self.precision)
        if not self._decoder_uploaded:
            self._ctx.set_decoder(Q=self.Q)
            self._decoder_uploaded = True
        first = self._next_sample
        self._next_sample += n * K
        r = self._ctx.klein_decode_host(self.seed, first, t, K, want_z=coefficients, want_v=True,
                                        flags=self._flags())
        v = r["v"][0] if single else r["v"]
        if not coefficients:
            return v
        z = r["z"].astype(int)
        return v, (z[0] if single else z)

    def adaptive_precision_sample(self, target_distance: Optional[float] = None) -> np.ndarray:
        """klein.py:273-302."""
        if target_distance is None:
            return self.sample_single()
        old_precision = self.precision
        relative_distance = target_distance / self.sigma
        if relative_distance < 1:
            self.precision = max(20, 2 * old_precision)
        elif relative_distance > 5:
            self.precision = max(5, old_precision // 2)
        try:
            sample = self.sample_single()
        finally:
            self.precision = old_precision
        return sample

    # ------------------------------------------------------------ densities
    def _coefficients_of(self, lattice_point):
        try:
            coeffs = np.linalg.solve(self.lattice.basis, lattice_point)
            coeffs_int = np.round(coeffs).astype(np.int64)
            err = np.linalg.norm(self.lattice.basis @ coeffs_int - lattice_point)
            if err > 1e-10:
                return None
        except np.linalg.LinAlgError:
            return None
        return coeffs_int

    def compute_log_density(self, lattice_point: np.ndarray) -> float:
        """log q(v) of Klein's proposal (klein.py:222-271), evaluated on the device."""
        z = self._coefficients_of(np.asarray(lattice_point, dtype=np.float64))
        if z is None:
            return -np.inf
        if self._uploaded_precision != self.precision:
            self._upload(self.precision)
        return float(self._ctx.log_density(z[None, :])[0])

    def diagnostic_info(self) -> Dict[str, Any]:
        """klein.py:339-354."""
        return {
            "algorithm": "Refined Klein",
            "sigma": self.sigma,
            "precision": self.precision,
            "use_log_space": self.use_log_space,
            "cache_size": len(self._sample_cache),
            "condition_number": np.linalg.cond(self.R),
            "min_R_diag": np.min(np.abs(self.R_diag)),
            "max_R_diag": np.max(np.abs(self.R_diag)),
            "min_conditional_sigma": self.sigma / np.max(np.abs(self.R_diag)),
            "max_conditional_sigma": self.sigma / np.min(np.abs(self.R_diag)),
            "device": self._ctx.device_info()["name"],
            "seed": self.seed,
        }


KleinSampler = RefinedKleinSampler


def _bases_inputs(name, bases, targets, sigma, n_draws, rows):
    """The checks ``klein_bases`` and ``decode.sampling_decode_bases`` share, before any library
    call: returns (columns (n, d, d), targets (n, T, d) float64, sigma (n,) float64, single)."""
    b = np.asarray(bases)
    if b.ndim != 3 or b.shape[1] != b.shape[2]:
        raise ValueError(f"bases must have shape (n, d, d), got {b.shape}")
    if b.dtype.kind not in "iuf":
        raise ValueError(f"bases must be real, got dtype {b.dtype}")
    n, d = b.shape[0], b.shape[1]
    if not 2 <= d <= _capi.LGS_CVP_MAX_D:
        raise ValueError(f"{name} supports 2 <= d <= {_capi.LGS_CVP_MAX_D}, got d = {d}")
    single = targets is None
    if targets is None:
        t3 = np.zeros((n, 1, d))
    else:
        t = np.asarray(targets)
        if t.dtype.kind not in "iuf":
            raise ValueError(f"targets must be real, got dtype {t.dtype}")
        t = t.astype(np.float64, copy=False)
        single = t.ndim == 2
        t3 = t[:, None, :] if single else t
        if t3.ndim != 3 or t3.shape[0] != n or t3.shape[2] != d:
            raise ValueError(f"targets must have shape ({n}, T, {d}) or ({n}, {d}), got {t.shape}")
    T = t3.shape[1]
    if not 1 <= T <= _capi.LGS_KLEINB_MAX_T:
        raise ValueError(f"{name} supports 1 <= T <= {_capi.LGS_KLEINB_MAX_T} targets per basis, got {T}")
    if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or n_draws < 1 or \
            T * int(n_draws) > 1 << 22:
        raise ValueError(f"n_draws must be a positive integer with T * n_draws <= 2^22, got {n_draws!r}")
    s = np.asarray(sigma)
    if s.dtype.kind not in "iuf" or s.ndim > 1 or (s.ndim == 1 and s.shape != (n,)):
        raise ValueError(f"sigma must be a real scalar or an array of shape ({n},), got {sigma!r}")
    s = np.ascontiguousarray(np.broadcast_to(s.astype(np.float64), (n,)))
    if not np.all((s > 0) & np.isfinite(s)):
        raise ValueError("sigma must be positive and finite")
    cols = np.swapaxes(b, 1, 2) if rows else b
    return cols, np.ascontiguousarray(t3, dtype=np.float64), s, single


def klein_bases(bases, sigma, targets=None, n_draws: int = 1, seed: int = 0, first_sample: int = 0,
                rows: bool = False, coefficients: bool = False, device: int = 0):
    """Klein draws in many small lattices at once (``lgs_klein_bases``): ``bases`` (n, d, d),
    2 <= d <= 64, ``sigma`` a scalar or one width per basis, ``targets`` (n, T, d), T <= 64, and
    ``n_draws`` = K draws of D_{L_p, sigma_p, t_{p,k}} around each.  The columns of ``bases[p]``
    generate lattice p; with ``rows=True`` its rows do (``decode.closest_vector_bases``'
    convention).  The QR factorisation and every draw run on the device; no basis is loaded into
    a context.  Draw j of target k of basis p is Klein sample ``first_sample + (p T + k) K + j``
    of ``seed``, whatever the batch.

    Returns the lattice points, shape (n, T, K, d) -- B z of the device's coefficients, formed
    here -- or ``(points, z)`` with ``coefficients=True`` (int64).  ``targets=None`` means one
    zero target per basis, and (n, d) targets one target each: the T axis is then dropped.  A
    basis the QR refuses (a column norm not in (0, inf)) is a ValueError."""
    from ..decode import _bases_context
    cols, t3, s, single = _bases_inputs("klein_bases", bases, targets, sigma, n_draws, rows)
    colsf = np.ascontiguousarray(cols, dtype=np.float64)
    r = _bases_context(device).klein_bases_host(seed, first_sample, colsf, t3, s, int(n_draws), want_z=False,
                                                want_v=False, want_R=False, want_draws=True)
    if r["qr_status"].any():
        raise ValueError(f"bases {np.flatnonzero(r['qr_status']).tolist()} are singular")
    z = r["z_draws"]
    v = np.einsum("nij,ntkj->ntki", colsf, z.astype(np.float64))
    if single:
        v, z = v[:, 0], z[:, 0]
    return (v, z) if coefficients else v
