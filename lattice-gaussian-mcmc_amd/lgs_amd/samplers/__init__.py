"""Samplers for lattice Gaussian distributions -- same exports as the reference's
``src/samplers/__init__.py:3-5``, plus the exact table sampler."""
from .base import DiscreteGaussianSampler, SamplingStats
from .klein import RefinedKleinSampler as KleinSampler
from .klein import RefinedKleinSampler, klein_bases
from .imhk import IMHKSampler, imhk_bases
from .exact import ExactSampler

__all__ = ["DiscreteGaussianSampler", "KleinSampler", "IMHKSampler", "RefinedKleinSampler",
           "SamplingStats", "ExactSampler", "klein_bases", "imhk_bases"]
