"""
gadfly_amd -- MI355X-native implementation of gadfly's GP hot path.

Public names follow /root/reference/gadfly/__init__.py:3-6 (``core`` and ``gp`` re-exported).
Importing the package needs neither a GPU nor the built HIP library; the first compute
call does, and fails loudly without them (no CPU fallback).
"""
from .core import (  # noqa: F401
    Hyperparameters, StellarOscillatorKernel, SolarOscillatorKernel,
    ShotNoiseKernel, Filter,
)
from . import scale  # noqa: F401
from .gp import GaussianProcess, ConditionalDistribution, LinAlgError  # noqa: F401
from .batch import (BatchedLogLikelihood, log_likelihood_batch, BatchedSampler, sample_batch,  # noqa: F401
                    predict_batch, sample_conditional_batch)
from . import terms  # noqa: F401
from .psd import PowerSpectrum, bin_power_spectrum  # noqa: F401
from .interp import interpolate_missing_data, interpolate_missing_data_batch, stitch_quarters  # noqa: F401
from .detrend import prepare_quarters, prepare_quarters_batch  # noqa: F401
from .linmodel import fit_linear_batch, quarter_polynomial_basis  # noqa: F401
from . import spectral  # noqa: F401
from . import conddraw  # noqa: F401
from .spectral import SpectralLikelihood  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # torch.autograd.Function over BatchedLogLikelihood.value_and_grad (gadfly_amd.grad); imported on first use
    if name == "LogLikelihood":
        from .grad import LogLikelihood
        return LogLikelihood
    # torch.autograd.Function over BatchedLogLikelihood.linear_value_and_grad (gadfly_amd.grad); imported on first use
    if name == "LinearModelLogLikelihood":
        from .grad import LinearModelLogLikelihood
        return LinearModelLogLikelihood
    # torch.autograd.Function over SpectralLikelihood.value_and_grad (gadfly_amd.spectral); imported on first use
    if name == "SpectralLogLikelihood":
        return spectral.SpectralLogLikelihood
    raise AttributeError(f"module 'gadfly_amd' has no attribute {name!r}")
