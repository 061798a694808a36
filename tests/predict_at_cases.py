"""Walkers of tests/test_gpu_predict_at_batch.py: B proposals around the solar-like kernel as exposure-integrated
SHO sums, their components, and the float64 oracle of one of them (oracle/seq.py through tests/solve_ref.py)."""
import functools

import numpy as np

import gadfly_amd
from gadfly_amd.synth import solar_like_hyperparameters
from gadfly_amd.terms import SHOTerm, TermConvolution, TermSum
from tests.solve_ref import oracle_predict

J, YERR = 30, 30.0


@functools.lru_cache(maxsize=None)
def walkers(b=5, j=J, seed=3):
    """(S0, w0, Q (b, j), delta): proposals around the solar-like kernel's own parameters (Q untouched)."""
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(j), texp=60.0)
    S0, w0, Q = (np.array([[getattr(tm, k) for tm in kern.term.terms]]) for k in ("S0", "w0", "Q"))
    rng = np.random.default_rng(seed)
    S0, w0 = (np.repeat(x, b, axis=0) * np.exp(0.05 * rng.normal(size=(b, j))) for x in (S0, w0))
    return S0, w0, np.repeat(Q, b, axis=0), float(kern.delta)


def kernels(S0, w0, Q, delta, first=None):
    """Exposure-integrated SHO sums of (B, J) parameters; ``first``: only the first so many terms (a component)."""
    return [TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q))
                                      for s, w, q in list(zip(*r))[:first]]), delta) for r in zip(S0, w0, Q)]


def oracle_alpha(kern, t, y, diag):
    """alpha = K^-1 y of one kernel from oracle/seq.py in float64."""
    co = kern.get_device_coefficients()
    return oracle_predict(t, y, diag, co[:6], float(np.sum(co[0]) + np.sum(co[2]) + co[6]))["alpha"]
