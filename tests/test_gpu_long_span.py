"""The streamed log-likelihood on the long scaling span (GF_SWEEP_LONG_SPAN) against the oracle:
block 64 with a fast term, a data gap, amplitudes at the edges of the accepted range, and the short-span fall-back."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.engine import StreamingBatch
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times
from oracle import cref

_CAD = float(np.diff(uniform_times(2, 60.0))[0])         # 60 s in the time unit of the API

pytestmark = pytest.mark.gpu


def _coeffs(J, scale=1.0, fast=None):
    co = list(gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0).get_device_coefficients())
    co = [np.array(v, dtype=np.float64) if i < 6 else v for i, v in enumerate(co)]
    if fast is not None:                    # the fastest term as a plain damped cosine (a > 0, b = 0: positive
        k = int(np.argmax(co[4]))           # definite whatever its damping) with c * cadence = fast
        co[2][k], co[3][k], co[4][k] = abs(co[2][k]), 0.0, fast / _CAD
    co[2] = co[2] * scale
    co[3] = co[3] * scale
    return tuple(co[:6]) + (co[6] * scale,)


def _check(co, t, y, diag, block_expected, tol=1e-8):
    eng = StreamingBatch([co, co], t, y, diag=diag)
    eng.generator_period = 1
    assert eng._pack.stream_block == block_expected
    ll = eng.log_likelihood().cpu().numpy()
    ref, info = cref.loglike(co[:6], t, diag + co[6], y)
    assert info == 0
    rel = float(np.max(np.abs(ll - ref)) / abs(ref))
    assert rel < tol, rel
    return eng


@pytest.mark.parametrize("fast", [1.0, 1.5, 3.0])
def test_fast_term_long_span(fast):
    N = 20000
    t = uniform_times(N, 60.0)
    rng = np.random.Generator(np.random.PCG64(7))
    y = 100.0 * rng.normal(size=N)
    block = 64 if 1.5 * 63 * fast <= 128.0 else (32 if 1.5 * 31 * fast <= 128.0 else 16)
    eng = _check(_coeffs(30, fast=fast), t, y, np.full(N, 900.0), block)
    assert eng._pack.block <= 16                 # the other routes keep the short span's block


def test_gap_and_jitter_long_span():
    N = 20000
    t = uniform_times(N, 60.0)
    t[9000:] += 5000 * _CAD                 # a gap of 5000 cadences
    rng = np.random.Generator(np.random.PCG64(8))
    t[1:] += rng.uniform(-1e-3, 1e-3, size=N - 1) * _CAD       # time-stamp jitter of 0.1 % of a cadence
    y = 100.0 * rng.normal(size=N)
    _check(_coeffs(30), t, y, np.full(N, 900.0), 64)


@pytest.mark.parametrize("scale", [1e-90, 1e90])
def test_extreme_amplitudes_long_span(scale):
    N = 8192
    t = uniform_times(N, 60.0)
    rng = np.random.Generator(np.random.PCG64(9))
    y = 100.0 * np.sqrt(scale) * rng.normal(size=N)
    _check(_coeffs(30, scale=scale), t, y, np.full(N, 900.0 * scale), 64)


@pytest.mark.parametrize("scale", [1e-120, 1e120])
def test_out_of_range_amplitudes_fall_back(scale):
    N = 8192
    t = uniform_times(N, 60.0)
    rng = np.random.Generator(np.random.PCG64(10))
    y = 100.0 * np.sqrt(scale) * rng.normal(size=N)
    eng = _check(_coeffs(30, scale=scale), t, y, np.full(N, 900.0 * scale), 0)
    assert eng._pack.block == 16
