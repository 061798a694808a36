"""Host side of the long scaling span: the block-scaled recurrence restated in numpy with the
streamed sweep's reset rule and span, against the C oracle; the library's spans; the host block rule."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd import _lib
from gadfly_amd.engine import StreamingBatch, _scaled_span
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times
from oracle import cref

_CAD = float(np.diff(uniform_times(2, 60.0))[0])         # 60 s in the time unit of the API


def _scaled_loglike(coeffs, t, diag, y, block, span):
    """The recurrence k_factor7 runs in scaled coordinates, with resets at multiples of `block`
    and where c_max (t_n - t_{n-1}) > span / (block - 1)."""
    c, a, U, V = cref.get_matrices(coeffs, t, diag)
    N, W = U.shape
    cmax = float(c.max())
    gap = span / (block - 1) if block > 1 else 0.0
    T, F = np.zeros((W, W)), np.zeros(W)
    w_prev, d_prev, z_prev, tref = np.zeros(W), 0.0, 0.0, t[0]
    ll, big, small = 0.0, 0.0, np.inf
    for n in range(N):
        reset = n % block == 0 or cmax * (t[n] - t[n - 1]) > gap
        T += d_prev * np.outer(w_prev, w_prev)
        F += w_prev * z_prev
        if reset:
            E = np.exp(-c * (t[n] - tref))
            T, F, tref = E[:, None] * T * E[None, :], E * F, t[n]
        rho = np.exp(-c * (t[n] - tref))
        u, v = U[n] * rho, V[n] / rho
        tmp = T @ u
        d = a[n] - u @ tmp
        z = y[n] - u @ F
        assert d > 0.0
        w_prev, d_prev, z_prev = (v - tmp) / d, d, z
        ll -= 0.5 * (z * z / d + np.log(d))
        big = max(big, np.abs(T).max(), np.abs(F).max(), np.abs(v).max(), np.abs(w_prev).max())
        small = min(small, np.abs(u[u != 0.0]).min())
    return ll - 0.5 * N * np.log(2 * np.pi), big, small


def _coeffs(J, scale=1.0, fast=None):
    co = [np.array(v, dtype=np.float64) if i < 6 else float(v) for i, v in enumerate(
        gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0).get_device_coefficients())]
    if fast is not None:                    # the fastest term as a plain damped cosine (a > 0, b = 0: positive
        k = int(np.argmax(co[4]))           # definite whatever its damping) with c * cadence = fast
        co[2][k], co[3][k], co[4][k] = abs(co[2][k]), 0.0, fast / _CAD
    co[2], co[3] = co[2] * scale, co[3] * scale
    return tuple(co[:6]), co[6] * scale


def test_library_spans():
    assert _scaled_span(False) == 28.0 and _scaled_span(True) == 128.0
    assert _lib.GF_SWEEP_LONG_SPAN == 0x200


def test_block_rule_bench_hyperparameters():
    (coeffs, _), cad = _coeffs(30), _CAD
    x = 1.5 * float(np.max(coeffs[4])) * cad
    assert 1.0 < float(np.max(coeffs[4])) * cad < 1.05          # the one fast term of the flagship workload
    assert StreamingBatch._scaling_block(x, _scaled_span(False)) == 16
    assert StreamingBatch._scaling_block(x, _scaled_span(True)) == 64


class _W:
    W = 60
    LONG_SPAN_AMPLITUDE = StreamingBatch.LONG_SPAN_AMPLITUDE


@pytest.mark.parametrize("scale,ok", [(1.0, True), (1e-90, True), (1e90, True), (1e-120, False), (1e120, False)])
def test_long_span_amplitude_guard(scale, ok):
    coeffs, _ = _coeffs(30, scale=scale)
    real = np.zeros((2, 1, 0))
    comp = np.stack([coeffs[2], coeffs[3], coeffs[4], coeffs[5]])[:, None, :]
    assert StreamingBatch._long_span_ok(_W(), real, comp, np.array([scale])) is ok
    wide = _W()
    wide.W = 80
    assert StreamingBatch._long_span_ok(wide, real, comp, np.array([1.0])) is False


def _compare(coeffs, t, diag, y, block, span=128.0):
    ref, info = cref.loglike(coeffs, t, diag, y)
    assert info == 0
    ll, big, small = _scaled_loglike(coeffs, t, diag, y, block, span)
    assert abs(ll - ref) <= 1e-10 * abs(ref), (ll, ref)
    return big, small


@pytest.mark.parametrize("fast", [1.0, 2.0, 3.0])
def test_scaled_recurrence_fast_term_block64(fast):
    N = 1500
    t = uniform_times(N, 60.0)
    y = 100.0 * np.random.Generator(np.random.PCG64(1)).normal(size=N)
    coeffs, shift = _coeffs(12, fast=fast)
    _compare(coeffs, t, np.full(N, 900.0) + shift, y, 64)


def test_scaled_recurrence_gap_block64():
    N = 1500
    t = uniform_times(N, 60.0)
    t[700:] += 3000 * _CAD                  # a gap of 3000 cadences
    rng = np.random.Generator(np.random.PCG64(2))
    coeffs, shift = _coeffs(12)
    _compare(coeffs, t, np.full(N, 900.0) + shift, 100.0 * rng.normal(size=N), 64)


@pytest.mark.parametrize("scale", [1e-100, 1e100])
def test_scaled_recurrence_extreme_amplitudes(scale):
    """Amplitudes (and the diagonal) at the edge of the accepted range: the scaled magnitudes stay inside FP64."""
    N = 1500
    t = uniform_times(N, 60.0)
    rng = np.random.Generator(np.random.PCG64(3))
    coeffs, shift = _coeffs(12, scale=scale, fast=1.0)
    big, small = _compare(coeffs, t, np.full(N, 900.0 * scale) + shift, np.sqrt(scale) * 100.0 * rng.normal(size=N), 64)
    assert big < 1e250 and small > 1e-250
