"""Host side of the streamed sweep's steady mode: the detection rule and the frozen-gain tail
restated in numpy -- in the kernel's block-scaled coordinates -- on the C oracle's own factor, against the
oracle's log-likelihood."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.core import Hyperparameters
from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters, uniform_times
from oracle import cref

# the kernel's rule (gadfly_hip.hip: ST_GRID, ST_LAG, ST_COUNT, ST_THR): anchors every GRID = 64 rows whatever the
# scaling block, so the lag is 1024 rows and the consecutive span 256 rows at every block
GRID, LAG, COUNT, THR = 64, 16, 4, 1e-10


def _kernel_coeffs(hp):
    co = gadfly_amd.StellarOscillatorKernel(hp, texp=60.0).get_device_coefficients()
    return tuple(np.array(v, dtype=np.float64) for v in co[:6]), float(co[6])


def _two_terms(*terms):
    return Hyperparameters([dict(hyperparameters=dict(S0=float(s), w0=2 * np.pi * float(nu), Q=float(q)),
                                 metadata=dict(source="test")) for s, nu, q in terms], name="two terms")


def _switch_row(t, dc, d, W):
    """First anchor (rows = 0 mod GRID) at which the pivot and the derotated gains have moved by less than THR
    -- the gains relative to the LARGEST gain -- over a lag of LAG anchors, at COUNT consecutive anchors."""
    rows = np.arange(0, len(t), GRID)
    gain = (W[rows, 0::2] + 1j * W[rows, 1::2]) * np.exp(-1j * dc[None, :] * t[rows, None])
    piv = d[rows]
    ok = np.zeros(len(rows), dtype=bool)
    dg = np.abs(gain[LAG:] - gain[:-LAG])
    ok[LAG:] = ((np.maximum(np.abs(dg.real), np.abs(dg.imag)).max(axis=1)
                 <= THR * np.maximum(np.abs(gain[LAG:].real), np.abs(gain[LAG:].imag)).max(axis=1))
                & (np.abs(piv[LAG:] - piv[:-LAG]) <= THR * piv[LAG:]))
    run = 0
    for k, good in enumerate(ok):
        run = run + 1 if good else 0
        if run >= COUNT:
            return int(rows[k]), gain[k], float(piv[k])
    return -1, None, None


def _steady_loglike(coeffs, t, diag, y, block=64):
    """Oracle factor up to the switch row, then the tail the kernel runs: pivot and derotated gains frozen, only
    the forward solve F~ += w~ z, z = y - u~ . F~ with its block decays.  Returns (log-likelihood, switch row)."""
    c, a, U, V = cref.get_matrices(coeffs, t, diag)
    d, W, info = cref.factor(t, c, a, U, V)
    assert info == 0
    dc = np.asarray(coeffs[5])
    sw, gain, dinf = _switch_row(t, dc, d, W)
    N, J = U.shape
    if sw >= 0:                             # rows after the switch row: w = G e^{i d t}, d = d_inf
        ph = gain[None, :] * np.exp(1j * dc[None, :] * t[sw + 1:, None])
        W, d = W.copy(), d.copy()
        W[sw + 1:, 0::2], W[sw + 1:, 1::2] = ph.real, ph.imag
        d[sw + 1:] = dinf
    F, w_prev, z_prev, tref = np.zeros(J), np.zeros(J), 0.0, t[0]
    z = np.empty(N)
    for n in range(N):
        F += w_prev * z_prev
        if n % block == 0:
            F *= np.exp(-c * (t[n] - tref))
            tref = t[n]
        rho = np.exp(-c * (t[n] - tref))
        z[n] = y[n] - (U[n] * rho) @ F
        w_prev, z_prev = W[n] / rho, z[n]
    ll = -0.5 * (np.sum(z * z / d) + np.sum(np.log(d))) - 0.5 * N * np.log(2 * np.pi)
    return ll, sw


def _series(N, seed=12345, cadence=60.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return uniform_times(N, cadence), np.cumsum(rng.normal(size=N)) * 5.0 + 30.0 * rng.normal(size=N)


def _check(hp, N=65536, cadence=60.0, block=64):
    coeffs, shift = _kernel_coeffs(hp)
    t, y = _series(N, cadence=cadence)
    diag = np.full(N, 900.0) + shift
    ref, info = cref.loglike(coeffs, t, diag, y)
    assert info == 0
    ll, sw = _steady_loglike(coeffs, t, diag, y, block)
    print(f"switch row {sw}, relative error {abs(ll - ref) / abs(ref):.2e}")
    assert abs(ll - ref) <= 1e-10 * abs(ref), (ll, ref, sw)
    return sw


def test_flagship_kernel_tail():
    sw = _check(jitter_hyperparameters(solar_like_hyperparameters(30), 1000))
    assert 0 < sw < 65536


@pytest.mark.parametrize("terms", [((50.0, 30.0, 3e4), (2.0, 3000.0, 2.0)), ((1e4, 2.0, 50.0), (2.0, 3000.0, 5.0))])
def test_slow_two_term_kernels_tail(terms):
    sw = _check(_two_terms(*terms))
    assert 0 < sw < 65536


def test_very_slow_weak_kernel_never_arms():
    assert _check(_two_terms((1e-3, 5.0, 1e5), (2.0, 3000.0, 2.0))) == -1


FAST_TERM = ((2.0, 3000.0, 0.6), (2.0, 1000.0, 3.0), (3.0, 400.0, 2.0))     # c_max * 240 s = 3.8: scaling block 16


def test_short_scaling_block_keeps_the_rule_in_rows():
    """A cadence at which the streamed sweep's scaling block is 16 (and 4 on the short span): the anchors of the
    rule stay on the 64-row grid, so its lag is still 1024 rows; the tail with decays every 16 rows at 1e-10."""
    from gadfly_amd.engine import StreamingBatch, _scaled_span
    coeffs, _ = _kernel_coeffs(_two_terms(*FAST_TERM))
    x = 1.5 * float(np.max(coeffs[4])) * 240e-6
    assert StreamingBatch._scaling_block(x, _scaled_span(True)) == 16
    assert StreamingBatch._scaling_block(x, _scaled_span(False)) == 4
    for block in (16, 4):
        sw = _check(_two_terms(*FAST_TERM), N=16384, cadence=240.0, block=block)
        assert 0 < sw < 16384 and sw % GRID == 0 and sw >= (LAG + COUNT - 1) * GRID
