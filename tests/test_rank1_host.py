"""Host side of the rank-one rows in front of the steady switch (k_steady_rank1): on a uniform cadence
with a constant diagonal the celerite recurrence, in the frame that rotates with the terms' phasors, is a time-invariant
Riccati iteration from S_0 = 0, and the difference of consecutive states keeps rank one (Chandrasekhar / Morf-Sidhu-
Kailath).  Pivot, gain and forward solve then need vectors of length J only.  The recursion is restated here in numpy
from the six coefficient arrays alone and set against the C oracle: its log-likelihood, the switch row of the kernel's
rule on the oracle's own factor, and the hand-over to the frozen tail of tests/test_steady_tail_host.py.

Complex J-vectors, <p, q> = sum_k Re(conj(p_k) q_k); u0 = a - i b, lambda = exp(-(c + i d) Delta),
a0 = sum a + diag.  Start r = 1, d = a0, Y = lambda r, sigma = 1 / d, f = 0; a row:
    k = r / d ;  z_n = y_n - <u0, f> ;  f <- lambda (f + k z_n)
    beta = <u0, Y> ;  r <- r - sigma beta Y ;  d' = d - sigma beta^2 ;  Y <- lambda (Y - beta k) ;  sigma <- sigma d / d'
"""
import functools

import numpy as np
import pytest

from oracle import cref
from tests.test_steady_host import FAST_TERM, GRID, _kernel_coeffs, _series, _switch_row, _two_terms
from tests.test_steady_tail_host import LAG_ROWS, _tail_rows

RTOL_LL = 1e-10         # the steady mode's host bar
RTOL_LIMIT = 1e-11      # what the conditioning limit is set for
JITTER_LIMIT = 1e-7     # the engine's limit on the stamp jitter, in units of 1 / wmax
COND_LIMIT = 1e5        # the engine's limit on a0 / min d (StreamingBatch.RANK1_COND_LIMIT)


def rank1_rows(coeffs, t, diag, y, stop=None):
    """The recursion on the whole series: d, z, and per anchor (rows = 0 mod GRID) the gain k and the pivot.  With
    `stop`, ends at that row and returns (d, z, k, s = f + k z) with the rows up to it: what the kernel leaves at
    its switch row."""
    ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in coeffs[2:6])
    N = len(t)
    delta = (t[-1] - t[0]) / (N - 1)
    u0c = ac + 1j * bc                          # conj(u0): <u0, x> = sum Re(conj(u0) x)
    lam = np.exp(-(cc + 1j * dc) * delta)
    d = float(np.sum(ac) + diag[0])
    r = np.ones(len(ac), dtype=np.complex128)
    Y = lam * r
    sigma = 1.0 / d
    f = np.zeros_like(r)
    dd, zz = np.empty(N), np.empty(N)
    gains = np.zeros(((N + GRID - 1) // GRID, len(ac)), dtype=np.complex128)
    for n in range(N):
        k = r / d
        z = y[n] - float(np.sum((u0c * f).real))
        dd[n], zz[n] = d, z
        assert d > 0.0
        s = f + k * z
        if n % GRID == 0:
            gains[n // GRID] = k
        if n == stop:
            return dd[:n + 1], zz[:n + 1], k, s
        f = lam * s
        beta = float(np.sum((u0c * Y).real))
        r = r - (sigma * beta) * Y
        dn = d - sigma * beta * beta
        Y = lam * (Y - beta * k)
        sigma = sigma * d / dn
        d = dn
    return dd, zz, gains


def rank1_switch_row(dd, gains):
    """The rule of tests/test_steady_host.py::_switch_row, in its own arithmetic, on the recursion's pivots and gains
    (which are derotated already: the rule's phasor is 1 with d = 0 and t = 0)."""
    N, J = len(dd), gains.shape[1]
    W = np.zeros((N, 2 * J))
    W[::GRID, 0::2], W[::GRID, 1::2] = gains.real, gains.imag
    return _switch_row(np.zeros(N), np.zeros(J), dd, W)[0]


def _loglike(d, z):
    return -0.5 * (np.sum(z * z / d) + np.sum(np.log(d))) - 0.5 * len(d) * np.log(2 * np.pi)


def _flagship(seed=1000):
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    return jitter_hyperparameters(solar_like_hyperparameters(30), seed)


CASES = {
    "flagship": (_flagship, 65536, 60.0),
    "slow-a": (lambda: _two_terms((50.0, 30.0, 3e4), (2.0, 3000.0, 2.0)), 65536, 60.0),
    "slow-b": (lambda: _two_terms((1e4, 2.0, 50.0), (2.0, 3000.0, 5.0)), 65536, 60.0),
    "never-arms": (lambda: _two_terms((1e-3, 5.0, 1e5), (2.0, 3000.0, 2.0)), 65536, 60.0),
    "fast-240s": (lambda: _two_terms(*FAST_TERM), 16384, 240.0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Problem, oracle factor and the recursion's rows, once per case (shared, never modified)."""
    make, N, cadence = CASES[name]
    coeffs, shift = _kernel_coeffs(make())
    t, y = _series(N, cadence=cadence)
    diag = np.full(N, 900.0) + shift
    ref, info = cref.loglike(coeffs, t, diag, y)
    assert info == 0
    c, a, U, V = cref.get_matrices(coeffs, t, diag)
    d, W, info = cref.factor(t, c, a, U, V)
    assert info == 0
    dd, zz, anchors = rank1_rows(coeffs, t, diag, y)
    return dict(coeffs=coeffs, t=t, diag=diag, y=y, ref=ref, d=d, W=W, rows=(dd, zz, anchors))


@pytest.mark.parametrize("name", list(CASES))
def test_loglike_and_switch_row(name):
    cs = _case(name)
    dd, zz, anchors = cs["rows"]
    err = abs(_loglike(dd, zz) - cs["ref"]) / abs(cs["ref"])
    sw_ref = _switch_row(cs["t"], np.asarray(cs["coeffs"][5]), cs["d"], cs["W"])[0]
    sw = rank1_switch_row(dd, anchors)
    cond = dd[0] / dd.min()
    print(f"{name}: LL error {err:.2e}, a0 / min d {cond:.3g}, switch row oracle {sw_ref} / recursion {sw}")
    assert err <= RTOL_LL
    assert sw == sw_ref
    assert (sw == -1) == (name == "never-arms")


@pytest.mark.parametrize("name", [n for n in CASES if n != "never-arms"])
def test_hand_over_to_the_frozen_tail(name):
    """d, k and s = f + k z at the switch row are what k_steady_finish starts from: the frozen tail behind them."""
    cs = _case(name)
    coeffs, t, y = cs["coeffs"], cs["t"], cs["y"]
    sw = rank1_switch_row(cs["rows"][0], cs["rows"][2])
    assert sw > 0
    dd, zz, k, s = rank1_rows(coeffs, t, cs["diag"], y, stop=sw)
    assert len(dd) == sw + 1
    dsw = dd[sw]
    ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in coeffs[2:6])
    delta = (t[sw] - t[sw - LAG_ROWS]) / LAG_ROWS
    fz = dict(sw=sw, alpha=ac + 1j * bc, lam=np.exp(-(cc + 1j * dc) * delta), G=k, s=s)
    zt = _tail_rows(fz, y)
    d = np.concatenate([dd, np.full(len(y) - sw - 1, dsw)])
    z = np.concatenate([zz, zt])
    err = abs(_loglike(d, z) - cs["ref"]) / abs(cs["ref"])
    print(f"{name}: switch row {sw}, LL error with the frozen tail {err:.2e}")
    assert err <= RTOL_LL


@pytest.mark.parametrize("seed", [1001, 1777])
def test_other_flagship_seeds(seed):
    coeffs, shift = _kernel_coeffs(_flagship(seed))
    t, y = _series(80000)
    diag = np.full(len(t), 900.0) + shift
    ref, info = cref.loglike(coeffs, t, diag, y)
    assert info == 0
    dd, zz, _ = rank1_rows(coeffs, t, diag, y)
    err = abs(_loglike(dd, zz) - ref) / abs(ref)
    print(f"seed {seed}: LL error {err:.2e}")
    assert err <= RTOL_LL


def test_stamp_jitter_limit():
    """The engine's jitter limit, 1e-7 / wmax: the recursion (which knows one cadence only) against the oracle on the
    jittered stamps."""
    cs = _case("flagship")
    coeffs, t, diag, y = cs["coeffs"], cs["t"], cs["diag"], cs["y"]
    wmax = float(max(np.max(coeffs[4]), np.max(np.abs(coeffs[5]))))
    tj = t + np.random.Generator(np.random.PCG64(99)).uniform(-1.0, 1.0, len(t)) * JITTER_LIMIT / wmax
    ref, info = cref.loglike(coeffs, tj, diag, y)
    assert info == 0
    dd, zz, _ = rank1_rows(coeffs, tj, diag, y)
    err = abs(_loglike(dd, zz) - ref) / abs(ref)
    print(f"jitter {JITTER_LIMIT:g} / wmax: LL error {err:.2e}")
    assert err <= RTOL_LL           # (measured 1.4e-11 with this draw of the jitter: the budget is the host bar)


COND_TERMS = ((6e6, 2.0, 50.0), (2.0, 3000.0, 5.0))


def test_conditioning_limit():
    """A kernel whose a0 / min d stands at the engine's limit: r and d are running differences, so the error grows
    with the conditioning; at the limit it stays within 1e-11."""
    coeffs, shift = _kernel_coeffs(_two_terms(*COND_TERMS))
    t, y = _series(65536)
    diag = np.full(len(t), 900.0) + shift
    ref, info = cref.loglike(coeffs, t, diag, y)
    assert info == 0
    dd, zz, _ = rank1_rows(coeffs, t, diag, y)
    cond = dd[0] / dd.min()
    err = abs(_loglike(dd, zz) - ref) / abs(ref)
    print(f"a0 / min d {cond:.3g}: LL error {err:.2e}")
    assert 0.5 * COND_LIMIT <= cond <= 2.0 * COND_LIMIT
    assert err <= RTOL_LIMIT
