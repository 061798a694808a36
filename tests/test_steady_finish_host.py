"""Host side of the steady tail's finishing launch (k_steady_finish), restated in numpy on the C
oracle's own factor with tests/test_steady_tail_host.py's block filter: the log-likelihood formed as the streamed
route forms it -- the sums of the rows up to the switch row, plus (N - sw) log d_inf, plus (sum z^2) / d_inf with the
64-row blocks starting at the switch row, running across tile boundaries, and each lane summing the z^2 of its own row
slot before one sum over the lanes -- against the oracle; and the state update of a block split over the two half-waves
(rows 0 .. 31 from the incoming state, rows 32 .. 63 from a zero state, joined by lambda^32) against the sequential one."""
import numpy as np
import pytest

from tests.test_steady_host import _two_terms
from tests.test_steady_tail_host import RTOL_BLOCK, _frozen, _problem, _tail_blocks

RTOL_LL = 1e-10         # tests/test_steady_host.py's bar: the mode's share of the accuracy budget


def _finish_loglike(fz, y, L=64):
    """What acc holds behind the finishing launch: the bounded reductions' sums over the rows 0 .. sw (host numbering:
    sw is the switch anchor, the tail starts at sw + 1), then the tail's share from per-lane sums of z^2."""
    sw, N = fz["sw"], len(y)
    d, z = fz["d"][:sw + 1], fz["z"][:sw + 1]
    s1, s2 = np.sum(np.log(d)), np.sum(z * z / d)
    zt, _ = _tail_blocks(fz, y, L=L)        # blocks from the switch row on, no restart at tile boundaries
    assert len(zt) == N - sw - 1
    lanes = np.bincount(np.arange(len(zt)) % L, weights=zt * zt, minlength=L)       # lane = row slot of a block
    s1 += (N - sw - 1) * np.log(fz["dinf"])
    s2 += np.sum(lanes) / fz["dinf"]
    return -0.5 * (s1 + N * np.log(2 * np.pi)) - 0.5 * s2


def _check(hp, N=65536):
    coeffs, t, diag, y, ref = _problem(hp, N)
    fz = _frozen(coeffs, t, diag, y)
    assert 0 < fz["sw"] < N
    ll = _finish_loglike(fz, y)
    print(f"switch row {fz['sw']}: finishing route against the oracle {abs(ll - ref) / abs(ref):.2e}")
    assert abs(ll - ref) <= RTOL_LL * abs(ref), (ll, ref)
    return fz


@pytest.fixture(scope="module")
def flagship():
    """The flagship walker (seed 1000, N = 65 536) through the finishing route, checked against the oracle once."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    return _check(jitter_hyperparameters(solar_like_hyperparameters(30), 1000))


def test_flagship_kernel_finishing_route(flagship):
    assert (65536 - flagship["sw"] - 1) % 64 != 0   # (the last block is a partial one)


@pytest.mark.parametrize("terms", [((50.0, 30.0, 3e4), (2.0, 3000.0, 2.0)), ((1e4, 2.0, 50.0), (2.0, 3000.0, 5.0))])
def test_slow_two_term_kernels_finishing_route(terms):
    _check(_two_terms(*terms))


def _advance(lam, G, s, zb):
    """The sequential state update over the rows of zb, two rows per step and a last odd row alone."""
    lam2, lamG = lam * lam, lam * G
    for j in range(0, len(zb) - 1, 2):
        s = lam2 * s + lamG * zb[j] + G * zb[j + 1]
    if len(zb) % 2:
        s = lam * s + G * zb[-1]
    return s


def _advance_split(lam, G, s, zb, half=32):
    """The update split over the half-waves: rows 0 .. half - 1 from the incoming state, the rows from `half` on from a
    zero state, then s = lambda^(rows in the high half) s_low + s_high.  A partial block bounds each half by itself."""
    lo, hi = zb[:half], zb[half:]
    s_low = _advance(lam, G, s, lo)
    if len(hi) == 0:
        return s_low
    s_high = _advance(lam, G, np.zeros_like(s), hi)
    return lam ** len(hi) * s_low + s_high


@pytest.mark.parametrize("lim", [1, 31, 32, 33, 63, 64])
def test_split_state_update_against_the_sequential_one(flagship, lim):
    """On the flagship walker's frozen lambda, G and state, z of the size of its tail rows."""
    fz = flagship
    lam, G = fz["lam"], fz["G"]
    rng = np.random.Generator(np.random.PCG64(77 + lim))
    zb = float(np.std(fz["z"][fz["sw"]:])) * rng.normal(size=lim)
    want = _advance(lam, G, fz["s"], zb)
    got = _advance_split(lam, G, fz["s"], zb)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"lim {lim}: split against sequential state update {err:.2e} of max |s|")
    assert err <= RTOL_BLOCK
