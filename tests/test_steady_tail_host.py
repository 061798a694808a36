"""Host side of the steady tail as a time-invariant block filter (k_steady_tail): the row form and
the 64-row block form restated in numpy on the C oracle's own factor, with the switch rule of
tests/test_steady_host.py and the cadence taken over a lag of 1024 rows.

Per complex term k: alpha = a + i b, lambda = exp(-(c + i d) Delta), G the frozen derotated gain, and the state
s = e^{-i d t_n} (F_2k + i F_2k+1)_n + G z_n (this row's update folded).  One row:
    x = lambda s ;  z_n = y_n - sum_k Re(alpha_k x_k) ;  s = x + G z_n.
A block of L rows: p_i = y_i - sum_k Re(alpha_k lambda_k^(i+1) s_k), z = H p with H the lower-triangular Toeplitz
matrix of the impulse response h, then s advances over the block's rows with the z now known."""
import numpy as np
import pytest

from oracle import cref
from tests.test_steady_host import FAST_TERM, _kernel_coeffs, _series, _switch_row, _two_terms

LAG_ROWS = 1024         # the cadence estimate: (t_sw - t_{sw - 1024}) / 1024
RTOL_LL = 1e-10         # the mode's share of the accuracy budget
RTOL_Z = 1e-9           # tail rows against the oracle's forward solve, relative to max |z|
RTOL_BLOCK = 1e-12      # block form against row form, relative to max |z|


def _frozen(coeffs, t, diag, y):
    """Oracle factor and forward solve, the switch row of the rule, and what the tail starts from: alpha, lambda,
    G, the folded derotated state at the switch row, d_inf."""
    c, a, U, V = cref.get_matrices(coeffs, t, diag)
    d, W, info = cref.factor(t, c, a, U, V)
    assert info == 0
    z = cref.solve_lower(t, c, U, W, y)
    ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in coeffs[2:6])
    sw, gain, dinf = _switch_row(t, dc, d, W)
    if sw < 0:
        return dict(sw=-1, d=d, z=z)
    F = np.zeros(U.shape[1])
    for n in range(sw + 1):                 # celerite's F just after row sw, that row's update folded
        if n:
            F *= np.exp(-c * (t[n] - t[n - 1]))
        F += W[n] * z[n]
    s = np.exp(-1j * dc * t[sw]) * (F[0::2] + 1j * F[1::2])
    delta = (t[sw] - t[sw - LAG_ROWS]) / LAG_ROWS
    return dict(sw=sw, d=d, z=z, alpha=ac + 1j * bc, lam=np.exp(-(cc + 1j * dc) * delta), G=gain, s=s, dinf=dinf)


def _tail_rows(fz, y):
    """Row form: z of the rows sw + 1 .. N - 1."""
    alpha, lam, G, s = fz["alpha"], fz["lam"], fz["G"], fz["s"].copy()
    out = np.empty(len(y) - fz["sw"] - 1)
    for i, yn in enumerate(y[fz["sw"] + 1:]):
        x = lam * s
        out[i] = yn - np.sum((alpha * x).real)
        s = x + G * out[i]
    return out


def _impulse_response(fz, L):
    alpha, lam, G = fz["alpha"], fz["lam"], fz["G"]
    kappa = np.array([np.sum((alpha * G * lam ** j).real) for j in range(L)])       # kappa(0) unused
    h = np.zeros(L)
    h[0] = 1.0
    for m in range(1, L):
        h[m] = -np.sum(kappa[1:m + 1] * h[m - 1::-1][:m])
    return h


def _tail_blocks(fz, y, L=64, tile=None):
    """Block form as the kernel runs it: blocks of L rows from sw + 1 on, restarted at every tile boundary (rows = 0
    mod `tile`), partial blocks at the tile ends; the state advances two rows per step, a last odd row alone."""
    alpha, lam, G, s = fz["alpha"], fz["lam"], fz["G"], fz["s"].copy()
    h = _impulse_response(fz, L)
    H = np.zeros((L, L))
    for m in range(L):
        H += np.diag(np.full(L - m, h[m]), -m)
    coef = alpha[None, :] * lam[None, :] ** np.arange(1, L + 1)[:, None]             # [row in block][term]
    lam2, lamG = lam * lam, lam * G
    first, N = fz["sw"] + 1, len(y)
    out = np.empty(N - first)
    b0 = first
    while b0 < N:
        end = N if tile is None else min(N, (b0 // tile + 1) * tile)
        lim = min(L, end - b0)
        p = np.zeros(L)
        p[:lim] = y[b0:b0 + lim] - (coef[:lim] * s[None, :]).real.sum(axis=1)
        zb = H @ p
        out[b0 - first:b0 - first + lim] = zb[:lim]
        for j in range(0, lim - 1, 2):
            s = lam2 * s + lamG * zb[j] + G * zb[j + 1]
        if lim % 2:
            s = lam * s + G * zb[lim - 1]
        b0 += lim
    return out, h


def _loglike(fz, ztail):
    sw, N = fz["sw"], len(fz["z"])
    z, d = fz["z"].copy(), fz["d"].copy()
    z[sw + 1:], d[sw + 1:] = ztail, fz["dinf"]
    return -0.5 * (np.sum(z * z / d) + np.sum(np.log(d))) - 0.5 * N * np.log(2 * np.pi)


def _problem(hp, N, cadence=60.0, jitter=0.0, seed=99):
    coeffs, shift = _kernel_coeffs(hp)
    t, y = _series(N, cadence=cadence)
    if jitter:
        wmax = float(max(np.max(coeffs[4]), np.max(np.abs(coeffs[5]))))
        t = t + np.random.Generator(np.random.PCG64(seed)).uniform(-1.0, 1.0, N) * jitter / wmax
    diag = np.full(N, 900.0) + shift
    ref, info = cref.loglike(coeffs, t, diag, y)
    assert info == 0
    return coeffs, t, diag, y, ref


def _check(hp, N=65536, cadence=60.0, jitter=0.0, blocks=True):
    coeffs, t, diag, y, ref = _problem(hp, N, cadence, jitter)
    fz = _frozen(coeffs, t, diag, y)
    if fz["sw"] < 0:
        return -1
    zmax = np.max(np.abs(fz["z"]))
    zr = _tail_rows(fz, y)
    ll = _loglike(fz, zr)
    ez = np.max(np.abs(zr - fz["z"][fz["sw"] + 1:])) / zmax
    print(f"switch row {fz['sw']}: LL error {abs(ll - ref) / abs(ref):.2e}, z error {ez:.2e}")
    assert abs(ll - ref) <= RTOL_LL * abs(ref), (ll, ref)
    assert ez <= RTOL_Z
    if blocks:
        zb, h = _tail_blocks(fz, y)
        eb = np.max(np.abs(zb - zr)) / zmax
        print(f"  block form against row form {eb:.2e}, max |h| {np.max(np.abs(h)):.3f}, h(63) {h[63]:.2e}")
        assert eb <= RTOL_BLOCK
        assert abs(_loglike(fz, zb) - ref) <= RTOL_LL * abs(ref)
    return fz["sw"]


def test_flagship_kernel_rows_and_blocks():
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    sw = _check(jitter_hyperparameters(solar_like_hyperparameters(30), 1000))
    assert 0 < sw < 65536


@pytest.mark.parametrize("terms", [((50.0, 30.0, 3e4), (2.0, 3000.0, 2.0)), ((1e4, 2.0, 50.0), (2.0, 3000.0, 5.0))])
def test_slow_two_term_kernels(terms):
    sw = _check(_two_terms(*terms))
    assert 0 < sw < 65536


def test_fast_term_at_240_s():
    sw = _check(_two_terms(*FAST_TERM), N=16384, cadence=240.0)
    assert 0 < sw < 16384


def test_partial_last_block():
    """N - switch - 1 is not a multiple of 64: the last block's rows beyond the series are never read."""
    N = 16384 + 37
    coeffs, t, diag, y, ref = _problem(_two_terms(*FAST_TERM), N, 240.0)
    fz = _frozen(coeffs, t, diag, y)
    assert fz["sw"] > 0 and (N - fz["sw"] - 1) % 64 != 0
    zr = _tail_rows(fz, y)
    zb, _ = _tail_blocks(fz, y)
    zmax = np.max(np.abs(fz["z"]))
    assert np.max(np.abs(zb - zr)) <= RTOL_BLOCK * zmax
    zt, _ = _tail_blocks(fz, y, tile=4096)      # (blocks restarted at the tile boundaries: odd partial blocks there)
    assert (4096 - fz["sw"] - 1) % 64 % 2 == 1
    assert np.max(np.abs(zt - zr)) <= RTOL_BLOCK * zmax
    assert np.max(np.abs(zb - fz["z"][fz["sw"] + 1:])) <= RTOL_Z * zmax
    assert abs(_loglike(fz, zb) - ref) <= RTOL_LL * abs(ref)


@pytest.mark.parametrize("level", [1e-10, 1e-9, 1e-8])
def test_stamp_jitter(level):
    """Uniform stamp jitter of level / wmax (seeded): wherever the rule arms, the constant-cadence tail holds 1e-10;
    a level at which the rule never arms passes by asserting exactly that."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    sw = _check(jitter_hyperparameters(solar_like_hyperparameters(30), 1000), jitter=level, blocks=False)
    print(f"jitter {level:g} / wmax: " + ("never arms" if sw < 0 else f"arms at row {sw}"))
    assert sw == -1 or 0 < sw < 65536
