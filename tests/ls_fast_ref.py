"""
CPU restatement of the non-uniform-FFT route of the Lomb-Scargle power spectrum (test helper; not part of
the product path): the four steps of ``gadfly_lsfft.hip`` + ``psd._ls_nufft`` in numpy.

1. wrap: t' = t - t[0], y' = (y - y[0]) - mean, x = frac(t' df) with df = 1 / (n d) -- every exponential the
   periodogram needs has period n d in t';
2. spread y' and 1 onto a fine grid of n_f cells (the next 2-3-5-smooth integer >= 4 (2 [n/2] + 1) + 2 w) with
   phi(z) = exp(beta (sqrt(1 - z^2) - 1)), z = (cell - x n_f) / (w / 2), w = 16, beta = 2.30 w, over the 16 cells
   floor(x n_f) - 7 ... floor(x n_f) + 8 (wrapping round the ends of the grid);
3. F(k) = conj(rfft(grid))[k];
4. divide by phi^(k) = w int_0^1 phi(z) cos(pi w k z / n_f) dz (64 Gauss-Legendre nodes on [0, 1]), form the seven
   sums from F_1(k), F_1(2k), F_y(k) and finish with the formula (and degenerate limits) of ``ls_ref``.
"""
import numpy as np

from tests import ls_ref

W = 16
BETA = 2.30 * W
SIGMA = 2
QUAD = 64


def grid_size(n):
    """Fine-grid cells of an n-point series: the next 2-3-5-smooth integer >= 2 (2 [n/2] + 1) sigma + 2 w."""
    m = 2 * (2 * (n // 2) + 1) * SIGMA + 2 * W
    while True:
        r = m
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 1


def phi(z):
    return np.exp(BETA * (np.sqrt(np.maximum(0.0, 1.0 - z * z)) - 1.0))


def wrap(t, n_f, df):
    """(u, cell): fine-grid positions u = frac(t' df) n_f in [0, n_f] and their cells floor(u) in [0, n_f)."""
    q = (np.asarray(t, dtype=np.float64) - t[0]) * df
    x = q - np.floor(q)
    x = np.where(x >= 1.0, x - 1.0, x)
    u = x * n_f
    return u, np.minimum(u.astype(np.int64), n_f - 1)


def spread(u, cell, strengths, n_f):
    grid = np.zeros(n_f)
    for o in range(-(W // 2 - 1), W // 2 + 1):
        c = cell + o
        np.add.at(grid, c % n_f, strengths * phi((c - u) / (W / 2)))
    return grid


def phi_hat(k, n_f):
    z, wq = np.polynomial.legendre.leggauss(QUAD)
    z, wq = 0.5 * (z + 1.0), 0.5 * wq                       # nodes and weights on [0, 1]
    a = W * wq * phi(z)
    return np.cos((np.pi * W / n_f) * np.asarray(k, dtype=np.float64)[:, None] * z[None, :]) @ a


def sums(t, y, d):
    """(n, the seven sums C, S, CC, CS, SS, YC, YS at k = 0 ... n // 2) of one series."""
    t = np.asarray(t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(t)
    n_f = grid_size(n)
    yc = y - y[0]
    yc = yc - yc.mean()
    u, cell = wrap(t, n_f, 1.0 / (n * d))
    F1 = np.conj(np.fft.rfft(spread(u, cell, np.ones(n), n_f)))
    Fy = np.conj(np.fft.rfft(spread(u, cell, yc, n_f)))
    k = np.arange(n // 2 + 1)
    F1k = F1[k] / phi_hat(k, n_f) / n
    F12 = F1[2 * k] / phi_hat(2 * k, n_f) / n
    Fyk = Fy[k] / phi_hat(k, n_f) / n
    CC = 0.5 * (1.0 + F12.real)
    return n, np.array([F1k.real, F1k.imag, CC, 0.5 * F12.imag, 1.0 - CC, Fyk.real, Fyk.imag])


def ls_power(t, y, d=None, include_zero_freq=False):
    """(frequency [uHz], power [ppm^2/uHz], norm) of one series, as ``ls_ref.ls_power`` returns them."""
    t = np.asarray(t, dtype=np.float64)
    if d is None:
        d = float(np.median(np.diff(t)))
    n, v = sums(t, y, d)
    Ch, Sh, Xh, YC, YS = ls_ref._centred(v)
    lam = Ch + Sh
    det = Ch * Sh - Xh * Xh
    P = np.zeros_like(lam)
    gen = (lam > ls_ref.ZERO_TOL) & (det > ls_ref.RANK_TOL * lam * lam)
    P[gen] = 0.5 * n * (Sh * YC * YC - 2 * Xh * YC * YS + Ch * YS * YS)[gen] / det[gen]
    one = (lam > ls_ref.ZERO_TOL) & ~gen
    u0 = np.where(Ch >= Sh, Ch, Xh)
    u1 = np.where(Ch >= Sh, Xh, Sh)
    with np.errstate(invalid="ignore", divide="ignore"):
        uv = (u0 * YC + u1 * YS) ** 2 / (u0 * u0 + u1 * u1)
    P[one] = 0.5 * n * uv[one] / lam[one]
    first = 0 if include_zero_freq else 1
    norm = d / (2 * np.pi) ** 0.5
    return np.fft.rfftfreq(n, d)[first:], P[first:] * norm, norm
