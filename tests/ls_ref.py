"""
CPU oracle of the Lomb-Scargle power spectrum (test helper; not part of the product path).

A direct numpy evaluation of what /root/reference/gadfly/psd.py:589-601 asks astropy for:
``LombScargle(t, y, normalization='psd').power(rfftfreq(n, d)) * d / sqrt(2 pi)`` with astropy's
defaults (no dy, fit_mean, center_data, nterms = 1), i.e. the floating-mean periodogram, evaluated
exactly (not astropy's Press-Rybicki approximation).  Phases are formed in cycles as one float64
product ``p = f t'`` (t' = t - t[0]) and reduced exactly, ``p - rint(p)``.  Two formulations pin each
other: the quadratic form of the centred 2 x 2 covariance (what the device evaluates, with the
degenerate limits of DESIGN.md 3.6) and astropy's tau-rotated form.
"""
import numpy as np

ZERO_TOL = 1e-10
RANK_TOL = 1e-10


def _sums(t, y, freq, chunk):
    t = np.asarray(t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(t)
    tp = t - t[0]
    yc = y - y.mean()
    w = 1.0 / n
    out = np.empty((7, len(freq)))
    for a in range(0, len(freq), chunk):
        f = np.asarray(freq[a:a + chunk], dtype=np.float64)
        p = f[:, None] * tp[None, :]
        p = p - np.rint(p)
        c, s = np.cos(2 * np.pi * p), np.sin(2 * np.pi * p)
        out[0, a:a + chunk] = c.sum(1) * w
        out[1, a:a + chunk] = s.sum(1) * w
        out[2, a:a + chunk] = (c * c).sum(1) * w
        out[3, a:a + chunk] = (c * s).sum(1) * w
        out[4, a:a + chunk] = (s * s).sum(1) * w
        out[5, a:a + chunk] = (c @ yc) * w
        out[6, a:a + chunk] = (s @ yc) * w
    return n, out


def _centred(v):
    C, S, CC, CS, SS, YC, YS = v
    return CC - C * C, SS - S * S, CS - C * S, YC, YS


def power_quadratic(t, y, freq, chunk=256):
    """P(f) = (n/2) v^T A^-1 v, A the centred covariance of the cos/sin columns; rank-one and zero limits."""
    n, v = _sums(t, y, freq, chunk)
    Ch, Sh, Xh, YC, YS = _centred(v)
    lam = Ch + Sh
    det = Ch * Sh - Xh * Xh
    P = np.zeros_like(lam)
    gen = (lam > ZERO_TOL) & (det > RANK_TOL * lam * lam)
    P[gen] = 0.5 * n * (Sh * YC * YC - 2 * Xh * YC * YS + Ch * YS * YS)[gen] / det[gen]
    one = (lam > ZERO_TOL) & ~gen
    u0 = np.where(Ch >= Sh, Ch, Xh)
    u1 = np.where(Ch >= Sh, Xh, Sh)
    with np.errstate(invalid="ignore", divide="ignore"):
        uv = (u0 * YC + u1 * YS) ** 2 / (u0 * u0 + u1 * u1)
    P[one] = 0.5 * n * uv[one] / lam[one]
    return P


def power_tau(t, y, freq, chunk=256):
    """astropy's form: rotate by tau (tan 2 omega tau = 2 X^ / (C^ - S^)), P = (n/2)(YC_t^2/CC_t + YS_t^2/SS_t).
    General frequencies only (no degenerate limit)."""
    n, v = _sums(t, y, freq, chunk)
    Ch, Sh, Xh, YC, YS = _centred(v)
    phi = 0.5 * np.arctan2(2 * Xh, Ch - Sh)
    ct, st = np.cos(phi), np.sin(phi)
    YCt = YC * ct + YS * st
    YSt = YS * ct - YC * st
    CCt = Ch * ct * ct + 2 * Xh * ct * st + Sh * st * st
    SSt = Sh * ct * ct - 2 * Xh * ct * st + Ch * st * st
    return 0.5 * n * (YCt * YCt / CCt + YSt * YSt / SSt)


def ls_power(t, y, d=None, include_zero_freq=False, freq_index=None, chunk=256):
    """(frequency [uHz], power [ppm^2/uHz], norm) of one series (t in 1/uHz, y in ppm) on rfftfreq's grid;
    ``freq_index`` picks a subset of the returned frequencies (indices after the zero-frequency drop)."""
    t = np.asarray(t, dtype=np.float64)
    if d is None:
        d = float(np.median(np.diff(t)))
    freq = np.fft.rfftfreq(len(t), d)
    if not include_zero_freq:
        freq = freq[1:]
    if freq_index is not None:
        freq = freq[np.asarray(freq_index)]
    norm = d / (2 * np.pi) ** 0.5
    return freq, power_quadratic(t, y, freq, chunk) * norm, norm
