"""
TEST INFRASTRUCTURE: numpy restatement of ``gadfly_amd.prepare_quarters`` -- the ``detrend=True`` branch of the
reference's ``PowerSpectrum.from_light_curve`` (gadfly/psd.py:482-535) on plain arrays.

Parity with lightkurve is unpinned: neither lightkurve nor astropy can be imported here, so ``remove_nans`` and
``remove_outliers(sigma=5)`` (astropy's ``sigma_clip(sigma, maxiters=5, cenfunc=median, stdfunc=std)``) are restated
from their documented behaviour: drop the rows whose time or flux is not finite; per round take the median and the
population standard deviation of the survivors, keep ``med - sigma_lower sd <= f <= med + sigma_upper sd``, stop
after the round that removed nothing or after ``maxiters`` rounds.  The gap fill and the numpy normalisation are
``oracle/interp_ref``'s (the reference's own steps).
"""
import numpy as np

from oracle import interp_ref


def sigma_clip(f, t=None, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5):
    """(keep mask, rounds run, margin): margin = min |f - bound| / max |bound| over all rounds and kept points --
    how far the nearest point stayed from a threshold, i.e. how much rounding in med / sd the mask tolerates."""
    f = np.asarray(f, dtype=np.float64)
    keep = np.isfinite(f) if t is None else np.isfinite(f) & np.isfinite(np.asarray(t, dtype=np.float64))
    idx = np.flatnonzero(keep)
    x = f[idx]
    rounds, margin = 0, np.inf
    if sigma is not None:
        lo_s = sigma if sigma_lower is None else sigma_lower
        hi_s = sigma if sigma_upper is None else sigma_upper
        while x.size and (maxiters is None or rounds < maxiters):
            rounds += 1
            med, sd = np.median(x), np.std(x)
            lo, hi = med - lo_s * sd, med + hi_s * sd
            scale = max(abs(lo), abs(hi))
            if sd > 0:
                margin = min(margin, float(np.min(np.minimum(np.abs(x - lo), np.abs(x - hi))) / scale))
            ok = (x >= lo) & (x <= hi)
            if ok.all():
                break
            x, idx = x[ok], idx[ok]
    mask = np.zeros(f.size, bool)
    mask[idx] = True
    return mask, rounds, margin


def legendre_basis(t, order, dtype=np.float64):
    """P_0 .. P_order at u = (t - mid) / half, mid and half from the first and last stamp (u = 0 if they coincide)."""
    t = np.asarray(t, dtype=dtype)
    half_ = dtype(0.5)
    mid, half = half_ * (t[0] + t[-1]), half_ * (t[-1] - t[0])
    u = (t - mid) / half if half != 0 else np.zeros_like(t)
    P = [np.ones_like(u), u]
    for j in range(1, 8):
        P.append((dtype(2 * j + 1) * u * P[j] - dtype(j) * P[j - 1]) / dtype(j + 1))
    return np.stack(P[:order + 1], axis=1)


def normalise_legendre(t, f, order):
    """The float64 restatement of what the device does: Legendre normal equations, Cholesky, f / fit, ppm."""
    P = legendre_basis(t, order)
    f = np.asarray(f, dtype=np.float64)
    L = np.linalg.cholesky(P.T @ P)
    c = np.linalg.solve(L.T, np.linalg.solve(L, P.T @ f))
    normed = f / (P @ c)
    return 1e6 * (normed / np.median(normed) - 1)


def normalise_numpy(t, f, order):
    """The reference's float64 route (psd.py:502-512)."""
    x = t - t.mean()
    normed = f / np.polyval(np.polyfit(x, f, order), x)
    return 1e6 * np.array(normed / np.median(normed) - 1)


def normalise_longdouble(t, f, order):
    """The same least-squares fit in 80-bit arithmetic: monomials of the centred, scaled time orthonormalised by a
    twice-iterated Gram-Schmidt, projection, f / fit, ppm.  Returned in float64."""
    t = np.asarray(t, dtype=np.longdouble)
    f = np.asarray(f, dtype=np.longdouble)
    x = t - t.mean()
    s = np.abs(x).max()
    u = x / s if s != 0 else x
    V = np.stack([u ** j for j in range(order + 1)], axis=1)
    Q = np.zeros_like(V)
    for j in range(order + 1):
        v = V[:, j].copy()
        for _ in range(2):
            for i in range(j):
                v -= Q[:, i] * (Q[:, i] @ v)
        Q[:, j] = v / np.sqrt(v @ v)
    normed = f / (Q @ (Q.T @ f))
    return np.asarray(1e6 * (normed / np.median(normed) - 1), dtype=np.float64)


NORMALISERS = {"legendre": normalise_legendre, "numpy": normalise_numpy, "longdouble": normalise_longdouble}


def prepare_quarters(quarters, detrend_poly_order=3, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5,
                     fill=True, in_ppm=False, normaliser="legendre", details=None):
    """(times, flux_ppm, cadence) of one star; ``details`` (a list) receives (mask, rounds, margin) per quarter."""
    norm = NORMALISERS[normaliser]
    ts, fs = [], []
    for t, f in quarters:
        t, f = np.asarray(t, dtype=np.float64), np.asarray(f, dtype=np.float64)
        mask, rounds, margin = sigma_clip(f, t, sigma, sigma_lower, sigma_upper, maxiters)
        if details is not None:
            details.append((mask, rounds, margin))
        t, f = t[mask], f[mask]
        if fill:
            t, f = interp_ref.interpolate_missing_data(t, f)
        if not in_ppm:
            f = norm(t, f, detrend_poly_order)
        ts.append(t)
        fs.append(f)
    t, f = np.concatenate(ts), np.concatenate(fs)
    if len(ts) > 1 and fill:
        t, f = interp_ref.interpolate_missing_data(t, f)
    return t, f, float(np.median(np.diff(t)))
