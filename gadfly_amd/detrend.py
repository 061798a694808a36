"""
Raw observing quarters to one detrended series per star, on the device: the ``detrend=True`` branch of the
reference's ``PowerSpectrum.from_light_curve`` (gadfly/psd.py:482-535) on plain arrays.

Per quarter: drop the rows whose time or flux is not finite and clip outliers about the median
(``lc.remove_nans().remove_outliers()``), fill the missing cadences (:func:`gadfly_amd.interpolate_missing_data`),
divide by a least-squares polynomial in time and by the median, ``1e6 (f / median - 1)``; then the quarters in the
order given, and one more fill over the gaps between them.  All quarters of all stars of a call go through the
clip, the compaction, the medians and the fit together, as ONE segmented batch (``gf_sigma_clip``,
``gf_seg_compact``, ``gf_seg_diff``, ``gf_seg_median``, ``gf_poly_normalise``, ``gf_seg_ppm``, and for the gap fill
``gf_interp_plan_seg`` / ``gf_interp_fill_seg``).

Parity with lightkurve is unpinned: neither lightkurve nor astropy is a dependency, so the clip is restated from
the documented behaviour of ``remove_outliers(sigma=5)`` -- astropy's ``sigma_clip(sigma, maxiters=5,
cenfunc=median, stdfunc=std)`` -- and tested against ``tests/detrend_ref.py``.
"""
import numpy as np

from . import _lib
from .interp import _fill_segments

__all__ = ["prepare_quarters", "prepare_quarters_batch"]


def _check_options(order, sigma, sigma_lower, sigma_upper, maxiters):
    """-> (sigma_lower, sigma_upper, maxiters) as ``gf_sigma_clip`` takes them (maxiters 0: no clip, -1: no cap)."""
    if int(order) != order or not 0 <= order <= _lib.GF_DETREND_MAX_ORDER:
        raise ValueError(f"detrend_poly_order={order!r} must be an integer in 0..{_lib.GF_DETREND_MAX_ORDER}")
    if sigma is None and sigma_lower is None and sigma_upper is None:
        return 1.0, 1.0, 0
    lo = sigma if sigma_lower is None else sigma_lower
    hi = sigma if sigma_upper is None else sigma_upper
    for name, v in (("sigma_lower", lo), ("sigma_upper", hi)):
        if v is None or not float(v) > 0.0:
            raise ValueError(f"{name}={v!r} must be positive (sigma=None switches the clip off)")
    if maxiters is None:
        return float(lo), float(hi), -1
    if int(maxiters) != maxiters or maxiters < 1:
        raise ValueError(f"maxiters={maxiters!r} must be None or an integer >= 1")
    return float(lo), float(hi), int(maxiters)


def _check_input(stars, need):
    """The stars' quarters as float64 arrays, checked over their finite rows: -> (ts, fs, labels, quarters per star)."""
    ts, fs, labels, counts = [], [], [], []
    if len(stars) < 1:
        raise ValueError("no stars")
    for b, quarters in enumerate(stars):
        if len(quarters) < 1:
            raise ValueError(f"star {b}: no quarters")
        last = -np.inf
        for q, (t, f) in enumerate(quarters):
            t = np.ascontiguousarray(t, dtype=np.float64)
            f = np.ascontiguousarray(f, dtype=np.float64)
            if t.ndim != 1 or t.shape != f.shape:
                raise ValueError(f"star {b}, quarter {q}: dimension mismatch")
            tf = t[np.isfinite(t) & np.isfinite(f)]
            if tf.size < need:
                raise ValueError(f"star {b}, quarter {q}: {tf.size} finite points, {need} are needed")
            if tf.size:
                if np.any(np.diff(tf) <= 0):
                    raise ValueError(f"star {b}, quarter {q}: times must be strictly increasing")
                if not tf[0] > last:
                    raise ValueError(f"star {b}, quarter {q}: starts at {tf[0]!r}, before the previous quarter "
                                     f"ends ({last!r}); quarters must be in chronological order")
                last = tf[-1]
            ts.append(t)
            fs.append(f)
            labels.append((b, q))
        counts.append(len(quarters))
    return ts, fs, labels, counts


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


class _Device:
    """The segmented entry points on one device and stream; every array argument is a tensor on that device."""

    def __init__(self, dev):
        import torch
        self.torch, self.lib, self.dev = torch, _lib.load(), dev
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def empty(self, n, dtype=None):
        return self.torch.empty(int(n), dtype=dtype or self.torch.float64, device=self.dev)

    def median(self, S, off, x, drop_last=0):
        med = self.empty(S)
        _lib.check(self.lib.gf_seg_median(S, _lib.ptr(off), _lib.ptr(x), None, drop_last, _lib.ptr(med), self.st),
                   "gf_seg_median")
        return med

    def cadence(self, S, off, t):
        """median(diff(t)) per segment"""
        d = self.empty(t.numel())
        _lib.check(self.lib.gf_seg_diff(S, _lib.ptr(off), _lib.ptr(t), _lib.ptr(d), self.st), "gf_seg_diff")
        return self.median(S, off, d, drop_last=1)

    def fill(self, off_h, off, t, f, dt, which=None, name=lambda s: f"segment {s}"):
        """`interpolate_missing_data` of the segments with `which[s] != 0` (host flags; None: all; the others are
        copied) at the cadences `dt` [S], which stay on the device: one plan, ONE read-back of the new offsets, one
        fill.  -> (new host offsets, new device offsets, t, f)"""
        S = len(off_h) - 1
        if which is not None:
            which = self.torch.as_tensor(np.asarray(which, dtype=np.uint8), device=self.dev)
        return _fill_segments(self.lib, self.dev, self.st, S, int(off_h[-1]), off, t, f, None, dt, which, name)


def prepare_quarters_batch(stars, detrend_poly_order=3, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5,
                           fill=True, in_ppm=False, device=None, return_device=False):
    """
    :func:`prepare_quarters` of B stars in one segmented batch: ``stars`` is a list of B lists of raw
    ``(times [d], flux)`` pairs.  Returns a list of B ``(times, flux_ppm, cadence)`` triples -- a ragged batch as
    ``log_likelihood_batch`` and ``PowerSpectrum.from_lomb_scargle`` take it; with ``return_device=True``
    ``([(times, flux_ppm), ...], cadences)`` with float64 device tensors, whose fluxes ``from_lomb_scargle`` and
    ``from_flux`` take without a copy.  A star's result does not depend on the other stars of the call, bit for bit.
    """
    import torch
    k = detrend_poly_order
    lo, hi, iters = _check_options(k, sigma, sigma_lower, sigma_upper, maxiters)
    k = int(k)
    need = max(2, k + 1)
    ts, fs, labels, per_star = _check_input(stars, need)
    S, B = len(ts), len(per_star)
    off_h = _offsets([len(t) for t in ts])
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _lib.require_device()
    with torch.cuda.device(dev):
        d = _Device(dev)
        lib, st = d.lib, d.st
        t0 = torch.as_tensor(np.concatenate(ts), device=dev)
        f0 = torch.as_tensor(np.concatenate(fs), device=dev)
        off0 = torch.as_tensor(off_h, device=dev)
        # drop the non-finite rows, clip, pack
        keep = d.empty(off_h[-1], torch.uint8)
        meta = d.empty(2 * S + 1, torch.int64)                      # kept [S], packed offsets [S + 1]
        rounds = d.empty(S, torch.int32)
        _lib.check(lib.gf_sigma_clip(S, _lib.ptr(off0), _lib.ptr(t0), _lib.ptr(f0), lo, hi, iters, _lib.ptr(keep),
                                     _lib.ptr(meta), _lib.ptr(rounds), st), "gf_sigma_clip")
        t1, f1 = d.empty(off_h[-1]), d.empty(off_h[-1])
        off1 = meta[S:]
        _lib.check(lib.gf_seg_compact(S, _lib.ptr(off0), _lib.ptr(keep), _lib.ptr(t0), _lib.ptr(f0), _lib.ptr(off1),
                                      _lib.ptr(t1), _lib.ptr(f1), st), "gf_seg_compact")
        dt1 = d.cadence(S, off1, t1) if fill else None
        off1_h = meta.cpu().numpy()[S:]
        for s, n in enumerate(np.diff(off1_h)):
            if n < need:
                raise ValueError(f"star {labels[s][0]}, quarter {labels[s][1]}: {n} points survive the clip, "
                                 f"{need} are needed (detrend_poly_order={k})")
        t1, f1 = t1[:int(off1_h[-1])], f1[:int(off1_h[-1])]
        if fill:
            off2_h, off2, t2, f2 = d.fill(off1_h, off1, t1, f1, dt1,
                                          name=lambda s: f"star {labels[s][0]}, quarter {labels[s][1]}")
        else:
            off2_h, off2, t2, f2 = off1_h, off1, t1, f1
        # polynomial and median out, ppm
        if not in_ppm:
            info = d.empty(S, torch.int32)
            normed = torch.empty_like(f2)
            _lib.check(lib.gf_poly_normalise(S, _lib.ptr(off2), _lib.ptr(t2), _lib.ptr(f2), k, _lib.ptr(normed),
                                             _lib.ptr(info), st), "gf_poly_normalise")
            f2 = normed
            med = d.median(S, off2, f2)
            _lib.check(lib.gf_seg_ppm(S, _lib.ptr(off2), _lib.ptr(f2), _lib.ptr(med), _lib.ptr(f2), st), "gf_seg_ppm")
        # stitch: a star's quarters are neighbours already; fill the gaps between them
        first = _offsets(per_star)
        off3_h = off2_h[first]
        off3 = torch.as_tensor(off3_h, device=dev)
        many = [n > 1 for n in per_star]
        if fill and any(many):
            off3_h, off3, t2, f2 = d.fill(off3_h, off3, t2, f2, d.cadence(B, off3, t2), many,
                                          name=lambda b: f"star {b}")
        cadence = d.cadence(B, off3, t2).cpu().numpy()
        if not in_ppm:
            bad = np.flatnonzero(info.cpu().numpy())
            if bad.size:
                raise ValueError(f"star {labels[bad[0]][0]}, quarter {labels[bad[0]][1]}: the polynomial fit of order "
                                 f"{k} is singular (its time stamps do not determine it)")
        pairs = [(t2[int(off3_h[b]):int(off3_h[b + 1])], f2[int(off3_h[b]):int(off3_h[b + 1])]) for b in range(B)]
        if return_device:
            return pairs, [float(c) for c in cadence]
        t_h, f_h = t2.cpu().numpy(), f2.cpu().numpy()
    return [(t_h[off3_h[b]:off3_h[b + 1]].copy(), f_h[off3_h[b]:off3_h[b + 1]].copy(), float(cadence[b]))
            for b in range(B)]


def prepare_quarters(quarters, detrend_poly_order=3, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5,
                     fill=True, in_ppm=False, device=None, return_device=False):
    """
    Raw observing quarters of ONE star -> ``(times [d], flux_ppm, cadence [d])``, the series the reference's
    ``PowerSpectrum.from_light_curve(detrend=True)`` hands to its FFT (``fill=True``) or Lomb-Scargle
    (``fill=False``) estimate.  ``quarters``: list of ``(times, flux)`` pairs in chronological order, NaNs and
    outliers included.  Same shape as :func:`gadfly_amd.stitch_quarters`' result, and the same values on clean input
    (the time axis bit for bit; the flux to rounding, since the fit is solved in a Legendre basis on the device).

    Per quarter: rows with a non-finite time or flux are dropped; the sigma clip keeps
    ``med - sigma_lower sd <= f <= med + sigma_upper sd`` (median and population standard deviation of the
    survivors) round after round until a round removes nothing, ``maxiters`` rounds at most (``None``: no cap;
    ``sigma=None``: no clip; an unset ``sigma_lower`` / ``sigma_upper`` is ``sigma``); with ``fill`` the missing
    cadences are interpolated at ``dt = median(diff(t))``; unless ``in_ppm`` the least-squares polynomial of order
    ``detrend_poly_order`` (0..8) and then the median are divided out, ``1e6 (normed / median - 1)``.  The quarters
    are concatenated, with more than one and ``fill`` the gaps between them are filled, ``cadence`` is the median
    spacing of the result.  ``return_device=True`` returns float64 device tensors.

    Raises ``ValueError`` (naming star and quarter) for times that are not strictly increasing over the finite
    rows, a quarter that starts before the previous one ends, fewer than ``max(2, order + 1)`` surviving points,
    and for options out of range.  Parity with lightkurve's ``remove_outliers`` is unpinned (module docstring).
    """
    out = prepare_quarters_batch([quarters], detrend_poly_order, sigma, sigma_lower, sigma_upper, maxiters, fill,
                                 in_ppm, device, return_device)
    if return_device:
        (pair,), (cadence,) = out
        return pair[0], pair[1], cadence
    return out[0]
