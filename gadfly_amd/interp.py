"""
``interpolate_missing_data`` on the device (mirror of /root/reference/gadfly/interp.py:6-60):
fill the missing cadences of an otherwise evenly sampled light curve by linear interpolation --
what the reference does before every FFT power spectrum (psd.py:495, :531).
The cadence statistic (a median) is taken on the host from the arrays the caller hands over; the
gap search, the prefix sum over the gaps and the fill run on the GPU (``gf_interp_plan``,
``gf_interp_fill``) and reproduce numpy's results bit for bit.  ``interpolate_missing_data_batch`` fills many
series in one call over one offset table (``gf_interp_plan_seg``, ``gf_interp_fill_seg``): the cadences are medians
taken on the device, and the only read-back is that of the filled series' offsets.
"""
import numpy as np

from . import _lib

__all__ = ["interpolate_missing_data", "interpolate_missing_data_batch", "stitch_quarters"]


def interpolate_missing_data(times, fluxes, cadences=None, device=None, return_device=False):
    """
    Assuming ``times`` are uniformly spaced with missing cadences, fill in the missing cadences
    with linear interpolation; ``cadences`` (integer cadence numbers) can be passed if known.
    Returns (interpolated_times, interpolated_fluxes) as numpy arrays, or as float64 device
    tensors with ``return_device=True`` (e.g. for :meth:`gadfly_amd.PowerSpectrum.from_flux`).
    """
    import torch
    lib = _lib.load()
    times = np.ascontiguousarray(times, dtype=np.float64)
    fluxes = np.ascontiguousarray(fluxes, dtype=np.float64)
    if times.ndim != 1 or times.shape != fluxes.shape or times.size < 2:
        raise ValueError("dimension mismatch")
    if np.any(np.diff(times) <= 0):
        raise ValueError("times must be strictly increasing")
    if cadences is None:
        dt = float(np.median(np.diff(times)))                       # reference interp.py:40
        cad = None
    else:
        cad = np.ascontiguousarray(cadences, dtype=np.int64)
        if cad.shape != times.shape:
            raise ValueError("dimension mismatch")
        dt = float(np.median(np.diff(times) / np.diff(cad)))        # reference interp.py:36
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = times.size
    with torch.cuda.device(dev):
        t_d = torch.as_tensor(times, device=dev)
        f_d = torch.as_tensor(fluxes, device=dev)
        c_d = None if cad is None else torch.as_tensor(cad, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        work = torch.empty(max(1, int(lib.gf_interp_work(n))), dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        cp = None if c_d is None else _lib.ptr(c_d)
        _lib.check(lib.gf_interp_plan(n, _lib.ptr(t_d), cp, dt, _lib.ptr(offsets), _lib.ptr(work), st),
                   "gf_interp_plan")
        total = int(offsets[n].item())
        t_out = torch.empty(total, dtype=torch.float64, device=dev)
        f_out = torch.empty(total, dtype=torch.float64, device=dev)
        _lib.check(lib.gf_interp_fill(n, _lib.ptr(t_d), _lib.ptr(f_d), cp, dt, _lib.ptr(offsets),
                                      _lib.ptr(t_out), _lib.ptr(f_out), st), "gf_interp_fill")
        if return_device:
            return t_out, f_out
        return t_out.cpu().numpy(), f_out.cpu().numpy()


def _batch_input(times, fluxes, cadences):
    """The checks of :func:`interpolate_missing_data_batch` that need no device.  -> (times, fluxes, cadences or
    None, lengths, on_device); host series come back as contiguous float64 / int64 arrays."""
    import torch
    S = len(times)
    if S < 1:
        raise ValueError("no series")
    if len(fluxes) != S or (cadences is not None and len(cadences) != S):
        raise ValueError(f"{S} time axes, {len(fluxes)} flux series"
                         + ("" if cadences is None else f", {len(cadences)} cadence series")
                         + ": the lists must have one length")
    resident = [isinstance(x, torch.Tensor) and x.is_cuda for x in list(times) + list(fluxes)]
    on_device = all(resident)
    if any(resident) and not on_device:
        raise ValueError("times and fluxes must be all host arrays or all device tensors")
    ts, fs, cs = [], [], (None if cadences is None else [])
    for s in range(S):
        t, f = times[s], fluxes[s]
        if on_device:
            if t.dtype != torch.float64 or f.dtype != torch.float64:
                raise ValueError(f"series {s}: device tensors must be float64")
        else:
            t = np.ascontiguousarray(t, dtype=np.float64)
            f = np.ascontiguousarray(f, dtype=np.float64)
        if t.ndim != 1 or tuple(t.shape) != tuple(f.shape):
            raise ValueError(f"series {s}: dimension mismatch")
        if t.shape[0] < 2:
            raise ValueError(f"series {s}: {t.shape[0]} points, 2 are needed")
        if not on_device and not np.all(np.isfinite(t)):
            raise ValueError(f"series {s}: times must be finite")
        if not on_device and np.any(np.diff(t) <= 0):
            raise ValueError(f"series {s}: times must be strictly increasing")
        if cs is not None:
            c = np.ascontiguousarray(cadences[s].cpu() if isinstance(cadences[s], torch.Tensor) else cadences[s],
                                     dtype=np.int64)
            if c.shape != tuple(t.shape):
                raise ValueError(f"series {s}: dimension mismatch")
            cs.append(c)
        ts.append(t)
        fs.append(f)
    return ts, fs, cs, [int(t.shape[0]) for t in ts], on_device


def interpolate_missing_data_batch(times, fluxes, cadences=None, device=None, return_device=False):
    """
    :func:`interpolate_missing_data` of S series of any lengths >= 2 in one device call: ``times`` and ``fluxes`` are
    lists of S 1-D host arrays, or of float64 tensors already on the device (finite, strictly increasing times: only
    host arrays can be checked without a read-back); ``cadences`` is None or a list of S int64 arrays.  Returns a
    list of S ``(times, fluxes)`` pairs of numpy arrays, or with ``return_device=True`` of float64 device tensors
    that are views of one allocation.  Series ``s`` of the result is, bit for bit, what the single call returns for
    it, alone or inside any batch.

    One upload of the concatenation, a fixed number of launches (``gf_seg_diff`` + ``gf_seg_median`` for the S
    cadences where no cadence numbers are given, ``gf_interp_plan_seg``, ``gf_interp_fill_seg``) and one
    synchronising read-back of the S + 1 offsets of the filled series.  With cadence numbers ``dt`` is formed on the
    host as the single call forms it (device time axes are copied back once for that).

    Raises ``ValueError`` naming the series: before any device work for lists of different lengths, a series
    shorter than 2, mismatched shapes and (host arrays) times that are not finite or not strictly increasing; after
    the read-back where a series' cadence is not a positive finite number or (device tensors) a time is not finite.
    """
    import torch
    ts, fs, cs, n, on_device = _batch_input(times, fluxes, cadences)
    S = len(n)
    off_h = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    total = int(off_h[-1])
    dt_h = None
    if cs is not None:                                              # reference interp.py:36
        dt_h = np.asarray([np.median(np.diff(t.cpu().numpy() if on_device else t) / np.diff(c))
                           for t, c in zip(ts, cs)], dtype=np.float64)
    _lib.require_device()
    lib = _lib.load()
    if device is not None:
        dev = torch.device(device)
    elif on_device:
        dev = ts[0].device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        # ONE upload: every part is 8 bytes per element -- [t | f] (host series), off, cadences, dt
        parts = ([] if on_device else [np.concatenate(ts), np.concatenate(fs)]) + [off_h.view(np.float64)]
        if cs is not None:
            parts += [np.concatenate(cs).view(np.float64), dt_h]
        sizes = np.cumsum([0] + [p.size for p in parts])
        up = torch.as_tensor(np.concatenate(parts), device=dev)
        cut = [up[sizes[k]:sizes[k + 1]] for k in range(len(parts))]
        if on_device:
            t_d, f_d = torch.cat([t.to(dev) for t in ts]), torch.cat([f.to(dev) for f in fs])
        else:
            t_d, f_d = cut[0], cut[1]
            cut = cut[2:]
        off = cut[0].view(torch.int64)
        c_d = None if cs is None else cut[1].view(torch.int64)
        st = torch.cuda.current_stream(dev).cuda_stream
        if cs is None:                                              # median(diff(t)), reference interp.py:40
            dt = torch.empty(S, dtype=torch.float64, device=dev)
            d = torch.empty(total, dtype=torch.float64, device=dev)
            _lib.check(lib.gf_seg_diff(S, _lib.ptr(off), _lib.ptr(t_d), _lib.ptr(d), st), "gf_seg_diff")
            _lib.check(lib.gf_seg_median(S, _lib.ptr(off), _lib.ptr(d), None, 1, _lib.ptr(dt), st), "gf_seg_median")
        else:
            dt = cut[2]
        finite = torch.isfinite(t_d).all().to(torch.int64).reshape(1) if on_device else None
        new_off_h, _, t_out, f_out = _fill_segments(lib, dev, st, S, total, off, t_d, f_d, c_d, dt, None,
                                                    lambda s: f"series {s}", finite)
        if not return_device:
            t_out, f_out = t_out.cpu().numpy(), f_out.cpu().numpy()
        pairs = [(t_out[new_off_h[s]:new_off_h[s + 1]], f_out[new_off_h[s]:new_off_h[s + 1]]) for s in range(S)]
    return pairs if return_device else [(t.copy(), f.copy()) for t, f in pairs]


def _fill_segments(lib, dev, st, S, total, off, t, f, cad, dt, which, name, finite=None):
    """``gf_interp_plan_seg``, ONE read-back (the S + 1 new offsets and the S flags in one int64 array), then
    ``gf_interp_fill_seg`` into one allocation.  Every array argument is a tensor on ``dev``; ``name(s)`` names
    segment s in the error for a cadence that is not positive.  ``finite``: None, or one int64 on the device that
    is 0 where the times were not checked on the host and are not all finite; it travels with the same read-back
    (the fill's searches for a grid time need finite times to end).
    -> (new host offsets, new device offsets, t, f)"""
    import torch
    plan = torch.empty(total + 1, dtype=torch.int64, device=dev)
    work = torch.empty(max(1, int(lib.gf_interp_seg_work(total))), dtype=torch.int64, device=dev)
    words = S + 1 + (S + 1) // 2                                    # new offsets [S + 1], info [S] int32, finite
    meta = torch.empty(words + 1, dtype=torch.int64, device=dev)
    new_off, info = meta[:S + 1], meta[S + 1:words].view(torch.int32)[:S]
    if finite is not None:
        meta[words:] = finite
    _lib.check(lib.gf_interp_plan_seg(S, total, _lib.ptr(off), _lib.ptr(t), _lib.ptr(cad), _lib.ptr(dt),
                                      _lib.ptr(which), _lib.ptr(plan), _lib.ptr(new_off), _lib.ptr(info),
                                      _lib.ptr(work), st), "gf_interp_plan_seg")
    meta_h = meta.cpu().numpy()
    new_off_h = meta_h[:S + 1]
    if finite is not None and not meta_h[words]:
        raise ValueError("times must be finite")
    bad = np.flatnonzero(meta_h[S + 1:words].view(np.int32)[:S])
    if bad.size:
        raise ValueError(f"{name(int(bad[0]))}: the cadence is not a positive finite number")
    n_out = int(new_off_h[-1])
    f_at = (n_out + 31) // 32 * 32                                  # the fluxes start on a 256-byte boundary too
    out = torch.empty(f_at + n_out, dtype=torch.float64, device=dev)
    t_out, f_out = out[:n_out], out[f_at:]
    _lib.check(lib.gf_interp_fill_seg(S, total, _lib.ptr(off), _lib.ptr(t), _lib.ptr(f), _lib.ptr(cad),
                                      _lib.ptr(dt), _lib.ptr(which), _lib.ptr(plan), _lib.ptr(t_out),
                                      _lib.ptr(f_out), st), "gf_interp_fill_seg")
    return new_off_h, new_off, t_out, f_out


def stitch_quarters(quarters, detrend_poly_order=3, in_ppm=False, device=None):
    """
    Several observing quarters of one star -> ONE gap-filled series in ppm, the way the reference prepares a
    ``LightCurveCollection`` (/root/reference/gadfly/psd.py:483-531): per quarter fill the missing cadences
    (:func:`interpolate_missing_data`), divide by a polynomial of order ``detrend_poly_order`` in ``t - mean(t)`` and
    by the median of the result, ``1e6 (f / median - 1)`` (skipped when the fluxes are in ppm already,
    ``in_ppm=True``); concatenate the quarters in the order given, which must be chronological (lightkurve's
    ``stitch(lambda x: x)``); fill the gaps
    BETWEEN the quarters the same way.  ``quarters``: list of (times [d], fluxes) pairs, NaNs and outliers already
    removed (``remove_nans().remove_outliers()`` is lightkurve's, outside this path).  Returns
    ``(times, flux_ppm, cadence)`` with cadence = median spacing (psd.py:534).  The gap filling runs on the device;
    the O(N) polynomial fit on the host, as numpy does it in the reference.
    """
    ts, fs = [], []
    for t, f in quarters:
        t, f = interpolate_missing_data(t, f, device=device)
        if not in_ppm:
            x = t - t.mean()
            fit = np.polyval(np.polyfit(x, f, detrend_poly_order), x)
            normed = f / fit
            f = 1e6 * np.array(normed / np.median(normed) - 1)
        ts.append(t)
        fs.append(f)
    t = np.concatenate(ts)                          # (lightkurve's stitch keeps the collection's order)
    f = np.concatenate(fs)
    if len(ts) > 1:
        t, f = interpolate_missing_data(t, f, device=device)
    return t, f, float(np.median(np.diff(t)))
