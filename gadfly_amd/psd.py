"""
Observed power spectra on the device: ``PowerSpectrum`` (mirror of
/root/reference/gadfly/psd.py:364-650 for the FFT estimate and its binning).

This is the step *after* ``GaussianProcess.sample`` in the reference's own hot-path test
(/root/reference/gadfly/tests/test_core.py:29-34: ``PowerSpectrum(...).bin(...)`` of a draw is
compared with ``kernel.get_psd``) and SURVEY.md 8f rank 3.  The transform is hipFFT's (through
``torch.fft.rfft`` on the device tensor), ``gf_psd_power`` forms the normalised power
(psd.py:566-587) and ``gf_psd_bin`` the two binned statistics of ``bin_power_spectrum``
(psd.py:186-300) for all series of a batch in one launch.  Frequencies are in uHz, power in
ppm^2/uHz, sampling intervals in 1/uHz (= 1e6 s) -- gadfly's native units; astropy Quantities are
accepted where astropy is installed.

``PowerSpectrum.from_lomb_scargle`` (and ``from_light_curve(..., method='lomb-scargle')``) is the
reference's estimate for gapped, unevenly sampled photometry (psd.py:589-601, astropy's
``LombScargle(normalization='psd')`` on ``rfftfreq``'s grid) without astropy: ``gf_ls_power``
evaluates the floating-mean periodogram as the exact direct sum over every (point, frequency) pair
in float64, for one series, an (R, N) batch or a ragged list in one call.  Where astropy would pick
its approximate Press-Rybicki "fast" method (a regular grid of this size), this is the exact value
of the quantity that method approximates.  ``method="nufft"`` reaches the same seven sums in
O(n log n) through a non-uniform FFT (``gadfly_lsfft.hip``: spreading onto an oversampled grid, hipFFT,
deconvolution) and agrees with the direct sum within its own test bar.  Plotting stays with the reference.
"""
import numpy as np

from . import _lib
from . import units as _units

__all__ = ["PowerSpectrum", "bin_power_spectrum", "ls_grid"]


def _value(x, unit_name):
    """Strip an astropy unit (converted to gadfly's native one) if there is one."""
    if _units.has_unit(x):
        _units.require_astropy("a Quantity argument")
        u = _units.u
        target = {"uHz": u.uHz, "psd": u.cds.ppm ** 2 / u.uHz, "1/uHz": 1 / u.uHz,
                  "ppm": u.cds.ppm}[unit_name]
        return np.asarray(x.to(target).value, dtype=np.float64)
    return x


def _bin_starts(axis, bins):
    """Bin edges and index ranges on an ascending axis, with scipy.stats.binned_statistic's rules
    (what /root/reference/gadfly/psd.py:257-274 relies on): an integer means
    ``linspace(min, max, bins + 1)``; bins are half-open, the last edge is closed (scipy's rounding
    test).  Returns (edges, start) with bin b = ``axis[start[b]:start[b+1]]``."""
    if np.ndim(bins) == 0:
        if int(bins) < 1:
            raise ValueError("`bins` must be a positive integer or an array of edges")
        lo, hi = float(axis.min()), float(axis.max())
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        edges = np.linspace(lo, hi, int(bins) + 1)
    else:
        edges = np.asarray(bins, dtype=np.float64)
        if edges.ndim != 1 or len(edges) < 2 or np.any(np.diff(edges) < 0):
            raise ValueError("bin edges must be a monotonically increasing 1-D array")
    widths = np.diff(edges)
    if widths.min() == 0:
        raise ValueError("The smallest edge difference is numerically 0.")
    start = np.searchsorted(axis, edges, side="left").astype(np.int64)
    decimal = int(-np.log10(widths.min())) + 6
    on_edge = (axis >= edges[-1]) & (np.around(axis, decimal) == np.around(edges[-1], decimal))
    start[-1] += int(np.count_nonzero(on_edge))
    return edges, start


def ls_grid(n, d):
    """rfftfreq's frequency grid of an n-point series with step d [1/uHz]: (frequencies [uHz], df), bit for
    bit ``np.fft.rfftfreq(n, d)`` (``k * (1.0 / (n * d))`` in float64); the device forms the same products."""
    df = 1.0 / (n * d)
    return np.arange(n // 2 + 1, dtype=np.int64) * df, df


def _finite_1d(x, what):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or len(x) < 2:
        raise ValueError(f"{what} must be 1-D with at least 2 points (shape {x.shape})")
    if not np.all(np.isfinite(x)):
        raise ValueError(f"{what} holds NaN or Inf")
    return x


def _ls_d(t, d):
    if d is None:
        d = float(np.median(np.diff(t)))
    d = float(_value(d, "1/uHz"))
    if not (np.isfinite(d) and d > 0):
        raise ValueError(f"the sampling interval d must be finite and positive (d = {d})")
    return d


def _flux_rows(flux):
    """flux as given (device tensors stay on the device), its shape."""
    import torch
    if torch.is_tensor(flux):
        if flux.is_complex() or not flux.is_floating_point():
            raise ValueError("flux must be a real floating-point array")
        return flux, tuple(flux.shape)
    f = np.asarray(_value(flux, "ppm"), dtype=np.float64)
    if not np.all(np.isfinite(f)):
        raise ValueError("flux holds NaN or Inf")
    return f, f.shape


def _ls_series(t, flux, d):
    """Host-side validation and layout of from_lomb_scargle's inputs (no device call): a list of
    (t_r [numpy], flux_r [numpy or tensor], d_r) and one of "single", "batch", "list"."""
    if flux is None:
        if not isinstance(t, (list, tuple)) or len(t) == 0:
            raise ValueError("without `flux`, `t` must be a non-empty list of (t, flux) pairs")
        out = []
        for pair in t:
            if len(pair) != 2:
                raise ValueError("`t` must be a list of (t, flux) pairs")
            tr = _finite_1d(_value(pair[0], "1/uHz"), "t")
            fr, shape = _flux_rows(pair[1])
            if shape != tr.shape:
                raise ValueError(f"t {tr.shape} and flux {shape} of a pair differ in shape")
            out.append((tr, fr, _ls_d(tr, d)))
        return out, "list"
    t = np.asarray(_value(t, "1/uHz"), dtype=np.float64)
    f, shape = _flux_rows(flux)
    if len(shape) not in (1, 2) or shape[-1] < 2:
        raise ValueError(f"flux must have shape (N,) or (R, N) with N >= 2 (shape {shape})")
    if t.shape != shape and t.shape != shape[-1:]:
        raise ValueError(f"t {t.shape} must have shape (N,) or that of flux {shape}")
    if len(shape) == 1:
        tr = _finite_1d(t, "t")
        return [(tr, f, _ls_d(tr, d))], "single"
    if shape[0] < 1:
        raise ValueError("flux has no rows")
    rows = [_finite_1d(t if t.ndim == 1 else t[r], "t") for r in range(shape[0])]
    ds = [_ls_d(tr, d) for tr in rows]
    if any(x != ds[0] for x in ds):
        raise ValueError("the rows of t have different median steps: pass `d`, or a list of (t, flux) pairs")
    return [(rows[r], f[r], ds[r]) for r in range(shape[0])], "batch"


_LS_WORK_BUDGET = 1 << 27                  # doubles (1 GiB) of partial sums per launch


def _ls_groups(lib, counts, outs):
    """Consecutive runs of series [a, b) whose workspace fits the budget (at least one series each).  A
    series' result does not depend on its group: its segment count is a function of its own length."""
    groups, a = [], 0
    while a < len(counts):
        b, s_max = a + 1, lib.gf_ls_segments(int(counts[a]))
        while b < len(counts):
            s2 = max(s_max, lib.gf_ls_segments(int(counts[b])))
            if lib.gf_ls_work(int(counts[a:b + 1].sum()), int(outs[a:b + 1].sum()), s2) > _LS_WORK_BUDGET:
                break
            b, s_max = b + 1, s2
        groups.append((a, b))
        a = b
    return groups


_LS_METHODS = ("direct", "nufft")
_LSFFT_BUDGET = 1 << 30                    # bytes of fine grids plus their transforms per group of series
_LSFFT_QUAD = 64                           # Gauss-Legendre nodes of the kernel's transform (gadfly_lsfft.hip)


def _lsfft_groups(nfs, axis_ids):
    """Consecutive runs of series [a, b) whose fine grids and transforms (one pair per series, one more per
    distinct time axis of the run) stay under the budget; at least one series each."""
    groups, a = [], 0
    while a < len(nfs):
        b, used, seen = a, 0, set()
        while b < len(nfs):
            cost = (16 * int(nfs[b]) + 16) * (1 if axis_ids[b] in seen else 2)
            if b > a and used + cost > _LSFFT_BUDGET:
                break
            used += cost
            seen.add(axis_ids[b])
            b += 1
        groups.append((a, b))
        a = b
    return groups


def _lsfft_layout(ts, dfs, nfs, outs):
    """Offsets of one group of series for ``gf_lsfft_*`` (include/gadfly_hip.h).  Series that are given the same
    time array share an axis: its wrap, its sort and its grid of ones.  Grids of equal n_f lie together (the ones
    of the class' axes, then its series), so that one batched rfft transforms a class.  Returns (A, integer
    offsets by name, df per axis, times of the axes, [(grid offset, transform offset, grids, n_f)] per class)."""
    R = len(ts)
    index, axis, ax_t, ax_df, ax_nf, owner = {}, [], [], [], [], []
    for r, tr in enumerate(ts):
        if id(tr) not in index:
            index[id(tr)] = len(ax_t)
            ax_t.append(tr)
            ax_df.append(dfs[r])
            ax_nf.append(int(nfs[r]))
            owner.append(r)
        axis.append(index[id(tr)])
    A = len(ax_t)
    gy, g1, sy, s1 = np.zeros(R, np.int64), np.full(R, -1, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    g1_axis, s1_axis = np.zeros(A, np.int64), np.zeros(A, np.int64)
    classes, g, c = [], 0, 0
    for nf in sorted(set(ax_nf)):
        m, g0, c0, cnt = nf // 2 + 1, g, c, 0
        for a in range(A):
            if ax_nf[a] == nf:
                g1_axis[a], s1_axis[a] = g, c
                g, c, cnt = g + nf, c + m, cnt + 1
        for r in range(R):
            if ax_nf[axis[r]] == nf:
                gy[r], sy[r] = g, c
                g, c, cnt = g + nf, c + m, cnt + 1
        classes.append((g0, c0, cnt, nf))
    for a in range(A):
        g1[owner[a]] = g1_axis[a]
    s1[:] = s1_axis[axis]
    cum = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.int64)        # noqa: E731
    off = dict(ax_off=cum([len(x) for x in ax_t]), cell_off=cum(ax_nf), pt_off=cum([len(x) for x in ts]),
               out_off=cum(outs), axis=np.asarray(axis, np.int64), gy_off=gy, g1_off=g1, sy_off=sy, s1_off=s1)
    return A, off, np.asarray(ax_df, np.float64), ax_t, classes


def _ls_nufft(lib, series, grids, norms, outs, out_off, pt_all, first, y_all, power, dev):
    """The non-uniform FFT route of from_lomb_scargle: per group of series prepare (wrap, centre,
    cell keys), a stable sort of the keys, the gather-spread, one batched rfft per grid size, the finish."""
    import torch
    st = torch.cuda.current_stream(dev).cuda_stream
    nfs = [int(lib.gf_lsfft_grid(len(tr))) for tr, _, _ in series]
    z, wq = np.polynomial.legendre.leggauss(_LSFFT_QUAD)
    quad = np.concatenate([0.5 * (z + 1.0), 0.5 * wq])                          # nodes, weights on [0, 1]
    for a, b in _lsfft_groups(nfs, [id(tr) for tr, _, _ in series]):
        ts = [tr for tr, _, _ in series[a:b]]
        A, off, df, ax_t, classes = _lsfft_layout(ts, [g[1] for g in grids[a:b]], nfs[a:b], outs[a:b])
        R, n_axes, cells = b - a, int(off["ax_off"][-1]), int(off["cell_off"][-1])
        names = list(off)
        meta_i = torch.as_tensor(np.concatenate([off[k] for k in names]), device=dev)
        at, o = {}, 0
        for k in names:
            at[k] = _lib.ptr(meta_i[o:]) if len(off[k]) else None
            o += len(off[k])
        meta_d = torch.as_tensor(np.concatenate([df, np.asarray(norms[a:b], np.float64), quad]), device=dev)
        t_ax = torch.as_tensor(np.concatenate(ax_t), device=dev)
        y = y_all[int(pt_all[a]):int(pt_all[b])]
        key = torch.empty(n_axes, dtype=torch.int64, device=dev)
        u = torch.empty(n_axes, dtype=torch.float64, device=dev)
        yc = torch.empty_like(y)
        part = torch.empty(int(lib.gf_lsfft_part(R)), dtype=torch.float64, device=dev)
        n_max = max(len(tr) for tr in ts)
        _lib.check(lib.gf_lsfft_prepare(A, R, n_max, at["ax_off"], at["cell_off"], _lib.ptr(meta_d), at["pt_off"],
                                        _lib.ptr(t_ax), _lib.ptr(y), _lib.ptr(key), _lib.ptr(u), _lib.ptr(yc),
                                        _lib.ptr(part), st),
                   "gf_lsfft_prepare")
        skey, perm = torch.sort(key, stable=True)
        start = torch.empty(cells + 1, dtype=torch.int64, device=dev)
        n_grid = sum(cnt * nf for _, _, cnt, nf in classes)
        n_spec = sum(cnt * (nf // 2 + 1) for _, _, cnt, nf in classes)
        grid = torch.empty(n_grid, dtype=torch.float64, device=dev)
        _lib.check(lib.gf_lsfft_spread(A, R, n_axes, cells, max(nfs[a:b]), at["ax_off"], at["cell_off"], at["pt_off"],
                                       at["axis"], at["gy_off"], at["g1_off"], _lib.ptr(skey), _lib.ptr(perm),
                                       _lib.ptr(u), _lib.ptr(yc), _lib.ptr(start), _lib.ptr(grid), st),
                   "gf_lsfft_spread")
        del start, skey, perm, key
        spec = torch.empty(n_spec, dtype=torch.complex128, device=dev)
        for g0, c0, cnt, nf in classes:
            m = nf // 2 + 1
            torch.fft.rfft(grid[g0:g0 + cnt * nf].view(cnt, nf), dim=-1, out=spec[c0:c0 + cnt * m].view(cnt, m))
        _lib.check(lib.gf_lsfft_finish(R, n_max, first, at["pt_off"], at["out_off"], at["axis"], at["cell_off"],
                                       at["sy_off"], at["s1_off"], _lib.ptr(meta_d[A:]), _lib.ptr(meta_d[A + R:]),
                                       _lib.ptr(spec), _lib.ptr(power[int(out_off[a]):]), st), "gf_lsfft_finish")


class PowerSpectrum:
    """
    An observed power spectrum (reference psd.py:364-396): ``frequency`` [uHz], ``power``
    [ppm^2/uHz] (shape (M,), or (R, M) for a batch of R series sharing the frequency axis),
    optional ``error``, ``name``, ``norm`` and ``detrended_lc``.  ``counts``: the number of ordinates averaged into
    each point of a binned spectrum (set by :func:`bin_power_spectrum`), None on an unbinned one.
    """

    def __init__(self, frequency, power, error=None, name=None, norm=None, detrended_lc=None):
        self.frequency = np.asarray(_value(frequency, "uHz"), dtype=np.float64)
        self.power = _value(power, "psd")
        self.error = None if error is None else _value(error, "psd")
        self.name = name
        self.norm = norm
        self.detrended_lc = detrended_lc
        self.counts = None
        self._power_dev = None              # device copy of `power` when it was made there

    @property
    def omega(self):
        """Angular frequency 2 pi f, f in uHz (reference psd.py:397-409)."""
        return 2 * np.pi * self.frequency

    @property
    def light_curve_rms(self):
        """Approximate rms of the light curve [ppm] (reference psd.py:411-421)."""
        return (np.asarray(self.power) * self.norm) ** 0.5

    def bin(self, bins=None, **kwargs):
        """Binned power spectrum (reference psd.py:423-441)."""
        return bin_power_spectrum(self, bins, **kwargs)

    def cutout(self, frequency_min=None, frequency_max=None):
        """Measurements with frequency_min <= f <= frequency_max (reference psd.py:611-650)."""
        lo = 0.0 if frequency_min is None else float(_value(frequency_min, "uHz"))
        hi = np.inf if frequency_max is None else float(_value(frequency_max, "uHz"))
        keep = (self.frequency <= hi) & (self.frequency >= lo)
        name = (self.name if self.name is not None else "Power spectrum") + " (cutout)"
        args = []
        if self.error is not None:
            args.append(np.asarray(self.error)[..., keep])
        return PowerSpectrum(self.frequency[keep], np.asarray(self.power)[..., keep], *args,
                             name=name, norm=self.norm)

    def plot(self, **kwargs):
        raise NotImplementedError(
            "plotting is outside the GP hot path (gadfly/psd.py:36-183 is left as-is)")

    # ------------------------------------------------------------------------------------
    @classmethod
    def from_flux(cls, flux, d, include_zero_freq=False, name=None, device=None):
        """FFT power spectrum of evenly sampled fluxes [ppm], sampling interval ``d`` [1/uHz].

        ``flux`` is (N,) or (R, N): a numpy array, or a float64 tensor already on the device
        (e.g. draws that never left it).  Same estimate as ``PowerSpectrum._fft``
        (reference psd.py:566-587) with the zero frequency dropped unless asked for
        (psd.py:559-561); everything after the upload runs on the GPU.
        """
        import torch
        lib = _lib.load()
        d = float(_value(d, "1/uHz"))
        if torch.is_tensor(flux):
            x = flux.to(dtype=torch.float64)
            if not x.is_cuda:
                x = x.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        else:
            flux = np.ascontiguousarray(_value(flux, "ppm"), dtype=np.float64)
            dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
            x = torch.as_tensor(flux, device=dev)
        if x.ndim not in (1, 2) or x.shape[-1] < 2:
            raise ValueError("flux must have shape (N,) or (R, N) with N >= 2")
        single = x.ndim == 1
        x2 = x.reshape(1, -1) if single else x.contiguous()
        R, N = x2.shape
        with torch.cuda.device(x2.device):
            spec = torch.view_as_real(torch.fft.rfft(x2, dim=-1)).contiguous()     # (R, M, 2)
            M = spec.shape[1]
            first = 0 if include_zero_freq else 1
            norm = d / (2 * np.pi) ** 0.5 / N
            power = torch.empty((R, M - first), dtype=torch.float64, device=x2.device)
            st = torch.cuda.current_stream(x2.device).cuda_stream
            _lib.check(lib.gf_psd_power(R, M, first, norm, _lib.ptr(spec), _lib.ptr(power), st),
                       "gf_psd_power")
        freq = np.fft.rfftfreq(N, d)[first:]
        host = power.cpu().numpy()
        ps = cls(freq, host[0] if single else host, name=name, norm=norm)
        ps._power_dev = power
        return ps

    @classmethod
    def from_lomb_scargle(cls, t, flux=None, d=None, include_zero_freq=False, name=None, device=None,
                          method="direct"):
        """Lomb-Scargle power spectrum of unevenly sampled (gapped) fluxes [ppm] at times ``t`` [1/uHz].

        The reference's ``PowerSpectrum._lomb_scargle`` (psd.py:589-601): astropy's floating-mean
        ``LombScargle(t, flux, normalization='psd').power(rfftfreq(N, d))`` times ``norm = d / sqrt(2 pi)``,
        ``d`` the median time step unless given, the zero frequency dropped unless asked for
        (psd.py:559-561).  Evaluated exactly (direct sum in float64) by ``gf_ls_power``; astropy's
        ``method='auto'`` would use its approximate Press-Rybicki method on such a grid instead
        (DESIGN.md 3.6).  Accepted shapes:

        * ``t`` (N,), ``flux`` (N,)              -> one spectrum, power (M,)
        * ``t`` (N,), ``flux`` (R, N)            -> power (R, M) on one frequency axis
        * ``t`` (R, N), ``flux`` (R, N)          -> power (R, M); every row must have the same ``d``
          (or ``d`` given), so that the rows share the frequency axis
        * ``t`` a list of ``(t_r, flux_r)`` pairs (any lengths), ``flux`` None -> a list of spectra

        ``flux`` may be a float64 tensor already on the device (e.g. a ``sample_device`` draw); the
        result keeps the device copy of the power, so ``.bin()`` stays on the GPU.

        ``method="direct"`` is the exact sum, n^2 / 2 pair evaluations.  ``method="nufft"`` forms the same sums in
        O(n log n) (``gf_lsfft_*``: a kernel of 16 cells on a twice oversampled grid, hipFFT, deconvolution;
        DESIGN.md 3.6.1) and agrees with it to rtol 1e-8, atol 1e-10 max(power), the direct route's own test bar
        (but for frequencies at which the fit is nearly rank one, where its 1e-13 is amplified as rounding is);
        series that are given the same time array share its sort and its grid of ones.  The same call is
        bit-identical from run to run; a series in a batch agrees with the same series alone to 1e-12 max(power).
        """
        import torch
        if method not in _LS_METHODS:
            raise ValueError(f'from_lomb_scargle was given method="{method}", but it must be one of: '
                             f"{list(_LS_METHODS)} (the exact direct sum, or the non-uniform FFT).")
        series, layout = _ls_series(t, flux, d)
        lib = _lib.load()
        first = 0 if include_zero_freq else 1
        dev = device
        for _, y, _ in series:
            if torch.is_tensor(y) and y.is_cuda:
                dev = y.device
                break
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        dev = torch.device(dev)
        grids = [ls_grid(len(tr), dr) for tr, _, dr in series]
        norms = [dr / (2 * np.pi) ** 0.5 for _, _, dr in series]
        counts = np.array([len(tr) for tr, _, _ in series], dtype=np.int64)
        outs = counts // 2 + 1 - first
        out_off = np.concatenate([[0], np.cumsum(outs)]).astype(np.int64)
        with torch.cuda.device(dev):
            ys = []
            for _, y, _ in series:
                yd = y.to(device=dev, dtype=torch.float64) if torch.is_tensor(y) else \
                    torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64), device=dev)
                ys.append(yd.reshape(-1))
            y_all = torch.cat(ys).contiguous()
            if not bool(torch.isfinite(y_all).all()):
                raise ValueError("flux holds NaN or Inf")
            power = torch.empty(int(out_off[-1]), dtype=torch.float64, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            pt_all = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            if method == "nufft":
                _ls_nufft(lib, series, grids, norms, outs, out_off, pt_all, first, y_all, power, dev)
                groups = []
            else:
                t_all = torch.as_tensor(np.concatenate([tr for tr, _, _ in series]), device=dev)
                groups = _ls_groups(lib, counts, outs)
            for a, b in groups:
                n = counts[a:b]
                pt = pt_all[a:b + 1] - pt_all[a]
                oo = out_off[a:b + 1] - out_off[a]
                s_max = max(lib.gf_ls_segments(int(x)) for x in n)
                work = torch.empty(int(lib.gf_ls_work(int(pt[-1]), int(oo[-1]), s_max)) + 4,
                                   dtype=torch.float64, device=dev)
                w = work[(-work.data_ptr() // 8) % 4:]                     # 32-byte aligned
                meta_i = torch.as_tensor(np.concatenate([pt, oo]), device=dev)
                meta_d = torch.as_tensor(np.array([g[1] for g in grids[a:b]] + norms[a:b],
                                                  dtype=np.float64), device=dev)
                _lib.check(lib.gf_ls_power(
                    b - a, int(n.max()), int(pt[-1]), int(oo[-1]), s_max, first,
                    _lib.ptr(meta_i), _lib.ptr(meta_i[b - a + 1:]), _lib.ptr(meta_d),
                    _lib.ptr(meta_d[b - a:]), _lib.ptr(t_all[int(pt_all[a]):]), _lib.ptr(y_all[int(pt_all[a]):]),
                    _lib.ptr(w), _lib.ptr(power[int(out_off[a]):]), st), "gf_ls_power")
            host = power.cpu().numpy()
        spectra = []
        for r in range(len(series)):
            p_dev = power[int(out_off[r]):int(out_off[r + 1])].view(1, -1)
            ps = cls(grids[r][0][first:], host[out_off[r]:out_off[r + 1]], name=name, norm=norms[r])
            ps._power_dev = p_dev
            spectra.append(ps)
        if layout == "list":
            return spectra
        if layout == "single":
            return spectra[0]
        R, m = len(series), int(outs[0])
        ps = cls(grids[0][0][first:], host.reshape(R, m), name=name, norm=norms[0])
        ps._power_dev = power.view(R, m)
        return ps

    @classmethod
    def from_light_curve(cls, light_curve, method="fft", include_zero_freq=False, name=None,
                         detrend=False, **kwargs):
        """Power spectrum of a light-curve-like object (``.time`` [days or Time], ``.flux`` [ppm]).

        The ``detrend=False`` branch of the reference (psd.py:537-563) on an already normalised
        light curve: ``method='fft'`` for an evenly sampled one, ``method='lomb-scargle'`` (the
        time axis ``jd * day`` in 1/uHz, see :meth:`from_lomb_scargle`; ``ls_method="nufft"`` picks its
        non-uniform FFT route) for a gapped one.
        Detrending / gap interpolation (psd.py:474-535) works on lightkurve objects there; on plain arrays it is
        :meth:`from_quarters`.
        """
        if method.lower() not in ("fft", "lomb-scargle"):
            raise ValueError(f'PowerSpectrum.from_lightcurve was given method="{method}", but it '
                             "must be one of: ['fft', 'lomb-scargle'].")
        if detrend:
            raise NotImplementedError(
                "only detrend=False runs on the device for light-curve objects (reference psd.py:474-535 needs "
                "lightkurve); PowerSpectrum.from_quarters detrends raw (times, flux) arrays")
        time = light_curve.time
        jd = np.asarray(getattr(time, "jd", time), dtype=np.float64)
        meta = getattr(light_curve, "meta", None) or {}
        if method.lower() == "lomb-scargle":
            t = jd * 86400.0 / _units.SECONDS_PER_INVERSE_UHZ
            return cls.from_lomb_scargle(t, light_curve.flux, include_zero_freq=include_zero_freq,
                                         name=meta.get("name", name), method=kwargs.get("ls_method", "direct"))
        d = np.median(np.diff(jd)) * 86400.0 / _units.SECONDS_PER_INVERSE_UHZ
        return cls.from_flux(light_curve.flux, d, include_zero_freq=include_zero_freq,
                             name=meta.get("name", name))

    @classmethod
    def from_quarters(cls, quarters, method="fft", include_zero_freq=False, name=None, ls_method="direct",
                      **prepare_kwargs):
        """Power spectrum of one star's raw observing quarters, a list of ``(times [d], flux)`` pairs: the
        ``detrend=True`` branch of the reference (psd.py:482-564) on plain arrays.  The quarters are clipped,
        detrended and stitched by :func:`gadfly_amd.prepare_quarters` (``prepare_kwargs``: its options but ``fill``)
        -- gap-filled for ``method='fft'``, left gapped for ``method='lomb-scargle'`` (time axis ``jd * day`` in
        1/uHz as in :meth:`from_light_curve`; ``ls_method`` picks :meth:`from_lomb_scargle`'s route).
        ``detrended_lc`` is ``(times [d], flux_ppm)``."""
        from .detrend import prepare_quarters
        if method.lower() not in ("fft", "lomb-scargle"):
            raise ValueError(f'PowerSpectrum.from_quarters was given method="{method}", but it '
                             "must be one of: ['fft', 'lomb-scargle'].")
        if "fill" in prepare_kwargs or "return_device" in prepare_kwargs:
            raise TypeError("from_quarters sets fill from the method and returns host arrays")
        fft = method.lower() == "fft"
        jd, flux, cadence = prepare_quarters(quarters, fill=fft, **prepare_kwargs)
        device = prepare_kwargs.get("device")
        if fft:
            d = cadence * 86400.0 / _units.SECONDS_PER_INVERSE_UHZ
            ps = cls.from_flux(flux, d, include_zero_freq=include_zero_freq, name=name, device=device)
        else:
            t = jd * 86400.0 / _units.SECONDS_PER_INVERSE_UHZ
            ps = cls.from_lomb_scargle(t, flux, include_zero_freq=include_zero_freq, name=name, device=device,
                                       method=ls_method)
        ps.detrended_lc = (jd, flux)
        return ps


def bin_power_spectrum(power_spectrum, bins=None, log=True, constant=1, device=None):
    """
    Bin a power spectrum into (by default log-spaced) frequency bins
    (reference psd.py:229-297): per bin the trapezoid mean of the power over the bin's span and
    the error estimate std / sqrt(n) * mean_x / span / constant (psd.py:186-227), for every
    series of the batch in one ``gf_psd_bin`` launch.  Returns a new :class:`PowerSpectrum`
    at the bin centres.
    """
    import torch
    lib = _lib.load()
    freq = np.asarray(power_spectrum.frequency, dtype=np.float64)
    if np.any(np.diff(freq) < 0):
        raise ValueError("the frequencies of the power spectrum must be sorted")
    axis = np.log10(freq) if log else freq
    if bins is None:
        bins = len(axis) // 10000
    edges, start = _bin_starts(axis, bins)
    nb = len(edges) - 1

    power = power_spectrum._power_dev
    if power is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        power = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(power_spectrum.power),
                                                     dtype=np.float64), device=dev)
    R, M = power.shape
    if M != len(axis):
        raise ValueError("dimension mismatch")
    with torch.cuda.device(power.device):
        x_d = torch.as_tensor(axis, device=power.device)
        s_d = torch.as_tensor(start, device=power.device)
        stat = torch.empty((R, nb), dtype=torch.float64, device=power.device)
        err = torch.empty_like(stat)
        st = torch.cuda.current_stream(power.device).cuda_stream
        _lib.check(lib.gf_psd_bin(R, M, nb, _lib.ptr(x_d), _lib.ptr(power), _lib.ptr(s_d),
                                  float(constant), _lib.ptr(stat), _lib.ptr(err), st), "gf_psd_bin")
        stat_h, err_h = stat.cpu().numpy(), err.cpu().numpy()
    mid = 0.5 * (edges[1:] + edges[:-1])
    centers = 10 ** mid if log else mid
    single = np.ndim(power_spectrum.power) == 1
    name = (power_spectrum.name if power_spectrum.name is not None else "Power spectrum") + " (binned)"
    binned = PowerSpectrum(centers, stat_h[0] if single else stat_h,
                           err_h[0] if single else err_h, name=name)
    binned.counts = np.diff(start)          # ordinates per bin (the Whittle weights of a binned spectrum)
    return binned
