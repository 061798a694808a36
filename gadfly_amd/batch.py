"""
Batched log-likelihood front-end: B independent evaluations on one GPU.

One "evaluation" is what BASELINE.json's metric counts: for fresh
hyperparameters, ``compute`` (matrix build + factor, /root/reference/gadfly/gp.py:202) followed
by ``log_likelihood`` (forward solve + reductions, gp.py:350).  Here the factor and the
forward solve share one sweep and nothing returns to the host until the B scalars are read.

Batch shapes:
  * walkers      : shared t, y; one kernel (hyperparameter set) per walker;
  * light curves : own t, y (and kernel) per problem -- a (B, N) array when the series share N, or a LIST of B
                   series of different lengths (real Kepler quarters, /root/reference/gadfly/core.py:509-512,
                   psd.py:483-531): every series is then extended to the longest one with MISSING-DATA rows -- its
                   own cadence continued, y = 0 and the diagonal PAD_DIAG = 2^1000.  Such a row has the pivot 2^1000
                   exactly, the gain 2^-1000 (no trace in the state at double precision) and z^2 / d of order 2^-1000: the sums
                   over the real rows are untouched, and what a pad row does add -- log 2^1000 to sum log d, one more
                   row to N log 2 pi -- is a known constant taken off again per problem.  No kernel knows about it.
"""
import numpy as np

from . import _lib
from .engine import CoefficientPack, StreamingBatch

__all__ = ["BatchedLogLikelihood", "log_likelihood_batch", "sho_coefficient_pack",
           "BatchedSampler", "sample_batch", "predict_batch"]


def sho_coefficient_pack(S0, w0, Q, delta, eps=1e-5):
    """
    Celerite coefficients of B exposure-integrated sums of J SHO terms at once: the term algebra of
    ``TermConvolution(TermSum(SHOTerm x J), delta)`` (what ``StellarOscillatorKernel`` is,
    /root/reference/gadfly/core.py:371-394) vectorised over the batch,
    so that a sampler proposing hyperparameter arrays does not build B x J Python objects per step
    (1.5 s for 2048 walkers of 30 terms against a millisecond here).

    ``S0, w0, Q``: arrays of shape (B, J); ``delta``: exposure in 1/uHz (scalar or (B,)).  Terms with
    Q < 1/2 become two real exponentials each, so the overdamped pattern must be the same for every
    problem of the batch.  Returns ``(Jr, Jc, real, comp, diag_add, c)`` in the layout of the
    per-object path (:func:`gadfly_amd.engine._coeff_pack`), with identical values.
    """
    S0, w0, Q = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (S0, w0, Q))
    if not (S0.shape == w0.shape == Q.shape):
        raise ValueError("dimension mismatch")
    B = S0.shape[0]
    over = Q < 0.5
    if np.any(over != over[0]):
        raise ValueError("all problems of a batch must share the term structure "
                         "(the same terms overdamped, Q < 1/2, in every problem)")
    over = over[0]
    und = ~over
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), (B,))[:, None]
    # overdamped terms: two real exponentials each, in term order (SHOTerm.get_coefficients)
    So, wo, Qo = S0[:, over], w0[:, over], Q[:, over]
    f = np.sqrt(np.maximum(1.0 - 4.0 * Qo * Qo, eps))
    amp = 0.5 * So * wo * Qo
    ar = np.stack([amp * (1.0 + 1.0 / f), amp * (1.0 - 1.0 / f)], axis=-1).reshape(B, -1)
    cr = np.stack([0.5 * wo / Qo * (1.0 - f), 0.5 * wo / Qo * (1.0 + f)], axis=-1).reshape(B, -1)
    # underdamped terms (Q == 1/2 lands here with f = sqrt(eps))
    Su, wu, Qu = S0[:, und], w0[:, und], Q[:, und]
    f = np.sqrt(np.maximum(4.0 * Qu * Qu - 1.0, eps))
    a = Su * wu * Qu
    cc = 0.5 * wu / Qu
    # exposure integration (TermConvolution.get_coefficients / get_diag_shift), complex form
    A = np.concatenate([ar.astype(np.complex128), a - 1j * (a / f)], axis=1)
    z = np.concatenate([cr.astype(np.complex128), cc - 1j * (cc * f)], axis=1)
    zd = z * delta
    with np.errstate(over="ignore", invalid="ignore"):
        Ap = 2.0 * A * (np.cosh(zd) - 1.0) / zd ** 2
        shift = np.sum((2.0 * A * (zd - np.sinh(zd)) / zd ** 2).real, axis=1)
    Jr, Jc = ar.shape[1], a.shape[1]
    real = np.zeros((2, B, max(Jr, 1)))
    comp = np.zeros((4, B, max(Jc, 1)))
    real[0, :, :Jr], real[1, :, :Jr] = Ap[:, :Jr].real, z[:, :Jr].real
    comp[0, :, :Jc], comp[1, :, :Jc] = Ap[:, Jr:].real, -Ap[:, Jr:].imag
    comp[2, :, :Jc], comp[3, :, :Jc] = z[:, Jr:].real, -z[:, Jr:].imag
    diag_add = np.sum(real[0, :, :Jr], axis=1) + np.sum(comp[0, :, :Jc], axis=1) + shift
    c = np.zeros((B, Jr + 2 * Jc))
    c[:, :Jr] = real[1, :, :Jr]
    c[:, Jr::2] = comp[2, :, :Jc]
    c[:, Jr + 1::2] = comp[2, :, :Jc]
    return Jr, Jc, real, comp, diag_add, c


class _Pack(CoefficientPack):
    """A coefficient pack of the engine that remembers whether its kernels are positive semi-definite by
    construction (sums of SHO terms with positive S0, w0, Q, possibly exposure-integrated)."""
    psd_safe = False


def _sho_only(kernel, dt_min=None, t_abs_max=0.0):
    """True when K + diag(>= 0) is positive semi-definite by construction, or so close to it that only rounding
    or cadence jitter stands in the way: a sum of SHO terms with S0, w0, Q > 0 is a covariance function whatever the
    hyperparameters; its exposure-integrated form (``TermConvolution``, every kernel gadfly builds) is one only
    where the celerite coefficients represent it exactly, i.e. for lags >= delta -- closer time stamps get the
    un-integrated form's continuation, which need not be a covariance (``TermConvolution(SHOTerm(S0=1, w0=2,
    Q=0.7), 1)`` on ``arange(200) * 0.2`` has 33 negative eigenvalues).  ``dt_min``: the smallest spacing of the
    time axis the kernel is evaluated on (None: unknown -> False for an integrated kernel); see EXPOSURE_SLACK for
    stamps marginally closer than delta."""
    from .terms import SHOTerm, TermConvolution
    base = kernel
    if isinstance(kernel, TermConvolution):
        base = kernel.term
        if not _exposure_resolved(float(kernel.delta), dt_min, t_abs_max):
            return False
    terms = getattr(base, "terms", None)
    if terms is None:
        terms = (base,)
    return len(terms) > 0 and all(type(t) is SHOTerm and t.S0 > 0.0 and t.w0 > 0.0 and t.Q > 0.0 for t in terms)


#: how far below the exposure time the closest pair of stamps may sit for the two-sweep route to be taken: real
#: cadences jitter (barycentric corrections, +-0.2 s in cfg3's jittered variant), and for lags this close to delta the
#: celerite form departs from the integrated kernel only to second order in the shortfall.  Such a matrix is no longer
#: a covariance BY CONSTRUCTION -- what guarantees the result there is the corrections' check of every pivot's sign
#: (gadfly_dense.hip: k_corr_small / k_pchol + k_spd_check), which sends anything indefinite to the final pass.
#: Grossly unresolved exposures (the advisor's example: stamps 0.2 apart, delta = 1) are indefinite for sure: not taken.
EXPOSURE_SLACK = 0.1


def _exposure_resolved(delta, dt_min, t_abs_max=0.0):
    """No two time stamps closer than (1 - EXPOSURE_SLACK) of the exposure time ``delta`` (and the rounding of the
    stamps themselves: a one-minute cadence on a JD-based axis jitters by 5e-7 of the spacing)."""
    if delta <= 0.0:
        return True
    if dt_min is None:
        return False
    tol = max(1e-9 * delta, 4.0 * float(np.spacing(abs(t_abs_max))))
    return dt_min >= (1.0 - EXPOSURE_SLACK) * delta - tol


#: diagonal of a missing-data row (ragged batches): a power of two, so that a + 2^1000 and the pivot are 2^1000 exactly
PAD_DIAG = 2.0 ** 1000


def _is_ragged(t):
    """A list / tuple / object array of 1-D series (not one rectangular array)."""
    if isinstance(t, np.ndarray):
        return t.dtype == object
    if isinstance(t, (list, tuple)) and len(t) and all(np.ndim(x) == 1 for x in t):
        return len({len(x) for x in t}) > 1         # (equal lengths: an ordinary (B, N) array)
    return False


def _pad_ragged(t, y, d, mean):
    """B series of different lengths -> rectangular (B, Nmax) arrays with missing-data rows at the end.
    Returns (t, y - mean, diag, rows per problem, largest real diagonal per problem, smallest real spacing,
    largest real |t|)."""
    B = len(t)
    ts = [np.ascontiguousarray(x, dtype=np.float64) for x in t]
    if not isinstance(y, (list, tuple)) and not (isinstance(y, np.ndarray) and y.dtype == object):
        raise ValueError("dimension mismatch")
    ys = [np.ascontiguousarray(x, dtype=np.float64) for x in y]
    if len(ys) != B or any(a.ndim != 1 or a.shape != b.shape for a, b in zip(ts, ys)):
        raise ValueError("dimension mismatch")
    rows = np.array([len(x) for x in ts], dtype=np.int64)
    if np.any(rows < 1):
        raise ValueError("dimension mismatch")
    if any(np.any(np.diff(x) < 0.0) for x in ts):
        raise ValueError("The input coordinates must be sorted")
    if d is None:
        ds = [np.zeros(n) for n in rows]
    elif isinstance(d, (list, tuple)) or (isinstance(d, np.ndarray) and d.dtype == object):
        ds = [np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x, n in zip(d, rows)]
        if len(ds) != B:
            raise ValueError("dimension mismatch")
    else:
        d = np.asarray(d, dtype=np.float64)
        if d.ndim > 1 or (d.ndim == 1 and d.shape[0] != B):
            raise ValueError("dimension mismatch")          # a scalar, or one value per problem
        ds = [np.full(n, float(d if d.ndim == 0 else d[i])) for i, n in enumerate(rows)]
    means = np.broadcast_to(np.asarray(mean, dtype=np.float64), (B,)) if np.ndim(mean) <= 1 else None
    if means is None:
        raise ValueError("dimension mismatch")
    Nmax = int(rows.max())
    T = np.empty((B, Nmax))
    Y = np.zeros((B, Nmax))
    D = np.full((B, Nmax), PAD_DIAG)
    for i, n in enumerate(rows):
        T[i, :n], Y[i, :n], D[i, :n] = ts[i], ys[i] - means[i], ds[i]
        if n < Nmax:
            # the series' own cadence continued: the row generator keeps stepping, no gap, no new phase range
            dt = float(np.median(np.diff(ts[i]))) if n > 1 else 1.0
            if not dt > 0.0:
                dt = 1.0
            T[i, n:] = ts[i][-1] + dt * np.arange(1, Nmax - n + 1)
    dmax = np.array([float(np.max(x)) if len(x) else 0.0 for x in ds])
    dmin_real = min(float(np.min(x)) for x in ds)
    dt_min = min((float(np.min(np.diff(x))) for x in ts if len(x) > 1), default=None)
    tabs = max(float(np.max(np.abs(x))) for x in ts)
    return T, Y, D, rows, dmax, dmin_real, dt_min, tabs


class BatchedLogLikelihood:
    """Reusable evaluator: device buffers are allocated once; each :meth:`evaluate` with new
    kernels costs an O(B J) coefficient upload plus the device work.

    ``t`` / ``y``: shared ((N,)), per problem ((B, N)), or -- ragged -- lists of B series of different lengths
    (``yerr`` / ``diag`` then a scalar, one value per problem, or a list of per-series arrays; ``mean`` a scalar or
    one value per problem)."""

    def __init__(self, kernels, t, y, yerr=None, diag=None, mean=0.0, device=None,
                 tile_rows=8192, overlap_build=False):
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        self.rows = None                    # ragged batches: real rows per problem
        self._pad_corr = None
        if _is_ragged(t):
            if len(t) != len(kernels):
                raise ValueError("dimension mismatch")
            dd = diag
            if yerr is not None:
                dd = ([np.asarray(e, dtype=np.float64) ** 2 for e in yerr]
                      if isinstance(yerr, (list, tuple)) or (isinstance(yerr, np.ndarray) and yerr.dtype == object)
                      else np.asarray(yerr, dtype=np.float64) ** 2)
            t, ym, d, self.rows, dmax, dmin_real, dt_min, tabs = _pad_ragged(t, y, dd, mean)
            self.engine = StreamingBatch([k.get_device_coefficients() for k in kernels], t, ym, diag=d,
                                         tile_rows=tile_rows, device=device, overlap_build=overlap_build)
            eng = self.engine
            torch = eng.torch
            # the condition estimates look at the REAL rows' diagonal, and the results lose the pad rows' constants
            eng._diag_amax = torch.as_tensor(dmax, dtype=torch.float64, device=eng.device)
            pad = (t.shape[1] - self.rows).astype(np.float64)
            self._pad_corr = torch.as_tensor(0.5 * pad * (np.log(PAD_DIAG) + np.log(2.0 * np.pi)),
                                             dtype=torch.float64, device=eng.device)
            self._diag_nonneg = dmin_real >= 0.0
            self._dt_min, self._t_abs_max = dt_min, tabs
            self._mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (len(kernels),)).copy()
            self._finish_init(kernels)
            eng.steady_state = False        # ragged batches: the pad rows' diagonal breaks the steady mode's premise
            return
        t = np.ascontiguousarray(t, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if np.any(np.diff(t, axis=-1) < 0.0):
            raise ValueError("The input coordinates must be sorted")
        if y.shape[-1] != t.shape[-1]:
            raise ValueError("dimension mismatch")
        d = None
        if yerr is not None:
            d = np.asarray(yerr, dtype=np.float64) ** 2
        elif diag is not None:
            d = np.asarray(diag, dtype=np.float64)
        if d is not None and d.ndim == 0:
            d = np.full(t.shape[-1], float(d))
        self.engine = StreamingBatch([k.get_device_coefficients() for k in kernels], t,
                                     y - mean, diag=d, tile_rows=tile_rows, device=device,
                                     overlap_build=overlap_build)
        self._diag_nonneg = d is None or bool(np.all(np.asarray(d) >= 0.0))
        #: smallest spacing of the time axes and their largest |t|: an exposure-integrated kernel is a covariance
        #: only while no two stamps are closer than its exposure time (see _sho_only)
        self._dt_min = float(np.min(np.diff(t, axis=-1))) if t.shape[-1] > 1 else None
        self._t_abs_max = float(np.max(np.abs(t))) if t.size else 0.0
        self._mean = np.asarray(mean, dtype=np.float64)
        self._finish_init(kernels)

    def _finish_init(self, kernels):
        #: the time-parallel route may drop its final pass (engine.two_sweep) when the matrix is positive
        #: semi-definite by construction: SHO kernels, a non-negative diagonal, no two time stamps closer than
        #: the exposure time.  Rounding can still break a pivot: the corrections check the sign of EVERY pivot
        #: of a chunk (a Cholesky attempt on (I - X G) X, gadfly_dense.hip: k_spd_check), not only the parity
        #: det(I - X G) gives, and a chunk that fails it leaves a non-finite value, which :meth:`resolve` repeats
        #: with the final pass
        self._init_safe = self._diag_nonneg and all(_sho_only(k, self._dt_min, self._t_abs_max) for k in kernels)
        self.two_sweep = True
        #: keep the row generator's share of the relative log-likelihood error below this by
        #: choosing its re-anchoring period from the measured conditioning
        self.generator_target = 1e-9
        self.auto_generator_period = True
        #: evaluations whose accuracy guard has not been looked at yet: (out, flag, pack, period)
        self._unresolved = []
        #: host coefficients of the kernels of construction (what :meth:`predict` takes when given none); a
        #: complexified batch (W > 63) is beyond :meth:`predict` anyway
        eng = self.engine
        self._pack0 = None if eng._complexified else tuple(eng._struct0) + tuple(eng._coeff_host[:3])
        #: evaluations repeated with exact generator rows by the guard so far
        self.guard_reruns = 0
        #: ... of which: evaluations whose steady-mode tail met a row it cannot take (engine.steady_violations)
        self.steady_reruns = 0
        self._viol_flags = {}               # id(out) -> violation flags of the evaluations not yet resolved
        self._last_cond = None
        #: exposure times of the kernels of construction (0: not exposure-integrated), for :meth:`sample_conditional`
        self._delta0 = self._deltas_of(kernels)

    @property
    def B(self):
        return self.engine.B

    def pack(self, kernels):
        pk = _Pack(*self.engine.pack_coefficients([k.get_device_coefficients() for k in kernels]))
        pk.psd_safe = all(_sho_only(k, self._dt_min, self._t_abs_max) for k in kernels)
        pk.delta = self._deltas_of(kernels)
        return pk

    def pack_parameters(self, S0, w0, Q, delta):
        """Coefficient pack straight from (B, J) hyperparameter arrays (:func:`sho_coefficient_pack`):
        the vectorised form of :meth:`pack` for ``StellarOscillatorKernel``-type kernels."""
        pk = _Pack(*self.engine.pack_arrays(*sho_coefficient_pack(S0, w0, Q, delta)))
        pk.psd_safe = bool(np.all(np.asarray(S0) > 0.0) and np.all(np.asarray(w0) > 0.0)
                           and np.all(np.asarray(Q) > 0.0)
                           and all(_exposure_resolved(float(dl), self._dt_min, self._t_abs_max)
                                   for dl in np.atleast_1d(np.asarray(delta, dtype=np.float64))))
        pk.delta = np.broadcast_to(np.asarray(delta, dtype=np.float64).reshape(-1), (self.B,)).copy()
        return pk

    #: cap on the gradient workspace of one call in bytes (:meth:`value_and_grad`): larger batches run in groups
    grad_workspace_bytes = _lib.GF_GRAD_WORKSPACE_BYTES

    def _host_pack(self, pack_or_kernels):
        """Stacked host coefficients (Jr, Jc, real, comp, diag_add) of the batch's original term structure from a
        list of kernels, a host pack (:func:`sho_coefficient_pack`, ``engine._coeff_pack``) or a device pack."""
        x = pack_or_kernels
        if isinstance(x, tuple) and len(x) >= 5 and isinstance(x[0], (int, np.integer)):
            return int(x[0]), int(x[1]), np.asarray(x[2]), np.asarray(x[3]), np.asarray(x[4])
        if isinstance(x, tuple):                       # a device pack (pack / pack_parameters)
            if self.engine._complexified:
                raise NotImplementedError("gradients of complexified (W > 63) packs are not supported")
            Jr, Jc = self.engine._struct0
            return (Jr, Jc, x[0].cpu().numpy(), x[1].cpu().numpy(), x[2].cpu().numpy())
        from .engine import _coeff_pack
        Jr, Jc, real, comp, diag_add, _ = _coeff_pack([k.get_device_coefficients() for k in x])
        return Jr, Jc, real, comp, diag_add

    def _grad_check_width(self, wide=False, hint=False):
        from .grad import check_width
        Jr, Jc = self.engine._struct0
        check_width(Jr + 2 * Jc, wide, hint=hint)

    def value_and_grad_coefficients(self, pack_or_kernels, time_parallel=False, chunk_len=None, wide=False):
        """log-likelihoods and their gradients with respect to the celerite coefficients.
        Returns ``(ll, grads)``: ll (B,) numpy (-inf where K is not positive definite, whose gradients are NaN);
        grads in the engine's stacked layout: ``real`` (2, B, Jr) = d/d(a, c), ``comp`` (4, B, Jc) =
        d/d(a, b, c, d), ``diag_add`` (B,) (also d/d of a constant added to the diagonal), ``mean`` (B,).

        ``time_parallel``: cut every series into chunks of ``chunk_len`` rows (None: the library's default for the
        batch) that are swept concurrently -- the route for one long series or a few, where one
        wave per problem leaves the device idle.  Same results to rounding; the default keeps the one-wave route and
        its bits.

        ``wide``: one workgroup per problem, the route for celerite widths beyond 63 -- gadfly's
        86-term default kernel among them -- up to :func:`gadfly_amd.grad.wide_max_width`; narrow kernels are taken
        too.  Same results to rounding; not together with ``time_parallel`` or ``chunk_len`` (ValueError)."""
        if wide and (time_parallel or chunk_len is not None):
            raise ValueError("wide=True does not combine with time_parallel or chunk_len")
        self._grad_check_width(wide, hint=True)
        from .grad import coefficient_gradients
        Jr, Jc, real, comp, diag_add = self._host_pack(pack_or_kernels)
        res = coefficient_gradients(self.engine, Jr, Jc, real, comp, diag_add, self.grad_workspace_bytes,
                                    chunk_len=chunk_len, time_parallel=time_parallel, wide=wide)
        #: (workspace bytes of a group, number of groups, problems per group) and the device time of the last call
        self.last_grad_plan = (res["workspace_bytes"], res["groups"], res["group_size"])
        self.last_grad_device_ms = res["device_ms"]
        #: rows per chunk of the last call (None: the one-wave route) and the problems it sent to the one-wave route
        self.last_grad_chunk_len = res.get("chunk_len")
        self.last_grad_reruns = res.get("reruns", 0)
        #: rows per segment of the last call (None: not the wide route)
        self.last_grad_seg = res.get("seg")
        ll = res["ll"]
        if self._pad_corr is not None:
            ll = ll + self._pad_corr.cpu().numpy()       # ragged batch: the missing-data rows' constants
        return ll, {k: res[k] for k in ("real", "comp", "diag_add", "mean")}

    def value_and_grad(self, S0, w0, Q, delta, wrt=("S0", "w0", "Q"), time_parallel=False, chunk_len=None,
                       wide=False):
        """log-likelihoods at (B, J) SHO hyperparameter arrays (as :meth:`pack_parameters` takes them) and their
        gradients.  Returns ``(ll, grads)``: ll (B,) numpy; grads a dict holding the names of ``wrt`` among
        ``"S0"``, ``"w0"``, ``"Q"`` ((B, J) each), ``"mean"`` ((B,): d/d of a constant mean, sum alpha) and
        ``"diag"`` ((B,): d/d of a constant added to the diagonal).  A problem whose matrix is not positive
        definite gets -inf and NaN gradients; the others are unaffected.  ``time_parallel``, ``chunk_len``: as
        :meth:`value_and_grad_coefficients` (one long series, or a few); ``wide``: as there (celerite widths beyond
        63)."""
        if wide and (time_parallel or chunk_len is not None):
            raise ValueError("wide=True does not combine with time_parallel or chunk_len")
        self._grad_check_width(wide, hint=True)
        from .grad import parameter_vjp
        wrt = tuple(wrt)
        unknown = set(wrt) - {"S0", "w0", "Q", "mean", "diag"}
        if unknown:
            raise ValueError(f"unknown gradient names {sorted(unknown)}")
        shapes = {np.shape(np.atleast_2d(np.asarray(v))) for v in (S0, w0, Q)}
        if len(shapes) != 1 or next(iter(shapes))[0] != self.B:
            raise ValueError(f"S0, w0, Q of shapes {sorted(shapes)} do not hold the batch's {self.B} problems")
        pk = sho_coefficient_pack(S0, w0, Q, delta)
        ll, g = self.value_and_grad_coefficients(pk, time_parallel=time_parallel, chunk_len=chunk_len, wide=wide)
        out = {}
        if {"S0", "w0", "Q"} & set(wrt):
            gS0, gw0, gQ = parameter_vjp(S0, w0, Q, delta, g["real"], g["comp"], g["diag_add"])
            out.update({k: v for k, v in (("S0", gS0), ("w0", gw0), ("Q", gQ)) if k in wrt})
        if "mean" in wrt:
            out["mean"] = g["mean"]
        if "diag" in wrt:
            out["diag"] = g["diag_add"]
        return ll, out

    #: cap on the workspace of one :meth:`predict` call in bytes: larger batches run in groups
    predict_workspace_bytes = _lib.GF_SOLVE_WORKSPACE_BYTES

    def _query_times(self, t):
        """``t=`` of :meth:`predict_device` -> (stamps (1 or B, M) float64, queries per problem or None, whether the
        result is a list): an array (M,) shared by all problems or (B, M), or a list / tuple of B 1-D arrays of any
        lengths (padded at the end with each series' last stamp; the pad is never read)."""
        B = self.B
        if _is_ragged(t) or (isinstance(t, (list, tuple)) and len(t) and all(np.ndim(x) == 1 for x in t)):
            qs = [np.ascontiguousarray(x, dtype=np.float64) for x in t]
            if len(qs) != B:
                raise ValueError(f"t= holds {len(qs)} series of query times for a batch of {B} problems")
            if any(np.any(np.diff(x) < 0.0) for x in qs):
                raise ValueError("The input coordinates must be sorted")
            nq = np.array([len(x) for x in qs], dtype=np.int64)
            T = np.zeros((B, int(nq.max())))
            for b, x in enumerate(qs):
                T[b, :len(x)] = x
                T[b, len(x):] = x[-1] if len(x) else 0.0
            return T, nq, True
        T = np.asarray(t, dtype=np.float64)
        if T.ndim == 1:
            T = T[None, :]
        if T.ndim != 2 or T.shape[0] not in (1, B):
            raise ValueError(f"t= of shape {np.shape(t)} is neither (M,) nor ({B}, M) nor a list of {B} series")
        if np.any(np.diff(T, axis=-1) < 0.0):
            raise ValueError("The input coordinates must be sorted")
        return np.ascontiguousarray(T), None, False

    def _mean_per_problem(self):
        """The mean of construction as a scalar or a (B, 1) column; ValueError if it varies along the rows (such a
        mean is known at the observed stamps only)."""
        m = self._mean
        if self.rows is not None:           # ragged data: the constructor keeps one value per problem, (B,)
            assert m.shape == (self.B,)
            return m[:, None]
        if m.size == 1:
            return m.reshape(())
        m = np.atleast_2d(m)
        if np.any(m != m[:, :1]):
            raise ValueError("a mean that varies along the rows cannot be evaluated at new times t; pass "
                             "include_mean=False and add the mean at t yourself")
        return m[:, :1]

    def _record_predict(self, res):
        """The ``last_predict_*`` attributes from the result of a solve_batch / variance_batch call."""
        #: (workspace bytes of a group, number of groups, problems per group) and the HIP events of the last call
        self.last_predict_plan = (res["workspace_bytes"], res["groups"], res["group_size"])
        self._predict_events, self._predict_at_events = res["events"], []
        self.last_predict_ll = res["ll"] if self._pad_corr is None else res["ll"] + self._pad_corr
        self.last_predict_info = res["info"]

    def _add_mean(self, x, include_mean):
        """Add the mean of construction to a (B, N) device tensor at the observed rows, in place."""
        if include_mean and np.any(self._mean != 0.0):
            # (whatever y - mean broadcast at construction: a scalar, (N,), (B, 1) or (B, N); ragged: one per problem)
            eng = self.engine
            m = self._mean[:, None] if self.rows is not None else self._mean
            m = np.array(np.broadcast_to(m, np.broadcast_shapes(np.shape(m), (1, 1))))
            x += eng.torch.as_tensor(m, dtype=eng.torch.float64, device=eng.device)

    def _query_mean(self, include_mean):
        """The mean a call with ``t=`` adds (:meth:`_mean_per_problem`), or None: looked at before anything is
        enqueued, as it may raise."""
        return self._mean_per_problem() if include_mean and np.any(self._mean != 0.0) else None

    def _mean_at(self, cf, alpha, ts, nq, mean):
        """The second launch of a call with ``t=``: K(t*, t) alpha of the coefficients ``cf`` at the query stamps,
        (B, M) on the device, with the per-problem ``mean`` of :meth:`_query_mean` added."""
        from .predict import predict_at
        eng = self.engine
        at = predict_at(eng, *cf, alpha, ts, nobs=self.rows, nq=nq)
        self._predict_at_events = at["events"]
        mu = at["mu"]
        if mean is not None:
            mu += eng.torch.as_tensor(np.array(mean), dtype=eng.torch.float64, device=eng.device)
        return mu

    def _empty_queries(self):
        eng = self.engine
        return eng.torch.empty((self.B, 0), dtype=eng.torch.float64, device=eng.device)

    def _predict_at(self, pack_or_kernels, kernel, include_mean, return_alpha, t):
        """:meth:`predict_device` with ``t=``: alpha as without it, then the two sums between the sorted axes."""
        from .predict import check_width, component_pack, solve_batch
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0)
        ts, nq, as_list = self._query_times(t)
        mean = self._query_mean(include_mean)
        component = None if kernel is None else component_pack(kernel, self.B)
        Jr, Jc, real, comp, diag_add = self._pack0 if pack_or_kernels is None else self._host_pack(pack_or_kernels)
        res = solve_batch(eng, Jr, Jc, real, comp, diag_add, None, self.predict_workspace_bytes,
                          want_alpha=True, want_mu=False)
        self._record_predict(res)
        if ts.shape[1] == 0:
            mu = self._empty_queries()
        else:
            mu = self._mean_at((Jr, Jc, real, comp) if component is None else component, res["alpha"], ts, nq, mean)
        mu, alpha = self._cut_queries(mu, nq, as_list), self._cut_rows(res["alpha"])
        return (mu, alpha) if return_alpha else mu

    def _variance_call(self, pack_or_kernels, ts=None, nq=None, **want):
        """One ``gf_var_batch`` call over the batch (:func:`gadfly_amd.predict.variance_batch`), the ``last_predict_*``
        attributes filled as :meth:`predict_device` fills them."""
        from .predict import check_width, variance_batch
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0)
        Jr, Jc, real, comp, diag_add = self._pack0 if pack_or_kernels is None else self._host_pack(pack_or_kernels)
        res = variance_batch(eng, Jr, Jc, real, comp, diag_add, ts=ts, nobs=self.rows, nq=nq,
                             cap_bytes=self.predict_workspace_bytes, **want)
        self._record_predict(res)
        return (Jr, Jc, real, comp), res

    def _cut_rows(self, x):
        """(B, N) -> the list of each series' real rows for a ragged batch."""
        if x is None or self.rows is None:
            return x
        return [x[b, :int(n)] for b, n in enumerate(self.rows)]

    @staticmethod
    def _cut_queries(x, nq, as_list):
        """(B, M) -> the list of each problem's own queries where ``t=`` was a list."""
        return [x[b, :int(n)] for b, n in enumerate(nq)] if as_list else x

    def _predict_var(self, pack_or_kernels, kernel, include_mean, return_alpha, t):
        """:meth:`predict_device` with ``return_var=True``."""
        if kernel is not None:
            raise NotImplementedError(
                "return_var with kernel=component is not supported: the component's conditional variance "
                "K'(0) - K' Sigma^-1 K'^T does not reduce to the inverse diagonal of Sigma")
        if t is None:
            _, res = self._variance_call(pack_or_kernels, want_alpha=return_alpha, want_mu=True, want_h=False,
                                         want_var=True)
            self._add_mean(res["mu"], include_mean)
            mu, var, alpha = self._cut_rows(res["mu"]), self._cut_rows(res["var"]), self._cut_rows(res["alpha"])
            return (mu, var, alpha) if return_alpha else (mu, var)
        ts, nq, as_list = self._query_times(t)
        mean = self._query_mean(include_mean)
        M = ts.shape[1]
        cf, res = self._variance_call(pack_or_kernels, ts=ts if M else None, nq=nq if M else None, want_alpha=True,
                                      want_mu=False, want_h=False, want_var=False)
        if M == 0:
            mu, var = self._empty_queries(), self._empty_queries()
        else:
            mu, var = self._mean_at(cf, res["alpha"], ts, nq, mean), res["var_at"]
        mu, var = self._cut_queries(mu, nq, as_list), self._cut_queries(var, nq, as_list)
        alpha = self._cut_rows(res["alpha"])
        return (mu, var, alpha) if return_alpha else (mu, var)

    def inverse_diagonal_device(self, pack_or_kernels=None):
        """h_n = (Sigma^-1)_nn of the B problems, Sigma = K + diag, as a float64 device tensor (B, N)
        (a list of B tensors for a ragged batch): the quantity the conditional variances and the leave-one-out
        residuals are made of, with no cancellation in it.  ``pack_or_kernels`` as :meth:`predict_device`; NaN rows
        where the matrix is not positive definite.  No host synchronisation."""
        _, res = self._variance_call(pack_or_kernels, want_alpha=False, want_mu=False, want_h=True, want_var=False)
        return self._cut_rows(res["hdiag"])

    def leave_one_out_device(self, pack_or_kernels=None, include_mean=True):
        """``(mean, var)`` of every observation given all the others of its series, E[y_n | y_-n] = y_n - alpha_n / h_n
        and Var[y_n | y_-n] = 1 / h_n (the observation's own noise included), from one device call: float64 device
        tensors (B, N), lists for a ragged batch.  (y_n - mean_n)^2 / var_n flags outliers.  No host synchronisation."""
        _, res = self._variance_call(pack_or_kernels, want_alpha=True, want_mu=False, want_h=True, want_var=False)
        eng = self.engine
        var = 1.0 / res["hdiag"]
        mean = eng.y.reshape(-1, eng.N) - res["alpha"] * var
        self._add_mean(mean, include_mean)
        return self._cut_rows(mean), self._cut_rows(var)

    @staticmethod
    def _to_host(x):
        return [v.cpu().numpy() for v in x] if isinstance(x, list) else x.cpu().numpy()

    def inverse_diagonal(self, pack_or_kernels=None):
        """:meth:`inverse_diagonal_device`, returned as numpy."""
        return self._to_host(self.inverse_diagonal_device(pack_or_kernels))

    def leave_one_out(self, pack_or_kernels=None, include_mean=True):
        """:meth:`leave_one_out_device`, returned as numpy."""
        return tuple(self._to_host(x) for x in self.leave_one_out_device(pack_or_kernels, include_mean=include_mean))

    def _predict_wide(self, pack_or_kernels, kernel, include_mean, return_alpha, t):
        """:meth:`predict_device` with ``wide=True``: alpha (and mu at the observed times) from
        ``gf_solve_batch_wide``; a component's share and the means at new times from ``gf_predict_batch_at`` over the
        kernel's groups of whole terms."""
        from .predict import check_width, component_pack, predict_at_groups, solve_batch_wide, term_groups
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0, wide=True)
        ts, nq, as_list, mean = None, None, False, None
        if t is not None:
            ts, nq, as_list = self._query_times(t)
            mean = self._query_mean(include_mean)
        component = None if kernel is None else component_pack(kernel, self.B, wide=True)
        if pack_or_kernels is not None:
            Jr, Jc, real, comp, diag_add = self._host_pack(pack_or_kernels)
        elif self._pack0 is not None:
            Jr, Jc, real, comp, diag_add = self._pack0
        else:                               # (a wide kernel with real terms: the engine holds them rewritten)
            from .engine import _coeff_pack
            Jr, Jc, real, comp, diag_add = _coeff_pack(eng._coeffs_list)[:5]
        sums =t is not None or component is not None
        res = solve_batch_wide(eng, Jr, Jc, real, comp, diag_add, self.predict_workspace_bytes,
                               want_alpha=return_alpha or sums, want_mu=not sums)
        self._record_predict(res)
        if not sums:
            mu = res["mu"]
            self._add_mean(mu, include_mean)
            mu = self._cut_rows(mu)
        else:
            groups = term_groups(*((Jr, Jc, real, comp) if component is None else component))
            if t is None:                   # the component's share at the observed stamps: t* = t
                at = predict_at_groups(eng, groups, res["alpha"], eng.t, nobs=self.rows, nq=self.rows)
                self._predict_at_events = at["events"]
                mu = at["mu"]
                self._add_mean(mu, include_mean)
                mu = self._cut_rows(mu)
            else:
                if ts.shape[1] == 0:
                    mu = self._empty_queries()
                else:
                    at = predict_at_groups(eng, groups, res["alpha"], ts, nobs=self.rows, nq=nq)
                    self._predict_at_events = at["events"]
                    mu = at["mu"]
                    if mean is not None:
                        mu += eng.torch.as_tensor(np.array(mean), dtype=eng.torch.float64, device=eng.device)
                mu = self._cut_queries(mu, nq, as_list)
        alpha = self._cut_rows(res["alpha"])
        return (mu, alpha) if return_alpha else mu

    def predict_device(self, pack_or_kernels=None, kernel=None, include_mean=True, return_alpha=False, t=None,
                       return_var=False, wide=False):
        """Conditional means of the B problems at their observed times in one device call: what
        ``GaussianProcess(kernel_b, t, yerr).predict(y)`` gives one kernel at a time -- mu = y - diag alpha with
        alpha = K^-1 (y - mean) -- as a float64 device tensor (B, N); a ragged batch returns a list of B tensors cut
        to each series' rows.  Nothing is copied back (no host synchronisation).

        ``pack_or_kernels``: a list of B kernels, a host pack (:func:`sho_coefficient_pack`) or a device pack
        (:meth:`pack`, :meth:`pack_parameters`); None: the kernels of construction.  ``kernel``: the part of the
        kernel whose share of the data is wanted (``predict(y, kernel=component)``: K'(t, t) alpha, the component's
        exposure shift not added) -- a list of B component kernels, one kernel for all problems or a host pack, all
        of one term structure.  ``include_mean=False`` leaves the mean out of the result.  ``return_alpha``: also
        alpha, ``(mu, alpha)``.  A problem whose matrix is not positive definite gets NaN in all its rows (the
        others are unaffected); :attr:`last_predict_ll` holds the log-likelihoods (-inf there) and
        :attr:`last_predict_info` the failing rows, both on the device.  Kernels or components wider than W = 63
        raise ``NotImplementedError``.

        ``t``: new times t* at which to predict instead (``GaussianProcess.predict(y, t=t*)``) --
        an array (M,) shared by all problems or (B, M), or a list / tuple of B 1-D arrays of any lengths, ascending
        per problem, whether the data are ragged or not; the result is (B, M) for an array and a list of B tensors
        for a list.  It is
        K(t*, t) alpha with the kernel's coefficients at every lag (no diagonal; an exposure-integrated kernel stays
        in coefficient form), or K'(t*, t) alpha with ``kernel=component``.  The mean added is a scalar or one value
        per problem: a mean that varies along the rows raises ``ValueError`` unless ``include_mean=False``.  An
        empty ``t`` gives an empty result (alpha is still solved for; the second launch is left out).

        ``return_var``: also the conditional variances (``predict(y, t, return_var=True)``), ``(mu,
        var)`` or ``(mu, var, alpha)`` -- at the observed times diag_n - diag_n^2 h_n, the variance of the noise-free
        process (exactly 0 where diag_n = 0), at new times K(0) - K(t*, t) Sigma^-1 K(t, t*) with the kernel in its
        coefficient form at every lag (an exposure-integrated kernel is exact for queries at least its exposure time
        from every stamp).  One ``gf_var_batch`` launch takes the place of ``gf_solve_batch``: the means keep their
        bits.  With ``kernel=component`` it raises ``NotImplementedError``.

        ``wide``: one workgroup per problem, the route for celerite widths beyond 63 -- gadfly's
        86-term default kernel among them -- up to ``gf_solve_wide_max_width()`` (192); narrow kernels are taken too
        (same results to rounding, not to the bit).  alpha and the means at the observed times come from
        ``gf_solve_batch_wide``; the means at new times ``t`` and a component's share (of any width up to the same
        limit, at the observed stamps or at ``t``) are ``gf_predict_batch_at``'s sums over groups of whole terms of
        width <= 63, added on the device: exact, K(t*, t) alpha being a sum over terms.  ``return_var`` with ``wide``
        raises ``NotImplementedError``: variances of wide kernels are not built."""
        if wide:
            if return_var:
                raise NotImplementedError("return_var with wide=True: conditional variances of wide kernels are not "
                                          "built (gf_var_batch is a one-wave kernel, W <= 63)")
            return self._predict_wide(pack_or_kernels, kernel, include_mean, return_alpha, t)
        if return_var:
            return self._predict_var(pack_or_kernels, kernel, include_mean, return_alpha, t)
        if t is not None:
            return self._predict_at(pack_or_kernels, kernel, include_mean, return_alpha, t)
        from .predict import check_width, component_pack, solve_batch
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0)
        component = None if kernel is None else component_pack(kernel, self.B)
        Jr, Jc, real, comp, diag_add = self._pack0 if pack_or_kernels is None else self._host_pack(pack_or_kernels)
        res = solve_batch(eng, Jr, Jc, real, comp, diag_add, component, self.predict_workspace_bytes,
                          want_alpha=return_alpha, want_mu=component is None)
        self._record_predict(res)
        mu = res["mu"] if component is None else res["mu_comp"]
        self._add_mean(mu, include_mean)
        mu, alpha = self._cut_rows(mu), self._cut_rows(res["alpha"])
        return (mu, alpha) if return_alpha else mu

    @property
    def last_predict_device_ms(self):
        """Summed device time of the last :meth:`predict_device` call's launches (synchronises)."""
        return self._events_ms(self._predict_events) + self.last_predict_at_ms

    @property
    def last_predict_at_ms(self):
        """The share of :attr:`last_predict_device_ms` spent in the launch that carries alpha to new times ``t``
        (0 for a call without ``t`` or with an empty one)."""
        return self._events_ms(self._predict_at_events)

    @staticmethod
    def _events_ms(events):
        for _, e1 in events:
            e1.synchronize()
        return sum(a.elapsed_time(b) for a, b in events)

    # -- R right-hand sides per factorisation, posterior draws ----------------------------------

    @staticmethod
    def _deltas_of(kernels):
        """Exposure time per kernel (0 for one that is not exposure-integrated)."""
        return np.array([float(getattr(k, "delta", 0.0) or 0.0) for k in kernels], dtype=np.float64)

    def _host_axes(self):
        """The observed stamps on the host, a list of B series cut to their real rows (copied back once)."""
        if getattr(self, "_t_host", None) is None:
            t = self.engine.t.cpu().numpy()
            rows = [t.shape[1]] * self.B if self.rows is None else [int(n) for n in self.rows]
            self._t_host = [t[b if t.shape[0] > 1 else 0, :n].copy() for b, n in enumerate(rows)]
        return self._t_host

    def _rhs_tensor(self, y):
        """y of shape (B, N), (B, R, N), (N,) or (R, N) shared -> ((1 or B, R, N) device tensor, restore(x) that gives
        a (B, R, N) result the layout of y: a shared y gives (B, N) / (B, R, N))."""
        eng = self.engine
        torch = eng.torch
        B, N = self.B, eng.N
        y = torch.as_tensor(y).to(dtype=torch.float64, device=eng.device)
        if y.ndim == 0 or y.shape[-1] != N or y.ndim > 3:
            raise ValueError(f"right-hand sides of shape {tuple(y.shape)} for {B} problems of {N} rows")
        if y.ndim == 1:
            return y[None, None, :], lambda x: x[:, 0]
        if y.ndim == 3:
            if y.shape[0] != B:
                raise ValueError(f"right-hand sides of shape {tuple(y.shape)} for {B} problems of {N} rows")
            return y, lambda x: x
        if y.shape[0] == B:                 # (B, N): one right-hand side per problem ((R, N) with R = B reads so too)
            return y[:, None, :], lambda x: x[:, 0]
        return y[None], lambda x: x

    def _solve_rhs(self, y, pack_or_kernels, **want):
        from .predict import check_width, solve_batch_rhs
        if self.rows is not None:
            raise NotImplementedError("right-hand sides for a ragged batch are not supported: pass per-series data "
                                      "to a batch of its own")
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0)
        y3, restore = self._rhs_tensor(y)
        Jr, Jc, real, comp, diag_add = self._pack0 if pack_or_kernels is None else self._host_pack(pack_or_kernels)
        res = solve_batch_rhs(eng, Jr, Jc, real, comp, diag_add, y3, self.predict_workspace_bytes, **want)
        self.last_predict_plan = (res["workspace_bytes"], res["groups"], res["group_size"])
        self._predict_events, self._predict_at_events = res["events"], []
        self.last_predict_ll, self.last_predict_info = res["ll"], res["info"]
        return res, restore

    def apply_inverse_device(self, y, pack_or_kernels=None):
        """alpha = (K_b + diag)^-1 y for B kernels at once, celerite2's ``apply_inverse``: ``y`` of shape (B, N),
        (B, R, N), or (N,) / (R, N) shared by all problems (host array or device tensor; the mean is NOT subtracted);
        returns a float64 device tensor of the same layout ((B, N) / (B, R, N) for a shared y).  The R right-hand sides
        of a problem go through ONE pass over its rows (``gf_solve_batch_rhs``).  NaN rows where the matrix is not
        positive definite; W > 63 raises ``NotImplementedError``.  No host synchronisation."""
        res, restore = self._solve_rhs(y, pack_or_kernels, want_alpha=True, want_mu=False)
        return restore(res["alpha"])

    def log_likelihood_device(self, y, pack_or_kernels=None):
        """The log-likelihoods of R data vectors per kernel (zero mean: pass y - mean), (B, R) on the device, from one
        factorisation per block of right-hand sides; ``y`` as :meth:`apply_inverse_device`.  -inf where the matrix is
        not positive definite."""
        res, _ = self._solve_rhs(y, pack_or_kernels, want_alpha=False, want_mu=False)
        return res["ll"]

    # -- linear mean models: generalised least squares from one forward sweep -------------------

    #: cap on the workspace of one :meth:`linear_gram_device` call in bytes: larger batches run in groups
    linear_workspace_bytes = _lib.GF_SOLVE_WORKSPACE_BYTES

    def _linear_gram(self, basis, pack_or_kernels):
        from .linmodel import check_width, linear_gram, stack_basis
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0)
        A, ncols = stack_basis(basis, self.B, eng.N, self.rows)
        Jr, Jc, real, comp, diag_add = self._pack0 if pack_or_kernels is None else self._host_pack(pack_or_kernels)
        A = eng.torch.as_tensor(A, dtype=eng.torch.float64, device=eng.device)
        res = linear_gram(eng, Jr, Jc, real, comp, diag_add, A, self.rows, self.linear_workspace_bytes)
        #: (workspace bytes of a group, number of groups, problems per group) and the HIP events of the last call
        self.last_linear_plan = (res["workspace_bytes"], res["groups"], res["group_size"])
        self._linear_events = res["events"]
        res["A"], res["pack"] = A, (Jr, Jc, real, comp, diag_add)
        return res, ncols

    def linear_gram_device(self, basis, pack_or_kernels=None):
        """[A | y]^T Sigma^-1 [A | y] of the linear mean models y = A beta + eps, eps ~ N(0, K_b + diag), for B
        kernels at once from ONE forward sweep (``gf_linear_gram``): ``basis`` (N, R) shared, (B, N, R), or a list of
        B arrays (N_b, R_b) (required for a ragged batch; zero-padded to the widest), y the data of construction minus
        their mean.  Returns ``(gram (B, R + 1, R + 1), logdet (B,), info (B,))`` as device tensors: y is the last
        column, logdet = log det Sigma, info the 1-based row of a failed pivot (that problem's gram and logdet are
        NaN).  W > 63 raises ``NotImplementedError``.  No host synchronisation."""
        res, _ = self._linear_gram(basis, pack_or_kernels)
        return res["gram"], res["logdet"], res["info"]

    @property
    def last_linear_device_ms(self):
        """Device time of the last :meth:`linear_gram_device` / :meth:`fit_linear` call (waits for it)."""
        return self._events_ms(self._linear_events)

    def fit_linear(self, basis, pack_or_kernels=None):
        """The generalised least squares fits of the B linear mean models (``basis`` as :meth:`linear_gram_device`):
        a :class:`gadfly_amd.linmodel.LinearFit` of numpy fields -- ``beta``, ``cov``, ``stderr``, ``chi2``, the
        profile log-likelihood ``ll``, the likelihood marginalised over beta ``ll_marginal``, ``ok``, ``ncols``,
        ``info``.  A problem whose matrix is not positive definite or whose basis is rank-deficient gets ``ok =
        False`` and NaN; the others are unaffected."""
        return self._fit_linear(basis, pack_or_kernels)[0]

    def _fit_linear(self, basis, pack_or_kernels):
        """:meth:`fit_linear`, and what :meth:`_linear_gram` returned with it."""
        from .linmodel import solve_normal_equations
        res, ncols = self._linear_gram(basis, pack_or_kernels)
        nrows = np.full(self.B, self.engine.N, dtype=np.int64) if self.rows is None else self.rows
        fit = solve_normal_equations(res["gram"].cpu().numpy(), res["logdet"].cpu().numpy(), nrows, ncols,
                                     res["info"].cpu().numpy())
        return fit, res

    def linear_value_and_grad_coefficients(self, basis, pack_or_kernels=None, marginal=False):
        """The log-likelihoods of the B linear mean models at their generalised least squares fits -- profiled over
        beta, or with ``marginal`` integrated over it under a flat prior -- and their gradients with respect to the
        celerite coefficients.  ``basis`` as :meth:`fit_linear`.  Returns ``(ll, grads)``: ll (B,)
        numpy, :meth:`fit_linear`'s ``ll`` or ``ll_marginal`` to the bit; grads in the engine's stacked layout,
        ``real`` (2, B, Jr), ``comp`` (4, B, Jc), ``diag_add`` (B,).  A problem whose fit failed (``ok`` False) gets
        NaN, the others are unaffected.  The fit is kept in :attr:`last_linear_fit`, the device time per stage in
        :attr:`last_linear_grad_ms`."""
        from .linmodel import linear_gradients
        self._grad_check_width()
        fit, res = self._fit_linear(basis, pack_or_kernels)
        g = linear_gradients(self.engine, *res["pack"], res["A"], fit, self.rows, bool(marginal),
                             self.grad_workspace_bytes, self.predict_workspace_bytes)
        stages = g.pop("stage_events")
        #: (workspace bytes of a group, number of groups, problems per group) of the last call's gf_loglike_grad step
        self.last_linear_grad_plan = g.pop("grad_plan")
        ms = {"gram": self._events_ms(res["events"]), "grad": stages.pop("grad_ms")}
        ms.update({k: self._events_ms(v) for k, v in stages.items()})
        #: the fit of the last :meth:`linear_value_and_grad` call and its device time in ms, stage by stage
        self.last_linear_fit, self.last_linear_grad_ms = fit, ms
        return (fit.ll_marginal if marginal else fit.ll), g

    def linear_value_and_grad(self, basis, S0, w0, Q, delta, wrt=("S0", "w0", "Q"), marginal=False,
                              return_fit=False):
        """:meth:`value_and_grad` under a linear mean fitted with the kernel: the profile (``marginal``: the
        marginal) log-likelihoods of y = A beta + eps at (B, J) SHO hyperparameter arrays and their gradients.
        Returns ``(ll, grads)`` -- with ``return_fit`` also the :class:`gadfly_amd.linmodel.LinearFit`; grads holds
        the names of ``wrt`` among ``"S0"``, ``"w0"``, ``"Q"`` ((B, J) each) and ``"diag"`` ((B,)).  W > 63 raises
        ``NotImplementedError``; every error is raised before anything is enqueued."""
        from .grad import parameter_vjp
        wrt = tuple(wrt)
        unknown = set(wrt) - {"S0", "w0", "Q", "diag"}
        if unknown:
            raise ValueError(f"unknown gradient names {sorted(unknown)}")
        shapes = {np.shape(np.atleast_2d(np.asarray(v))) for v in (S0, w0, Q)}
        if len(shapes) != 1 or next(iter(shapes))[0] != self.B:
            raise ValueError(f"S0, w0, Q of shapes {sorted(shapes)} do not hold the batch's {self.B} problems")
        pk = sho_coefficient_pack(S0, w0, Q, delta)
        ll, g = self.linear_value_and_grad_coefficients(basis, pk, marginal=marginal)
        out = {}
        if {"S0", "w0", "Q"} & set(wrt):
            gS0, gw0, gQ = parameter_vjp(S0, w0, Q, delta, g["real"], g["comp"], g["diag_add"])
            out.update({k: v for k, v in (("S0", gS0), ("w0", gw0), ("Q", gQ)) if k in wrt})
        if "diag" in wrt:
            out["diag"] = g["diag_add"]
        return (ll, out, self.last_linear_fit) if return_fit else (ll, out)

    def linear_trend_device(self, basis, beta):
        """The fitted trends A beta of the B problems on the device: (B, N), or a list of B series for a ragged batch
        or a list ``basis``; ``beta`` (B, R) as :meth:`fit_linear` gives it."""
        from .linmodel import stack_basis
        eng = self.engine
        torch = eng.torch
        as_list = isinstance(basis, (list, tuple)) or self.rows is not None
        A, ncols = stack_basis(basis, self.B, eng.N, self.rows)
        beta = torch.as_tensor(np.asarray(beta, dtype=np.float64), device=eng.device)
        if tuple(beta.shape) != (self.B, A.shape[2]):
            raise ValueError(f"beta of shape {tuple(beta.shape)} for {self.B} problems of {A.shape[2]} columns")
        A = torch.as_tensor(A, dtype=torch.float64, device=eng.device)
        trend = torch.matmul(A, beta[:, :, None])[:, :, 0]
        if not as_list:
            return trend
        rows = [eng.N] * self.B if self.rows is None else [int(n) for n in self.rows]
        return [trend[b, :n] for b, n in enumerate(rows)]

    def sample_conditional_device(self, pack_or_kernels=None, t=None, size=None, normals=None, seed=None,
                                  include_mean=True):
        """Draws from the conditional distribution of the B processes given their data, exact and with
        every cross-covariance between the queries, in O((N + M) W^2) per draw: no M x M matrix is formed.

        Returns a float64 device tensor (B, M), or (B, size, M) with ``size``, at the new times ``t`` -- every form
        :meth:`predict_device` takes as ``t=`` -- or (B, N) / (B, size, N) at the observed stamps without ``t``; a
        list of B tensors where ``t`` was a list or the batch is ragged.  The draws are of the noise-free process
        (what ``predict`` gives the mean and variance of) and are NOT centred: they are draws around the data.

        ``normals=(eps, eta)`` fixes the draw: standard normals of shapes (B, size, Nu) and (B, size, N) (no ``size``
        axis without ``size``), Nu the length of the union of observed and query stamps; lists of per-problem arrays
        for ragged layouts, shapes as :func:`gadfly_amd.conddraw.union_axes` reports them.  Otherwise they come from a
        device generator seeded with ``seed`` as :class:`BatchedSampler` seeds its own: the same seed gives the same
        bits.  ``size`` draws are ``size`` right-hand sides of one solve, ``gf_solve_batch_rhs``'s block of them per
        factorisation; the union-axis prior draws cost one fused sweep each.

        :attr:`last_predict_ll` ((B, size): the residuals' log-likelihoods), :attr:`last_predict_info`,
        :attr:`last_predict_plan` and :attr:`last_predict_device_ms` are filled from the solve as :meth:`predict_device`
        fills them; :attr:`last_conditional_info` holds the failing row of the UNION-axis factor per problem (0: none;
        such a problem's draws are NaN, the others are unaffected) and :attr:`last_conditional_ms` the device time
        split into sweeps, assembly, solve and the new-times launch.

        Raises before anything is enqueued: ``NotImplementedError`` for W > 63; ``ValueError`` for unsorted queries,
        ``normals`` of the wrong shape, a mean that varies along the rows together with ``t``, and -- for an
        exposure-integrated kernel -- a query closer than the exposure time to a different observed stamp or to
        another query (coincident stamps are merged and fine).  Packs made from raw coefficient arrays carry no
        exposure time and are not checked.  ``kernel=component`` draws are not offered."""
        from . import conddraw
        from .predict import check_width
        eng = self.engine
        Jr0, Jc0 = eng._struct0
        check_width(Jr0 + 2 * Jc0)
        if size is not None:
            size = int(size)
            if size < 1:
                raise ValueError("size must be a positive number of draws")
        ts = nq = mean = None
        as_list = self.rows is not None
        if t is not None:
            ts, nq, as_list = self._query_times(t)
            mean = self._query_mean(include_mean)
        if pack_or_kernels is None:
            pack, deltas = self._pack0, self._delta0
        else:
            pack = self._host_pack(pack_or_kernels)
            deltas = getattr(pack_or_kernels, "delta", None)
            if deltas is None and not isinstance(pack_or_kernels, tuple):
                deltas = self._deltas_of(pack_or_kernels)
        z, info, res, events = conddraw.conditional_draws(self, pack, self._host_axes(), ts, nq, deltas, size, normals,
                                                          seed, mean, include_mean)
        self.last_predict_plan = (res["workspace_bytes"], res["groups"], res["group_size"])
        self._predict_events, self._predict_at_events = res["events"], events["at"]
        self.last_predict_ll = res["ll"] if self._pad_corr is None else res["ll"] + self._pad_corr[:, None]
        self.last_predict_info = res["info"]
        self.last_conditional_info = info
        self._cond_events = events
        if size is None:
            z = z[:, 0]
        if as_list:
            lens = self.rows if t is None else (nq if nq is not None else [ts.shape[1]] * self.B)
            return [z[b, ..., :int(n)] for b, n in enumerate(lens)]
        return z

    @property
    def last_conditional_ms(self):
        """Device time of the last :meth:`sample_conditional_device` call by part (synchronises): ``sweeps`` (the
        union-axis prior draws), ``assembly``, ``solve``, ``at`` (the new-times launch)."""
        return {k: self._events_ms(v) for k, v in self._cond_events.items()}

    def sample_conditional(self, pack_or_kernels=None, t=None, size=None, normals=None, seed=None, include_mean=True):
        """:meth:`sample_conditional_device`, returned as numpy (a list of arrays where that returns a list)."""
        return self._to_host(self.sample_conditional_device(pack_or_kernels, t=t, size=size, normals=normals,
                                                            seed=seed, include_mean=include_mean))

    def predict(self, pack_or_kernels=None, kernel=None, include_mean=True, return_alpha=False, t=None,
                return_var=False, wide=False):
        """:meth:`predict_device`, returned as numpy (lists of arrays for a ragged batch or a list of query times)."""
        out = self.predict_device(pack_or_kernels, kernel=kernel, include_mean=include_mean,
                                  return_alpha=return_alpha, t=t, return_var=return_var, wide=wide)
        return tuple(self._to_host(x) for x in out) if (return_alpha or return_var) else self._to_host(out)

    def evaluate_device(self, pack=None):
        """Enqueue one evaluation per problem; returns the (B,) device tensor (no host sync).

        Accuracy guard (device side): with a generator period > 1 the rows between anchors carry a
        rotation error that the log-likelihood amplifies by the problem's condition number, and the
        period was chosen from the conditioning of EARLIER evaluations.  Every evaluation therefore
        also leaves a flag per problem on the device -- GEN_ERR * period * max(a) / min(d) above the
        target, from the min pivot its own reduction returns -- and :meth:`resolve` (called by
        :meth:`evaluate`, :meth:`calibrate`, or by the caller before reading asynchronous results)
        repeats flagged evaluations with exact rows, writing the corrected values into the tensor
        returned here.  A walker that wanders into a badly conditioned region is thus never silently
        evaluated at a period its conditioning does not allow.
        """
        eng = self.engine
        if pack is not None:
            eng.use_coefficients(pack)
            self._safe = self._diag_nonneg and bool(getattr(pack, "psd_safe", False))
        elif not hasattr(self, "_safe"):
            self._safe = self._init_safe
        eng.two_sweep = bool(self.two_sweep and self._safe)
        # small batches of long series are chunked in time as well (exact, see engine.evaluate)
        out = eng.evaluate()[0]
        if self._pad_corr is not None:
            out = out + self._pad_corr      # ragged batch: the missing-data rows' constants (-inf / NaN stay)
        period = int(eng.generator_period)
        if eng._fused_ok() or eng._wide_ok():
            torch = eng.torch
            acc = eng.last_acc()
            amax = eng._pack.diag_add if eng.diag is None else eng._pack.diag_add + eng._diag_amax
            # min pivot and largest diagonal of THIS evaluation (what calibrate() looks at; the
            # engine's own state may belong to a guard rerun of an older pack by then); a two-sweep
            # evaluation has the nominal pass' pivots only: margin (engine.TWO_SWEEP_MARGIN)
            dmin = acc[:, 2].clone()
            if getattr(eng, "_two_sweep_used", False):
                dmin = dmin / eng.TWO_SWEEP_MARGIN
            self._last_cond = (dmin, amax)
            flag = None
            if period > 1:
                # a non-positive pivot (failed factorisation: -inf either way) is not an accuracy case
                # (GEN_ERR * period + the phase-quantum term of a time axis far from zero: engine.PHASE_ERR)
                flag = (eng.generator_error_coefficient(period) * amax > self.generator_target * dmin) & (dmin > 0)
            if getattr(eng, "_two_sweep_used", False):
                # no final pass ran: a pivot that rounding pushed below zero inside a chunk shows up as a
                # non-finite value (det(I - X G) <= 0) -- repeated with the final pass by resolve()
                bad = ~torch.isfinite(out)
                flag = bad if flag is None else (flag | bad)
            viol = eng.steady_violations() if getattr(eng, "steady_used", False) else None
            if viol is not None:            # (a new tensor: the engine's buffer belongs to the next evaluation)
                flag = viol if flag is None else (flag | viol)
                self._viol_flags[id(out)] = viol
            if flag is not None:
                self._unresolved.append((out, flag, eng._pack, period))
                if len(self._unresolved) > 64:      # bound the backlog of a caller that never resolves
                    self.resolve()
        return out

    def resolve(self):
        """Look at the accuracy guards of all evaluations enqueued since the last call (one host
        sync) and repeat the flagged ones with exact generator rows, in place.  Returns the number
        of evaluations repeated."""
        if not self._unresolved:
            return 0
        eng = self.engine
        torch = eng.torch
        pending, self._unresolved = self._unresolved, []
        flags = torch.stack([f for _, f, _, _ in pending]).cpu().numpy()      # the sync
        redone = 0
        keep_pack, keep_period, keep_two = eng._pack, eng.generator_period, eng.two_sweep
        keep_steady, viols, self._viol_flags = eng.steady_state, self._viol_flags, {}
        eng.steady_state = False            # every repeat is the reference formulation: full rows to the end
        for (out, flag, pack, _), hit in zip(pending, flags):
            if not hit.any():
                continue
            if id(out) in viols:
                self.steady_reruns += int(viols[id(out)].sum().item())
            # (the pack is switched directly: use_coefficients() would also drop the engine's
            # construction-time coefficient list, which the stored-factor classes still need)
            eng._pack = pack
            eng.generator_period = 1
            eng.two_sweep = False           # the repeat is the reference formulation: exact rows, final pass
            exact = eng.evaluate()[0]
            if self._pad_corr is not None:
                exact = exact + self._pad_corr
            out.copy_(torch.where(flag, exact, out))
            redone += int(hit.sum())
        eng._pack, eng.generator_period, eng.two_sweep = keep_pack, keep_period, keep_two
        eng.steady_state = keep_steady
        self.guard_reruns += redone
        return redone

    def evaluate(self, kernels=None):
        out = self.evaluate_device(None if kernels is None else self.pack(kernels))
        if (self.auto_generator_period and self._last_cond is not None and len(self._unresolved) <= 1
                and (not self._unresolved or self._unresolved[0][0] is out)):
            # the common case -- nothing else pending: the values, the guard's flags and the two numbers the
            # period calibration reads come back in ONE copy (a chain of single evaluations paid four round trips)
            torch = self.engine.torch
            dmin, amax = self._last_cond
            parts = [out, dmin.min().reshape(1), amax.max().reshape(1)]
            if self._unresolved:
                parts.append(self._unresolved[0][1].to(out.dtype))
            host = torch.cat(parts).cpu().numpy()
            B = out.shape[0]
            if not self._unresolved or not host[B + 2:].any():
                self._unresolved, self._viol_flags = [], {}
                eng = self.engine
                cond = host[B + 1] / host[B] if host[B] > 0.0 else float("inf")
                eng.generator_period = eng.period_for_condition(float(cond), self.generator_target)
                return host[:B].copy()
        self.resolve()
        res = out.cpu().numpy()
        if self.auto_generator_period:
            # the result copy synchronised anyway: adapt the generator period of the NEXT
            # evaluation to the conditioning just seen (hyperparameters move slowly in a sampler)
            self._calibrate_last()
        return res

    def _calibrate_last(self):
        """(condition, period) from the min pivots of the last evaluation enqueued HERE."""
        eng = self.engine
        if self._last_cond is None:
            return eng.calibrate_generator(self.generator_target)
        dmin, amax = self._last_cond
        dmin = float(dmin.min().item())
        cond = float(amax.max().item()) / dmin if dmin > 0.0 else float("inf")
        eng.generator_period = eng.period_for_condition(cond, self.generator_target)
        return cond, eng.generator_period

    def calibrate(self):
        """After asynchronous evaluations (:meth:`evaluate_device`): set the generator period
        from the condition estimate of the last one.  Returns (condition, period)."""
        self.resolve()
        return self._calibrate_last()


def log_likelihood_batch(kernels, t, y, yerr=None, diag=None, mean=0.0, device=None):
    """log-likelihoods of B problems (numpy array of shape (B,)); -inf where K is not
    positive definite (celerite2's ``quiet=True`` convention)."""
    return BatchedLogLikelihood(kernels, t, y, yerr=yerr, diag=diag, mean=mean,
                                device=device).evaluate()


def predict_batch(kernels, t, y, yerr=None, diag=None, mean=0.0, kernel=None, device=None, t_pred=None,
                  return_var=False, wide=False):
    """One-shot form of :meth:`BatchedLogLikelihood.predict`: the conditional means of B problems at their observed
    times as numpy, (B, N) or a list of B arrays for ragged ``t``; ``kernel=`` selects the share of one part of the
    kernel (a list of B components, or one for all).  ``t_pred``: new times to predict at instead, what
    :meth:`BatchedLogLikelihood.predict` takes as ``t=`` (here ``t`` names the observed stamps).  ``return_var``: also
    the conditional variances, ``(mu, var)``.  ``wide``: the route for kernels wider than W = 63 (as there)."""
    return BatchedLogLikelihood(kernels, t, y, yerr=yerr, diag=diag, mean=mean,
                                device=device).predict(kernel=kernel, t=t_pred, return_var=return_var, wide=wide)


def sample_conditional_batch(kernels, t, y, yerr=None, diag=None, mean=0.0, t_pred=None, size=None, normals=None,
                             seed=None, device=None):
    """One-shot form of :meth:`BatchedLogLikelihood.sample_conditional_device`: posterior draws of B kernels given
    their data, at ``t_pred`` (what that method takes as ``t=``) or at the observed stamps, as a float64 device tensor
    (a list for ragged layouts)."""
    return BatchedLogLikelihood(kernels, t, y, yerr=yerr, diag=diag, mean=mean, device=device
                                ).sample_conditional_device(t=t_pred, size=size, normals=normals, seed=seed)


def _is_series_list(x):
    return isinstance(x, (list, tuple)) or (isinstance(x, np.ndarray) and x.dtype == object)


def _center_draws(x, size):
    """The reference's centring rule (gp.py:392: ``result -= result.mean(axis=0 if result.ndim == 2 else None)``) per
    problem, in place, on a tensor whose last axis is time: a single draw ((..., N), ``size`` None) loses its
    time-mean, ``size`` draws ((..., size, N)) their across-realisation mean."""
    x -= x.mean(dim=-1, keepdim=True) if size is None else x.mean(dim=-2, keepdim=True)
    return x


class BatchedSampler:
    """Light curves of B DIFFERENT kernels in one fused device sweep: ``y_b = L_b D_b^{1/2} eps_b`` with
    ``K_b = L_b D_b L_b^T``, what ``GaussianProcess(kernel_b, t, yerr).sample()`` gives one kernel at a time
    (the reference's gp.py:372-395).  The sweep that factors draws as it goes (gf_sample_fused: the pad
    column that carries the log-likelihood's forward solve carries the draw), so no factor is ever stored and a
    call costs what one :meth:`BatchedLogLikelihood.evaluate` costs.

    Constructor arguments and validation are :class:`BatchedLogLikelihood`'s without ``y``: ``t`` shared ((N,)),
    per problem ((B, N)) or -- ragged -- a list of B axes of different lengths (``yerr`` / ``diag`` then a scalar,
    one value per problem or a list of per-series arrays; ``mean`` a scalar or one value per problem).  A ragged
    batch is extended to the longest series with missing-data rows at the END of each series.  A draw is a
    FORWARD recurrence -- row n depends on rows < n only -- so pad rows cannot touch the real rows: they are cut
    off, and there is no pad correction of any kind.

    ``size`` draws per problem take ``size`` sweeps (cost: ``size`` x one sweep, each with its own factorisation in
    registers).  For many draws of ONE kernel use :meth:`GaussianProcess.sample_device`: its stored factor and
    MFMA ``dot_tril`` are the right tool there.  One wave (a workgroup of up to seven for wide kernels) works
    per problem: a batch below a few hundred problems leaves most of the chip idle.  That is accepted; there is
    no time-parallel sampler and no sharding of draws over several GPUs.

    Generator rows: exact every row by default (``generator_period = 1``, any power of two up to 64 may be set).
    With ``auto_generator_period = True`` the evaluator's rule applies instead: the period follows
    ``engine.period_for_condition`` on the max a / min d the last call measured (``generator_target``), and a
    call whose own conditioning does not allow the period it ran at is repeated with exact rows.

    Kernels whose structure or phases the fused sweeps do not take (W > 176, wide kernels that are not made of
    complex terms after rewriting, phases beyond 1e12 rad) raise ``NotImplementedError`` naming the condition."""

    def __init__(self, kernels, t, yerr=None, diag=None, mean=0.0, device=None, tile_rows=8192):
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        kernels = list(kernels)
        B = len(kernels)
        if B < 1:
            raise ValueError("dimension mismatch")
        self.rows = None                    # ragged batches: real rows per problem
        self._dmax = None
        if _is_ragged(t):
            if len(t) != B:
                raise ValueError("dimension mismatch")
            dd = diag
            if yerr is not None:
                dd = ([np.asarray(e, dtype=np.float64) ** 2 for e in yerr] if _is_series_list(yerr)
                      else np.asarray(yerr, dtype=np.float64) ** 2)
            zeros = [np.zeros(np.shape(x)) for x in t]
            t, _, d, self.rows, self._dmax, _, dt_min, tabs = _pad_ragged(t, zeros, dd, mean)
            mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (B,)).copy()
        else:
            t = np.ascontiguousarray(t, dtype=np.float64)
            if t.ndim not in (1, 2) or t.shape[-1] < 1 or (t.ndim == 2 and t.shape[0] not in (1, B)):
                raise ValueError("dimension mismatch")
            if np.any(np.diff(t, axis=-1) < 0.0):
                raise ValueError("The input coordinates must be sorted")
            N = t.shape[-1]
            d = None
            if yerr is not None:
                d = np.asarray(yerr, dtype=np.float64) ** 2
            elif diag is not None:
                d = np.asarray(diag, dtype=np.float64)
            if d is not None:
                if d.ndim == 0:
                    d = np.full(N, float(d))
                if d.ndim > 2 or d.shape[-1] != N or (d.ndim == 2 and d.shape[0] not in (1, B)):
                    raise ValueError("dimension mismatch")
            mean = np.asarray(mean, dtype=np.float64)
            if not (mean.ndim == 0 or mean.shape == (B,) or mean.shape == (B, N)):
                raise ValueError("dimension mismatch")
            dt_min = float(np.min(np.diff(t, axis=-1))) if N > 1 else None
            tabs = float(np.max(np.abs(t)))
        self._t, self._d, self._mean = t, d, mean
        self._dt_min, self._t_abs_max = dt_min, tabs
        self._B, self._N = B, int(t.shape[-1])
        self._device, self._tile_rows = device, tile_rows
        # (host work only: the term structures are compared here, the device is first touched by the first draw)
        self._coeffs = [k.get_device_coefficients() for k in kernels]
        from .engine import _coeff_pack
        _coeff_pack(self._coeffs)
        self._engine = None
        #: rows between exact re-anchorings of the row generator (1: exact rows, the default)
        self.generator_period = 1
        #: True: the evaluator's rule instead -- period from the measured conditioning, with its re-run
        self.auto_generator_period = False
        self.generator_target = 1e-9
        #: draws repeated with exact rows by the guard of the automatic period so far
        self.guard_reruns = 0
        self._auto_period = None
        self._info = None

    @property
    def B(self):
        return self._B

    @property
    def N(self):
        """Rows per problem (the longest series of a ragged batch)."""
        return self._N

    @property
    def engine(self):
        if self._engine is None:
            eng = StreamingBatch(self._coeffs, self._t, np.zeros((1, self._N)), diag=self._d,
                                 tile_rows=self._tile_rows, device=self._device)
            if self._dmax is not None:      # ragged: the condition estimates look at the REAL rows' diagonal
                eng._diag_amax = eng.torch.as_tensor(self._dmax, dtype=eng.torch.float64, device=eng.device)
            self._engine = eng
        return self._engine

    def pack(self, kernels):
        return self.engine.pack_coefficients([k.get_device_coefficients() for k in kernels])

    def pack_parameters(self, S0, w0, Q, delta):
        """Coefficient pack straight from (B, J) hyperparameter arrays (:func:`sho_coefficient_pack`)."""
        return self.engine.pack_arrays(*sho_coefficient_pack(S0, w0, Q, delta))

    @property
    def last_info(self):
        """Per problem: 0, or the 1-based row at which the last call's factorisation failed (synchronises)."""
        return None if self._info is None else self._info.cpu().numpy()

    def _check_normals(self, normals, size):
        """Shape of ``normals`` against the output's, on the host (before anything is enqueued)."""
        B, N = self._B, self._N

        def shape(x):                       # (a device tensor is not to be converted for this)
            return tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))

        if self.rows is not None:
            if not _is_series_list(normals) or len(normals) != B:
                raise ValueError("dimension mismatch")
            for x, n in zip(normals, self.rows):
                if shape(x) != ((int(n),) if size is None else (size, int(n))):
                    raise ValueError("dimension mismatch")
        elif shape(normals) != ((B, N) if size is None else (B, size, N)):
            raise ValueError("dimension mismatch")

    def _sweeps(self, eps, out, period):
        eng = self.engine
        torch = eng.torch
        eng.generator_period = int(period)
        dmin = info = None
        for r in range(eps.shape[1]):       # one sweep per draw
            m, i = eng.sample_fused(eps[:, r, :], out[:, r, :])
            dmin = m if dmin is None else torch.minimum(dmin, m)
            info = i if info is None else torch.maximum(info, i)
        return dmin, info

    def sample_device(self, pack=None, size=None, normals=None, seed=None, include_mean=True, center=True):
        """One draw per problem -- a float64 device tensor (B, N) -- or ``size`` draws, (B, size, N); a ragged
        batch returns a list of B tensors (N_b,) / (size, N_b).  ``size`` draws cost ``size`` sweeps.

        ``pack``: new kernels for this and the following calls (:meth:`pack`, :meth:`pack_parameters`).
        ``normals``: the standard normals eps to use, a host array or device tensor of the output's shape (a list
        for a ragged batch); otherwise they come from ONE ``torch.randn`` call for the whole (B[, size], N) block
        on the device, from a ``torch.Generator`` seeded with ``seed``.  ``center=True`` applies the
        reference's rule per problem (gp.py:392): the time-mean of a single draw is removed, the
        across-realisation mean of ``size`` draws.  ``center=False`` returns ``L D^{1/2} eps`` (+ mean) untouched.
        A problem whose matrix is not positive definite gets NaN in all its rows and its failing row in
        :attr:`last_info`; the other problems are unaffected."""
        if size is not None:
            size = int(size)
            if size < 1:
                raise ValueError("size must be a positive number of draws")
        if normals is not None:
            self._check_normals(normals, size)
        B, N, R = self._B, self._N, (1 if size is None else size)
        eng = self.engine
        torch = eng.torch
        f64 = dict(dtype=torch.float64, device=eng.device)
        if pack is not None:
            eng.use_coefficients(pack)
        with torch.cuda.device(eng.device):
            buf = torch.empty((B * R * N + 4,), **f64)      # (the sweeps read three elements past the end)
            buf[B * R * N:] = 0.0
            eps = buf[:B * R * N].view(B, R, N)
            if normals is None:
                gen = None
                if seed is not None:
                    gen = torch.Generator(device=eng.device)
                    gen.manual_seed(int(seed))
                torch.randn((B, R, N), generator=gen, out=eps)
            elif self.rows is not None:
                eps.zero_()
                for b, (x, n) in enumerate(zip(normals, self.rows)):
                    eps[b, :, :int(n)] = torch.as_tensor(x).to(**f64).reshape(R, int(n))
            else:
                eps.copy_(torch.as_tensor(normals).to(**f64).reshape(B, R, N))
            out = torch.empty((B, R, N), **f64)
            period = int(self.generator_period)
            if self.auto_generator_period:
                period = int(self._auto_period or eng.generator_period)
            dmin, info = self._sweeps(eps, out, period)
            if self.auto_generator_period:
                amax = eng._pack.diag_add if eng._diag_amax is None else eng._pack.diag_add + eng._diag_amax
                ok = info == 0
                if period > 1:
                    flag = (eng.generator_error_coefficient(period) * amax > self.generator_target * dmin) & ok
                    if bool(flag.any()):            # (host synchronisation, as the evaluator's resolve())
                        dmin, info = self._sweeps(eps, out, 1)
                        ok = info == 0
                        self.guard_reruns += 1
                worst = torch.where(ok, amax / dmin, torch.zeros_like(dmin)).max()
                self._auto_period = eng.period_for_condition(float(worst), self.generator_target)
            self._info = info
            out.masked_fill_((info != 0)[:, None, None], float("nan"))
            if include_mean and np.any(self._mean != 0.0):
                mu = torch.as_tensor(np.ascontiguousarray(self._mean)).to(**f64)
                out += mu.reshape((1, 1, 1) if mu.ndim == 0 else ((B, 1, 1) if mu.ndim == 1 else (B, 1, N)))
            if center and size is not None:
                _center_draws(out, size)
            if self.rows is not None:
                res = []
                for b, n in enumerate(self.rows):
                    x = out[b, :, :int(n)]
                    x = x[0] if size is None else x.contiguous()
                    res.append(_center_draws(x.clone(), None) if (center and size is None) else x)
                return res
            if size is None:
                out = out[:, 0, :]
                if center:
                    _center_draws(out, None)
            return out

    def sample(self, pack=None, size=None, normals=None, seed=None, include_mean=True, center=True):
        """:meth:`sample_device`, returned as numpy (a list of arrays for a ragged batch)."""
        out = self.sample_device(pack=pack, size=size, normals=normals, seed=seed, include_mean=include_mean,
                                 center=center)
        if isinstance(out, list):
            return [x.cpu().numpy() for x in out]
        return out.cpu().numpy()


def sample_batch(kernels, t, yerr=None, diag=None, mean=0.0, size=None, normals=None, seed=None, device=None):
    """One-shot form of :class:`BatchedSampler`: draws of B kernels as a float64 device tensor (B, N) or
    (B, size, N) (a list for ragged ``t``), centred as the reference centres its draws -- ready for
    ``PowerSpectrum.from_flux``."""
    return BatchedSampler(kernels, t, yerr=yerr, diag=diag, mean=mean,
                          device=device).sample_device(size=size, normals=normals, seed=seed)
