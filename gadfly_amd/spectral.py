"""
Spectral log-likelihoods of B sums of SHO terms against an observed power spectrum, with analytic gradients
(``gf_spectral_like``).

gadfly compares a kernel's power spectrum with an observed one: its ``hyperparameters.json`` was fitted by chi-square
of sums of SHO spectra against the binned VIRGO spectrum (gadfly's notebooks/virgo_lc.ipynb), and
gadfly/tests/test_core.py:29-34 compares a draw's binned spectrum with ``kernel.get_psd``.
:class:`SpectralLikelihood` joins the two sides on the device: the observed power is the device copy a
:class:`gadfly_amd.PowerSpectrum` keeps, the model is ``TermConvolution.get_psd`` over a ``TermSum`` of ``SHOTerm`` s
plus a white floor, for B parameter sets at once and any number of terms up to 256:

    S_b(w) = sinc^2(delta_b w / 2) sum_j sqrt(2/pi) S0_j w0_j^4 / (((w - w0_j)(w + w0_j))^2 + w^2 w0_j^2 / Q_j^2) + c_b
    whittle:  l_b = - sum_k n_k (ln S_b(w_k) + P_k / S_b(w_k))       n_k: ordinates averaged into P_k (1 if raw)
    chi2:     l_b = - 1/2 sum_k ((P_k - S_b(w_k)) / e_k)^2           e_k: the spectrum's error

Both are log-likelihoods (to be maximised), summed over the used frequencies: those whose power and weight / error are
finite and whose weight / error is positive (the empty bins of ``.bin()`` are NaN and drop out, as with the notebook's
``nansum``).  :class:`SpectralLogLikelihood` is a ``torch.autograd.Function`` for ``torch.optim`` or a sampler.
Frequencies in uHz, power in ppm^2/uHz, delta in 1/uHz.

The curvature of both objectives is the Fisher information (``gf_spectral_fisher``)

    F_b = sum_k v_k grad S_b(w_k) grad S_b(w_k)^T,    v_k = n_k / S_k^2 (whittle),  v_k = 1 / e_k^2 (chi2)

in the parameter order S0_0 .. S0_{J-1}, w0_0 .., Q_0 .., floor: :meth:`SpectralLikelihood.fisher_device`.  From it
come the covariances and standard errors of a fit (:meth:`SpectralLikelihood.covariance`,
:meth:`SpectralLikelihood.standard_errors`) and the fit itself, a damped Fisher scoring of B problems in lockstep
(:meth:`SpectralLikelihood.fit`).
"""
import numpy as np

from . import _lib

__all__ = ["SpectralLikelihood", "SpectralLogLikelihood", "SpectralFit", "white_floor", "check_parameters",
           "parameter_index", "OBJECTIVES", "PARAMETERS", "MAX_TERMS", "DEFAULT_WORKSPACE_BYTES"]

OBJECTIVES = {"whittle": 0, "chi2": 1}
MAX_TERMS = 256                         # gf_spectral_like's limit on J
MAX_GROUP = 65535                       # problems per launch (the grid's second axis)
#: default cap on the workspace of one launch (the batch is split into groups beneath it)
DEFAULT_WORKSPACE_BYTES = 2 << 30


PARAMETERS = ("S0", "w0", "Q", "floor")     # the canonical order of the Fisher matrix's blocks


def parameter_index(names, J, what="wrt"):
    """Rows of the (3 J + 1)-parameter Fisher matrix the blocks ``names`` select, in the canonical order (S0, w0, Q,
    floor) whatever the order of ``names``; ValueError for an unknown name or an empty selection."""
    names = (names,) if isinstance(names, str) else tuple(names)
    bad = [k for k in names if k not in PARAMETERS]
    if bad or not names:
        raise ValueError(f"{what} holds unknown names {bad} (S0, w0, Q, floor)" if bad else f"{what} is empty")
    idx = [np.arange(i * J, (i + 1) * J if i < 3 else 3 * J + 1) for i, k in enumerate(PARAMETERS) if k in names]
    return np.concatenate(idx)


class SpectralFit:
    """What :meth:`SpectralLikelihood.fit` returns: ``S0, w0, Q`` (B, J), ``floor`` (B,) and ``ll`` (B,) at the last
    accepted point, ``iterations`` (B,), ``converged`` (B,) bool, and the covariance ``cov`` (B, P', P') of the free
    parameters there with ``cov_ok`` (B,) (see :meth:`SpectralLikelihood.covariance`); ``free`` names the blocks."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return (f"SpectralFit({int(np.sum(self.converged))} of {len(self.converged)} converged, "
                f"at most {int(np.max(self.iterations))} iterations, free={self.free})")


def _scaled_inverse(F):
    """(cov, ok) of a (B, P, P) stack: the inverse of each matrix through the Cholesky factor of its Marquardt-scaled
    form D^-1/2 F D^-1/2, D = diag F; NaN and ok = False where that is not positive definite or not finite."""
    F = np.asarray(F, dtype=np.float64)
    B, P, _ = F.shape
    cov = np.full((B, P, P), np.nan)
    d = np.diagonal(F, axis1=1, axis2=2)
    ok = np.all(np.isfinite(F.reshape(B, -1)), axis=1) & np.all(d > 0.0, axis=1)
    if not ok.any():
        return cov, ok
    rows = np.flatnonzero(ok)
    s = 1.0 / np.sqrt(d[rows])
    ss = s[:, :, None] * s[:, None, :]          # (exactly symmetric, and so is everything scaled by it)
    C = F[rows] * ss
    try:
        L = np.linalg.cholesky(C)
        good = np.ones(len(rows), dtype=bool)
    except np.linalg.LinAlgError:               # one of them is not positive definite: find out which
        L = np.zeros_like(C)
        good = np.zeros(len(rows), dtype=bool)
        for i in range(len(rows)):
            try:
                L[i] = np.linalg.cholesky(C[i])
                good[i] = True
            except np.linalg.LinAlgError:
                L[i] = np.eye(P)
    Li = np.linalg.inv(L)
    inv = np.matmul(np.transpose(Li, (0, 2, 1)), Li)
    inv = (0.5 * (inv + np.transpose(inv, (0, 2, 1)))) * ss
    good &= np.all(np.isfinite(inv.reshape(len(rows), -1)), axis=1)
    cov[rows[good]] = inv[good]
    ok[rows[~good]] = False
    return cov, ok


def white_floor(yerr, d):
    """Expected periodogram of white noise of standard deviation ``yerr`` [ppm] sampled every ``d`` [1/uHz] under
    ``PowerSpectrum``'s normalisation (``norm = d / sqrt(2 pi) / N``): ``yerr^2 d / sqrt(2 pi)`` [ppm^2/uHz]."""
    return np.asarray(yerr, dtype=np.float64) ** 2 * float(d) / np.sqrt(2.0 * np.pi)


def _host(x):
    """A float64 numpy array of a numpy-like or a torch tensor (detached, copied to the host)."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def check_parameters(S0, w0, Q, delta, floor=None, rows=1):
    """Host-side check and layout of one call's parameters (no device call): ``S0, w0, Q`` of shape (B, J) or (J,),
    ``delta`` and ``floor`` scalar or (B,), for a spectrum of ``rows`` power rows (1: shared by all problems).
    Returns contiguous float64 arrays ``(S0, w0, Q [B][J], delta [B], floor [B] or None)``; ValueError otherwise."""
    S0, w0, Q = (_host(v) for v in (S0, w0, Q))
    if not (S0.shape == w0.shape == Q.shape) or S0.ndim not in (1, 2):
        raise ValueError(f"S0, w0, Q must share one shape (B, J) or (J,) (shapes {S0.shape}, {w0.shape}, {Q.shape})")
    if S0.ndim == 1:
        S0, w0, Q = (np.broadcast_to(v, (rows,) + v.shape) for v in (S0, w0, Q))
    B, J = S0.shape
    if B < 1 or J < 1:
        raise ValueError(f"no problems or no terms (shape {S0.shape})")
    if J > MAX_TERMS:
        raise ValueError(f"{J} terms: spectral likelihoods take at most {MAX_TERMS}")
    if rows != 1 and rows != B:
        raise ValueError(f"{B} parameter sets for a spectrum of {rows} power rows (one row, or one per problem)")
    for name, v, ok in (("S0", S0, S0 >= 0.0), ("w0", w0, w0 > 0.0), ("Q", Q, Q > 0.0)):
        if not np.all(np.isfinite(v)) or not np.all(ok):
            raise ValueError(f"{name} must be finite and {'>= 0' if name == 'S0' else '> 0'}")
    out = [np.ascontiguousarray(v) for v in (S0, w0, Q)]
    for name, v in (("delta", delta), ("floor", floor)):
        if v is None:
            if name == "delta":
                raise ValueError("delta must be given (0 for no exposure integration)")
            out.append(None)
            continue
        v = _host(v)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
            raise ValueError(f"{name} must be a scalar or of shape ({B},) (shape {v.shape})")
        if not np.all(np.isfinite(v)) or np.any(v < 0.0):
            raise ValueError(f"{name} must be finite and >= 0")
        out.append(np.array(np.broadcast_to(v, (B,))))
    return tuple(out)


def kernel_parameters(kernels):
    """(S0, w0, Q [B][J], delta [B]) of a list of SHO-sum kernels (``StellarOscillatorKernel``, a ``TermSum`` of
    ``SHOTerm`` s, one ``SHOTerm``; exposure-integrated or not), all of the same number of terms."""
    from .terms import SHOTerm, TermConvolution
    rows, deltas = [], []
    for k in kernels:
        base, delta = (k.term, float(k.delta)) if isinstance(k, TermConvolution) else (k, 0.0)
        terms = getattr(base, "terms", None)
        if terms is None:
            terms = (base,)
        if len(terms) == 0 or not all(isinstance(t, SHOTerm) for t in terms):
            raise ValueError("spectral likelihoods take sums of SHO terms only")
        rows.append([(t.S0, t.w0, t.Q) for t in terms])
        deltas.append(delta)
    if len(rows) == 0 or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("the kernels of a batch must have the same number of terms (and there must be one)")
    p = np.asarray(rows, dtype=np.float64)
    return p[:, :, 0], p[:, :, 1], p[:, :, 2], np.asarray(deltas)


class SpectralLikelihood:
    """Reusable evaluator over one observed spectrum.

    ``spectrum``: a :class:`gadfly_amd.PowerSpectrum` with power (M,) shared by all problems, or (R, M) with one row
    per problem; its device copy (``from_flux``, ``from_lomb_scargle``) is used in place where there is one.
    ``objective``: "whittle" or "chi2".  ``weights``: n_k (whittle; default ``spectrum.counts``, else 1) or e_k (chi2;
    default ``spectrum.error``, required), of shape (M,) or the power's.  ``frequency_min`` / ``frequency_max`` [uHz]
    restrict the sum to a band.  Everything is checked on the host first; device buffers are made at the first
    evaluation."""

    def __init__(self, spectrum, objective="whittle", weights=None, frequency_min=None, frequency_max=None,
                 device=None):
        if objective not in OBJECTIVES:
            raise ValueError(f"objective must be one of {sorted(OBJECTIVES)} (got {objective!r})")
        self.objective = objective
        self.spectrum = spectrum
        freq = np.asarray(spectrum.frequency, dtype=np.float64)
        if freq.ndim != 1 or len(freq) < 1:
            raise ValueError(f"the frequency axis must be 1-D and not empty (shape {freq.shape})")
        if not np.all(np.isfinite(freq)) or np.any(np.diff(freq) < 0.0):
            raise ValueError("the frequencies of the spectrum must be finite and ascending")
        dev_power = getattr(spectrum, "_power_dev", None)
        shape = tuple(dev_power.shape) if dev_power is not None else np.shape(spectrum.power)
        if len(shape) not in (1, 2) or shape[-1] != len(freq):
            raise ValueError(f"power of shape {shape} on a frequency axis of {len(freq)} points")
        self.rows = 1 if len(shape) == 1 else int(shape[0])
        if self.rows < 1:
            raise ValueError("the spectrum has no rows")
        if weights is None:
            weights = spectrum.error if objective == "chi2" else getattr(spectrum, "counts", None)
            if weights is None and objective == "chi2":
                raise ValueError("objective 'chi2' needs errors: the spectrum has none (bin it, or pass `weights`)")
        if weights is not None:
            weights = np.asarray(_host(weights))
            if weights.shape not in ((len(freq),), (self.rows, len(freq))):
                raise ValueError(f"weights of shape {weights.shape} for power of shape {shape}")
        lo = -np.inf if frequency_min is None else float(frequency_min)
        hi = np.inf if frequency_max is None else float(frequency_max)
        keep = np.flatnonzero((freq >= lo) & (freq <= hi))
        if len(keep) == 0:
            raise ValueError(f"no frequency of the spectrum lies in [{lo}, {hi}] uHz")
        self._lo, self._hi = int(keep[0]), int(keep[-1]) + 1           # ascending axis: a contiguous band
        self.frequency = freq[self._lo:self._hi]
        self.omega = 2.0 * np.pi * self.frequency
        self.M = len(self.frequency)
        self._weights = None if weights is None else np.ascontiguousarray(np.atleast_2d(weights)[:, self._lo:self._hi])
        self._device = device
        self._dev = None
        self.workspace_bytes = DEFAULT_WORKSPACE_BYTES
        self.last_plan = None               # (workspace bytes, groups, problems per group) of the last call
        self.last_power_ptr = None          # the power pointer the last call's first launch received
        self._events = []
        self._used = self._info = None

    # ------------------------------------------------------------------------------------
    def _buffers(self):
        """Device buffers of the spectrum, made once: omega (M,), power (rows, M) with its row stride, weights."""
        if self._dev is not None:
            return self._dev
        torch = _lib.require_device()
        power = getattr(self.spectrum, "_power_dev", None)
        if power is not None:
            dev = power.device
            power = power.view(1, -1) if power.ndim == 1 else power
            if power.dtype != torch.float64 or power.stride(1) != 1:
                power = power.to(torch.float64).contiguous()
        else:
            dev = torch.device("cuda", torch.cuda.current_device()) if self._device is None \
                else torch.device(self._device)
            power = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(_host(self.spectrum.power))), device=dev)
        power = power[:, self._lo:self._hi]                             # a view: no copy, the row stride stays
        f64 = dict(dtype=torch.float64, device=dev)
        omega = torch.as_tensor(self.omega, **f64)
        weight = None if self._weights is None else torch.as_tensor(self._weights, **f64)
        self._dev = dict(device=dev, power=power, omega=omega, weight=weight,
                         power_bs=int(power.stride(0)) if power.shape[0] > 1 else 0,
                         weight_bs=int(weight.stride(0)) if weight is not None and weight.shape[0] > 1 else 0)
        return self._dev

    @property
    def power_device(self):
        """The (rows, M) device tensor of the observed power the launches read (a view of the spectrum's own)."""
        return self._buffers()["power"]

    def workspace_plan(self, B, J):
        """(doubles per problem, problems per group, number of groups) under ``self.workspace_bytes``."""
        from .rowcall import group_plan
        per = _lib.load().gf_spectral_work(1, int(self.M), int(J))
        per, group, _ = group_plan(per, B, self.workspace_bytes, f"no spectral workspace for M = {self.M}, J = {J}")
        group = min(group, MAX_GROUP)
        return per, group, (B + group - 1) // group

    def run_device(self, S0, w0, Q, delta, floor=None, grad=False, model=False):
        """Check, upload, launch group by group; nothing is copied back.  Returns a dict of device tensors: ``ll``,
        ``used``, ``info`` (B,) and, as asked, the gradients ``S0``, ``w0``, ``Q`` (B, J), ``floor`` (B,) and
        ``model`` (B, M).  The other calls are views of this one."""
        S0, w0, Q, delta, floor = check_parameters(S0, w0, Q, delta, floor, self.rows)
        B, J = S0.shape
        torch = _lib.require_device()
        lib = _lib.load()
        per, group, ngroups = self.workspace_plan(B, J)
        d = self._buffers()
        dev = d["device"]
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            pars = torch.as_tensor(np.stack([S0, w0, Q]), **f64)                        # (3, B, J)
            dl = torch.as_tensor(delta, **f64)
            fl = None if floor is None else torch.as_tensor(floor, **f64)
            work = torch.empty((group * per,), **f64)
            out = dict(ll=torch.empty((B,), **f64), used=torch.empty((B,), dtype=torch.int64, device=dev),
                       info=torch.empty((B,), dtype=torch.int32, device=dev))
            if grad:
                out.update(S0=torch.empty((B, J), **f64), w0=torch.empty((B, J), **f64),
                           Q=torch.empty((B, J), **f64), floor=torch.empty((B,), **f64))
            if model:
                out["model"] = torch.empty((B, self.M), **f64)

            def at(x, b0, per_problem=1):
                return None if x is None else x.data_ptr() + x.element_size() * b0 * per_problem

            self._events = []
            self.last_power_ptr = d["power"].data_ptr()
            for b0 in range(0, B, group):
                nb = min(group, B - b0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(lib.gf_spectral_like(
                    nb, self.M, J, OBJECTIVES[self.objective], at(pars[0], b0, J), at(pars[1], b0, J),
                    at(pars[2], b0, J), at(dl, b0), at(fl, b0), d["omega"].data_ptr(),
                    at(d["power"], b0, d["power_bs"]), d["power_bs"], at(d["weight"], b0, d["weight_bs"]),
                    d["weight_bs"], work.data_ptr(), at(out["ll"], b0), at(out["used"], b0), at(out["info"], b0),
                    at(out.get("S0"), b0, J), at(out.get("w0"), b0, J), at(out.get("Q"), b0, J),
                    at(out.get("floor"), b0), at(out.get("model"), b0, self.M), st), "gf_spectral_like")
                e1.record()
                self._events.append((e0, e1))
        self.last_plan = (8 * per * group, ngroups, group)
        self._used, self._info = out["used"], out["info"]
        return out

    @property
    def last_used(self):
        """(B,) counts of the frequencies the last call summed over."""
        return None if self._used is None else self._used.cpu().numpy()

    @property
    def last_info(self):
        """(B,) of the last call: 0, or k + 1 for the first used frequency k where the model was not positive."""
        return None if self._info is None else self._info.cpu().numpy()

    @property
    def last_device_ms(self):
        """Summed device time of the last call's launches (HIP events around each)."""
        if self._events:
            self._events[-1][1].synchronize()
        return sum(a.elapsed_time(b) for a, b in self._events)

    # ------------------------------------------------------------------------------------
    def model_device(self, S0, w0, Q, delta, floor=None):
        """(B, M) device tensor: the B kernels' spectra S_b at the evaluator's frequencies."""
        return self.run_device(S0, w0, Q, delta, floor, model=True)["model"]

    def evaluate_device(self, S0, w0, Q, delta, floor=None):
        """(B,) device tensor of log-likelihoods (-inf where a model spectrum is not positive, see ``last_info``)."""
        return self.run_device(S0, w0, Q, delta, floor)["ll"]

    def value_and_grad(self, S0, w0, Q, delta, floor=None, wrt=("S0", "w0", "Q", "floor")):
        """``(ll, g)``: the (B,) log-likelihoods and a dict of their gradients, ``g["S0"], g["w0"], g["Q"]`` of
        shape (B, J) and ``g["floor"]`` (B,), as numpy arrays (NaN for a problem whose ll is -inf)."""
        bad = [k for k in wrt if k not in ("S0", "w0", "Q", "floor")]
        if bad:
            raise ValueError(f"wrt holds unknown names {bad} (S0, w0, Q, floor)")
        out = self.run_device(S0, w0, Q, delta, floor, grad=True)
        return out["ll"].cpu().numpy(), {k: out[k].cpu().numpy() for k in wrt}

    def evaluate(self, kernels, floor=None):
        """(B,) numpy log-likelihoods of a list of SHO-sum kernels (as ``BatchedLogLikelihood`` takes them)."""
        S0, w0, Q, delta = kernel_parameters(kernels)
        return self.evaluate_device(S0, w0, Q, delta, floor).cpu().numpy()

    # ------------------------------------------------------------------------------------
    def fisher_plan(self, B, J):
        """(doubles per problem, problems per group, number of groups) of the Fisher call under
        ``self.workspace_bytes``."""
        from .rowcall import group_plan
        per = _lib.load().gf_spectral_fisher_work(1, int(self.M), int(J))
        per, group, _ = group_plan(per, B, self.workspace_bytes, f"no Fisher workspace for M = {self.M}, J = {J}")
        group = min(group, MAX_GROUP)
        return per, group, (B + group - 1) // group

    def _fisher_arguments(self, S0, w0, Q, delta, floor, wrt, log, what="wrt"):
        """The host side of a Fisher call: checked parameters, the selected rows and (B, P') parameter values."""
        S0, w0, Q, delta, floor = check_parameters(S0, w0, Q, delta, floor, self.rows)
        B, J = S0.shape
        idx = parameter_index(wrt, J, what)
        theta = np.concatenate([S0, w0, Q, (np.zeros(B) if floor is None else floor)[:, None]], axis=1)[:, idx]
        if log and np.any(theta == 0.0):
            raise ValueError("log=True needs every selected parameter to be non-zero (an S0 = 0, or floor None or 0)")
        return (S0, w0, Q, delta, floor), idx, theta

    def fisher_device(self, S0, w0, Q, delta, floor=None, wrt=PARAMETERS, log=False):
        """(B, P', P') device tensor: the Fisher information of the objective (see the module docstring) with respect
        to the blocks ``wrt`` in the canonical order S0, w0, Q, floor (P' = 3 J + 1 for all four).  ``log=True``: with
        respect to ln theta, ``F_ij theta_i theta_j``.  A problem whose model is not positive at a used frequency
        gets NaN (``last_info``); one without used frequencies a matrix of zeros.  The same host checks, uploads and
        group plan as :meth:`run_device`."""
        (S0, w0, Q, delta, floor), idx, theta = self._fisher_arguments(S0, w0, Q, delta, floor, wrt, log)
        B, J = S0.shape
        P = 3 * J + 1
        torch = _lib.require_device()
        lib = _lib.load()
        per, group, ngroups = self.fisher_plan(B, J)
        d = self._buffers()
        dev = d["device"]
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            pars = torch.as_tensor(np.stack([S0, w0, Q]), **f64)                        # (3, B, J)
            dl = torch.as_tensor(delta, **f64)
            fl = None if floor is None else torch.as_tensor(floor, **f64)
            work = torch.empty((group * per,), **f64)
            F = torch.empty((B, P, P), **f64)
            used = torch.empty((B,), dtype=torch.int64, device=dev)
            info = torch.empty((B,), dtype=torch.int32, device=dev)

            def at(x, b0, per_problem=1):
                return None if x is None else x.data_ptr() + x.element_size() * b0 * per_problem

            self._events = []
            self.last_power_ptr = d["power"].data_ptr()
            for b0 in range(0, B, group):
                nb = min(group, B - b0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(lib.gf_spectral_fisher(
                    nb, self.M, J, OBJECTIVES[self.objective], at(pars[0], b0, J), at(pars[1], b0, J),
                    at(pars[2], b0, J), at(dl, b0), at(fl, b0), d["omega"].data_ptr(),
                    at(d["power"], b0, d["power_bs"]), d["power_bs"], at(d["weight"], b0, d["weight_bs"]),
                    d["weight_bs"], work.data_ptr(), at(F, b0, P * P), at(used, b0), at(info, b0), st),
                    "gf_spectral_fisher")
                e1.record()
                self._events.append((e0, e1))
            if len(idx) != P:
                sel = torch.as_tensor(idx, dtype=torch.int64, device=dev)
                F = F.index_select(1, sel).index_select(2, sel)
            if log:
                th = torch.as_tensor(theta, **f64)
                F = F * th[:, :, None] * th[:, None, :]
        self.last_plan = (8 * per * group, ngroups, group)
        self._used, self._info = used, info
        return F

    def fisher(self, S0, w0, Q, delta, floor=None, wrt=PARAMETERS, log=False):
        """:meth:`fisher_device` as a (B, P', P') numpy array."""
        return self.fisher_device(S0, w0, Q, delta, floor, wrt, log).cpu().numpy()

    def covariance(self, S0, w0, Q, delta, floor=None, wrt=PARAMETERS, log=False):
        """``(cov, ok)``: the inverse Fisher matrices (B, P', P') and a (B,) bool.  Each matrix is inverted through
        the Cholesky factor of its Marquardt-scaled form D^-1/2 F D^-1/2, D = diag F (on the host, in LAPACK: DESIGN.md
        3.14); a problem whose matrix is not positive definite or holds NaN -- a zero diagonal entry, a term with
        S0 = 0, a model that is not positive -- gets NaN and ``ok = False``."""
        return _scaled_inverse(self.fisher(S0, w0, Q, delta, floor, wrt, log))

    def standard_errors(self, S0, w0, Q, delta, floor=None, wrt=PARAMETERS, log=False):
        """The square roots of the covariance's diagonal as a dict over ``wrt``: ``S0, w0, Q`` (B, J), ``floor``
        (B,); NaN for a problem :meth:`covariance` could not invert."""
        cov, _ = self.covariance(S0, w0, Q, delta, floor, wrt, log)
        se = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
        J = np.atleast_2d(_host(S0)).shape[-1]
        out, at = {}, 0
        for k in PARAMETERS:
            if k in wrt:
                n = J if k != "floor" else 1
                out[k] = se[:, at:at + n] if k != "floor" else se[:, at]
                at += n
        return out

    def fit(self, S0, w0, Q, delta, floor=None, free=PARAMETERS, max_iter=100, xtol=1e-10, damping=1e-3,
            max_step=1.0):
        """Maximise the objective of all B problems at once over the blocks ``free``, from the given start: a damped
        Fisher scoring (Levenberg-Marquardt) in u = ln theta, the problems in lockstep -- one gradient call and at
        most one Fisher call per iteration for the whole batch.  Per problem, with lambda starting at ``damping``:

            F_u = F o theta theta^T,  g_u = g o theta        at the accepted point
            d = solve(F_u + lambda diag(F_u), g_u);   d *= min(1, max_step / max|d|)
            ll' = ll(exp(u + d))
            if ll' finite and ll' >= ll:  accept; lambda = max(lambda / 10, 1e-9); converged if max|d| < xtol
            else:                         reject; lambda = min(10 lambda, 1e9)

        Converged and failed problems are frozen; parameters outside ``free`` keep their bits.  Free parameters must
        be > 0 (ValueError).  A problem whose start is -inf or that has no used frequency ends with
        ``converged = False`` and leaves the others alone.  Returns a :class:`SpectralFit`."""
        (S0, w0, Q, delta, floor), idx, theta = self._fisher_arguments(S0, w0, Q, delta, floor, free, False, "free")
        if np.any(theta <= 0.0):
            raise ValueError("free parameters must be > 0 (the fit works in their logarithms)")
        free = tuple(k for k in PARAMETERS if k in free)
        B, J = S0.shape
        full = np.concatenate([S0, w0, Q, (np.zeros(B) if floor is None else floor)[:, None]], axis=1)

        def split(th):
            """The call arguments at the free parameters ``th`` (the others as given)."""
            p = full.copy()
            p[:, idx] = th
            return p[:, :J], p[:, J:2 * J], p[:, 2 * J:3 * J], delta, (None if floor is None else p[:, 3 * J])

        def value_and_gradient(th):
            ll, g = self.value_and_grad(*split(th))
            return ll, np.concatenate([g[k] if k != "floor" else g[k][:, None] for k in PARAMETERS], axis=1)[:, idx]

        u = np.log(theta)
        ll, g = value_and_gradient(np.exp(u))
        active = np.isfinite(ll) & (self.last_used > 0) & np.all(np.isfinite(g), axis=1)
        lam = np.full(B, float(damping))
        iterations = np.zeros(B, dtype=np.int64)
        converged = np.zeros(B, dtype=bool)
        Fu, stale = None, True
        for _ in range(int(max_iter)):
            if not active.any():
                break
            th = np.exp(u)
            if stale:
                Fu = self.fisher(*split(th), wrt=free, log=True)
                stale = False
            gu = g * th
            d = np.zeros_like(u)
            rows = np.flatnonzero(active)
            diag = np.eye(len(idx)) * np.diagonal(Fu[rows], axis1=1, axis2=2)[:, None, :]
            A = Fu[rows] + lam[rows, None, None] * diag
            try:
                d[rows] = np.linalg.solve(A, gu[rows][:, :, None])[:, :, 0]
            except np.linalg.LinAlgError:       # a singular system among them: one by one
                for i, b in enumerate(rows):
                    try:
                        d[b] = np.linalg.solve(A[i], gu[b])
                    except np.linalg.LinAlgError:
                        d[b] = np.nan
            solved = active & np.all(np.isfinite(d), axis=1)
            d[~solved] = 0.0
            big = np.max(np.abs(d), axis=1)
            d *= np.minimum(1.0, float(max_step) / np.where(big > 0.0, big, 1.0))[:, None]
            step = np.max(np.abs(d), axis=1)
            ll2, g2 = value_and_gradient(np.exp(u + d))
            accept = solved & np.isfinite(ll2) & (ll2 >= ll)
            reject = active & ~accept
            iterations[active] += 1
            u[accept] += d[accept]
            ll[accept], g[accept] = ll2[accept], g2[accept]
            lam[accept] = np.maximum(lam[accept] / 10.0, 1e-9)
            lam[reject] = np.minimum(lam[reject] * 10.0, 1e9)
            done = accept & (step < float(xtol))
            converged |= done
            active &= ~done
            stale = bool(accept.any())
        a0, aw, aq, _, fl = split(np.exp(u))
        cov, cov_ok = self.covariance(a0, aw, aq, delta, fl, wrt=free)
        return SpectralFit(S0=np.array(a0), w0=np.array(aw), Q=np.array(aq),
                           floor=np.zeros(B) if fl is None else np.array(fl), ll=ll, iterations=iterations,
                           converged=converged, cov=cov, cov_ok=cov_ok, free=free)


def _function():
    import torch

    class SpectralLogLikelihood(torch.autograd.Function):
        """``SpectralLogLikelihood.apply(S0, w0, Q, floor, evaluator, delta)``: the (B,) log-likelihoods of a
        :class:`SpectralLikelihood` at tensors of SHO hyperparameters ((B, J) or (J,)) and white floors (None, a
        scalar or (B,)), differentiable with respect to S0, w0, Q and floor (the device gradient of
        :meth:`SpectralLikelihood.value_and_grad`)."""

        @staticmethod
        def forward(ctx, S0, w0, Q, floor, evaluator, delta):
            ll, g = evaluator.value_and_grad(S0, w0, Q, delta, floor)
            like = dict(dtype=S0.dtype, device=S0.device)
            ctx.save_for_backward(*(torch.as_tensor(g[k], **like) for k in ("S0", "w0", "Q", "floor")))
            ctx.shapes = [tuple(x.shape) for x in (S0, w0, Q)] + \
                [tuple(floor.shape) if torch.is_tensor(floor) else None]
            return torch.as_tensor(ll, **like)

        @staticmethod
        def backward(ctx, grad_output):
            gS0, gw0, gQ, gf = ctx.saved_tensors
            go = grad_output[:, None]
            grads = [(go * g).sum_to_size(s) for g, s in zip((gS0, gw0, gQ), ctx.shapes)]
            gfl = None if ctx.shapes[3] is None else (grad_output * gf).sum_to_size(ctx.shapes[3])
            return grads[0], grads[1], grads[2], gfl, None, None

    return SpectralLogLikelihood


def __getattr__(name):
    # the autograd Function needs torch: made on first use, so that importing the package does not import torch
    if name == "SpectralLogLikelihood":
        cls = _function()
        globals()[name] = cls
        return cls
    raise AttributeError(f"module 'gadfly_amd.spectral' has no attribute {name!r}")
