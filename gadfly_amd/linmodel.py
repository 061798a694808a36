"""
Linear mean models under batched kernels: y = A beta + eps, eps ~ N(0, Sigma_b), Sigma_b = K_b + diag.

``gf_linear_gram`` sweeps every problem forwards once and returns the (R + 1) x (R + 1) Gram matrix
[A | y]^T Sigma^-1 [A | y] with sum log D: no upper solve, nothing of size N comes back.  The generalised least squares
fit, its covariance, the profile likelihood and the likelihood marginalised over beta follow from it on the host
(:func:`solve_normal_equations`, pure numpy).  The groups under the byte cap and the launches are
:mod:`gadfly_amd.rowcall`'s.
"""
import numpy as np

from . import _lib
from .rowcall import GroupedCall, check_pack_batch, group_plan

__all__ = ["MAX_COLUMNS", "check_width", "workspace_plan", "stack_basis", "linear_gram", "solve_normal_equations",
           "LinearFit", "quarter_polynomial_basis", "fit_linear_batch", "DEFAULT_WORKSPACE_BYTES",
           "quadform_gradients", "linear_gradients"]

#: default cap on the workspace of one call (the batch is split into groups beneath it)
DEFAULT_WORKSPACE_BYTES = _lib.GF_SOLVE_WORKSPACE_BYTES
#: most columns a design matrix may hold
MAX_COLUMNS = _lib.GF_LINEAR_MAX_COLS

#: a scaled normal matrix (unit diagonal) whose smallest Cholesky pivot falls below this is called rank-deficient:
#: its condition number is beyond ~1e12, where float64 leaves beta no digits worth reporting
RANK_PIVOT_MIN = 1e-12


def check_width(W, what="this kernel"):
    """The one-wave row kernel's width limit: NotImplementedError beyond it."""
    if W > _lib.GF_SOLVE_MAX_WIDTH:
        raise NotImplementedError(
            f"linear mean models take celerite widths W <= {_lib.GF_SOLVE_MAX_WIDTH} (one wave per problem); "
            f"{what} has W = {W}")


def workspace_plan(N, W, B, R, cap_bytes=DEFAULT_WORKSPACE_BYTES):
    """(doubles per problem, problems per group, number of groups) of a gf_linear_gram call with R columns."""
    check_width(W)
    if not 1 <= int(R) <= MAX_COLUMNS:
        raise ValueError(f"a design matrix holds 1 .. {MAX_COLUMNS} columns, not {int(R)}")
    return group_plan(_lib.load().gf_linear_gram_work(int(N), int(W), int(R)), B, cap_bytes,
                      f"no linear-model workspace for N = {N}, W = {W}, R = {R}")


def stack_basis(basis, B, N, rows=None):
    """The design matrices of B problems of N (padded) rows as one host array.

    ``basis``: (N, R) shared by all problems, (B, N, R), or a list of B arrays (N_b, R_b) -- required for a ragged
    batch (``rows``: the real rows per problem), allowed otherwise; the column counts of a list may differ.  Returns
    (A (1 or B, N, R) float64, zero-padded rows and columns; ncols (B,) int64)."""
    if isinstance(basis, (list, tuple)) or (isinstance(basis, np.ndarray) and basis.dtype == object):
        mats = [np.asarray(a, dtype=np.float64) for a in basis]
        if len(mats) != B:
            raise ValueError(f"basis= holds {len(mats)} design matrices for a batch of {B} problems")
        want = [N] * B if rows is None else [int(n) for n in rows]
        if any(a.ndim != 2 or a.shape[0] != n for a, n in zip(mats, want)):
            raise ValueError("dimension mismatch")
        ncols = np.array([a.shape[1] for a in mats], dtype=np.int64)
        if np.any(ncols < 1) or np.any(ncols > MAX_COLUMNS):
            raise ValueError(f"a design matrix holds 1 .. {MAX_COLUMNS} columns, not {ncols.tolist()}")
        A = np.zeros((B, N, int(ncols.max())))
        for b, a in enumerate(mats):
            A[b, :a.shape[0], :a.shape[1]] = a
        return A, ncols
    if rows is not None:
        raise ValueError("a ragged batch takes basis= as a list of one (N_b, R_b) design matrix per series")
    A = np.asarray(basis, dtype=np.float64)
    if A.ndim == 2:
        A = A[None]
    if A.ndim != 3 or A.shape[0] not in (1, B) or A.shape[1] != N:
        raise ValueError("dimension mismatch")
    if not 1 <= A.shape[2] <= MAX_COLUMNS:
        raise ValueError(f"a design matrix holds 1 .. {MAX_COLUMNS} columns, not {A.shape[2]}")
    return np.ascontiguousarray(A), np.full(B, A.shape[2], dtype=np.int64)


def linear_gram(engine, Jr, Jc, real, comp, diag_add, A, nobs=None, cap_bytes=DEFAULT_WORKSPACE_BYTES):
    """Enqueue ``gf_linear_gram`` over an engine's data (t, y - mean, diag on the device) for stacked host coefficient
    arrays of its ORIGINAL term structure.  ``A``: float64 device tensor (1 or B, N, R), row-major; ``nobs``: (B,)
    real rows per problem, or None for N.  Returns a dict of device tensors -- ``gram`` (B, R + 1, R + 1), ``logdet``
    (B,), ``info`` (B,) -- with the plan and ``events`` as :func:`gadfly_amd.predict.solve_batch`.  No host
    synchronisation."""
    import torch
    W = Jr + 2 * Jc
    if (Jr, Jc) != engine._struct0:
        raise ValueError("coefficient pack does not match the batch structure")
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, diag_add)
    if A.ndim != 3 or A.shape[0] not in (1, B) or A.shape[1] != N or A.dtype != torch.float64:
        raise ValueError(f"design matrices of shape {tuple(A.shape)} for a batch of {B} problems of {N} rows")
    R = int(A.shape[2])
    plan = workspace_plan(N, W, B, R, cap_bytes)
    if nobs is not None:
        nobs = np.ascontiguousarray(nobs, dtype=np.int64)
        if nobs.shape != (B,) or np.any(nobs < 1) or np.any(nobs > N):
            raise ValueError("dimension mismatch")
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        A = A.to(engine.device).contiguous()
        abs_ = 0 if A.shape[0] == 1 else N * R
        nobs = None if nobs is None else torch.as_tensor(nobs, dtype=torch.int64, device=engine.device)
        rc = GroupedCall(engine, "gf_linear_gram", plan, (real, comp, diag_add))
        gram = torch.empty((B, R + 1, R + 1), **f64)
        logdet = torch.empty((B,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        events = rc.run(lambda g: g.launch(
            g.nb, N, R, Jr, Jc, *g.coef[0], *g.data, g.at(nobs), g.at(A, abs_), R, abs_, *g.work,
            g.at(gram, (R + 1) * (R + 1)), g.at(logdet), g.at(info), g.stream))
        return dict(gram=gram, logdet=logdet, info=info, events=events, **rc.plan)


class LinearFit:
    """What :func:`solve_normal_equations` returns, numpy fields over the B problems:

    ``beta`` (B, R) and ``stderr`` (B, R), ``cov`` (B, R, R) -- entries beyond a problem's ``ncols`` are zero --,
    ``factor`` (B, R, R) upper triangular with factor factor^T = cov to rounding (the scaled inverse Cholesky factor),
    ``chi2`` = y^T Sigma^-1 y - g^T beta, ``ll`` the profile log-likelihood, ``ll_marginal`` the log-likelihood
    marginalised over beta under a flat prior, ``logdet`` = log det Sigma, ``logdet_normal`` = log det A^T Sigma^-1 A,
    ``ok`` (False: NaN in every field of that problem), ``ncols``, ``nrows``, ``info``."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return f"LinearFit(B={len(self.ok)}, ok={int(np.sum(self.ok))}, R={self.beta.shape[1]})"


def _cholesky_each(C):
    """Lower Cholesky factors of a stack of matrices: all at once, one by one if any of them fails.  Returns
    (L, good); L of a failed one is the identity."""
    try:
        return np.linalg.cholesky(C), np.ones(len(C), dtype=bool)
    except np.linalg.LinAlgError:               # one of them is not positive definite: find out which
        L = np.zeros_like(C)
        good = np.zeros(len(C), dtype=bool)
        for i in range(len(C)):
            try:
                L[i] = np.linalg.cholesky(C[i])
                good[i] = True
            except np.linalg.LinAlgError:
                L[i] = np.eye(C.shape[1])
        return L, good


def solve_normal_equations(gram, logdet, nrows, ncols, info=None):
    """The generalised least squares fits of B problems from their Gram matrices, in numpy.

    ``gram`` (B, C, C) = [A | y]^T Sigma^-1 [A | y] with y the LAST column and A zero-padded to C - 1 columns;
    ``logdet`` (B,) = log det Sigma; ``nrows`` (B,) rows and ``ncols`` (B,) real columns per problem.  The normal
    matrix is scaled to a unit diagonal and factored by a batched Cholesky (one by one if one of them fails); a
    problem whose matrix is not finite, not positive definite or rank-deficient (:data:`RANK_PIVOT_MIN`) gets
    ``ok = False`` and NaN, the others are unaffected.  Returns a :class:`LinearFit`."""
    gram = np.asarray(gram, dtype=np.float64)
    if gram.ndim != 3 or gram.shape[1] != gram.shape[2] or gram.shape[1] < 2:
        raise ValueError("dimension mismatch")
    B, C, _ = gram.shape
    logdet = np.asarray(logdet, dtype=np.float64).reshape(-1)
    nrows = np.broadcast_to(np.asarray(nrows, dtype=np.int64), (B,)).copy()
    ncols = np.broadcast_to(np.asarray(ncols, dtype=np.int64), (B,)).copy()
    if logdet.shape != (B,) or np.any(ncols < 1) or np.any(ncols > C - 1):
        raise ValueError("dimension mismatch")
    info = np.zeros(B, dtype=np.int32) if info is None else np.asarray(info, dtype=np.int32).reshape(-1)
    R = C - 1
    nan = np.nan
    beta, cov, fac = np.full((B, R), nan), np.full((B, R, R), nan), np.full((B, R, R), nan)
    chi2, ldn = np.full(B, nan), np.full(B, nan)
    ok = np.zeros(B, dtype=bool)
    for r in np.unique(ncols):
        idx = np.flatnonzero(ncols == r)
        M, g, yy = gram[idx, :r, :r], gram[idx, :r, R], gram[idx, R, R]
        d = np.diagonal(M, axis1=1, axis2=2)
        fine = (np.all(np.isfinite(gram[idx].reshape(len(idx), -1)), axis=1) & np.all(d > 0.0, axis=1)
                & np.isfinite(logdet[idx]) & (info[idx] == 0))
        if not fine.any():
            continue
        idx, M, g, yy, d = idx[fine], M[fine], g[fine], yy[fine], d[fine]
        s = 1.0 / np.sqrt(d)
        ss = s[:, :, None] * s[:, None, :]      # (exactly symmetric, and so is everything scaled by it)
        L, good = _cholesky_each(M * ss)
        piv = np.diagonal(L, axis1=1, axis2=2)
        good &= np.min(piv, axis=1) ** 2 > RANK_PIVOT_MIN
        Li = np.linalg.inv(L)
        inv = np.matmul(np.transpose(Li, (0, 2, 1)), Li)
        inv = (0.5 * (inv + np.transpose(inv, (0, 2, 1)))) * ss
        bt = np.matmul(inv, g[:, :, None])[:, :, 0]
        good &= np.all(np.isfinite(inv.reshape(len(idx), -1)), axis=1) & np.all(np.isfinite(bt), axis=1)
        k = idx[good]
        beta[k], cov[k], fac[k] = 0.0, 0.0, 0.0
        beta[k, :r] = bt[good]
        fac[k, :r, :r] = s[good][:, :, None] * np.transpose(Li[good], (0, 2, 1))
        cov[k, :r, :r] = inv[good]
        chi2[k] = yy[good] - np.sum(g[good] * bt[good], axis=1)
        ldn[k] = 2.0 * np.sum(np.log(piv[good]), axis=1) - 2.0 * np.sum(np.log(s[good]), axis=1)
        ok[k] = True
    log2pi = np.log(2.0 * np.pi)
    ll = -0.5 * (chi2 + logdet + nrows * log2pi)
    ll_marginal = ll - 0.5 * ldn + 0.5 * ncols * log2pi
    stderr = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
    return LinearFit(beta=beta, cov=cov, factor=fac, stderr=stderr, chi2=chi2, ll=ll, ll_marginal=ll_marginal,
                     logdet=np.where(ok, logdet, nan), logdet_normal=ldn, ok=ok, ncols=ncols, nrows=nrows, info=info)


def quarter_polynomial_basis(t, breaks, order):
    """Per-segment Legendre design matrix of one stitched series: (N, S (order + 1)).

    ``breaks``: the S + 1 ascending row offsets of the S segments (quarters), ``breaks[0] = 0``, ``breaks[S] = N``.
    Columns s (order + 1) + k hold P_k in segment s's own time scaled to [-1, 1] (first row -1, last row +1) and zero
    outside the segment.  A one-row segment gets the constant column only; its other columns are zero."""
    from numpy.polynomial import legendre
    t = np.asarray(t, dtype=np.float64)
    breaks = np.asarray(breaks, dtype=np.int64)
    order = int(order)
    if t.ndim != 1 or breaks.ndim != 1 or len(breaks) < 2 or order < 0:
        raise ValueError("dimension mismatch")
    if breaks[0] != 0 or breaks[-1] != len(t) or np.any(np.diff(breaks) < 1):
        raise ValueError(f"breaks {breaks.tolist()} are not ascending row offsets from 0 to N = {len(t)}")
    S, P = len(breaks) - 1, order + 1
    A = np.zeros((len(t), S * P))
    for s in range(S):
        a, b = int(breaks[s]), int(breaks[s + 1])
        ts = t[a:b]
        span = ts[-1] - ts[0]
        if b - a == 1 or not span > 0.0:
            A[a:b, s * P] = 1.0
            continue
        x = (2.0 * ts - (ts[0] + ts[-1])) / span
        A[a:b, s * P:(s + 1) * P] = legendre.legvander(x, order)
    return A


def fit_linear_batch(kernels, t, y, basis, yerr=None, diag=None, mean=0.0, device=None):
    """One-shot :meth:`gadfly_amd.BatchedLogLikelihood.fit_linear`: the GLS fits of B kernels' linear mean models."""
    from .batch import BatchedLogLikelihood
    return BatchedLogLikelihood(kernels, t, y, yerr=yerr, diag=diag, mean=mean, device=device).fit_linear(basis)


# ---- gradients of the profile and the marginal likelihood ----------------------------------------

def quadform_gradients(engine, Jr, Jc, real, comp, x, w=None, nobs=None):
    """Enqueue ``gf_quadform_grad`` over an engine's time axes: sum_r w_r x_r^T (d Sigma / d theta) x_r for every
    celerite coefficient of B problems.  ``x``: float64 device tensor (B, R, N), or (1, R, N) shared; ``w``: None
    (ones), or a float64 device tensor (R,) or (B, R); ``nobs``: (B,) real rows per problem, or None.  Returns a dict of
    device tensors in gf_loglike_grad's layout -- ``real`` (2, B, max(Jr, 1)), ``comp`` (4, B, max(Jc, 1)),
    ``diag_add`` (B,) -- and ``events``.  No host synchronisation."""
    import torch
    W = Jr + 2 * Jc
    check_width(W)
    B, N = engine.B, engine.N
    check_pack_batch(B, Jr, Jc, real, comp, np.zeros(B))
    if x.ndim != 3 or x.shape[0] not in (1, B) or x.shape[2] != N or x.dtype != torch.float64:
        raise ValueError(f"vectors of shape {tuple(x.shape)} for a batch of {B} problems of {N} rows")
    R = int(x.shape[1])
    if not 1 <= R <= MAX_COLUMNS + 1:
        raise ValueError(f"gf_quadform_grad takes 1 .. {MAX_COLUMNS + 1} vectors per problem, not {R}")
    if w is not None and (tuple(w.shape) not in ((R,), (B, R)) or w.dtype != torch.float64):
        raise ValueError(f"weights of shape {tuple(w.shape)} for {R} vectors in {B} problems")
    if nobs is not None:
        nobs = np.ascontiguousarray(nobs, dtype=np.int64)
        if nobs.shape != (B,) or np.any(nobs < 1) or np.any(nobs > N):
            raise ValueError("dimension mismatch")
    dev = engine.device
    f64 = dict(dtype=torch.float64, device=dev)
    lib, p = engine.lib, _lib.ptr
    per = int(lib.gf_quadform_grad_work(W, R))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        x = x.to(dev).contiguous()
        w = None if w is None else w.to(dev).contiguous()
        nobs = None if nobs is None else torch.as_tensor(nobs, dtype=torch.int64, device=dev)
        cr_ = torch.as_tensor(np.ascontiguousarray(real, dtype=np.float64), **f64)
        cc_ = torch.as_tensor(np.ascontiguousarray(comp, dtype=np.float64), **f64)
        work = torch.empty((B * per,), **f64)
        g_real = torch.zeros((2, B, max(Jr, 1)), **f64)
        g_comp = torch.zeros((4, B, max(Jc, 1)), **f64)
        g_diag = torch.empty((B,), **f64)
        t = engine.t
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = lib.gf_quadform_grad(
            B, N, R, Jr, Jc, p(cr_[0]), p(cr_[1]), p(cc_[0]), p(cc_[1]), p(cc_[2]), p(cc_[3]),
            p(t), engine._bs(t), p(nobs), p(x), 0 if x.shape[0] == 1 else R * N, N,
            p(w), 0 if w is None or w.ndim == 1 else R, p(work), per, p(g_real), p(g_comp), p(g_diag), stream)
        _lib.check(st, "gf_quadform_grad")
        e1.record()
    return dict(real=g_real, comp=g_comp, diag_add=g_diag, events=[(e0, e1)])


def _solve_columns(engine, Jr, Jc, real, comp, diag_add, AT, rows, cap_bytes):
    """X = Sigma^-1 A, the columns as rows: (B, R, N) on the device from ``AT`` (1 or B, R, N).  ``rows``: real rows per
    problem of a ragged batch -- each problem is then solved on its own over its real rows (the rest stays zero)."""
    import torch
    from .predict import rhs_workspace_plan, solve_batch_rhs
    if rows is None:
        res = solve_batch_rhs(engine, Jr, Jc, real, comp, diag_add, AT, cap_bytes, want_alpha=True, want_mu=False)
        return res["alpha"], res["events"]
    B, N, R, W = engine.B, engine.N, int(AT.shape[1]), Jr + 2 * Jc
    per = max(rhs_workspace_plan(int(n), W, 1, R, cap_bytes, 0)[0] for n in np.unique(rows))
    f64 = dict(dtype=torch.float64, device=engine.device)
    with torch.cuda.device(engine.device):
        ybs = 0 if AT.shape[0] == 1 else R * N
        rc = GroupedCall(engine, "gf_solve_batch_rhs", (per, 1, B), (real, comp, diag_add))
        X = torch.zeros((B, R, N), **f64)
        ll = torch.empty((B, R), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device=engine.device)
        events = rc.run(lambda g: g.launch(
            g.nb, int(rows[g.b0]), R, Jr, Jc, *g.coef[0], *g.data[:4], g.at(AT, ybs), ybs, N, 0, *g.work,
            g.at(X, R * N), None, R * N, N, g.at(ll, R), g.at(info), g.stream))
    return X, events


def linear_gradients(engine, Jr, Jc, real, comp, diag_add, A, fit, rows=None, marginal=False,
                     grad_cap_bytes=_lib.GF_GRAD_WORKSPACE_BYTES, solve_cap_bytes=DEFAULT_WORKSPACE_BYTES):
    """The coefficient adjoints of the profile (or, ``marginal``, the marginal) log-likelihood of B linear mean models
    at their fits.  ``A``: the design matrices on the device, (1 or B, N, R) as
    :func:`linear_gram` took them; ``fit``: the :class:`LinearFit` of the same coefficients; ``rows``: real rows per
    problem of a ragged batch.

    beta-hat maximises the likelihood, so the profile gradient is gf_loglike_grad's at the fixed residual
    r = y - A beta-hat; the marginal one adds +1/2 sum_k c_k^T (d Sigma / d theta) c_k with C = Sigma^-1 A F,
    F F^T = (A^T Sigma^-1 A)^-1 (``gf_solve_batch_rhs``, one batched product, ``gf_quadform_grad``).  Returns a dict of
    numpy arrays -- ``real`` (2, B, Jr), ``comp`` (4, B, Jc), ``diag_add`` (B,), NaN for the problems with
    ``fit.ok`` False, whose neighbours are unaffected --, ``stage_events``, name -> pairs of HIP events (``grad_ms``:
    the summed device time of the gf_loglike_grad launches), and ``grad_plan``, (workspace bytes of a group, groups,
    problems per group) of those launches."""
    import torch
    from .grad import coefficient_gradients
    B, N = engine.B, engine.N
    R = int(A.shape[2])
    ok = np.asarray(fit.ok, dtype=bool)
    dev = engine.device
    f64 = dict(dtype=torch.float64, device=dev)
    stages = {}
    with torch.cuda.device(dev):
        beta = torch.as_tensor(np.where(ok[:, None], fit.beta, 0.0), **f64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        # column by column, elementwise: one order of operations per element whatever B, N and R (a library product
        # may sum in another order for another shape), and a padded column (zeros, beta = 0) changes no bit
        resid = engine.y.expand(B, N).clone()
        for i in range(R):
            resid.addcmul_(A[:, :, i], beta[:, i:i + 1], value=-1.0)
        e1.record()
        stages["residual"] = [(e0, e1)]
    g = coefficient_gradients(engine, Jr, Jc, real, comp, diag_add, grad_cap_bytes, y=resid, rows=rows)
    stages["grad_ms"] = g["device_ms"]
    g_real, g_comp, g_diag = g["real"].copy(), g["comp"].copy(), g["diag_add"].copy()
    if marginal:
        with torch.cuda.device(dev):
            AT = A.transpose(1, 2).contiguous()
            X, stages["solve"] = _solve_columns(engine, Jr, Jc, real, comp, diag_add, AT, rows, solve_cap_bytes)
            F = torch.as_tensor(np.where(ok[:, None, None], fit.factor, 0.0), **f64)
            C = torch.empty((B, R, N), **f64)
            stream = torch.cuda.current_stream(dev).cuda_stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for b0 in range(0, B, 32768):                   # C_b = F_b^T X_b (gf_bgemm: at most 65535 per launch)
                nb = min(32768, B - b0)
                _lib.check(engine.lib.gf_bgemm(nb, 1, 0, R, N, R, F[b0].data_ptr(), R, R * R, X[b0].data_ptr(), N,
                                               R * N, None, 0, 0, C[b0].data_ptr(), N, R * N, stream), "gf_bgemm")
            e1.record()
            stages["product"] = [(e0, e1)]
            half = torch.full((R,), 0.5, **f64)
            q = quadform_gradients(engine, Jr, Jc, real, comp, C, half, rows)
            stages["quadform"] = q["events"]
            g_real = g_real + q["real"].cpu().numpy()[:, :, :Jr]
            g_comp = g_comp + q["comp"].cpu().numpy()[:, :, :Jc]
            g_diag = g_diag + q["diag_add"].cpu().numpy()
    bad = ~ok
    g_real[:, bad], g_comp[:, bad], g_diag[bad] = np.nan, np.nan, np.nan
    return dict(real=g_real, comp=g_comp, diag_add=g_diag, stage_events=stages,
                grad_plan=(g["workspace_bytes"], g["groups"], g["group_size"]))
