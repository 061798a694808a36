"""References of the linear-mean-model calls, host only: numpy and the oracle, no device import.

Two independent statements of [A | y]^T Sigma^-1 [A | y] and log det Sigma:
  * :func:`dense_gram`: oracle/dense.py's K, a Cholesky solve, the products;
  * :func:`forward_gram`: the forward-sweep route the device takes, restated on oracle/seq.py (factor, solve_lower,
    Z^T D^-1 Z), in float64 or 80-bit.  An 80-bit run takes the float64 run's generator rows (phases theta_n =
    fl(d t_n) rounded in float64, as celerite2 and the device do) and carries everything behind them in 80 bits.
and the generalised least squares quantities from a Gram matrix in plain numpy (:func:`gls_from_gram`), which shares
no code with gadfly_amd.linmodel.solve_normal_equations."""
import functools

import numpy as np

from oracle import dense, seq
from tests import grad_cases as gc


def matrices(t, co, dtype=np.float64):
    """(c, U, V) with float64 generator rows, cast to ``dtype``."""
    c, _, U, V = seq.celerite_matrices(co, t, 0.0, dtype=np.float64)
    return c.astype(dtype), U.astype(dtype), V.astype(dtype)


def forward_gram(t, co, a, A, y, dtype=np.float64):
    """(gram (R + 1, R + 1), logdet, info) of one problem by the forward route: ``a`` the full diagonal A_n (noise plus
    diag_add), ``A`` (N, R), ``y`` (N,).  A failed pivot gives NaN and the 1-based row."""
    t = np.asarray(t, dtype=np.float64)
    c, U, V = matrices(t, co, dtype)
    td = t.astype(dtype)
    R = A.shape[1]
    d, Wm, info = seq.factor(td, c, np.asarray(a, dtype=dtype), U, V)
    if info:
        return np.full((R + 1, R + 1), np.nan), np.nan, info
    Y = np.concatenate([A, np.asarray(y)[:, None]], axis=1).astype(dtype)
    Z = seq.solve_lower(td, c, U, Wm, Y).reshape(len(t), R + 1)
    Zs = Z / np.sqrt(d)[:, None]
    return Zs.T @ Zs, np.sum(np.log(d)), 0


def dense_gram(t, co, diag, A, y):
    """(gram, logdet) of one problem from the dense matrix: ``diag`` the noise diagonal alone (the kernel's value at
    lag zero is the amplitude the device receives as diag_add)."""
    K = dense.dense_K(co, t, diag)
    L = np.linalg.cholesky(K)
    Y = np.concatenate([A, np.asarray(y)[:, None]], axis=1)
    Z = np.linalg.solve(L, Y)
    return Z.T @ Z, 2.0 * np.sum(np.log(np.diag(L)))


def gls_from_gram(G, logdet, nrows):
    """dict(beta, cov, chi2, ll, ll_marginal, cond) of one problem from its Gram matrix, any dtype: plain inverse of
    the normal matrix."""
    G = np.asarray(G)
    R = G.shape[0] - 1
    M, g, yy = G[:R, :R], G[:R, R], G[R, R]
    if G.dtype == np.longdouble:                # (numpy's LAPACK is float64: Gauss-Jordan in 80 bits)
        cov = _inverse_ld(M)
        sign, ldn = 1.0, _logdet_ld(M)
    else:
        cov = np.linalg.inv(M)
        sign, ldn = np.linalg.slogdet(M)
    beta = cov @ g
    chi2 = yy - g @ beta
    log2pi = np.log(np.asarray(2.0 * np.pi, dtype=G.dtype))
    ll = -0.5 * (chi2 + logdet + nrows * log2pi)
    s = 1.0 / np.sqrt(np.diag(M).astype(np.float64))
    return dict(beta=beta, cov=cov, chi2=chi2, ll=ll, ll_marginal=ll - 0.5 * ldn + 0.5 * R * log2pi,
                cond=float(np.linalg.cond(M.astype(np.float64))), cond_scaled=float(np.linalg.cond(
                    M.astype(np.float64) * s[:, None] * s[None, :])), sign=sign)


def _cholesky_ld(M):
    n = M.shape[0]
    L = np.zeros_like(M)
    for j in range(n):
        L[j, j] = np.sqrt(M[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def _inverse_ld(M):
    L = _cholesky_ld(M)
    n = M.shape[0]
    Li = np.zeros_like(M)
    for j in range(n):
        Li[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) / L[i, i]
    return Li.T @ Li


def _logdet_ld(M):
    return 2 * np.sum(np.log(np.diag(_cholesky_ld(M))))


# ---- problems --------------------------------------------------------------------------------------------------------

def gaussian_basis(N, R, seed):
    return np.random.default_rng([11, N, R, seed]).normal(size=(N, R))


def legendre_basis(t, breaks, order):
    """Per-segment Legendre basis written out independently of gadfly_amd.quarter_polynomial_basis (explicit
    recurrence): (N, S (order + 1))."""
    t = np.asarray(t, dtype=np.float64)
    S, P = len(breaks) - 1, order + 1
    A = np.zeros((len(t), S * P))
    for s in range(S):
        a, b = breaks[s], breaks[s + 1]
        ts = t[a:b]
        if b - a == 1:
            A[a, s * P] = 1.0
            continue
        x = (2.0 * ts - (ts[0] + ts[-1])) / (ts[-1] - ts[0])
        p0, p1 = np.ones_like(x), x
        A[a:b, s * P] = p0
        for k in range(1, P):
            A[a:b, s * P + k] = p1
            p0, p1 = p1, ((2 * k + 1) * x * p1 - k * p0) / (k + 1)
    return A


@functools.lru_cache(maxsize=None)
def walkers(B=5, J=30, N=900, order=3, shift=0.0):
    """The walkers' problem of the tests: B solar-like SHO kernels of J terms with perturbed amplitudes over one
    one-minute axis of N rows in three gapped segments, data drawn from each kernel plus a per-segment cubic trend,
    white noise of 30 ppm.  Returns a dict: t (N,) (moved by ``shift``), breaks, A (N, 3 (order + 1)), y (B, N), yerr,
    co (B tuples of six coefficient arrays), diag_add (B,), real / comp stacked as the device takes them."""
    import gadfly_amd
    from gadfly_amd.engine import _coeff_pack
    from gadfly_amd.synth import solar_like_hyperparameters, uniform_times
    rng = np.random.default_rng([900, B, J, N])
    t0 = uniform_times(N, 60.0)
    breaks = (0, N // 3, 2 * N // 3 + 7, N)
    t0 = t0.copy()
    dt = t0[1] - t0[0]
    for s in breaks[1:-1]:
        t0[s:] += 37.0 * dt
    t = t0 + shift
    kernels, cos = [], []
    for b in range(B):
        hp = [dict(h) for h in solar_like_hyperparameters(J)]
        for h in hp:
            h["hyperparameters"] = dict(h["hyperparameters"])
            h["hyperparameters"]["S0"] = h["hyperparameters"]["S0"] * (1.0 + 0.1 * b)
        kernels.append(gadfly_amd.StellarOscillatorKernel(hp, texp=60.0))
        cos.append(kernels[-1].get_device_coefficients())
    yerr = 30.0
    A = legendre_basis(t0, breaks, order)
    Jr, Jc, real, comp, diag_add, _ = _coeff_pack(cos)
    y = np.empty((B, N))
    for b, co in enumerate(cos):
        c, U, V = matrices(t0, co[:6])
        d, Wm, info = seq.factor(t0, c, np.full(N, yerr ** 2) + diag_add[b], U, V)
        assert info == 0
        y[b] = seq.dot_tril(t0, c, U, Wm, d, rng.normal(size=N)) + A @ (200.0 * rng.normal(size=A.shape[1]))
    return dict(t=t, breaks=breaks, A=A, y=y, yerr=yerr, kernels=tuple(kernels), co=tuple(c[:6] for c in cos),
                diag_add=np.asarray(diag_add), Jr=Jr, Jc=Jc, real=real, comp=comp, B=B, N=N)


def edge(Jr, Jc, N):
    """grad_cases.edge_problem's B = 3 problems (shared axis, per-problem noise diagonals and data)."""
    return gc.edge_problem(Jr, Jc, N)


def edge_reference(prob, A, dtype=np.float64):
    """forward_gram of every problem of an edge problem against the design matrix A (N, R) or (B, N, R): (gram (B, R +
    1, R + 1), logdet (B,), info (B,))."""
    B = prob["y"].shape[0]
    out = [forward_gram(prob["t"], gc.coefficients(prob, b), prob["diag"][b] + prob["diag_add"][b],
                        A if A.ndim == 2 else A[b], prob["y"][b], dtype) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]))


def gram_error(got, ref):
    """Largest |got - ref| over sqrt(ref_ii ref_jj) of one Gram matrix (entries of zero columns compare to zero)."""
    ref = np.asarray(ref, dtype=np.float64)
    d = np.sqrt(np.abs(np.diag(ref)))
    scale = d[:, None] * d[None, :]
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(np.max(np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), err)))


# ---- the dense answer in 80 bits -------------------------------------------------------------------------------------

def dense_K_ld(cos, t, diags):
    """oracle/dense.py's dense_K in 80 bits for several kernels that share their rates (c_r, c_c, d_c) on one axis:
    every exponential, cosine and sine is made once, for the upper triangle.  ``diags``: the noise diagonal per
    kernel.  Returns a list of (N, N) longdouble matrices."""
    ld = np.longdouble
    t = np.asarray(t, dtype=np.float64).astype(ld)
    N = len(t)
    iu = np.triu_indices(N)
    tau = np.abs(t[iu[0]] - t[iu[1]])
    ref = cos[0]
    assert all(np.array_equal(co[k], ref[k]) for co in cos for k in (1, 4, 5)), "the kernels do not share their rates"
    acc = [np.zeros(len(tau), dtype=ld) for _ in cos]
    for j in range(len(ref[0])):
        e = np.exp(-ld(ref[1][j]) * tau)
        for a, co in zip(acc, cos):
            a += ld(co[0][j]) * e
    for j in range(len(ref[2])):
        e = np.exp(-ld(ref[4][j]) * tau)
        ec, es = e * np.cos(ld(ref[5][j]) * tau), e * np.sin(ld(ref[5][j]) * tau)
        for a, co in zip(acc, cos):
            a += ld(co[2][j]) * ec + ld(co[3][j]) * es
    out = []
    for a, dg in zip(acc, diags):
        K = np.zeros((N, N), dtype=ld)
        K[iu] = a
        K = K + np.triu(K, 1).T
        K[np.diag_indices(N)] += np.broadcast_to(np.asarray(dg, dtype=np.float64), (N,)).astype(ld)
        out.append(K)
    return out


def dense_gram_ld(K, A, y):
    """(gram, logdet) in 80 bits from a dense longdouble K: a right-looking Cholesky, one column at a time, the
    right-hand sides [A | y] carried along."""
    ld = np.longdouble
    N = K.shape[0]
    M = np.concatenate([K, np.concatenate([A, np.asarray(y)[:, None]], axis=1).astype(ld)], axis=1)
    logdet = ld(0)
    for j in range(N):                  # Gaussian elimination of [K | Y]: row j becomes row j of [D L^T | Z]
        piv = M[j, j]
        logdet += np.log(piv)
        if j + 1 < N:
            f = M[j + 1:, j] / piv
            M[j + 1:, j + 1:] -= f[:, None] * M[j, j + 1:][None, :]
    Z = M[:, N:]
    d = np.diagonal(M[:, :N])
    Zs = Z / np.sqrt(d)[:, None]
    return Zs.T @ Zs, logdet
