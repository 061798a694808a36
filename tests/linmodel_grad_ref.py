"""References of the linear-mean-model gradients, host only.

* :func:`dense_linear_loglike`: the independent reference -- dense Sigma = coefficient-form kernel of
  sho_coefficient_pack_torch + diag + diag_add, Cholesky, the generalised least squares fit and the profile or the
  marginal log-likelihood, all in torch float64 on the CPU, so that autograd differentiates THROUGH beta-hat and
  log det (A^T Sigma^-1 A) with respect to S0, w0, Q.
* :func:`composed_gradients`: the composition the device runs, restated on the host references of its pieces:
  tests/grad_ref.batch_grad at the fixed residual, tests/quadform_ref.recurrences over C = Sigma^-1 A F with weight
  1/2, gadfly_amd.grad.parameter_vjp.
* :func:`problem`: the problems both tests share."""
import functools

import numpy as np
import torch

from gadfly_amd.batch import sho_coefficient_pack
from gadfly_amd.grad import parameter_vjp, sho_coefficient_pack_torch
from oracle import dense
from tests import grad_ref
from tests import quadform_ref as qr

DT = 60.0 / 1e6                      # one-minute cadence (units of 1e6 s: frequencies in uHz)
DELTA = 60.0 / 1e6


@functools.lru_cache(maxsize=None)
def problem(B=3, J=10, n_over=2, N=300, R=8, seed=0):
    """B problems of J SHO terms (the first ``n_over`` overdamped) on one axis of N rows in three gapped segments,
    with a design matrix of R columns: a per-segment line (6 columns) and slow global waves behind them, scaled to the
    data.  dict: S0, w0, Q (B, J), t (N,), y (B, N), diag (N,), A (N, R), breaks."""
    rng = np.random.default_rng([71, B, J, N, R, seed])
    S0 = rng.uniform(0.5, 3.0, (B, J))
    w0 = rng.uniform(50.0, 1500.0, (B, J))
    Q = rng.uniform(0.7, 20.0, (B, J))
    Q[:, :n_over] = rng.uniform(0.15, 0.45, (B, n_over))
    t = np.arange(N) * DT
    breaks = (0, N // 3, 2 * N // 3, N)
    t[breaks[1]:] += 50 * DT
    t[breaks[2]:] += 9 * DT
    cols = []
    for s in range(3):
        a, b = breaks[s], breaks[s + 1]
        x = np.zeros(N)
        x[a:b] = np.linspace(-1.0, 1.0, b - a) if b - a > 1 else 0.0
        one = np.zeros(N)
        one[a:b] = 1.0
        cols += [one, x]
    u = (t - t[0]) / max(t[-1] - t[0], DT)
    k = 1
    while len(cols) < R:
        cols.append(np.sin(np.pi * k * u) if len(cols) % 2 == 0 else np.cos(np.pi * k * u))
        k += len(cols) % 2
    A = np.stack(cols[:R], axis=1)
    diag = 300.0 + rng.uniform(0.0, 30.0, N)
    y = rng.normal(size=(B, N)) * 20.0 + (A @ rng.normal(size=(R, B)) * 30.0).T
    return dict(S0=S0, w0=w0, Q=Q, t=t, y=y, diag=diag, A=A, breaks=breaks, B=B, J=J, N=N, R=R)


def dense_linear_loglike(S0, w0, Q, delta, t, y, diag, A, marginal):
    """(B,) profile (``marginal``: marginal) log-likelihoods of y_b = A_b beta + eps under the dense matrix of the
    torch coefficient pack: torch float64 CPU tensors; t (N,), diag (N,) shared, y (B, N), A (N, R) or (B, N, R).
    Differentiable in S0, w0, Q."""
    Jr, Jc, real, comp, diag_add = sho_coefficient_pack_torch(S0, w0, Q, delta)
    t, y, diag, A = (torch.as_tensor(x, dtype=torch.float64) for x in (t, y, diag, A))
    at = (t[:, None] - t[None, :]).abs()
    B, N = real.shape[1], len(t)
    eye = torch.eye(N, dtype=torch.float64)
    out = []
    for b in range(B):
        K = torch.zeros((N, N), dtype=torch.float64)
        for j in range(Jr):
            K = K + real[0, b, j] * torch.exp(-real[1, b, j] * at)
        for k in range(Jc):
            a, bb, cc, dd = comp[0, b, k], comp[1, b, k], comp[2, b, k], comp[3, b, k]
            K = K + torch.exp(-cc * at) * (a * torch.cos(dd * at) + bb * torch.sin(dd * at))
        K = K * (1.0 - eye) + torch.diag(diag + diag_add[b])
        Ab = A if A.ndim == 2 else A[b]
        L = torch.linalg.cholesky(K)
        Z = torch.linalg.solve_triangular(L, torch.cat([Ab, y[b][:, None]], dim=1), upper=False)
        Za, zy = Z[:, :-1], Z[:, -1]
        M = Za.T @ Za
        Lm = torch.linalg.cholesky(M)
        h = torch.linalg.solve_triangular(Lm, (Za.T @ zy)[:, None], upper=False)[:, 0]
        chi2 = zy @ zy - h @ h
        ll = -0.5 * chi2 - torch.sum(torch.log(torch.diagonal(L))) - 0.5 * N * np.log(2.0 * np.pi)
        if marginal:
            ll = ll - torch.sum(torch.log(torch.diagonal(Lm))) + 0.5 * Ab.shape[1] * np.log(2.0 * np.pi)
        out.append(ll)
    return torch.stack(out)


def dense_reference(prob, marginal, A=None):
    """(ll (B,), dict S0, w0, Q -> (B, J)) of a :func:`problem` by autograd through :func:`dense_linear_loglike`."""
    xs = [torch.tensor(prob[k], requires_grad=True) for k in ("S0", "w0", "Q")]
    ll = dense_linear_loglike(*xs, DELTA, prob["t"], prob["y"], prob["diag"], prob["A"] if A is None else A,
                              marginal)
    g = torch.autograd.grad(ll.sum(), xs)
    return ll.detach().numpy(), {k: v.numpy() for k, v in zip(("S0", "w0", "Q"), g)}


def composed_gradients(prob, marginal):
    """(ll (B,), dict S0, w0, Q -> (B, J)): the steps of BatchedLogLikelihood.linear_value_and_grad on the host
    references of its device pieces (dense solves stand in for the sweeps)."""
    B, N, R = prob["B"], prob["N"], prob["R"]
    t, A, diag = prob["t"], prob["A"], prob["diag"]
    Jr, Jc, real, comp, diag_add, _ = sho_coefficient_pack(prob["S0"], prob["w0"], prob["Q"], DELTA)
    resid = np.empty((B, N))
    C = np.empty((B, R, N))
    ll = np.empty(B)
    for b in range(B):
        co = (real[0, b, :Jr], real[1, b, :Jr]) + tuple(comp[i, b, :Jc] for i in range(4))
        K = dense.dense_K(co, t, 0.0)
        K[np.diag_indices(N)] = diag + diag_add[b]
        X = np.linalg.solve(K, A)                           # Sigma^-1 A
        M = A.T @ X
        beta = np.linalg.solve(M, X.T @ prob["y"][b])
        resid[b] = prob["y"][b] - A @ beta
        F = np.linalg.cholesky(np.linalg.inv(M))            # F F^T = M^-1
        C[b] = (X @ F).T
        sign, ldet = np.linalg.slogdet(K)
        ll[b] = -0.5 * (resid[b] @ np.linalg.solve(K, resid[b]) + ldet + N * np.log(2.0 * np.pi))
        if marginal:
            ll[b] += -0.5 * np.linalg.slogdet(M)[1] + 0.5 * R * np.log(2.0 * np.pi)
    _, g = grad_ref.batch_grad(np.broadcast_to(t, (B, N)), resid, np.broadcast_to(diag, (B, N)), Jr, Jc, real, comp,
                               diag_add)
    g_real, g_comp, g_diag = g["real"].copy(), g["comp"].copy(), g["diag_add"].copy()
    if marginal:
        for b in range(B):
            co = (real[0, b, :Jr], real[1, b, :Jr]) + tuple(comp[i, b, :Jc] for i in range(4))
            qr_, qc_, qd = qr.stacked(qr.weighted(qr.recurrences(t, co, C[b]), R, np.full(R, 0.5)), Jr, Jc)
            g_real[:, b] += qr_
            g_comp[:, b] += qc_
            g_diag[b] += qd
    gS0, gw0, gQ = parameter_vjp(prob["S0"], prob["w0"], prob["Q"], DELTA, g_real, g_comp, g_diag)
    return ll, dict(S0=gS0, w0=gw0, Q=gQ)


def scaled_error(theta, got, ref):
    """max |theta g - theta g_ref| / max(1, max |theta g_ref|): tests/test_gpu_grad.py's measure."""
    a, r = theta * got, theta * ref
    return float(np.max(np.abs(a - r)) / max(1.0, float(np.max(np.abs(r)))))


# ---- raw coefficient problems (odd widths cannot be had from SHO terms) ----------------------------------------------

def dense_coefficient_linear_grad(prob, b, A, marginal):
    """(ll, dict of the six coefficient adjoints + diag_add) of problem b of a tests/grad_cases.edge_problem under
    the linear mean A (N, R), by autograd through the dense generalised least squares likelihood."""
    from tests import grad_cases as gc
    f64 = torch.float64
    co = [torch.tensor(x, requires_grad=True) for x in gc.coefficients(prob, b)]
    shift = torch.zeros((), dtype=f64, requires_grad=True)
    t, y, diag, A = (torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in (prob["t"], prob["y"][b],
                                                                                prob["diag"][b], A))
    ar, cr, ac, bc, cc, dc = co
    at = (t[:, None] - t[None, :]).abs()
    N = len(t)
    K = torch.zeros((N, N), dtype=f64)
    for j in range(prob["Jr"]):
        K = K + ar[j] * torch.exp(-cr[j] * at)
    for k in range(prob["Jc"]):
        K = K + torch.exp(-cc[k] * at) * (ac[k] * torch.cos(dc[k] * at) + bc[k] * torch.sin(dc[k] * at))
    K = K * (1.0 - torch.eye(N, dtype=f64)) + torch.diag(diag + float(prob["diag_add"][b]) + shift)
    L = torch.linalg.cholesky(K)
    Z = torch.linalg.solve_triangular(L, torch.cat([A, y[:, None]], dim=1), upper=False)
    Za, zy = Z[:, :-1], Z[:, -1]
    Lm = torch.linalg.cholesky(Za.T @ Za)
    h = torch.linalg.solve_triangular(Lm, (Za.T @ zy)[:, None], upper=False)[:, 0]
    ll = -0.5 * (zy @ zy - h @ h) - torch.sum(torch.log(torch.diagonal(L))) - 0.5 * N * np.log(2.0 * np.pi)
    if marginal:
        ll = ll - torch.sum(torch.log(torch.diagonal(Lm))) + 0.5 * A.shape[1] * np.log(2.0 * np.pi)
    gr = torch.autograd.grad(ll, co + [shift], allow_unused=True)
    g = {k: (np.zeros(len(c)) if v is None else v.numpy()) for k, c, v in zip(gc.NAMES, co, gr)}
    g["diag_add"] = gr[6].item()
    return ll.item(), g
