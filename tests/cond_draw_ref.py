"""
Test reference of the conditional draws: a numpy restatement of Matheron's rule with DENSE matrices
-- oracle/dense.py's kernel matrices, ``numpy.linalg.cholesky`` of the noise-free union-axis matrix K_u (= L_u D_u^{1/2}
by uniqueness of the Cholesky factor) and a dense solve on the observed axis -- plus the problems and query designs the
host and GPU tests share.  Nothing here shares code with the semiseparable recurrences.
"""
import functools

import numpy as np
import scipy.linalg as sla

from gadfly_amd.conddraw import _PackKernel, union_axes
from oracle import dense
from tests import grad_cases as gc

#: (N, M) of the linear-map identity and the three term structures it runs at (W = 6, 20, 60: one per kernel instance)
SHAPES = ((1, 1), (5, 0), (12, 9), (40, 17))
STRUCTURES = ((0, 3), (0, 10), (0, 30))
#: grad_cases' one-minute axis stretched to a cadence of 1.2e-3: w0 dt = 0.06 .. 1.8 for its SHO terms (w0 = 50 ..
#: 1500), oscillations that the cadence resolves without oversampling them a hundredfold (where the NOISE-FREE
#: union-axis matrix of any smooth kernel is singular to working precision and no factor of it, dense or
#: semiseparable, means much)
STRETCH = 20.0


def queries(t, M, seed=0):
    """M ascending queries on the axis t: before t_0, behind the last stamp, coincident with stamps, and -- from M = 5
    on -- inside the largest gap; the rest anywhere between 10 % before and 10 % behind the data."""
    if M == 0:
        return np.zeros(0)
    rng = np.random.default_rng([19, len(t), M, seed])
    span = max(t[-1] - t[0], gc.DT * STRETCH)
    q = list(rng.uniform(t[0] - 0.1 * span, t[-1] + 0.1 * span, M))
    q[0] = t[0] - 0.05 * span
    if M >= 2:
        q[1] = t[-1] + 0.05 * span
    if M >= 3:
        q[2] = t[len(t) // 3]
    if M >= 5 and len(t) > 1:
        k = int(np.argmax(np.diff(t)))
        q[3], q[4] = t[k] + 0.3 * (t[k + 1] - t[k]), t[k] + 0.7 * (t[k + 1] - t[k])
    if M >= 6:
        q[5] = t[-1]
    return np.sort(np.array(q))


@functools.lru_cache(maxsize=None)
def problem(Jr, Jc, N, M, seed=0):
    """grad_cases.edge_problem (B = 3 kernels, per-row diagonals, a gapped jittered axis) with per-problem data means
    and M queries per problem.  Raw coefficients: diag_add = k(0), no exposure shift."""
    prob = dict(gc.edge_problem(Jr, Jc, N, seed=seed))
    prob["t"] = prob["t"] * STRETCH
    prob["mean"] = np.array([0.0, 3.5, -120.0])
    prob["y"] = prob["y"] + prob["mean"][:, None]
    prob["ts"] = np.stack([queries(prob["t"], M, seed=b) for b in range(prob["B"])])
    prob["M"] = M
    return prob


def kernels(prob):
    """Objects with ``get_device_coefficients`` for the B problems (what the batch classes take as kernels)."""
    return [_PackKernel(prob["Jr"], prob["Jc"], prob["real"], prob["comp"], prob["diag_add"], b)
            for b in range(prob["B"])]


def kernel_matrix(co, x1, x2):
    """oracle/dense.py's ``kernel_value(co, x1[:, None] - x2[None, :])`` term by term in torch float64 (on the GPU where
    there is one): the same formula without the (n1, n2, J) temporary, for the one test whose matrices have 1e7
    entries (compared with dense.kernel_value in tests/test_cond_draw_host.py).  Eager tensor arithmetic only: nothing
    of the package under test."""
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    ar, cr, ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in co)
    tau = torch.abs(torch.as_tensor(np.asarray(x1, dtype=np.float64), device=dev)[:, None]
                    - torch.as_tensor(np.asarray(x2, dtype=np.float64), device=dev)[None, :])
    k = torch.zeros_like(tau)
    for a, c in zip(ar, cr):
        k += float(a) * torch.exp(-float(c) * tau)
    for a, b, c, d in zip(ac, bc, cc, dc):
        k += (float(a) * torch.cos(float(d) * tau) + float(b) * torch.sin(float(d) * tau)) * torch.exp(-float(c) * tau)
    return k.cpu().numpy()


def draw(co, shift, t, dg, y, mean, ts, eps, eta):
    """Steps 1-6 for one problem with dense matrices.  ``co`` = (ar, cr, ac, bc, cc, dc); ``shift`` = diag_add - k(0);
    ``ts`` None: draws at the observed stamps.  ``eps`` (R, Nu), ``eta`` (R, N) -> z (R, M or N).  Beyond 512 union
    rows the kernel matrix is made once on the union axis (:func:`kernel_matrix`) and Sigma and K* are cut from it."""
    ax = union_axes(t, ts)
    u, orow, qrow = ax.u[0], ax.obs_rows[0], ax.query_rows[0]
    eps, eta = np.atleast_2d(eps), np.atleast_2d(eta)
    if len(u) <= 512:
        Ku = dense.dense_K(co, u, shift)
        Sigma = dense.dense_K(co, t, dg + shift)
        Ks = None if ts is None else dense.kernel_value(co, np.asarray(ts)[:, None] - np.asarray(t)[None, :])
    else:
        Kuu = kernel_matrix(co, u, u)
        Sigma = Kuu[np.ix_(orow, orow)]
        Sigma[np.diag_indices_from(Sigma)] += dg + shift
        Ks = None if ts is None else Kuu[np.ix_(qrow, orow)]
        Ku = Kuu
        Ku[np.diag_indices_from(Ku)] += shift
    L = np.linalg.cholesky(Ku)
    w = eps @ L.T                                              # (R, Nu)
    r = (y - mean)[None, :] - (w[:, orow] + np.sqrt(dg)[None, :] * eta)
    alpha = sla.cho_solve(sla.cho_factor(Sigma, lower=True), r.T).T
    if ts is None:
        return w[:, orow] + (r - dg[None, :] * alpha) + mean
    return w[:, qrow] + alpha @ Ks.T + mean


def linear_map(co, shift, t, dg, y, mean, ts):
    """(A, c) of z = c + A [eps; eta]: the Nu + N unit normal vectors and the zero vector through :func:`draw`."""
    nu, n = int(union_axes(t, ts).nu[0]), len(t)
    eye = np.eye(nu + n)
    z = draw(co, shift, t, dg, y, mean, ts, np.vstack([eye[:, :nu], np.zeros((1, nu))]),
             np.vstack([eye[:, nu:], np.zeros((1, n))]))
    c = z[-1]
    return (z[:-1] - c[None, :]).T, c


def dense_posterior(co, shift, t, dg, y, mean, ts):
    """(mean, covariance) of the noise-free process given y from the dense oracle: at ts, or at t itself."""
    Sigma = dense.dense_K(co, t, dg + shift)
    cf = sla.cho_factor(Sigma, lower=True)
    if ts is None:
        K0 = dense.dense_K(co, t, shift)
        return K0 @ sla.cho_solve(cf, y - mean) + mean, K0 - K0 @ sla.cho_solve(cf, K0)
    Ks = dense.kernel_value(co, np.asarray(ts)[:, None] - np.asarray(t)[None, :])
    Kss = dense.dense_K(co, ts, shift)
    return Ks @ sla.cho_solve(cf, y - mean) + mean, Kss - Ks @ sla.cho_solve(cf, Ks.T)


@functools.lru_cache(maxsize=None)
def yardstick():
    """The restatement's own worst float64 disagreement with the dense oracle over SHAPES x STRUCTURES, at new times
    and at the observed stamps, in units of K(0): (of the offset c against the conditional mean, relative to max
    |mean|; of A A^T against the conditional covariance)."""
    worst_c = worst_cov = 0.0
    for Jr, Jc in STRUCTURES:
        for N, M in SHAPES:
            prob = problem(Jr, Jc, N, M)
            co, k0 = gc.coefficients(prob, 0), prob["diag_add"][0]
            args = (co, 0.0, prob["t"], prob["diag"][0], prob["y"][0], prob["mean"][0])
            for ts in ((prob["ts"][0], None) if M else (None,)):
                A, c = linear_map(*args, ts)
                mu, cov = dense_posterior(*args, ts)
                worst_c = max(worst_c, float(np.max(np.abs(c - mu)) / np.max(np.abs(mu))))
                worst_cov = max(worst_cov, float(np.max(np.abs(A @ A.T - cov)) / k0))
    return worst_c, worst_cov
