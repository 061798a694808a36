"""
Test oracles of the log-likelihood gradient; in tests/ because oracle/ is frozen.

* :func:`loglike_grad` -- a numpy restatement of the reverse pass the device runs: the plain celerite recurrence
  of oracle/celerite_ref.c forward (every row's S kept), explicit adjoints backward, O(N W^2), vectorised per row.
  With ``dtype=np.longdouble`` the same pass in 80-bit on the float64 phases theta = fl(d t): the reference of the
  randomized device tests.
* :func:`dense_loglike` -- the independent reference: K built densely from the torch coefficient pack, Cholesky,
  log L, all in torch float64 on the CPU, so autograd differentiates it with respect to S0, w0, Q.
* :func:`dense_coefficient_loglike` -- the same dense log L straight from raw coefficient tensors of any structure
  (odd Jr included), differentiable in every coefficient, a constant mean and a constant on the diagonal.  It sees
  time differences only: the translation-invariant reference.
"""
import numpy as np
import torch

from gadfly_amd.grad import sho_coefficient_pack_torch


def rows(t, Jr, Jc, ar, cr, ac, bc, cc, dc, dtype=np.float64):
    """c (W,), U, V (N, W), cos, sin (N, Jc) of one problem (ref_get_matrices).  The phases are theta = fl(d t), ONE
    float64 multiply, whatever ``dtype``: cos / sin of them and everything after run in ``dtype`` (as
    random_cases.loglike80: an 80-bit product would be another matrix on a far axis, not a better value of this one)."""
    th = (np.asarray(dc, dtype=np.float64)[None, :] * np.asarray(t, dtype=np.float64)[:, None]).astype(dtype)
    co, si = np.cos(th), np.sin(th)
    N, W = len(t), Jr + 2 * Jc
    U, V = np.empty((N, W), dtype=dtype), np.empty((N, W), dtype=dtype)
    U[:, :Jr], V[:, :Jr] = ar[None, :], 1.0
    U[:, Jr::2], U[:, Jr + 1::2] = ac * co + bc * si, ac * si - bc * co
    V[:, Jr::2], V[:, Jr + 1::2] = co, si
    c = np.empty(W, dtype=dtype)
    c[:Jr], c[Jr::2], c[Jr + 1::2] = cr, cc, cc
    return c, U, V, co, si


def loglike_grad(t, y, diag, Jr, Jc, ar, cr, ac, bc, cc, dc, diag_add, dtype=np.float64):
    """log L and its gradient for one problem: dict with ar, cr, ac, bc, cc, dc, diag_add, mean
    (y holds the data minus the mean; phase_rows (N, Jc) are the rows' phase adjoints that dc sums).  Returns
    (ll, None) when a pivot is not positive.  ``dtype``: np.float64, or np.longdouble for the 80-bit pass on the
    float64 phases (:func:`rows`)."""
    t64 = np.asarray(t, dtype=np.float64)
    t, y, diag = (np.asarray(x, dtype=np.float64).astype(dtype) for x in (t, y, diag))
    ar, cr, ac, bc, cc, dc = (np.asarray(x, dtype=np.float64)[:n].astype(dtype) for x, n in
                              zip((ar, cr, ac, bc, cc, dc), (Jr, Jr, Jc, Jc, Jc, Jc)))
    N = len(t)
    c, U, V, co, si = rows(t64, Jr, Jc, ar, cr, ac, bc, cc, dc, dtype)
    W = len(c)
    A = diag + dtype(diag_add)
    dtn = np.concatenate([np.zeros(1, dtype=dtype), t[:-1] - t[1:]])
    P = np.exp(c[None, :] * dtn[:, None])
    S = np.zeros((N, W, W), dtype=dtype)
    Wm, G, f = np.zeros((N, W), dtype=dtype), np.zeros((N, W), dtype=dtype), np.zeros((N, W), dtype=dtype)
    D, z = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    Sp, Gp, wp = np.zeros((W, W), dtype=dtype), np.zeros(W, dtype=dtype), np.zeros(W, dtype=dtype)
    Dp, zp = dtype(0.0), dtype(0.0)
    for n in range(N):
        p = P[n]
        Sn = p[:, None] * p[None, :] * (Sp + Dp * np.outer(wp, wp))
        fn = Sn @ U[n]
        Dn = A[n] - U[n] @ fn
        if not Dn > 0.0:
            return -np.inf, None
        Gn = p * (Gp + wp * zp)
        zn = y[n] - U[n] @ Gn
        wn = (V[n] - fn) / Dn
        S[n], f[n], D[n], G[n], z[n], Wm[n] = Sn, fn, Dn, Gn, zn, wn
        Sp, Gp, wp, Dp, zp = Sn, Gn, wn, Dn, zn
    ll = -0.5 * (np.sum(z * z / D) + np.sum(np.log(D)) + N * np.log(2.0 * dtype(np.pi)))
    Mb, Hb = np.zeros((W, W), dtype=dtype), np.zeros(W, dtype=dtype)
    Ub, Vb, cb = np.zeros((N, W), dtype=dtype), np.zeros((N, W), dtype=dtype), np.zeros(W, dtype=dtype)
    Ab, yb = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    for n in range(N - 1, -1, -1):
        wn, Dn, zn, Gn, un, fn, p = Wm[n], D[n], z[n], G[n], U[n], f[n], P[n]
        q = Mb @ wn
        Db = wn @ q
        Wb = 2.0 * Dn * q + Hb * zn
        zb = wn @ Hb
        Gb = Hb.copy()
        zb -= zn / Dn
        Db += 0.5 * (zn / Dn) ** 2 - 0.5 / Dn
        ub = -zb * Gn
        Gb -= zb * un
        vb = Wb / Dn
        fb = -Wb / Dn
        Db -= (Wb @ wn) / Dn
        ub -= Db * fn
        fb -= Db * un
        ub += S[n] @ fb
        Sb = Mb + 0.5 * (np.outer(fb, un) + np.outer(un, fb))
        cb += dtn[n] * (2.0 * np.sum(Sb * S[n], axis=1) + Gb * Gn)
        Mb = p[:, None] * p[None, :] * Sb
        Hb = p * Gb
        Ub[n], Vb[n], Ab[n], yb[n] = ub, vb, Db, zb
    g = dict(ar=np.sum(Ub[:, :Jr], axis=0), cr=cb[:Jr])
    U0b, U1b, V0b, V1b = Ub[:, Jr::2], Ub[:, Jr + 1::2], Vb[:, Jr::2], Vb[:, Jr + 1::2]
    U0, U1 = U[:, Jr::2], U[:, Jr + 1::2]
    g["ac"] = np.sum(U0b * co + U1b * si, axis=0)
    g["bc"] = np.sum(U0b * si - U1b * co, axis=0)
    g["cc"] = cb[Jr::2] + cb[Jr + 1::2]
    th = -U0b * U1 + U1b * U0 - V0b * si + V1b * co
    # d theta_n / d d = t_n, summed as (t_n - t_0): rotating every phase of a term by one angle leaves K unchanged,
    # so sum_n th_n = 0 analytically -- in floating point it is rounding residue, which t_0 = 2e5 would multiply
    g["dc"] = np.sum((t - t[0])[:, None] * th, axis=0)
    g["phase_rows"] = th                       # (N, Jc) adjoints of theta_n, for other associations of the sum
    g["diag_add"] = np.sum(Ab)
    g["mean"] = -np.sum(yb)
    return ll, g


def batch_grad(t, y, diag, Jr, Jc, real, comp, diag_add, dtype=np.float64):
    """:func:`loglike_grad` over a batch in the engine's stacked layout (t, y, diag (B, N)): (ll (B,), dict with
    real (2, B, Jr), comp (4, B, Jc), diag_add (B,), mean (B,)), float64 whatever ``dtype`` the pass ran in."""
    B = real.shape[1]
    ll = np.empty(B)
    out = dict(real=np.full((2, B, Jr), np.nan), comp=np.full((4, B, Jc), np.nan),
               diag_add=np.full(B, np.nan), mean=np.full(B, np.nan))
    for b in range(B):
        ll[b], g = loglike_grad(t[b], y[b], diag[b], Jr, Jc, real[0, b], real[1, b], comp[0, b], comp[1, b],
                                comp[2, b], comp[3, b], diag_add[b], dtype)
        if g is None:
            continue
        out["real"][0, b], out["real"][1, b] = g["ar"], g["cr"]
        for i, k in enumerate(("ac", "bc", "cc", "dc")):
            out["comp"][i, b] = g[k]
        out["diag_add"][b], out["mean"][b] = g["diag_add"], g["mean"]
    return ll, out


def dense_loglike(S0, w0, Q, delta, t, y, diag):
    """(B,) log-likelihoods of dense K = celerite kernel of the torch pack + diag (torch float64 CPU tensors,
    t, y, diag (N,) shared), differentiable in S0, w0, Q."""
    Jr, Jc, real, comp, diag_add = sho_coefficient_pack_torch(S0, w0, Q, delta)
    t = torch.as_tensor(t, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64)
    diag = torch.as_tensor(diag, dtype=torch.float64)
    tau = t[:, None] - t[None, :]
    at = tau.abs()
    sgn = torch.sign(tau)
    B, N = real.shape[1], len(t)
    eye = torch.eye(N, dtype=torch.float64)
    out = []
    for b in range(B):
        K = torch.zeros((N, N), dtype=torch.float64)
        for j in range(Jr):
            K = K + real[0, b, j] * torch.exp(-real[1, b, j] * at)
        for k in range(Jc):
            a, bb, cc, dd = comp[0, b, k], comp[1, b, k], comp[2, b, k], comp[3, b, k]
            K = K + torch.exp(-cc * at) * (a * torch.cos(dd * tau) + bb * sgn * torch.sin(dd * tau))
        K = K * (1.0 - eye) + torch.diag(diag + diag_add[b])
        L = torch.linalg.cholesky(K)
        alpha = torch.cholesky_solve(y[:, None], L)[:, 0]
        out.append(-0.5 * (y @ alpha) - torch.sum(torch.log(torch.diagonal(L))) - 0.5 * N * np.log(2.0 * np.pi))
    return torch.stack(out)


def dense_coefficient_loglike(t, y, diag, Jr, Jc, ar, cr, ac, bc, cc, dc, diag_add, mean=0, shift=0):
    """log L of ONE problem from raw coefficient tensors (torch float64, CPU; any Jr, Jc): dense K from the lags
    tau = t_i - t_j, diagonal diag + diag_add + shift (the recurrence's A_n, not K(0)), data y - mean, Cholesky.
    Differentiable in ar, cr, ac, bc, cc, dc, diag_add, mean and shift."""
    f64 = torch.float64
    t, y, diag = (torch.as_tensor(np.asarray(x, dtype=np.float64)) if not torch.is_tensor(x) else x.to(f64)
                  for x in (t, y, diag))
    ar, cr, ac, bc, cc, dc = (torch.as_tensor(x, dtype=f64)[:n] for x, n in
                              zip((ar, cr, ac, bc, cc, dc), (Jr, Jr, Jc, Jc, Jc, Jc)))
    tau = t[:, None] - t[None, :]
    at = tau.abs()
    N = len(t)
    K = torch.zeros((N, N), dtype=f64)
    for j in range(Jr):
        K = K + ar[j] * torch.exp(-cr[j] * at)
    for k in range(Jc):
        K = K + torch.exp(-cc[k] * at) * (ac[k] * torch.cos(dc[k] * tau) + bc[k] * torch.sin(dc[k] * at))
    K = K * (1.0 - torch.eye(N, dtype=f64)) + torch.diag(diag + diag_add + shift)
    r = y - mean
    L = torch.linalg.cholesky(K)
    alpha = torch.cholesky_solve(r[:, None], L)[:, 0]
    return -0.5 * (r @ alpha) - torch.sum(torch.log(torch.diagonal(L))) - 0.5 * N * np.log(2.0 * np.pi)
