"""
Test references of the batched conditional variance; in tests/ because oracle/ is frozen.

* :func:`var_passes` -- a numpy restatement of the two passes gf_var_batch runs: the forward sweep with a checkpoint
  every ``seg`` rows and the queries staged at their owners, then the segments recomputed last first with the upper
  solve and the matrix recurrence Y over their staged rows, the queries evaluated once Y is the value of the row after
  them.  ``dtype=np.longdouble`` runs the same passes in 80-bit on the float64 phases (tests.grad_ref.rows).
* :func:`dense_reference` -- the independent reference: K densely from the raw coefficients and the lags,
  inv(K + diag), then the textbook formulas.
* :func:`loo_reference` -- leave-one-out the honest way: delete a row, predict it from the others.
* :func:`work_formula` -- gf_var_batch_work restated.
* :func:`queries` -- the query times of the edge cases: before the first row, ties, inside intervals, after the end.
"""
import numpy as np

from tests.grad_ref import rows


def kernel_value(tau, Jr, Jc, ar, cr, ac, bc, cc, dc):
    """k(tau) of the celerite form in its coefficients, elementwise."""
    at = np.abs(np.asarray(tau, dtype=np.float64))
    k = np.zeros_like(at)
    for j in range(Jr):
        k = k + ar[j] * np.exp(-cr[j] * at)
    for j in range(Jc):
        k = k + np.exp(-cc[j] * at) * (ac[j] * np.cos(dc[j] * at) + bc[j] * np.sin(dc[j] * at))
    return k


def dense_sigma(t, diag, Jr, Jc, co, diag_add):
    """(K, Sigma): K from the lags with K(0) = diag_add on its diagonal, Sigma = K + diag."""
    t = np.asarray(t, dtype=np.float64)
    K = kernel_value(t[:, None] - t[None, :], Jr, Jc, *co)
    K[np.diag_indices(len(t))] = diag_add
    return K, K + np.diag(np.asarray(diag, dtype=np.float64))


def dense_reference(t, y, diag, Jr, Jc, co, diag_add, ts=None):
    """dict(alpha, mu, hdiag, var, var_at) of one problem from the dense inverse: h = diag(Sigma^-1),
    var_n = K(0) - K_n Sigma^-1 K_n^T, var_at = K(0) - K(t*, t) Sigma^-1 K(t, t*)."""
    t, y, diag = (np.asarray(x, dtype=np.float64) for x in (t, y, diag))
    K, Sg = dense_sigma(t, diag, Jr, Jc, co, diag_add)
    inv = np.linalg.inv(Sg)
    alpha = inv @ y
    out = dict(alpha=alpha, mu=y - diag * alpha, hdiag=np.diag(inv).copy(),
               var=diag_add - np.einsum("ij,jk,ik->i", K, inv, K), var_at=None)
    if ts is not None:
        Ks = kernel_value(np.asarray(ts, dtype=np.float64)[:, None] - t[None, :], Jr, Jc, *co)
        out["var_at"] = diag_add - np.einsum("ij,jk,ik->i", Ks, inv, Ks)
    return out


def loo_reference(t, y, diag, Jr, Jc, co, diag_add):
    """(mean, var) of y_n given every other row, row by row: the row and column of Sigma deleted, then the textbook
    prediction of an observation (its own noise included)."""
    t, y, diag = (np.asarray(x, dtype=np.float64) for x in (t, y, diag))
    _, Sg = dense_sigma(t, diag, Jr, Jc, co, diag_add)
    N = len(t)
    mean, var = np.zeros(N), np.zeros(N)
    for n in range(N):
        keep = np.arange(N) != n
        if N == 1:
            mean[n], var[n] = 0.0, Sg[n, n]
            continue
        sol = np.linalg.solve(Sg[np.ix_(keep, keep)], np.column_stack([y[keep], Sg[keep, n]]))
        mean[n] = Sg[n, keep] @ sol[:, 0]
        var[n] = Sg[n, n] - Sg[n, keep] @ sol[:, 1]
    return mean, var


def queries(t, dt):
    """Ascending query times around the rows of ``t`` (typical spacing ``dt``): before t_0, t_0 - 1e-9, ties at t_0, a
    middle row and the last row, mid-interval points (the gap of grad_cases' axes among them), after the end."""
    N = len(t)
    q = [t[0] - 5 * dt, t[0] - 1e-9, t[0], t[N // 2], t[N - 1], t[N - 1] + 0.3 * dt, t[N - 1] + 40 * dt]
    q += [0.5 * (t[n] + t[n + 1]) for n in sorted({0, max(N // 2 - 1, 0), N - 2}) if 0 <= n < N - 1]
    q += [t[n] + 0.25 * (t[n + 1] - t[n]) for n in (N // 3,) if n < N - 1]
    return np.sort(np.array(q))


def work_formula(N, W, M, seg, lib_seg):
    """gf_var_batch_work: gf_solve_batch's workspace for the segment length in use (``lib_seg`` =
    gf_solve_batch_seg(N, W) when seg = 0), one Y slot and 64 doubles per query."""
    WM = 16 if W <= 16 else 32 if W <= 32 else 64
    K = lib_seg if seg == 0 else min(seg, N)
    nseg = -(-N // K)
    return nseg * (WM + 4) * 64 + K * 3 * 64 + 2 * (-(-N // 64) * 64) + WM * 64 + M * 64


def var_passes(t, y, diag, Jr, Jc, co, diag_add, seg, ts=None, nobs=None, dtype=np.float64):
    """The device's two passes for one problem.  ``co`` = (ar, cr, ac, bc, cc, dc), ``seg`` rows per segment, ``ts``
    ascending query times or None, ``nobs`` real rows (the rest are missing-data rows at the end) or None for all.
    Returns dict(ll, info, alpha, mu, hdiag, var, var_at) in ``dtype``."""
    t64 = np.asarray(t, dtype=np.float64)
    t, y = t64.astype(dtype), np.asarray(y, dtype=np.float64).astype(dtype)
    N = len(t)
    diag = np.zeros(N, dtype=dtype) if diag is None else np.asarray(diag, dtype=np.float64).astype(dtype)
    co = tuple(np.asarray(x, dtype=np.float64).astype(dtype) for x in co)
    c, U, V, _, _ = rows(t64, Jr, Jc, *co, dtype=dtype)
    W = len(c)
    k0 = dtype(diag_add)
    A = diag + k0
    K = int(min(max(seg, 1), N))
    nseg = -(-N // K)
    No = N if nobs is None else int(nobs)
    M = 0 if ts is None else len(ts)
    if M:
        ts64 = np.asarray(ts, dtype=np.float64)
        tq = ts64.astype(dtype)
        _, Uq, Vq, _, _ = rows(ts64, Jr, Jc, *co, dtype=dtype)
    Rq, var_at = np.zeros((M, W), dtype=dtype), np.zeros(M, dtype=dtype)

    def fwd(state, n):
        S, G, w, D, z = state
        p = np.exp(c * ((t[n - 1] if n else t[n]) - t[n]))
        S = p[:, None] * p[None, :] * (S + D * np.outer(w, w))
        f = S @ U[n]
        G = p * (G + w * z)
        D = A[n] - U[n] @ f
        z = y[n] - U[n] @ G
        w = (V[n] - f) / D
        return (S, G, w, D, z), p

    # pass 1
    state = (np.zeros((W, W), dtype=dtype), np.zeros(W, dtype=dtype), np.zeros(W, dtype=dtype), dtype(0), dtype(0))
    ck, zs, Ds = [], np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    m = 0
    while m < M and (No == 0 or tq[m] < t[0]):                 # owned by no row
        Rq[m], var_at[m] = Vq[m], k0
        m += 1
    for n in range(N):
        if n % K == 0:
            ck.append(state)
        state, _ = fwd(state, n)
        S, _, w, D, _ = state
        if not D > 0.0:
            nan = np.full(N, np.nan)
            return dict(ll=-np.inf, info=n + 1, alpha=nan, mu=nan, hdiag=nan, var=nan,
                        var_at=np.full(M, np.nan) if M else None)
        Ds[n], zs[n] = state[3], state[4]
        while m < M and n < No and (n + 1 >= No or tq[m] < t[n + 1]):
            ps = np.exp(c * (t[n] - tq[m]))
            f = (ps[:, None] * ps[None, :] * (S + D * np.outer(w, w))) @ Uq[m]
            Rq[m], var_at[m] = Vq[m] - f, k0 - Uq[m] @ f
            m += 1
    ll = -0.5 * (np.sum(np.log(Ds)) + np.sum(zs * zs / Ds) + N * np.log(2.0 * dtype(np.pi)))
    # pass 2
    alpha, h = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    H, un, pn, an = np.zeros(W, dtype=dtype), np.zeros(W, dtype=dtype), np.zeros(W, dtype=dtype), dtype(0)
    Y = np.zeros((W, W), dtype=dtype)
    mq = M - 1
    while mq >= 0 and (No == 0 or tq[mq] >= t[No - 1]):        # owned by the last row: var* = d*
        mq -= 1
    for s in range(nseg - 1, -1, -1):
        n0, n1 = s * K, min(s * K + K, N)
        state, staged = ck[s], []
        for n in range(n0, n1):
            state, p = fwd(state, n)
            staged.append((state[2], U[n], p))
        for n in range(n1 - 1, n0 - 1, -1):
            w, u, p = staged[n - n0]
            H = pn * (H + un * an)
            a = zs[n] / Ds[n] - w @ H
            Z = pn[:, None] * pn[None, :] * Y
            q = Z @ w
            h[n] = 1.0 / Ds[n] + w @ q
            r = 0.5 * h[n] * u - q
            Y = Z + np.outer(u, r) + np.outer(r, u)
            un, pn, an = u, p, a
            alpha[n] = a
            while mq >= 0 and (n == 0 or tq[mq] >= t[n - 1]):
                x = np.exp(c * (tq[mq] - t[n])) * Rq[mq]
                var_at[mq] = var_at[mq] - x @ Y @ x
                mq -= 1
    return dict(ll=ll, info=0, alpha=alpha, mu=y - diag * alpha, hdiag=h, var=diag * (1.0 - diag * h),
                var_at=var_at if M else None)
