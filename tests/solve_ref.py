"""
Test references of the batched conditional mean; in tests/ because oracle/ is frozen.

* :func:`oracle_predict` -- the yardstick: oracle/seq.py's ``factor``, ``apply_inverse``, ``log_likelihood`` and
  ``predict_mean_at`` at t* = t on raw coefficients of any structure, in float64 or 80-bit.
* :func:`solve_passes` -- a numpy restatement of the three passes gf_solve_batch runs: the forward sweep with a
  checkpoint every ``seg`` rows, the segments recomputed last first with the upper solve over their staged rows, and
  the component's forward pass over the finished alpha.
* :func:`split_component` -- the first ``num / den`` of each kind of term of a stacked coefficient pack.
"""
import numpy as np

from oracle import seq
from tests.grad_ref import rows


def matrices(t, co, dtype=np.float64):
    """(c, U, V) of seq.celerite_matrices for (ar, cr, ac, bc, cc, dc) in ``dtype`` (an 80-bit pass rounds the phases
    d t in 80-bit too: on a far time axis that is another matrix, not a better value of the float64 one)."""
    c, _, U, V = seq.celerite_matrices(co, t, 0.0, dtype=dtype)
    return c, U, V


def oracle_predict(t, y, diag, co, diag_add, comp=None, dtype=np.float64):
    """dict(ll, info, alpha, mu, mu_comp) of one problem from oracle/seq.py: A_n = diag_n + diag_add, alpha =
    apply_inverse(y), mu = y - diag alpha, mu_comp = predict_mean_at(t* = t) with the component's U', V', c'."""
    t, y, diag = (np.asarray(x, dtype=dtype) for x in (t, y, diag))
    c, U, V = matrices(t, co, dtype)
    a = diag + dtype(diag_add)
    d, Wm, info = seq.factor(t, c, a, U, V)
    N = len(t)
    if info:
        nan = np.full(N, np.nan)
        return dict(ll=-np.inf, info=info, alpha=nan, mu=nan, mu_comp=None if comp is None else nan)
    alpha = seq.apply_inverse(t, c, U, Wm, d, y)
    ll, _ = seq.log_likelihood(t, c, a, U, V, y)
    out = dict(ll=ll, info=0, alpha=alpha, mu=y - diag * alpha, mu_comp=None)
    if comp is not None:
        c2, U2, V2 = matrices(t, comp, dtype)
        out["mu_comp"] = seq.predict_mean_at(t, c2, U2, V2, alpha, t, U2, V2)
    return out


def split_component(Jr, Jc, real, comp, num=1, den=2):
    """The first ``num / den`` of each kind of term (at least one term in all): (Jr', Jc', real', comp') in the stacked
    layout, real' (2, B, max(Jr', 1)), comp' (4, B, max(Jc', 1))."""
    jr, jc = Jr * num // den, Jc * num // den
    if jr + jc == 0:
        jr, jc = (1, 0) if Jr else (0, 1)
    B = real.shape[1]
    r2, c2 = np.zeros((2, B, max(jr, 1))), np.zeros((4, B, max(jc, 1)))
    r2[:, :, :jr], c2[:, :, :jc] = real[:, :, :jr], comp[:, :, :jc]
    return jr, jc, r2, c2


def solve_passes(t, y, diag, Jr, Jc, co, diag_add, seg, comp=None):
    """The device's three passes for one problem in float64.  ``co`` = (ar, cr, ac, bc, cc, dc), ``comp`` = (Jr', Jc',
    the six arrays of the component) or None, ``seg`` rows per segment.  Returns dict(ll, info, alpha, mu, mu_comp)."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = len(t)
    diag = np.zeros(N) if diag is None else np.asarray(diag, dtype=np.float64)
    c, U, V, _, _ = rows(t, Jr, Jc, *co)
    W = len(c)
    A = diag + diag_add
    K = int(min(max(seg, 1), N))
    nseg = -(-N // K)

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
    state = (np.zeros((W, W)), np.zeros(W), np.zeros(W), 0.0, 0.0)
    ck, zs, Ds = [], np.zeros(N), np.zeros(N)
    for n in range(N):
        if n % K == 0:
            ck.append(state)
        state, _ = fwd(state, n)
        if not state[3] > 0.0:
            nan = np.full(N, np.nan)
            return dict(ll=-np.inf, info=n + 1, alpha=nan, mu=nan, mu_comp=None if comp is None else nan)
        Ds[n], zs[n] = state[3], state[4]
    ll = -0.5 * (np.sum(np.log(Ds)) + np.sum(zs * zs / Ds) + N * np.log(2.0 * np.pi))
    # pass 2
    if comp is not None:
        c2, U2, V2, _, _ = rows(t, comp[0], comp[1], *comp[2:])
        W2 = len(c2)
        H2, u2n, up = np.zeros(W2), np.zeros(W2), np.zeros(N)
    alpha = np.zeros(N)
    H, un, pn, an, tnext = np.zeros(W), np.zeros(W), np.zeros(W), 0.0, t[N - 1]
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
            if comp is not None:
                H2 = np.exp(c2 * (t[n] - tnext)) * (H2 + u2n * an)
                up[n] = V2[n] @ H2
                u2n, tnext = U2[n], t[n]
            un, pn, an = u, p, a
            alpha[n] = a
    out = dict(ll=ll, info=0, alpha=alpha, mu=y - diag * alpha, mu_comp=None)
    # pass 3
    if comp is not None:
        F, lo = np.zeros(W2), np.zeros(N)
        for n in range(N):
            F = np.exp(c2 * ((t[n - 1] if n else t[n]) - t[n])) * F + V2[n] * alpha[n]
            lo[n] = U2[n] @ F
        out["mu_comp"] = lo + up
    return out
