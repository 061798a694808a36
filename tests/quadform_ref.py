"""References of gf_quadform_grad, host only: numpy and the oracle, no device import.

Two independent statements of x^T (d K / d theta) x for every celerite coefficient theta:
  * :func:`recurrences`: the numpy restatement of the diagonal linear recurrences the device runs, on the generator
    rows cos / sin of theta_n = fl(d t_n) (the matrix gf_loglike_grad differentiates, on any axis);
  * :func:`dense_forms`: x^T D x with the closed-form derivative matrices D of oracle/dense.kernel_value over the lags
    (:func:`derivative_matrices`, pinned to central differences of kernel_value by tests/test_quadform_host.py).
Both return the value PER VECTOR, so that one reference of the most vectors serves every smaller count and every
weighting: sum_r w_r q_r.  Lag zero belongs to the diagonal: it is not part of d/da."""
import numpy as np

NAMES = ("ar", "cr", "ac", "bc", "cc", "dc")


def derivative_matrices(t, co):
    """dict name -> (J, N, N): d K / d (a_r, c_r, a_c, b_c, c_c, d_c) of oracle/dense.kernel_value over the lags
    |t_i - t_j|, zero on the diagonal."""
    ar, cr, ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in co)
    t = np.asarray(t, dtype=np.float64)
    tau = np.abs(t[:, None] - t[None, :])[None]
    off = 1.0 - np.eye(len(t))[None]
    er = np.exp(-cr[:, None, None] * tau)
    ec = np.exp(-cc[:, None, None] * tau)
    co_, si = np.cos(dc[:, None, None] * tau), np.sin(dc[:, None, None] * tau)
    a, b = ac[:, None, None], bc[:, None, None]
    return dict(ar=er * off, cr=-ar[:, None, None] * tau * er * off,
                ac=ec * co_ * off, bc=ec * si * off,
                cc=-tau * ec * (a * co_ + b * si) * off, dc=tau * ec * (b * co_ - a * si) * off)


def dense_forms(t, co, X):
    """(q, scale): dicts name -> (R, J), q_r = x_r^T D x_r and scale_r = |x_r|^T |D| |x_r| for the R rows of X (R, N);
    ``q["diag"]``, ``scale["diag"]`` (R,) = |x_r|^2."""
    X = np.asarray(X, dtype=np.float64)
    q, scale = {}, {}
    for k, D in derivative_matrices(t, co).items():
        q[k] = np.einsum("rn,jnm,rm->rj", X, D, X, optimize=True)
        scale[k] = np.einsum("rn,jnm,rm->rj", np.abs(X), np.abs(D), np.abs(X), optimize=True)
    q["diag"] = scale["diag"] = np.sum(X * X, axis=1)
    return q, scale


def recurrences(t, co, X, dtype=np.float64):
    """dict name -> (R, J) (and ``diag`` (R,)) by the recurrences of gadfly_quadform.hip, row by row:
        F <- p (F + v_{n-1} x_{n-1}),  T <- p T + dt F,  sums of x_n v_n F and x_n v_n T
    with v = 1 (real term), cos theta_n and sin theta_n (complex term), theta_n = fl(d t_n) in float64 whatever
    ``dtype``."""
    ar, cr, ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in co)
    t64 = np.asarray(t, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    R, N = X.shape
    th = (dc[None, :] * t64[:, None])
    cs, sn = np.cos(th.astype(dtype)), np.sin(th.astype(dtype))
    tt = t64.astype(dtype)
    arx, crx, acx, bcx, ccx = (v.astype(dtype) for v in (ar, cr, ac, bc, cc))
    Jr, Jc = len(ar), len(ac)
    z = lambda J: np.zeros((R, J), dtype=dtype)               # noqa: E731
    Fr, Tr, P1r, P2r = z(Jr), z(Jr), z(Jr), z(Jr)
    Fc, Fs, Tc, Ts, C1, S1, C2, S2 = (z(Jc) for _ in range(8))
    for n in range(1, N):
        dt = tt[n] - tt[n - 1]
        x0, x1 = X[:, n - 1][:, None], X[:, n][:, None]
        p = np.exp(-crx * dt)[None]
        Fr = p * (Fr + x0)
        Tr = p * Tr + dt * Fr
        P1r += x1 * Fr
        P2r += x1 * Tr
        p = np.exp(-ccx * dt)[None]
        Fc = p * (Fc + cs[n - 1][None] * x0)
        Fs = p * (Fs + sn[n - 1][None] * x0)
        Tc = p * Tc + dt * Fc
        Ts = p * Ts + dt * Fs
        C1 += x1 * (cs[n][None] * Fc + sn[n][None] * Fs)
        S1 += x1 * (sn[n][None] * Fc - cs[n][None] * Fs)
        C2 += x1 * (cs[n][None] * Tc + sn[n][None] * Ts)
        S2 += x1 * (sn[n][None] * Tc - cs[n][None] * Ts)
    out = dict(ar=2 * P1r, cr=-2 * arx[None] * P2r, ac=2 * C1, bc=2 * S1,
               cc=-2 * (acx[None] * C2 + bcx[None] * S2), dc=2 * (bcx[None] * C2 - acx[None] * S2),
               diag=np.sum(X * X, axis=1))
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def weighted(q, R, w=None):
    """sum over the first R vectors of w_r q_r for every entry of a per-vector dict: name -> (J,), ``diag`` a float."""
    w = np.ones(R) if w is None else np.asarray(w, dtype=np.float64)[:R]
    return {k: np.tensordot(w, v[:R], axes=(0, 0)) for k, v in q.items()}


def stacked(g, Jr, Jc):
    """A dict of :func:`weighted` in gf_loglike_grad's layout: (real (2, Jr), comp (4, Jc), diag)."""
    return np.stack([g["ar"], g["cr"]]), np.stack([g["ac"], g["bc"], g["cc"], g["dc"]]), float(g["diag"])
