"""Test oracle of the batched sampler (numpy, no GPU): the recurrence the sampling sweeps implement, in its plain
(unscaled) form, and the reference's centring rule.

The sweeps carry the symmetric state S of the factorisation (K = L D L^T, celerite's recurrence) with one MORE column
F, the state of the draw, updated by the same rank-one step with its own multiplier:

    T = [S | F]  (W x (W + 1));   after row n:  T <- T + r_n q_n^T,   q_n = [r_n / d_n | x_n / d_n]
    before row n:  T <- diag(p_n) T diag([p_n | 1]),   p_n = exp(-c (t_n - t_{n-1}))
    tmp = S u_n;  d_n = a_n - u_n . tmp;  r_n = v_n - tmp  (= d_n w_n);
    x_n = sqrt(d_n) eps_n;  out_n = x_n + u_n . F

which is y = L D^{1/2} eps (celerite2's matmul_lower with V := W after factor): the forward solve of the
log-likelihood with the sign flipped and the input carried instead of the output.
"""
import numpy as np


def draw(t, c, a, U, V, eps):
    """(out, d, info): out = L D^{1/2} eps row by row as above; info = 0 or the 1-based failing row (out is NaN
    from there on)."""
    dtype = U.dtype
    N, W = U.shape
    eps = np.asarray(eps, dtype=dtype)
    T = np.zeros((W, W + 1), dtype=dtype)
    out = np.full(N, np.nan, dtype=dtype)
    d = np.array(a, dtype=dtype, copy=True)
    r = np.zeros(W, dtype=dtype)
    q = np.zeros(W + 1, dtype=dtype)
    one = np.ones(1, dtype=dtype)
    for n in range(N):
        if n > 0:
            p = np.exp(c * (t[n - 1] - t[n]))
            T = p[:, None] * (T + np.outer(r, q)) * np.concatenate([p, one])[None, :]
        tmp = T[:, :W] @ U[n]
        d[n] = a[n] - U[n] @ tmp
        if not d[n] > 0:
            return out, d, n + 1
        r = V[n] - tmp
        x = np.sqrt(d[n]) * eps[n]
        out[n] = x + U[n] @ T[:, W]
        q = np.concatenate([r, x[None]]) / d[n]
    return out, d, 0


def center(x, size):
    """The reference's rule for one problem's draws: the time-mean of a single draw ((N,), size None) is removed,
    the across-realisation mean of `size` draws ((size, N)) -- `result -= result.mean(axis=0 if 2-D else None)`."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == (1 if size is None else 2)
    return x - (x.mean() if size is None else x.mean(axis=0))
