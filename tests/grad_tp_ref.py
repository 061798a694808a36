"""TEST INFRASTRUCTURE: numpy restatement of the time-parallel gradient (gadfly_gradtp.hip), stage by
stage, in the notation of tests/grad_ref.loglike_grad: the plain, unscaled recurrence with exact rows.  Never imported
by the product.

A chunk [n0, n1) takes the state (X, Y) = (M_n0, H_n0) that enters its first row; the first row of a chunk applies P
with dt = t[n0 - 1] - t[n0] like any other row (only row 0 of the series has dt = 0).
  A  nominal pass from (0, 0): the chunk map (Phi, G, Xbar, Ybar, m) of oracle/lft.py in plain coordinates;
     lft.start_states gives the true start of every chunk
  B  forward pass from the true starts: log L, the rows, the true Phi
  C  reverse sweep 1 from (0, 0) -> srcH, scan -> Hbar at every boundary; sweep 2 from (0, Hbar) -> srcM, scan -> Mbar
     at every boundary; sweep 3 from the true terminals -> the adjoints.
"""
import numpy as np

from oracle import lft
from tests.grad_ref import rows


def fwd_chunk(c, U, V, A, y, dtn, n0, n1, X, Y):
    """Rows n0 .. n1 - 1 from the start state (X, Y): end state, Phi = prod A_n, Gram sums G, m, the rows' values
    (S, f, D, G, z, w, p), sum log D, sum z^2 / D, and the 1-based row of a non-positive pivot (0: none)."""
    W = len(c)
    Phi, G, m = np.eye(W), np.zeros((W, W)), np.zeros(W)
    R, ld, qd = [], 0.0, 0.0
    for n in range(n0, n1):
        p = np.exp(c * dtn[n])
        S = p[:, None] * p[None, :] * X
        f = S @ U[n]
        D = A[n] - U[n] @ f
        if not D > 0:
            return X, Y, Phi, G, m, R, ld, qd, n + 1
        Gn = p * Y
        z = y[n] - U[n] @ Gn
        w = (V[n] - f) / D
        h = Phi.T @ (p * U[n])
        G += np.outer(h, h) / D
        m += h * z / D
        Phi = (np.eye(W) - np.outer(w, U[n])) @ (p[:, None] * Phi)
        R.append((S, f, D, Gn, z, w, p))
        X, Y = S + D * np.outer(w, w), Gn + w * z
        ld += np.log(D)
        qd += z * z / D
    return X, Y, Phi, G, m, R, ld, qd, 0


def rev_chunk(U, dtn, n0, n1, R, Mb, Hb):
    """The reverse step over the rows of a chunk from the terminal adjoint (Mb, Hb) of its end state: the adjoint of
    its start state, Ubar, Vbar of its rows, and its share of cbar, sum Abar, sum ybar."""
    W = U.shape[1]
    Ub, Vb, cb, Ab, yb = np.zeros((n1 - n0, W)), np.zeros((n1 - n0, W)), np.zeros(W), 0.0, 0.0
    for n in range(n1 - 1, n0 - 1, -1):
        S, fn, Dn, Gn, zn, wn, p = R[n - n0]
        un = U[n]
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
        ub += S @ fb
        Sb = Mb + 0.5 * (np.outer(fb, un) + np.outer(un, fb))
        cb += dtn[n] * (2.0 * np.sum(Sb * S, axis=1) + Gb * Gn)
        Mb = p[:, None] * p[None, :] * Sb
        Hb = p * Gb
        Ub[n - n0], Vb[n - n0] = ub, vb
        Ab += Db
        yb += zb
    return Mb, Hb, Ub, Vb, cb, Ab, yb


def loglike_grad_chunked(t, y, diag, Jr, Jc, ar, cr, ac, bc, cc, dc, diag_add, chunk_len):
    """(ll, g, stages): ll and g as tests/grad_ref.loglike_grad; stages a dict of
    bounds [(n0, n1)], maps [(Phi, G, Xbar, Ybar, m)] of the nominal pass, starts [(X, Y)] from lft.start_states,
    Phi (true), Hout / Mout (the scans' terminal adjoints of every chunk) and Hin / Min (what sweep 3 returns as the
    adjoint of every chunk's start state: chunk c's equals Hout / Mout of chunk c - 1)."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = len(t)
    c, U, V, co, si = rows(t, Jr, Jc, ar, cr, ac, bc, cc, dc)
    W = len(c)
    A = np.asarray(diag, dtype=np.float64) + diag_add
    dtn = np.concatenate([[0.0], t[:-1] - t[1:]])
    L = min(int(chunk_len), N)
    bounds = [(a, min(a + L, N)) for a in range(0, N, L)]
    nc = len(bounds)
    maps = []
    for a, b in bounds:
        Xb, Yb, Ph, G, m = fwd_chunk(c, U, V, A, y, dtn, a, b, np.zeros((W, W)), np.zeros(W))[:5]
        maps.append((Ph, G, Xb, Yb, m))
    starts = lft.start_states(maps)
    F, ld, qd = [], 0.0, 0.0
    for (a, b), (X, Y) in zip(bounds, starts):
        _, _, Ph, _, _, R, l, q, bad = fwd_chunk(c, U, V, A, y, dtn, a, b, X, Y)
        assert bad == 0, bad
        F.append((Ph, R))
        ld += l
        qd += q
    ll = -0.5 * (qd + ld + N * np.log(2 * np.pi))
    zM, zH = np.zeros((W, W)), np.zeros(W)
    srcH = [rev_chunk(U, dtn, a, b, F[i][1], zM, zH)[1] for i, (a, b) in enumerate(bounds)]
    Hout, Hb = [None] * nc, zH
    for i in range(nc - 1, -1, -1):
        Hout[i] = Hb
        Hb = F[i][0].T @ Hb + srcH[i]
    srcM = [rev_chunk(U, dtn, a, b, F[i][1], zM, Hout[i])[0] for i, (a, b) in enumerate(bounds)]
    Mout, Mb = [None] * nc, zM
    for i in range(nc - 1, -1, -1):
        Mout[i] = Mb
        Mb = F[i][0].T @ Mb @ F[i][0] + srcM[i]
    Ub, Vb, cb, Ab, yb = np.zeros((N, W)), np.zeros((N, W)), np.zeros(W), 0.0, 0.0
    Hin, Min = [], []
    for i, (a, b) in enumerate(bounds):
        Mi, Hi, ub, vb, cbi, Abi, ybi = rev_chunk(U, dtn, a, b, F[i][1], Mout[i], Hout[i])
        Ub[a:b], Vb[a:b] = ub, vb
        cb += cbi
        Ab += Abi
        yb += ybi
        Hin.append(Hi)
        Min.append(Mi)
    g = dict(ar=np.sum(Ub[:, :Jr], axis=0), cr=cb[:Jr])
    U0b, U1b, V0b, V1b = Ub[:, Jr::2], Ub[:, Jr + 1::2], Vb[:, Jr::2], Vb[:, Jr + 1::2]
    U0, U1 = U[:, Jr::2], U[:, Jr + 1::2]
    g["ac"] = np.sum(U0b * co + U1b * si, axis=0)
    g["bc"] = np.sum(U0b * si - U1b * co, axis=0)
    g["cc"] = cb[Jr::2] + cb[Jr + 1::2]
    th = -U0b * U1 + U1b * U0 - V0b * si + V1b * co
    g["dc"] = np.sum((t - t[0])[:, None] * th, axis=0)
    g["diag_add"], g["mean"] = Ab, -yb
    stages = dict(bounds=bounds, maps=maps, starts=starts, Phi=[f[0] for f in F], Hout=Hout, Mout=Mout, Hin=Hin,
                  Min=Min, c=c, U=U, V=V, A=A, dtn=dtn)
    return ll, g, stages


def sequential_states(stages, y):
    """(M, H) entering the first row of every chunk by the sequential recurrence over the whole series."""
    c, U, V, A, dtn = (stages[k] for k in ("c", "U", "V", "A", "dtn"))
    W = len(c)
    X, Y, out = np.zeros((W, W)), np.zeros(W), []
    for a, b in stages["bounds"]:
        out.append((X, Y))
        X, Y = fwd_chunk(c, U, V, A, np.asarray(y, dtype=np.float64), dtn, a, b, X, Y)[:2]
    return out
