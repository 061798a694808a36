"""TEST INFRASTRUCTURE: the chunk-map algebra of oracle/lft.py in 80-bit ``np.longdouble``, the reference of
tests/test_gpu_chunk_combine.py and tests/test_gpu_chunk_corrections.py (gf_chunk_combine, gf_chunk_combine_tree,
gf_chunk_corrections at their raw entry points).  Never imported by the product.

* :func:`gauss_jordan` -- numpy.linalg does not take longdouble: Gauss-Jordan with partial pivoting, one vectorised
  rank-one update per pivot; the pivots give log |det| and its sign.
* :func:`apply`, :func:`compose`, :func:`start_states` -- the formulas of oracle/lft.py.
* :func:`corrections` -- log det(I - X G) and e^T G v - 2 m^T e - m^T X m of the two-sweep evaluation
  (include/gadfly_hip.h, gf_chunk_corrections).
* :func:`synthetic` -- the random family of oracle/lft.random_maps, one seed per (width, problem).
* :func:`real_maps` -- the nominal-pass maps of a tests/grad_cases.edge_problem in plain, unscaled coordinates (what
  gf_loglike_grad_chunked hands the combines), with the true start states and the per-chunk differences of
  sum log D and sum z^2 / D by the SEQUENTIAL recurrence over the whole series: independent of the map algebra.
* :func:`planted_failure` -- a problem whose nominal pass is healthy and whose true pivots are not.
* :func:`pack_matrices`, :func:`pack_vectors`, :func:`unpack_matrices` -- the device's 64 x 64 slots.
"""
import functools

import numpy as np

from oracle import lft
from tests import grad_cases as gc
from tests.grad_ref import rows

LD = np.longdouble
SLOT = 64


def gauss_jordan(A, rhs, dtype=LD):
    """(A^-1 rhs, log |det A|, sign det A) by Gauss-Jordan elimination with partial pivoting on [A | rhs]."""
    A = np.asarray(A, dtype=dtype)
    n = A.shape[0]
    M = np.concatenate([A, np.asarray(rhs, dtype=dtype).reshape(n, -1)], axis=1)
    logdet, sign = dtype(0.0), 1
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            sign = -sign
        piv = M[k, k]
        if piv == 0.0:
            raise np.linalg.LinAlgError("singular matrix")
        if piv < 0.0:
            sign = -sign
        logdet += np.log(np.abs(piv))
        row = M[k] / piv
        f = M[:, k].copy()
        f[k] = 0.0
        M -= f[:, None] * row[None, :]
        M[k] = row
    return M[:, n:], logdet, sign


def _ld(M):
    return tuple(np.asarray(x, dtype=LD) for x in M)


def apply(M, X, Y):
    """State (X, Y) through one chunk map (oracle/lft.apply)."""
    Ph, G, Xb, Yb, m = _ld(M)
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    n = Ph.shape[0]
    sol = gauss_jordan(np.eye(n, dtype=LD) - X @ G, np.concatenate([X, (Y - X @ m)[:, None]], axis=1))[0]
    K, v = sol[:, :n], sol[:, n]
    K = (K + K.T) / 2
    Xn = Xb + Ph @ K @ Ph.T
    return (Xn + Xn.T) / 2, Yb + Ph @ v


def compose(M1, M2):
    """The map of chunk 1 followed by chunk 2 (oracle/lft.compose)."""
    P1, G1, X1, Y1, m1 = _ld(M1)
    P2, G2, X2, Y2, m2 = _ld(M2)
    n = P1.shape[0]
    sol = gauss_jordan(np.eye(n, dtype=LD) - X1 @ G2, np.concatenate([P1, X1, (Y1 - X1 @ m2)[:, None]], axis=1))[0]
    DP1, DX1, v = sol[:, :n], sol[:, n:2 * n], sol[:, 2 * n]
    X12 = X2 + P2 @ DX1 @ P2.T
    G12 = G1 + P1.T @ G2 @ DP1
    return P2 @ DP1, (G12 + G12.T) / 2, (X12 + X12.T) / 2, Y2 + P2 @ v, m1 + P1.T @ (m2 - G2 @ v)


def start_states(maps):
    """Start state of every chunk by applying the maps one after the other from a zero state: the states of the
    first k chunks are the first k entries whatever follows."""
    n = maps[0][0].shape[0]
    X, Y = np.zeros((n, n), dtype=LD), np.zeros(n, dtype=LD)
    out = []
    for i, M in enumerate(maps):
        out.append((X, Y))
        if i + 1 < len(maps):
            X, Y = apply(M, X, Y)
    return out


def corrections(X, Y, G, m, dtype=LD):
    """(log |det(I - X G)|, e^T G v - 2 m^T e - m^T X m, sign det(I - X G)) with e = Y - X m, v = (I - X G)^-1 e."""
    X, Y, G, m = (np.asarray(x, dtype=dtype) for x in (X, Y, G, m))
    e = Y - X @ m
    v, logdet, sign = gauss_jordan(np.eye(len(Y), dtype=dtype) - X @ G, e, dtype)
    return logdet, e @ (G @ v[:, 0]) - 2 * (m @ e) - m @ (X @ m), sign


def corrections64(X, Y, G, m):
    """The same two values in float64 with numpy.linalg (LU with partial pivoting): what a plain float64 evaluation
    of the formulas gives, the yardstick of the device's bar."""
    X, Y, G, m = (np.asarray(x, dtype=np.float64) for x in (X, Y, G, m))
    e = Y - X @ m
    A = np.eye(len(Y)) - X @ G
    return np.linalg.slogdet(A)[1], e @ (G @ np.linalg.solve(A, e)) - 2 * (m @ e) - m @ (X @ m)


def chunk_conditions(maps, starts):
    """cond(I - X_c G_c) of every chunk: the solves of the sequential combine (chunk 0: the identity)."""
    return [float(np.linalg.cond(np.eye(len(Y)) - np.asarray(X @ M[1], dtype=np.float64)))
            for M, (X, Y) in zip(maps, starts)]


def chain_condition(maps, starts):
    """The largest of them: kappa of a chain."""
    return max(chunk_conditions(maps, starts))


def scaled_error(got, ref, floor=1.0):
    """max |got - ref| / max(floor, max |ref|), in 80 bits."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / max(LD(floor), np.max(np.abs(ref))))


# ---- the case generators ----------------------------------------------------------------------------------------
def synthetic(W, nch, b=0, rank=None):
    """Problem b of the synthetic family at width W: lft.random_maps (non-symmetric Phi, PSD Xbar, NSD G) from the
    generator seeded with W (b = 0) or (W, b); rank min(6, W) unless given."""
    rng = np.random.default_rng(W if b == 0 else [W, b])
    return lft.random_maps(rng, nch, W, rank=min(6, W) if rank is None else rank)


@functools.lru_cache(maxsize=None)
def synthetic_case(W, nch, b=0, rank=None):
    """dict(maps, starts (80-bit), starts64 (oracle/lft.py in float64), conds (cond(I - X G) per chunk), W) of
    synthetic(W, nch, b, rank): computed once, shared, never changed.  A chain's first k chunks are the chain of k
    chunks."""
    maps = synthetic(W, nch, b, rank)
    starts = start_states(maps)
    return dict(maps=maps, starts=starts, starts64=lft.start_states(maps), conds=chunk_conditions(maps, starts), W=W)


@functools.lru_cache(maxsize=None)
def real_case(Jr, Jc, N, L, b=0):
    """The same dict for real_maps(Jr, Jc, N, L, b): maps rounded to float64 (what the device is given), starts the
    80-bit SEQUENTIAL states, starts64 oracle/lft.py on the rounded maps; with dld, dqd of real_maps."""
    r = real_maps(Jr, Jc, N, L, b)
    maps = [tuple(np.asarray(x, dtype=np.float64) for x in M) for M in r["maps"]]
    return dict(maps=maps, starts=r["starts"], starts64=lft.start_states(maps),
                conds=chunk_conditions(r["maps"], r["starts"]), W=r["W"], dld=r["dld"], dqd=r["dqd"])


def fwd_chunk(c, U, V, A, y, dtn, n0, n1, X, Y, stop=True):
    """tests/grad_tp_ref.fwd_chunk in the dtype of its arguments, Phi updated by its rank-one form: rows n0 .. n1 - 1
    from the start state (X, Y) -> dict(X, Y (end state), Phi, G, m, ld = sum log |D|, qd = sum z^2 / D,
    bad = 1-based rows of the non-positive pivots).  ``stop``: end at the first such row (as the product does); else
    carry on through it with the indefinite state."""
    dt = U.dtype.type
    W = len(c)
    Phi, G, m = np.eye(W, dtype=dt), np.zeros((W, W), dtype=dt), np.zeros(W, dtype=dt)
    ld, qd, bad = dt(0.0), dt(0.0), []
    for n in range(n0, n1):
        p = np.exp(c * dtn[n])
        S = p[:, None] * p[None, :] * X
        f = S @ U[n]
        D = A[n] - U[n] @ f
        if not D > 0:
            bad.append(n + 1)
            if stop:
                break
        Gn = p * Y
        z = y[n] - U[n] @ Gn
        w = (V[n] - f) / D
        pu = p * U[n]
        h = Phi.T @ pu
        G += h[:, None] * h[None, :] / D
        m += h * z / D
        Phi = p[:, None] * Phi
        Phi -= w[:, None] * (U[n] @ Phi)[None, :]
        X, Y = S + D * w[:, None] * w[None, :], Gn + w * z
        ld += np.log(np.abs(D))
        qd += z * z / D
    return dict(X=X, Y=Y, Phi=Phi, G=G, m=m, ld=ld, qd=qd, bad=bad)


def _problem_rows(prob, b, dtype, diag=None):
    co = [np.asarray(x, dtype=np.float64).astype(dtype) for x in gc.coefficients(prob, b)]
    c, U, V, _, _ = rows(prob["t"], prob["Jr"], prob["Jc"], *co, dtype)
    t = prob["t"].astype(dtype)
    A = (prob["diag"][b] if diag is None else np.asarray(diag)).astype(dtype) + dtype(prob["diag_add"][b])
    dtn = np.concatenate([np.zeros(1, dtype=dtype), t[:-1] - t[1:]])
    return c, U, V, A, prob["y"][b].astype(dtype), dtn


def _maps_of(prob, b, L, dtype, diag=None, stop=True):
    N = prob["N"]
    c, U, V, A, y, dtn = _problem_rows(prob, b, dtype, diag)
    W = len(c)
    bounds = [(a, min(a + L, N)) for a in range(0, N, L)]
    zX, zY = np.zeros((W, W), dtype=dtype), np.zeros(W, dtype=dtype)
    maps, starts, dld, dqd, bad = [], [], [], [], []
    X, Y = zX, zY
    for a, e in bounds:
        nom = fwd_chunk(c, U, V, A, y, dtn, a, e, zX, zY)
        assert not nom["bad"], ("the nominal pass fails", a, nom["bad"])
        tru = fwd_chunk(c, U, V, A, y, dtn, a, e, X, Y, stop=stop)
        maps.append((nom["Phi"], nom["G"], nom["X"], nom["Y"], nom["m"]))
        starts.append((X, Y))
        dld.append(tru["ld"] - nom["ld"])
        dqd.append(tru["qd"] - nom["qd"])
        bad.append(tru["bad"])
        if tru["bad"] and stop:
            break
        X, Y = tru["X"], tru["Y"]
    return dict(maps=maps, starts=starts, dld=dld, dqd=dqd, bad=bad, bounds=bounds, W=W)


@functools.lru_cache(maxsize=None)
def real_maps(Jr, Jc, N, L, b=0, dtype=LD):
    """Problem b of grad_cases.edge_problem(Jr, Jc, N) in chunks of L rows, plain coordinates, everything in
    ``dtype``: dict(maps [(Phi, G, Xbar, Ybar, m)] of the nominal pass (every chunk from the zero state), starts
    [(X, Y)] entering every chunk by the sequential recurrence over the whole series, dld / dqd [per chunk]
    sum log D / sum z^2 / D from the true start minus the same from the zero start, bad [per chunk] the 1-based rows
    of non-positive true pivots (none), bounds, W).  Computed once, shared, never changed."""
    return _maps_of(gc.edge_problem(Jr, Jc, N), b, L, dtype)


#: the edge problems are strongly correlated from row to row (q of a chunk's own rows comes within a few per cent of
#: the whole past's after one row), so the window for a lowered A_r that the chunk's LATER nominal pivots survive is
#: narrow: 1e-4 of q at W = 16
_SHARES = (0.5, 0.25, 0.1, 0.03, 0.01, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5)


@functools.lru_cache(maxsize=None)
def planted_failure(Jr, Jc, nrows, N=197, L=16, chunk=None, b=1):
    """Problem b of edge_problem(Jr, Jc, N) with exactly ``nrows`` (1 or 2) non-positive TRUE pivots, all in chunk
    ``chunk`` (default: 3 for one row; 6 for two, the chunk that holds the gap of the time axis -- the rows of a chunk
    without one are so strongly correlated that no second window opens), whose nominal pass (every chunk from the
    zero state) is healthy.  With q_n = u_n^T S_n u_n the pivot of row n is A_n - q_n, and the true q (the whole
    past) differs from the nominal one (the chunk's own rows): an A_n between the two, A = q (true) - s (the gap),
    keeps the nominal pivot positive and makes the true one negative.  One row: the chunk's first, r (nominal q = 0).
    Two rows: the first pair (n1, n2) of the chunk, in row order, for which that works -- at n2 with the true
    recurrence carried on through the indefinite state n1 left.  s is the largest of 0.5, 0.25, 0.1, ... for which
    the rest of the chunk's nominal pass stays positive and the true pass has one more non-positive pivot.  Returns
    real_maps' dict from the recurrence that does not stop (80 bits; bad = per chunk the 1-based rows of its
    non-positive pivots), with diag (N,) of the problem in float64, chunk, and rows = the 0-based planted rows."""
    chunk = (3 if nrows == 1 else 6) if chunk is None else chunk
    prob = gc.edge_problem(Jr, Jc, N)
    diag = prob["diag"][b].copy()
    add = LD(prob["diag_add"][b])
    c, U, V, A0, y, dtn = _problem_rows(prob, b, LD)
    W, r, e = len(c), chunk * L, min(chunk * L + L, N)
    X0, Y0 = real_maps(Jr, Jc, N, L, b)["starts"][chunk]
    zX, zY = np.zeros((W, W), dtype=LD), np.zeros(W, dtype=LD)

    def q_of(n, X):
        p = np.exp(c * dtn[n])
        return U[n] @ ((p[:, None] * p[None, :] * X) @ U[n])

    def accept(n, a, planted):
        """diag[n] <- a - diag_add (rounded to float64, as the product would be given it) if the chunk then has a
        healthy nominal pass and one non-positive true pivot more than before."""
        trial = diag.copy()
        trial[n] = np.float64(a - add)
        A = trial.astype(LD) + add
        if fwd_chunk(c, U, V, A, y, dtn, r, e, zX, zY)["bad"]:
            return False
        if len(fwd_chunk(c, U, V, A, y, dtn, r, e, X0, Y0, stop=False)["bad"]) != len(planted) + 1:
            return False
        diag[n] = trial[n]
        return True

    def plant(n, planted):
        A = diag.astype(LD) + add
        qt = q_of(n, fwd_chunk(c, U, V, A, y, dtn, r, n, X0, Y0, stop=False)["X"])
        qn = q_of(n, fwd_chunk(c, U, V, A, y, dtn, r, n, zX, zY)["X"])
        return bool(qt > qn) and any(accept(n, qt - s * (qt - qn), planted) for s in _SHARES)

    planted = []
    if nrows == 1:
        assert plant(r, [])
        planted = [r]
    else:
        for n1 in range(r, e):
            keep = diag[n1]
            if plant(n1, []):
                n2 = next((n for n in range(n1 + 1, e) if plant(n, [n1])), None)
                if n2 is not None:
                    planted = [n1, n2]
                    break
            diag[n1] = keep
    assert len(planted) == nrows, planted
    out = _maps_of(prob, b, L, LD, diag=diag, stop=False)
    out.update(diag=diag, rows=planted, chunk=chunk)
    return out


# ---- the device's slots -------------------------------------------------------------------------------------------
def pack_matrices(mats):
    """[len(mats)][4096] float64: element (i, j) of a W x W matrix at j * 64 + i of its slot, zero beyond W."""
    out = np.zeros((len(mats), SLOT, SLOT))
    for s, M in enumerate(mats):
        M = np.asarray(M, dtype=np.float64)
        out[s, :M.shape[1], :M.shape[0]] = M.T
    return out.reshape(len(mats), SLOT * SLOT)


def pack_vectors(vecs):
    """[len(vecs)][64] float64, zero beyond W."""
    out = np.zeros((len(vecs), SLOT))
    for s, v in enumerate(vecs):
        out[s, :len(v)] = np.asarray(v, dtype=np.float64)
    return out


def unpack_matrices(slots, W):
    """(the leading W x W blocks [n][W][W] as matrices (i, j), everything outside them [n][...] flattened)."""
    s = np.asarray(slots).reshape(-1, SLOT, SLOT)
    mask = np.ones((SLOT, SLOT), dtype=bool)
    mask[:W, :W] = False
    return s[:, :W, :W].transpose(0, 2, 1), s[:, mask]
