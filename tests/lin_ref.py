"""TEST INFRASTRUCTURE: the triangular sweeps on the STORED scaled factor (gf_chunk_linear,
gf_chunk_linear_combine[_seg], gf_chunk_segment_transitions, gf_chunk_transition, gf_scaled_propagator) in 80-bit
``np.longdouble``, on the stored rows themselves -- u~, w~ [N][W], d [N], reset spans de [N] (de < 0: no reset; de >= 0: the state is multiplied by
E = exp(-c de) on that row), decay rates c [W] -- so nothing here depends on a factorisation.  The reference of
tests/test_gpu_chunk_linear.py, test_gpu_chunk_linear_combine.py and test_gpu_chunk_transition.py, pinned without a
device by tests/test_lin_ref_host.py.  Never imported by the product.

Every array carries a leading problem axis B (the row loop is Python: B problems share one trip), and every function
takes ``dtype``: the same code in float64 is the "plain float64 restatement" whose error sets the device's bar.

* :func:`sweep` -- the three recurrences of the comment above ``struct LinArgs`` (gadfly_linear.hip) over rows n0 .. n1 - 1
  from a start state: Z, the end state, and the state in front of every chunk boundary it crosses, in the kernels'
  convention (lower / matmul: pending update folded in, the boundary row's own decay NOT yet applied; upper: the
  boundary's decay already applied).
* :func:`local_states` -- every chunk from a zero state: what the local pass leaves in F_state.
* :func:`transitions` -- per chunk Phi, G = sum h h^T / d, m = sum h z / d of the closed-loop recurrence.
* :func:`scan`, :func:`diag_scan`, :func:`chunk_decay`, :func:`segment_transitions` -- the combines.
* :func:`dense_lower` -- L[n, m] = u~_n^T (prod E) w~_m, unit lower triangular: the host tests' independent check.
* :func:`synthetic` -- the random family, one seed per (W, problem).
* :func:`scaled_error`, :func:`pack_states`, :func:`contraction`.
"""
import functools

import numpy as np

LD = np.longdouble
LOWER, UPPER, MATMUL = 0, 1, 2
SLOT = 64


def _decay(c, de, dtype):
    """E [B][W] of one row: exp(-c de) where de >= 0, ones elsewhere."""
    de = np.asarray(de, dtype=dtype)
    return np.where((de >= 0)[:, None], np.exp(-c * np.where(de >= 0, de, 0)[:, None]), dtype(1.0))


def _rows(rows, dtype):
    W = rows["c"].shape[1]
    return (np.asarray(rows["c"], dtype=dtype), np.asarray(rows["Ut"][:, :, :W], dtype=dtype),
            np.asarray(rows["Wt"][:, :, :W], dtype=dtype), np.asarray(rows["d"], dtype=dtype), rows["de"])


def scaled_input(mode, rows, Y, scale, dtype=LD):
    """The sweep's input rows: Y, or with ``scale`` Y / d (solves) or Y sqrt(d) (matmul)."""
    Y = np.asarray(Y, dtype=dtype)
    if not scale:
        return Y
    d = np.asarray(rows["d"], dtype=dtype)[:, :, None]
    return Y * np.sqrt(d) if mode == MATMUL else Y / d


def sweep(mode, rows, Y, L=None, n0=0, n1=None, F0=None, dtype=LD):
    """Rows n0 .. n1 - 1 of problem batch ``rows`` on the (already scaled) input Y [B][N][R], from the state F0
    [B][W][R] (zero if None) -> (Z [B][n1 - n0][R], end state, {chunk c: the state handed to chunk c} for every
    boundary n = c L strictly inside the range).  End state: pending update folded; upper: the decay of row n0 applied
    as well (the state is handed DOWN across that boundary)."""
    c, U, Wt, _, de = _rows(rows, dtype)
    Y = np.asarray(Y, dtype=dtype)
    B, N, R = Y.shape
    n1 = N if n1 is None else n1
    F = np.zeros((B, c.shape[1], R), dtype=dtype) if F0 is None else np.array(F0, dtype=dtype)
    Z = np.zeros((B, n1 - n0, R), dtype=dtype)
    at, carry, tmp = {}, None, np.empty_like(F)

    def push(v):                                    # F += v carry^T (in place: longdouble temporaries set the pace)
        np.multiply(v[:, :, None], carry[:, None, :], out=tmp)
        np.add(F, tmp, out=F)

    def decay(n):
        if np.any(de[:, n] >= 0):
            np.multiply(_decay(c, de[:, n], dtype)[:, :, None], F, out=F)

    def dot(v):
        return (v[:, None, :] @ F)[:, 0]

    if mode == UPPER:
        for n in range(n1 - 1, n0 - 1, -1):
            if n < n1 - 1:
                push(U[:, n + 1])
                decay(n + 1)
                if L and (n + 1) % L == 0:
                    at[(n + 1) // L - 1] = F.copy()
            carry = Y[:, n] - dot(Wt[:, n])
            Z[:, n - n0] = carry
        push(U[:, n0])
        decay(n0)
        return Z, F, at
    for n in range(n0, n1):
        if n > n0:
            push(Wt[:, n - 1])
            if L and n % L == 0:
                at[n // L] = F.copy()
        decay(n)
        Z[:, n - n0] = Y[:, n] + dot(U[:, n]) if mode == MATMUL else Y[:, n] - dot(U[:, n])
        carry = Y[:, n] if mode == MATMUL else Z[:, n - n0]
    push(Wt[:, n1 - 1])
    return Z, F, at


def bounds(N, L):
    return [(a, min(a + L, N)) for a in range(0, N, L)]


def sequential(mode, rows, Y, L, dtype=LD):
    """(Z, starts [nch][B][W][R]) of the UNCHUNKED recurrence over the whole series: starts[c] is the state handed to
    chunk c (zero for the first chunk of the direction)."""
    Z, _, at = sweep(mode, rows, Y, L, dtype=dtype)
    nch = len(bounds(Y.shape[1], L))
    zero = np.zeros((Y.shape[0], rows["c"].shape[1], Y.shape[2]), dtype=dtype)
    return Z, np.array([at.get(c, zero) for c in range(nch)])


def local_states(mode, rows, Y, L, dtype=LD):
    """[nch][B][W][R]: the end state of every chunk swept from a zero state."""
    return np.array([sweep(mode, rows, Y, None, a, e, dtype=dtype)[1] for a, e in bounds(Y.shape[1], L)])


def transitions(rows, L, r=None, dbar=None, zbar=None, dtype=LD):
    """Per chunk (Phi, G, m) [nch][B][W][W], [nch][B][W][W], [nch][B][W] of the closed-loop recurrence on the rows
    u~, r (default w~ d), dbar (default d), zbar (default d), reset spans: Phi = I; per row fold the pending update
    Phi -= (r_{n-1} / d_{n-1}) h_{n-1}^T (nothing where d <= 0), scale the rows by E_n, h_n = Phi^T u~_n;
    G = sum h h^T / d, m = sum h z / d over the rows with d > 0."""
    c, U, Wt, d, de = _rows(rows, dtype)
    dbar = d if dbar is None else np.asarray(dbar, dtype=dtype)
    zbar = dbar if zbar is None else np.asarray(zbar, dtype=dtype)
    r = Wt * d[:, :, None] if r is None else np.asarray(r, dtype=dtype)[:, :, :c.shape[1]]
    B, N, W = U.shape
    out = []
    for a, e in bounds(N, L):
        Phi = np.broadcast_to(np.eye(W, dtype=dtype), (B, W, W)).copy()
        G, m = np.zeros((B, W, W), dtype=dtype), np.zeros((B, W), dtype=dtype)
        pend = None
        for n in range(a, e):
            if pend is not None:
                Phi = Phi - pend
            if np.any(de[:, n] >= 0):
                Phi = _decay(c, de[:, n], dtype)[:, :, None] * Phi
            h = (U[:, n, None, :] @ Phi)[:, 0]
            ok = dbar[:, n] > 0
            rinv = np.where(ok, 1 / np.where(ok, dbar[:, n], 1), 0).astype(dtype)
            G = G + h[:, :, None] * h[:, None, :] * rinv[:, None, None]
            m = m + h * (zbar[:, n] * rinv)[:, None]
            pend = (r[:, n] * rinv[:, None])[:, :, None] * h[:, None, :]
        out.append((Phi - pend, G, m))
    return tuple(np.array([o[k] for o in out]) for k in range(3))


def scan(mode, Phi, loc):
    """Start states [nch][...][W][R] from the local end states: lower F_{c+1} = Fbar_c + Phi_c F_c (ascending), upper
    G_{c-1} = Gbar_c + Phi_c^T G_c (descending).  Phi [nch][...][W][W]."""
    out = np.zeros_like(loc)
    nch = len(loc)
    if mode == UPPER:
        for c in range(nch - 1, 0, -1):
            out[c - 1] = loc[c] + np.swapaxes(Phi[c], -1, -2) @ out[c]
    else:
        for c in range(nch - 1):
            out[c + 1] = loc[c] + Phi[c] @ out[c]
    return out


def diag_scan(D, loc):
    """F_{c+1} = Fbar_c + D_c o F_c: D [nch][...][W], loc [nch][...][W][R]."""
    out = np.zeros_like(loc)
    for c in range(len(loc) - 1):
        out[c + 1] = loc[c] + D[c][..., None] * out[c]
    return out


def chunk_decay(rows, L, dtype=LD):
    """D [nch][B][W] = exp(-c (sum of the spans de > 0 inside the chunk))."""
    c = np.asarray(rows["c"], dtype=dtype)
    de = np.asarray(rows["de"], dtype=dtype)
    return np.array([np.exp(-c * np.sum(np.where(de[:, a:e] > 0, de[:, a:e], 0), axis=1)[:, None])
                     for a, e in bounds(de.shape[1], L)])


def chunk_decay_product(rows, L, dtype=LD):
    """The same D as the product of the chunk's row decays."""
    c = np.asarray(rows["c"], dtype=dtype)
    out = []
    for a, e in bounds(rows["de"].shape[1], L):
        D = np.ones_like(c)
        for n in range(a, e):
            D = D * _decay(c, rows["de"][:, n], dtype)
        out.append(D)
    return np.array(out)


def segment_transitions(Phi, seg_len):
    """Psi_s = Phi_{e-1} ... Phi_b of every segment of seg_len chunks: [nseg][...][W][W]."""
    out = []
    for b in range(0, len(Phi), seg_len):
        P = Phi[b]
        for c in range(b + 1, min(b + seg_len, len(Phi))):
            P = Phi[c] @ P
        out.append(P)
    return np.array(out)


def dense_lower(rows, b=0, dtype=LD):
    """The dense unit lower triangular L [N][N] of problem b: L[n, m] = u~_n^T (prod_{m < k <= n} E_k) w~_m."""
    c, U, Wt, _, de = _rows(rows, dtype)
    N = U.shape[1]
    Lm = np.eye(N, dtype=dtype)
    for m in range(N):
        v = Wt[b, m].copy()
        for n in range(m + 1, N):
            if de[b, n] >= 0:
                v = v * np.exp(-c[b] * dtype(de[b, n]))
            Lm[n, m] = U[b, n] @ v
    return Lm


def scaled_error(got, ref):
    """max |got - ref| / max(1, max |ref|), in 80 bits."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref)) / max(LD(1.0), np.max(np.abs(ref))))


# ---- the synthetic family ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(W, N, B=3, block=16, resets=(), grid=True, key=0):
    """B problems of width W, N rows, float64 (what the device is given): u~, w~ ~ N(0, 0.25 / W) in the leading W of
    64 columns (zero beyond: at this scale the 80-bit lower solve of N = 400 rows stays below 10 max |y|; with
    entries four times larger it reaches 1e73), c ~ U(0.01, 2), d ~ U(0.5, 2); reset rows on the multiples of
    ``block`` (``grid``) and at the rows ``resets``, spans ~ U(0, 1), every fifth (from the second) exactly 0;
    de = -1 elsewhere.  One generator per (W, problem) (and ``key``).  Computed once, shared, never changed."""
    out = dict(c=np.zeros((B, W)), Ut=np.zeros((B, N, SLOT)), Wt=np.zeros((B, N, SLOT)), d=np.zeros((B, N)),
               de=np.full((B, N), -1.0))
    for b in range(B):
        rng = np.random.default_rng([W, b, key])
        out["c"][b] = rng.uniform(0.01, 2.0, W)
        out["Ut"][b, :, :W] = rng.normal(size=(N, W)) * 0.5 / np.sqrt(W)
        out["Wt"][b, :, :W] = rng.normal(size=(N, W)) * 0.5 / np.sqrt(W)
        out["d"][b] = rng.uniform(0.5, 2.0, N)
        at = sorted(set(range(0, N, block) if grid else ()) | set(n for n in resets if n < N))
        span = rng.uniform(0.0, 1.0, len(at))
        span[1::5] = 0.0
        out["de"][b, at] = span
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rhs(W, N, R, B=3, key=0):
    """Y [B][N][R] ~ N(0, 1), float64; the first R' columns of rhs(..., R) are rhs(..., R')."""
    Y = np.stack([np.random.default_rng([W, b, key, 7]).normal(size=(N, 80))[:, :R] for b in range(B)])
    Y.setflags(write=False)
    return Y


def contraction(rng, W, rho=0.9):
    """A random W x W matrix of spectral norm rho."""
    A = rng.normal(size=(W, W))
    return A * (rho / np.linalg.norm(A, 2))


def rows_of_width(W):
    """ROWS = 4 ceil(W / 4): the state rows the sweep kernels carry."""
    return 4 * ((W + 3) // 4)


def pack_maps(M, identity_tail=True):
    """[nch][B][W][W] -> the device's slots [B * nch][4096] (element (i, j) at j * 64 + i), float64.  Beyond the
    leading W x W: zero, and with ``identity_tail`` ones on the diagonal W <= j < ROWS -- what gf_chunk_transition
    writes for Phi (include/gadfly_hip.h)."""
    M = np.asarray(M, dtype=np.float64)
    nch, B, W, _ = M.shape
    out = np.zeros((B, nch, SLOT, SLOT))
    out[:, :, :W, :W] = M.transpose(1, 0, 3, 2)
    if identity_tail:
        for j in range(W, rows_of_width(W)):
            out[:, :, j, j] = 1.0
    return out.reshape(B * nch, SLOT * SLOT)


def unpack_maps(S, B, nch):
    """The device's slots -> full 64 x 64 matrices [nch][B][64][64] as (i, j)."""
    return np.asarray(S).reshape(B, nch, SLOT, SLOT).transpose(1, 0, 3, 2)


def pack_states(F):
    """[nch][B][W][R] -> the device's F_state [B * nch][64 * R] ([i][R] per slot, zero beyond W), float64."""
    F = np.asarray(F, dtype=np.float64)
    nch, B, W, R = F.shape
    out = np.zeros((B, nch, SLOT, R))
    out[:, :, :W] = F.transpose(1, 0, 2, 3)
    return out.reshape(B * nch, SLOT * R)


def unpack_states(S, B, nch, W, R):
    """The device's F_state -> ([nch][B][W][R], the rows >= W [B * nch][64 - W][R])."""
    S = np.asarray(S).reshape(B, nch, SLOT, R)
    return S[:, :, :W].transpose(1, 0, 2, 3), S[:, :, W:].reshape(B * nch, SLOT - W, R)
