"""Edge cases of the generic sweep kernels (gf_build_matrices, gf_factor, gf_solve, gf_solve_chunk[_rhs],
gf_chunk_diag_scan, gf_general_matmul), shared by tests/test_sweep_cases_host.py and the GPU modules
test_gpu_sweep_edges.py, test_gpu_solve_chunk_edges.py and test_gpu_general_matmul_edges.py.  Host only: numpy and
the oracle, no device import.

Problems are tests.grad_cases.edge_problem with the matrices built from its ``diag`` alone (a = diag + sum of the
amplitudes, no further shift): conditions max(a) / min(d) of about 16.  References are oracle/cref.py in float64
(factor, the three sweeps, the conditional mean) and oracle/seq.py for the matrix build."""
import functools

import numpy as np

from oracle import cref, seq
from tests import grad_cases as gc

#: max-norm error relative to the largest reference entry of the array: every comparison of d, W, z, Z, mu and the
#: chunk states.  The float64 C oracle sits within 1.6e-14 of the 80-bit recurrence on these problems
#: (test_sweep_cases_host.py pins it), the kernels are expected at about 1e-12.
TOL = 1e-10

#: (Jr, Jc): W = 1, 2, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 255, 256, 256 -- both sides of
#: every line of dispatch_factor, launch_solve_rhs, launch_solve_vec and the CT choice of gf_general_matmul
STRUCTURES = ((1, 0), (0, 1), (0, 8), (1, 8), (0, 16), (3, 15), (0, 24), (1, 24), (0, 32), (1, 32), (0, 48), (1, 48),
              (0, 64), (1, 64), (0, 96), (1, 96), (3, 126), (0, 128), (256, 0))
#: rows against the depth-8 register rings of the sweeps (k_solve_vec, k_solve_rhs: DEPTH; k_gmm: GB)
LENGTHS = (1, 2, 7, 8, 9, 16, 17, 70)

LOWER, UPPER, MATMUL = 0, 1, 2          # the GF_* modes of include/gadfly_hip.h


def structure_of(W):
    """The first structure of STRUCTURES with width W."""
    return next(s for s in STRUCTURES if s[0] + 2 * s[1] == W)


def leading_dim(W):
    return (W + 15) // 16 * 16


def pad(X, ld, fill=0.0):
    """(N, W) -> (N, ld) with ``fill`` in the pad columns."""
    out = np.full((X.shape[0], ld), fill, dtype=np.float64)
    out[:, :X.shape[1]] = X
    return out


def relerr(got, ref):
    """max |got - ref| / max |ref| (NaN or Inf in ``got`` gives inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


def propagator(t, c):
    """P[n][j] = exp(c_j (t[n-1] - t[n])), row 0 = 1."""
    P = np.ones((len(t), len(c)))
    P[1:] = np.exp(c[None, :] * (t[:-1] - t[1:])[:, None])
    return P


@functools.lru_cache(maxsize=None)
def reference(Jr, Jc, N, B=3, own_axes=False):
    """The B problems of grad_cases.edge_problem(Jr, Jc, N, B) through the float64 oracle, computed once and shared
    (never changed: the arrays are read-only).  ``own_axes``: problem b lives on the axis t (1 + b / 64) instead of
    the shared one.  Tuple of dicts: co (six coefficient arrays), t, diag, y, c, a, U, V, P, d, W, info, z."""
    prob = gc.edge_problem(Jr, Jc, N, B)
    out = []
    for b in range(B):
        co = gc.coefficients(prob, b)
        t = prob["t"] * (1.0 + b / 64.0) if own_axes else prob["t"]
        c, a, U, V = seq.celerite_matrices(co, t, prob["diag"][b])
        d, Wm, info = cref.factor(t, c, a, U, V)
        r = dict(co=co, t=t, diag=prob["diag"][b], y=prob["y"][b], c=c, a=a, U=U, V=V, P=propagator(t, c), d=d,
                 W=Wm, info=info, diag_add=prob["diag_add"][b])
        r["z"] = cref.solve_lower(t, c, U, Wm, r["y"]) if info == 0 else None
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return tuple(out)


def rhs(N, R, seed=0):
    """(N, R) right-hand sides of unit scale."""
    return np.random.default_rng([seed, N, R]).normal(size=(N, R))


def sweep_reference(mode, ref, Y, scaled):
    """The oracle's Z (N, R) of one problem of ``reference`` for the mode and the per-row scale d (1 / d before the
    solves, sqrt(d) before the product), as gf_solve applies it."""
    t, c, U, Wm, d = ref["t"], ref["c"], ref["U"], ref["W"], ref["d"]
    Y = carried_input(mode, ref, Y, scaled)
    if mode == LOWER:
        return cref.solve_lower(t, c, U, Wm, Y)
    if mode == UPPER:
        return cref.solve_upper(t, c, U, Wm, Y)
    return cref.matmul_lower(t, c, U, Wm, Y)


def carried_input(mode, ref, Y, scaled):
    Y = np.asarray(Y, dtype=np.float64).reshape(len(ref["t"]), -1)
    if not scaled:
        return Y
    return Y * np.sqrt(ref["d"])[:, None] if mode == MATMUL else Y / ref["d"][:, None]


# ---- chunk mode of the sweeps ------------------------------------------------------------------------------------
# Convention of the kernels (SolveArgs and k_solve_vec in gadfly_stored.hip): the state of slot (problem, chunk) holds the
# pending push of the row before the chunk folded in; ascending sweeps (LOWER, MATMUL) apply the decay of the boundary
# on ENTRY, at the chunk's first row; the descending sweep (UPPER) applies it on EXIT, across its own first row.

def chunks_of(N, chunk_len):
    """[(a, e)]: rows [a, e) of every chunk."""
    return [(a, min(a + chunk_len, N)) for a in range(0, N, chunk_len)]


def true_chunk_states(mode, ref, Yin, Z, chunk_len):
    """True start state of every chunk and the state each chunk must leave, from the oracle's sequential sweep:
    ``Yin`` (N, R) the (scaled) input rows, ``Z`` (N, R) the oracle's result.  Returns (start, end), each
    (nch, W, R); one right-hand side is R = 1.  end[k] is what the next chunk in sweep direction starts from."""
    P, N = ref["P"], len(ref["t"])
    push = ref["U"] if mode == UPPER else ref["W"]
    carry = (Yin if mode == MATMUL else Z).reshape(N, -1)
    Wd, R = push.shape[1], carry.shape[1]
    G = np.zeros((N, Wd, R))            # state after row n in sweep order: push of row n folded
    F = np.zeros((Wd, R))
    if mode == UPPER:                   # ... and decayed across the boundary n-1 | n
        for n in range(N - 1, -1, -1):
            G[n] = P[n][:, None] * (F + np.outer(push[n], carry[n]))
            F = G[n]
    else:                               # ... not yet decayed
        for n in range(N):
            G[n] = P[n][:, None] * F + np.outer(push[n], carry[n])
            F = G[n]
    ch = chunks_of(N, chunk_len)
    zero = np.zeros((Wd, R))
    if mode == UPPER:
        start = [G[e] if e < N else zero for a, e in ch]
        end = [G[a] for a, e in ch]
    else:
        start = [G[a - 1] if a > 0 else zero for a, e in ch]
        end = [G[e - 1] for a, e in ch]
    return np.array(start), np.array(end)


def chunk_sweep(mode, ref, Yin, a, e, start):
    """One chunk [a, e) swept in numpy as the kernels do it, from the state ``start`` (W, R): (Z rows (e - a, R),
    end state (W, R))."""
    P, U, Wm = ref["P"], ref["U"], ref["W"]
    Yin = Yin.reshape(len(ref["t"]), -1)
    F = np.array(start, dtype=np.float64)
    Z = np.empty((e - a, Yin.shape[1]))
    carry = None
    if mode == UPPER:
        for n in range(e - 1, a - 1, -1):
            if n < e - 1:
                F = P[n + 1][:, None] * (F + np.outer(U[n + 1], carry))
            carry = Z[n - a] = Yin[n] - Wm[n] @ F
        return Z, P[a][:, None] * (F + np.outer(U[a], carry))
    for n in range(a, e):
        F = P[n][:, None] * (F if n == a else F + np.outer(Wm[n - 1], carry))
        dot = U[n] @ F
        Z[n - a] = Yin[n] + dot if mode == MATMUL else Yin[n] - dot
        carry = Yin[n] if mode == MATMUL else Z[n - a]
    return Z, F + np.outer(Wm[e - 1], carry)


def chunk_decays(ref, chunk_len):
    """D (nch, W): the product of each chunk's propagator rows (gf_chunk_diag_scan's transitions)."""
    return np.array([np.prod(ref["P"][a:e], axis=0) for a, e in chunks_of(len(ref["t"]), chunk_len)])


def diag_scan(D, loc):
    """numpy form of gf_chunk_diag_scan: D (nch, rows), loc (nch, rows, R) local end states -> true start states."""
    out = np.zeros_like(loc)
    for k in range(1, len(loc)):
        out[k] = loc[k - 1] + D[k - 1][:, None] * out[k - 1]
    return out


# ---- conditional mean ----------------------------------------------------------------------------------------------

def gmm_chunking(B, N):
    """(nch, chunk_len) gf_general_matmul picks: about N / 256 chunks, at most 1024 / B, at least one."""
    n = max(1, min(N // 256, max(1024 // B, 1)))
    length = (N + n - 1) // n
    return (N + length - 1) // length, length


def gmm_work(B, M, N, W):
    """gf_general_matmul_work restated."""
    nch, _ = gmm_chunking(B, N)
    CT = 1 if W <= 64 else 2 if W <= 128 else 4
    return B * 2 * M + (3 * B * 2 * nch * CT * 64 if nch > 1 else 0)


def qidx_of(t2, t1):
    """Number of observed rows with t2 <= t1[m]."""
    return np.searchsorted(t2, t1, side="right").astype(np.int64)


QUERY_SETS = ("full", "all_before", "all_after", "one_chunk_only", "M1")


def query_set(name, t, B):
    """Sorted query times on the observed axis t (N,) for the chunking gf_general_matmul picks with B problems.
    full: before t[0], exactly t[0], exactly t[N-1], after t[N-1]; exactly on the last row of chunk k and on the first
    row of chunk k + 1 and strictly between them, for every boundary; one query three times.  all_before / all_after:
    three queries outside the data on one side.  one_chunk_only: every query strictly inside chunk 1 (the only chunk
    when there is one), so every other chunk returns early.  M1: a single query between two rows."""
    N = len(t)
    step = gc.DT if N < 2 else float(np.min(np.diff(t)))
    nch, L = gmm_chunking(B, N)
    if name == "all_before":
        return t[0] - step * np.array([40.0, 2.5, 0.5])
    if name == "all_after":
        return t[-1] + step * np.array([0.5, 2.5, 40.0])
    if name == "M1":
        return np.array([t[N // 3] + 0.5 * step])
    if name == "one_chunk_only":
        a, e = chunks_of(N, L)[min(1, nch - 1)]
        rows = sorted(set(r for r in (a, a + 1, (a + e) // 2, e - 3, e - 2) if a <= r <= e - 2))
        if not rows:                    # a chunk of one row: on the row itself
            return np.array([t[a]])
        return np.array([0.5 * (t[r] + t[r + 1]) for r in rows])
    assert name == "full", name
    q = [t[0] - 3.0 * step, t[0] - 0.5 * step, t[0], t[-1], t[-1] + 0.5 * step, t[-1] + 3.0 * step]
    for a, e in chunks_of(N, L)[:-1]:
        q += [t[e - 1], 0.5 * (t[e - 1] + t[e]), t[e]]
    rep = t[(2 * N) // 3] + 0.25 * step
    return np.sort(np.array(q + [rep, rep, rep]))


def general_matmul_reference(ref, t1, alpha):
    """cref.general_matmul of one problem of ``reference`` at the query times t1, with the query-side rows."""
    _, _, U1, V1 = seq.celerite_matrices(ref["co"], t1, np.zeros(len(t1)))
    return cref.general_matmul(t1, ref["t"], ref["c"], U1, V1, ref["U"], ref["V"], alpha), U1, V1
