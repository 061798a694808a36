"""
Test references of the conditional mean at new times, shared by tests/test_predict_at_host.py and
tests/test_gpu_predict_at_edges.py; in tests/ because oracle/ is frozen.

* :func:`queries` -- the query design of a problem: 150 sorted stamps that hold every way a query can sit among the
  observed rows; :func:`pick` -- M of them.
* :func:`sweeps` -- a numpy restatement of the two sweeps gf_predict_batch_at runs, ``nobs`` / ``nq`` included.
* :func:`oracle_at` -- the yardstick, oracle/seq.predict_mean_at; :func:`dense_at` -- kernel_value(t* - t) @ alpha.
* :func:`reference` -- alpha (oracle/seq.apply_inverse) and the oracle's means of grad_cases.edge_problem(Jr, Jc, N) at
  its query design: computed once, shared, never changed.
"""
import functools

import numpy as np

from oracle import seq
from tests import grad_cases as gc
from tests.grad_ref import rows
from tests.solve_ref import matrices, oracle_predict

#: a single row; two; three; both sides of the 64 rows a lane buffer holds; two full buffers and a bit; the longest
#: length of grad_cases.LENGTHS
LENGTHS = (1, 2, 3, 63, 64, 65, 130, 197)
#: queries per problem of the design: two full output buffers and a third of 22
M_DESIGN = 150
#: what a JD-based axis adds to a zero-based one (BJD 2454833 in the axis' unit of 1 / (0.0864 d))
JD0 = 2454833.0 * 0.0864


def queries(t, seed, M=M_DESIGN):
    """M sorted query stamps for the observed axis t: two equal stamps before the first row; up to 16 stamps equal to
    observed ones; two stamps after the last row; (N >= 2) 70 stamps spanning one observed interval with both ends
    coincident, so that more than 64 queries fall between two rows; uniform random stamps from three cadences before
    the first row to three after the last for the rest."""
    t = np.asarray(t, dtype=np.float64)
    N = len(t)
    rng = np.random.default_rng([seed, N, 77])
    parts = [np.full(2, t[0] - 2.5 * gc.DT), rng.choice(t, size=min(N, 16), replace=False),
             np.array([t[-1] + 0.7 * gc.DT, t[-1] + 40.0 * gc.DT])]
    if N >= 2:
        k = N // 3
        span = np.linspace(t[k], t[k + 1], 70)
        span[0], span[-1] = t[k], t[k + 1]
        parts.append(span)
    have = sum(len(p) for p in parts)
    assert have <= M
    parts.append(rng.uniform(t[0] - 3.0 * gc.DT, t[-1] + 3.0 * gc.DT, M - have))
    return np.sort(np.concatenate(parts))


def pick(M, total=M_DESIGN):
    """Indices of M of the design's queries, spread over all of them (the middle one for M = 1)."""
    if M == 1:
        return np.array([total // 2])
    idx = np.round(np.linspace(0, total - 1, M)).astype(np.int64)
    assert len(np.unique(idx)) == M
    return idx


def sweeps(t, ts, Jr, Jc, co, alpha, nobs=None, nq=None, fill=np.nan):
    """The device's two sweeps for one problem in float64: (M,) means, ``fill`` from ``nq`` on.  ``co`` = (ar, cr, ac,
    bc, cc, dc); only the first ``nobs`` observed rows and the first ``nq`` queries exist."""
    t, ts, alpha = (np.asarray(x, dtype=np.float64) for x in (t, ts, alpha))
    No = len(t) if nobs is None else int(min(max(nobs, 0), len(t)))
    Mq = len(ts) if nq is None else int(min(max(nq, 0), len(ts)))
    c, U, V, _, _ = rows(t[:No], Jr, Jc, *co)
    _, Us, Vs, _, _ = rows(ts[:Mq], Jr, Jc, *co)
    mu = np.full(len(ts), fill)
    # forward: the observed rows at or before each query; the state steps from observed stamp to observed stamp
    F, n, last = np.zeros(len(c)), 0, None
    for m in range(Mq):
        while n < No and t[n] <= ts[m]:
            F = (np.exp(c * (last - t[n])) * F if n else F) + V[n] * alpha[n]
            last = t[n]
            n += 1
        mu[m] = np.sum((Us[m] * np.exp(c * (last - ts[m]))) * F) if n else 0.0
    # backward: the observed rows beyond each query
    H, n, last = np.zeros(len(c)), No - 1, None
    for m in range(Mq - 1, -1, -1):
        while n >= 0 and t[n] > ts[m]:
            H = (np.exp(c * (t[n] - last)) * H if n < No - 1 else H) + U[n] * alpha[n]
            last = t[n]
            n -= 1
        if n < No - 1:
            mu[m] += np.sum((Vs[m] * np.exp(c * (ts[m] - last))) * H)
    return mu


def oracle_at(t, ts, co, alpha, dtype=np.float64):
    """oracle/seq.predict_mean_at for (ar, cr, ac, bc, cc, dc) of any structure."""
    c, U, V = matrices(t, co, dtype)
    _, Us, Vs = matrices(ts, co, dtype)
    return seq.predict_mean_at(np.asarray(t, dtype=dtype), c, U, V, np.asarray(alpha, dtype=dtype),
                               np.asarray(ts, dtype=dtype), Us, Vs)


def dense_at(t, ts, co, alpha):
    """kernel_value(t* - t) @ alpha with the kernel of the six coefficient vectors."""
    ar, cr, ac, bc, cc, dc = (np.asarray(x, dtype=np.float64) for x in co)
    tau = np.abs(np.asarray(ts, dtype=np.float64)[:, None] - np.asarray(t, dtype=np.float64)[None, :])[:, :, None]
    K = np.sum(ar * np.exp(-cr * tau), axis=2)
    K = K + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=2)
    return K @ np.asarray(alpha, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def reference(Jr, Jc, N, jd=False):
    """dict(prob, ts (B, M_DESIGN), alpha (B, N), mu (B, M_DESIGN)) for grad_cases.edge_problem(Jr, Jc, N), on the
    JD-based axis t + JD0 with ``jd``: alpha from oracle/seq.py's factor and apply_inverse, a query design per problem,
    mu from oracle/seq.predict_mean_at, all float64."""
    prob = dict(gc.edge_problem(Jr, Jc, N))
    if jd:
        prob["t"] = prob["t"] + JD0
    B = prob["B"]
    ts = np.stack([queries(prob["t"], b) for b in range(B)])
    alpha, mu = np.empty((B, N)), np.empty((B, M_DESIGN))
    for b in range(B):
        co = gc.coefficients(prob, b)
        sol = oracle_predict(prob["t"], prob["y"][b], prob["diag"][b], co, prob["diag_add"][b])
        assert sol["info"] == 0
        alpha[b] = sol["alpha"]
        mu[b] = oracle_at(prob["t"], ts[b], co, alpha[b])
    for x in (ts, alpha, mu):
        x.setflags(write=False)
    return dict(prob=prob, ts=ts, alpha=alpha, mu=mu)
