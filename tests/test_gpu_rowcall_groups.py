"""GPU: a problem's result does not depend on the group it lands in, for every grouped one-wave call of
BatchedLogLikelihood (gf_solve_batch, gf_var_batch with and without queries, gf_loglike_grad; DESIGN.md 3.7, 3.9,
3.11, 3.12).  Each call runs once with the whole batch in one group and once under a workspace cap of two problems
(B = 5: groups of 2, 2, 1); every array that comes back, the log-likelihoods and ``info`` must have the same bits.
The queries, their counts and the observed-row counts differ from problem to problem, so a group that reads another
group's rows of any of them gives other numbers."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.synth import uniform_times
from gadfly_amd.terms import SHOTerm, TermSum

pytestmark = pytest.mark.gpu

B, N, M = 5, 130, 65
ROWS = (130, 97, 64, 65, 3)          # padded N = 130: two full runs of 64 rows and a tail of two
NQ = (65, 1, 64, 33, 17)
CAD = 180.0
DT = CAD * 1e-6
YERR = 30.0
MEAN = np.array([2.5, -1.0, 4.0, 0.5, -3.0])


def _kernels():
    """Two SHO terms per problem, the first overdamped (two real terms), the second underdamped (one complex term):
    W = 4, other parameters in every problem."""
    rng = np.random.default_rng(5)
    f = np.exp(0.1 * rng.normal(size=(B, 4)))
    return [TermSum(SHOTerm(S0=50.0 * a, w0=2000.0 * b, Q=0.3), SHOTerm(S0=1.0 * c, w0=12000.0 * d, Q=4.0))
            for a, b, c, d in f]


def _queries(rng, t, m):
    """m ascending stamps around one series, the first before its first stamp and the last after its last one (a single
    query: after the last)."""
    q = np.sort(rng.uniform(t[0], t[-1], m))
    q[-1] = t[-1] + 7.5 * DT
    if m > 1:
        q[0] = t[0] - 5.5 * DT
    return q


def _ragged():
    rng = np.random.default_rng(11)
    ts = [uniform_times(n, CAD) + 3.0 * DT * b for b, n in enumerate(ROWS)]
    ys = [100.0 * rng.normal(size=n) + m for n, m in zip(ROWS, MEAN)]
    ev = gadfly_amd.BatchedLogLikelihood(_kernels(), ts, ys, yerr=YERR, mean=MEAN)
    return ev, [_queries(rng, t, m) for t, m in zip(ts, NQ)], _queries(rng, ts[0], M)


def _rectangular():
    rng = np.random.default_rng(13)
    t = uniform_times(N, CAD)
    ts = np.stack([t + 3.0 * DT * b for b in range(B)])
    ys = 100.0 * rng.normal(size=(B, N)) + MEAN[:, None]
    ev = gadfly_amd.BatchedLogLikelihood(_kernels(), ts, ys, yerr=YERR, mean=MEAN[:, None])
    return ev, np.stack([_queries(rng, x, M) for x in ts]), _queries(rng, t, M)


def _predict(t=None, **kw):
    """A predict_device call as (cap attribute, plan attribute, function of (evaluator, per-problem queries, shared
    queries) -> everything the call leaves behind); ``t``: None, "own" or "shared"."""
    def run(ev, queries, shared):
        at = {} if t is None else dict(t=queries if t == "own" else shared)
        out = ev.predict_device(**kw, **at)
        return list(out if isinstance(out, tuple) else (out,)) + [ev.last_predict_ll, ev.last_predict_info]
    return "predict_workspace_bytes", "last_predict_plan", run


def _loo(ev, queries, shared):
    return list(ev.leave_one_out_device()) + [ev.last_predict_ll, ev.last_predict_info]


def _grad(ev, queries, shared):
    ll, g = ev.value_and_grad_coefficients(_kernels())
    return [ll] + [g[k] for k in ("real", "comp", "diag_add", "mean")]


CALLS = {
    "var_alpha": lambda: _predict(return_var=True, return_alpha=True),
    "var_alpha_at_own": lambda: _predict(t="own", return_var=True, return_alpha=True),
    "alpha_at_own": lambda: _predict(t="own", return_alpha=True),
    "var_at_shared": lambda: _predict(t="shared", return_var=True),
    "inverse_diagonal": lambda: ("predict_workspace_bytes", "last_predict_plan", lambda ev, q, s: [
        ev.inverse_diagonal_device(), ev.last_predict_ll, ev.last_predict_info]),
    "leave_one_out": lambda: ("predict_workspace_bytes", "last_predict_plan", _loo),
    "grad_coefficients": lambda: ("grad_workspace_bytes", "last_grad_plan", _grad),
}


def _host(x):
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _same(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("batch", ["ragged", "rectangular"])
def test_groups_of_two_give_the_bits_of_one_group(batch, call):
    ev, queries, shared = _ragged() if batch == "ragged" else _rectangular()
    cap, plan, run = CALLS[call]()
    whole = _host(run(ev, queries, shared))
    nbytes, groups, size = getattr(ev, plan)
    assert (groups, size) == (1, B)
    assert all(np.all(np.isfinite(x)) for x in whole[-2:])          # (log L and info, or the last two gradients)
    setattr(ev, cap, 2 * (nbytes // B))
    grouped = _host(run(ev, queries, shared))
    assert getattr(ev, plan)[1:] == (3, 2)
    assert len(whole) == len(grouped)
    for i, (a, b) in enumerate(zip(whole, grouped)):
        assert _same(a, b), (batch, call, i)
    if batch == "ragged" and "own" in call:                          # a list of queries: cut to each problem's own
        assert [len(x) for x in whole[0]] == list(NQ)
