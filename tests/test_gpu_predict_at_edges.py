"""GPU: gf_predict_batch_at through its raw C entry point at the shapes where it can go wrong -- every structure of
tests/grad_cases.py, every length of predict_at_ref.LENGTHS (both sides of the 64 rows a lane buffer holds), the query
design of predict_at_ref.queries (equal stamps, coincident stamps, queries outside the data, more than 64 queries
between two rows), M = 1, 64, 65, 150 -- against oracle/seq.predict_mean_at in float64.  alpha is the oracle's
(seq.apply_inverse), so only this kernel is under test.  Its calling conventions (strides, nobs / nq, output bounds),
bit identity across batches and query sets, a NaN alpha, a JD-based axis, its argument checks."""
import numpy as np
import pytest
import torch

from tests import grad_cases as gc
from tests import predict_at_ref as pr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77                  # what the output holds before a call: no result of these problems
BAR = 1e-9                           # of max |reference| per problem: the bar of tests/test_gpu_predict_edges.py


def _dev(x, dtype=np.float64):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C")).cuda()      # (a copy: references are read-only)


def _bs(a):
    """Batch stride in elements of a host array: 0 for a shared 1-D one, the row length of a (B, S) one."""
    return 0 if a.ndim == 1 else a.shape[1]


def at_call(hip, Jr, Jc, real, comp, t, ts, alpha, N, M, nobs=None, nq=None):
    """One gf_predict_batch_at call on host arrays: real (2, B, max(Jr, 1)), comp (4, B, max(Jc, 1)); t (N,) shared or
    (B, S >= N); ts (M,) shared or (B, S >= M); alpha (B, S >= N); nobs, nq (B,) or None (NULL).  The output is
    allocated one problem and one row too long (mu_bs = M + 1) and pre-filled with a sentinel that must survive beyond
    nq[b] (M without nq) in every row and in all of row B.  Returns mu (B, M), the sentinel still in it from nq[b] on."""
    lib, p = hip.load(), hip.ptr
    B = real.shape[1]
    assert real.shape == (2, B, max(Jr, 1)) and comp.shape == (4, B, max(Jc, 1)) and alpha.shape[0] == B
    rd, cd, td, qd, ad = _dev(real), _dev(comp), _dev(t), _dev(ts), _dev(alpha)
    nod = None if nobs is None else _dev(nobs, np.int64)
    nqd = None if nq is None else _dev(nq, np.int64)
    mu = torch.full((B + 1, M + 1), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.gf_predict_batch_at(B, N, M, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]),
                                 p(td), _bs(t), p(nod), p(qd), _bs(ts), p(nqd), p(ad), alpha.shape[1], p(mu), M + 1,
                                 None)
    hip.check(rc, "gf_predict_batch_at")
    torch.cuda.synchronize()
    out = mu.cpu().numpy()
    assert np.all(out[B] == SENTINEL) and np.all(out[:, M] == SENTINEL)
    for b in range(B):
        keep = M if nq is None else int(min(max(nq[b], 0), M))
        assert np.all(out[b, keep:] == SENTINEL), b
        assert not np.any(out[b, :keep] == SENTINEL), b
    return out[:B, :M]


def _errs(got, ref):
    return [float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got, ref)]


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_edge_shapes_match_the_oracle(hip, Jr, Jc):
    """B = 3 problems of different coefficients, alpha and query designs on a shared observed axis at every length:
    within 1e-9 of max |reference| per problem of oracle/seq.py in float64; every problem alone gives the same bits."""
    bad, worst = [], 0.0
    for N in pr.LENGTHS:
        ref = pr.reference(Jr, Jc, N)
        prob = ref["prob"]
        base = at_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ref["ts"], ref["alpha"], N, pr.M_DESIGN)
        for b, e in enumerate(_errs(base, ref["mu"])):
            worst = max(worst, e)
            if not e <= BAR:
                bad.append((N, b, e))
        for b in range(prob["B"]):
            one = at_call(hip, Jr, Jc, prob["real"][:, b:b + 1], prob["comp"][:, b:b + 1], prob["t"],
                          ref["ts"][b:b + 1], ref["alpha"][b:b + 1], N, pr.M_DESIGN)
            assert np.array_equal(one[0], base[b]), (N, b)
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: worst error against oracle/seq.py {worst:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", [(0, 1), (1, 8), (3, 30)])
def test_query_counts_and_query_independence(hip, Jr, Jc):
    """M = 1, 64, 65 of the design's 150 queries: the oracle's values at those queries within the bar, and the same
    bits as the same queries among all 150 (a query alone in the call at M = 1)."""
    for N in (1, 64, 197):
        ref = pr.reference(Jr, Jc, N)
        prob = ref["prob"]
        args = (hip, Jr, Jc, prob["real"], prob["comp"], prob["t"])
        full = at_call(*args, ref["ts"], ref["alpha"], N, pr.M_DESIGN)
        for M in (1, 64, 65, 150):
            idx = pr.pick(M)
            got = at_call(*args, ref["ts"][:, idx], ref["alpha"], N, M)
            assert np.array_equal(got, full[:, idx]), (N, M)
            scale = np.max(np.abs(ref["mu"]), axis=1, keepdims=True)       # (of the whole design: M = 1 may hit a zero)
            assert np.all(np.abs(got - ref["mu"][:, idx]) <= BAR * scale), (N, M)


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (1, 16), (1, 31)])
def test_strides_shared_and_per_problem_axes(hip, Jr, Jc):
    """Shared t and ts (stride 0) against B copies at strides of N + 3 and M + 5, alpha at a stride of N + 2, the pad
    elements NaN: never read.  Then axes that really differ per problem against the oracle."""
    for N in (3, 65, 130):
        ref = pr.reference(Jr, Jc, N)
        prob = ref["prob"]
        B, M = prob["B"], pr.M_DESIGN
        t, ts, alpha = prob["t"], ref["ts"][0], ref["alpha"]
        base = at_call(hip, Jr, Jc, prob["real"], prob["comp"], t, ts, alpha, N, M)
        wide_t, wide_q, wide_a = np.full((B, N + 3), np.nan), np.full((B, M + 5), np.nan), np.full((B, N + 2), np.nan)
        wide_t[:, :N], wide_q[:, :M], wide_a[:, :N] = t, ts, alpha
        for tt in (t, wide_t):
            for qq in (ts, wide_q):
                got = at_call(hip, Jr, Jc, prob["real"], prob["comp"], tt, qq, wide_a, N, M)
                assert np.array_equal(got, base), (N, tt.shape, qq.shape)
        # every problem on its own observed axis (the shared one, stretched) with its own queries
        tb = np.stack([t * (1.0 + 0.05 * b) for b in range(B)])
        qb = np.stack([pr.queries(tb[b], 10 + b) for b in range(B)])
        got = at_call(hip, Jr, Jc, prob["real"], prob["comp"], tb, qb, alpha, N, M)
        want = [pr.oracle_at(tb[b], qb[b], gc.coefficients(prob, b), alpha[b]) for b in range(B)]
        assert all(e <= BAR for e in _errs(got, want)), (N, _errs(got, want))


@pytest.mark.parametrize("Jr,Jc", [(0, 8), (2, 15), (0, 31)])
def test_counts_give_the_shorter_problem_to_the_bit(hip, Jr, Jc):
    """nobs / nq that differ per problem, nobs = 1 and nq = 0 among them, clamped where they exceed N / M: the bits of
    the same problem called alone at those lengths; t and alpha from nobs[b] on and ts from nq[b] on are NaN (never
    read), the output from nq[b] on keeps its sentinel (at_call)."""
    N, M = 130, pr.M_DESIGN
    ref = pr.reference(Jr, Jc, N)
    prob = ref["prob"]
    B = prob["B"]
    for nobs, nq in (((1, 64, 130), (150, 65, 0)), ((65, 129, 1), (1, 64, 150)), ((500, 63, 2), (149, 500, 3))):
        no, mq = np.minimum(nobs, N), np.minimum(nq, M)
        tb, qb, ab = np.tile(prob["t"], (B, 1)), ref["ts"].copy(), ref["alpha"].copy()
        for b in range(B):
            tb[b, no[b]:], ab[b, no[b]:], qb[b, mq[b]:] = np.nan, np.nan, np.nan
        got = at_call(hip, Jr, Jc, prob["real"], prob["comp"], tb, qb, ab, N, M, nobs=np.array(nobs),
                      nq=np.array(nq))
        for b in range(B):
            if mq[b] == 0:
                continue
            one = at_call(hip, Jr, Jc, prob["real"][:, b:b + 1], prob["comp"][:, b:b + 1], prob["t"][:no[b]],
                          ref["ts"][b:b + 1, :mq[b]], ref["alpha"][b:b + 1, :no[b]], int(no[b]), int(mq[b]))
            assert np.array_equal(got[b, :mq[b]], one[0]), (nobs, nq, b)
            want = pr.oracle_at(prob["t"][:no[b]], ref["ts"][b, :mq[b]], gc.coefficients(prob, b),
                                ref["alpha"][b, :no[b]])
            assert np.max(np.abs(one[0] - want)) <= BAR * np.max(np.abs(want)), (nobs, nq, b)
    # only nobs, only nq
    full = at_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ref["ts"], ref["alpha"], N, M)
    got = at_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ref["ts"], ref["alpha"], N, M,
                  nq=np.array([150, 7, 66]))
    assert all(np.array_equal(got[b, :k], full[b, :k]) for b, k in enumerate((150, 7, 66)))
    got = at_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ref["ts"], ref["alpha"], N, M,
                  nobs=np.array([130, 130, 130]))
    assert np.array_equal(got, full)


def test_nan_alpha_stays_in_its_problem(hip):
    """alpha of a problem gf_solve_batch could not factor is NaN in every row: so is every mean of that problem, the
    queries before the first and after the last row included; its neighbours keep their bits."""
    Jr, Jc, N = 1, 16, 65
    ref = pr.reference(Jr, Jc, N)
    prob = ref["prob"]
    args = (hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ref["ts"])
    base = at_call(*args, ref["alpha"], N, pr.M_DESIGN)
    alpha = ref["alpha"].copy()
    alpha[1] = np.nan
    got = at_call(*args, alpha, N, pr.M_DESIGN)
    assert np.all(np.isnan(got[1])) and np.array_equal(got[[0, 2]], base[[0, 2]])


@pytest.mark.parametrize("Jr,Jc", [(1, 16)])
def test_jd_based_axis(hip, Jr, Jc):
    """t + 2454833 d (phases of ~3e8 rad): the float64 oracle, which rounds the same phases fl(d t), at the same bar."""
    for N in (65, 197):
        ref = pr.reference(Jr, Jc, N, jd=True)
        prob = ref["prob"]
        got = at_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ref["ts"], ref["alpha"], N, pr.M_DESIGN)
        e = _errs(got, ref["mu"])
        print(f"JD axis, N = {N}: {max(e):.1e}")
        assert all(x <= BAR for x in e), (N, e)


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    N, M, B = 50, 40, 2
    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")      # noqa: E731
    real, comp, t, ts, alpha = f(2, B, 1), f(4, B, 32), f(N), f(M), f(B, N)
    mu = torch.full((B, M), SENTINEL, dtype=torch.float64, device="cuda")

    def call(N=N, M=M, Jc=8, t=p(t), ts=p(ts), alpha=p(alpha), out=p(mu), alpha_bs=N, mu_bs=M, B=B):
        c = [p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]), p(comp[3])]
        return lib.gf_predict_batch_at(B, N, M, 0, Jc, *c, t, 0, None, ts, 0, None, alpha, alpha_bs, out, mu_bs, None)

    assert call(Jc=32) == -3 and "63" in hip.last_error()                                 # W = 64
    for kw in (dict(M=0), dict(N=0), dict(B=0), dict(Jc=0), dict(ts=None), dict(t=None), dict(alpha=None),
               dict(out=None), dict(mu_bs=M - 1), dict(alpha_bs=N - 1)):
        assert call(**kw) == -1, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert bool(torch.all(mu == SENTINEL))
    assert call() == 0                                                                   # the same arguments, whole
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(mu))) and not bool(torch.any(mu == SENTINEL))
