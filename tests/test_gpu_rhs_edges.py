"""GPU: gf_solve_batch_rhs and gf_predict_batch_at_rhs through their raw C entry points -- every
instance of the solve kernel and both sides of each instance boundary, lengths around the 64-row output blocks, the
library's segment length and 16 rows, right-hand-side counts around the block RB a wave carries.  Column r of every
output against gf_solve_batch / gf_predict_batch_at on that column alone, BIT FOR BIT (tests/test_gpu_predict_edges.py's
and tests/test_gpu_predict_at_edges.py's callers), and against oracle/seq.py in float64 within 1e-9 of max |reference|
per problem.  A problem that is not positive definite between two good ones; the argument checks."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import seq
from tests import grad_cases as gc
from tests.solve_ref import matrices
from tests.test_gpu_predict_at_edges import at_call
from tests.test_gpu_predict_edges import solve_call

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
INFO_SENTINEL = -77
BAR = 1e-9                           # of max |reference| per problem: the bar of tests/test_gpu_predict_edges.py
#: W = 1, 2, 16, 16, 17, 32, 63, 63: k_solve_rhs<16>, <32>, <64> and both sides of each boundary
STRUCTURES = ((1, 0), (0, 1), (2, 7), (0, 8), (1, 8), (0, 16), (1, 31), (3, 30))
LENGTHS = (1, 2, 3, 17, 64, 65, 197)
QUERIES = (0, 1, 63, 64, 65, 130)
B = 3


def _dev(x, dtype=np.float64):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C")).cuda()


def rhs_counts(RB):
    return sorted({r for r in (1, 2, RB - 1, RB, RB + 1, 2 * RB + 1) if r >= 1})


@functools.lru_cache(maxsize=None)
def problem(Jr, Jc, N, R):
    """grad_cases.edge_problem's B = 3 kernels and per-row diagonals on per-problem axes (the shared axis stretched by
    2 % per problem), with R right-hand sides per problem of the data's scale."""
    prob = dict(gc.edge_problem(Jr, Jc, N))
    rng = np.random.default_rng([7, Jr, Jc, N])
    prob["t"] = prob["t"][None, :] * (1.0 + 0.02 * np.arange(B))[:, None]
    prob["Y"] = np.sqrt(prob["diag_add"])[:, None, None] * rng.normal(size=(B, R, N))
    return prob


def solve_rhs_call(hip, prob, Y, seg=0, alpha=True, mu=True):
    """One gf_solve_batch_rhs call: Y (B, R, N).  Outputs one problem too long, sentinel beyond."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, N = prob["Jr"], prob["Jc"], prob["N"]
    nb, R = Y.shape[0], Y.shape[1]
    per = int(lib.gf_solve_batch_rhs_work(N, Jr + 2 * Jc, R, seg))
    assert per > 0
    work = torch.full((nb * per,), float("nan"), dtype=torch.float64, device="cuda")
    rd, cd, ad = _dev(prob["real"]), _dev(prob["comp"]), _dev(prob["diag_add"])
    td, dd, yd = _dev(prob["t"]), _dev(prob["diag"]), _dev(Y)
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    a = f((nb + 1) * R * N) if alpha else None
    m = f((nb + 1) * R * N) if mu else None
    ll = f((nb + 1) * R)
    info = torch.full((nb + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_solve_batch_rhs(nb, N, R, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                                p(td), N, p(dd), N, p(yd), R * N, N, seg, p(work), per, p(a), p(m), R * N, N,
                                p(ll), p(info), None)
    hip.check(rc, "gf_solve_batch_rhs")
    torch.cuda.synchronize()
    res = dict(ll=ll.cpu().numpy(), info=info.cpu().numpy())
    assert np.all(res["ll"][nb * R:] == SENTINEL) and res["info"][nb] == INFO_SENTINEL
    res["ll"], res["info"] = res["ll"][:nb * R].reshape(nb, R), res["info"][:nb]
    for k, x in (("alpha", a), ("mu", m)):
        if x is None:
            res[k] = None
            continue
        x = x.cpu().numpy()
        assert np.all(x[nb * R * N:] == SENTINEL), k
        res[k] = x[:nb * R * N].reshape(nb, R, N)
    return res


def _single(hip, prob, y):
    """gf_solve_batch on one right-hand side per problem, y (B, N)."""
    return solve_call(hip, prob["Jr"], prob["Jc"], prob["real"], prob["comp"], prob["diag_add"], prob["t"], y,
                      prob["diag"], prob["N"])


def _same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _oracle(prob, Y):
    """oracle/seq.py in float64: alpha (B, R, N), mu, ll (B, R)."""
    nb, R, N = Y.shape
    alpha, mu, ll = np.empty_like(Y), np.empty_like(Y), np.empty((nb, R))
    for b in range(nb):
        co = gc.coefficients(prob, b)
        c, U, V = matrices(prob["t"][b], co)
        a = prob["diag"][b] + prob["diag_add"][b]
        d, Wm, info = seq.factor(prob["t"][b], c, a, U, V)
        assert info == 0
        z = seq.solve_lower(prob["t"][b], c, U, Wm, Y[b].T).reshape(N, R)
        alpha[b] = seq.solve_upper(prob["t"][b], c, U, Wm, z / d[:, None]).reshape(N, R).T
        mu[b] = Y[b] - prob["diag"][b] * alpha[b]
        ll[b] = -0.5 * (np.sum(np.log(d)) + N * np.log(2 * np.pi)) - 0.5 * np.sum(z * z / d[:, None], axis=0)
    return dict(alpha=alpha, mu=mu, ll=ll)


@pytest.mark.parametrize("Jr,Jc", STRUCTURES)
def test_solve_columns_have_the_single_call_bits(hip, Jr, Jc):
    """Every N, seg in (library's, 16) and R around the instance's block: alpha, mu, ll of column r and info equal
    gf_solve_batch's on that column bit for bit; at the largest R every output within 1e-9 of max |reference| per
    problem of oracle/seq.py (log L: relative)."""
    RB = int(hip.load().gf_solve_batch_rhs_block(Jr + 2 * Jc))
    assert RB >= 1
    counts = rhs_counts(RB)
    worst = 0.0
    for N in LENGTHS:
        prob = problem(Jr, Jc, N, counts[-1])
        singles = [_single(hip, prob, prob["Y"][:, r]) for r in range(counts[-1])]
        for seg in (0, 16):
            for R in counts:
                got = solve_rhs_call(hip, prob, prob["Y"][:, :R], seg=seg)
                for r in range(R):
                    one = singles[r]
                    assert _same_bits(got["alpha"][:, r], one["alpha"]), (N, seg, R, r)
                    assert _same_bits(got["mu"][:, r], one["mu"]), (N, seg, R, r)
                    assert _same_bits(got["ll"][:, r], one["ll"]), (N, seg, R, r)
                    assert np.array_equal(got["info"], one["info"]), (N, seg, R, r)
        ref = _oracle(prob, prob["Y"])
        for b in range(B):
            for k in ("alpha", "mu"):
                e = float(np.max(np.abs(got[k][b] - ref[k][b])) / np.max(np.abs(ref[k][b])))
                worst = max(worst, e)
                assert e <= BAR, (N, b, k, e)
            e = float(np.max(np.abs(got["ll"][b] - ref["ll"][b]) / np.abs(ref["ll"][b])))
            worst = max(worst, e)
            assert e <= BAR, (N, b, "ll", e)
    print(f"(Jr, Jc) = ({Jr}, {Jc}), RB = {RB}: worst error against oracle/seq.py {worst:.1e}")


def test_solve_outputs_may_be_null_and_y_may_be_shared(hip):
    Jr, Jc, N, R = 1, 8, 65, 11
    prob = problem(Jr, Jc, N, R)
    base = solve_rhs_call(hip, prob, prob["Y"])
    for kw in (dict(alpha=False), dict(mu=False), dict(alpha=False, mu=False)):
        got = solve_rhs_call(hip, prob, prob["Y"], **kw)
        assert _same_bits(got["ll"], base["ll"])
        for k in ("alpha", "mu"):
            assert got[k] is None if not kw.get(k, True) else _same_bits(got[k], base[k])
    # one block of right-hand sides shared by all problems (y_bs = 0) against B copies of it
    lib, p = hip.load(), hip.ptr
    Y0 = np.ascontiguousarray(prob["Y"][0])
    ref = solve_rhs_call(hip, prob, np.broadcast_to(Y0, (B, R, N)))
    per = int(lib.gf_solve_batch_rhs_work(N, Jr + 2 * Jc, R, 0))
    work = torch.empty((B * per,), dtype=torch.float64, device="cuda")
    rd, cd, ad = _dev(prob["real"]), _dev(prob["comp"]), _dev(prob["diag_add"])
    td, dd, yd = _dev(prob["t"]), _dev(prob["diag"]), _dev(Y0)
    a = torch.empty((B, R, N), dtype=torch.float64, device="cuda")
    ll = torch.empty((B, R), dtype=torch.float64, device="cuda")
    info = torch.empty((B,), dtype=torch.int32, device="cuda")
    rc = lib.gf_solve_batch_rhs(B, N, R, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                                p(td), N, p(dd), N, p(yd), 0, N, 0, p(work), per, p(a), None, R * N, N, p(ll), p(info),
                                None)
    hip.check(rc, "gf_solve_batch_rhs")
    assert _same_bits(a.cpu().numpy(), ref["alpha"]) and _same_bits(ll.cpu().numpy(), ref["ll"])


def test_not_positive_definite_problem_between_two_good_ones(hip):
    """tests/golden/not_positive_definite.npz between two copies of itself with its diagonal made positive: NaN in all R
    columns of that problem, ll = -inf, its info row the golden's failing row; the neighbours keep the bits they have
    alone."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "not_positive_definite.npz"))
    Jr, Jc, N = len(g["ar"]), len(g["ac"]), len(g["t"])
    RB = int(hip.load().gf_solve_batch_rhs_block(Jr + 2 * Jc))
    R = 2 * RB + 1
    amp = float(np.sum(g["ar"]) + np.sum(g["ac"]))
    real = np.repeat(np.stack([g["ar"], g["cr"]])[:, None, :], B, axis=1)
    comp = np.repeat(np.stack([g["ac"], g["bc"], g["cc"], g["dc"]])[:, None, :], B, axis=1)
    good = np.abs(g["diag_user"]) + 0.05 * amp
    prob = dict(Jr=Jr, Jc=Jc, N=N, real=real, comp=comp, t=np.repeat(g["t"][None], B, axis=0),
                diag_add=np.array([amp, amp + float(g["diag_shift"]), amp]),
                diag=np.stack([good, g["diag_user"], good]))
    rng = np.random.default_rng(3)
    Y = rng.normal(size=(B, R, N)) * np.sqrt(amp)
    Y[1, 0] = g["y"]
    for seg in (0, 16):
        got = solve_rhs_call(hip, prob, Y, seg=seg)
        assert got["info"][1] == int(g["info"]) and got["info"][0] == 0 and got["info"][2] == 0
        assert np.all(got["ll"][1] == -np.inf)
        assert np.all(np.isnan(got["alpha"][1])) and np.all(np.isnan(got["mu"][1]))
        for b in (0, 2):
            alone = solve_rhs_call(hip, {k: (v[:, b:b + 1] if k in ("real", "comp") else v[b:b + 1])
                                         if isinstance(v, np.ndarray) else v for k, v in prob.items()}, Y[b:b + 1],
                                   seg=seg)
            for k in ("alpha", "mu", "ll"):
                assert np.all(np.isfinite(got[k][b])) and _same_bits(got[k][b], alone[k][0]), (seg, b, k)


def test_solve_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    N, nb, R = 50, 2, 3
    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")      # noqa: E731
    real, comp, da, t, y = f(2, nb, 1), f(4, nb, 32), f(nb), f(N), f(nb * R * N)
    work = f(nb * int(lib.gf_solve_batch_rhs_work(N, 63, R, 0)))
    out = [torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for n in (nb * R * N, nb * R * N, nb * R)]
    info = torch.full((nb,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    assert lib.gf_solve_batch_rhs_work(N, 64, R, 0) == 0 and lib.gf_solve_batch_rhs_work(N, 16, 0, 0) == 0
    assert lib.gf_solve_batch_rhs_block(64) == 0 and lib.gf_solve_batch_rhs_block(0) == 0

    def call(N=N, R=R, Jc=8, work_bs=None, y=y, t=t, ll=out[2], info=info, work=work, y_rs=N, seg=0):
        wb = int(lib.gf_solve_batch_rhs_work(N, 2 * Jc, max(R, 1), max(seg, 0))) if work_bs is None else work_bs
        c = [p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]), p(comp[3])]
        return lib.gf_solve_batch_rhs(nb, N, R, 0, Jc, *c, p(da), p(t), 0, None, 0, p(y), R * N, y_rs, seg, p(work), wb,
                                      p(out[0]), p(out[1]), R * N, N, p(ll), p(info), None)

    need = int(lib.gf_solve_batch_rhs_work(N, 16, R, 0))
    assert call(Jc=32, work_bs=need) == -3 and "63" in hip.last_error()
    for kw in (dict(R=0, work_bs=need), dict(R=-1, work_bs=need), dict(N=0, work_bs=need), dict(work_bs=need - 1),
               dict(y=None), dict(t=None), dict(ll=None), dict(info=None), dict(work=None), dict(y_rs=N - 1),
               dict(seg=-1, work_bs=need)):
        assert call(**kw) == -1, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out) and bool(torch.all(info == INFO_SENTINEL))


# ---- gf_predict_batch_at_rhs

def design(prob, M, seed):
    """M ascending queries per problem: before t_0, behind the last stamp, coincident with stamps, inside the axis."""
    rng = np.random.default_rng([11, seed, M])
    out = np.empty((B, M))
    for b in range(B):
        t = prob["t"][b]
        span = max(t[-1] - t[0], gc.DT)
        q = rng.uniform(t[0] - 0.1 * span, t[-1] + 0.1 * span, M)
        hit = rng.choice(M, size=min(M, max(1, M // 4)), replace=False) if M else []
        q[hit] = rng.choice(t, size=len(hit))
        if M >= 2:
            q[0], q[-1] = t[0] - 0.2 * span, t[-1] + 0.2 * span
        out[b] = np.sort(q)
    return out


def at_rhs_call(hip, prob, ts, alpha, nobs=None, nq=None):
    """One gf_predict_batch_at_rhs call: ts (B, M), alpha (B, R, N) -> mu (B, R, M), sentinel in what is not written."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, N = prob["Jr"], prob["Jc"], prob["N"]
    R, M = alpha.shape[1], ts.shape[1]
    rd, cd, td, qd, ad = _dev(prob["real"]), _dev(prob["comp"]), _dev(prob["t"]), _dev(ts), _dev(alpha)
    nod = None if nobs is None else _dev(nobs, np.int64)
    nqd = None if nq is None else _dev(nq, np.int64)
    mu = torch.full((B + 1, R, M + 1), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.gf_predict_batch_at_rhs(B, N, M, R, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]),
                                     p(td), N, p(nod), p(qd), M, p(nqd), p(ad), R * N, N, p(mu), R * (M + 1), M + 1,
                                     None)
    hip.check(rc, "gf_predict_batch_at_rhs")
    torch.cuda.synchronize()
    out = mu.cpu().numpy()
    assert np.all(out[B] == SENTINEL) and np.all(out[:, :, M] == SENTINEL)
    return out[:B, :, :M]


@pytest.mark.parametrize("Jr,Jc", STRUCTURES)
def test_predict_at_columns_have_the_single_call_bits(hip, Jr, Jc):
    """Every M of QUERIES (M = 0: the status code of an empty call) at N = 65 and 197 with ragged nobs / nq: column r
    equals gf_predict_batch_at on alpha[:, r] bit for bit, rows from nq[b] on are not written."""
    lib = hip.load()
    RB = int(lib.gf_predict_batch_at_rhs_block())
    counts = rhs_counts(RB)
    for N in (65, 197):
        prob = problem(Jr, Jc, N, counts[-1])
        alpha = prob["Y"] / prob["diag_add"][:, None, None]
        for M in QUERIES:
            if M == 0:
                z = torch.zeros(8, dtype=torch.float64, device="cuda")
                q = z.data_ptr()
                assert lib.gf_predict_batch_at_rhs(B, N, 0, 1, Jr, Jc, q, q, q, q, q, q, q, 0, None, q, 0, None, q, N,
                                                   N, q, 0, 0, None) == -1
                continue
            ts = design(prob, M, N)
            for nobs, nq in ((None, None), (np.array([N, N - 1, max(N - 64, 0)]), np.array([M, M // 2, 0]))):
                singles = [at_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["t"], ts, alpha[:, r], N, M,
                                   nobs=nobs, nq=nq) for r in range(counts[-1])]
                for R in counts:
                    got = at_rhs_call(hip, prob, ts, alpha[:, :R], nobs=nobs, nq=nq)
                    for r in range(R):
                        assert _same_bits(got[:, r], singles[r]), (N, M, R, r, nobs is None)


def test_predict_at_matches_the_oracle_and_propagates_nan(hip):
    Jr, Jc, N, M = 3, 30, 130, 65
    RB = int(hip.load().gf_predict_batch_at_rhs_block())
    R = RB + 1
    prob = problem(Jr, Jc, N, R)
    alpha = prob["Y"] / prob["diag_add"][:, None, None]
    ts = design(prob, M, 5)
    got = at_rhs_call(hip, prob, ts, alpha)
    for b in range(B):
        co = gc.coefficients(prob, b)
        c, U, V = matrices(prob["t"][b], co)
        _, Us, Vs = matrices(ts[b], co)
        for r in range(R):
            ref = seq.predict_mean_at(prob["t"][b], c, U, V, alpha[b, r], ts[b], Us, Vs).reshape(-1)
            assert np.max(np.abs(got[b, r] - ref)) <= BAR * np.max(np.abs(ref)), (b, r)
    bad = alpha.copy()
    bad[1, 2] = np.nan
    nan = at_rhs_call(hip, prob, ts, bad)
    assert np.all(np.isnan(nan[1, 2]))
    keep = np.ones((B, R), dtype=bool)
    keep[1, 2] = False
    assert _same_bits(nan[keep], got[keep])
