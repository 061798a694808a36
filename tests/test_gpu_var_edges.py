"""GPU: gf_var_batch through its raw C entry point at the shapes where it can go wrong (tests/grad_cases.py) -- every
width at a boundary of its instances (k_var<16>, <32>, <64>, with and without queries), every length of
grad_cases.LENGTHS, segments of one row, the library's length and the whole series: alpha, mu, log L and info with
gf_solve_batch's bits; h, the variances at the observed times and at new ones against the numpy restatement of the
passes (tests/var_ref.var_passes, itself held to the dense inverse by tests/test_var_host.py); bit identity across
segment lengths and batches; query counts around the 64-lane runs, all in one interval, before the first row, after
the last one, on the stamps; per-problem counts; workspace and output bounds; the failing pivot; argument checks."""
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from tests import grad_cases as gc
from tests.test_gpu_predict_edges import solve_call
from tests.var_ref import dense_reference, queries, var_passes

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77                  # what every output holds before a call: no result of these problems
INFO_SENTINEL = -77
OUTS = ("alpha", "mu", "hdiag", "var")
KEYS = ("ll", "info") + OUTS + ("var_at",)
SOLVE_KEYS = ("ll", "info", "alpha", "mu")
TOL = 1e-9                           # of max |reference| per problem: the bar of gf_solve_batch's tests


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _bs(a):
    return 0 if a.ndim == 1 else a.shape[1]


def var_call(hip, Jr, Jc, real, comp, diag_add, t, y, diag, N, ts=None, nobs=None, nq=None, seg=0, outs=OUTS,
             work_extra=0, work_fill=0.0):
    """One gf_var_batch call on host arrays (layouts as tests.test_gpu_predict_edges.solve_call); ``ts`` (M,) shared or
    (B, M) or None, ``nobs`` / ``nq`` (B,) or None.  Every output is one problem too long and pre-filled with a
    sentinel that must survive; the workspace holds ``work_fill`` and is ``work_extra`` doubles per problem larger than
    asked, and nothing beyond gf_var_batch_work of any problem's share may change.  Returns dict(ll, info, alpha,
    mu, hdiag, var, var_at) with None for the outputs not asked for."""
    lib, p = hip.load(), hip.ptr
    B = real.shape[1]
    M = 0 if ts is None else ts.shape[-1]
    need = int(lib.gf_var_batch_work(N, Jr + 2 * Jc, M, seg))
    assert need > 0
    per = need + work_extra
    work = torch.full((B * per,), work_fill, dtype=torch.float64, device="cuda")
    rd, cd, ad, td, yd = _dev(real), _dev(comp), _dev(diag_add), _dev(t), _dev(y)
    dd = None if diag is None else _dev(diag)
    qd = None if ts is None else _dev(ts)
    cnt = [None if c is None else torch.as_tensor(np.asarray(c, dtype=np.int64)).cuda() for c in (nobs, nq)]
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    bufs = {k: (f((B + 1) * N) if k in outs else None) for k in OUTS}
    bufs["var_at"] = f((B + 1) * M) if M else None
    ll = f(B + 1)
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_var_batch(B, N, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                          p(td), _bs(t), p(dd), 0 if diag is None else _bs(diag), p(yd), _bs(y),
                          p(qd), 0 if ts is None else _bs(ts), M, p(cnt[0]), p(cnt[1]), seg, p(work), per,
                          p(bufs["alpha"]), p(bufs["mu"]), p(bufs["hdiag"]), p(bufs["var"]), p(bufs["var_at"]),
                          p(ll), p(info), None)
    hip.check(rc, "gf_var_batch")
    torch.cuda.synchronize()
    if work_extra:
        tail = work.reshape(B, per)[:, need:].cpu().numpy()
        assert np.all(np.isnan(tail)) if np.isnan(work_fill) else np.all(tail == work_fill)
    res = dict(ll=ll.cpu().numpy(), info=info.cpu().numpy())
    assert res["ll"][B] == SENTINEL and res["info"][B] == INFO_SENTINEL
    res["ll"], res["info"] = res["ll"][:B], res["info"][:B]
    for k, n in [(k, N) for k in OUTS] + [("var_at", M)]:
        if bufs[k] is None:
            res[k] = None
            continue
        x = bufs[k].cpu().numpy()
        assert np.all(x[B * n:] == SENTINEL), k
        res[k] = x[:B * n].reshape(B, n)
    return res


def _identical(a, b, rows=slice(None), keys=KEYS):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k][rows], b[k][rows], equal_nan=True)
               for k in keys)


def _problem_args(prob):
    return (prob["Jr"], prob["Jc"], prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"], prob["diag"],
            prob["N"])


def _one(prob, b):
    return (prob["Jr"], prob["Jc"], prob["real"][:, b:b + 1], prob["comp"][:, b:b + 1], prob["diag_add"][b:b + 1],
            prob["t"], prob["y"][b:b + 1], prob["diag"][b:b + 1], prob["N"])


@functools.lru_cache(maxsize=None)
def _reference(Jr, Jc, N):
    """tests/var_ref.var_passes in float64 for the B problems of grad_cases.edge_problem(Jr, Jc, N) with the queries of
    var_ref.queries: computed once, shared, never changed."""
    prob = gc.edge_problem(Jr, Jc, N)
    ts = queries(prob["t"], gc.DT)
    return ts, tuple(var_passes(prob["t"], prob["y"][b], prob["diag"][b], Jr, Jc, gc.coefficients(prob, b),
                                prob["diag_add"][b], N, ts=ts) for b in range(prob["B"]))


def _errors(got, ref, b, keys=("hdiag", "var", "var_at")):
    return {k: float(np.max(np.abs(got[k][b] - ref[k])) / np.max(np.abs(ref[k]))) for k in keys}


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_edge_shapes_match_the_reference_for_every_segment_length(hip, Jr, Jc):
    """B = 3 problems on a shared axis at every length of grad_cases.LENGTHS, with queries before the first row, on
    stamps, inside intervals and after the end: alpha, mu, log L, info bit for bit gf_solve_batch's; h, var and var_at
    within 1e-9 of max |reference| per problem; segments of one row and of the whole series, every problem alone and
    the call without queries give the same bits."""
    bad, worst = [], dict(hdiag=0.0, var=0.0, var_at=0.0)
    for N in gc.LENGTHS:
        prob = gc.edge_problem(Jr, Jc, N)
        ts, refs = _reference(Jr, Jc, N)
        base = var_call(hip, *_problem_args(prob), ts=ts)
        assert np.all(base["info"] == 0), (N, base["info"])
        solve = solve_call(hip, *_problem_args(prob))
        assert all(np.array_equal(base[k], solve[k]) for k in SOLVE_KEYS), N
        for b, ref in enumerate(refs):
            errs = _errors(base, ref, b)
            worst = {k: max(worst[k], errs[k]) for k in worst}
            if any(not e <= TOL for e in errs.values()):
                bad.append((N, b, errs))
        for seg in sorted({1, N} - {int(hip.load().gf_solve_batch_seg(N, Jr + 2 * Jc))}):
            assert _identical(var_call(hip, *_problem_args(prob), ts=ts, seg=seg), base), (N, seg)
        for b in range(prob["B"]):
            one = var_call(hip, *_one(prob, b), ts=ts, seg=2)
            assert all(np.array_equal(one[k][0], base[k][b]) for k in KEYS), (N, b)
        plain = var_call(hip, *_problem_args(prob))                    # k_var<., false>
        assert plain["var_at"] is None and _identical(plain, base, keys=("ll", "info") + OUTS), N
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: h {worst['hdiag']:.1e}, var {worst['var']:.1e}, "
          f"var_at {worst['var_at']:.1e}")
    assert not bad, bad


def _query_sets(t, M):
    """M queries all inside one interval, all before the first row, all after the last row, and on the stamps (every
    stamp from the middle on in turn, repeated: ties with rows and with each other)."""
    N = len(t)
    n = N // 3
    u = (np.arange(M) + 0.5) / max(M, 1)
    return dict(inside=t[n] + u * (t[n + 1] - t[n]), before=t[0] - (2.0 - u) * 7 * gc.DT,
                after=t[N - 1] + u * 9 * gc.DT, ties=np.sort(t[N // 2 + np.arange(M) % (N - N // 2)]))


@pytest.mark.parametrize("Jr,Jc", [(0, 8), (1, 16), (1, 31)])
def test_query_counts_and_places(hip, Jr, Jc):
    """N = 101 in segments of 11 rows, M in {1, 63, 64, 65} (M = 0 is the call without queries above): the staged
    queries cross the 64-lane runs of var_at; a query's value is the one it has alone in the restatement."""
    N = 101
    prob = gc.edge_problem(Jr, Jc, N)
    t = prob["t"]
    for M in (1, 63, 64, 65):
        for name, ts in _query_sets(t, M).items():
            got = var_call(hip, *_problem_args(prob), ts=ts, seg=11)
            assert np.all(got["info"] == 0)
            for b in range(prob["B"]):
                ref = var_passes(t, prob["y"][b], prob["diag"][b], Jr, Jc, gc.coefficients(prob, b),
                                 prob["diag_add"][b], N, ts=ts)
                e = _errors(got, ref, b)
                assert all(v <= TOL for v in e.values()), (M, name, b, e)
            if name == "before":                 # nothing observed yet: no more than the prior variance
                assert np.all(got["var_at"] <= prob["diag_add"][:, None]) and np.all(got["var_at"] > 0.0)


def test_per_problem_counts_and_missing_data_rows(hip):
    """Three problems of 101, 60 and 1 real rows (the rest missing-data rows of diag = 2^1000 at the end, as ragged
    batches pad) and of 65, 7 and 0 real queries on per-problem axes: each problem's real rows and queries are those of
    its short problem alone (dense inverse, 1e-9), var_at beyond nq[b] is never written, and the queries behind the
    last real row belong to it."""
    Jr, Jc, N, M = 1, 16, 101, 65
    prob = gc.edge_problem(Jr, Jc, N)
    nobs, nq = np.array([101, 60, 1]), np.array([65, 7, 0])
    t = prob["t"]
    diag, y = prob["diag"].copy(), prob["y"].copy()
    ts = np.zeros((3, M))
    for b in range(3):
        diag[b, nobs[b]:], y[b, nobs[b]:] = 2.0 ** 1000, 0.0
        q = np.sort(np.concatenate([queries(t[:nobs[b]], gc.DT), t[0] + (t[nobs[b] - 1] - t[0] + 3 * gc.DT)
                                    * np.linspace(0.01, 0.99, M)]))
        q = q[np.linspace(0, len(q) - 1, nq[b]).astype(int)]          # spread over the axis, both ends kept
        ts[b, :nq[b]] = q
        ts[b, nq[b]:] = q[-1] if nq[b] else 0.0
    args = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], t, y, diag, N)
    got = var_call(hip, *args, ts=ts, nobs=nobs, nq=nq, seg=11)
    assert np.all(got["info"] == 0) and all(np.all(np.isfinite(got[k])) for k in OUTS)
    for b in range(3):
        n, m = nobs[b], nq[b]
        assert np.all(got["var_at"][b, m:] == SENTINEL)
        ref = dense_reference(t[:n], y[b, :n], diag[b, :n], Jr, Jc, gc.coefficients(prob, b), prob["diag_add"][b],
                              ts=ts[b, :m] if m else None)
        for k in OUTS:
            assert np.max(np.abs(got[k][b, :n] - ref[k])) <= TOL * np.max(np.abs(ref[k])), (b, k)
        if m:
            assert np.max(np.abs(got["var_at"][b, :m] - ref["var_at"])) <= TOL * np.max(np.abs(ref["var_at"])), b
    assert _identical(got, var_call(hip, *args, ts=ts, nobs=nobs, nq=nq, seg=N))


@pytest.mark.parametrize("Jr,Jc", [(0, 8), (1, 16), (1, 31)])
def test_call_conventions(hip, Jr, Jc):
    for N, seg in ((101, 0), (13, 4)):
        prob = gc.edge_problem(Jr, Jc, N)
        B = prob["B"]
        real, comp, da = prob["real"], prob["comp"], prob["diag_add"]
        t, y, diag = prob["t"], prob["y"][0], prob["diag"][0]
        ts = queries(t, gc.DT)
        base = var_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, ts=ts, seg=seg)
        assert np.all(base["info"] == 0) and all(np.all(np.isfinite(base[k])) for k in KEYS)
        # shared arrays (stride 0) against B copies at a stride three longer
        wide = [np.full((B, len(x) + 3), np.nan) for x in (t, y, diag, ts)]
        for w, x in zip(wide, (t, y, diag, ts)):
            w[:, :len(x)] = x
        M = len(ts)
        got = var_call(hip, Jr, Jc, real, comp, da, *wide[:3], N, ts=wide[3][:, :M].copy(), seg=seg)
        assert _identical(base, got), N
        # a workspace 17 doubles per problem longer than asked and full of NaN: nothing is read before it is written,
        # nothing is written beyond gf_var_batch_work
        assert _identical(base, var_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, ts=ts, seg=seg, work_extra=17,
                                         work_fill=float("nan"))), N
        # each output NULL in turn: the others do not change
        for drop in OUTS:
            keep = tuple(k for k in OUTS if k != drop)
            got = var_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, ts=ts, seg=seg, outs=keep)
            assert got[drop] is None and _identical(got, base, keys=("ll", "info", "var_at") + keep), (N, drop)
        # diag = NULL against zeros: the variance at the observed times is exactly 0, h finite
        da2 = da * 1.05
        null = var_call(hip, Jr, Jc, real, comp, da2, t, y, None, N, ts=ts, seg=seg)
        assert _identical(null, var_call(hip, Jr, Jc, real, comp, da2, t, y, np.zeros(N), N, ts=ts, seg=seg)), N
        assert np.all(null["var"] == 0.0) and np.all(np.isfinite(null["hdiag"])) and np.all(null["hdiag"] > 0.0)


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (0, 31)])
def test_failing_pivot_at_segment_edges(hip, Jr, Jc):
    """N = 101 in segments of 11 rows; one problem of three loses positive definiteness from row r on: info is the C
    oracle's failing row, log L is -inf, every row of every output of that problem NaN, its neighbours bit-unchanged."""
    N = 101
    prob = gc.edge_problem(Jr, Jc, N)
    ts = queries(prob["t"], gc.DT)
    args = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"])
    base = var_call(hip, *args, prob["diag"], N, ts=ts, seg=11)
    assert np.all(base["info"] == 0)
    for r in (0, 10, 11, 98, 99, 100):
        diag = prob["diag"].copy()
        diag[1, r:] = -1e6
        got = var_call(hip, *args, diag, N, ts=ts, seg=11)
        _, info = cref.loglike(gc.coefficients(prob, 1), prob["t"], diag[1], prob["y"][1])
        assert info >= r + 1 and got["info"][1] == info, (r, got["info"], info)
        assert got["ll"][1] == -np.inf
        for k in OUTS + ("var_at",):
            assert np.all(np.isnan(got[k][1])), (r, k)
        assert _identical(got, base, rows=[0, 2]), r


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    N, B, M = 50, 2, 5
    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")      # noqa: E731
    real, comp, da, t, y, ts = f(2, B, 1), f(4, B, 32), f(B), f(N), f(N), f(M)
    work = f(B * int(lib.gf_var_batch_work(N, 63, M, 0)))
    out = [torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for n in (B * N,) * 4 + (B * M, B)]
    info = torch.full((B,), INFO_SENTINEL, dtype=torch.int32, device="cuda")

    def call(N=N, Jc=8, M=M, work_bs=None, y=y, ts=ts, var_at=p(out[4]), seg=0, ts_bs=0):
        wb = int(lib.gf_var_batch_work(N, 2 * Jc, max(M, 0), seg)) if work_bs is None else work_bs
        c = [p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]), p(comp[3])]
        return lib.gf_var_batch(B, N, 0, Jc, *c, p(da), p(t), 0, None, 0, p(y), 0, p(ts), ts_bs, M, None, None, seg,
                                p(work), wb, p(out[0]), p(out[1]), p(out[2]), p(out[3]), var_at, p(out[5]), p(info),
                                None)

    need = int(lib.gf_var_batch_work(N, 16, M, 0))
    assert call(Jc=32, work_bs=need) == -3 and "63" in hip.last_error()                   # W = 64
    for kw in (dict(work_bs=need - 1), dict(N=0, work_bs=need), dict(y=None), dict(seg=-1, work_bs=need),
               dict(M=-1, work_bs=need), dict(var_at=None), dict(ts=None), dict(M=0), dict(ts_bs=-1)):
        assert call(**kw) == -1, kw                      # (M = 0 with var_at: the two go together)
        assert hip.last_error(), kw
    # the workspace is sized for the segment length and the queries asked for
    assert call(seg=N, work_bs=int(lib.gf_var_batch_work(N, 16, M, N)) - 1) == -1
    assert call(work_bs=int(lib.gf_var_batch_work(N, 16, M - 1, 0))) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out) and bool(torch.all(info == INFO_SENTINEL))
