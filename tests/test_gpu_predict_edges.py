"""GPU: gf_solve_batch through its raw C entry point at the shapes where it can go wrong (tests/grad_cases.py) -- every
width at a boundary of its three instances (k_solve<16>, <32>, <64>; odd widths), every length of grad_cases.LENGTHS,
segment lengths from one row to the whole series -- against oracle/seq.py in float64 (tests/solve_ref.oracle_predict);
bit identity across segment lengths and batches; its calling conventions (strides, diag = NULL, outputs that may be
NULL, workspace, output bounds); the failing pivot at the first and last rows of a segment; its argument checks."""
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from tests import grad_cases as gc
from tests.solve_ref import oracle_predict, split_component

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77                  # what every output holds before a call: no result of these problems
INFO_SENTINEL = -77
KEYS = ("ll", "info", "alpha", "mu", "mu_comp")
OUTS = ("alpha", "mu", "mu_comp")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _bs(a):
    """Batch stride in elements of a host array: 0 for a shared (N,) one, the row length of a (B, S) one."""
    return 0 if a.ndim == 1 else a.shape[1]


def solve_call(hip, Jr, Jc, real, comp, diag_add, t, y, diag, N, component=None, seg=0, outs=OUTS, work_extra=0,
               work_fill=0.0):
    """One gf_solve_batch call on host arrays: real (2, B, max(Jr, 1)), comp (4, B, max(Jc, 1)), diag_add (B,);
    ``component`` = (Jr', Jc', real', comp') in the same layout or None; t, y, diag (N,) shared or (B, S >= N) per
    problem, diag may be None (NULL); ``outs``: which of alpha, mu, mu_comp are asked for (the others NULL).  The
    workspace holds ``work_fill`` on entry and is ``work_extra`` doubles per problem larger than gf_solve_batch_work
    asks.  Every output is allocated one problem too long and pre-filled with a sentinel that must survive.  Returns
    dict(ll, info, alpha, mu, mu_comp) with None for the outputs not asked for."""
    lib, p = hip.load(), hip.ptr
    B, lr, lc = real.shape[1], max(Jr, 1), max(Jc, 1)
    assert real.shape == (2, B, lr) and comp.shape == (4, B, lc) and diag_add.shape == (B,)
    per = int(lib.gf_solve_batch_work(N, Jr + 2 * Jc, seg))
    assert per > 0
    per += work_extra
    work = torch.full((B * per,), work_fill, dtype=torch.float64, device="cuda")
    rd, cd, ad, td, yd = _dev(real), _dev(comp), _dev(diag_add), _dev(t), _dev(y)
    dd = None if diag is None else _dev(diag)
    if component is None:
        outs = tuple(k for k in outs if k != "mu_comp")
        jr2 = jc2 = 0
        c2 = [None] * 6
    else:
        jr2, jc2, r2, k2 = component
        assert r2.shape == (2, B, max(jr2, 1)) and k2.shape == (4, B, max(jc2, 1))
        r2d, k2d = _dev(r2), _dev(k2)
        c2 = [p(r2d[0]), p(r2d[1]), p(k2d[0]), p(k2d[1]), p(k2d[2]), p(k2d[3])]
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    bufs = {k: (f((B + 1) * N) if k in outs else None) for k in OUTS}
    ll = f(B + 1)
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_solve_batch(B, N, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                            jr2, jc2, *c2, p(td), _bs(t), p(dd), 0 if diag is None else _bs(diag), p(yd), _bs(y),
                            seg, p(work), per, p(bufs["alpha"]), p(bufs["mu"]), p(bufs["mu_comp"]), p(ll), p(info),
                            None)
    hip.check(rc, "gf_solve_batch")
    torch.cuda.synchronize()
    res = dict(ll=ll.cpu().numpy(), info=info.cpu().numpy())
    assert res["ll"][B] == SENTINEL and res["info"][B] == INFO_SENTINEL
    res["ll"], res["info"] = res["ll"][:B], res["info"][:B]
    for k in OUTS:
        if bufs[k] is None:
            res[k] = None
            continue
        x = bufs[k].cpu().numpy()
        assert np.all(x[B * N:] == SENTINEL), k
        res[k] = x[:B * N].reshape(B, N)
    return res


def _identical(a, b, rows=slice(None), keys=KEYS):
    """Two results agree to the bit (NaN = NaN) on the problems ``rows``."""
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k][rows], b[k][rows], equal_nan=True)
               for k in keys)


def _component(prob):
    return split_component(prob["Jr"], prob["Jc"], prob["real"], prob["comp"])


@functools.lru_cache(maxsize=None)
def _reference(Jr, Jc, N):
    """oracle/seq.py in float64 for the B problems of grad_cases.edge_problem(Jr, Jc, N), the component the first
    half of each kind of term: computed once, shared, never changed."""
    prob = gc.edge_problem(Jr, Jc, N)
    jr, jc, r2, c2 = _component(prob)
    out = []
    for b in range(prob["B"]):
        comp = (r2[0, b, :jr], r2[1, b, :jr]) + tuple(c2[i, b, :jc] for i in range(4))
        out.append(oracle_predict(prob["t"], prob["y"][b], prob["diag"][b], gc.coefficients(prob, b),
                                  prob["diag_add"][b], comp=comp))
    return tuple(out)


def _segments(N):
    """0 (the library's choice), 1, 2, 3, a length that leaves a last segment of exactly one row, one whose last
    segment is exactly full, and the whole series."""
    segs = [0, 1, 2, 3]
    one = [k for k in range(2, N) if N % k == 1]
    full = [k for k in range(2, N) if N % k == 0]
    segs += one[:1] + one[-1:] + full[:1] + full[-1:] + [N]
    return sorted(set(k for k in segs if k <= N))


def _problem_args(prob):
    return (prob["Jr"], prob["Jc"], prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"], prob["diag"],
            prob["N"])


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_edge_shapes_match_the_oracle_for_every_segment_length(hip, Jr, Jc):
    """B = 3 problems of different coefficients, data and diagonals on a shared axis at every length of
    grad_cases.LENGTHS: alpha, mu and mu' within 1e-9 of max |reference| per problem and log L within 1e-9 relative of
    oracle/seq.py in float64, at the library's segment length; every other segment length, and every problem alone,
    gives the same bits."""
    bad, worst = [], dict(ll=0.0, alpha=0.0, mu=0.0, mu_comp=0.0)
    for N in gc.LENGTHS:
        prob = gc.edge_problem(Jr, Jc, N)
        component = _component(prob)
        base = solve_call(hip, *_problem_args(prob), component=component)
        assert np.all(base["info"] == 0), (N, base["info"])
        for b, ref in enumerate(_reference(Jr, Jc, N)):
            errs = dict(ll=abs(base["ll"][b] - ref["ll"]) / abs(ref["ll"]))
            for k in OUTS:
                errs[k] = float(np.max(np.abs(base[k][b] - ref[k])) / np.max(np.abs(ref[k])))
            worst = {k: max(worst[k], errs[k]) for k in worst}
            if any(not e <= 1e-9 for e in errs.values()):
                bad.append((N, b, errs))
        for seg in _segments(N)[1:]:
            got = solve_call(hip, *_problem_args(prob), component=component, seg=seg)
            assert _identical(got, base), (N, seg)
        for b in range(prob["B"]):
            one = solve_call(hip, Jr, Jc, prob["real"][:, b:b + 1], prob["comp"][:, b:b + 1],
                             prob["diag_add"][b:b + 1], prob["t"], prob["y"][b:b + 1], prob["diag"][b:b + 1], N,
                             component=(component[0], component[1], component[2][:, b:b + 1],
                                        component[3][:, b:b + 1]), seg=2)
            assert all(np.array_equal(one[k][0], base[k][b]) for k in KEYS), (N, b)
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: log L {worst['ll']:.1e}, alpha {worst['alpha']:.1e}, "
          f"mu {worst['mu']:.1e}, mu' {worst['mu_comp']:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", [(0, 8), (1, 16), (1, 31)])
def test_call_conventions(hip, Jr, Jc):
    """N = 101 and N = 13 at the library's segment length and at 11 / 4 rows (last segments of two rows and one)."""
    for N, seg in ((101, 0), (101, 11), (13, 4)):
        prob = gc.edge_problem(Jr, Jc, N)
        B = prob["B"]
        real, comp, da = prob["real"], prob["comp"], prob["diag_add"]
        component = _component(prob)
        t, y, diag = prob["t"], prob["y"][0], prob["diag"][0]
        kw = dict(component=component, seg=seg)
        base = solve_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, **kw)
        assert np.all(base["info"] == 0) and all(np.all(np.isfinite(base[k])) for k in KEYS)
        # t, y, diag shared (stride 0) against B copies at a stride of N + 3 (the three pad elements are never read)
        wide = [np.full((B, N + 3), np.nan) for _ in range(3)]
        for w, x in zip(wide, (t, y, diag)):
            w[:, :N] = x
        assert _identical(base, solve_call(hip, Jr, Jc, real, comp, da, *wide, N, **kw)), N
        # a workspace 17 doubles per problem longer than asked and full of NaN against a zeroed minimal one: nothing is
        # read before it is written, and the stride is the caller's
        assert _identical(base, solve_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, work_extra=17,
                                           work_fill=float("nan"), **kw)), N
        # each output NULL in turn: the others do not change (mu_comp = NULL goes with no component)
        for drop in OUTS:
            keep = tuple(k for k in OUTS if k != drop)
            got = solve_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, seg=seg, outs=keep,
                             component=None if drop == "mu_comp" else component)
            assert got[drop] is None
            assert _identical(got, base, keys=("ll", "info") + keep), (N, drop)
        # diag = NULL against an array of zeros (the white noise folded into diag_add), and mu = y exactly
        da2 = da * 1.05
        null = solve_call(hip, Jr, Jc, real, comp, da2, t, y, None, N, **kw)
        assert np.all(null["info"] == 0)
        assert _identical(null, solve_call(hip, Jr, Jc, real, comp, da2, t, y, np.zeros(N), N, **kw)), N
        assert np.array_equal(null["mu"], np.broadcast_to(y, (B, N)))


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (0, 31)])
def test_failing_pivot_at_segment_edges(hip, Jr, Jc):
    """N = 101 in segments of 11 rows.  One problem of three loses positive definiteness from row r on -- the first
    row, both sides of a segment boundary (10 | 11), the last row of a segment (98), the first row of the last
    segment (99), the last row (100): info is the C oracle's failing row, log L is -inf, every row of every output of
    that problem NaN, and its neighbours do not notice."""
    N = 101
    prob = gc.edge_problem(Jr, Jc, N)
    component = _component(prob)
    args = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"])
    base = solve_call(hip, *args, prob["diag"], N, component=component, seg=11)
    assert np.all(base["info"] == 0)
    for r in (0, 10, 11, 98, 99, 100):
        diag = prob["diag"].copy()
        diag[1, r:] = -1e6
        got = solve_call(hip, *args, diag, N, component=component, seg=11)
        _, info = cref.loglike(gc.coefficients(prob, 1), prob["t"], diag[1], prob["y"][1])
        assert info >= r + 1 and got["info"][1] == info, (r, got["info"], info)
        assert got["ll"][1] == -np.inf
        for k in OUTS:
            assert np.all(np.isnan(got[k][1])), (r, k)
        assert _identical(got, base, rows=[0, 2]), r


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    N, B = 50, 2
    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")      # noqa: E731
    real, comp, da, t, y = f(2, B, 1), f(4, B, 32), f(B), f(N), f(N)
    work = f(B * int(lib.gf_solve_batch_work(N, 63, 0)))
    out = [torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for n in (B * N, B * N, B * N, B)]
    info = torch.full((B,), INFO_SENTINEL, dtype=torch.int32, device="cuda")

    def call(N=N, Jc=8, Jc2=0, work_bs=None, y=y, mu_comp=None, seg=0):
        wb = int(lib.gf_solve_batch_work(N, 2 * Jc, seg)) if work_bs is None else work_bs
        c = [p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]), p(comp[3])]
        return lib.gf_solve_batch(B, N, 0, Jc, *c, p(da), 0, Jc2, *c, p(t), 0, None, 0, p(y), 0, seg, p(work), wb,
                                  p(out[0]), p(out[1]), mu_comp, p(out[3]), p(info), None)

    need = int(lib.gf_solve_batch_work(N, 16, 0))
    assert call(Jc=32, work_bs=need) == -3 and "63" in hip.last_error()                   # W = 64
    assert call(Jc2=32, mu_comp=p(out[2])) == -3 and "63" in hip.last_error()             # W' = 64
    for kw in (dict(work_bs=need - 1), dict(N=0, work_bs=need), dict(y=None), dict(seg=-1, work_bs=need),
               dict(Jc2=4), dict(mu_comp=p(out[2]))):
        assert call(**kw) == -1, kw
        assert hip.last_error(), kw
    # the workspace is sized for the segment length asked for
    assert call(seg=N, work_bs=int(lib.gf_solve_batch_work(N, 16, N)) - 1) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out) and bool(torch.all(info == INFO_SENTINEL))
