"""GPU: gf_solve_batch_wide through its raw C entry point at the shapes where it can go wrong -- both
sides of the boundaries of its three instances (W = 64 | 65, 128 | 129), the 86-term default kernel's width, the largest
width and an odd one beside it, lengths at the edges of the segments and of the 64-row runs, every segment rule at
N = 101 -- against oracle/seq.py in float64 (tests/solve_ref.oracle_predict), against the one-wave kernel where both run,
bit-identity across the segment length and the batch, a workspace full of NaN, the optional outputs, and the failing
pivot."""
import functools

import numpy as np
import pytest
import torch

from tests import grad_cases as gc
from tests.solve_ref import oracle_predict

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
INFO_SENTINEL = -77
KEYS = ("ll", "info", "alpha", "mu")

#: W = 2, 17, 63 (narrow); 64, 64, 65 and 128, 128, 129: both sides of the instance boundaries, with and without real
#: terms; 172 and 176: the 86-term default kernel, bare and with four real terms; 192, the largest, and 191 beside it
STRUCTURES = ((0, 1), (1, 8), (3, 30), (0, 32), (2, 31), (1, 32), (0, 64), (2, 63), (1, 64), (0, 86), (4, 86), (0, 96),
              (1, 95))
LENGTHS = (1, 2, 3, 5, 17, 101, 197)
SEGS = (1, 2, 7, 50, 101, 1000)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def wide_call(hip, prob, seg=0, rows=slice(None), diag=None, no_diag=False, outs=("alpha", "mu")):
    """One gf_solve_batch_wide call on the problems ``rows`` of a grad_cases.edge_problem (shared t, per-problem y and
    diag; ``no_diag``: diag = NULL) at ``seg`` rows per segment.  The workspace is full of NaN on entry and every output
    is one problem too long and pre-filled with a sentinel that must survive; ``outs``: which of alpha and mu are asked
    for (the other NULL, None in the result)."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, N = prob["Jr"], prob["Jc"], prob["N"]
    real, comp, da = prob["real"][:, rows], prob["comp"][:, rows], prob["diag_add"][rows]
    y, dg = prob["y"][rows], (prob["diag"] if diag is None else diag)[rows]
    B = real.shape[1]
    per = int(lib.gf_solve_wide_work(N, Jr + 2 * Jc, seg))
    assert per > 0
    work = torch.full((B * per,), float("nan"), dtype=torch.float64, device="cuda")
    rd, cd, ad, td, yd = _dev(real), _dev(comp), _dev(da), _dev(prob["t"]), _dev(y)
    dd = None if no_diag else _dev(dg)
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    bufs = {k: (f((B + 1) * N) if k in outs else None) for k in ("alpha", "mu")}
    ll = f(B + 1)
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_solve_batch_wide(B, N, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                                 p(td), 0, p(dd), 0 if no_diag else N, p(yd), N, seg, p(work), per,
                                 p(bufs["alpha"]), p(bufs["mu"]), p(ll), p(info), None)
    hip.check(rc, "gf_solve_batch_wide")
    torch.cuda.synchronize()
    res = dict(ll=ll.cpu().numpy(), info=info.cpu().numpy())
    assert res["ll"][B] == SENTINEL and res["info"][B] == INFO_SENTINEL
    res["ll"], res["info"] = res["ll"][:B], res["info"][:B]
    for k, buf in bufs.items():
        if buf is None:
            res[k] = None
            continue
        x = buf.cpu().numpy()
        assert np.all(x[B * N:] == SENTINEL), k
        res[k] = x[:B * N].reshape(B, N)
    return res


def _same(a, ia, b, ib, keys=KEYS):
    """Problem ia of result a and problem ib of result b agree to the bit (NaN = NaN)."""
    return all(np.array_equal(a[k][ia], b[k][ib], equal_nan=True) for k in keys)


def _errors(got, b, ref):
    """(log L relative, alpha and mu in units of max |reference|) of problem b against a reference dict."""
    out = [abs(got["ll"][b] - ref["ll"]) / abs(ref["ll"])]
    for k in ("alpha", "mu"):
        scale = float(np.max(np.abs(ref[k])))
        out.append(float(np.max(np.abs(got[k][b] - ref[k]))) / (scale if scale > 0.0 else 1.0))
    return out


@functools.lru_cache(maxsize=None)
def _references(Jr, Jc, N):
    """(problem, oracle/seq.py in float64 per problem): computed once, shared, never changed."""
    prob = gc.edge_problem(Jr, Jc, N)
    ref = tuple(oracle_predict(prob["t"], prob["y"][b], prob["diag"][b], gc.coefficients(prob, b), prob["diag_add"][b])
                for b in range(prob["B"]))
    return prob, ref


@pytest.mark.parametrize("Jr,Jc", STRUCTURES)
def test_edge_shapes_match_the_oracle(hip, Jr, Jc):
    """B = 3 at every length of LENGTHS and the default segments: log L to 1e-9 relative, alpha and mu to 1e-9 of
    max |reference| per problem."""
    bad, worst = [], [0.0, 0.0, 0.0]
    for N in LENGTHS:
        prob, ref = _references(Jr, Jc, N)
        got = wide_call(hip, prob)
        assert np.all(got["info"] == 0), (N, got["info"])
        for b in range(prob["B"]):
            assert ref[b]["info"] == 0
            errs = _errors(got, b, ref[b])
            worst = [max(w, e) for w, e in zip(worst, errs)]
            if not all(e <= 1e-9 for e in errs):
                bad.append((N, b, errs))
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: oracle log L {worst[0]:.1e}, alpha {worst[1]:.1e}, "
          f"mu {worst[2]:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", STRUCTURES)
def test_segment_rules_and_batch_independence(hip, Jr, Jc):
    """N = 101 at 1, 2, 7, 50, 101 and 1000 rows per segment: every output equal to the bit over all the segment rules
    (and so within the bars), and problem 1 alone (B = 1), as the last of two (B = 2) and as the first of rows 1..2 at
    seven rows per segment with the bits it has among three."""
    N = 101
    prob, ref = _references(Jr, Jc, N)
    base = wide_call(hip, prob)
    assert np.all(base["info"] == 0)
    for b in range(prob["B"]):
        assert all(e <= 1e-9 for e in _errors(base, b, ref[b])), b
    for seg in SEGS:
        got = wide_call(hip, prob, seg=seg)
        for b in range(prob["B"]):
            assert _same(got, b, base, b), (seg, b)
    assert _same(wide_call(hip, prob, rows=slice(1, 2)), 0, base, 1)
    assert _same(wide_call(hip, prob, rows=slice(0, 2)), 1, base, 1)
    assert _same(wide_call(hip, prob, rows=slice(1, 3), seg=7), 0, base, 1)


@pytest.mark.parametrize("Jr,Jc", [s for s in STRUCTURES if s[0] + 2 * s[1] <= 63])
def test_narrow_widths_match_the_one_wave_kernel(hip, Jr, Jc):
    """W <= 63 against gf_solve_batch on the same problems: log L to 1e-12, alpha and mu to 1e-10 of max |reference|."""
    from tests.test_gpu_predict_edges import solve_call
    worst = [0.0, 0.0, 0.0]
    for N in LENGTHS:
        prob, _ = _references(Jr, Jc, N)
        got = wide_call(hip, prob)
        one = solve_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"], prob["diag"],
                         N)
        assert np.all(one["info"] == 0)
        for b in range(prob["B"]):
            e = _errors(got, b, dict(ll=one["ll"][b], alpha=one["alpha"][b], mu=one["mu"][b]))
            worst = [max(w, x) for w, x in zip(worst, e)]
    print(f"(Jr, Jc) = ({Jr}, {Jc}): against the one-wave kernel log L {worst[0]:.1e}, alpha {worst[1]:.1e}, "
          f"mu {worst[2]:.1e}")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-10 and worst[2] <= 1e-10, worst


@pytest.mark.parametrize("Jr,Jc", [(1, 8), (2, 63), (4, 86)])
def test_optional_arguments(hip, Jr, Jc):
    """diag = NULL gives mu = y exactly; alpha = NULL and mu = NULL each leave the other's bits (and ll, info)
    unchanged."""
    for N in (5, 101):
        prob, _ = _references(Jr, Jc, N)
        base = wide_call(hip, prob)
        nod = wide_call(hip, prob, no_diag=True)
        assert np.all(nod["info"] == 0) and np.array_equal(nod["mu"], prob["y"])
        only_mu = wide_call(hip, prob, outs=("mu",))
        only_alpha = wide_call(hip, prob, outs=("alpha",))
        assert only_mu["alpha"] is None and only_alpha["mu"] is None
        for b in range(prob["B"]):
            assert _same(only_mu, b, base, b, ("ll", "info", "mu")), (N, b)
            assert _same(only_alpha, b, base, b, ("ll", "info", "alpha")), (N, b)


@pytest.mark.parametrize("Jr,Jc", [(1, 8), (1, 32), (4, 86)])
def test_failing_pivot_between_healthy_problems(hip, Jr, Jc):
    """N = 101 at 11 rows per segment: problem 1 of three loses positive definiteness from row r on -- the first row,
    both sides of a segment boundary, the last row: log L is -inf, info the 1-based failing row, every row of that
    problem NaN, and its neighbours have the bits of a call without it."""
    N = 101
    prob, _ = _references(Jr, Jc, N)
    base = wide_call(hip, prob, seg=11)
    for r in (0, 10, 11, 100):
        diag = prob["diag"].copy()
        diag[1, r:] = -1e9                 # (far below diag_add = sum a of the widest structure)
        got = wide_call(hip, prob, seg=11, diag=diag)
        assert got["info"][1] == r + 1 and got["info"][0] == 0 and got["info"][2] == 0, (r, got["info"])
        assert got["ll"][1] == -np.inf
        assert np.all(np.isnan(got["alpha"][1])) and np.all(np.isnan(got["mu"][1])), r
        assert _same(got, 0, base, 0) and _same(got, 2, base, 2), r
