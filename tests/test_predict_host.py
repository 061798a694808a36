"""CPU: the numpy restatement of gf_solve_batch's three passes (tests/solve_ref.solve_passes: checkpoints, segments
recomputed last first, the component's forward pass) against oracle/seq.py (factor, apply_inverse, predict_mean_at) at
every structure and length of tests/grad_cases.py and several segment lengths; the library's segment and workspace
formulas."""
import numpy as np
import pytest

from tests import grad_cases as gc
from tests.solve_ref import oracle_predict, solve_passes, split_component


def _segs(N):
    """1, 2, N, and (N > 2) the lengths that leave a last segment of one row and an exactly full one."""
    out = {1, 2, N}
    if N > 2:
        out.add(N - 1)                                  # last segment: one row
        out.add(-(-N // 2))                             # two segments, the last full when N is even
        out.update(k for k in range(2, N) if N % k == 0 and k > 2)
    return sorted(k for k in out if 1 <= k <= max(N, 2))


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_three_passes_match_the_oracle(Jr, Jc):
    worst = 0.0
    for N in gc.LENGTHS:
        prob = gc.edge_problem(Jr, Jc, N)
        jr, jc, r2, c2 = split_component(Jr, Jc, prob["real"], prob["comp"])
        b = N % prob["B"]
        co = gc.coefficients(prob, b)
        comp = (jr, jc, r2[0, b, :jr], r2[1, b, :jr]) + tuple(c2[i, b, :jc] for i in range(4))
        ref = oracle_predict(prob["t"], prob["y"][b], prob["diag"][b], co, prob["diag_add"][b], comp=comp[2:])
        assert ref["info"] == 0
        segs = _segs(N) if N <= 26 else [1, 7, N - 1, N]
        first = None
        for seg in segs:
            got = solve_passes(prob["t"], prob["y"][b], prob["diag"][b], Jr, Jc, co, prob["diag_add"][b], seg, comp)
            assert got["info"] == 0
            assert abs(got["ll"] - ref["ll"]) <= 1e-11 * abs(ref["ll"]), (N, seg)
            for k in ("alpha", "mu", "mu_comp"):
                e = _rel(got[k], ref[k])
                worst = max(worst, e)
                assert e < 1e-10, (N, seg, k, e)
            if first is None:
                first = got
            else:                                       # the recompute replays pass 1: nothing depends on seg
                assert all(np.array_equal(got[k], first[k]) for k in ("alpha", "mu", "mu_comp")), (N, seg)
    print(f"(Jr, Jc) = ({Jr}, {Jc}): worst error against oracle/seq.py {worst:.1e}")


def test_failing_pivot_and_null_diagonal():
    prob = gc.edge_problem(2, 7, 26)
    co = gc.coefficients(prob, 1)
    diag = prob["diag"][1].copy()
    diag[11:] = -1e6
    got = solve_passes(prob["t"], prob["y"][1], diag, 2, 7, co, prob["diag_add"][1], 5)
    ref = oracle_predict(prob["t"], prob["y"][1], diag, co, prob["diag_add"][1])
    assert got["info"] == ref["info"] == 12 and got["ll"] == -np.inf and np.all(np.isnan(got["alpha"]))
    free = solve_passes(prob["t"], prob["y"][1], None, 2, 7, co, 1.05 * prob["diag_add"][1], 5)
    assert np.array_equal(free["mu"], prob["y"][1])


def test_oracle_component_is_the_dense_product():
    """predict_mean_at at t* = t is K'(t, t) alpha with K' the component's dense matrix, its full diagonal k'(0)
    included (the coincident stamp counts) and no diagonal shift."""
    Jr, Jc, N = 1, 8, 17
    prob = gc.edge_problem(Jr, Jc, N)
    jr, jc, r2, c2 = split_component(Jr, Jc, prob["real"], prob["comp"])
    comp = (r2[0, 0, :jr], r2[1, 0, :jr]) + tuple(c2[i, 0, :jc] for i in range(4))
    ref = oracle_predict(prob["t"], prob["y"][0], prob["diag"][0], gc.coefficients(prob, 0), prob["diag_add"][0],
                         comp=comp)
    tau = np.abs(prob["t"][:, None] - prob["t"][None, :])
    Kc = sum(a * np.exp(-c * tau) for a, c in zip(comp[0], comp[1]))
    Kc = Kc + sum(np.exp(-c * tau) * (a * np.cos(d * tau) + b * np.sin(d * tau)) for a, b, c, d in zip(*comp[2:]))
    assert _rel(ref["mu_comp"], Kc @ ref["alpha"]) < 1e-11


def test_segment_and_workspace_formulas():
    from gadfly_amd import _lib
    lib = _lib.load()
    for N in (1, 2, 3, 64, 65, 197, 3000, 10 ** 5, 10 ** 9):
        for W, WM in ((1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (63, 64)):
            K = lib.gf_solve_batch_seg(N, W)
            assert 1 <= K <= N
            assert K == N or 3 * K * K >= N * (WM + 4)
            assert K == 1 or 3 * (K - 1) * (K - 1) < N * (WM + 4)
            n64 = -(-N // 64) * 64
            for seg in (0, 1, 2, K, N, N + 5):
                k = K if seg == 0 else min(seg, N)
                want = -(-N // k) * (WM + 4) * 64 + k * 3 * 64 + 2 * n64
                assert lib.gf_solve_batch_work(N, W, seg) == want, (N, W, seg)
        assert lib.gf_solve_batch_seg(N, 64) == 0 and lib.gf_solve_batch_work(N, 64, 0) == 0
        assert lib.gf_solve_batch_work(N, 8, -1) == 0
    assert lib.gf_solve_batch_seg(0, 8) == 0 and lib.gf_solve_batch_work(0, 8, 0) == 0
