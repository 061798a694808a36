"""CPU: the numpy restatement of gf_var_batch's passes (tests/var_ref.var_passes: checkpoints, queries staged at their
owners, segments recomputed last first, the matrix recurrence Y) against the dense inverse and against its own 80-bit
run, at every structure of tests/grad_cases.py; the leave-one-out identities against a reference that deletes the row;
the library's workspace formula."""
import functools

import numpy as np
import pytest

from tests import grad_cases as gc
from tests.var_ref import dense_reference, loo_reference, var_passes, work_formula
from tests.var_ref import queries as var_ref_queries

LENGTHS = (1, 2, 3, 5, 17, 100, 197)

#: bars, a decade or two above what these cases measure (the docstring of test_passes_match_... holds the figures)
H_REL_80 = 2e-13            # h against the 80-bit pass, relative per row
VAR_DENSE = 3e-11           # observed-time variance against the dense inverse, in units of max diag
VAR_AT_DENSE = 1e-12        # new-time variance against the dense inverse, in units of K(0)
VAR_AT_80 = 1e-13           # ... and against the 80-bit pass
LOO_MEAN = 1e-12            # leave-one-out mean against the deleting reference, in units of max |y|
LOO_VAR = 1e-12             # leave-one-out variance, relative per row


def queries(t):
    return var_ref_queries(t, gc.DT)


def _lib_seg(N, W):
    from gadfly_amd import _lib
    return int(_lib.load().gf_solve_batch_seg(N, W))


@functools.lru_cache(maxsize=None)
def _case(Jr, Jc, N):
    prob = gc.edge_problem(Jr, Jc, N)
    b = N % prob["B"]
    ts = queries(prob["t"])
    args = (prob["t"], prob["y"][b], prob["diag"][b], Jr, Jc, gc.coefficients(prob, b), prob["diag_add"][b])
    return args, ts, dense_reference(*args, ts=ts), var_passes(*args, N, ts=ts, dtype=np.longdouble)


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_passes_match_the_dense_inverse_and_the_80_bit_run(Jr, Jc):
    """N in {1, 2, 3, 5, 17, 100, 197}, segments of one row, the library's length and the whole series.  Measured over
    all structures: h within 1.2e-14 relative of the 80-bit pass; the observed-time variance within 1.4e-12 max diag of
    the dense inverse (W = 2; 6e-13 elsewhere); the new-time variance within 5.3e-14 K(0) of the dense inverse (W = 2;
    2.5e-14 elsewhere) and 5.0e-15 K(0) of the 80-bit pass; alpha within 3.4e-14 of max |alpha| of the dense solve."""
    worst = dict(h80=0.0, var=0.0, at=0.0, at80=0.0, alpha=0.0)
    for N in LENGTHS:
        args, ts, dense, ext = _case(Jr, Jc, N)
        diag, k0 = args[2], args[6]
        first = None
        for seg in sorted({1, _lib_seg(N, Jr + 2 * Jc), N}):
            got = var_passes(*args, seg, ts=ts)
            assert got["info"] == 0
            e = dict(h80=float(np.max(np.abs(got["hdiag"] - ext["hdiag"]) / np.abs(ext["hdiag"]))),
                     var=float(np.max(np.abs(got["var"] - dense["var"])) / np.max(diag)),
                     at=float(np.max(np.abs(got["var_at"] - dense["var_at"])) / k0),
                     at80=float(np.max(np.abs(got["var_at"] - ext["var_at"])) / k0),
                     alpha=float(np.max(np.abs(got["alpha"] - dense["alpha"])) / np.max(np.abs(dense["alpha"]))))
            worst = {k: max(worst[k], e[k]) for k in worst}
            assert e["h80"] <= H_REL_80 and e["var"] <= VAR_DENSE and e["at"] <= VAR_AT_DENSE, (N, seg, e)
            assert e["at80"] <= VAR_AT_80 and e["alpha"] <= 1e-10, (N, seg, e)
            assert np.all(got["var_at"] > 0.0) and np.all(got["var_at"] <= k0 * (1 + 1e-12))
            if first is None:
                first = got
            else:                                       # the recompute replays pass 1: nothing depends on seg
                assert all(np.array_equal(got[k], first[k]) for k in ("alpha", "hdiag", "var", "var_at")), (N, seg)
    print(f"(Jr, Jc) = ({Jr}, {Jc}): " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_a_query_alone_and_queries_that_no_row_or_the_last_row_owns():
    Jr, Jc, N = 1, 8, 17
    args, ts, dense, _ = _case(Jr, Jc, N)
    full = var_passes(*args, 5, ts=ts)
    for m in range(len(ts)):                            # M = 1: a query's value does not depend on the others
        one = var_passes(*args, 5, ts=ts[m:m + 1])
        assert one["var_at"][0] == full["var_at"][m], m
    t, k0 = args[0], args[6]
    # far before the first row the prior variance K(0); at a stamp with diag = 0 nothing is left
    far = var_passes(*args, 5, ts=np.array([t[0] - 1e3]))
    assert abs(far["var_at"][0] - k0) <= 1e-12 * k0
    clean = var_passes(t, args[1], np.zeros(N), *args[3:6], 1.0000001 * k0, 5, ts=t.copy())
    assert np.all(clean["var"] == 0.0) and np.all(np.isfinite(clean["hdiag"]))


def test_missing_data_rows_at_the_end_change_nothing():
    """Rows of diag = 2^1000 behind the real ones (ragged batches): h, the variances and the queries of the real rows
    are those of the short problem to rounding, the queries after the last real row belong to it."""
    Jr, Jc, N, pad = 2, 7, 17, 6
    args, ts, _, _ = _case(Jr, Jc, N)
    t, y, diag = args[:3]
    tp = np.concatenate([t, t[-1] + gc.DT * np.arange(1, pad + 1)])
    yp, dp = np.concatenate([y, np.zeros(pad)]), np.concatenate([diag, np.full(pad, 2.0 ** 1000)])
    short = var_passes(*args, 5, ts=ts)
    for seg in (1, 5, N + pad):
        got = var_passes(tp, yp, dp, *args[3:], seg, ts=ts, nobs=N)
        for k in ("alpha", "hdiag", "var"):
            assert np.allclose(got[k][:N], short[k], rtol=1e-12, atol=0.0), (seg, k)
        assert np.allclose(got["var_at"], short["var_at"], rtol=1e-12, atol=0.0), seg
        assert np.all(np.isfinite(got["var"])) and np.all(np.isfinite(got["hdiag"]))


def test_failing_pivot():
    args, ts, _, _ = _case(2, 7, 17)
    diag = args[2].copy()
    diag[11:] = -1e6
    got = var_passes(args[0], args[1], diag, *args[3:], 5, ts=ts)
    assert got["info"] == 12 and got["ll"] == -np.inf
    assert all(np.all(np.isnan(got[k])) for k in ("alpha", "mu", "hdiag", "var", "var_at"))


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (2, 7), (1, 16), (3, 30)])
def test_leave_one_out_identities(Jr, Jc):
    """E[y_n | y_-n] = y_n - alpha_n / h_n and Var[y_n | y_-n] = 1 / h_n against deleting row n and predicting it.
    Measured: 2.6e-14 of max |y| and 1.3e-14 relative."""
    for N in (1, 2, 3, 17, 100):
        args, _, _, _ = _case(Jr, Jc, N)
        got = var_passes(*args, 7)
        mean, var = loo_reference(*args)
        y = args[1]
        em = float(np.max(np.abs((y - got["alpha"] / got["hdiag"]) - mean)) / np.max(np.abs(y)))
        ev = float(np.max(np.abs(1.0 / got["hdiag"] - var) / var))
        print(f"(Jr, Jc) = ({Jr}, {Jc}), N = {N}: leave-one-out mean {em:.1e}, variance {ev:.1e}")
        assert em <= LOO_MEAN and ev <= LOO_VAR, (N, em, ev)


def test_workspace_formula_and_zero_returns():
    from gadfly_amd import _lib
    lib = _lib.load()
    for N in (1, 2, 3, 64, 65, 197, 3000, 10 ** 5, 10 ** 9):
        for W in (1, 16, 17, 32, 33, 63):
            K = int(lib.gf_solve_batch_seg(N, W))
            for seg in (0, 1, 2, K, N, N + 5):
                for M in (0, 1, 64, 7222, N):
                    want = work_formula(N, W, M, seg, K)
                    assert lib.gf_var_batch_work(N, W, M, seg) == want, (N, W, M, seg)
                    WM = 16 if W <= 16 else 32 if W <= 32 else 64
                    assert want == lib.gf_solve_batch_work(N, W, seg) + WM * 64 + 64 * M
        assert lib.gf_var_batch_work(N, 64, 0, 0) == 0 and lib.gf_var_batch_work(N, 0, 0, 0) == 0
        assert lib.gf_var_batch_work(N, 8, -1, 0) == 0 and lib.gf_var_batch_work(N, 8, 0, -1) == 0
    assert lib.gf_var_batch_work(0, 8, 0, 0) == 0
