"""CPU: the numpy restatement of gf_predict_batch_at's two sweeps (tests/predict_at_ref.sweeps: the sorted axes merged,
the state stepping from observed stamp to observed stamp, queries that only read it) against oracle/seq.predict_mean_at
and, on zero-based axes, the dense kernel_value(t* - t) @ alpha, at every structure of tests/grad_cases.py and every
length of predict_at_ref.LENGTHS with the query design of predict_at_ref.queries; ``nobs`` / ``nq``; the design itself;
the host layer's checks that need no device."""
import numpy as np
import pytest

from tests import grad_cases as gc
from tests import predict_at_ref as pr

BAR = 1e-9            # of max |reference| per problem: the bar of tests/test_gpu_predict_edges.py


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def test_query_design_holds_every_position():
    for N in pr.LENGTHS:
        t = gc.edge_problem(0, 8, N)["t"]
        ts = pr.queries(t, 1)
        assert ts.shape == (pr.M_DESIGN,) and np.all(np.diff(ts) >= 0.0)
        assert np.sum(ts == t[0] - 2.5 * gc.DT) == 2 and np.sum(ts > t[-1]) >= 2
        assert np.sum(np.isin(ts, t)) >= min(N, 16)
        if N >= 2:
            k = N // 3
            assert np.sum((ts >= t[k]) & (ts <= t[k + 1])) >= 70 > 64
            assert np.sum(ts == t[k]) >= 1 and np.sum(ts == t[k + 1]) >= 1
    for M in (1, 64, 65, 150):
        idx = pr.pick(M)
        assert len(idx) == M and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < pr.M_DESIGN


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_two_sweeps_match_the_oracle_and_the_dense_product(Jr, Jc):
    worst = dict(seq=0.0, dense=0.0)
    for N in pr.LENGTHS:
        ref = pr.reference(Jr, Jc, N)
        prob = ref["prob"]
        for b in range(prob["B"]):
            co = gc.coefficients(prob, b)
            got = pr.sweeps(prob["t"], ref["ts"][b], Jr, Jc, co, ref["alpha"][b])
            e = dict(seq=_rel(got, ref["mu"][b]),
                     dense=_rel(got, pr.dense_at(prob["t"], ref["ts"][b], co, ref["alpha"][b])))
            worst = {k: max(worst[k], e[k]) for k in worst}
            assert e["seq"] <= BAR and e["dense"] <= BAR, (N, b, e)
    print(f"(Jr, Jc) = ({Jr}, {Jc}): worst error against oracle/seq.py {worst['seq']:.1e}, against the dense product "
          f"{worst['dense']:.1e}")


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (2, 7), (1, 31)])
def test_jd_axis_against_the_float64_oracle(Jr, Jc):
    """t + 2454833 d: the dense form rounds d (t* - t) where the sweeps and the oracle round d t* and d t (a phase
    quantum of ~1e-7 rad there), so the float64 oracle alone is the reference."""
    for N in (3, 65, 197):
        ref = pr.reference(Jr, Jc, N, jd=True)
        prob = ref["prob"]
        for b in range(prob["B"]):
            got = pr.sweeps(prob["t"], ref["ts"][b], Jr, Jc, gc.coefficients(prob, b), ref["alpha"][b])
            assert _rel(got, ref["mu"][b]) <= BAR, (N, b)


@pytest.mark.parametrize("Jr,Jc", [(0, 1), (2, 7), (3, 30)])
def test_counts_are_the_shorter_problem(Jr, Jc):
    """nobs / nq: the first rows and the first queries alone, bit for bit; nothing from nobs / nq on is looked at."""
    N = 130
    ref = pr.reference(Jr, Jc, N)
    prob = ref["prob"]
    co = gc.coefficients(prob, 1)
    t, ts, alpha = prob["t"], ref["ts"][1], ref["alpha"][1]
    for nobs, nq in ((1, 150), (64, 65), (65, 64), (130, 1), (77, 0), (0, 20), (500, 500), (-3, 10)):
        no, mq = min(max(nobs, 0), N), min(max(nq, 0), pr.M_DESIGN)
        tt, aa, qq = t.copy(), alpha.copy(), ts.copy()
        tt[no:], aa[no:], qq[mq:] = np.nan, np.nan, np.nan
        got = pr.sweeps(tt, qq, Jr, Jc, co, aa, nobs=nobs, nq=nq, fill=-7.0)
        assert np.all(got[mq:] == -7.0)
        if no and mq:
            assert np.array_equal(got[:mq], pr.sweeps(t[:no], ts[:mq], Jr, Jc, co, alpha[:no]))
            assert _rel(got[:mq], pr.oracle_at(t[:no], ts[:mq], co, alpha[:no])) <= BAR
        else:
            assert np.all(got[:mq] == 0.0)


def test_a_query_does_not_depend_on_the_others():
    ref = pr.reference(1, 8, 65)
    prob = ref["prob"]
    co = gc.coefficients(prob, 2)
    full = pr.sweeps(prob["t"], ref["ts"][2], 1, 8, co, ref["alpha"][2])
    for M in (1, 64, 65):
        idx = pr.pick(M)
        assert np.array_equal(pr.sweeps(prob["t"], ref["ts"][2][idx], 1, 8, co, ref["alpha"][2]), full[idx])


def test_signature_and_width_limit():
    from gadfly_amd import _lib
    from gadfly_amd.predict import check_width
    res, args = _lib.SIGNATURES["gf_predict_batch_at"]
    assert res is _lib._int and len(args) == 22
    lib = _lib.load()
    # argument checks come before any launch: no device needed
    assert lib.gf_predict_batch_at(1, 5, 5, 0, 32, *([None] * 6), None, 0, None, None, 0, None, None, 5, None, 5,
                                   None) == -3 and "63" in _lib.last_error()
    assert lib.gf_predict_batch_at(1, 5, 0, 0, 8, *([None] * 6), None, 0, None, None, 0, None, None, 5, None, 5,
                                   None) == -1 and "M=0" in _lib.last_error()
    assert lib.gf_predict_batch_at(1, 5, 5, 0, 8, *([None] * 6), None, 0, None, None, 0, None, None, 5, None, 5,
                                   None) == -1 and "null" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        check_width(64)
