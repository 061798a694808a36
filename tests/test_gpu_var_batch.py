"""GPU: BatchedLogLikelihood.predict(return_var=True), inverse_diagonal and leave_one_out -- the
conditional variances of B different kernels in one device call against GaussianProcess.predict(y, t, return_var=True)
one kernel at a time and against the dense inverse (tests/var_ref.py), at the observed times and at new ones in every
form ``t=`` takes; ragged data; yerr = 0; the means' bits; leave-one-out against deleting the row; the two
NotImplementedErrors; a problem that is not positive definite; run-to-run bit identity."""
import functools

import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.synth import uniform_times
from tests.predict_at_cases import kernels as _kernels, walkers as _walkers
from tests.var_ref import dense_reference, loo_reference

pytestmark = pytest.mark.gpu

N, B, J, YERR = 420, 4, 6, 30.0
CAD = 180.0                          # seconds: three exposure times, so that mid-interval queries stay 1.5 delta away
DT = CAD * 1e-6
GAP = (200, 40)                      # the series loses 40 cadences after row 200
DENSE = 1e-9                         # of max |reference| per problem: the bar of this kernel family's raw tests
#: against GaussianProcess, in units of K(0): its variance is K(0) minus a sum of that size through a stored factor, as
#: its means are a difference the existing tests hold to 1e-8
GP = 1e-8


def _axis(n=N, gap=GAP):
    t = uniform_times(n, CAD)
    t[gap[0]:] += gap[1] * DT
    return t


def _data(n=N, seed=8):
    return _axis(n), 100.0 * np.random.default_rng(seed).normal(size=n)


def _queries(t, gap_row=GAP[0]):
    """Sorted stamps at least 1.5 exposure times from every observed one: before the first row, after the last, inside
    the gap, and the midpoints of every seventh interval."""
    mid = 0.5 * (t[:-1] + t[1:])[::7]
    return np.sort(np.concatenate([t[0] - DT * np.array([30.0, 7.5, 1.5]), t[-1] + DT * np.array([1.5, 9.0, 40.0]),
                                   np.linspace(t[gap_row - 1] + 1.5 * DT, t[gap_row] - 1.5 * DT, 9), mid]))


def _problem():
    S0, w0, Q, delta = _walkers(B, J)
    t, y = _data()
    return _kernels(S0, w0, Q, delta), t, y


def _coefficients(kern):
    co = kern.get_device_coefficients()
    return co[:6], float(np.sum(co[0]) + np.sum(co[2]) + co[6])


@functools.lru_cache(maxsize=None)
def _reference():
    """The dense inverse for the B walkers on the gapped series, at the observed stamps and at the queries: computed
    once, shared, never changed."""
    kernels, t, y = _problem()
    ts = _queries(t)
    out = []
    for k in kernels:
        co, k0 = _coefficients(k)
        out.append(dense_reference(t, y, np.full(N, YERR ** 2), 0, J, co, k0, ts=ts))
    return tuple(out)


def _err(got, ref, scale=None):
    return float(np.max(np.abs(got - ref)) / (np.max(np.abs(ref)) if scale is None else scale))


def test_variances_at_the_observed_times_match_the_single_gp_and_the_dense_inverse():
    kernels, t, y = _problem()
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mu, var = ev.predict(return_var=True)
    assert mu.shape == var.shape == (B, N)
    assert np.all(ev.last_predict_info.cpu().numpy() == 0) and ev.last_predict_device_ms > 0.0
    assert ev.last_predict_plan[1] == 1 and np.all(np.isfinite(ev.last_predict_ll.cpu().numpy()))
    assert np.array_equal(mu, ev.predict())                          # the means keep their bits
    mu3, var3, alpha = ev.predict(return_var=True, return_alpha=True)
    assert np.array_equal(mu3, mu) and np.array_equal(var3, var)
    assert np.array_equal(alpha, ev.predict(return_alpha=True)[1])
    h = ev.inverse_diagonal()
    worst = dict(var=0.0, h=0.0, gp=0.0)
    for b, ref in enumerate(_reference()):
        k0 = _coefficients(kernels[b])[1]
        gm, gv = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=YERR, device="cuda:0").predict(y, return_var=True)
        e = dict(var=_err(var[b], ref["var"]), h=_err(h[b], ref["hdiag"]), gp=_err(var[b], gv, k0))
        worst = {k: max(worst[k], e[k]) for k in worst}
        assert _err(mu[b], gm) <= 1e-8
        assert np.all(var[b] > 0.0) and np.all(var[b] < YERR ** 2)
    print(f"observed times, J = {J}, N = {N}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["var"] <= DENSE and worst["h"] <= DENSE and worst["gp"] <= GP, worst
    dm, dv = ev.predict_device(return_var=True)
    assert dm.is_cuda and dv.is_cuda and np.array_equal(dv.cpu().numpy(), var)        # and from run to run
    assert np.array_equal(gadfly_amd.predict_batch(kernels, t, y, yerr=YERR, return_var=True)[1], var)
    pk = ev.pack(kernels)                                              # a device pack, a list of kernels
    assert np.array_equal(ev.predict(pk, return_var=True)[1], var)
    assert np.array_equal(ev.predict(kernels, return_var=True)[1], var)


def test_variances_at_new_times_in_every_form_of_t():
    kernels, t, y = _problem()
    ts = _queries(t)
    M = len(ts)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mu, var = ev.predict(t=ts, return_var=True)
    assert mu.shape == var.shape == (B, M)
    assert np.array_equal(mu, ev.predict(t=ts))                      # the means keep their bits
    assert 0.0 < ev.last_predict_at_ms < ev.last_predict_device_ms
    worst = dict(var=0.0, gp=0.0)
    for b, ref in enumerate(_reference()):
        k0 = _coefficients(kernels[b])[1]
        gm, gv = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=YERR,
                                            device="cuda:0").predict(y, t=ts, return_var=True)
        e = dict(var=_err(var[b], ref["var_at"]), gp=_err(var[b], gv, k0))
        worst = {k: max(worst[k], e[k]) for k in worst}
        assert _err(mu[b], gm) <= 1e-8
        assert np.all(var[b] > 0.0) and np.all(var[b] <= k0)
    print(f"new times, J = {J}, N = {N}, M = {M}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["var"] <= DENSE and worst["gp"] <= GP, worst
    # (B, M) stamps that happen to be equal, a list of series (a list back), lists of different lengths, an empty t
    assert np.array_equal(ev.predict(t=np.tile(ts, (B, 1)), return_var=True)[1], var)
    ml, vl = ev.predict(t=[ts] * B, return_var=True)
    assert isinstance(vl, list) and all(np.array_equal(a, b) for a, b in zip(vl, var))
    cuts = (M, 65, 1, 0)
    ml, vl, al = ev.predict(t=[ts[:c] for c in cuts], return_var=True, return_alpha=True)
    assert all(np.array_equal(vl[b], var[b, :c]) and np.array_equal(ml[b], mu[b, :c]) for b, c in enumerate(cuts))
    assert al.shape == (B, N)
    m0, v0 = ev.predict(t=np.empty(0), return_var=True)
    assert m0.shape == v0.shape == (B, 0)
    assert np.array_equal(gadfly_amd.predict_batch(kernels, t, y, yerr=YERR, t_pred=ts, return_var=True)[1], var)


def test_ragged_data_give_each_series_alone():
    """Missing-data rows (diag = 2^1000, at the end) add terms of order 2^-1000 to Y and S: each series of a ragged
    batch has the variances it has alone, to 1e-12 relative."""
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers(B, J))
    lens, mq = (300, 1, 133), (70, 5, 0)
    rng = np.random.default_rng(23)
    tb = [uniform_times(n, CAD) for n in lens]
    ys = [100.0 * rng.normal(size=n) + 2.5 for n in lens]
    qs = [np.sort(rng.uniform(x[0] - 20 * DT, x[-1] + 20 * DT, m)) for x, m in zip(tb, mq)]
    kernels = _kernels(S0, w0, Q, delta)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, tb, ys, yerr=YERR, mean=2.5)
    mu, var = ev.predict(return_var=True)
    mq_, vq = ev.predict(t=qs, return_var=True)
    h = ev.inverse_diagonal()
    lm, lv = ev.leave_one_out()
    plain = ev.predict()
    for b in range(3):
        one = gadfly_amd.BatchedLogLikelihood(kernels[b:b + 1], tb[b], ys[b], yerr=YERR, mean=2.5)
        m1, v1 = one.predict(return_var=True)
        assert var[b].shape == (lens[b],) and np.array_equal(mu[b], plain[b])
        assert np.allclose(var[b], v1[0], rtol=1e-12, atol=0.0) and np.allclose(mu[b], m1[0], rtol=1e-12, atol=1e-9)
        assert np.allclose(h[b], one.inverse_diagonal()[0], rtol=1e-12, atol=0.0)
        l1 = one.leave_one_out()
        assert np.allclose(lm[b], l1[0][0], rtol=1e-10, atol=1e-9) and np.allclose(lv[b], l1[1][0], rtol=1e-12)
        assert vq[b].shape == (mq[b],)
        if mq[b]:
            assert np.allclose(vq[b], one.predict(t=qs[b], return_var=True)[1][0], rtol=1e-12, atol=0.0)


def test_noise_free_data_have_zero_variance_at_the_observed_times():
    kernels, t, y = _problem()
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=0.0)
    mu, var = ev.predict(return_var=True)
    h = ev.inverse_diagonal()
    assert np.all(var == 0.0) and np.all(np.isfinite(h)) and np.all(h > 0.0)
    assert np.array_equal(mu, np.broadcast_to(y, (B, N)))
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y)               # no diagonal at all
    assert np.all(ev.predict(return_var=True)[1] == 0.0)


def test_leave_one_out_matches_deleting_the_row():
    n = 150
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers(B, J))
    kernels = _kernels(S0, w0, Q, delta)
    t, y = _data(n)
    mean = 4.0
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y + mean, yerr=YERR, mean=mean)
    lm, lv = ev.leave_one_out()
    lm0, _ = ev.leave_one_out(include_mean=False)
    dm, dv = ev.leave_one_out_device()
    assert dm.is_cuda and np.array_equal(dm.cpu().numpy(), lm) and np.array_equal(dv.cpu().numpy(), lv)
    for b, k in enumerate(kernels):
        co, k0 = _coefficients(k)
        rm, rv = loo_reference(t, y, np.full(n, YERR ** 2), 0, J, co, k0)
        assert np.max(np.abs(lm0[b] - rm)) <= DENSE * np.max(np.abs(y)), b
        assert np.max(np.abs(lm[b] - mean - rm)) <= DENSE * np.max(np.abs(y)), b
        assert np.max(np.abs(lv[b] - rv) / rv) <= DENSE, b


def test_component_and_width_limit_raise():
    t, y = _data()
    S0, w0, Q, delta = _walkers(2, J)
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=2)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    for kw in (dict(), dict(t=_queries(t))):
        with pytest.raises(NotImplementedError, match="inverse diagonal"):
            ev.predict(kernel=subs, return_var=True, **kw)
    S0, w0, Q, delta = _walkers(2, 32)
    ev = gadfly_amd.BatchedLogLikelihood(_kernels(S0, w0, Q, delta), t, y, yerr=YERR)
    for call in (lambda: ev.predict(return_var=True), lambda: ev.predict(t=_queries(t), return_var=True),
                 ev.inverse_diagonal, ev.leave_one_out):
        with pytest.raises(NotImplementedError, match="W = 64"):
            call()


def test_non_positive_definite_problem_is_isolated():
    kernels, t, y = _problem()
    ts = _queries(t)
    diag = np.full((B, N), YERR ** 2)
    clean = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag)
    cv, cq, ch = clean.predict(return_var=True)[1], clean.predict(t=ts, return_var=True)[1], clean.inverse_diagonal()
    diag[1, 300:] = -1e9
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag)
    mu, var = ev.predict(return_var=True)
    assert ev.last_predict_ll.cpu().numpy()[1] == -np.inf and ev.last_predict_info.cpu().numpy()[1] == 301
    mq, vq = ev.predict(t=ts, return_var=True)
    h = ev.inverse_diagonal()
    lm, lv = ev.leave_one_out()
    keep = [0, 2, 3]
    for got, ref in ((var, cv), (vq, cq), (h, ch)):
        assert np.all(np.isnan(got[1])) and np.array_equal(got[keep], ref[keep])
    assert all(np.all(np.isnan(x[1])) and np.all(np.isfinite(x[keep])) for x in (mu, mq, lm, lv))
