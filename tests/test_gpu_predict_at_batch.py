"""GPU: BatchedLogLikelihood.predict(t=...) / predict_batch(t_pred=...) -- conditional means of B
different kernels at new times in one device call against oracle/seq.py in float64 and against
GaussianProcess.predict(y, t=t*) one kernel at a time, with and without a component; t* = t against the call without
``t``; means; ragged data and ragged query lists; per-problem axes; a problem that is not positive definite; the
width limit; unsorted, misshapen and empty ``t``."""
import functools

import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.synth import uniform_times
from tests.predict_at_cases import J, YERR, kernels as _kernels, oracle_alpha, walkers as _walkers
from tests.predict_at_ref import oracle_at

pytestmark = pytest.mark.gpu

N, B, M = 3000, 5, 400
DT = 60e-6
GAP = (1400, 250)                     # the series loses 250 cadences after row 1400


def _err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def _axis(n=N, gap=GAP):
    t = uniform_times(n, 60.0)
    t[gap[0]:] += gap[1] * DT
    return t


def _data(n=N, seed=8, gap=GAP):
    return _axis(n, gap), 100.0 * np.random.default_rng(seed).normal(size=n)


def _queries(t, m=M, seed=5, gap_row=GAP[0]):
    """m sorted stamps: a twentieth before the first row and a twentieth after the last (up to 50 cadences out), a
    quarter inside the gap (its two ends among them), 3 in 20 coincident with observed rows, the rest between rows
    anywhere (m = 400: 20, 20, 100, 60 and 200)."""
    rng = np.random.default_rng(seed)
    parts = [t[0] - rng.uniform(0.0, 50.0, m // 20) * DT, t[-1] + rng.uniform(0.0, 50.0, m // 20) * DT,
             np.linspace(t[gap_row - 1], t[gap_row], m // 4), rng.choice(t, size=3 * m // 20, replace=False)]
    parts.append(rng.uniform(t[0], t[-1], m - sum(len(p) for p in parts)))
    return np.sort(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def _reference():
    """oracle/seq.py in float64 for the B walkers on the gapped series: alpha, then the full kernel's and the
    component's (the first third of the terms) means at the query stamps.  Computed once, never changed."""
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    ts = _queries(t)
    out = []
    for k, s in zip(_kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)):
        alpha = oracle_alpha(k, t, y, np.full(N, YERR ** 2))
        out.append(dict(alpha=alpha, mu=oracle_at(t, ts, k.get_device_coefficients()[:6], alpha),
                        mu_comp=oracle_at(t, ts, s.get_device_coefficients()[:6], alpha)))
    return tuple(out)


def test_walkers_at_new_times_match_the_oracle_and_the_single_gp():
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    ts = _queries(t)
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mu, alpha = ev.predict(t=ts, return_alpha=True)
    assert mu.shape == (B, M) and alpha.shape == (B, N)
    assert np.all(ev.last_predict_info.cpu().numpy() == 0) and ev.last_predict_device_ms > 0.0
    assert 0.0 < ev.last_predict_at_ms < ev.last_predict_device_ms          # the solve and the new launch
    tl = ev.predict(t=[ts] * B)                              # a list of series, equal lengths or not: a list back
    assert isinstance(tl, list) and all(np.array_equal(x, m) for x, m in zip(tl, mu))
    mc = ev.predict(kernel=subs, t=ts)
    worst = dict(alpha=0.0, mu=0.0, mu_comp=0.0, gp=0.0, gp_comp=0.0)
    for b, ref in enumerate(_reference()):
        e = dict(alpha=_err(alpha[b], ref["alpha"]), mu=_err(mu[b], ref["mu"]), mu_comp=_err(mc[b], ref["mu_comp"]))
        gp = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=YERR, device="cuda:0")
        e["gp"], e["gp_comp"] = _err(mu[b], gp.predict(y, t=ts)), _err(mc[b], gp.predict(y, t=ts, kernel=subs[b]))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print("walkers at t*, J = 30, N = 3000, M = 400: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(worst[k] <= 1e-9 for k in ("alpha", "mu", "mu_comp")), worst
    assert worst["gp"] <= 1e-8 and worst["gp_comp"] <= 1e-8, worst
    # (B, M) stamps that happen to be equal, one component for all problems, the device form, the one-shot form
    assert np.array_equal(ev.predict(t=np.tile(ts, (B, 1))), mu)
    assert np.array_equal(ev.predict(kernel=subs[2], t=ts)[2], mc[2])
    dev = ev.predict_device(t=ts)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), mu)
    assert np.array_equal(gadfly_amd.predict_batch(kernels, t, y, yerr=YERR, t_pred=ts), mu)


def test_observed_stamps_as_queries_are_the_call_without_t():
    """kernel=component at t* = t is the component's share at the observed stamps: the same two sums (the state
    decays by the same factors; the order of one product differs)."""
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    here = ev.predict_device(kernel=subs).cpu().numpy()
    there = ev.predict_device(kernel=subs, t=t).cpu().numpy()
    e = [float(np.max(np.abs(a - b)) / np.max(np.abs(a))) for a, b in zip(here, there)]
    print(f"t* = t against the call without t: {max(e):.1e}")
    assert max(e) <= 1e-12, e


def test_means_and_a_row_varying_mean():
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    ts = _queries(t)
    kernels = _kernels(S0, w0, Q, delta)
    refs = _reference()
    for mean in (7.0, np.linspace(-3.0, 5.0, B)[:, None]):
        ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y[None, :] + mean, yerr=YERR, mean=mean)
        with_mean, without = ev.predict(t=ts), ev.predict(t=ts, include_mean=False)
        m = np.broadcast_to(mean, (B, 1))
        for b, ref in enumerate(refs):
            scale = np.max(np.abs(ref["mu"]))
            assert np.max(np.abs(without[b] - ref["mu"])) <= 1e-9 * scale
            assert np.max(np.abs(with_mean[b] - (ref["mu"] + m[b]))) <= 1e-9 * scale
    trend = np.linspace(0.0, 1.0, N)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y + trend, yerr=YERR, mean=trend)
    with pytest.raises(ValueError, match="mean"):
        ev.predict(t=ts)
    assert ev.predict(t=ts, include_mean=False).shape == (B, M)
    assert ev.predict().shape == (B, N)                      # (at the observed stamps such a mean is known)


def test_ragged_data_and_ragged_queries_give_each_series_alone_to_the_bit():
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers())
    lens, mq = (700, 1, 333), (150, 65, 0)
    rng = np.random.default_rng(23)
    tb = [uniform_times(n, 60.0) for n in lens]
    ys = [100.0 * rng.normal(size=n) + 2.5 for n in lens]
    qs = [np.sort(rng.uniform(x[0] - 20 * DT, x[-1] + 20 * DT, m)) for x, m in zip(tb, mq)]
    qs[0][10:14] = tb[0][[100, 100, 101, 350]]                        # coincident stamps, one of them twice
    qs[0].sort()
    means = np.array([2.5, 2.0, 3.0])
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, tb, ys, yerr=YERR, mean=means)
    mu, alpha = ev.predict(t=qs, return_alpha=True)
    mc = ev.predict(kernel=subs, t=qs, include_mean=False)
    assert [len(x) for x in mu] == list(mq) == [len(x) for x in mc] and [len(x) for x in alpha] == list(lens)
    shared = ev.predict(t=qs[1])                                      # one (M,) axis for ragged data: (B, M)
    assert shared.shape == (3, mq[1]) and np.array_equal(shared[1], mu[1])
    for b in range(3):
        one = gadfly_amd.BatchedLogLikelihood(kernels[b:b + 1], tb[b], ys[b], yerr=YERR, mean=float(means[b]))
        if mq[b] == 0:
            assert one.predict(t=qs[b]).shape == (1, 0)
            continue
        m1, a1 = one.predict(t=qs[b], return_alpha=True)
        assert np.array_equal(m1[0], mu[b]) and np.array_equal(a1[0], alpha[b]), b
        assert np.array_equal(one.predict(kernel=subs[b], t=qs[b], include_mean=False)[0], mc[b]), b
    # a ragged query list for rectangular data
    t, y = _data(900, gap=(400, 30))
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    q2 = [_queries(t, m, seed=m, gap_row=400) for m in (210, 300, 250)]
    got = ev.predict(t=q2)
    for b in range(3):
        assert np.array_equal(got[b], ev.predict(t=q2[b])[b]), b


def test_per_problem_axes():
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers())
    n, m = 1500, 300
    rng = np.random.default_rng(17)
    t0 = _axis(n, (700, 40))
    tb = np.stack([t0, t0 * 1.01, t0 + rng.uniform(-0.1, 0.1, n) * DT])
    ys = 100.0 * rng.normal(size=(3, n))
    diag = YERR ** 2 * rng.uniform(0.8, 1.2, (3, n))
    qb = np.stack([_queries(tb[b], m, seed=b, gap_row=700) for b in range(3)])
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, tb, ys, diag=diag)
    mu, mc = ev.predict(t=qb), ev.predict(kernel=subs, t=qb)
    for b in range(3):
        alpha = oracle_alpha(kernels[b], tb[b], ys[b], diag[b])
        e = [_err(mu[b], oracle_at(tb[b], qb[b], kernels[b].get_device_coefficients()[:6], alpha)),
             _err(mc[b], oracle_at(tb[b], qb[b], subs[b].get_device_coefficients()[:6], alpha))]
        print(f"problem {b}: mu {e[0]:.1e}, mu' {e[1]:.1e}")
        assert max(e) <= 1e-9, (b, e)
        one = gadfly_amd.BatchedLogLikelihood(kernels[b:b + 1], tb[b], ys[b], diag=diag[b])
        assert np.array_equal(one.predict(t=qb[b])[0], mu[b])


def test_non_positive_definite_problem_is_isolated():
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers(j=6))
    n = 900
    t, y = _data(n, gap=(400, 30))
    ts = _queries(t, 200, gap_row=400)
    diag = np.full((3, n), YERR ** 2)
    kernels = _kernels(S0, w0, Q, delta)
    clean = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag).predict(t=ts)
    diag[1, 500:] = -1e9
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag)
    mu = ev.predict(t=ts)
    assert np.all(np.isnan(mu[1])) and np.array_equal(mu[[0, 2]], clean[[0, 2]])
    assert ev.last_predict_ll.cpu().numpy()[1] == -np.inf and ev.last_predict_info.cpu().numpy()[1] == 501


def test_width_limit_and_the_checks_of_t():
    t, y = _data(500, gap=(200, 30))
    ts = _queries(t, 100, gap_row=200)
    S0, w0, Q, delta = _walkers(2, 86)
    ev = gadfly_amd.BatchedLogLikelihood(_kernels(S0, w0, Q, delta), t, y, yerr=YERR)
    with pytest.raises(NotImplementedError, match="W = 172"):
        ev.predict(t=ts)
    S0, w0, Q, delta = _walkers(2, 6)
    kernels = _kernels(S0, w0, Q, delta)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    with pytest.raises(ValueError, match="The input coordinates must be sorted"):
        ev.predict(t=ts[::-1])
    with pytest.raises(ValueError, match="The input coordinates must be sorted"):
        ev.predict(t=[ts, ts[:50][::-1]])
    with pytest.raises(ValueError):                                   # three axes for two problems
        ev.predict(t=np.tile(ts, (3, 1)))
    with pytest.raises(ValueError):                                   # three series of stamps for two problems
        ev.predict(t=[ts, ts[:50], ts[:20]])
    # an empty t: an empty result, alpha and the log-likelihoods as ever, only the solve launched
    mu, alpha = ev.predict(t=np.empty(0), return_alpha=True)
    assert mu.shape == (2, 0) and alpha.shape == (2, 500) and np.all(np.isfinite(alpha))
    assert ev.last_predict_at_ms == 0.0 < ev.last_predict_device_ms          # only the solve launched
    assert np.all(np.isfinite(ev.last_predict_ll.cpu().numpy()))
    assert [x.shape for x in ev.predict(t=[np.empty(0), ts[:7]])] == [(0,), (7,)]
    good = ev.predict(t=ts)                                           # the evaluator is still usable
    assert good.shape == (2, 100) and np.all(np.isfinite(good))
