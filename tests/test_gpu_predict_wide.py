"""GPU: the wide conditional-mean route through the public interface --
BatchedLogLikelihood.predict(..., wide=True) on three stars of gadfly's 86-term kernel (W = 172) against oracle/seq.py in
float64 and against GaussianProcess.predict one kernel at a time; the granulation's and the p-modes' shares; new times
as an array, per problem and as a list; a ragged batch; groups under a workspace cap; a narrow batch against the
default route; what still raises; a matrix that is not positive definite among healthy ones."""
import functools

import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.batch import sho_coefficient_pack
from gadfly_amd.synth import solar_like_hyperparameters
from tests import random_cases as rc
from tests.predict_at_ref import oracle_at
from tests.solve_ref import oracle_predict

pytestmark = pytest.mark.gpu

B, N, J, NG = 3, 300, 86, 5             # NG granulation terms in front of the J - NG p-modes
DELTA = 60e-6
YERR = 25.0


def _params(j=J, b=B, seed=86):
    """(S0, w0, Q) (b, j): the solar-like kernel's own parameters, each problem's a few per cent off."""
    rng = np.random.default_rng(seed)
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(min(j, J)), texp=60.0)
    S0, w0, Q = (np.array([[getattr(x, n) for x in kern.term.terms]] * b) for n in ("S0", "w0", "Q"))
    if j > J:                           # (more terms than the table holds: its last modes again, a little higher)
        S0, w0, Q = (np.concatenate([x, f * x[:, J - j:]], axis=1) for x, f in ((S0, 1.0), (w0, 1.3), (Q, 1.0)))
    for x in (S0, w0, Q):
        x *= rng.uniform(0.95, 1.05, x.shape)
    assert np.all(Q >= 0.5)
    return S0, w0, Q


def _co(kern):
    co = kern.get_device_coefficients()
    return co[:6], float(np.sum(co[0]) + np.sum(co[2]) + co[6])


@functools.lru_cache(maxsize=None)
def _solar(cadence):
    """Three stars on N = 300 rows at ``cadence`` seconds with a gap, white noise of 25, and oracle/seq.py in float64
    for each: computed once, shared, never changed."""
    rng = np.random.default_rng([87, int(cadence)])
    S0, w0, Q = _params()
    t = np.arange(N) * cadence * 1e-6
    t[N // 2:] += 37 * cadence * 1e-6
    y = rng.normal(size=(B, N)) * 40.0
    kernels = rc.sho_kernels(S0, w0, Q, DELTA)
    refs = []
    for b, k in enumerate(kernels):
        co, da = _co(k)
        refs.append(oracle_predict(t, y[b], np.full(N, YERR ** 2), co, da))
        assert refs[-1]["info"] == 0
    return S0, w0, Q, t, y, kernels, tuple(refs)


def _parts(S0, w0, Q):
    """(granulation kernels, p-mode kernels): W' = 10 and W' = 162."""
    return (rc.sho_kernels(S0[:, :NG], w0[:, :NG], Q[:, :NG], DELTA),
            rc.sho_kernels(S0[:, NG:], w0[:, NG:], Q[:, NG:], DELTA))


def _err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("cadence", [60.0, 1765.0])
def test_solar_kernels_match_the_oracle_and_the_single_gp(cadence):
    S0, w0, Q, t, y, kernels, refs = _solar(cadence)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    assert ev.engine._struct0 == (0, J)
    with pytest.raises(NotImplementedError, match="W = 172"):
        ev.predict()
    mu, alpha = ev.predict(return_alpha=True, wide=True)
    assert mu.shape == alpha.shape == (B, N) and ev.last_predict_plan[1] == 1
    ll = ev.last_predict_ll.cpu().numpy()
    assert np.all(ev.last_predict_info.cpu().numpy() == 0)
    assert np.array_equal(ev.predict(wide=True), mu)
    # kernels and a host pack are the same coefficients: the same bits; so is the one-shot form
    for pk in (kernels, sho_coefficient_pack(S0, w0, Q, DELTA)):
        m2, a2 = ev.predict(pk, return_alpha=True, wide=True)
        assert np.array_equal(m2, mu) and np.array_equal(a2, alpha)
    assert np.array_equal(gadfly_amd.predict_batch(kernels, t, y, yerr=YERR, wide=True), mu)
    worst = dict(alpha=0.0, mu=0.0, ll=0.0, gp=0.0)
    for b, ref in enumerate(refs):
        e = dict(alpha=_err(alpha[b], ref["alpha"]), mu=_err(mu[b], ref["mu"]),
                 ll=abs(ll[b] - ref["ll"]) / abs(ref["ll"]))
        gp = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=YERR, device="cuda:0")
        e["gp"] = _err(mu[b], gp.predict(y[b]))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print(f"solar kernels, {cadence:.0f} s cadence: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(worst[k] <= 1e-9 for k in ("alpha", "mu", "ll")), worst
    assert worst["gp"] <= 1e-8, worst
    # a scalar mean and one per problem
    for mean in (7.0, np.linspace(-3.0, 5.0, B)[:, None]):
        em = gadfly_amd.BatchedLogLikelihood(kernels, t, y + mean, yerr=YERR, mean=mean)
        with_mean, without = em.predict(wide=True), em.predict(include_mean=False, wide=True)
        m = np.broadcast_to(mean, (B, 1))
        for b, ref in enumerate(refs):
            scale = np.max(np.abs(ref["mu"]))
            assert np.max(np.abs(without[b] - ref["mu"])) <= 1e-9 * scale
            assert np.max(np.abs(with_mean[b] - (ref["mu"] + m[b]))) <= 1e-9 * scale


@pytest.mark.parametrize("cadence", [60.0, 1765.0])
def test_shares_of_the_granulation_and_of_the_p_modes(cadence):
    S0, w0, Q, t, y, kernels, refs = _solar(cadence)
    gran, modes = _parts(S0, w0, Q)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mg, alpha = ev.predict(kernel=gran, wide=True, return_alpha=True)
    assert len(ev._predict_at_events) == 1                    # W' = 10: one group
    mp = ev.predict(kernel=modes, wide=True)
    assert len(ev._predict_at_events) == 3                    # W' = 162: three groups
    whole = ev.predict(t=t, wide=True, include_mean=False)
    assert len(ev._predict_at_events) == 3                    # W = 172: three groups
    worst = [0.0, 0.0, 0.0]
    for b, ref in enumerate(refs):
        e = [_err(mg[b], oracle_at(t, t, _co(gran[b])[0], ref["alpha"])),
             _err(mp[b], oracle_at(t, t, _co(modes[b])[0], ref["alpha"])),
             float(np.max(np.abs(mg[b] + mp[b] - whole[b])) / np.max(np.abs(whole[b])))]
        worst = [max(a, x) for a, x in zip(worst, e)]
    print(f"shares, {cadence:.0f} s cadence: granulation {worst[0]:.1e}, p-modes {worst[1]:.1e}, "
          f"sum against the whole {worst[2]:.1e}")
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9 and worst[2] <= 1e-12, worst
    # a host pack as the component, one kernel for all problems, the mean added as on the narrow route
    pk = sho_coefficient_pack(S0[:, NG:], w0[:, NG:], Q[:, NG:], DELTA)
    assert np.array_equal(ev.predict(kernel=pk, wide=True), mp)
    assert np.array_equal(ev.predict(kernel=modes[2], wide=True)[2], mp[2])
    em = gadfly_amd.BatchedLogLikelihood(kernels, t, y + 3.0, yerr=YERR, mean=3.0)
    bare = em.predict(kernel=gran, wide=True, include_mean=False)
    assert max(_err(bare[b], mg[b]) for b in range(B)) <= 1e-12       # ((y + 3) - 3 is y to rounding only)
    assert np.array_equal(em.predict(kernel=gran, wide=True), bare + 3.0)


def _queries(t, rng, M):
    """M sorted stamps: before the first row, between rows, on rows, after the last."""
    dt = t[1] - t[0]
    q = np.concatenate([[t[0] - 2.5 * dt, t[0] - 2.5 * dt], rng.choice(t, size=min(5, M // 4), replace=False),
                        [t[-1] + 0.7 * dt, t[-1] + 40.0 * dt]])
    return np.sort(np.concatenate([q, rng.uniform(t[0] - dt, t[-1] + dt, M - len(q))]))


@pytest.mark.parametrize("cadence", [60.0, 1765.0])
def test_new_times(cadence):
    S0, w0, Q, t, y, kernels, refs = _solar(cadence)
    gran, _ = _parts(S0, w0, Q)
    rng = np.random.default_rng(11)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y + 2.0, yerr=YERR, mean=2.0)
    worst = 0.0
    # (M,) shared
    ts = _queries(t, rng, 70)
    mu, alpha = ev.predict(t=ts, wide=True, return_alpha=True)
    assert mu.shape == (B, 70) and alpha.shape == (B, N)
    mc = ev.predict(t=ts, wide=True, kernel=gran, include_mean=False)
    for b, ref in enumerate(refs):
        want = oracle_at(t, ts, _co(kernels[b])[0], ref["alpha"])
        worst = max(worst, _err(alpha[b], ref["alpha"]), _err(mu[b] - 2.0, want),
                    _err(mc[b], oracle_at(t, ts, _co(gran[b])[0], ref["alpha"])))
    # (B, M) per problem
    tb = np.stack([_queries(t, rng, 33) for _ in range(B)])
    mu = ev.predict(t=tb, wide=True, include_mean=False)
    assert mu.shape == (B, 33)
    for b, ref in enumerate(refs):
        worst = max(worst, _err(mu[b], oracle_at(t, tb[b], _co(kernels[b])[0], ref["alpha"])))
    # a list of three series of different lengths, one of them empty
    tl = [_queries(t, rng, 40), np.zeros(0), _queries(t, rng, 9)]
    mu = ev.predict(t=tl, wide=True, include_mean=False)
    assert [len(x) for x in mu] == [40, 0, 9]
    for b in (0, 2):
        worst = max(worst, _err(mu[b], oracle_at(t, tl[b], _co(kernels[b])[0], refs[b]["alpha"])))
    print(f"new times, {cadence:.0f} s cadence: {worst:.1e}")
    assert worst <= 1e-9
    empty = ev.predict(t=np.zeros(0), wide=True)
    assert empty.shape == (B, 0)


def test_ragged_batch_gives_each_series_alone_to_the_bit():
    S0, w0, Q, t, y, kernels, _ = _solar(60.0)
    gran, _ = _parts(S0, w0, Q)
    lens = (300, 1, 133)
    ts = [t[:n].copy() for n in lens]
    ys = [y[b, :n] + 2.5 for b, n in enumerate(lens)]
    means = np.array([2.5, 2.0, 3.0])
    tq = [t[:7] + 1e-6, t[:1], t[100:140] - 2e-6]
    ev = gadfly_amd.BatchedLogLikelihood(kernels, ts, ys, yerr=YERR, mean=means)
    mu, alpha = ev.predict(return_alpha=True, wide=True)
    mc = ev.predict(kernel=gran, include_mean=False, wide=True)
    mq = ev.predict(t=tq, wide=True)
    ll = ev.last_predict_ll.cpu().numpy()
    assert [len(x) for x in mu] == list(lens) == [len(x) for x in alpha] == [len(x) for x in mc]
    assert [len(x) for x in mq] == [7, 1, 40]
    for b, n in enumerate(lens):
        one = gadfly_amd.BatchedLogLikelihood(kernels[b:b + 1], ts[b], ys[b], yerr=YERR, mean=float(means[b]))
        m1, a1 = one.predict(return_alpha=True, wide=True)
        assert np.array_equal(m1[0], mu[b]) and np.array_equal(a1[0], alpha[b]), b
        assert np.array_equal(one.predict(kernel=gran[b], include_mean=False, wide=True)[0], mc[b]), b
        assert np.array_equal(one.predict(t=tq[b], wide=True)[0], mq[b]), b
        l1 = one.last_predict_ll.cpu().numpy()[0]
        # the pad rows' constants come off again: each of the npad pad rows added log 2^1000 to a running sum of the
        # size of their total, one rounding of that sum per row at most
        npad = max(lens) - n
        pad_total = 0.5 * npad * (1000.0 * np.log(2.0) + np.log(2.0 * np.pi))
        assert abs(ll[b] - l1) <= 1e-12 * abs(l1) + npad * np.spacing(pad_total), (b, ll[b], l1)


def test_groups_under_a_workspace_cap():
    S0, w0, Q, t, y, kernels, _ = _solar(60.0)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mu, alpha = ev.predict(return_alpha=True, wide=True)
    mq = ev.predict(t=t[:50] + 1e-6, wide=True)
    per = gadfly_amd._lib.load().gf_solve_wide_work(N, 2 * J, 0)
    assert ev.last_predict_plan == (8 * per * B, 1, B)
    ev.predict_workspace_bytes = 8 * per
    m3, a3 = ev.predict(return_alpha=True, wide=True)
    assert ev.last_predict_plan == (8 * per, 3, 1)
    assert np.array_equal(m3, mu) and np.array_equal(a3, alpha)
    assert np.array_equal(ev.predict(t=t[:50] + 1e-6, wide=True), mq)


def test_narrow_batch_agrees_with_the_default_route():
    S0, w0, Q = _params(j=6)
    _, _, _, t, y, _, _ = _solar(60.0)
    kernels = rc.sho_kernels(S0, w0, Q, DELTA)
    subs = rc.sho_kernels(S0[:, :2], w0[:, :2], Q[:, :2], DELTA)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    ts = t[:40] + 1e-6
    for kw in (dict(), dict(kernel=subs), dict(t=ts), dict(t=ts, kernel=subs)):
        m0, a0 = ev.predict(return_alpha=True, **kw)
        l0 = ev.last_predict_ll.cpu().numpy()
        m1, a1 = ev.predict(return_alpha=True, wide=True, **kw)
        l1 = ev.last_predict_ll.cpu().numpy()
        for b in range(B):
            assert _err(m1[b], m0[b]) <= 1e-10 and _err(a1[b], a0[b]) <= 1e-10, (kw.keys(), b)
        assert np.all(np.abs(l1 - l0) <= 1e-10 * np.abs(l0))


def test_what_still_raises():
    S0, w0, Q, t, y, kernels, _ = _solar(60.0)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    for kw in (dict(), dict(t=t[:5]), dict(return_var=True)):
        with pytest.raises(NotImplementedError, match="W = 172"):
            ev.predict(**kw)
    with pytest.raises(NotImplementedError, match="variances of wide kernels are not built"):
        ev.predict(return_var=True, wide=True)
    with pytest.raises(NotImplementedError, match="variances of wide kernels are not built"):
        ev.predict(return_var=True, wide=True, t=t[:5])
    S97, w97, Q97 = _params(j=97, b=2)
    big = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S97, w97, Q97, DELTA), t, y[:2], yerr=YERR)
    with pytest.raises(NotImplementedError, match="W <= 192.*W = 194"):
        big.predict(wide=True)
    with pytest.raises(NotImplementedError, match="192.*the component has W = 194"):
        ev.predict(kernel=rc.sho_kernels(S97[:1], w97[:1], Q97[:1], DELTA)[0], wide=True)
    with pytest.raises(ValueError):                                   # two components for three problems
        ev.predict(kernel=_parts(S0, w0, Q)[0][:2], wide=True)
    mu = ev.predict(wide=True)                                        # the evaluator is still usable
    assert mu.shape == (B, N) and np.all(np.isfinite(mu))


def test_non_positive_definite_problem_is_isolated():
    S0, w0, Q, t, y, kernels, _ = _solar(60.0)
    gran, _ = _parts(S0, w0, Q)
    diag = np.full((B, N), YERR ** 2)
    clean = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag).predict(wide=True)
    diag[1, 200:] = -1e9
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag)
    mu = ev.predict(wide=True)
    assert np.all(np.isnan(mu[1])) and np.array_equal(mu[[0, 2]], clean[[0, 2]])
    assert ev.last_predict_ll.cpu().numpy()[1] == -np.inf and ev.last_predict_info.cpu().numpy()[1] == 201
    assert np.all(np.isnan(ev.predict(kernel=gran, wide=True)[1]))
    assert np.all(np.isnan(ev.predict(t=t[:9] + 1e-6, wide=True)[1]))
