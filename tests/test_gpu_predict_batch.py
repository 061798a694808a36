"""GPU: BatchedLogLikelihood.predict / predict_batch -- conditional means of B different kernels in
one device call against oracle/seq.py in float64 and against GaussianProcess.predict one kernel at a time, with and
without a component; kernels, host packs and device packs; per-problem and JD-based axes; ragged batches; means;
groups under a workspace cap; a long series; the width limit and the component's validation."""
import functools

import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.batch import sho_coefficient_pack
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times
from gadfly_amd.terms import SHOTerm, TermConvolution, TermSum
from tests.solve_ref import oracle_predict

pytestmark = pytest.mark.gpu

J, N, B = 30, 3000, 5
JD0 = 2454833.0 * 0.0864
YERR = 30.0


def _base(j=J):
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(j), texp=60.0)
    terms = kern.term.terms
    return [np.array([[getattr(tm, k) for tm in terms]]) for k in ("S0", "w0", "Q")], float(kern.delta)


@functools.lru_cache(maxsize=None)
def _walkers(b=B, j=J, seed=3):
    """(S0, w0, Q (b, j), delta): proposals around the solar-like kernel's own parameters."""
    (S0, w0, Q), delta = _base(j)
    rng = np.random.default_rng(seed)
    S0, w0 = (np.repeat(x, b, axis=0) * np.exp(0.05 * rng.normal(size=(b, j))) for x in (S0, w0))
    return S0, w0, np.repeat(Q, b, axis=0), delta


def _kernels(S0, w0, Q, delta, first=None):
    """Exposure-integrated SHO sums of (B, J) parameters; ``first``: only the first so many terms (a component)."""
    return [TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q))
                                      for s, w, q in list(zip(*r))[:first]]), delta) for r in zip(S0, w0, Q)]


def _data(n=N, seed=8):
    rng = np.random.default_rng(seed)
    return uniform_times(n, 60.0), 100.0 * rng.normal(size=n)


def _oracle(kern, t, y, diag, sub=None):
    co = kern.get_device_coefficients()
    comp = None if sub is None else sub.get_device_coefficients()[:6]
    return oracle_predict(t, y, diag, co[:6], float(np.sum(co[0]) + np.sum(co[2]) + co[6]), comp=comp)


@functools.lru_cache(maxsize=None)
def _shared_reference():
    """oracle/seq.py in float64 for the B walkers on the shared series, the component the first third of the terms."""
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    subs = _kernels(S0, w0, Q, delta, first=J // 3)
    return tuple(_oracle(k, t, y, np.full(N, YERR ** 2), s) for k, s in zip(_kernels(S0, w0, Q, delta), subs))


def _err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def test_walkers_match_the_oracle_and_the_single_gp():
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mu, alpha = ev.predict(return_alpha=True)
    assert mu.shape == alpha.shape == (B, N) and ev.last_predict_plan[1] == 1
    ll = ev.last_predict_ll.cpu().numpy()
    assert np.all(ev.last_predict_info.cpu().numpy() == 0)
    mc = ev.predict(kernel=subs)
    # kernels, a host pack and a device pack are the same coefficients: the same bits
    for pk in (kernels, sho_coefficient_pack(S0, w0, Q, delta), ev.pack_parameters(S0, w0, Q, delta),
               ev.pack(kernels)):
        m2, a2 = ev.predict(pk, return_alpha=True)
        assert np.array_equal(m2, mu) and np.array_equal(a2, alpha)
    sub_pack = sho_coefficient_pack(S0[:, :J // 3], w0[:, :J // 3], Q[:, :J // 3], delta)
    assert np.array_equal(ev.predict(kernel=sub_pack), mc)
    worst = dict(alpha=0.0, mu=0.0, mu_comp=0.0, ll=0.0, gp=0.0, gp_comp=0.0)
    for b, ref in enumerate(_shared_reference()):
        e = dict(alpha=_err(alpha[b], ref["alpha"]), mu=_err(mu[b], ref["mu"]), mu_comp=_err(mc[b], ref["mu_comp"]),
                 ll=abs(ll[b] - ref["ll"]) / abs(ref["ll"]))
        gp = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=YERR, device="cuda:0")
        e["gp"], e["gp_comp"] = _err(mu[b], gp.predict(y)), _err(mc[b], gp.predict(y, kernel=subs[b]))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print("walkers, J = 30, N = 3000: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(worst[k] <= 1e-9 for k in ("alpha", "mu", "mu_comp", "ll")), worst
    assert worst["gp"] <= 1e-8 and worst["gp_comp"] <= 1e-8, worst
    # one component kernel for all problems
    one = ev.predict(kernel=subs[2])
    assert np.array_equal(one[2], mc[2])
    # the log-likelihood is value_and_grad's: the same recurrence summed in the same order (the two kernels may
    # place their fused multiply-adds differently: a few ulp of each of the N terms at most)
    llg, _ = ev.value_and_grad(S0, w0, Q, delta)
    print(f"log L against value_and_grad: {np.max(np.abs(ll - llg) / np.abs(llg)):.1e}")
    assert np.all(np.abs(ll - llg) <= 1e-12 * np.abs(llg))
    # a workspace cap of two problems: groups of 2, 2, 1 -- the same bits
    ev.predict_workspace_bytes = 2 * (ev.last_predict_plan[0] // B)
    m3, a3 = ev.predict(return_alpha=True)
    assert ev.last_predict_plan[1:] == (3, 2)
    assert np.array_equal(m3, mu) and np.array_equal(a3, alpha)
    assert np.array_equal(ev.predict(kernel=subs), mc)
    # the one-shot form
    assert np.array_equal(gadfly_amd.predict_batch(kernels, t, y, yerr=YERR), mu)


def test_per_problem_axes_and_a_jd_axis():
    """Three problems with their own axes and data: a gapped axis, the same on a JD-based axis (t + 2454833 d: phases
    of 5e9 rad), a jittered one.  1e-9 against the float64 oracle, 1e-8 on the JD axis (the project's bar there)."""
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers())
    n = 1500
    rng = np.random.default_rng(17)
    t0 = uniform_times(n, 60.0)
    t0[n // 2:] += 40 * 60e-6
    ts = np.stack([t0, t0 + JD0, t0 + rng.uniform(-0.1, 0.1, n) * 60e-6])
    ys = 100.0 * rng.normal(size=(3, n))
    diag = YERR ** 2 * rng.uniform(0.8, 1.2, (3, n))
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, ts, ys, diag=diag)
    mu, alpha = ev.predict(return_alpha=True)
    mc = ev.predict(kernel=subs)
    for b, bar in enumerate((1e-9, 1e-8, 1e-9)):
        ref = _oracle(kernels[b], ts[b], ys[b], diag[b], subs[b])
        e = [_err(alpha[b], ref["alpha"]), _err(mu[b], ref["mu"]), _err(mc[b], ref["mu_comp"])]
        print(f"problem {b}: alpha {e[0]:.1e}, mu {e[1]:.1e}, mu' {e[2]:.1e}")
        assert all(x <= bar for x in e), (b, e)
        one = gadfly_amd.BatchedLogLikelihood(kernels[b:b + 1], ts[b], ys[b], diag=diag[b])
        assert np.array_equal(one.predict()[0], mu[b])


def test_ragged_batch_gives_each_series_alone_to_the_bit():
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers())
    lens = (700, 1, 333)
    rng = np.random.default_rng(23)
    ts = [uniform_times(n, 60.0) + JD0 * (i == 2) for i, n in enumerate(lens)]
    ys = [100.0 * rng.normal(size=n) + 2.5 for n in lens]
    means = np.array([2.5, 2.0, 3.0])
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, ts, ys, yerr=YERR, mean=means)
    mu, alpha = ev.predict(return_alpha=True)
    mc = ev.predict(kernel=subs, include_mean=False)
    ll = ev.last_predict_ll.cpu().numpy()
    assert [len(x) for x in mu] == list(lens) == [len(x) for x in alpha] == [len(x) for x in mc]
    for b, n in enumerate(lens):
        one = gadfly_amd.BatchedLogLikelihood(kernels[b:b + 1], ts[b], ys[b], yerr=YERR, mean=float(means[b]))
        m1, a1 = one.predict(return_alpha=True)
        assert np.array_equal(m1[0], mu[b]) and np.array_equal(a1[0], alpha[b]), b
        assert np.array_equal(one.predict(kernel=subs[b], include_mean=False)[0], mc[b]), b
        l1 = one.last_predict_ll.cpu().numpy()[0]
        # the pad rows' constants come off again: each of the npad pad rows added log 2^1000 to a running sum of the
        # size of their total, one rounding of that sum per row at most
        npad = max(lens) - n
        pad_total = 0.5 * npad * (1000.0 * np.log(2.0) + np.log(2.0 * np.pi))
        assert abs(ll[b] - l1) <= 1e-12 * abs(l1) + npad * np.spacing(pad_total), (b, ll[b], l1)


def test_means_scalar_and_per_problem():
    S0, w0, Q, delta = _walkers()
    t, y = _data()
    kernels = _kernels(S0, w0, Q, delta)
    refs = _shared_reference()
    for mean in (7.0, np.linspace(-3.0, 5.0, B)[:, None]):
        ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y[None, :] + mean, yerr=YERR, mean=mean)
        with_mean, without = ev.predict(), ev.predict(include_mean=False)
        m = np.broadcast_to(mean, (B, 1))
        for b, ref in enumerate(refs):
            scale = np.max(np.abs(ref["mu"]))
            assert np.max(np.abs(without[b] - ref["mu"])) <= 1e-9 * scale
            assert np.max(np.abs(with_mean[b] - (ref["mu"] + m[b]))) <= 1e-9 * scale


def test_long_series_against_the_single_gp():
    """N = 20 000, W = 60, B = 2: 313 blocks of 64 rows, 30 segments, the second problem's workspace and outputs at
    64-bit offsets from the first's."""
    S0, w0, Q, delta = (x[:2] if np.ndim(x) else x for x in _walkers())
    n = 20_000
    t, y = _data(n, seed=31)
    kernels, subs = _kernels(S0, w0, Q, delta), _kernels(S0, w0, Q, delta, first=J // 3)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    mu, mc = ev.predict(), ev.predict(kernel=subs)
    for b in range(2):
        gp = gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=YERR, device="cuda:0")
        e = _err(mu[b], gp.predict(y)), _err(mc[b], gp.predict(y, kernel=subs[b]))
        print(f"N = 20 000, problem {b}: mu {e[0]:.1e}, mu' {e[1]:.1e} against GaussianProcess.predict")
        assert max(e) <= 1e-8, (b, e)


def test_width_limit_and_component_validation():
    t, y = _data(500)
    S0, w0, Q, delta = _walkers(2, 32)
    wide = _kernels(S0, w0, Q, delta)
    ev = gadfly_amd.BatchedLogLikelihood(wide, t, y, yerr=YERR)
    with pytest.raises(NotImplementedError, match="W = 64"):
        ev.predict()
    S0, w0, Q, delta = _walkers(2, 6)
    kernels = _kernels(S0, w0, Q, delta)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=YERR)
    with pytest.raises(NotImplementedError, match="W = 64"):
        ev.predict(kernel=wide)
    with pytest.raises(ValueError):                                   # components of two term structures
        ev.predict(kernel=[_kernels(S0, w0, Q, delta, first=2)[0], _kernels(S0, w0, Q, delta, first=3)[1]])
    with pytest.raises(ValueError):                                   # three components for two problems
        ev.predict(kernel=_kernels(S0, w0, Q, delta, first=2) + _kernels(S0, w0, Q, delta, first=2)[:1])
    with pytest.raises(ValueError):                                   # a pack of another batch size
        ev.predict(sho_coefficient_pack(S0[:1], w0[:1], Q[:1], delta))
    mu = ev.predict()                                                 # the evaluator is still usable
    assert mu.shape == (2, 500) and np.all(np.isfinite(mu))


def test_non_positive_definite_problem_is_isolated():
    S0, w0, Q, delta = (x[:3] if np.ndim(x) else x for x in _walkers(j=6))
    n = 900
    t, y = _data(n)
    diag = np.full((3, n), YERR ** 2)
    kernels = _kernels(S0, w0, Q, delta)
    clean = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag).predict()
    diag[1, 500:] = -1e9
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag)
    mu = ev.predict()
    assert np.all(np.isnan(mu[1])) and np.array_equal(mu[[0, 2]], clean[[0, 2]])
    assert ev.last_predict_ll.cpu().numpy()[1] == -np.inf and ev.last_predict_info.cpu().numpy()[1] == 501
