"""GPU: posterior draws of B kernels at any times through the public interface --
BatchedLogLikelihood.sample_conditional_device and its wrappers against the dense restatement of
tests/cond_draw_ref.py and the dense oracle."""
import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd import conddraw
from gadfly_amd.batch import BatchedLogLikelihood
from tests import cond_draw_ref as ref
from tests import grad_cases as gc

pytestmark = pytest.mark.gpu

MARGIN = 10.0            # on the restatement's own deviation from the dense oracle: the device sums in another order


def _bll(prob, **kw):
    return BatchedLogLikelihood(ref.kernels(prob), prob["t"], prob["y"], diag=prob["diag"],
                                mean=prob["mean"][:, None], **kw)


def _unit_normals(B, nu, n):
    """The nu + n unit normal vectors and one zero vector as size = nu + n + 1 draws."""
    S = nu + n + 1
    eps, eta = np.zeros((B, S, nu)), np.zeros((B, S, n))
    eps[:, np.arange(nu), np.arange(nu)] = 1.0
    eta[:, nu + np.arange(n), np.arange(n)] = 1.0
    return eps, eta, S


@pytest.mark.parametrize("J", [3, 10, 30])
def test_linear_map_of_the_device_draw_is_the_dense_conditional(hip, J):
    """B = 3 kernels of J SHO terms (W = 6, 20, 60: k_solve_rhs<16>, <32>, <64>), N = 40 on a gapped axis, M = 17
    queries before, inside the gap, on stamps and behind; the Nu + N unit normal vectors and the zero vector as
    size = Nu + N + 1 draws (many blocks of right-hand sides).  The zero-normal draw is predict_device(t=...) within
    1e-9 of max |reference|; A A^T is the dense oracle's posterior covariance within an ABSOLUTE bar in units of K(0):
    cond_draw_ref.yardstick -- the host restatement's own worst deviation from the dense oracle, 2.6e-15 of K(0) --
    times 10; its diagonal equals predict_device(return_var=True) to the same bar.  The same at the observed stamps
    (A A^T = K - K Sigma^-1 K).  Measured on an MI355X (bar 2.6e-14 of K(0)): A A^T worst 4.7e-15 at new times and
    8.6e-16 at the observed stamps, its diagonal against return_var 2.9e-15 / 1.7e-16, the zero-normal draw equal to
    predict_device(t=...) to the bit."""
    N, M = 40, 17
    prob = ref.problem(0, J, N, M)
    B = prob["B"]
    bar = MARGIN * ref.yardstick()[1]
    bll = _bll(prob)
    worst = dict(zero=0.0, cov=0.0, var=0.0)
    for ts in (prob["ts"], None):
        ax = conddraw.union_axes(prob["t"], ts)
        nu = int(ax.nu[0])
        assert np.all(ax.nu == nu)
        eps, eta, S = _unit_normals(B, nu, N)
        z = bll.sample_conditional(t=ts, size=S, normals=(eps, eta))
        assert z.shape == (B, S, M if ts is not None else N)
        assert np.all(bll.last_conditional_info.cpu().numpy() == 0)
        assert bll.last_predict_ll.shape == (B, S) and np.all(bll.last_predict_info.cpu().numpy() == 0)
        mu, var = bll.predict(t=ts, return_var=True)
        for b in range(B):
            co, k0 = gc.coefficients(prob, b), prob["diag_add"][b]
            c, A = z[b, -1], (z[b, :-1] - z[b, -1][None, :]).T
            ref_mu, ref_cov = ref.dense_posterior(co, 0.0, prob["t"], prob["diag"][b], prob["y"][b], prob["mean"][b],
                                                  None if ts is None else ts[b])
            e0 = float(np.max(np.abs(c - mu[b])) / np.max(np.abs(ref_mu)))
            e1 = float(np.max(np.abs(A @ A.T - ref_cov)) / k0)
            e2 = float(np.max(np.abs(np.diag(A @ A.T) - var[b])) / k0)
            worst = dict(zero=max(worst["zero"], e0), cov=max(worst["cov"], e1), var=max(worst["var"], e2))
            print(f"J = {J}, {'t*' if ts is not None else 't'}, b = {b}: zero-normal draw {e0:.2e}, A A^T {e1:.2e}, "
                  f"diag {e2:.2e} (bar {bar:.2e})")
    assert worst["zero"] <= 1e-9, worst
    assert worst["cov"] <= bar and worst["var"] <= bar, (worst, bar)


def _rough_problem(B, J, N, M, seed):
    """B kernels of J SHO terms on a gapped axis of cadence 1.2e-3 (cond_draw_ref.STRETCH), M queries per problem: at
    mid-cadence, on stamps, before and behind the data."""
    prob = dict(gc.edge_problem(0, J, N, B=B, seed=seed))
    t = prob["t"] * ref.STRETCH
    rng = np.random.default_rng([23, seed])
    ts = np.empty((B, M))
    for b in range(B):
        mid = rng.choice(N - 1, size=M - 20, replace=False)
        on = rng.choice(N, size=10, replace=False)
        dt = gc.DT * ref.STRETCH
        ts[b] = np.sort(np.concatenate([0.5 * (t[mid] + t[mid + 1]), t[on], t[0] - dt * np.arange(1, 6),
                                        t[-1] + dt * np.arange(1, 6)]))
    prob.update(t=t, ts=ts, mean=np.linspace(-50.0, 50.0, B))
    prob["y"] = prob["y"] + prob["mean"][:, None]
    return prob


def test_fixed_normal_draws_match_the_host_restatement(hip):
    """B = 5, J = 30, N = 3000, M = 300, size = 3: 1e-6 relative to max |reference| per problem."""
    B, J, N, M, S = 5, 30, 3000, 300, 3
    prob = _rough_problem(B, J, N, M, 1)
    ax = conddraw.union_axes(prob["t"], prob["ts"])
    nu = int(ax.nu[0])
    assert np.all(ax.nu == nu) and nu == N + M - 10
    rng = np.random.default_rng(8)
    eps, eta = rng.normal(size=(B, S, nu)), rng.normal(size=(B, S, N))
    z = _bll(prob).sample_conditional(t=prob["ts"], size=S, normals=(eps, eta))
    assert z.shape == (B, S, M)
    for b in range(B):
        want = ref.draw(gc.coefficients(prob, b), 0.0, prob["t"], prob["diag"][b], prob["y"][b], prob["mean"][b],
                        prob["ts"][b], eps[b], eta[b])
        err = float(np.max(np.abs(z[b] - want)) / np.max(np.abs(want)))
        print(f"b = {b}: {err:.2e}")
        assert err <= 1e-6, (b, err)


def test_ragged_batch_equals_each_series_alone(hip):
    """Series of 50, 64 and 129 rows with per-series queries as a list: each problem's draws equal those of the series
    alone with the same normals to 1e-12 relative (DESIGN.md 3.12's ragged bar); the lists have the right lengths."""
    lens, nqs, S = (50, 64, 129), (7, 0, 33), 2
    full = _rough_problem(3, 10, 129, 40, 2)
    ks = ref.kernels(full)
    t = [full["t"][:n] for n in lens]
    y = [full["y"][b, :n] for b, n in enumerate(lens)]
    dg = [full["diag"][b, :n] for b, n in enumerate(lens)]
    qs = [np.sort(np.concatenate([full["ts"][b][full["ts"][b] < t[b][-1]][:m], t[b][-1:] + 1e-3]))[:m]
          for b, m in enumerate(nqs)]
    ax = conddraw.union_axes(t, qs)
    rng = np.random.default_rng(4)
    eps = [rng.normal(size=(S, int(n))) for n in ax.nu]
    eta = [rng.normal(size=(S, n)) for n in lens]
    bll = BatchedLogLikelihood(ks, t, y, diag=dg, mean=full["mean"])
    for tq in (qs, None):
        e = eps if tq is not None else [x[:, :n] for x, n in zip(eps, lens)]
        got = bll.sample_conditional(t=tq, size=S, normals=(e, eta))
        assert isinstance(got, list) and len(got) == 3
        for b in range(3):
            assert got[b].shape == (S, nqs[b] if tq is not None else lens[b])
            one = BatchedLogLikelihood([ks[b]], t[b], y[b][None, :], diag=dg[b], mean=full["mean"][b])
            alone = one.sample_conditional(t=None if tq is None else tq[b], size=S, normals=(e[b][None], eta[b][None]))
            if got[b].size:
                assert np.max(np.abs(got[b] - alone[0])) <= 1e-12 * np.max(np.abs(alone[0])), (b, tq is None)


def test_seeds_sizes_and_the_mean(hip):
    prob = ref.problem(0, 10, 40, 17)
    bll = _bll(prob)
    for ts in (prob["ts"], None):
        a = bll.sample_conditional(t=ts, size=3, seed=11)
        assert np.array_equal(a, bll.sample_conditional(t=ts, size=3, seed=11))
        assert not np.array_equal(a, bll.sample_conditional(t=ts, size=3, seed=12))
        assert np.array_equal(bll.sample_conditional(t=ts, seed=5), bll.sample_conditional(t=ts, size=1, seed=5)[:, 0])
        nomean = bll.sample_conditional(t=ts, size=3, seed=11, include_mean=False)
        assert np.array_equal(a, nomean + prob["mean"][:, None, None])
        assert np.all(np.isfinite(a)) and a.shape == (3, 3, 17 if ts is not None else 40)
    dev = bll.sample_conditional_device(t=prob["ts"], seed=3)
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.float64 and tuple(dev.shape) == (3, 17)
    one = gadfly_amd.sample_conditional_batch(ref.kernels(prob), prob["t"], prob["y"], diag=prob["diag"],
                                              mean=prob["mean"][:, None], t_pred=prob["ts"], seed=3)
    assert np.array_equal(one.cpu().numpy(), dev.cpu().numpy())
    ms = bll.last_conditional_ms
    assert set(ms) == {"sweeps", "assembly", "solve", "at"} and all(v >= 0.0 for v in ms.values())


def test_apply_inverse_and_log_likelihoods_of_many_right_hand_sides(hip):
    prob = ref.problem(0, 10, 40, 17)
    B, N, R = prob["B"], 40, 11
    bll = _bll(prob)
    _, alpha = bll.predict(return_alpha=True)
    resid = prob["y"] - prob["mean"][:, None]
    got = bll.apply_inverse_device(resid)
    assert tuple(got.shape) == (B, N) and np.array_equal(got.cpu().numpy(), alpha)
    ll1 = bll.log_likelihood_device(resid).cpu().numpy()
    assert ll1.shape == (B, 1) and np.allclose(ll1[:, 0], bll.evaluate(), rtol=1e-9, atol=0)
    rng = np.random.default_rng(2)
    Y = rng.normal(size=(B, R, N)) * np.sqrt(prob["diag_add"])[:, None, None]
    a3, ll3 = bll.apply_inverse_device(Y).cpu().numpy(), bll.log_likelihood_device(Y).cpu().numpy()
    shared = bll.apply_inverse_device(Y[0]).cpu().numpy()
    assert a3.shape == (B, R, N) and ll3.shape == (B, R) and shared.shape == (B, R, N)
    assert np.array_equal(shared[0], a3[0])
    assert tuple(bll.apply_inverse_device(Y[0, 0]).shape) == (B, N)
    from oracle import dense
    for b in range(B):
        co = gc.coefficients(prob, b)
        want = dense.apply_inverse(co, prob["t"], prob["diag"][b], Y[b].T).T
        assert np.max(np.abs(a3[b] - want)) <= 1e-9 * np.max(np.abs(want))
        for r in (0, R - 1):
            wl = dense.log_likelihood(co, prob["t"], prob["diag"][b], Y[b, r])
            assert abs(ll3[b, r] - wl) <= 1e-9 * abs(wl)


def test_gaussian_process_wrapper(hip):
    """GaussianProcess.sample_conditional for one small problem against the restatement; at M = 12 the covariance its
    linear map implies against ConditionalDistribution.covariance (the dense, celerite2-compatible route)."""
    from gadfly_amd import terms
    N, M = 30, 12
    rng = np.random.default_rng(6)
    t = np.sort(rng.uniform(0.0, 10.0, N))
    ts = np.sort(np.concatenate([rng.uniform(-1.0, 11.0, M - 2), t[[3, 20]]]))
    kernel = terms.SHOTerm(S0=1.3, w0=2.1, Q=3.0) + terms.SHOTerm(S0=0.4, w0=5.0, Q=0.8)
    y = rng.normal(size=N)
    gp = gadfly_amd.GaussianProcess(kernel, mean=0.7)
    gp.compute(t, yerr=0.3)
    ax = conddraw.union_axes(t, ts)
    nu = int(ax.nu[0])
    eps, eta, S = _unit_normals(1, nu, N)
    z = gp.sample_conditional(y, t=ts, size=S, normals=(eps[0], eta[0]))
    assert z.shape == (S, M)
    co = kernel.get_device_coefficients()
    want = ref.draw(co[:6], co[6], t, np.full(N, 0.09), y, 0.7, ts, eps[0], eta[0])
    assert np.max(np.abs(z - want)) <= 1e-9 * np.max(np.abs(want))
    A = (z[:-1] - z[-1][None, :]).T
    cond = gp.condition(y, t=ts)
    assert np.max(np.abs(z[-1] - cond.mean)) <= 1e-9 * np.max(np.abs(cond.mean))
    cov = cond.covariance
    assert np.max(np.abs(A @ A.T - cov)) <= 1e-9 * np.max(np.abs(cov))
    one = gp.sample_conditional(y, t=ts, seed=1)
    assert one.shape == (M,) and np.array_equal(one, gp.sample_conditional(y, t=ts, seed=1))
    assert gp.sample_conditional(y, seed=1).shape == (N,)


def test_errors_before_anything_is_enqueued(hip):
    # W = 64
    prob = gc.edge_problem(0, 32, 20)
    ks = [conddraw._PackKernel(0, 32, prob["real"], prob["comp"], prob["diag_add"], b) for b in range(3)]
    wide = BatchedLogLikelihood(ks, prob["t"], prob["y"], diag=prob["diag"])
    with pytest.raises(NotImplementedError, match="64"):
        wide.sample_conditional_device(seed=0)
    with pytest.raises(NotImplementedError, match="64"):
        wide.apply_inverse_device(prob["y"])
    # an exposure-integrated kernel with a query at half an exposure from a stamp
    from gadfly_amd.synth import solar_like_hyperparameters
    k = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(4), texp=60.0)
    delta = float(k.delta)
    t = np.arange(50) * delta
    bll = BatchedLogLikelihood([k, k], t, np.zeros((2, 50)), yerr=30.0)
    with pytest.raises(ValueError, match="exposure time"):
        bll.sample_conditional_device(t=np.array([t[7] + 0.5 * delta]), seed=0)
    with pytest.raises(ValueError, match="sorted"):
        bll.sample_conditional_device(t=np.array([t[9], t[7]]), seed=0)
    with pytest.raises(ValueError, match="normals"):
        bll.sample_conditional_device(t=t[[7]], normals=(np.zeros((2, 51)), np.zeros((2, 50))))
    out = bll.sample_conditional_device(t=np.array([t[7], t[-1] + 3 * delta]), seed=0)      # on a stamp: merged, fine
    assert tuple(out.shape) == (2, 2) and bool(torch.all(torch.isfinite(out)))
