"""GPU: gradients of batched log-likelihoods -- the device reverse pass against the numpy oracle
(tests/grad_ref.py) and the C oracle's values, against central differences of evaluate(), translation invariance,
batch independence and determinism, ragged batches, failures, the width limit, and the torch autograd Function."""
import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd.batch import sho_coefficient_pack
from gadfly_amd.grad import parameter_vjp
from oracle import cref
from tests.grad_ref import batch_grad

pytestmark = pytest.mark.gpu

DT = 60.0 / 1e6                      # one-minute cadence (units of 1e6 s: frequencies in uHz)
DELTA = 60.0 / 1e6
JD0 = 2.12e5                         # a BKJD-like axis: t + 2.12e5


def _params(rng, B, J, n_over=0, amp=1.0):
    S0 = amp * rng.uniform(0.5, 3.0, (B, J))
    w0 = rng.uniform(50.0, 1500.0, (B, J))
    Q = rng.uniform(0.7, 20.0, (B, J))
    if n_over:
        Q[:, :n_over] = rng.uniform(0.15, 0.45, (B, n_over))
    return S0, w0, Q


def _axis(N, gaps=True):
    t = np.arange(N) * DT
    if gaps:
        t[N // 3:] += 50 * DT
        t[2 * N // 3:] += 9 * DT
    return t


def _scaled_close(theta, got, ref, tol):
    a, r = theta * got, theta * ref
    return np.max(np.abs(a - r)) <= tol * max(1.0, np.max(np.abs(r))), np.max(np.abs(a - r))


# W = 4, 20, 40, 60: every column count of the kernel (16, 32, 64), with real terms at W = 4 and W = 20
@pytest.mark.parametrize("J,n_over,N", [(2, 1, 6000), (10, 2, 4000), (20, 0, 3000), (30, 0, 2000)])
def test_device_matches_numpy_reverse_pass(J, n_over, N):
    rng = np.random.default_rng(11 + J)
    B = 8
    S0, w0, Q = _params(rng, B, J, n_over)
    t = _axis(N)
    y = rng.normal(size=N) * 20.0
    diag = 300.0 + rng.uniform(0.0, 30.0, N)
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), t, y, diag=diag)
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=("S0", "w0", "Q", "mean", "diag"))
    Jr, Jc, real, comp, diag_add, _ = sho_coefficient_pack(S0, w0, Q, DELTA)
    cond = (np.sum(np.abs(real[0]), axis=1) + np.sum(np.abs(comp[0]), axis=1) + diag.max()) / diag.min()
    llr, gr = batch_grad(np.broadcast_to(t, (B, N)), np.broadcast_to(y, (B, N)), np.broadcast_to(diag, (B, N)),
                         Jr, Jc, real, comp, diag_add)
    ref = parameter_vjp(S0, w0, Q, DELTA, gr["real"], gr["comp"], gr["diag_add"])
    ok = cond <= 1e7
    assert ok.all()
    assert np.all(np.abs(ll[ok] - llr[ok]) <= 1e-9 * np.abs(llr[ok]))
    for name, theta, r in zip(("S0", "w0", "Q"), (S0, w0, Q), ref):
        good, err = _scaled_close(theta[ok], g[name][ok], r[ok], 1e-7)
        assert good, (name, err)
    for name, key in (("mean", "mean"), ("diag", "diag_add")):
        assert np.all(np.abs(g[name][ok] - gr[key][ok]) <= 1e-7 * np.maximum(1.0, np.abs(gr[key][ok])))


def _kernels_like(S0, w0, Q):
    """Exposure-integrated SHO sums of (B, J) parameters (the batch's kernels; value_and_grad brings its own)."""
    from gadfly_amd.terms import SHOTerm, TermConvolution, TermSum
    return [TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q)) for s, w, q in zip(*r)]), DELTA)
            for r in zip(S0, w0, Q)]


@pytest.mark.parametrize("offset", [0.0, JD0])
def test_value_matches_c_oracle(offset):
    rng = np.random.default_rng(5)
    B, J, N = 3, 4, 4000
    S0, w0, Q = _params(rng, B, J)
    t = _axis(N) + offset
    y = rng.normal(size=N) * 20.0
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), t, y, yerr=15.0)
    ll, _ = ev.value_and_grad(S0, w0, Q, DELTA)
    for b, k in enumerate(_kernels_like(S0, w0, Q)):
        co = k.get_device_coefficients()
        ref, info = cref.loglike(co[:6], t, np.full(N, 225.0) + co[6], y)
        assert info == 0 and abs(ll[b] - ref) <= 1e-8 * abs(ref), (b, ll[b], ref)


def test_directional_derivative_matches_evaluate():
    from gadfly_amd.synth import solar_like_hyperparameters
    rng = np.random.default_rng(9)
    N, J = 100_000, 30
    hp = solar_like_hyperparameters(J)
    kern = gadfly_amd.StellarOscillatorKernel(hp, texp=60.0)
    t = np.arange(N) * DT
    # data drawn from the kernel: L n, n white (the stored factor's dot_tril)
    gp = gadfly_amd.GaussianProcess(kern, t=t, yerr=30.0, device="cuda:0")
    y = np.asarray(gp.dot_tril(rng.normal(size=N)))
    S0t, w0t, Qt = _pack_of(kern)
    delta = float(kern.delta)
    S0, w0, Q = (x * 1.1 for x in (S0t, w0t, Qt))
    ev = gadfly_amd.BatchedLogLikelihood([kern], t, y, yerr=30.0)
    ev.auto_generator_period = False
    ev.engine.generator_period = 1
    ll, g = ev.value_and_grad(S0, w0, Q, delta)
    v = rng.normal(size=(3, J))
    v /= np.linalg.norm(v)
    vg = float(np.sum(v[0] * S0 * g["S0"] + v[1] * w0 * g["w0"] + v[2] * Q * g["Q"]))
    h = 1e-3

    def at(s):
        e = [np.exp(s * v[i]) for i in range(3)]
        return float(ev.evaluate_device(ev.pack_parameters(S0 * e[0], w0 * e[1], Q * e[2], delta)).cpu()[0])

    # central differences at h and h / 2, Richardson-combined: the narrow p-modes (line widths of 1e-3 of w0) give
    # log L curvature on the scale of the step itself, and the plain difference at h carried a 2 % truncation error
    d1 = (at(h) - at(-h)) / (2.0 * h)
    d2 = (at(h / 2) - at(-h / 2)) / h
    fd = (4.0 * d2 - d1) / 3.0
    assert abs(at(0.0) - ll[0]) <= 1e-8 * abs(ll[0])
    assert abs(fd - vg) <= 1e-3 * abs(vg) + 0.1, (fd, vg)


def _pack_of(kern):
    """(1, J) S0, w0, Q arrays of a StellarOscillatorKernel's SHO terms."""
    terms = kern.term.terms if hasattr(kern, "term") else kern.terms
    S0 = np.array([[tm.S0 for tm in terms]])
    w0 = np.array([[tm.w0 for tm in terms]])
    Q = np.array([[tm.Q for tm in terms]])
    return S0, w0, Q


def test_translation_invariance():
    rng = np.random.default_rng(21)
    B, J, N = 4, 6, 5000
    S0, w0, Q = _params(rng, B, J, 1)
    t = _axis(N)
    y = rng.normal(size=N) * 20.0
    res = []
    for off in (0.0, JD0):
        ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), t + off, y, yerr=20.0)
        res.append(ev.value_and_grad(S0, w0, Q, DELTA))
    (l0, g0), (l1, g1) = res
    assert np.all(np.abs(l0 - l1) <= 1e-8 * np.abs(l0))
    for name, theta in (("S0", S0), ("w0", w0), ("Q", Q)):
        good, err = _scaled_close(theta, g1[name], g0[name], 1e-6)
        assert good, (name, err)


def test_batch_independence_and_determinism():
    rng = np.random.default_rng(33)
    B, J, N = 64, 10, 3000
    S0, w0, Q = _params(rng, B, J)
    t = _axis(N)
    y = rng.normal(size=(B, N)) * 20.0
    big = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), np.broadcast_to(t, (B, N)), y, yerr=20.0)
    lb, gb = big.value_and_grad(S0, w0, Q, DELTA)
    assert big.last_grad_plan[1] == 1
    lb2, gb2 = big.value_and_grad(S0, w0, Q, DELTA)
    per = big.last_grad_plan[0] // B
    big.grad_workspace_bytes = per * 22              # groups of 22, 22, 20
    lb3, gb3 = big.value_and_grad(S0, w0, Q, DELTA)
    assert big.last_grad_plan[1:] == (3, 22)
    one = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0[5:6], w0[5:6], Q[5:6]), t, y[5], yerr=20.0)
    l1, g1 = one.value_and_grad(S0[5:6], w0[5:6], Q[5:6], DELTA)
    for ll, g in ((lb2, gb2), (lb3, gb3)):
        assert np.array_equal(ll, lb)
        for k in ("S0", "w0", "Q"):
            assert np.array_equal(g[k], gb[k])
    assert l1[0] == lb[5]
    for k in ("S0", "w0", "Q"):
        assert np.array_equal(g1[k][0], gb[k][5])


def test_ragged_matches_each_series_alone():
    rng = np.random.default_rng(44)
    J = 5
    lens = (3000, 2200, 1500)
    S0, w0, Q = _params(rng, 3, J, 1)
    ts = [_axis(n) for n in lens]
    ys = [rng.normal(size=n) * 20.0 for n in lens]
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), ts, ys, yerr=20.0, mean=1.5)
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=("S0", "w0", "Q", "mean", "diag"))
    for b in range(3):
        one = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0[b:b + 1], w0[b:b + 1], Q[b:b + 1]), ts[b], ys[b], yerr=20.0,
                                               mean=1.5)
        l1, g1 = one.value_and_grad(S0[b:b + 1], w0[b:b + 1], Q[b:b + 1], DELTA,
                                    wrt=("S0", "w0", "Q", "mean", "diag"))
        assert abs(ll[b] - l1[0]) <= 1e-9 * abs(l1[0])
        for k in ("S0", "w0", "Q", "mean", "diag"):
            assert np.allclose(g[k][b], g1[k][0], rtol=1e-9, atol=1e-9 * np.max(np.abs(g1[k][0]))), k


def test_non_positive_definite_problem_is_isolated():
    rng = np.random.default_rng(55)
    B, J, N = 4, 3, 2000
    S0, w0, Q = _params(rng, B, J)
    t = _axis(N)
    y = rng.normal(size=N) * 20.0
    diag = np.full((B, N), 100.0)
    diag[2, 700:] = -1e6                              # planted: problem 2 loses positive definiteness at row 701
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), np.broadcast_to(t, (B, N)),
                                         np.broadcast_to(y, (B, N)), diag=diag)
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=("S0", "w0", "Q", "mean", "diag"))
    assert ll[2] == -np.inf and np.all(np.isfinite(np.delete(ll, 2)))
    for k, v in g.items():
        assert np.all(np.isnan(v[2])), k
        assert np.all(np.isfinite(np.delete(v, 2, axis=0))), k


def test_pack_of_another_batch_size_is_refused():
    rng = np.random.default_rng(67)
    B, J, N = 4, 3, 500
    S0, w0, Q = _params(rng, B, J)
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), _axis(N), rng.normal(size=N), yerr=1.0)
    with pytest.raises(ValueError, match="batch"):
        ev.value_and_grad(S0[:2], w0[:2], Q[:2], DELTA)
    with pytest.raises(ValueError, match="batch"):
        ev.value_and_grad_coefficients(_kernels_like(S0[:3], w0[:3], Q[:3]))
    big = [np.concatenate([x, x]) for x in (S0, w0, Q)]
    with pytest.raises(ValueError, match="batch"):
        ev.value_and_grad_coefficients(sho_coefficient_pack(*big, DELTA))
    with pytest.raises(ValueError, match="batch"):
        ev.value_and_grad_coefficients(gadfly_amd.BatchedLogLikelihood(
            _kernels_like(S0[:2], w0[:2], Q[:2]), _axis(N), rng.normal(size=N), yerr=1.0).pack_parameters(
                S0[:2], w0[:2], Q[:2], DELTA))
    ll, _ = ev.value_and_grad(S0, w0, Q, DELTA)         # the evaluator is still usable
    assert np.all(np.isfinite(ll))


def test_wide_kernel_raises():
    rng = np.random.default_rng(66)
    B, J, N = 2, 40, 500
    S0, w0, Q = _params(rng, B, J)
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), _axis(N), rng.normal(size=N), yerr=1.0)
    with pytest.raises(NotImplementedError, match="63"):
        ev.value_and_grad(S0, w0, Q, DELTA)


def test_autograd_function_gradcheck_and_lbfgs():
    rng = np.random.default_rng(77)
    N, J = 200, 2
    # a well-conditioned problem (amplitudes S0 w0 Q of 10-40 against a white-noise variance of 4): the numerical
    # Jacobian's own noise, the rounding of log L over twice its step, stays far below the tolerance
    S0, w0, Q = np.array([[0.01, 0.005]]), np.array([[300.0, 900.0]]), np.array([[3.0, 8.0]])
    t = _axis(N, gaps=False)
    y = rng.normal(size=N) * 3.0
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), t, y, yerr=2.0)
    args = tuple(torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (S0, w0, Q))
    f = lambda a, b, c: gadfly_amd.LogLikelihood.apply(a, b, c, ev, DELTA)      # noqa: E731
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-5, rtol=1e-3)

    # B = 3 problems of different parameters: backward weights every problem's gradient with its own grad_output
    B, N = 3, 60
    f3 = np.array([[1.0], [1.3], [0.8]])
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0 * f3, w0 / f3, Q * f3), t[:N], y[:N], yerr=2.0)
    args = tuple(torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (S0 * f3, w0 / f3, Q * f3))
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-5, rtol=1e-3)

    N = 4096
    S0t = np.array([[0.05, 0.02]])
    w0t = np.array([[300.0, 900.0]])
    Qt = np.array([[3.0, 8.0]])
    t = np.arange(N) * DT
    kern = _kernels_like(S0t, w0t, Qt)[0]
    co = kern.get_device_coefficients()
    c, a, U, V = cref.get_matrices(co[:6], t, np.full(N, 4.0) + co[6])
    d, Wm, info = cref.factor(t, c, a, U, V)
    assert info == 0
    y = cref.matmul_lower(t, c, U, Wm, rng.normal(size=N) * np.sqrt(d))
    ev = gadfly_amd.BatchedLogLikelihood([kern], t, y, yerr=2.0)
    x = torch.tensor(np.log(np.concatenate([S0t, w0t, Qt]) * 1.3), requires_grad=True)
    opt = torch.optim.LBFGS([x], max_iter=50, line_search_fn="strong_wolfe")

    def nll():
        opt.zero_grad()
        e = torch.exp(x)
        loss = -gadfly_amd.LogLikelihood.apply(e[0:1], e[1:2], e[2:3], ev, DELTA).sum()
        loss.backward()
        return loss

    l0 = nll().item()
    g0 = float(x.grad.norm())
    opt.step(nll)
    l1 = nll().item()
    g1 = float(x.grad.norm())
    assert l1 < l0 and g1 <= 1e-2 * g0, (l0, l1, g0, g1)
