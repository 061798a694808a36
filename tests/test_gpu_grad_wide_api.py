"""GPU: the wide gradient route through the public interface --
BatchedLogLikelihood.value_and_grad(..., wide=True) on gadfly's 86-term default kernel (W = 172) against the 80-bit
numpy reverse pass, narrow kernels and a ragged list against the one-wave route, the split into groups,
GaussianProcess.value_and_grad(..., wide=True) against the batch call and log_likelihood, the early errors, the autograd
Function, and a matrix that is not positive definite among healthy ones."""
import functools

import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd import grad as gg
from gadfly_amd.batch import sho_coefficient_pack
from gadfly_amd.grad import parameter_vjp
from gadfly_amd.synth import solar_like_hyperparameters
from tests import grad_cases as gc
from tests import random_cases as rc
from tests.grad_ref import batch_grad

pytestmark = pytest.mark.gpu

ALL = ("S0", "w0", "Q", "mean", "diag")
DELTA = 60e-6
N_SOLAR = 300


@functools.lru_cache(maxsize=None)
def _solar(cadence):
    """Two stars of the 86-term solar kernel (the second with S0, w0, Q a few per cent off), N = 300 rows at
    ``cadence`` seconds with a gap, white noise of 25: (kernel, S0, w0, Q, t, y, pack, 80-bit log L and coefficient
    adjoints, their chain rule), once."""
    rng = np.random.default_rng([86, int(cadence)])
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(86), texp=60.0)
    terms = kern.term.terms
    S0, w0, Q = (np.array([[getattr(x, n) for x in terms]] * 2) for n in ("S0", "w0", "Q"))
    for x in (S0, w0, Q):
        x[1] *= rng.uniform(0.95, 1.05, x.shape[1])
    assert S0.shape == (2, 86) and np.all(Q >= 0.5)
    t = np.arange(N_SOLAR) * cadence * 1e-6
    t[N_SOLAR // 2:] += 37 * cadence * 1e-6
    y = rng.normal(size=(2, N_SOLAR)) * 40.0
    pk = sho_coefficient_pack(S0, w0, Q, DELTA)[:5]
    diag = np.full((2, N_SOLAR), 25.0 ** 2)
    llr, gr = batch_grad(np.broadcast_to(t, (2, N_SOLAR)), y, diag, *pk, dtype=np.longdouble)
    ref = dict(zip(("S0", "w0", "Q"), parameter_vjp(S0, w0, Q, DELTA, gr["real"], gr["comp"], gr["diag_add"])))
    return kern, S0, w0, Q, t, y, pk, llr, gr, ref


@pytest.mark.parametrize("cadence", [60.0, 1765.0])
def test_solar_kernel_matches_the_80_bit_pass(cadence):
    kern, S0, w0, Q, t, y, pk, llr, gr, ref = _solar(cadence)
    Jr, Jc, real, comp, _ = pk
    assert Jr + 2 * Jc == 172 and np.all(np.isfinite(llr))
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, yerr=25.0)
    with pytest.raises(NotImplementedError, match="63.*wide=True"):
        ev.value_and_grad(S0, w0, Q, DELTA)
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL, wide=True)
    assert ev.last_grad_seg == gg._lib.load().gf_grad_wide_seg(N_SOLAR, 172) and ev.last_grad_chunk_len is None
    ll2, gco = ev.value_and_grad_coefficients(pk, wide=True)
    assert np.array_equal(ll, ll2) and np.all(np.isfinite(ll))
    errs = {"ll": float(np.max(np.abs(ll - llr) / np.abs(llr)))}
    for name, theta in (("S0", S0), ("w0", w0), ("Q", Q)):
        errs[name] = max(gc.scaled_error(theta[b], g[name][b], ref[name][b]) for b in range(2))
    for i, name in enumerate(("ac", "bc", "cc", "dc")):
        errs[name] = max(gc.scaled_error(comp[i, b, :Jc], gco["comp"][i, b], gr["comp"][i, b]) for b in range(2))
    for name, key in (("mean", "mean"), ("diag", "diag_add")):
        assert np.array_equal(g[name], gco[key])
        errs[name] = float(np.max(np.abs(g[name] - gr[key]) / np.maximum(1.0, np.abs(gr[key]))))
    print(f"solar kernel, {cadence:.0f} s cadence: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert errs.pop("ll") <= 1e-9
    assert max(errs.values()) <= 1e-7, errs


def _close(ll, g, ll1, g1, thetas):
    assert np.all(np.abs(ll - ll1) <= 1e-9 * np.abs(ll1)), (ll, ll1)
    for name, theta in thetas.items():
        for b in range(len(ll)):
            assert gc.scaled_error(theta[b], g[name][b], g1[name][b]) <= 1e-7, (name, b)
    for name in ("mean", "diag"):
        assert np.all(np.abs(g[name] - g1[name]) <= 1e-7 * np.maximum(1.0, np.abs(g1[name]))), name


def test_narrow_kernels_match_the_default_route():
    """J = 5, N = 700 on a shared axis, and a ragged list of two series with per-problem mean and yerr."""
    rng = np.random.default_rng(31)
    J = 5
    S0, w0, Q = rng.uniform(0.5, 3.0, (2, J)), rng.uniform(50.0, 1500.0, (2, J)), rng.uniform(0.7, 20.0, (2, J))
    t = np.arange(700) * 60e-6
    y = rng.normal(size=(2, 700)) * 20.0
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, yerr=12.0)
    ll1, g1 = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL)
    assert ev.last_grad_seg is None
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL, wide=True)
    assert ev.last_grad_seg == 27
    _close(ll, g, ll1, g1, dict(S0=S0, w0=w0, Q=Q))
    ts = [np.arange(n) * 60e-6 for n in (700, 431)]
    ys = [rng.normal(size=len(x)) * 20.0 for x in ts]
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), ts, ys, yerr=[12.0, 15.0],
                                         mean=[0.5, -1.0])
    ll1, g1 = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL)
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL, wide=True)
    _close(ll, g, ll1, g1, dict(S0=S0, w0=w0, Q=Q))


def test_group_split_keeps_every_bit():
    """B = 4 stars of a W = 80 kernel in one, two and four groups under the byte cap."""
    rng = np.random.default_rng(5)
    B, J, N = 4, 40, 120
    S0, w0, Q = rng.uniform(0.5, 3.0, (B, J)), rng.uniform(50.0, 1500.0, (B, J)), rng.uniform(0.7, 20.0, (B, J))
    t = np.arange(N) * 60e-6
    y = rng.normal(size=(B, N)) * 100.0
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, yerr=30.0)
    per = 8 * gg.workspace_plan(N, 2 * J, B, wide=True)[0]
    base = None
    for groups, cap in ((1, 4 * per), (2, 2 * per + 8), (4, per)):
        ev.grad_workspace_bytes = cap
        ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL, wide=True)
        assert ev.last_grad_plan == (per * (B // groups), groups, B // groups), ev.last_grad_plan
        assert np.all(np.isfinite(ll))
        if base is None:
            base = (ll, g)
        assert np.array_equal(ll, base[0]) and all(np.array_equal(g[k], base[1][k]) for k in ALL), groups


def test_gaussian_process_takes_the_wide_route():
    kern, S0, w0, Q, t, y, *_ = _solar(60.0)
    gp = gadfly_amd.GaussianProcess(kern, t=t, yerr=25.0, mean=3.0)
    val, g = gp.value_and_grad(y[0] + 3.0, wrt=ALL, wide=True)
    ev = gadfly_amd.BatchedLogLikelihood([kern], t, y[0] + 3.0, yerr=25.0, mean=3.0)
    ll, gb = ev.value_and_grad(S0[:1], w0[:1], Q[:1], float(kern.delta), wrt=ALL, wide=True)
    assert gp.last_grad_seg == ev.last_grad_seg and gp.last_grad_chunk_len is None
    assert val == ll[0] and np.isfinite(val)
    for k in ("S0", "w0", "Q"):
        assert g[k].shape == (86,) and np.array_equal(g[k], gb[k][0]), k
    for k in ("mean", "diag"):
        assert isinstance(g[k], float) and g[k] == gb[k][0], k
    ref = gp.log_likelihood(y[0] + 3.0)
    assert abs(val - ref) <= 1e-8 * abs(ref), (val, ref)
    with pytest.raises(ValueError):
        gp.value_and_grad(y[0], wide=True, chunk_len=64)


def test_early_errors_enqueue_nothing():
    kern, S0, w0, Q, t, y, pk, *_ = _solar(60.0)
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, yerr=25.0)
    for kw in (dict(time_parallel=True), dict(chunk_len=64)):
        with pytest.raises(ValueError):
            ev.value_and_grad(S0, w0, Q, DELTA, wide=True, **kw)
        with pytest.raises(ValueError):
            ev.value_and_grad_coefficients(pk, wide=True, **kw)
    with pytest.raises(ValueError):
        gg.coefficient_gradients(ev.engine, *pk, wide=True, rows=np.array([N_SOLAR, N_SOLAR]))
    with pytest.raises(NotImplementedError, match="63"):
        ev.value_and_grad(S0, w0, Q, DELTA)
    # one term more than the widest instance takes
    J = gg.wide_max_width() // 2 + 1
    rng = np.random.default_rng(2)
    P = [rng.uniform(lo, hi, (1, J)) for lo, hi in ((0.5, 3.0), (50.0, 1500.0), (0.7, 20.0))]
    big = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(*P, DELTA), t, y[0], yerr=25.0)
    with pytest.raises(NotImplementedError, match=str(gg.wide_max_width())):
        big.value_and_grad(*P, DELTA, wide=True)
    for e in (ev, big):
        assert not [a for a in vars(e) if a.startswith("last_grad")], vars(e).keys()


def test_autograd_function_takes_the_wide_route():
    """torch.autograd.gradcheck on the well-conditioned two-term problem of tests/test_gpu_grad.py, same eps and
    tolerances."""
    rng = np.random.default_rng(77)
    N = 200
    S0, w0, Q = np.array([[0.01, 0.005]]), np.array([[300.0, 900.0]]), np.array([[3.0, 8.0]])
    t = np.arange(N) * 60e-6
    y = rng.normal(size=N) * 3.0
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, yerr=2.0)
    args = tuple(torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (S0, w0, Q))
    f = lambda a, b, c: gadfly_amd.LogLikelihood.apply(a, b, c, ev, DELTA, False, True)      # noqa: E731
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-5, rtol=1e-3)
    assert ev.last_grad_seg == 15
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wide=True)
    out = f(*args)
    assert np.array_equal(out.detach().numpy(), ll)
    out.sum().backward()
    for x, k in zip(args, ("S0", "w0", "Q")):
        assert np.array_equal(x.grad.numpy(), g[k]), k


def test_not_positive_definite_problem_among_healthy_ones():
    rng = np.random.default_rng(3)
    B, J, N = 3, 40, 150
    S0, w0, Q = rng.uniform(0.5, 3.0, (B, J)), rng.uniform(50.0, 1500.0, (B, J)), rng.uniform(0.7, 20.0, (B, J))
    t = np.arange(N) * 60e-6
    y = rng.normal(size=(B, N)) * 100.0
    diag = np.full((B, N), 900.0)
    good = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, diag=diag)
    ll0, g0 = good.value_and_grad(S0, w0, Q, DELTA, wrt=ALL, wide=True)
    diag[1, 70:] = -1e9
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, DELTA), t, y, diag=diag)
    ll, g = ev.value_and_grad(S0, w0, Q, DELTA, wrt=ALL, wide=True)
    assert ll[1] == -np.inf and np.all(np.isfinite(ll[[0, 2]])) and np.all(np.isfinite(ll0))
    for k in ALL:
        assert np.all(np.isnan(g[k][1])), k
        assert np.array_equal(g[k][[0, 2]], g0[k][[0, 2]]) and np.all(np.isfinite(g[k][[0, 2]])), k
    assert np.array_equal(ll[[0, 2]], ll0[[0, 2]])
    res = gg.coefficient_gradients(ev.engine, *sho_coefficient_pack(S0, w0, Q, DELTA)[:5], wide=True)
    assert list(res["info"]) == [0, 71, 0]
