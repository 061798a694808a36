"""GPU: the time-parallel gradient through the public interface --
BatchedLogLikelihood.value_and_grad(..., time_parallel=True) on the seeded walker batches of
random_cases.grad_problem against the 80-bit numpy reverse pass, a ragged list and a long series against the one-wave
route, GaussianProcess.value_and_grad against the batch call and log_likelihood, the autograd Function, and a matrix
that is not positive definite beside a healthy one."""
import functools

import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd import grad as gg
from gadfly_amd.batch import sho_coefficient_pack
from gadfly_amd.grad import parameter_vjp
from tests import grad_cases as gc
from tests import random_cases as rc
from tests.grad_ref import batch_grad

pytestmark = pytest.mark.gpu

ALL = ("S0", "w0", "Q", "mean", "diag")


@functools.lru_cache(maxsize=None)
def _reference(seed):
    """(problem, pack, 80-bit log L and coefficient adjoints, their chain rule to S0, w0, Q) of a seed: once."""
    p = rc.grad_problem(seed)
    S0, w0, Q, delta, t, y, B, N = (p[k] for k in ("S0", "w0", "Q", "delta", "t", "y", "B", "N"))
    pk = sho_coefficient_pack(S0, w0, Q, delta)[:5]
    llr, gr = batch_grad(np.broadcast_to(t, (B, N)), np.broadcast_to(y, (B, N)),
                         np.broadcast_to(p["diag_user"], (B, N)), *pk, dtype=np.longdouble)
    ref = dict(zip(("S0", "w0", "Q"), parameter_vjp(S0, w0, Q, delta, gr["real"], gr["comp"], gr["diag_add"])))
    return p, pk, llr, gr, ref


@pytest.mark.parametrize("seed", range(500, 508))
def test_random_walkers_match_the_80_bit_pass(seed):
    """Default chunks and chunks of 16 rows: log L to 1e-9, every gradient to 1e-7 (scaled), no seed and no walker
    skipped.  (In numpy the float64 chunked pass sits <= 2.8e-14 (log L) and <= 3.4e-12 (adjoints) from the 80-bit
    pass on walker 0 of seeds 500-531 at chunks of 16 and 64 rows, the sequential float64 pass <= 1.0e-11.)"""
    p, pk, llr, gr, ref = _reference(seed)
    S0, w0, Q, delta, B = (p[k] for k in ("S0", "w0", "Q", "delta", "B"))
    Jr, Jc, real, comp, _ = pk
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, delta), p["t"], p["y"], yerr=p["yerr"])
    assert np.all(np.isfinite(llr))
    for L in (None, 16):
        ll, g = ev.value_and_grad(S0, w0, Q, delta, wrt=ALL, time_parallel=True, chunk_len=L)
        assert ev.last_grad_reruns == 0 and ev.last_grad_chunk_len == (L or gg.default_chunk_len(B, p["N"], Jr + 2 * Jc))
        ll2, gco = ev.value_and_grad_coefficients(pk, time_parallel=True, chunk_len=L)
        assert np.array_equal(ll, ll2) and np.all(np.isfinite(ll))
        errs = {"ll": float(np.max(np.abs(ll - llr) / np.abs(llr)))}
        for name, theta in (("S0", S0), ("w0", w0), ("Q", Q)):
            errs[name] = max(gc.scaled_error(theta[b], g[name][b], ref[name][b]) for b in range(B))
        for i, name in enumerate(("ar", "cr")):
            errs[name] = max(gc.scaled_error(real[i, b, :Jr], gco["real"][i, b], gr["real"][i, b]) for b in range(B))
        for i, name in enumerate(("ac", "bc", "cc", "dc")):
            errs[name] = max(gc.scaled_error(comp[i, b, :Jc], gco["comp"][i, b], gr["comp"][i, b]) for b in range(B))
        for name, key in (("mean", "mean"), ("diag", "diag_add")):
            assert np.array_equal(g[name], gco[key])
            errs[name] = float(np.max(np.abs(g[name] - gr[key]) / np.maximum(1.0, np.abs(gr[key]))))
        print(f"seed {seed} {p['kind']} J={p['J']} B={B} N={p['N']} chunk_len={ev.last_grad_chunk_len}: "
              + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
        assert errs.pop("ll") <= 1e-9
        assert max(errs.values()) <= 1e-7, errs


def _close(ll, g, ll1, g1, thetas):
    assert np.all(np.abs(ll - ll1) <= 1e-9 * np.abs(ll1)), (ll, ll1)
    for name, theta in thetas.items():
        for b in range(len(ll)):
            assert gc.scaled_error(theta[b], g[name][b], g1[name][b]) <= 1e-7, (name, b)
    for name in ("mean", "diag"):
        assert np.all(np.abs(g[name] - g1[name]) <= 1e-7 * np.maximum(1.0, np.abs(g1[name]))), name


def test_ragged_list_matches_the_one_wave_route():
    rng = np.random.default_rng(31)
    J = 5
    S0, w0, Q = rng.uniform(0.5, 3.0, (2, J)), rng.uniform(50.0, 1500.0, (2, J)), rng.uniform(0.7, 20.0, (2, J))
    delta = 60e-6
    ts = [np.arange(n) * 60e-6 for n in (700, 431)]
    ys = [rng.normal(size=len(t)) * 20.0 for t in ts]
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, delta), ts, ys, yerr=[12.0, 15.0],
                                         mean=[0.5, -1.0])
    ll1, g1 = ev.value_and_grad(S0, w0, Q, delta, wrt=ALL)
    ll, g = ev.value_and_grad(S0, w0, Q, delta, wrt=ALL, time_parallel=True, chunk_len=64)
    assert ev.last_grad_reruns == 0
    _close(ll, g, ll1, g1, dict(S0=S0, w0=w0, Q=Q))


def test_long_series_default_chunking_matches_the_one_wave_route(hip):
    """edge_problem((0, 30), N = 20 000, B = 1): 200 chunks of 100 rows by the default rule, on the raw coefficient
    entry of the evaluator; the device's one-wave route as the reference, at the project's bars."""
    Jr, Jc, N = 0, 30, 20_000
    prob = gc.edge_problem(Jr, Jc, N, B=1)
    kernels = rc.sho_kernels(np.ones((1, Jc)), np.full((1, Jc), 100.0), np.full((1, Jc), 2.0), 60e-6)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, prob["t"], prob["y"], diag=prob["diag"][0])
    pk = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"])
    ll1, g1 = ev.value_and_grad_coefficients(pk)
    ll, g = ev.value_and_grad_coefficients(pk, time_parallel=True)
    L = ev.last_grad_chunk_len
    assert L == hip.load().gf_grad_chunk_len(1, N, 60) and -(-N // L) > 64 and ev.last_grad_reruns == 0
    assert np.isfinite(ll1[0]) and abs(ll[0] - ll1[0]) <= 1e-9 * abs(ll1[0])
    for i in range(4):
        assert gc.scaled_error(prob["comp"][i, 0], g["comp"][i, 0], g1["comp"][i, 0]) <= 1e-7, i
    for k in ("mean", "diag_add"):
        assert abs(g[k][0] - g1[k][0]) <= 1e-7 * max(1.0, abs(g1[k][0])), k
    print(f"N = {N}, chunk_len = {L}: time-parallel route {ev.last_grad_device_ms:.1f} ms of device time")


def _gp_problem():
    from gadfly_amd.synth import solar_like_hyperparameters
    rng = np.random.default_rng(12)
    N = 3000
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(6), texp=60.0)
    t = np.arange(N) * 60e-6
    t[N // 2:] += 40 * 60e-6
    y = rng.normal(size=N) * 40.0 + 3.0
    return kern, t, y


def test_gaussian_process_value_and_grad():
    kern, t, y = _gp_problem()
    terms = kern.term.terms
    S0, w0, Q = (np.array([[getattr(x, n) for x in terms]]) for n in ("S0", "w0", "Q"))
    gp = gadfly_amd.GaussianProcess(kern, t=t, yerr=25.0, mean=3.0)
    val, g = gp.value_and_grad(y, wrt=ALL)
    ev = gadfly_amd.BatchedLogLikelihood([kern], t, y, yerr=25.0, mean=3.0)
    ll, gb = ev.value_and_grad(S0, w0, Q, float(kern.delta), wrt=ALL, time_parallel=True)
    assert gp.last_grad_chunk_len == ev.last_grad_chunk_len
    assert val == ll[0] and np.isfinite(val)
    for k in ("S0", "w0", "Q"):
        assert g[k].shape == (len(terms),) and np.array_equal(g[k], gb[k][0]), k
    for k in ("mean", "diag"):
        assert isinstance(g[k], float) and g[k] == gb[k][0], k
    ref = gp.log_likelihood(y)
    assert abs(val - ref) <= 1e-8 * abs(ref), (val, ref)
    assert set(gp.value_and_grad(y, wrt=("Q",))[1]) == {"Q"}
    with pytest.raises(ValueError):
        gp.value_and_grad(y, wrt=("rho",))
    with pytest.raises(ValueError):
        gp.value_and_grad(y[:-1])


def test_gaussian_process_value_and_grad_refusals():
    from gadfly_amd.synth import solar_like_hyperparameters
    kern, t, y = _gp_problem()
    with pytest.raises(RuntimeError):
        gadfly_amd.GaussianProcess(kern).value_and_grad(y)
    wide = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(86), texp=60.0)
    gp = gadfly_amd.GaussianProcess(wide, t=t, yerr=25.0)
    with pytest.raises(NotImplementedError, match="63"):
        gp.value_and_grad(y)


def test_autograd_function_takes_the_time_parallel_route():
    rng = np.random.default_rng(77)
    B, N = 3, 300
    f3 = np.array([[1.0], [1.3], [0.8]])
    S0, w0, Q = np.array([[0.01, 0.005]]) * f3, np.array([[300.0, 900.0]]) / f3, np.array([[3.0, 8.0]]) * f3
    t = np.arange(N) * 60e-6
    y = rng.normal(size=N) * 3.0
    delta = 60e-6
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, delta), t, y, yerr=2.0)
    ll, g = ev.value_and_grad(S0, w0, Q, delta, time_parallel=True)
    args = tuple(torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (S0, w0, Q))
    out = gadfly_amd.LogLikelihood.apply(*args, ev, delta, True)
    assert np.array_equal(out.detach().numpy(), ll)
    wgt = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    (out * wgt).sum().backward()
    for x, k in zip(args, ("S0", "w0", "Q")):
        assert np.array_equal(x.grad.numpy(), wgt.numpy()[:, None] * g[k]), k
    # the default stays the one-wave route
    ll1, _ = ev.value_and_grad(S0, w0, Q, delta)
    assert np.array_equal(gadfly_amd.LogLikelihood.apply(*args, ev, delta).detach().numpy(), ll1)


def test_not_positive_definite_problem_beside_a_healthy_one():
    """Problem 1 loses positive definiteness at row 150 (chunk 9 of 16 rows): the chunked route flags it and it is run
    again through the one-wave kernel -- log L, info and the NaN gradients are that route's, to the bit."""
    rng = np.random.default_rng(3)
    B, J, N = 2, 4, 400
    S0, w0, Q = rng.uniform(0.5, 3.0, (B, J)), rng.uniform(50.0, 1500.0, (B, J)), rng.uniform(0.7, 20.0, (B, J))
    delta = 60e-6
    t = np.arange(N) * 60e-6
    y = rng.normal(size=(B, N)) * 20.0
    diag = np.full((B, N), 300.0)
    diag[1, 150:] = -1e7
    ev = gadfly_amd.BatchedLogLikelihood(rc.sho_kernels(S0, w0, Q, delta), t, y, diag=diag)
    ll1, g1 = ev.value_and_grad(S0, w0, Q, delta, wrt=ALL)
    ll, g = ev.value_and_grad(S0, w0, Q, delta, wrt=ALL, time_parallel=True, chunk_len=16)
    assert ev.last_grad_reruns == 1
    assert ll1[1] == -np.inf and ll[1] == -np.inf and np.isfinite(ll[0])
    for k in ALL:
        assert np.all(np.isnan(g[k][1])) and np.all(np.isnan(g1[k][1])), k
    _close(ll[:1], {k: v[:1] for k, v in g.items()}, ll1[:1], {k: v[:1] for k, v in g1.items()},
           dict(S0=S0, w0=w0, Q=Q))
    pk = sho_coefficient_pack(S0, w0, Q, delta)[:5]
    one = gg.coefficient_gradients(ev.engine, *pk)
    tp = gg.coefficient_gradients(ev.engine, *pk, time_parallel=True, chunk_len=16)
    assert one["info"][1] == 151 and np.array_equal(tp["info"], one["info"]) and tp["reruns"] == 1
    for k in ("ll", "real", "comp", "diag_add", "mean"):
        assert np.array_equal(tp[k][..., 1:2, :] if tp[k].ndim == 3 else tp[k][1:2],
                              one[k][..., 1:2, :] if one[k].ndim == 3 else one[k][1:2], equal_nan=True), k
