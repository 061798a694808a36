"""GPU: gradients of the profile and the marginal likelihood of linear mean models through the
public interface -- BatchedLogLikelihood.linear_value_and_grad / linear_value_and_grad_coefficients and
gadfly_amd.LinearModelLogLikelihood -- against torch autograd through the dense generalised least squares likelihood
(tests/linmodel_grad_ref.py).  Bar: tests/test_gpu_grad.py's, theta g within 1e-7 of max(1, max |theta g_ref|)."""
import functools

import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd.batch import sho_coefficient_pack
from tests import cond_draw_ref as cdr
from tests import grad_cases as gc
from tests import linmodel_grad_ref as lg
from tests import linmodel_ref as lr

pytestmark = pytest.mark.gpu

BAR = 1e-7
DELTA = lg.DELTA
MODES = pytest.mark.parametrize("marginal", [False, True], ids=["profile", "marginal"])


def _kernels_like(S0, w0, Q):
    """Exposure-integrated SHO sums of (B, J) parameters (the batch's kernels; the calls bring their own)."""
    from gadfly_amd.terms import SHOTerm, TermConvolution, TermSum
    return [TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q)) for s, w, q in zip(*r)]), DELTA)
            for r in zip(S0, w0, Q)]


def _evaluator(prob, which=slice(None), **kw):
    S0, w0, Q = (prob[k][which] for k in ("S0", "w0", "Q"))
    return gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), prob["t"], prob["y"][which],
                                           diag=prob["diag"], **kw)


@functools.lru_cache(maxsize=None)
def _reference(marginal):
    return lg.dense_reference(lg.problem(), marginal)


def _same(g1, g2, b1=slice(None), b2=slice(None)):
    return all(np.array_equal(g1[k][b1], g2[k][b2]) for k in ("S0", "w0", "Q"))


@MODES
def test_matches_autograd_through_the_dense_likelihood(marginal):
    prob = lg.problem()
    ev = _evaluator(prob)
    ll, g, fit = ev.linear_value_and_grad(prob["A"], prob["S0"], prob["w0"], prob["Q"], DELTA, marginal=marginal,
                                          wrt=("S0", "w0", "Q", "diag"), return_fit=True)
    llr, gr = _reference(marginal)
    assert np.all(fit.ok) and np.all(np.abs(ll - llr) <= 1e-9 * np.abs(llr))
    for k in ("S0", "w0", "Q"):
        err = lg.scaled_error(prob[k], g[k], gr[k])
        print(f"{'marginal' if marginal else 'profile'} d/d{k}: {err:.2e}")
        assert g[k].shape == prob[k].shape and err <= BAR, (k, err)
    assert g["diag"].shape == (prob["B"],) and np.all(np.isfinite(g["diag"]))
    # the value is fit_linear's, bit for bit
    ref = ev.fit_linear(prob["A"], sho_coefficient_pack(prob["S0"], prob["w0"], prob["Q"], DELTA))
    assert np.array_equal(ll, ref.ll_marginal if marginal else ref.ll)
    assert np.array_equal(fit.beta, ref.beta)


def test_the_two_modes_differ_by_far_more_than_the_bar():
    """... on the device as in the reference (about 20 % here): the marginal test above fails if the quadratic-form term
    is left out."""
    prob = lg.problem()
    ev = _evaluator(prob)
    args = (prob["A"], prob["S0"], prob["w0"], prob["Q"], DELTA)
    _, gp = ev.linear_value_and_grad(*args)
    _, gm = ev.linear_value_and_grad(*args, marginal=True)
    for got, ref in ((gp, gm), (_reference(False)[1], _reference(True)[1]), (gp, _reference(True)[1])):
        gap = max(lg.scaled_error(prob[k], got[k], ref[k]) for k in ("S0", "w0", "Q"))
        assert gap > 100 * BAR, gap


@pytest.mark.parametrize("Jr,Jc", [(2, 30), (3, 30)], ids=["W62", "W63"])
@MODES
def test_widest_kernels_at_the_coefficient_adjoints(Jr, Jc, marginal):
    """W = 62 and 63 at N = 129, raw coefficients (an odd width cannot be had from SHO terms)."""
    N, R = 129, 8
    prob = gc.edge_problem(Jr, Jc, N)
    A = lr.gaussian_basis(N, R, Jr + 2 * Jc)
    ev = gadfly_amd.BatchedLogLikelihood(cdr.kernels(prob), prob["t"], prob["y"], diag=prob["diag"])
    pack = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"])
    ll, g = ev.linear_value_and_grad_coefficients(A, pack, marginal=marginal)
    fit = ev.fit_linear(A, pack)
    assert np.array_equal(ll, fit.ll_marginal if marginal else fit.ll)
    for b in range(prob["B"]):
        llr, gr = lg.dense_coefficient_linear_grad(prob, b, A, marginal)
        assert abs(ll[b] - llr) <= 1e-9 * abs(llr)
        co = gc.coefficients(prob, b)
        got = (g["real"][0, b], g["real"][1, b], g["comp"][0, b], g["comp"][1, b], g["comp"][2, b], g["comp"][3, b])
        for name, theta, gg in zip(gc.NAMES, co, got):
            err = gc.scaled_error(theta, gg, gr[name])
            assert err <= BAR, (b, name, err)
        assert abs(g["diag_add"][b] - gr["diag_add"]) <= BAR * max(1.0, abs(gr["diag_add"]))


@MODES
def test_ragged_batch_and_column_counts_have_the_bits_of_calls_of_their_own(marginal):
    prob = lg.problem()
    lens, cols = (300, 220, 150), (8, 5, 3)
    ts = [prob["t"][:n] for n in lens]
    ys = [prob["y"][b, :n] for b, n in enumerate(lens)]
    bases = [prob["A"][:n, :r] for n, r in zip(lens, cols)]
    S0, w0, Q = prob["S0"], prob["w0"], prob["Q"]
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), ts, ys, yerr=18.0)
    ll, g = ev.linear_value_and_grad(bases, S0, w0, Q, DELTA, marginal=marginal, wrt=("S0", "w0", "Q", "diag"))
    assert np.all(np.isfinite(ll))
    for b in range(3):
        s = slice(b, b + 1)
        one = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0[s], w0[s], Q[s]), ts[b], ys[b], yerr=18.0)
        l1, g1 = one.linear_value_and_grad(bases[b], S0[s], w0[s], Q[s], DELTA, marginal=marginal,
                                           wrt=("S0", "w0", "Q", "diag"))
        assert l1[0] == ll[b], b
        assert _same(g1, g, 0, b) and g1["diag"][0] == g["diag"][b], b
    # equal lengths, unequal column counts: the grouped route with padded columns
    evr = _evaluator(prob)
    full = [prob["A"][:, :r] for r in cols]
    ll, g = evr.linear_value_and_grad(full, S0, w0, Q, DELTA, marginal=marginal)
    for b in range(3):
        s = slice(b, b + 1)
        l1, g1 = _evaluator(prob, s).linear_value_and_grad(full[b], S0[s], w0[s], Q[s], DELTA, marginal=marginal)
        assert l1[0] == ll[b] and _same(g1, g, 0, b), b


@MODES
def test_groups_under_a_small_workspace_cap_change_no_bit(marginal):
    prob = lg.problem()
    ev = _evaluator(prob)
    args = (prob["A"], prob["S0"], prob["w0"], prob["Q"], DELTA)
    ll, g = ev.linear_value_and_grad(*args, marginal=marginal)
    assert ev.last_linear_plan[1] == 1 and ev.last_linear_grad_plan[1] == 1
    ev.grad_workspace_bytes = ev.predict_workspace_bytes = ev.linear_workspace_bytes = 1      # one problem per group
    ll2, g2 = ev.linear_value_and_grad(*args, marginal=marginal)
    assert ev.last_linear_plan[1] == 3 and ev.last_linear_grad_plan[1] == 3
    assert np.array_equal(ll, ll2) and _same(g, g2)
    assert set(ev.last_linear_grad_ms) == ({"gram", "residual", "grad", "solve", "product", "quadform"} if marginal
                                           else {"gram", "residual", "grad"})


@MODES
def test_failed_problems_get_nan_and_their_neighbours_keep_their_bits(marginal):
    prob = lg.problem()
    B, N = prob["B"], prob["N"]
    S0, w0, Q = prob["S0"], prob["w0"], prob["Q"]
    good = _evaluator(prob)
    llg, gg = good.linear_value_and_grad(prob["A"], S0, w0, Q, DELTA, marginal=marginal)
    # a failed pivot: problem 1 loses positive definiteness at row 101
    diag = np.broadcast_to(prob["diag"], (B, N)).copy()
    diag[1, 100:] = -1e6
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), np.broadcast_to(prob["t"], (B, N)), prob["y"],
                                         diag=diag)
    ll, g, fit = ev.linear_value_and_grad(prob["A"], S0, w0, Q, DELTA, marginal=marginal, return_fit=True,
                                          wrt=("S0", "w0", "Q", "diag"))
    assert fit.ok.tolist() == [True, False, True] and fit.info[1] == 101 and np.isnan(ll[1])
    assert all(np.all(np.isnan(v[1])) for v in g.values())
    for b in (0, 2):
        assert ll[b] == llg[b] and _same(g, gg, b, b)
    # a rank-deficient basis: problem 2's last column repeats its first
    A = np.broadcast_to(prob["A"], (B,) + prob["A"].shape).copy()
    A[2, :, -1] = A[2, :, 0]
    ll, g, fit = good.linear_value_and_grad(A, S0, w0, Q, DELTA, marginal=marginal, return_fit=True)
    assert fit.ok.tolist() == [True, True, False] and np.isnan(ll[2])
    assert all(np.all(np.isnan(v[2])) for v in g.values())
    for b in (0, 1):
        assert ll[b] == llg[b] and _same(g, gg, b, b)


def test_errors_come_before_anything_is_enqueued():
    rng = np.random.default_rng(66)
    B, J, N = 2, 32, 129                                     # W = 64
    S0, w0, Q = rng.uniform(0.5, 3.0, (B, J)), rng.uniform(50.0, 1500.0, (B, J)), rng.uniform(0.7, 20.0, (B, J))
    t = np.arange(N) * lg.DT
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), t, rng.normal(size=N), yerr=1.0)
    A = np.ones((N, 2))
    with pytest.raises(NotImplementedError, match="64"):
        ev.linear_value_and_grad(A, S0, w0, Q, DELTA)
    with pytest.raises(NotImplementedError, match="64"):
        ev.linear_value_and_grad(A, S0, w0, Q, DELTA, marginal=True)
    assert not hasattr(ev, "last_linear_plan") and not hasattr(ev, "last_linear_fit")
    prob = lg.problem()
    ev = _evaluator(prob)
    args = (prob["S0"], prob["w0"], prob["Q"], DELTA)
    with pytest.raises(ValueError, match="unknown gradient names"):
        ev.linear_value_and_grad(prob["A"], *args, wrt=("S0", "mean"))
    with pytest.raises(ValueError, match="batch"):
        ev.linear_value_and_grad(prob["A"], prob["S0"][:2], prob["w0"][:2], prob["Q"][:2], DELTA)
    with pytest.raises(ValueError, match="dimension mismatch"):
        ev.linear_value_and_grad(prob["A"][:-1], *args)
    with pytest.raises(ValueError, match="columns"):
        ev.linear_value_and_grad(np.ones((prob["N"], 256)), *args)
    assert not hasattr(ev, "last_linear_plan")
    ll, _ = ev.linear_value_and_grad(prob["A"], *args)       # the evaluator is still usable
    assert np.all(np.isfinite(ll))


@MODES
def test_autograd_function_gradcheck_and_optimiser_step(marginal):
    rng = np.random.default_rng(77)
    N = 60
    # a well-conditioned tiny problem, as tests/test_gpu_grad.py's: the numerical Jacobian's own noise stays far
    # below the tolerance
    f3 = np.array([[1.0], [1.3], [0.8]])
    S0, w0, Q = np.array([[0.01, 0.005]]) * f3, np.array([[300.0, 900.0]]) / f3, np.array([[3.0, 8.0]]) * f3
    t = np.arange(N) * lg.DT
    A = np.stack([np.ones(N), np.linspace(-1.0, 1.0, N)], axis=1)
    y = rng.normal(size=N) * 3.0 + A @ np.array([5.0, -2.0])
    ev = gadfly_amd.BatchedLogLikelihood(_kernels_like(S0, w0, Q), t, y, yerr=2.0)
    args = tuple(torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (S0, w0, Q))
    f = lambda a, b, c: gadfly_amd.LinearModelLogLikelihood.apply(a, b, c, ev, A, DELTA, marginal)    # noqa: E731
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-5, rtol=1e-3)
    x = torch.tensor(np.log(np.stack([S0, w0, Q]) * 1.2), requires_grad=True)
    opt = torch.optim.SGD([x], lr=1e-4)
    opt.zero_grad()
    e = torch.exp(x)
    loss = -gadfly_amd.LinearModelLogLikelihood.apply(e[0], e[1], e[2], ev, A, DELTA, marginal).sum()
    loss.backward()
    assert x.grad.shape == x.shape and bool(torch.all(torch.isfinite(x.grad))) and float(x.grad.norm()) > 0.0
    opt.step()
