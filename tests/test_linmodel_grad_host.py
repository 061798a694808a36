"""CPU: the identities behind BatchedLogLikelihood.linear_value_and_grad on the host references of
its pieces (tests/linmodel_grad_ref.py): gf_loglike_grad's restatement at the fixed residual, the quadratic-form
recurrences over Sigma^-1 A F with weight 1/2 and parameter_vjp reproduce what torch autograd gives through the dense
generalised least squares likelihood, profile and marginal.  Bar: tests/test_gpu_grad.py's, theta g within 1e-7 of
max(1, max |theta g_ref|) (the composition itself sits near 1e-11)."""
import numpy as np
import pytest

from gadfly_amd.linmodel import solve_normal_equations
from tests import linmodel_grad_ref as lg

BAR = 1e-7


@pytest.fixture(scope="module")
def prob():
    return lg.problem(B=2, J=10, n_over=2, N=300, R=8)


@pytest.mark.parametrize("marginal", [False, True], ids=["profile", "marginal"])
def test_composition_matches_autograd_through_the_dense_likelihood(prob, marginal):
    ll, g = lg.composed_gradients(prob, marginal)
    llr, gr = lg.dense_reference(prob, marginal)
    assert np.all(np.abs(ll - llr) <= 1e-10 * np.abs(llr))
    for k in ("S0", "w0", "Q"):
        err = lg.scaled_error(prob[k], g[k], gr[k])
        print(f"{'marginal' if marginal else 'profile'} d/d{k}: {err:.2e}")
        assert err <= BAR, (k, err)


def test_profile_and_marginal_gradients_can_be_told_apart(prob):
    """They differ by far more than the bar: a test at the bar sees a quadratic-form term that is left out."""
    _, gp = lg.dense_reference(prob, False)
    _, gm = lg.dense_reference(prob, True)
    gap = max(lg.scaled_error(prob[k], gm[k], gp[k]) for k in ("S0", "w0", "Q"))
    assert gap > 100 * BAR


def test_factor_of_the_fit_squares_to_its_covariance():
    """LinearFit.factor: upper triangular, factor factor^T = cov to rounding, zero beyond a problem's columns, NaN for
    a problem that failed."""
    rng = np.random.default_rng(8)
    B, R = 4, 5
    Z = rng.normal(size=(B, 40, R + 1))
    gram = np.einsum("bni,bnj->bij", Z, Z)
    ncols = np.array([5, 3, 5, 5])
    gram[1, 3:5, :] = gram[1, :, 3:5] = 0.0                 # padded columns of problem 1
    gram[3, 0] = gram[3, :, 0] = 0.0                        # problem 3: a zero column -- rank-deficient
    fit = solve_normal_equations(gram, np.zeros(B), 40, ncols)
    assert fit.ok.tolist() == [True, True, True, False]
    for b in range(3):
        F = fit.factor[b]
        assert np.array_equal(F, np.triu(F))
        assert np.allclose(F @ F.T, fit.cov[b], rtol=1e-12, atol=1e-14 * np.max(np.abs(fit.cov[b])))
    assert np.all(fit.factor[1, 3:] == 0.0) and np.all(fit.factor[1, :, 3:] == 0.0)
    assert np.all(np.isnan(fit.factor[3]))
