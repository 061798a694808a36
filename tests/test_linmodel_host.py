"""Host: the references of the linear-mean-model calls against each other, the numpy normal-equation solves and the
per-quarter Legendre basis.  No device."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd.linmodel import solve_normal_equations, stack_basis
from oracle import dense
from tests import grad_cases as gc
from tests import linmodel_ref as lr


@pytest.mark.parametrize("Jr,Jc,N,R", [(1, 0, 3, 2), (2, 7, 65, 5), (1, 16, 129, 9), (1, 31, 64, 3)])
def test_forward_route_equals_the_dense_answer_and_its_80_bit_run(Jr, Jc, N, R):
    """Z^T D^-1 Z of oracle/seq.py's forward sweep is [A | y]^T Sigma^-1 [A | y] of the dense matrix, and the float64
    run sits within 1e-11 of sqrt(G_ii G_jj) of its own 80-bit run (conditions of a few tens: 2e-13 measured on the
    walkers' problems)."""
    prob = lr.edge(Jr, Jc, N)
    A = lr.gaussian_basis(N, R, 0)
    for b in range(prob["B"]):
        co = gc.coefficients(prob, b)
        a = prob["diag"][b] + prob["diag_add"][b]
        G, ld, info = lr.forward_gram(prob["t"], co, a, A, prob["y"][b])
        Gd, ldd = lr.dense_gram(prob["t"], co, prob["diag"][b], A, prob["y"][b])
        Gl, ldl, _ = lr.forward_gram(prob["t"], co, a, A, prob["y"][b], np.longdouble)
        assert info == 0
        assert lr.gram_error(G, Gd) < 1e-9 and abs(ld - ldd) < 1e-10 * max(1.0, abs(ldd))
        assert lr.gram_error(G, Gl) < 1e-11 and abs(ld - float(ldl)) < 1e-12 * max(1.0, abs(float(ldl)))


def test_forward_route_reports_the_failing_row():
    prob = lr.edge(1, 8, 17)
    a = prob["diag"][0] + prob["diag_add"][0]
    a[5] = -1e9
    G, ld, info = lr.forward_gram(prob["t"], gc.coefficients(prob, 0), a, lr.gaussian_basis(17, 2, 0), prob["y"][0])
    assert info == 6 and np.all(np.isnan(G)) and np.isnan(ld)


def test_golden_dense_80_bit_answer_belongs_to_the_walkers():
    """tests/golden/linmodel/walkers_dense80.npz (the DENSE matrix in 80 bits, make_golden.py beside it) against the
    float64 forward route on the same walkers: 1e-11 of sqrt(G_ii G_jj), log det 1e-12 (2e-13 measured)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linmodel", "walkers_dense80.npz"))
    w = lr.walkers()
    assert np.array_equal(z["y_check"], w["y"][:, ::97])
    for b in range(w["B"]):
        a = np.full(w["N"], w["yerr"] ** 2) + w["diag_add"][b]
        G, ld, info = lr.forward_gram(w["t"], w["co"][b], a, w["A"], w["y"][b])
        assert info == 0 and lr.gram_error(G, z["gram_hi"][b]) < 1e-11
        assert abs(ld - z["logdet_hi"][b]) < 1e-12 * abs(ld)
        assert lr.gls_from_gram(G, ld, w["N"])["cond"] <= 1e4


def _whitened(prob, b, A):
    K = dense.dense_K(gc.coefficients(prob, b), prob["t"], prob["diag"][b])
    L = np.linalg.cholesky(K)
    return np.linalg.solve(L, A), np.linalg.solve(L, prob["y"][b]), 2.0 * np.sum(np.log(np.diag(L)))


def test_normal_equations_against_lstsq_mixed_columns_and_a_duplicate():
    """beta, cov, chi2 and both likelihoods of four problems with 3, 5, 5 and 4 real columns in a Gram matrix padded
    to 5, against numpy.linalg.lstsq on the whitened dense system; the fourth problem's basis holds one column twice:
    ok = False and NaN there, the others unaffected."""
    N, R = 65, 5
    prob = lr.edge(2, 7, N)
    ncols = np.array([3, 5, 5, 4])
    gram, logdet, want = np.zeros((4, R + 1, R + 1)), np.zeros(4), []
    for k, b in enumerate((0, 1, 2, 0)):
        A = lr.gaussian_basis(N, R, k)[:, :ncols[k]]
        if k == 3:
            A[:, 2] = A[:, 0]
        Aw, yw, logdet[k] = _whitened(prob, b, A)
        r = ncols[k]
        Z = np.concatenate([Aw, np.zeros((N, R - r)), yw[:, None]], axis=1)
        gram[k] = Z.T @ Z
        want.append((Aw, yw))
    fit = solve_normal_equations(gram, logdet, np.full(4, N), ncols)
    assert fit.ok.tolist() == [True, True, True, False]
    for f in (fit.beta, fit.cov, fit.stderr, fit.chi2, fit.ll, fit.ll_marginal):
        assert np.all(np.isnan(f[3]))
    for k in range(3):
        Aw, yw = want[k]
        r = ncols[k]
        beta, res, rank, sv = np.linalg.lstsq(Aw, yw, rcond=None)
        cov = np.linalg.inv(Aw.T @ Aw)
        se = np.sqrt(np.diag(cov))
        assert rank == r
        assert np.max(np.abs(fit.beta[k, :r] - beta) / se) < 1e-9
        assert np.all(fit.beta[k, r:] == 0.0) and np.all(fit.cov[k, r:] == 0.0) and np.all(fit.cov[k, :, r:] == 0.0)
        assert np.max(np.abs(fit.cov[k, :r, :r] - cov) / (se[:, None] * se[None, :])) < 1e-9
        assert np.array_equal(fit.cov[k], fit.cov[k].T)
        assert np.allclose(fit.stderr[k, :r], se, rtol=1e-9)
        chi2 = float(np.sum((yw - Aw @ beta) ** 2))
        assert abs(fit.chi2[k] - chi2) < 1e-9 * chi2
        ll = -0.5 * (chi2 + logdet[k] + N * np.log(2 * np.pi))
        llm = ll - 0.5 * np.linalg.slogdet(Aw.T @ Aw)[1] + 0.5 * r * np.log(2 * np.pi)
        assert abs(fit.ll[k] - ll) < 1e-10 * abs(ll) and abs(fit.ll_marginal[k] - llm) < 1e-10 * abs(llm)


def test_normal_equations_pass_a_failed_sweep_on():
    """NaN in a problem's Gram matrix (a failed pivot: info != 0) gives ok = False there alone."""
    prob = lr.edge(1, 0, 17)
    A = lr.gaussian_basis(17, 2, 0)
    G, ld, info = lr.edge_reference(prob, A)
    G[1], ld[1], info[1] = np.nan, np.nan, 4
    fit = solve_normal_equations(G, ld, np.full(3, 17), np.full(3, 2), info)
    assert fit.ok.tolist() == [True, False, True] and np.all(np.isnan(fit.beta[1])) and fit.info[1] == 4
    one = solve_normal_equations(G[2:], ld[2:], 17, 2)
    assert np.array_equal(one.beta[0], fit.beta[2]) and one.ll[0] == fit.ll[2]
    with pytest.raises(ValueError):
        solve_normal_equations(G, ld, 17, 3)


def test_quarter_polynomial_basis():
    t = np.concatenate([np.linspace(0.0, 1.0, 7), np.linspace(3.0, 3.5, 4) ** 1.1, [9.0], np.linspace(11.0, 12.0, 5)])
    breaks = [0, 7, 11, 12, 17]
    order = 3
    A = gadfly_amd.quarter_polynomial_basis(t, breaks, order)
    assert A.shape == (17, 16)
    for s in range(4):
        a, b = breaks[s], breaks[s + 1]
        blk = A[:, 4 * s:4 * s + 4]
        assert np.all(blk[:a] == 0.0) and np.all(blk[b:] == 0.0)
        if b - a == 1:
            assert blk[a].tolist() == [1.0, 0.0, 0.0, 0.0]
            continue
        assert np.allclose(blk[a], [1.0, -1.0, 1.0, -1.0], atol=1e-14)         # P_k(-1) = (-1)^k
        assert np.allclose(blk[b - 1], [1.0, 1.0, 1.0, 1.0], atol=1e-14)       # P_k(+1) = 1
    assert np.allclose(A, lr.legendre_basis(t, breaks, order), atol=1e-14)
    x = (2 * t[:7] - (t[0] + t[6])) / (t[6] - t[0])
    assert np.allclose(A[:7, 2], 0.5 * (3 * x * x - 1), atol=1e-14)
    assert gadfly_amd.quarter_polynomial_basis(t, [0, 17], 0).shape == (17, 1)
    for bad in ([0, 7, 7, 17], [1, 17], [0, 16], [0]):
        with pytest.raises(ValueError):
            gadfly_amd.quarter_polynomial_basis(t, bad, 2)


def test_stack_basis_shapes_and_errors():
    A, nc = stack_basis(np.ones((6, 2)), 3, 6)
    assert A.shape == (1, 6, 2) and nc.tolist() == [2, 2, 2]
    A, nc = stack_basis([np.ones((4, 2)), np.ones((6, 3)), np.ones((5, 1))], 3, 6, rows=[4, 6, 5])
    assert A.shape == (3, 6, 3) and nc.tolist() == [2, 3, 1]
    assert np.all(A[0, 4:] == 0.0) and np.all(A[0, :, 2:] == 0.0) and np.all(A[2, :5, 0] == 1.0)
    for basis, rows in ((np.ones((5, 2)), None), (np.ones((2, 6, 2)), None), (np.ones((6, 0)), None),
                        (np.ones((6, 256)), None), ([np.ones((6, 2))] * 2, None), ([np.ones((6, 0))] * 3, None),
                        (np.ones((6, 2)), [4, 6, 5]), ([np.ones((6, 2))] * 3, [4, 6, 5])):
        with pytest.raises(ValueError):
            stack_basis(basis, 3, 6, rows)
