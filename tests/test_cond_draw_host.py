"""Host: the union axes of the conditional draws, the dense restatement of Matheron's rule against the dense oracle
(the linear map z = c + A [eps; eta]: c is the conditional mean, A A^T the conditional covariance), and every error the
draw raises before anything is enqueued -- with no GPU and no library."""
import types

import numpy as np
import pytest

import gadfly_amd
from gadfly_amd import conddraw, predict
from gadfly_amd.batch import BatchedLogLikelihood
from tests import cond_draw_ref as ref
from tests import grad_cases as gc


def test_union_axes_merges_coincident_stamps_and_maps_rows_back():
    t = np.array([0.0, 1.0, 2.0, 5.0, 6.0])
    ts = np.array([-1.0, 1.0, 3.0, 3.5, 6.0, 9.0])          # before, coincident, in the gap (twice), coincident, behind
    ax = conddraw.union_axes(t, ts)
    assert len(ax.u) == 1 and np.array_equal(ax.u[0], [-1.0, 0.0, 1.0, 2.0, 3.0, 3.5, 5.0, 6.0, 9.0])
    assert np.array_equal(ax.u[0][ax.obs_rows[0]], t) and np.array_equal(ax.u[0][ax.query_rows[0]], ts)
    assert ax.nu.tolist() == [9] and ax.nobs.tolist() == [5] and ax.nq.tolist() == [6]
    assert ax.obs_rows[0].dtype == np.int64 and ax.query_rows[0].dtype == np.int64
    # M = 0 and no queries at all: the axis itself
    for none in (np.zeros(0), None):
        a0 = conddraw.union_axes(t, none)
        assert np.array_equal(a0.u[0], t) and np.array_equal(a0.obs_rows[0], np.arange(5)) and a0.nq.tolist() == [0]
    # equal stamps of one axis share a row too
    a1 = conddraw.union_axes(np.array([0.0, 1.0, 1.0, 2.0]), np.array([1.0, 1.0]))
    assert np.array_equal(a1.u[0], [0.0, 1.0, 2.0]) and a1.obs_rows[0].tolist() == [0, 1, 1, 2]
    assert a1.query_rows[0].tolist() == [1, 1]


def test_union_axes_ragged_counts_and_lists():
    t = np.array([[0.0, 1.0, 2.0, 3.0], [10.0, 11.0, 12.0, 13.0]])
    ts = np.array([[0.5, 1.0, 7.0], [9.0, 12.0, 12.0]])
    ax = conddraw.union_axes(t, ts, nobs=[4, 2], nq=[3, 1])
    assert ax.nobs.tolist() == [4, 2] and ax.nq.tolist() == [3, 1] and ax.nu.tolist() == [6, 3]
    assert np.array_equal(ax.u[1], [9.0, 10.0, 11.0])
    for b in range(2):
        assert np.array_equal(ax.u[b][ax.obs_rows[b]], t[b, :ax.nobs[b]])
        assert np.array_equal(ax.u[b][ax.query_rows[b]], ts[b, :ax.nq[b]])
    # a shared observed axis with a list of per-problem queries of different lengths
    ax = conddraw.union_axes(t[0], [np.array([0.5]), np.array([-1.0, 3.0, 4.0]), np.zeros(0)])
    assert ax.nu.tolist() == [5, 6, 4] and ax.nq.tolist() == [1, 3, 0] and ax.nobs.tolist() == [4, 4, 4]
    # a list of observed series of different lengths
    ax = conddraw.union_axes([t[0], t[1, :2]], [np.array([1.5]), np.array([10.0, 10.5])])
    assert ax.nu.tolist() == [5, 3] and ax.obs_rows[1].tolist() == [0, 2] and ax.query_rows[1].tolist() == [0, 1]
    with pytest.raises(ValueError, match="dimension"):
        conddraw.union_axes(t, ts, nobs=[4, 5])
    with pytest.raises(ValueError, match="series"):
        conddraw.union_axes(t, [np.zeros(1)] * 3)


@pytest.mark.parametrize("Jr,Jc", ref.STRUCTURES)
def test_linear_map_of_the_restatement_is_the_dense_conditional(Jr, Jc):
    """z = c + A [eps; eta]: c equals the dense conditional mean and A A^T the dense K** - K*^T Sigma^-1 K* (at the
    observed stamps K - K Sigma^-1 K), for every (N, M) of cond_draw_ref.SHAPES.  The size of the disagreement is the
    yardstick of the GPU bar (cond_draw_ref.yardstick); here it is held to 1e-11 (of K(0); of
    max |mean| for c): the draw enters A A^T through L_u L_u^T only, which a dense Cholesky factor reproduces to a few
    (Nu + N) eps of K(0) whatever the condition of the noise-free K_u (1e8 .. 1e13 here), and the solves with Sigma
    (condition ~6e2) lose cond eps on top: 97 x 1.1e-16 x 6e2 = 6e-12."""
    for N, M in ref.SHAPES:
        prob = ref.problem(Jr, Jc, N, M)
        for b in range(prob["B"]):
            co, k0 = gc.coefficients(prob, b), prob["diag_add"][b]
            args = (co, 0.0, prob["t"], prob["diag"][b], prob["y"][b], prob["mean"][b])
            for ts in ((prob["ts"][b], None) if M else (None,)):
                A, c = ref.linear_map(*args, ts)
                mu, cov = ref.dense_posterior(*args, ts)
                nu = int(conddraw.union_axes(prob["t"], ts).nu[0])
                assert A.shape == ((M if ts is not None else N), nu + N)
                assert np.max(np.abs(c - mu)) <= 1e-11 * np.max(np.abs(mu)), (N, M, b)
                assert np.max(np.abs(A @ A.T - cov)) <= 1e-11 * k0, (N, M, b)
    wc, wcov = ref.yardstick()
    print(f"yardstick: offset {wc:.2e} of max |mean|, A A^T {wcov:.2e} of K(0)")
    assert wc <= 1e-11 and wcov <= 1e-11


def test_draws_at_coincident_queries_equal_the_draws_at_those_stamps():
    """A query on an observed stamp shares its row: the draw there is the draw at the observed stamp."""
    prob = ref.problem(0, 3, 12, 9)
    co = gc.coefficients(prob, 1)
    t, dg, y, m = prob["t"], prob["diag"][1], prob["y"][1], prob["mean"][1]
    ts = t[[2, 7]]
    rng = np.random.default_rng(5)
    eps, eta = rng.normal(size=(2, 12)), rng.normal(size=(2, 12))
    at = ref.draw(co, 0.0, t, dg, y, m, ts, eps, eta)
    obs = ref.draw(co, 0.0, t, dg, y, m, None, eps, eta)
    assert np.allclose(at, obs[:, [2, 7]], rtol=0, atol=1e-9 * np.max(np.abs(obs)))


def test_threaded_kernel_matrix_is_the_dense_oracles():
    from oracle import dense
    prob = ref.problem(0, 30, 40, 17)
    co = gc.coefficients(prob, 2)
    want = dense.kernel_value(co, prob["ts"][2][:, None] - prob["t"][None, :])
    got = ref.kernel_matrix(co, prob["ts"][2], prob["t"])
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want))


def test_errors_are_raised_on_the_host():
    # W = 64
    with pytest.raises(NotImplementedError, match="64"):
        predict.check_width(64)
    t = np.arange(10.0)
    # unsorted queries
    with pytest.raises(ValueError, match="sorted"):
        conddraw.union_axes(t, np.array([3.0, 2.0]))
    with pytest.raises(ValueError, match="sorted"):
        BatchedLogLikelihood._query_times(types.SimpleNamespace(B=1), np.array([3.0, 2.0]))
    # exposure-integrated kernel: a query half an exposure from a DIFFERENT stamp, or from another query
    delta = 1.0
    ok = conddraw.union_axes(t, np.array([-2.0, 3.0, 20.0]))          # coincident with a stamp: merged, fine
    conddraw.check_exposure(ok, [delta])
    conddraw.check_exposure(conddraw.union_axes(t, np.array([3.5])), [0.0])      # not integrated: anything goes
    with pytest.raises(ValueError, match=r"problem 0: observed stamp 3\.0 and query 3\.5"):
        conddraw.check_exposure(conddraw.union_axes(t, np.array([3.5, 30.0])), [delta])
    with pytest.raises(ValueError, match=r"problem 1: query 20\.0 and query 20\.5"):
        conddraw.check_exposure(conddraw.union_axes(t, [np.array([30.0]), np.array([20.0, 20.5])]), [delta, delta])
    # observed stamps closer than the exposure time are the caller's own axis: not this check's business
    conddraw.check_exposure(conddraw.union_axes(np.array([0.0, 0.5, 5.0]), np.array([2.0])), [delta])
    # within the slack of batch._exposure_resolved (10 %)
    conddraw.check_exposure(conddraw.union_axes(2.0 * t, np.array([2.0 + 0.95 * delta])), [delta])
    with pytest.raises(ValueError, match="exposure time"):
        conddraw.check_exposure(conddraw.union_axes(2.0 * t, np.array([2.0 + 0.85 * delta])), [delta])
    # normals of the wrong shape
    ax = conddraw.union_axes(np.stack([t, t + 0.25]), np.array([0.5, 4.6, 11.0]))
    assert ax.nu.tolist() == [13, 13]
    conddraw.check_normals((np.zeros((2, 4, 13)), np.zeros((2, 4, 10))), ax, 4)
    conddraw.check_normals((np.zeros((2, 13)), np.zeros((2, 10))), ax, None)
    conddraw.check_normals(([np.zeros((4, 13))] * 2, [np.zeros((4, 10))] * 2), ax, 4)
    for bad in ((np.zeros((2, 4, 12)), np.zeros((2, 4, 10))), (np.zeros((2, 4, 13)), np.zeros((2, 4, 13))),
                (np.zeros((2, 13)), np.zeros((2, 10))), (np.zeros((2, 4, 13)),), np.zeros((2, 4, 13))):
        with pytest.raises(ValueError, match="normals"):
            conddraw.check_normals(bad, ax, 4)
    rag = conddraw.union_axes(t, [np.array([0.5]), np.array([0.5, 1.5])])
    with pytest.raises(ValueError, match="list"):
        conddraw.check_normals((np.zeros((2, 11)), np.zeros((2, 10))), rag, None)
    conddraw.check_normals(([np.zeros(11), np.zeros(12)], np.zeros((2, 10))), rag, None)
    # a mean that varies along the rows, together with t=
    fake = types.SimpleNamespace(_mean=np.arange(10.0), rows=None, B=1)
    with pytest.raises(ValueError, match="varies along the rows"):
        BatchedLogLikelihood._mean_per_problem(fake)
    # the public names exist
    assert callable(gadfly_amd.sample_conditional_batch)
    for name in ("sample_conditional_device", "sample_conditional", "apply_inverse_device", "log_likelihood_device"):
        assert callable(getattr(BatchedLogLikelihood, name))
    assert callable(gadfly_amd.GaussianProcess.sample_conditional)
