"""GPU: linear mean models from one forward sweep (gf_linear_gram, BatchedLogLikelihood.linear_gram_device /
fit_linear).

The edge grid runs the raw C entry point on tests/grad_cases.edge_problem's coefficients: every instance of the sweep
kernel and both sides of each instance boundary, lengths around the 64-row blocks, column counts whose R + 1 crosses
each block of 64 columns.  Bars: every Gram entry within 1e-10 of sqrt(G_ii G_jj) of oracle/seq.py's float64 forward
route (tests/linmodel_ref.py; that route sits 2e-13 from its 80-bit run), log det within 1e-12 relative; the walkers'
beta within 1e-8 of a standard error, cov within 1e-8 of sqrt(C_ii C_jj), both likelihoods within 1e-9 relative of the
DENSE 80-bit answer (tests/golden/linmodel/walkers_dense80.npz).  Worst values of the edge grid are printed."""
import functools
import os

import numpy as np
import pytest
import torch

import gadfly_amd
from gadfly_amd.linmodel import solve_normal_equations
from tests import fused_cases as fc
from tests import linmodel_ref as lr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
INFO_SENTINEL = -77
GRAM_BAR, LOGDET_BAR = 1e-10, 1e-12
#: W = 1, 2, 16, 17, 32, 33, 62, 63: k_lin_sweep<16>, <32>, <64>, both sides of each boundary, real and complex mixed
STRUCTURES = ((1, 0), (0, 1), (0, 8), (1, 8), (0, 16), (1, 16), (0, 31), (1, 31))
LENGTHS = (1, 2, 3, 63, 64, 65, 129)
COLUMNS = (1, 2, 62, 63, 64, 65, 127, 128)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linmodel", "walkers_dense80.npz")


def _dev(x, dtype=np.float64):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C")).cuda()


def gram_call(hip, prob, A, nobs=None):
    """One gf_linear_gram call on an edge problem: A (N, R) shared or (B, N, R).  Outputs one problem too long,
    sentinel beyond; the workspace starts as NaN."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, N, nb = prob["Jr"], prob["Jc"], prob["N"], prob["y"].shape[0]
    R = A.shape[-1]
    C = R + 1
    per = int(lib.gf_linear_gram_work(N, Jr + 2 * Jc, R))
    assert per > 0
    work = torch.full((nb * per,), float("nan"), dtype=torch.float64, device="cuda")
    rd, cd, ad = _dev(prob["real"]), _dev(prob["comp"]), _dev(prob["diag_add"])
    td, dd, yd, Ad = _dev(prob["t"]), _dev(prob["diag"]), _dev(prob["y"]), _dev(A)
    nd = None if nobs is None else _dev(nobs, np.int64)
    gram = torch.full(((nb + 1) * C * C,), SENTINEL, dtype=torch.float64, device="cuda")
    logdet = torch.full((nb + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    info = torch.full((nb + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_linear_gram(nb, N, R, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                            p(td), 0 if prob["t"].ndim == 1 else N, p(dd), N, p(yd), N, p(nd),
                            p(Ad), R, 0 if A.ndim == 2 else N * R, p(work), per, p(gram), p(logdet), p(info), None)
    hip.check(rc, "gf_linear_gram")
    torch.cuda.synchronize()
    g, ld, inf = gram.cpu().numpy(), logdet.cpu().numpy(), info.cpu().numpy()
    assert np.all(g[nb * C * C:] == SENTINEL) and ld[nb] == SENTINEL and inf[nb] == INFO_SENTINEL
    return g[:nb * C * C].reshape(nb, C, C), ld[:nb], inf[:nb]


@functools.lru_cache(maxsize=None)
def edge_case(Jr, Jc, N):
    """(problem, A (N, 128) Gaussian, the float64 reference's gram (B, 129, 129), logdet) -- the reference of fewer
    columns is the leading block and the y row and column of this one."""
    prob = lr.edge(Jr, Jc, N)
    A = lr.gaussian_basis(N, max(COLUMNS), Jr + 2 * Jc)
    G, ld, info = lr.edge_reference(prob, A)
    assert np.all(info == 0)
    return prob, A, G, ld


def _lead(G, R):
    """The leading R columns and the last one of (B, C, C) Gram matrices."""
    k = np.r_[np.arange(R), G.shape[-1] - 1]
    return G[:, k][:, :, k]


@pytest.mark.parametrize("Jr,Jc", STRUCTURES, ids=[fc.ident(s) for s in STRUCTURES])
def test_edge_grid_against_the_float64_forward_route(hip, Jr, Jc):
    worst_g = worst_l = 0.0
    for N in LENGTHS:
        prob, A, G, ld = edge_case(Jr, Jc, N)
        wide = None
        for R in reversed(COLUMNS):
            g, l, inf = gram_call(hip, prob, A[:, :R])
            assert np.all(inf == 0), (N, R)
            ref = _lead(G, R)
            for b in range(g.shape[0]):
                assert np.array_equal(g[b], g[b].T), (N, R, b)
                worst_g = max(worst_g, lr.gram_error(g[b], ref[b]))
            worst_l = max(worst_l, float(np.max(np.abs(l - ld) / np.maximum(1.0, np.abs(ld)))))
            if wide is None:
                wide = g, l
            else:           # fewer columns: the same bits as the leading block of the widest call
                assert np.array_equal(g, _lead(wide[0], R)) and np.array_equal(l, wide[1]), (N, R)
    print(f"linear gram W={Jr + 2 * Jc}: worst entry {worst_g:.2e} of sqrt(G_ii G_jj), worst logdet {worst_l:.2e}")
    assert worst_g < GRAM_BAR and worst_l < LOGDET_BAR


@pytest.mark.parametrize("Jr,Jc", STRUCTURES, ids=[fc.ident(s) for s in STRUCTURES])
def test_edge_legendre_basis_per_problem_matrices_and_row_counts(hip, Jr, Jc):
    """A per-segment Legendre basis (segments of 40, 1 and 88 rows, order 3) as one matrix per problem, and the same
    call with nobs = (129, 64, 1): a problem stopped early has the bits of the call on its first rows alone, and its
    later rows (NaN here) are never read."""
    N = 129
    prob = lr.edge(Jr, Jc, N)
    A1 = gadfly_amd.quarter_polynomial_basis(prob["t"], [0, 40, 41, N], 3)
    A = np.stack([A1 * (1.0 + 0.5 * b) for b in range(3)])
    G, ld, _ = lr.edge_reference(prob, A)
    g, l, inf = gram_call(hip, prob, A)
    assert np.all(inf == 0)
    worst = max(lr.gram_error(g[b], G[b]) for b in range(3))
    print(f"linear gram W={Jr + 2 * Jc}, Legendre basis: worst entry {worst:.2e}")
    assert worst < GRAM_BAR and np.max(np.abs(l - ld) / np.abs(ld)) < LOGDET_BAR
    nobs = np.array([N, 64, 1])
    cut = {k: np.array(prob[k]) for k in ("y", "diag")}
    Ac = A.copy()
    for b, n in enumerate(nobs):
        cut["y"][b, n:], cut["diag"][b, n:], Ac[b, n:] = np.nan, np.nan, np.nan
    gn, ln, infn = gram_call(hip, dict(prob, **cut), Ac, nobs=nobs)
    assert np.all(infn == 0) and np.array_equal(gn[0], g[0]) and ln[0] == l[0]
    for b in (1, 2):
        n = int(nobs[b])
        short = dict(prob, N=n, t=prob["t"][:n], y=prob["y"][b:b + 1, :n], diag=prob["diag"][b:b + 1, :n],
                     real=prob["real"][:, b:b + 1], comp=prob["comp"][:, b:b + 1], diag_add=prob["diag_add"][b:b + 1])
        g1, l1, i1 = gram_call(hip, short, A[b:b + 1, :n])
        assert i1[0] == 0 and np.array_equal(gn[b], g1[0]) and ln[b] == l1[0], b


# ---- the walkers, through the public calls -----------------------------------------------------------------------------

def _evaluator(w, sel=None, **kw):
    sel = range(w["B"]) if sel is None else sel
    return gadfly_amd.BatchedLogLikelihood([w["kernels"][b] for b in sel], w["t"], w["y"][list(sel)],
                                           yerr=w["yerr"], **kw)


def _golden():
    z = np.load(GOLDEN)
    ld = np.longdouble
    return (z["gram_hi"].astype(ld) + z["gram_lo"].astype(ld), z["logdet_hi"].astype(ld) + z["logdet_lo"].astype(ld),
            z["y_check"])


def _fit_errors(fit, b, ref):
    se = np.sqrt(np.diag(ref["cov"]).astype(np.float64))
    return (float(np.max(np.abs(fit.beta[b] - ref["beta"].astype(np.float64)) / se)),
            float(np.max(np.abs(fit.cov[b] - ref["cov"].astype(np.float64)) / (se[:, None] * se[None, :]))),
            abs(fit.ll[b] - float(ref["ll"])) / abs(float(ref["ll"])),
            abs(fit.ll_marginal[b] - float(ref["ll_marginal"])) / abs(float(ref["ll_marginal"])))


def test_walkers_against_the_dense_80_bit_answer(hip):
    w = lr.walkers()
    G80, ld80, ycheck = _golden()
    assert np.array_equal(ycheck, w["y"][:, ::97]), "the golden file belongs to other data: run its make_golden.py"
    fit = _evaluator(w).fit_linear(w["A"])
    assert fit.ok.all() and np.all(fit.info == 0) and np.all(fit.ncols == 12)
    for b in range(w["B"]):
        ref = lr.gls_from_gram(G80[b], ld80[b], w["N"])
        assert ref["cond"] <= 1e4, ref["cond"]
        eb, ec, el, em = _fit_errors(fit, b, ref)
        print(f"walker {b}: cond {ref['cond']:.0f}, beta {eb:.1e} se, cov {ec:.1e}, ll {el:.1e}, marginal {em:.1e}")
        assert eb < 1e-8 and ec < 1e-8 and el < 1e-9 and em < 1e-9
        assert np.allclose(fit.stderr[b], np.sqrt(np.diag(fit.cov[b])), rtol=0, atol=0)


def test_walkers_on_a_jd_based_axis(hip):
    """The same problem at t + 2454833 d against the float64 forward route on that axis, at the project's bar there."""
    w = lr.walkers(shift=fc.SHIFT)
    fit = _evaluator(w).fit_linear(w["A"])
    assert fit.ok.all()
    for b in range(w["B"]):
        a = np.full(w["N"], w["yerr"] ** 2) + w["diag_add"][b]
        G, ld, info = lr.forward_gram(w["t"], w["co"][b], a, w["A"], w["y"][b])
        ref = lr.gls_from_gram(G, ld, w["N"])
        assert info == 0 and ref["cond"] <= 1e4
        errs = _fit_errors(fit, b, ref)
        print(f"walker {b}, JD axis: beta {errs[0]:.1e} se, cov {errs[1]:.1e}, ll {errs[2]:.1e}, {errs[3]:.1e}")
        assert max(errs) < 1e-8


def test_consistent_with_the_solve_calls(hip):
    """gram[R, R] and logdet give log_likelihood_device(y); gram[:R, :R] is A^T apply_inverse_device(A^T)."""
    w = lr.walkers()
    ev = _evaluator(w)
    gram, logdet, info = ev.linear_gram_device(w["A"])
    R = w["A"].shape[1]
    assert gram.shape == (w["B"], R + 1, R + 1) and gram.is_cuda and info.dtype == torch.int32
    g, ld = gram.cpu().numpy(), logdet.cpu().numpy()
    ll = ev.log_likelihood_device(w["y"]).cpu().numpy().reshape(-1)
    mine = -0.5 * (g[:, R, R] + ld + w["N"] * np.log(2 * np.pi))
    assert np.max(np.abs(mine - ll) / np.abs(ll)) < 1e-12
    alpha = ev.apply_inverse_device(w["A"].T.copy()).cpu().numpy()              # (B, R, N)
    prod = alpha @ w["A"]
    for b in range(w["B"]):
        assert lr.gram_error(g[b, :R, :R], 0.5 * (prod[b] + prod[b].T)) < 1e-10


def _bits(ev, basis):
    g, ld, info = ev.linear_gram_device(basis)
    return g.cpu().numpy(), ld.cpu().numpy(), info.cpu().numpy()


def test_bit_identities(hip):
    w = lr.walkers()
    ev = _evaluator(w)
    A = w["A"]
    R = A.shape[1]
    g, ld, info = _bits(ev, A)
    g2, ld2, _ = _bits(ev, A)
    assert np.array_equal(g, g2) and np.array_equal(ld, ld2)                   # two runs
    for b in (0, 3):                                                           # alone
        g1, ld1, _ = _bits(_evaluator(w, [b]), A)
        assert np.array_equal(g1[0], g[b]) and ld1[0] == ld[b]
    per = int(hip.load().gf_linear_gram_work(w["N"], 60, R))
    ev.linear_workspace_bytes = 8 * per * 2 + 8                                # groups of 2, 2, 1
    gg, ldg, _ = _bits(ev, A)
    assert ev.last_linear_plan[1:] == (3, 2)
    assert np.array_equal(gg, g) and np.array_equal(ldg, ld)
    ev.linear_workspace_bytes = type(ev).linear_workspace_bytes
    extra = np.concatenate([A, lr.gaussian_basis(w["N"], 60, 1)], axis=1)      # 72 columns: a second block of 64
    ge, lde, _ = _bits(ev, extra)
    assert np.array_equal(_lead(ge, R), g) and np.array_equal(lde, ld)
    padded = [np.concatenate([A, np.zeros((w["N"], 5))], axis=1)] + [A] * 4    # a list: problem 0 sets the width
    gp, ldp, _ = _bits(ev, padded)
    assert gp.shape[1] == R + 6 and np.array_equal(_lead(gp, R), g) and np.all(gp[:, R:R + 5] == 0.0)


def test_ragged_batch_equals_calls_of_their_own(hip):
    """Three series of 900, 640 and 333 rows with three, two and one quarter."""
    w = lr.walkers()
    rows, brk = (900, 640, 333), ((0, 300, 607, 900), (0, 300, 640), (0, 333))
    ts, ys = [w["t"][:n] for n in rows], [w["y"][b, :n] for b, n in enumerate(rows)]
    bases = [gadfly_amd.quarter_polynomial_basis(t, bk, 3) for t, bk in zip(ts, brk)]
    ks = list(w["kernels"][:3])
    ev = gadfly_amd.BatchedLogLikelihood(ks, ts, ys, yerr=w["yerr"], mean=1.5)
    g, ld, info = _bits(ev, bases)
    fit = ev.fit_linear(bases)
    assert fit.ok.all() and fit.ncols.tolist() == [12, 8, 4] and fit.nrows.tolist() == list(rows)
    trend = ev.linear_trend_device(bases, fit.beta)
    for b in range(3):
        one = gadfly_amd.BatchedLogLikelihood(ks[b:b + 1], ts[b], ys[b][None, :], yerr=w["yerr"], mean=1.5)
        g1, ld1, _ = _bits(one, bases[b])
        r = bases[b].shape[1]
        assert np.array_equal(_lead(g[b:b + 1], r), g1) and ld[b] == ld1[0], b
        f1 = one.fit_linear(bases[b])
        assert np.array_equal(fit.beta[b, :r], f1.beta[0]) and fit.ll[b] == f1.ll[0]
        assert fit.ll_marginal[b] == f1.ll_marginal[0]
        assert trend[b].shape == (rows[b],)
        assert np.allclose(trend[b].cpu().numpy(), bases[b] @ fit.beta[b, :r], rtol=1e-13, atol=1e-9)
    with pytest.raises(ValueError):
        ev.linear_gram_device(bases[0])                                         # a ragged batch takes a list
    with pytest.raises(ValueError):
        ev.linear_gram_device([bases[0], bases[1], bases[2][:-1]])


def test_a_failed_problem_between_good_ones(hip):
    w = lr.walkers()
    ev = _evaluator(w)
    g, ld, _ = _bits(ev, w["A"])
    good = ev.fit_linear(w["A"])
    diag = np.full((w["B"], w["N"]), w["yerr"] ** 2)
    diag[2, 130] = -1e9
    bad = gadfly_amd.BatchedLogLikelihood(list(w["kernels"]), w["t"], w["y"], diag=diag)
    gb, ldb, infob = _bits(bad, w["A"])
    assert infob.tolist() == [0, 0, 131, 0, 0]
    assert np.all(np.isnan(gb[2])) and np.isnan(ldb[2])
    keep = [0, 1, 3, 4]
    assert np.array_equal(gb[keep], g[keep]) and np.array_equal(ldb[keep], ld[keep])
    fit = bad.fit_linear(w["A"])
    assert fit.ok.tolist() == [True, True, False, True, True] and fit.info[2] == 131
    assert np.all(np.isnan(fit.beta[2])) and np.isnan(fit.ll[2]) and np.array_equal(fit.beta[keep], good.beta[keep])
    # a rank-deficient basis (one column twice) for problem 1 alone
    dup = w["A"].copy()
    dup[:, 5] = dup[:, 1]
    fit = ev.fit_linear([w["A"], dup, w["A"], w["A"], w["A"]])
    assert fit.ok.tolist() == [True, False, True, True, True] and np.all(fit.info == 0)
    assert np.all(np.isnan(fit.cov[1])) and np.isnan(fit.ll_marginal[1])
    keep = [0, 2, 3, 4]
    assert np.array_equal(fit.beta[keep], good.beta[keep]) and np.array_equal(fit.ll[keep], good.ll[keep])


def test_errors_are_raised_before_anything_is_enqueued(hip):
    from gadfly_amd.synth import solar_like_hyperparameters
    w = lr.walkers()
    N = w["N"]
    k64 = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(32), texp=60.0)
    wide = gadfly_amd.BatchedLogLikelihood([k64], w["t"], w["y"][:1], yerr=w["yerr"])
    with pytest.raises(NotImplementedError, match="W = 64"):
        wide.linear_gram_device(w["A"])
    with pytest.raises(NotImplementedError, match="W = 64"):
        wide.fit_linear(w["A"])
    ev = _evaluator(w)
    ev._linear_events = "untouched"
    for basis in (w["A"][:-1], w["A"].T, np.zeros((N, 0)), np.zeros((N, 256)), np.zeros((2, N, 3)), [w["A"]] * 4,
                  [w["A"]] * 4 + [w["A"][:-1]], [w["A"]] * 4 + [np.zeros((N, 0))], np.zeros(N)):
        with pytest.raises(ValueError):
            ev.linear_gram_device(basis)
    with pytest.raises(ValueError):
        ev.linear_trend_device(w["A"], np.zeros((w["B"], 3)))
    assert ev._linear_events == "untouched"
    with pytest.raises(ValueError, match="sorted"):
        gadfly_amd.fit_linear_batch(list(w["kernels"]), w["t"][::-1], w["y"], w["A"], yerr=w["yerr"])
    mine = ev.fit_linear(w["A"])
    fit = gadfly_amd.fit_linear_batch(list(w["kernels"]), w["t"], w["y"], w["A"], yerr=w["yerr"])
    assert np.array_equal(fit.beta, mine.beta) and np.array_equal(fit.ll_marginal, mine.ll_marginal)
    # y means the data minus the mean ((y + 2) - 2 rounds y in its last place: 1e-13 of its scale, not the same bits)
    fit = gadfly_amd.fit_linear_batch(list(w["kernels"]), w["t"], w["y"] + 2.0, w["A"], yerr=w["yerr"], mean=2.0)
    assert np.max(np.abs(fit.beta - mine.beta) / mine.stderr) < 1e-9
    assert ev.last_linear_device_ms > 0.0
    trend = ev.linear_trend_device(w["A"], fit.beta)
    assert trend.shape == (w["B"], N) and np.allclose(trend.cpu().numpy(), fit.beta @ w["A"].T, rtol=1e-13, atol=1e-9)
