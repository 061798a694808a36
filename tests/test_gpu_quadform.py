"""GPU: gf_quadform_grad at its raw entry point (gadfly_quadform.hip).

The grid: the term structures of tests/test_gpu_predict_edges.py (W = 1 .. 63, real and complex mixed), N around the
first rows and the 64-row marks, R = 1, RB - 1, RB, RB + 1, 2 RB + 1 and 256 vectors for the RB the library reports,
B = 3, with and without weights.  Bar: |got - ref| <= 1e-10 sum_r |w_r| |x_r|^T |dK/dtheta| |x_r|, the forward-error
scale of the sum (expected: about N 2^-53 of it).  On the zero-based axis the reference is the DENSE one (closed-form
derivative matrices of oracle/dense.kernel_value); on the axis moved by 2.12e5 it is the float64 restatement of the
recurrences, which takes the same generator rows cos / sin fl(d t_n) -- the dense lag form rounds the phases
differently there and is no yardstick.  Worst values are printed."""
import functools

import numpy as np
import pytest
import torch

from tests import fused_cases as fc
from tests import grad_cases as gc
from tests import quadform_ref as qr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
BAR = 1e-10
STRUCTURES = ((1, 0), (0, 1), (2, 7), (0, 8), (1, 8), (2, 15), (0, 16), (1, 16), (0, 31), (1, 31), (3, 30))
LENGTHS = (1, 2, 3, 63, 64, 65, 129)
RMAX = 256
JD0 = 2.12e5


def _dev(x, dtype=np.float64):
    return torch.as_tensor(np.array(x, dtype=dtype, order="C")).cuda()


def vector_counts(hip):
    rb = hip.load().gf_quadform_grad_block()
    return (1, rb - 1, rb, rb + 1, 2 * rb + 1, RMAX)


def quad_call(hip, prob, X, w=None, nobs=None, t=None, which=None):
    """One gf_quadform_grad call on an edge problem (``which``: these problems only): X (B, R, N) or (R, N) shared, w
    None, (R,) or (B, R).  Outputs one problem too long, sentinel beyond; the workspace starts as NaN.  Returns
    (real (2, nb, lr), comp (4, nb, lc), diag (nb,))."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, N = prob["Jr"], prob["Jc"], prob["N"]
    sel = np.arange(prob["B"]) if which is None else np.asarray(which)
    nb = len(sel)
    lr, lc = max(Jr, 1), max(Jc, 1)
    X = np.asarray(X)
    R = X.shape[-2]
    if X.ndim == 3:
        X = X[sel]
    if w is not None and np.ndim(w) == 2:
        w = np.asarray(w)[sel]
    per = int(lib.gf_quadform_grad_work(Jr + 2 * Jc, R))
    assert per > 0
    work = torch.full((nb * per,), float("nan"), dtype=torch.float64, device="cuda")
    rd, cd = _dev(prob["real"][:, sel]), _dev(prob["comp"][:, sel])
    td, xd = _dev(prob["t"] if t is None else t), _dev(X)
    wd = None if w is None else _dev(w)
    nd = None if nobs is None else _dev(np.asarray(nobs)[sel], np.int64)
    g_real = torch.full((2 * (nb + 1) * lr,), SENTINEL, dtype=torch.float64, device="cuda")
    g_comp = torch.full((4 * (nb + 1) * lc,), SENTINEL, dtype=torch.float64, device="cuda")
    g_diag = torch.full((nb + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.gf_quadform_grad(nb, N, R, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]),
                              p(td), 0, p(nd), p(xd), 0 if X.ndim == 2 else R * N, N,
                              p(wd), 0 if w is None or np.ndim(w) == 1 else R, p(work), per,
                              p(g_real), p(g_comp), p(g_diag), None)
    hip.check(rc, "gf_quadform_grad")
    torch.cuda.synchronize()
    gr, gcx, gd = g_real.cpu().numpy(), g_comp.cpu().numpy(), g_diag.cpu().numpy()
    # the layout is (k, nb, l): everything behind it is untouched
    assert np.all(gr[2 * nb * lr:] == SENTINEL) and np.all(gcx[4 * nb * lc:] == SENTINEL) and gd[nb] == SENTINEL
    gr, gcx = gr[:2 * nb * lr].reshape(2, nb, lr), gcx[:4 * nb * lc].reshape(4, nb, lc)
    if Jr == 0:
        assert np.all(gr == SENTINEL)           # (a kind the problem has no term of is not written)
    if Jc == 0:
        assert np.all(gcx == SENTINEL)
    return gr[:, :, :Jr], gcx[:, :, :Jc], gd[:nb]


@functools.lru_cache(maxsize=None)
def edge_case(Jr, Jc, N):
    """(problem, X (3, 256, N), w (3, 256), per-vector references on the zero-based axis (dense) and on the moved one
    (restatement), per-vector scales), the references as lists over the problems."""
    prob = gc.edge_problem(Jr, Jc, N)
    rng = np.random.default_rng([17, Jr, Jc, N])
    X = rng.normal(size=(prob["B"], RMAX, N))
    w = rng.uniform(-1.0, 2.0, (prob["B"], RMAX))
    dense, scale, moved = [], [], []
    for b in range(prob["B"]):
        co = gc.coefficients(prob, b)
        q, s = qr.dense_forms(prob["t"], co, X[b])
        dense.append(q)
        scale.append(s)
        moved.append(qr.recurrences(prob["t"] + JD0, co, X[b]))
    return prob, X, w, dense, moved, scale


def _worst(prob, got, ref, scale, R, w):
    """Largest |got - ref| / scale over the entries of the three outputs of every problem (0 / 0 counts as 0, a nonzero
    error over a zero scale as inf)."""
    Jr, Jc = prob["Jr"], prob["Jc"]
    worst = 0.0
    for b in range(prob["B"]):
        wb = None if w is None else (w if np.ndim(w) == 1 else w[b])
        r = qr.stacked(qr.weighted(ref[b], R, wb), Jr, Jc)
        s = qr.stacked(qr.weighted(scale[b], R, None if wb is None else np.abs(wb)), Jr, Jc)
        for g, rr, ss in zip((got[0][:, b], got[1][:, b], got[2][b]), r, s):
            err = np.abs(np.asarray(g) - np.asarray(rr))
            ss = np.asarray(ss, dtype=np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(err == 0.0, 0.0, err / ss)
            worst = max(worst, float(np.max(rel)) if rel.size else 0.0)
    return worst


@pytest.mark.parametrize("Jr,Jc", STRUCTURES, ids=[fc.ident(s) for s in STRUCTURES])
def test_edge_grid_against_the_dense_forms_and_the_restatement(hip, Jr, Jc):
    worst = {"zero-based": 0.0, "moved": 0.0}
    for N in LENGTHS:
        prob, X, w, dense, moved, scale = edge_case(Jr, Jc, N)
        for R in vector_counts(hip):
            for wt in (None, w[:, :R], w[0, :R]):
                got = quad_call(hip, prob, X[:, :R], wt)
                worst["zero-based"] = max(worst["zero-based"], _worst(prob, got, dense, scale, R, wt))
                got = quad_call(hip, prob, X[:, :R], wt, t=prob["t"] + JD0)
                worst["moved"] = max(worst["moved"], _worst(prob, got, moved, scale, R, wt))
                if N == 1:                      # no pair of rows: exact zeros, and the diagonal's sum alone
                    assert np.all(got[0] == 0.0) and np.all(got[1] == 0.0)
                    ref = [qr.weighted(dense[b], R, None if wt is None else (wt if wt.ndim == 1 else wt[b]))["diag"]
                           for b in range(3)]
                    assert np.allclose(got[2], ref, rtol=1e-13, atol=0.0)
    print(f"quadform W={Jr + 2 * Jc}: worst error {worst['zero-based']:.2e} (dense, zero-based axis), "
          f"{worst['moved']:.2e} (restatement, axis + {JD0:g}) of the forward-error scale")
    assert worst["zero-based"] <= BAR and worst["moved"] <= BAR


@pytest.mark.parametrize("Jr,Jc", ((2, 7), (1, 31)), ids=[fc.ident(s) for s in ((2, 7), (1, 31))])
def test_bits_across_batch_position_trailing_vectors_and_runs(hip, Jr, Jc):
    N = 129
    prob, X, w, *_ = edge_case(Jr, Jc, N)
    rb = hip.load().gf_quadform_grad_block()
    R = 2 * rb + 1
    base = quad_call(hip, prob, X[:, :R], w[:, :R])
    again = quad_call(hip, prob, X[:, :R], w[:, :R])
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    # batch position: each problem alone, and the batch reversed
    for b in range(3):
        one = quad_call(hip, prob, X[:, :R], w[:, :R], which=[b])
        assert all(np.array_equal(o[..., 0, :] if o.ndim == 3 else o[0], g[..., b, :] if g.ndim == 3 else g[b])
                   for o, g in zip(one, base)), b
    rev = quad_call(hip, prob, X[:, :R], w[:, :R], which=[2, 1, 0])
    assert all(np.array_equal(np.flip(r, axis=r.ndim - 2 if r.ndim == 3 else 0), g) for r, g in zip(rev, base))
    # trailing vectors: zeros, or anything at weight zero, behind a problem's own -- in the same block, in a further
    # one, and up to the most the entry point takes
    for more in (1, rb - 1, rb, RMAX - R):
        Xz = np.concatenate([X[:, :R], np.zeros((3, more, N))], axis=1)
        wz = np.concatenate([w[:, :R], w[:, R:R + more]], axis=1)
        assert all(np.array_equal(a, b) for a, b in zip(quad_call(hip, prob, Xz, wz), base)), more
        w0 = np.concatenate([w[:, :R], np.zeros((3, more))], axis=1)
        assert all(np.array_equal(a, b) for a, b in zip(quad_call(hip, prob, X[:, :R + more], w0), base)), more
    # the leading vectors without weights: as many ones
    plain = quad_call(hip, prob, X[:, :R])
    ones = quad_call(hip, prob, X[:, :R], np.ones(R))
    assert all(np.array_equal(a, b) for a, b in zip(plain, ones))
    # one set of vectors shared by the three problems
    shared = quad_call(hip, prob, X[1, :R], w[1, :R])
    own = quad_call(hip, prob, X[:, :R], w[:, :R], which=[1])
    assert all(np.array_equal(s[..., 1, :] if s.ndim == 3 else s[1], o[..., 0, :] if o.ndim == 3 else o[0])
               for s, o in zip(shared, own))


@pytest.mark.parametrize("Jr,Jc", ((0, 8), (3, 30)), ids=[fc.ident(s) for s in ((0, 8), (3, 30))])
def test_row_counts_end_a_problem_early(hip, Jr, Jc):
    """nobs = (129, 64, 1): a problem stopped early has the bits of the call on its first rows alone, and its later
    rows (NaN here) are never read."""
    N, R = 129, 9
    prob, X, w, *_ = edge_case(Jr, Jc, N)
    nobs = np.array([N, 64, 1])
    Xc = X[:, :R].copy()
    for b, n in enumerate(nobs):
        Xc[b, :, n:] = np.nan
    got = quad_call(hip, prob, Xc, w[:, :R], nobs=nobs)
    for b, n in enumerate(nobs):
        short = dict(prob, N=int(n), t=prob["t"][:n])
        one = quad_call(hip, short, np.ascontiguousarray(X[:, :R, :n]), w[:, :R], which=[b])
        assert all(np.array_equal(o[..., 0, :] if o.ndim == 3 else o[0], g[..., b, :] if g.ndim == 3 else g[b])
                   for o, g in zip(one, got)), (b, n)
    assert np.all(np.isfinite(got[2]))
