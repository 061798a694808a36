"""CPU: the two references of gf_quadform_grad against each other and against the oracle (tests/quadform_ref.py), and
every argument check of the entry point by exact status and exact gf_last_error() text.  Every pointer is NULL: the
null-pointer check is the last one, so no case can reach a launch."""
import numpy as np
import pytest

from gadfly_amd import _lib
from oracle import dense
from tests import grad_cases as gc
from tests import quadform_ref as qr

Z = None
BAR = 1e-10         # of sum_r |w_r| |x_r|^T |dK/dtheta| |x_r|, the forward-error scale of the sum


@pytest.mark.parametrize("Jr,Jc", [(2, 3), (1, 0), (0, 1)])
def test_closed_form_derivative_matrices_are_those_of_the_oracle_kernel(Jr, Jc):
    """Central differences of oracle/dense.kernel_value in every coefficient, step 1e-6 relative: truncation and
    rounding leave about 1e-9 of the largest entry."""
    prob = gc.edge_problem(Jr, Jc, 17)
    t, co = prob["t"], gc.coefficients(prob, 1)
    D = qr.derivative_matrices(t, co)
    lag = t[:, None] - t[None, :]
    for i, name in enumerate(qr.NAMES):
        for j in range(len(co[i])):
            h = 1e-6 * abs(co[i][j])
            up, dn = [np.array(c) for c in co], [np.array(c) for c in co]
            up[i][j] += h
            dn[i][j] -= h
            fd = (dense.kernel_value(up, lag) - dense.kernel_value(dn, lag)) / (2 * h)
            fd[np.diag_indices_from(fd)] = 0.0
            assert np.max(np.abs(fd - D[name][j])) <= 1e-7 * max(1.0, np.max(np.abs(D[name][j]))), (name, j)


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (0, 1), (2, 7), (3, 30)])
@pytest.mark.parametrize("N", [1, 2, 3, 65])
def test_recurrences_match_the_dense_forms_on_a_zero_based_axis(Jr, Jc, N):
    prob = gc.edge_problem(Jr, Jc, N)
    X = np.random.default_rng([5, Jr, Jc, N]).normal(size=(9, N))
    for b in range(prob["B"]):
        co = gc.coefficients(prob, b)
        q, scale = qr.dense_forms(prob["t"], co, X)
        r = qr.recurrences(prob["t"], co, X)
        for k in q:
            assert np.all(np.abs(r[k] - q[k]) <= BAR * scale[k]), (k, b)
        if N == 1:
            assert all(np.all(r[k] == 0.0) for k in qr.NAMES)
            assert np.array_equal(r["diag"], X[:, 0] ** 2)


def test_weighted_sums_and_layout():
    prob = gc.edge_problem(2, 3, 10)
    X = np.random.default_rng(3).normal(size=(5, 10))
    q = qr.recurrences(prob["t"], gc.coefficients(prob, 0), X)
    w = np.array([0.5, -1.0, 2.0, 0.0, 3.0])
    g = qr.weighted(q, 4, w)
    assert np.allclose(g["cc"], sum(w[r] * q["cc"][r] for r in range(4)))
    real, comp, dg = qr.stacked(g, 2, 3)
    assert real.shape == (2, 2) and comp.shape == (4, 3) and dg == pytest.approx(float(w[:4] @ q["diag"][:4]))


# ---- the entry point's argument checks -------------------------------------------------------------------------------

def quad(B=1, N=16, R=3, Jr=0, Jc=2, t_bs=0, x_bs=0, x_rs=None, w_bs=0, work_bs=1 << 40):
    x_rs = N if x_rs is None else x_rs
    return ((B, N, R, Jr, Jc) + (Z,) * 6 + (Z, t_bs, Z) + (Z, x_bs, x_rs, Z, w_bs) + (Z, work_bs) + (Z,) * 3 + (Z,))


SHAPE = "gf_quadform_grad: bad shape (B={B}, N={N}, R={R} of 1..256, Jr={Jr}, Jc={Jc})"
STRIDE = "gf_quadform_grad: bad stride (t_bs={t}, x_bs={xb}, x_rs={xr}, w_bs={w} for R=3, N=16)"
CASES = [
    (dict(B=0), -1, SHAPE.format(B=0, N=16, R=3, Jr=0, Jc=2)),
    (dict(N=0), -1, SHAPE.format(B=1, N=0, R=3, Jr=0, Jc=2)),
    (dict(R=0), -1, SHAPE.format(B=1, N=16, R=0, Jr=0, Jc=2)),
    (dict(R=257), -1, SHAPE.format(B=1, N=16, R=257, Jr=0, Jc=2)),
    (dict(Jc=-1, Jr=3), -1, SHAPE.format(B=1, N=16, R=3, Jr=3, Jc=-1)),
    (dict(Jr=0, Jc=0), -1, SHAPE.format(B=1, N=16, R=3, Jr=0, Jc=0)),
    (dict(Jr=0, Jc=32), -3, "gf_quadform_grad: width W=64 exceeds the one-wave limit 63"),
    (dict(Jr=2, Jc=31), -3, "gf_quadform_grad: width W=64 exceeds the one-wave limit 63"),
    (dict(work_bs=319), -1, "gf_quadform_grad: work_bs=319 < gf_quadform_grad_work(W, R)=320"),
    (dict(R=9, work_bs=320), -1, "gf_quadform_grad: work_bs=320 < gf_quadform_grad_work(W, R)=640"),
    (dict(t_bs=-1), -1, STRIDE.format(t=-1, xb=0, xr=16, w=0)),
    (dict(x_rs=15), -1, STRIDE.format(t=0, xb=0, xr=15, w=0)),
    (dict(x_bs=-48), -1, STRIDE.format(t=0, xb=-48, xr=16, w=0)),
    (dict(x_bs=47), -1, STRIDE.format(t=0, xb=47, xr=16, w=0)),
    (dict(x_bs=55, x_rs=20), -1, STRIDE.format(t=0, xb=55, xr=20, w=0)),
    (dict(w_bs=-1), -1, STRIDE.format(t=0, xb=0, xr=16, w=-1)),
    (dict(), -1, "gf_quadform_grad: null pointer"),
    (dict(R=256, x_bs=256, N=1, w_bs=2), -1, "gf_quadform_grad: null pointer"),   # (w NULL: w_bs is not looked at)
]


@pytest.mark.parametrize("kw,status,text", CASES, ids=[f"{i}-{'-'.join(c[0]) or 'null'}" for i, c in enumerate(CASES)])
def test_quadform_grad_refuses_before_any_launch(kw, status, text):
    lib = _lib.load()
    assert lib.gf_quadform_grad(*quad(**kw)) == status
    assert _lib.last_error() == text


def test_weight_stride_is_checked_where_there_are_weights():
    """A non-null w with a batch stride shorter than R: refused (the pointer is never read: the launch is not reached)."""
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_double * 4)()
    args = list(quad(w_bs=2))
    args[17] = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gf_quadform_grad(*args) == -1
    assert _lib.last_error() == STRIDE.format(t=0, xb=0, xr=16, w=2)


def test_quadform_grad_work_sizes_and_block():
    """Five sums per lane for every block of gf_quadform_grad_block() vectors; 0 for what gf_quadform_grad refuses."""
    lib = _lib.load()
    rb = lib.gf_quadform_grad_block()
    assert rb == 8
    for R in (1, rb - 1, rb, rb + 1, 2 * rb + 1, 256):
        for W in (1, 16, 17, 63):
            assert lib.gf_quadform_grad_work(W, R) == -(-R // rb) * 5 * 64
    for W, R in ((0, 3), (64, 3), (4, 0), (4, 257), (-1, 3)):
        assert lib.gf_quadform_grad_work(W, R) == 0
