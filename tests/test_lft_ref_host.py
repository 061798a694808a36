"""CPU: pins tests/lft_ref.py, the 80-bit reference of tests/test_gpu_chunk_combine.py and
tests/test_gpu_chunk_corrections.py, and the case generators those tests use -- without the device.

* the 80-bit map algebra against the SEQUENTIAL 80-bit recurrence over the whole series (independent of the algebra),
  compose against apply (associativity: the property a tree needs), corrections against the recurrence's own sums;
* the float64 oracle/lft.py against the 80-bit reference on the very cases the device tests judge with it, with the
  conditioning of those cases asserted: a generator change that makes them ill-posed fails here, not on the device;
* the planted failing cases report what their docstrings claim.
"""
import numpy as np
import pytest

from oracle import lft
from tests import grad_cases as gc
from tests import lft_ref as R

LD = R.LD
EPS80, EPS64 = float(np.finfo(LD).eps), float(np.finfo(np.float64).eps)
#: the reference's own bar: 64 eps80 kappa -- the backward-error scale W eps kappa of a pivoted W x W elimination at the
#: widest W, in the 80-bit format; a 32nd of the smallest bar a float64 result is ever held to with it
REF_BAR = 64 * EPS80

SYNTH_WIDTHS = (1, 2, 17, 33, 48, 63)
REAL_STRUCTURES = ((1, 0), (0, 1), (2, 7), (0, 16), (1, 16), (1, 24), (3, 30))
REAL_SHAPES = ((197, 16), (300, 37), (64, 8), (100, 1))


def test_longdouble_is_wider_than_double():
    assert EPS80 <= 2.0 ** -63, "np.longdouble is no extended format here: the reference would judge nothing"


def test_gauss_jordan_against_numpy():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 40):
        A, B = rng.normal(size=(n, n)), rng.normal(size=(n, 3))
        Z, ld, sg = R.gauss_jordan(A, B)
        s64, l64 = np.linalg.slogdet(A)
        kappa = np.linalg.cond(A)
        assert sg == int(s64) and abs(float(ld) - l64) <= 1e-13 * kappa
        assert R.scaled_error(np.linalg.solve(A, B), Z) <= n * EPS64 * kappa
        assert R.scaled_error(A.astype(LD) @ Z, B) <= n * EPS80 * kappa           # the residual, in 80 bits
    with pytest.raises(np.linalg.LinAlgError):
        R.gauss_jordan(np.zeros((2, 2)), np.ones(2))


def test_slot_layout():
    """Element (i, j) at j * 64 + i, zero beyond W; vectors in 64-double slots."""
    M = np.arange(12.0).reshape(3, 4)[:, :3] + 1.0          # non-symmetric
    s = R.pack_matrices([M, 2 * M])
    assert s.shape == (2, 4096) and s[0, 2 * 64 + 1] == M[1, 2] and s[1, 0 * 64 + 2] == 2 * M[2, 0]
    assert np.count_nonzero(s[0]) == 9
    lead, rest = R.unpack_matrices(s, 3)
    assert np.array_equal(lead[0], M) and np.array_equal(lead[1], 2 * M) and not rest.any()
    v = R.pack_vectors([np.array([1.0, 2.0, 3.0])])
    assert v.shape == (1, 64) and np.array_equal(v[0, :3], [1.0, 2.0, 3.0]) and not v[0, 3:].any()


@pytest.mark.parametrize("Jr,Jc", REAL_STRUCTURES)
def test_reference_states_equal_the_sequential_recurrence(Jr, Jc):
    """80-bit start_states on the nominal-pass maps against the 80-bit sequential recurrence over the whole series,
    scaled by the largest entry: within 64 eps80 kappa (measured: 9.1e-18 at the worst, (3, 30) in chunks of one
    row); and the corrections against the recurrence's own sums, sum log D and sum z^2 / D from the true start minus
    the same from the zero start, to 1e-14 (those are differences of sums twenty times their size)."""
    for N, L in REAL_SHAPES:
        r = R.real_maps(Jr, Jc, N, L)
        s = R.start_states(r["maps"])
        kappa = R.chain_condition(r["maps"], r["starts"])
        for k in (0, 1):
            ref = np.array([x[k] for x in r["starts"]])
            assert R.scaled_error(np.array([x[k] for x in s]), ref, 0.0) <= REF_BAR * kappa, (N, L, k)
        for M, (X, Y), dl, dq in zip(r["maps"], r["starts"], r["dld"], r["dqd"]):
            ld, q, sg = R.corrections(X, Y, M[1], M[4])
            assert sg == 1
            assert abs(ld - dl) <= 1e-14 * max(1, abs(dl)) and abs(q - dq) <= 1e-14 * max(1, abs(dq)), (N, L)


def _apply_all(maps, X, Y):
    for M in maps:
        X, Y = R.apply(M, X, Y)
    return X, Y


@pytest.mark.parametrize("case", ["synthetic-17", "synthetic-48", "real-2-7", "real-1-24"])
def test_compose_is_associative_against_apply(case):
    """Four maps a, b, c, d and a non-zero state s: ((a b) c) d, a (b (c d)) and (a b) (c d) applied to s all equal
    d(c(b(a(s)))) -- the identity a scan over the maps rests on, in whatever order it pairs them."""
    kind, *w = case.split("-")
    if kind == "synthetic":
        maps = R.synthetic(int(w[0]), 6)
        kappa = 1e3
    else:
        maps = R.real_maps(int(w[0]), int(w[1]), 197, 16)["maps"]
        kappa = 1e2
    (X, Y), (a, b, c, d) = R.start_states(maps[:2])[1], maps[2:6]
    ref = _apply_all((a, b, c, d), X, Y)
    forms = (R.compose(R.compose(R.compose(a, b), c), d), R.compose(a, R.compose(b, R.compose(c, d))),
             R.compose(R.compose(a, b), R.compose(c, d)))
    for i, M in enumerate(forms):
        got = R.apply(M, X, Y)
        for k in (0, 1):
            assert R.scaled_error(got[k], ref[k], 0.0) <= REF_BAR * kappa, (case, i, k)
    # the zero state through a composite gives the composite's own nominal end state
    W = a[0].shape[0]
    got = R.apply(forms[2], np.zeros((W, W)), np.zeros(W))
    ref0 = _apply_all((a, b, c, d), np.zeros((W, W)), np.zeros(W))
    assert R.scaled_error(got[0], ref0[0], 0.0) <= REF_BAR * kappa
    assert R.scaled_error(forms[2][2], ref0[0], 0.0) <= REF_BAR * kappa


@pytest.mark.parametrize("W", SYNTH_WIDTHS)
def test_float64_oracle_on_the_synthetic_family(W):
    """lft.random_maps(default_rng(W), 37, W) at its default rank 6 and at the device tests' rank min(6, W): float64
    oracle/lft.py within 1e-13 of the 80-bit states scaled by max(1, |X|) (measured: 1.4e-15 in X, 8.7e-15 in Y, at
    W = 63; eps64 times the bound on the condition is 2.2e-13), cond(I - X G) < 1e3 (measured 6.7e2), |X| < 10
    (measured 4.6)."""
    for maps in (lft.random_maps(np.random.default_rng(W), 37, W), R.synthetic(W, 37)):
        s80, s64 = R.start_states(maps), lft.start_states(maps)
        assert R.chain_condition(maps, s80) < 1e3
        assert max(float(np.max(np.abs(X))) for X, _ in s80) < 10.0
        for k in (0, 1):
            assert max(R.scaled_error(a[k], b[k]) for a, b in zip(s64, s80)) <= 1e-13, (W, k)


@pytest.mark.parametrize("Jr,Jc", REAL_STRUCTURES)
def test_float64_oracle_on_the_real_family(Jr, Jc):
    """The plain-coordinate maps of the edge problems: float64 oracle/lft.py on the float64 maps within 1e-12 of the
    float64 sequential states, scaled by the largest entry (measured: 1.2e-14 in X, 5.7e-14 in Y; eps64 times the
    bound on the condition, 2.2e-13, over a chain of up to 100 chunks); the largest eigenvalue of X G < 0.995
    (measured 0.982: I - X G keeps 0.018) and cond(I - X G) < 1e3 (measured 78)."""
    for N, L in REAL_SHAPES:
        r = R.real_maps(Jr, Jc, N, L, 0, np.float64)
        s = lft.start_states(r["maps"])
        for k in (0, 1):
            ref = np.array([x[k] for x in r["starts"]])
            assert R.scaled_error(np.array([x[k] for x in s]), ref, 0.0) <= 1e-12, (N, L, k)
        assert R.chain_condition(r["maps"], r["starts"]) < 1e3
        top = max(float(np.max(np.linalg.eigvals(X @ M[1]).real)) for M, (X, _) in zip(r["maps"], r["starts"]))
        assert top < 0.995, (N, L, top)


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (0, 31)])
@pytest.mark.parametrize("nrows", [1, 2])
def test_planted_failures_are_what_they_claim(Jr, Jc, nrows):
    """N = 197 in chunks of 16 rows, problem 1: the nominal pass of every chunk is healthy (asserted by the
    generator); the true recurrence has exactly ``nrows`` non-positive pivots, all in the named chunk, the first at
    the first planted row; one row: the chunk's first, and det(I - X G) < 0; two rows: det(I - X G) > 0 -- a parity
    check passes it -- with two negative eigenvalues; log |det| and the quadratic form still equal the recurrence's
    own sums (on log |D|), so the case is a consistent indefinite problem, not a broken one."""
    f = R.planted_failure(Jr, Jc, nrows)
    ch = f["chunk"]
    assert ch == (3 if nrows == 1 else 6) and len(f["rows"]) == nrows
    assert all(ch * 16 <= n < ch * 16 + 16 for n in f["rows"])
    if nrows == 1:
        assert f["rows"] == [48]
    assert [len(b) for b in f["bad"]] == [nrows if c == ch else 0 for c in range(13)]
    assert f["bad"][ch][0] == f["rows"][0] + 1
    healthy = R.real_maps(Jr, Jc, 197, 16, 1)
    orig = gc.edge_problem(Jr, Jc, 197)["diag"][1]
    assert np.all(f["diag"][f["rows"]] < orig[f["rows"]]) and np.sum(f["diag"] != orig) == nrows
    for c in range(ch + 1):                     # up to the failing chunk the start states are the healthy problem's
        assert np.array_equal(f["starts"][c][0], healthy["starts"][c][0])
    M, (X, Y) = f["maps"][ch], f["starts"][ch]
    ld, q, sg = R.corrections(X, Y, M[1], M[4])
    assert sg == (-1 if nrows == 1 else 1)
    ev = np.linalg.eigvals(np.eye(f["W"]) - np.asarray(X @ M[1], dtype=np.float64)).real
    assert np.sum(ev < 0) == nrows and np.min(np.abs(ev)) > 1e-3
    assert abs(ld - f["dld"][ch]) <= 1e-12 * max(1, abs(f["dld"][ch]))
    assert abs(q - f["dqd"][ch]) <= 1e-12 * max(1, abs(f["dqd"][ch]))
