"""No device: tests/lin_ref.py against dense algebra in 80 bits, and the conditioning of every synthetic case the device
tests run (tests/lin_cases.py)."""
import numpy as np
import pytest

from tests import lft_ref
from tests import lin_cases as C
from tests import lin_ref as R

EPS80 = float(np.finfo(np.longdouble).eps)


def test_longdouble_is_80_bit():
    assert np.finfo(np.longdouble).nmant == 63


def _small(W, N=61, key=11):
    return R.synthetic(W, N, B=2, block=16, resets=(5, 6, 31, 47, 48), key=key), R.rhs(W, N, 3, B=2, key=key)


@pytest.mark.parametrize("W", [1, 4, 13])
def test_sweeps_equal_the_dense_triangular_algebra(W):
    """lower = L^-1 y, upper = L^-T y, matmul = L y with L[n, m] = u~_n^T (prod E) w~_m built entry by entry; the
    input scalings y / d and y sqrt(d)."""
    rows, Y = _small(W)
    for b in range(2):
        Lm = R.dense_lower(rows, b)
        d = rows["d"][b].astype(R.LD)[:, None]
        for scale in (0, 1):
            for mode, want in ((R.LOWER, lambda y: lft_ref.gauss_jordan(Lm, y)[0]),
                               (R.UPPER, lambda y: lft_ref.gauss_jordan(Lm.T, y)[0]),
                               (R.MATMUL, lambda y: Lm @ y)):
                Z = R.sweep(mode, rows, R.scaled_input(mode, rows, Y, scale))[0][b]
                y = Y[b].astype(R.LD)
                y = y if not scale else (y * np.sqrt(d) if mode == R.MATMUL else y / d)
                assert R.scaled_error(Z, want(y)) < 64 * 61 * EPS80, (W, b, mode, scale)


@pytest.mark.parametrize("W", [1, 4, 13, 63])
@pytest.mark.parametrize("L", [1, 7, 16, 64])
def test_chunk_transitions_reproduce_the_sequential_states(W, L):
    """F_{c+1} = Fbar_c + Phi_c F_c (upper: the transpose, descending) gives the states of the unchunked recurrence;
    matmul the same with D_c; a final pass from those states gives the unchunked Z."""
    rows, Y = _small(W)
    Phi = R.transitions(rows, L)[0]
    for mode in C.MODES:
        Z, starts = R.sequential(mode, rows, Y, L)
        loc = R.local_states(mode, rows, Y, L)
        got = R.diag_scan(R.chunk_decay(rows, L), loc) if mode == R.MATMUL else R.scan(mode, Phi, loc)
        assert R.scaled_error(got, starts) < 64 * 61 * EPS80, (mode, W, L)
        for c, (a, e) in enumerate(R.bounds(Y.shape[1], L)):
            Zc = R.sweep(mode, rows, Y, None, a, e, F0=starts[c])[0]
            assert R.scaled_error(Zc, Z[:, a:e]) < 64 * 61 * EPS80, (mode, W, L, c)


def test_transition_sums_and_rows_without_a_pivot():
    """G = sum h h^T / d and m = sum h z / d against the rows h = Phi_n^T u~_n formed from the dense prefix products;
    a row with d <= 0 adds nothing to G, m and the pending update."""
    rows, _ = _small(5, N=20)
    d = rows["d"].copy()
    d[:, [3, 9]] = (0.0, -1.5)
    z = np.random.default_rng(3).normal(size=d.shape)
    Phi, G, m = R.transitions(rows, 20, dbar=d, zbar=z)
    c, U, Wt = rows["c"].astype(R.LD), rows["Ut"][:, :, :5].astype(R.LD), rows["Wt"][:, :, :5].astype(R.LD)
    r = Wt * rows["d"].astype(R.LD)[:, :, None]
    for b in range(2):
        P, Gs, ms = np.eye(5, dtype=R.LD), 0, 0
        for n in range(20):
            if rows["de"][b, n] >= 0:
                P = np.diag(np.exp(-c[b] * R.LD(rows["de"][b, n]))) @ P
            h = P.T @ U[b, n]
            if d[b, n] > 0:
                Gs, ms = Gs + np.outer(h, h) / R.LD(d[b, n]), ms + h * R.LD(z[b, n]) / R.LD(d[b, n])
                P = (np.eye(5, dtype=R.LD) - np.outer(r[b, n] / R.LD(d[b, n]), U[b, n])) @ P
        assert R.scaled_error(Phi[0, b], P) < 1e3 * EPS80
        assert R.scaled_error(G[0, b], Gs) < 1e3 * EPS80 and R.scaled_error(m[0, b], ms) < 1e3 * EPS80


@pytest.mark.parametrize("seg_len", [1, 2, 5, 8, 9, 12])
def test_segment_composition_agrees_with_chunk_by_chunk_application(seg_len):
    rows, Y = _small(13, N=9 * 7)
    Phi = R.transitions(rows, 7)[0]
    Psi = R.segment_transitions(Phi, seg_len)
    v = Y[:, :13, :].astype(R.LD)
    for s, b0 in enumerate(range(0, 9, seg_len)):
        w = v
        for c in range(b0, min(b0 + seg_len, 9)):
            w = Phi[c] @ w
        assert R.scaled_error(Psi[s] @ v, w) < 1e3 * EPS80


def test_chunk_decay_is_the_product_of_the_row_decays():
    for W, L in ((1, 7), (13, 16), (63, 64)):
        rows, _ = _small(W)
        assert R.scaled_error(R.chunk_decay(rows, L), R.chunk_decay_product(rows, L)) < 64 * EPS80
    assert np.any(_small(13)[0]["de"] == 0.0)


def test_float64_restatement_is_the_same_code():
    rows, Y = _small(13)
    for mode in C.MODES:
        Z = R.sweep(mode, rows, Y)[0]
        Z64 = R.sweep(mode, rows, Y, dtype=np.float64)[0]
        assert Z64.dtype == np.float64 and 0 < R.scaled_error(Z64, Z) < 1e-13


def test_reset_rows_cover_every_offset():
    de = C.rows_of(C.reset_cases(7)[0])["de"][0]
    at = np.flatnonzero(de >= 0)
    assert set(at % 16) == set(range(16)) and {100, 101, 102, 63, 64, 127, 128} <= set(at)
    assert np.any(de[at] == 0.0) and not np.any(C.rows_of(C.reset_cases(7)[1])["de"] >= 0)


@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_conditioning_of_every_device_case(cls):
    """A condition, not a measurement: max |Z_ref| <= 100 max |Y| for every sweep and max |Phi_c| <= 10 for every
    chunk of every synthetic case the device tests run, by the float64 restatement (which the 80-bit reference meets
    to 1e-10 on a sample, below)."""
    for cs, Rmax in C.linear_cases():
        if cs[0] not in C.CLASSES[cls]:
            continue
        for mode in C.MODES:
            ref = C.sweep_ref(cs, mode, Rmax, np.float64)
            assert np.max(np.abs(ref["Z"])) <= 100 * np.max(np.abs(ref["Y"])), (cs, mode)
        assert np.max(np.abs(C.map_ref(cs, np.float64)[0])) <= 10, cs


def test_conditioning_sample_in_80_bits():
    for W in (1, 13, 63):
        cs = C.width_case(W)
        for mode in C.MODES:
            a, b = C.sweep_ref(cs, mode, 16, np.float64), C.sweep_ref(cs, mode, 16)
            assert R.scaled_error(a["Z"], b["Z"]) < 1e-10
            assert np.max(np.abs(b["Z"])) <= 100 * np.max(np.abs(b["Y"]))
        assert np.max(np.abs(C.map_ref(cs)[0])) <= 10
