"""Host side of the group phase of the steady tail's finishing launch (k_steady_finish), restated in
numpy.  In front of every 16 blocks the kernel forms U = H [y_k .. y_k+15], a (64 x 64) (64 x 16) product, on the matrix
pipe: H in 16 x 16 tiles, lower block triangle only (10 tiles), each tile in four slices of 4 columns
(v_mfma_f64_16x16x4_f64), rows of y clamped to the series' last row; every block then takes its column of U.

  (1) the tiled product against the dense one (a dot product's rounding bound) and, carried through the folded block
      form in place of its u = H y, against the row form: the bar is tests/test_steady_fold_host.py's own;
  (2) on the longer series of tests/steady_group_cases.py the oracle's exact rows still stand for the frozen filter:
      what the reference contributes to tests/test_gpu_steady_group.py's bar on sum z^2 / d, at every tail it runs."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, B_FIN, SW, frozen_state, row_form
from tests.steady_group_cases import GROUP, J_GROUP, LONGEST_G, TAILS_G, case
from tests.test_gpu_steady import _fast_terms
from tests.test_steady_finish_host import _advance_split
from tests.test_steady_fold_host import FACTOR, FLOOR, L, _block_form, _row_form, _tables
from tests.test_steady_tail_host import RTOL_Z, _frozen, _problem

TILE, SLICE = 16, 4
MARGIN = 1e-2           # the reference's share of the GPU test's bar: at least two orders of magnitude under it


def _tiled_product(H, Y):
    """U = H Y as the group phase sums it: per 16-row tile I of U one accumulator, over the tiles Jt <= I of H's block
    row and their four 4-column slices in turn, a slice's four products one after the other (fused)."""
    U = np.zeros((L, Y.shape[1]))
    for I in range(L // TILE):
        acc = np.zeros((TILE, Y.shape[1]), dtype=np.longdouble)
        for Jt in range(I + 1):
            for q in range(TILE // SLICE):
                for k in range(SLICE):
                    c = TILE * Jt + SLICE * q + k
                    # an FMA: the product exact, one rounding to float64 per step
                    acc = (acc + np.outer(H[TILE * I:TILE * (I + 1), c].astype(np.longdouble),
                                          Y[c].astype(np.longdouble))).astype(np.float64).astype(np.longdouble)
        U[TILE * I:TILE * (I + 1)] = acc.astype(np.float64)
    return U


def _group_y(y, g0):
    """Y of the group whose first block starts at row g0: column c holds the rows g0 + 64 c .. + 63, clamped to the
    series' last row as the kernel's loads are."""
    idx = g0 + L * np.arange(GROUP)[None, :] + np.arange(L)[:, None]
    return y[np.minimum(idx, len(y) - 1)]


def _group_form(fz, y):
    """tests/test_steady_fold_host.py::_block_form(fold=True) with u from the group phase."""
    lam, G, s = fz["lam"], fz["G"], fz["s"].copy()
    H, _, Q = _tables(fz)
    first, N = fz["sw"] + 1, len(y)
    lanes = np.zeros(L)
    for k, b0 in enumerate(range(first, N, L)):
        if k % GROUP == 0:
            U = _tiled_product(H, _group_y(y, b0))
        lim = min(L, N - b0)
        zb = U[:, k % GROUP] + Q @ np.concatenate([s.real, s.imag])
        lanes[:lim] += zb[:lim] ** 2
        s = _advance_split(lam, G, s, zb[:lim])
    return float(np.sum(lanes)), s


@pytest.fixture(scope="module", params=[1, 30, 31])
def fast(request):
    J = request.param
    N = 8192
    coeffs, t, diag, y, _ = _problem(_fast_terms(J), N)
    fz = _frozen(coeffs, t, diag, y)
    assert 1024 < fz["sw"] < N - 1 - LONGEST_G, fz["sw"]
    return J, fz, y


def test_tiles_above_the_diagonal_are_zero_and_the_rest_is_the_dense_product(fast):
    """The 6 tiles the phase skips hold zeros, and the 10 it runs give H Y to a dot product's bound: 64 roundings of
    2^-53 on sum |h| |y|.  Columns do not mix: a column of clamped rows leaves the others' bits alone."""
    J, fz, y = fast
    H, _, _ = _tables(fz)
    for I in range(L // TILE):
        for Jt in range(I + 1, L // TILE):
            assert not np.any(H[TILE * I:TILE * (I + 1), TILE * Jt:TILE * (Jt + 1)])
    first = fz["sw"] + 1
    Y = _group_y(y[:first + L * GROUP], first)
    U = _tiled_product(H, Y)
    bound = L * 2.0 ** -53 * (np.abs(H) @ np.abs(Y))
    err = np.abs(U - H @ Y)
    print(f"J = {J}: tiled against dense, worst error / bound {np.max(err / bound):.2f}")
    assert np.all(err <= bound)
    Yc = _group_y(y[:first + L + 1], first)                 # a block and a row: 14 columns of clamped rows
    Uc = _tiled_product(H, Yc)
    assert np.array_equal(Uc[:, 0], U[:, 0]) and Uc[0, 1] == U[0, 1]


@pytest.mark.parametrize("tail", [1, 64, 65, 1024, 1025, 1089, 2048, LONGEST_G])
def test_group_form_against_the_row_form(fast, tail):
    """The folded block with its u from the group phase, against the row form in what the launch keeps (the sum of z^2
    as the lanes form it, the state behind the last row): at most FACTOR times the present block form's error or FLOOR,
    the bar of tests/test_steady_fold_host.py."""
    J, fz, y = fast
    y = y[:fz["sw"] + 1 + tail]
    zr, sr = _row_form(fz, y)
    q_row = float(np.sum(np.bincount(np.arange(len(zr)) % L, weights=zr * zr, minlength=L)))
    smax = np.max(np.abs(sr))
    qb, sb = _block_form(fz, y, False)
    qg, sg = _group_form(fz, y)
    eb = (abs(qb - q_row) / q_row, np.max(np.abs(sb - sr)) / smax)
    eg = (abs(qg - q_row) / q_row, np.max(np.abs(sg - sr)) / smax)
    print(f"J = {J}, tail of {tail} rows: sum z^2 block {eb[0]:.2e} group {eg[0]:.2e}; state block {eb[1]:.2e} "
          f"group {eg[1]:.2e}")
    for i, quantity in enumerate(("sum z^2", "state")):
        bound = max(FACTOR * eb[i], FLOOR)
        assert eg[i] <= bound, (J, tail, quantity, eg[i], bound)


@pytest.mark.parametrize("J", J_GROUP)
def test_exact_rows_are_a_reference_on_the_long_series(J):
    """tests/test_steady_instances_host.py on the long series: the frozen row form in longdouble from the oracle's state
    at ANCHOR against the oracle's exact rows, in the quantity the GPU test bars -- sum z^2 / d_inf of a tail against
    sum z_n^2 / d_n, bar 2 RTOL_Z max|z| sum |z_n| / d_inf + RTOL_Z sum z_n^2 / d_n -- at every tail it runs.  The
    reference's share of that bar stays below MARGIN (measured: 8.8e-5 at worst, at J = 1; no tail had to be shortened)."""
    c = case(J)
    ks = np.array(TAILS_G)
    worst, worst_z = 0.0, 0.0
    for b in range(B_FIN):
        rows = c.rows[b]
        zl = row_form(frozen_state(rows, c.t), c.y[SW:])
        assert len(zl) == LONGEST_G
        worst_z = max(worst_z, float(np.max(np.abs(zl - rows.z[SW:])) / c.zmax[b]))
        share = (np.cumsum(zl * zl)[ks - 1] / np.longdouble(rows.dinf)).astype(np.float64)
        s = c.sums[b]
        bar = 2.0 * RTOL_Z * c.zmax[b] * s.zabs[ks - 1] / rows.dinf + RTOL_Z * s.z2d[ks - 1]
        ratio = np.abs(share - s.z2d[ks - 1]) / bar
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= MARGIN, (J, b, ratio.tolist())
    print(f"J = {J}: switch at {ANCHOR}; tails up to {LONGEST_G} rows: the reference's share of the bar {worst:.1e}, "
          f"tail z {worst_z:.1e} max|z|")
