"""CPU: the numpy restatement of the non-uniform-FFT Lomb-Scargle route (tests/ls_fast_ref.py: wrap, spread,
rfft, quadrature deconvolution, the shared final formula) against the exact oracle tests/ls_ref.py at the
direct route's own bar, rtol = 1e-8 and atol = 1e-10 max(power); the host side of method="nufft" (grid sizes,
the layout and grouping of series, the refused method) -- no GPU needed.  The worst errors are printed
(pytest -s) for DESIGN.md 3.6.1."""
import numpy as np
import pytest

from tests import ls_fast_ref, ls_ref

JD_SHIFT = 2454833.0 * 0.0864          # BKJD 0 in 1/uHz (jd * day)
RTOL, ATOL = 1e-8, 1e-10


def _gapped(n, seed, cadence=60e-6, red=True):
    """n points of a jittered axis with one long and many single-point gaps removed (fewer than n remain)."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * cadence
    keep = np.ones(n, bool)
    keep[n // 4: n // 4 + n // 10] = False
    keep[rng.integers(0, n, n // 20)] = False
    t = t[keep]
    y = 50 * rng.normal(size=len(t))
    if red:
        y = y + 300 * np.sin(2 * np.pi * 3000.0 * t) + np.cumsum(rng.normal(size=len(t)))
    return t, y


def _with_n_points(n, seed, red=True):
    t, y = _gapped(int(n * 1.2) + 10, seed, red=red)
    return t[:n], y[:n]


def _sparse(seed=7, cadences=20000, kept=0.3, d=60e-6):
    """30 % of the cadences kept: with d the nominal cadence the axis wraps 1 / kept = 3.3 times round n d."""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(cadences, int(kept * cadences), replace=False))
    t = idx * d
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=len(t)) + np.cumsum(rng.normal(size=len(t)))
    return t, y, d


def _errors(got, want):
    """(worst error over max power, worst relative error where atol does not already cover it)."""
    err = np.abs(got - want)
    big = want > ATOL * want.max()
    return err.max() / want.max(), (err[big] / want[big]).max() if big.any() else 0.0


def _check(label, got, want):
    assert got.shape == want.shape and np.all(np.isfinite(got))
    to_max, rel = _errors(got, want)
    print(f"ls_fast_ref {label}: |dP|/max P = {to_max:.2e}, worst relative = {rel:.2e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL * want.max())


@pytest.mark.parametrize("n", [2, 3, 5, 257, 4096, 10007])
@pytest.mark.parametrize("red", [True, False])
@pytest.mark.parametrize("zero", [False, True])
def test_restatement_meets_the_direct_bar(n, red, zero):
    t, y = _with_n_points(n, n, red=red)
    f, got, norm = ls_fast_ref.ls_power(t, y, include_zero_freq=zero)
    f2, want, norm2 = ls_ref.ls_power(t, y, include_zero_freq=zero)
    np.testing.assert_array_equal(f, f2)
    assert norm == norm2
    _check(f"n={n} red={red} zero={zero}", got, want)


@pytest.mark.parametrize("shift", [0.0, JD_SHIFT])
def test_sparse_axis_wraps_round_the_grid(shift):
    t, y, d = _sparse()
    assert (t[-1] - t[0]) / (len(t) * d) > 3.0
    _, got, _ = ls_fast_ref.ls_power(t + shift, y, d=d)
    _, want, _ = ls_ref.ls_power(t + shift, y, d=d)
    _check(f"30% of 20000 cadences, shift={shift:.0f}", got, want)


def test_even_grid_with_degenerate_ends():
    n, d = 4096, 60e-6
    rng = np.random.default_rng(n)
    t = np.arange(n) * d
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=n) + np.cumsum(rng.normal(size=n))
    _, got, norm = ls_fast_ref.ls_power(t, y, d=d, include_zero_freq=True)
    _, want, _ = ls_ref.ls_power(t, y, d=d, include_zero_freq=True)
    _check("even grid n=4096", got, want)
    assert got[0] == 0.0
    yc = y - y.mean()
    nyq = 0.5 * n * np.mean(yc * (-1.0) ** np.arange(n)) ** 2 * norm           # the rank-one limit
    assert abs(got[-1] - nyq) <= 1e-8 * nyq


@pytest.mark.parametrize("red", [True, False])
def test_full_quarter_at_chosen_frequencies(red):
    n = 205_470
    t, y = _with_n_points(n, 31, red=red)
    M = n // 2
    pick = np.unique(np.concatenate([np.arange(0, 20), np.arange(M - 100, M),
                                     np.random.default_rng(32).integers(0, M, 121)]))
    _, got, _ = ls_fast_ref.ls_power(t, y)
    _, want, _ = ls_ref.ls_power(t, y, freq_index=pick, chunk=16)
    _check(f"n={n} red={red}, {len(pick)} frequencies", got[pick], want)


def test_cell_boundaries_and_both_ends_of_the_grid():
    """Points exactly on a cell boundary (u integer), at u = 0 and within w/2 cells of both ends of the fine
    grid, where the spreading window wraps."""
    n, d = 64, 1.0
    n_f = ls_fast_ref.grid_size(n)
    assert n_f == 300                                     # 4 (2 * 32 + 1) + 32 = 292 -> 300
    period = n * d
    u_want = np.array([0.0, 0.25, 3.0, 7.5, 8.0, 150.0, 151.5, n_f - 8.0, n_f - 7.25, n_f - 1.0, n_f - 0.5])
    rng = np.random.default_rng(3)
    rest = np.sort(rng.uniform(8.0, n_f - 8.0, n - len(u_want)))
    u_all = np.concatenate([u_want, rest])
    t = u_all / n_f * period                              # (u = k: t = k * 64 / 300, exact in binary for k = 75 j)
    t[5] = 150.0 / 300.0 * period                         # exactly half the period: u = 150 to the bit
    y = rng.normal(size=n) * 10 + np.arange(n)
    u, cell = ls_fast_ref.wrap(t, n_f, 1.0 / period)
    assert u[0] == 0.0 and u[5] == 150.0 and cell[5] == 150
    assert np.any(cell < 8) and np.any(cell >= n_f - 8)
    _, got, _ = ls_fast_ref.ls_power(t, y, d=d, include_zero_freq=True)
    _, want, _ = ls_ref.ls_power(t, y, d=d, include_zero_freq=True)
    _check("cell boundaries and grid ends", got, want)


def test_wrap_and_spread_are_periodic():
    """A point at u and the same point one period later land on the same cells with the same weights, and the
    grid of a point near the end equals that of the point shifted by one cell and rolled."""
    n_f = 45
    u = np.array([0.5, 44.5])
    g = ls_fast_ref.spread(u, u.astype(np.int64), np.ones(2), n_f)
    one = ls_fast_ref.spread(u[:1], np.array([0]), np.ones(1), n_f)
    np.testing.assert_allclose(g, one + np.roll(one, -1), rtol=1e-15, atol=0)
    assert np.count_nonzero(one) == 16
    uu, cell = ls_fast_ref.wrap(np.array([0.0, 1.25, 2.25, -0.75]), n_f, 1.0)
    np.testing.assert_array_equal(uu[1:], 0.25 * n_f)
    np.testing.assert_array_equal(cell, [0, 11, 11, 11])


def test_constant_series_is_exactly_zero():
    t, _ = _with_n_points(1001, 9)
    for value in (1234.5, -0.1):
        _, p, _ = ls_fast_ref.ls_power(t, np.full(len(t), value), include_zero_freq=True)
        assert np.all(p == 0.0)


def test_grid_sizes_are_smooth_and_hold_every_mode():
    for n in (2, 3, 5, 257, 4096, 10007, 71_000, 1_500_000, 4_400_000):
        n_f = ls_fast_ref.grid_size(n)
        assert n_f >= 4 * (2 * (n // 2) + 1) + 32 and n_f // 2 >= 2 * (n // 2)
        r = n_f
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        assert r == 1
        assert n_f <= 1.07 * (4 * (2 * (n // 2) + 1) + 32) + 8
    assert ls_fast_ref.grid_size(2) == 45 and ls_fast_ref.grid_size(5) == 54


def test_quadrature_of_the_kernel_transform():
    """64 nodes resolve phi^ over the whole band in use (k <= n_f / 4 + ...): against 512 nodes."""
    n_f = 4500
    k = np.arange(0, n_f // 4 + 1)
    z, wq = np.polynomial.legendre.leggauss(512)
    z, wq = 0.5 * (z + 1.0), 0.5 * wq
    fine = np.cos((np.pi * ls_fast_ref.W / n_f) * k[:, None] * z[None, :]) @ (ls_fast_ref.W * wq * ls_fast_ref.phi(z))
    got = ls_fast_ref.phi_hat(k, n_f)
    assert np.all(got > 0)
    assert np.max(np.abs(got - fine) / fine) < 1e-12


def test_unknown_method_is_refused_before_any_device_work():
    from gadfly_amd import psd
    t, y = _with_n_points(257, 1)
    with pytest.raises(ValueError, match="direct.*nufft"):
        psd.PowerSpectrum.from_lomb_scargle(t, y, method="fast")


def test_layout_shares_axes_and_keeps_grids_of_one_size_together():
    """Host layout of a group (psd._lsfft_layout): series given the same time array share an axis and its grid of
    ones, every grid and transform has a range of its own, and the grids of one n_f are one contiguous batch."""
    from gadfly_amd import psd
    ta, tb, tc = np.arange(64.0), np.arange(33.0), np.arange(65.0)
    ts = [ta, tb, ta, tc, tb, ta]
    nfs = [ls_fast_ref.grid_size(len(x)) for x in ts]
    assert nfs[0] == nfs[3] != nfs[1]                     # n = 64 and 65 share a grid size
    outs = [len(x) // 2 for x in ts]
    A, off, df, ax_t, classes = psd._lsfft_layout(ts, [1.0 / len(x) for x in ts], nfs, outs)
    assert A == 3 and [len(x) for x in ax_t] == [64, 33, 65]
    np.testing.assert_array_equal(off["axis"], [0, 1, 0, 2, 1, 0])
    np.testing.assert_array_equal(off["ax_off"], [0, 64, 97, 162])
    np.testing.assert_array_equal(off["cell_off"], np.concatenate([[0], np.cumsum([nfs[0], nfs[1], nfs[3]])]))
    np.testing.assert_array_equal(off["pt_off"], np.concatenate([[0], np.cumsum([len(x) for x in ts])]))
    np.testing.assert_array_equal(off["out_off"], np.concatenate([[0], np.cumsum(outs)]))
    np.testing.assert_array_equal(df, [1 / 64, 1 / 33, 1 / 65])
    assert np.all(off["pt_off"][:-1] >= off["ax_off"][off["axis"]])
    # the ones of an axis are written by its first series only
    np.testing.assert_array_equal(off["g1_off"] >= 0, [True, True, False, True, False, False])
    assert off["s1_off"][0] == off["s1_off"][2] == off["s1_off"][5] and off["s1_off"][1] == off["s1_off"][4]
    # every grid (3 of ones, 6 of y') and every transform has its own range; classes are contiguous batches
    starts = sorted([(g, nfs[r]) for r, g in enumerate(off["gy_off"])]
                    + [(g, nfs[r]) for r, g in enumerate(off["g1_off"]) if g >= 0])
    assert len(starts) == 9 and starts[0][0] == 0
    for (g, nf), (g2, _) in zip(starts, starts[1:]):
        assert g + nf == g2
    spec = sorted({(int(c), nfs[r] // 2 + 1) for r, c in enumerate(off["sy_off"])}
                  | {(int(c), nfs[r] // 2 + 1) for r, c in enumerate(off["s1_off"])})
    assert len(spec) == 9 and spec[0][0] == 0
    for (c, m), (c2, _) in zip(spec, spec[1:]):
        assert c + m == c2
    assert [nf for _, _, _, nf in classes] == sorted(set(nfs)) and sum(cnt for _, _, cnt, _ in classes) == 9
    g, c = 0, 0
    for g0, c0, cnt, nf in classes:
        assert (g0, c0) == (g, c)
        g, c = g + cnt * nf, c + cnt * (nf // 2 + 1)
        inside = [r for r in range(len(ts)) if g0 <= off["gy_off"][r] < g]
        assert all(nfs[r] == nf for r in inside)


def test_groups_stay_under_the_budget(monkeypatch):
    from gadfly_amd import psd
    nfs = [1000] * 10
    monkeypatch.setattr(psd, "_LSFFT_BUDGET", 5 * 16016)
    shared = psd._lsfft_groups(nfs, [7] * 10)              # one axis: its grids once per group
    assert shared == [(0, 4), (4, 8), (8, 10)]
    own = psd._lsfft_groups(nfs, list(range(10)))          # an axis each: two grids per series
    assert own == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)]
    monkeypatch.setattr(psd, "_LSFFT_BUDGET", 1)
    assert psd._lsfft_groups(nfs[:3], [0, 1, 2]) == [(0, 1), (1, 2), (2, 3)]      # at least one series each


def test_library_grid_size_is_the_restatement_s():
    from gadfly_amd import _lib
    lib = _lib.load()
    for n in (2, 3, 5, 64, 257, 4096, 10007, 71_000, 1_500_000):
        assert lib.gf_lsfft_grid(n) == ls_fast_ref.grid_size(n)
    assert lib.gf_lsfft_grid(1) < 0 and lib.gf_lsfft_part(3) == 3 * 64
    st = lib.gf_lsfft_finish(1, 10, 2, *([None] * 11))
    assert st < 0 and b"first" in lib.gf_last_error()
