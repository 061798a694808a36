"""
GPU: PowerSpectrum.from_lomb_scargle (gf_ls_power) against the CPU oracle tests/ls_ref.py (a direct numpy
evaluation of the floating-mean periodogram astropy's LombScargle(normalization='psd') computes for
/root/reference/gadfly/psd.py:589-601), against the FFT path on even grids, on a JD-based time axis, as
batches and ragged lists (bit-identical to single calls), at degenerate frequencies, at full light-curve
size, in the reference's statistical round trip on a gapped axis and through from_light_curve.
"""
import numpy as np
import pytest

from tests import ls_ref

pytestmark = pytest.mark.gpu

JD_SHIFT = 2454833.0 * 0.0864          # BKJD 0 in 1/uHz (jd * day)


def _gapped(n, seed, cadence=60e-6):
    """n points of a jittered axis with one long and many single-point gaps removed (fewer than n remain)."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * cadence
    keep = np.ones(n, bool)
    keep[n // 4: n // 4 + n // 10] = False
    keep[rng.integers(0, n, n // 20)] = False
    t = t[keep]
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=len(t)) + np.cumsum(rng.normal(size=len(t)))
    return t, y


def _with_n_points(n, seed):
    t, y = _gapped(int(n * 1.2) + 10, seed)
    return t[:n], y[:n]


@pytest.mark.parametrize("n", [257, 4096, 10007, 20000])
@pytest.mark.parametrize("zero", [False, True])
def test_oracle_parity(hip, n, zero):
    import gadfly_amd
    t, y = _with_n_points(n, n)
    ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, y, include_zero_freq=zero)
    d = float(np.median(np.diff(t)))
    freq, power, norm = ls_ref.ls_power(t, y, include_zero_freq=zero)
    np.testing.assert_array_equal(ps.frequency, np.fft.rfftfreq(n, d)[0 if zero else 1:])
    assert ps.norm == norm == d / (2 * np.pi) ** 0.5
    assert ps.power.shape == power.shape and np.all(np.isfinite(ps.power))
    np.testing.assert_allclose(ps.power, power, rtol=1e-8, atol=1e-10 * power.max())


@pytest.mark.parametrize("n", [4096, 10000, 100000])
def test_even_grid_equals_fft_path(hip, n):
    import gadfly_amd
    rng = np.random.default_rng(n)
    d = 60e-6
    t = np.arange(n) * d
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=n) + np.cumsum(rng.normal(size=n))
    ls = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, y, d=d)
    ff = gadfly_amd.PowerSpectrum.from_flux(y, d)
    np.testing.assert_array_equal(ls.frequency, ff.frequency)
    assert ls.norm == d / (2 * np.pi) ** 0.5
    assert np.max(np.abs(ls.power[:-1] - ff.power[:-1])) <= 1e-10 * ff.power.max()


def test_jd_axis(hip):
    import gadfly_amd
    t, y = _with_n_points(20000, 11)
    tj = t + JD_SHIFT
    ts = tj - JD_SHIFT                      # exact (Sterbenz): the same points near zero
    d = 60e-6                               # (the median step of tj is rounded at ulp(2e5): one grid for both)
    a = gadfly_amd.PowerSpectrum.from_lomb_scargle(ts, y, d=d)
    b = gadfly_amd.PowerSpectrum.from_lomb_scargle(tj, y, d=d)
    np.testing.assert_allclose(b.power, a.power, rtol=1e-10, atol=1e-10 * a.power.max())
    _, want, _ = ls_ref.ls_power(tj, y, d=d)
    np.testing.assert_allclose(b.power, want, rtol=1e-8, atol=1e-10 * want.max())


def test_batches_and_ragged_lists_are_bit_identical(hip):
    import torch
    import gadfly_amd
    t, _ = _with_n_points(12000, 21)
    rng = np.random.default_rng(22)
    flux = 100 * rng.normal(size=(4, len(t))) + np.cumsum(rng.normal(size=(4, len(t))), axis=-1)
    dev = torch.as_tensor(flux, device="cuda")
    ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, dev)
    again = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, flux)
    assert ps.power.shape == (4, len(t) // 2) and ps._power_dev.is_cuda
    np.testing.assert_array_equal(ps.power, again.power)
    for r in range(4):
        one = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, flux[r])
        np.testing.assert_array_equal(ps.power[r], one.power)
    # (R, N) time axes with one common step
    rows = gadfly_amd.PowerSpectrum.from_lomb_scargle(np.stack([t] * 4), flux)
    np.testing.assert_array_equal(rows.power, ps.power)
    b = ps.bin(20)
    assert b.power.shape == (4, 20) and b.error.shape == (4, 20) and np.all(np.isfinite(b.power))
    # a ragged list of 5 series, 3001 ... 20011 points
    pairs = [_with_n_points(n, n) for n in (3001, 20011, 7777, 12345, 4096)]
    many = gadfly_amd.PowerSpectrum.from_lomb_scargle(pairs)
    assert isinstance(many, list) and len(many) == 5
    for (tr, yr), got in zip(pairs, many):
        one = gadfly_amd.PowerSpectrum.from_lomb_scargle(tr, yr)
        np.testing.assert_array_equal(got.frequency, one.frequency)
        np.testing.assert_array_equal(got.power, one.power)
        assert got.norm == one.norm and got._power_dev.is_cuda
    b = many[1].bin(20)
    assert b.power.shape == (20,) and np.all(np.isfinite(b.power))


def test_degenerate_frequencies(hip):
    import gadfly_amd
    n, d = 10000, 60e-6
    t = np.arange(n) * d
    y = np.random.default_rng(5).normal(size=n) * 40
    ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, y, include_zero_freq=True)
    assert np.all(np.isfinite(ps.power))
    assert ps.power[0] == 0.0
    _, want, norm = ls_ref.ls_power(t, y, include_zero_freq=True)
    yc = y - y.mean()
    nyq = 0.5 * n * np.mean(yc * (-1.0) ** np.arange(n)) ** 2 * norm           # the rank-one limit
    assert abs(want[-1] - nyq) <= 1e-12 * nyq
    assert abs(ps.power[-1] - nyq) <= 1e-8 * nyq
    np.testing.assert_allclose(ps.power, want, rtol=1e-8, atol=1e-10 * want.max())
    const = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, np.full(n, 1234.5), include_zero_freq=True)
    assert np.all(const.power == 0.0)
    tg, _ = _gapped(5000, 6)
    const = gadfly_amd.PowerSpectrum.from_lomb_scargle(tg, np.full(len(tg), -0.1))
    assert np.all(const.power == 0.0)


def test_full_size(hip):
    import gadfly_amd
    t, y = _with_n_points(400_000, 31)
    ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, y)
    M = len(ps.power)
    assert M == 200_000 and np.all(np.isfinite(ps.power))
    rng = np.random.default_rng(32)
    tile = 16 * 256                                    # frequencies per workgroup of the sum pass
    edges = np.arange(tile, M, tile)
    pick = np.unique(np.concatenate([
        np.arange(M - 100, M), np.arange(0, 20), edges - 1, edges, edges + 15,
        rng.integers(0, M, 60)]))
    pick = pick[(pick >= 0) & (pick < M)]
    assert len(pick) >= 250
    _, want, _ = ls_ref.ls_power(t, y, freq_index=pick, chunk=16)
    np.testing.assert_allclose(ps.power[pick], want, rtol=1e-8, atol=1e-10 * want.max())


def test_round_trip_on_gapped_axis(hip, n_trials=4, nbins=15):
    """The reference's hot-path test (gadfly/tests/test_core.py:19-51) on a gapped axis: sample_device ->
    Lomb-Scargle -> log bins, within 5 sigma of kernel.get_psd for 3 < f < 1000 uHz."""
    import gadfly_amd
    from gadfly_amd.synth import solar_like_hyperparameters
    np.random.seed(42)
    kernel = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(30), texp=60.0)
    t = np.arange(100_000) * 60e-6
    keep = np.ones(len(t), bool)
    for a, w in ((21_000, 700), (48_000, 1500), (77_000, 400)):
        keep[a:a + w] = False
    t = t[keep]
    gp = gadfly_amd.GaussianProcess(kernel, t=t)
    draws = gp.sample_device(size=n_trials)
    ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, draws, name="draws").bin(nbins)
    model = kernel.get_psd(2 * np.pi * ps.frequency)
    ok = (ps.frequency < 1e3) & (ps.frequency > 3)
    for r in range(n_trials):
        dev = np.abs((model[ok] - ps.power[r][ok]) / np.nanmax(ps.error[r]))
        assert np.nanmax(dev) < 5


def test_from_light_curve(hip):
    import types
    import gadfly_amd
    from gadfly_amd import units
    from tests.fake_units import FakeTime
    t, y = _with_n_points(6000, 41)
    days = t * units.SECONDS_PER_INVERSE_UHZ / 86400.0
    lc = types.SimpleNamespace(time=FakeTime(days, format="bkjd"), flux=y, meta={"name": "KIC 0"})
    got = gadfly_amd.PowerSpectrum.from_light_curve(lc, method="lomb-scargle")
    tt = lc.time.jd * 86400.0 / units.SECONDS_PER_INVERSE_UHZ
    want = gadfly_amd.PowerSpectrum.from_lomb_scargle(tt, y)
    assert got.name == "KIC 0"
    np.testing.assert_array_equal(got.frequency, want.frequency)
    np.testing.assert_array_equal(got.power, want.power)
    assert got.norm == want.norm
