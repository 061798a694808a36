"""
GPU: PowerSpectrum.from_lomb_scargle(method="nufft") (gf_lsfft_prepare / _spread / _finish around a torch sort
and hipFFT) against the exact CPU oracle tests/ls_ref.py at the direct route's own bar (rtol 1e-8, atol 1e-10
max), on sparse axes that wrap round the fine grid, on a JD-based axis, against the FFT path on an even grid,
against method="direct" on the device, in every input layout, at degenerate frequencies, through .bin() and
from_light_curve.  Each test prints its worst errors before it asserts (pytest -s).
"""
import functools

import numpy as np
import pytest

from tests import ls_ref

pytestmark = pytest.mark.gpu

JD_SHIFT = 2454833.0 * 0.0864          # BKJD 0 in 1/uHz (jd * day)
RTOL, ATOL = 1e-8, 1e-10


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


def _sparse(seed=7, cadences=20000, kept=0.3, d=60e-6):
    """30 % of the cadences kept: with d the nominal cadence the axis wraps 1 / kept = 3.3 times round n d."""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(cadences, int(kept * cadences), replace=False))
    t = idx * d
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=len(t)) + np.cumsum(rng.normal(size=len(t)))
    return t, y, d


@functools.lru_cache(maxsize=None)
def _oracle(n):
    """The exact power of _with_n_points(n, n) with the zero frequency, computed once per n."""
    t, y = _with_n_points(n, n)
    _, power, _ = ls_ref.ls_power(t, y, include_zero_freq=True)
    power.setflags(write=False)
    return power


def _fast(*args, **kwargs):
    import gadfly_amd
    return gadfly_amd.PowerSpectrum.from_lomb_scargle(*args, method="nufft", **kwargs)


def _direct(*args, **kwargs):
    import gadfly_amd
    return gadfly_amd.PowerSpectrum.from_lomb_scargle(*args, method="direct", **kwargs)


def _check(label, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = np.abs(got - want)
    big = want > ATOL * want.max()
    rel = (err[big] / want[big]).max() if big.any() else 0.0
    print(f"nufft {label}: |dP|/max P = {err.max() / want.max():.2e}, worst relative = {rel:.2e}")
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL * want.max())


def _within(label, got, want, frac):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    worst = np.max(np.abs(got - want)) / want.max()
    print(f"nufft {label}: |dP|/max P = {worst:.2e} (bound {frac:.0e})")
    assert worst <= frac


@pytest.mark.parametrize("n", [2, 3, 5, 257, 4096, 10007])
@pytest.mark.parametrize("zero", [False, True])
def test_oracle_parity(hip, n, zero):
    t, y = _with_n_points(n, n)
    ps = _fast(t, y, include_zero_freq=zero)
    d = float(np.median(np.diff(t)))
    np.testing.assert_array_equal(ps.frequency, np.fft.rfftfreq(n, d)[0 if zero else 1:])
    assert ps.norm == d / (2 * np.pi) ** 0.5
    _check(f"n={n} zero={zero}", ps.power, _oracle(n)[0 if zero else 1:])


def test_sparse_axis_wraps_round_the_grid(hip):
    t, y, d = _sparse()
    assert (t[-1] - t[0]) / (len(t) * d) > 3.0
    _, want, _ = ls_ref.ls_power(t, y, d=d)
    _check("30% of 20000 cadences", _fast(t, y, d=d).power, want)


def test_jd_axis(hip):
    t, y, d = _sparse(seed=11)
    tj = t + JD_SHIFT
    ts = tj - JD_SHIFT                      # exact (Sterbenz): the same points near zero
    a = _fast(ts, y, d=d)
    b = _fast(tj, y, d=d)
    _check("BKJD axis against the shifted-back one", b.power, a.power)
    _, want, _ = ls_ref.ls_power(tj, y, d=d)
    _check("BKJD axis against the oracle", b.power, want)


def test_even_grid_equals_fft_path(hip):
    import gadfly_amd
    n, d = 4096, 60e-6
    rng = np.random.default_rng(n)
    t = np.arange(n) * d
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=n) + np.cumsum(rng.normal(size=n))
    ls = _fast(t, y, d=d)
    ff = gadfly_amd.PowerSpectrum.from_flux(y, d)
    np.testing.assert_array_equal(ls.frequency, ff.frequency)
    assert ls.norm == d / (2 * np.pi) ** 0.5
    _within("even grid against from_flux", ls.power[:-1], ff.power[:-1], 1e-10)


def test_agrees_with_the_direct_route(hip):
    t, y = _with_n_points(20000, 20000)
    for zero in (False, True):
        a = _direct(t, y, include_zero_freq=zero)
        b = _fast(t, y, include_zero_freq=zero)
        np.testing.assert_array_equal(a.frequency, b.frequency)
        assert a.norm == b.norm
        _check(f"n=20000 against method='direct', zero={zero}", b.power, a.power)


def test_layouts_agree_with_single_calls(hip):
    import torch
    t, _ = _with_n_points(12000, 21)
    rng = np.random.default_rng(22)
    flux = 100 * rng.normal(size=(4, len(t))) + np.cumsum(rng.normal(size=(4, len(t))), axis=-1)
    singles = [_fast(t, flux[r]).power for r in range(4)]
    # (R, N) flux on a shared axis, from the host and from a device tensor
    ps = _fast(t, flux)
    dev = _fast(t, torch.as_tensor(flux, device="cuda"))
    assert ps.power.shape == (4, len(t) // 2) and ps._power_dev.is_cuda and ps._power_dev.shape == ps.power.shape
    np.testing.assert_array_equal(ps.power, dev.power)
    np.testing.assert_array_equal(ps.power, _fast(t, flux).power)           # the same call twice: bit-identical
    for r in range(4):
        _within(f"shared axis, row {r}", ps.power[r], singles[r], 1e-12)
    # (R, N) time axes with one common step
    rows = _fast(np.stack([t] * 4), flux)
    for r in range(4):
        _within(f"(R, N) axes, row {r}", rows.power[r], singles[r], 1e-12)
    # a device-tensor flux of one series
    one = _fast(t, torch.as_tensor(flux[2], device="cuda"))
    np.testing.assert_array_equal(one.power, singles[2])
    # a ragged list
    pairs = [_with_n_points(n, n) for n in (12000, 2, 4097, 1001)]
    many = _fast(pairs)
    again = _fast(pairs)
    assert isinstance(many, list) and len(many) == 4
    for (tr, yr), got, twice in zip(pairs, many, again):
        alone = _fast(tr, yr)
        np.testing.assert_array_equal(got.frequency, alone.frequency)
        assert got.norm == alone.norm and got._power_dev.is_cuda
        _within(f"ragged list, n={len(tr)}", got.power, alone.power, 1e-12)
        np.testing.assert_array_equal(got.power, twice.power)


def test_degenerate_frequencies(hip):
    n, d = 10000, 60e-6
    t = np.arange(n) * d
    y = np.random.default_rng(5).normal(size=n) * 40
    ps = _fast(t, y, include_zero_freq=True)
    ref = _direct(t, y, include_zero_freq=True)
    assert np.all(np.isfinite(ps.power))
    assert ps.power[0] == 0.0 == ref.power[0]
    yc = y - y.mean()
    nyq = 0.5 * n * np.mean(yc * (-1.0) ** np.arange(n)) ** 2 * ps.norm         # the rank-one limit
    print(f"nufft Nyquist: {ps.power[-1]:.15e}, direct {ref.power[-1]:.15e}, limit {nyq:.15e}")
    assert abs(ps.power[-1] - nyq) <= 1e-8 * nyq and abs(ps.power[-1] - ref.power[-1]) <= 1e-8 * nyq
    _check("even grid with f = 0 and Nyquist against method='direct'", ps.power, ref.power)
    const = _fast(t, np.full(n, 1234.5), include_zero_freq=True)
    assert np.all(const.power == 0.0)
    tg, _ = _gapped(5000, 6)
    const = _fast(tg, np.full(len(tg), -0.1))
    assert np.all(const.power == 0.0)


def test_bin_runs_from_the_device_copy(hip):
    t, y = _with_n_points(4097, 4097)
    ps = _fast(t, y, name="a star")
    assert ps.name == "a star" and ps._power_dev is not None and ps._power_dev.is_cuda
    np.testing.assert_array_equal(ps._power_dev.cpu().numpy().reshape(-1), ps.power)
    peak = ps.power.max()
    ps.power = np.full_like(ps.power, np.nan)           # .bin() reads the device copy, not this
    b = ps.bin(15)
    assert b.power.shape == (15,) and b.error.shape == (15,) and np.all(np.isfinite(b.power))
    want = _direct(t, y).bin(15)
    np.testing.assert_allclose(b.power, want.power, rtol=RTOL, atol=ATOL * peak)


def test_from_light_curve(hip):
    import types
    import gadfly_amd
    from gadfly_amd import units
    from tests.fake_units import FakeTime
    t, y = _with_n_points(6000, 41)
    days = t * units.SECONDS_PER_INVERSE_UHZ / 86400.0
    lc = types.SimpleNamespace(time=FakeTime(days, format="bkjd"), flux=y, meta={"name": "KIC 0"})
    got = gadfly_amd.PowerSpectrum.from_light_curve(lc, method="lomb-scargle", ls_method="nufft")
    tt = lc.time.jd * 86400.0 / units.SECONDS_PER_INVERSE_UHZ
    want = _fast(tt, y)
    assert got.name == "KIC 0"
    np.testing.assert_array_equal(got.frequency, want.frequency)
    np.testing.assert_array_equal(got.power, want.power)
    assert got.norm == want.norm
    _check("from_light_curve against method='direct'",
           got.power, gadfly_amd.PowerSpectrum.from_light_curve(lc, method="lomb-scargle").power)


def test_unknown_method_is_refused(hip):
    t, y = _with_n_points(257, 1)
    import gadfly_amd
    with pytest.raises(ValueError, match="direct.*nufft"):
        gadfly_amd.PowerSpectrum.from_lomb_scargle(t, y, method="fast")
