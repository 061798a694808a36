"""CPU: the Lomb-Scargle oracle (tests/ls_ref.py) against itself and the FFT path, and the host side of
PowerSpectrum.from_lomb_scargle (frequency grid, argument validation) -- no GPU needed."""
import numpy as np
import pytest

from gadfly_amd import psd
from oracle import psd_ref
from tests import ls_ref


def _gapped(n, seed, cadence=60e-6):
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * cadence
    keep = np.ones(n, bool)
    keep[n // 4: n // 4 + n // 10] = False
    keep[rng.integers(0, n, n // 20)] = False
    t = t[keep]
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=len(t)) + np.cumsum(rng.normal(size=len(t)))
    return t, y


@pytest.mark.parametrize("n,seed", [(257, 1), (1000, 2), (4096, 3)])
def test_quadratic_form_equals_tau_form(n, seed):
    t, y = _gapped(n, seed)
    d = float(np.median(np.diff(t)))
    freq = np.fft.rfftfreq(len(t), d)[1:]
    a = ls_ref.power_quadratic(t, y, freq)
    b = ls_ref.power_tau(t, y, freq)
    assert np.all(np.isfinite(a)) and np.all(a >= 0)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * a.max())


@pytest.mark.parametrize("n", [512, 1000, 4097])
def test_even_sampling_equals_fft_power(n):
    rng = np.random.default_rng(n)
    d = 60e-6
    t = np.arange(n) * d
    y = 300 * np.sin(2 * np.pi * 3000.0 * t) + 50 * rng.normal(size=n)
    f, p, norm = ls_ref.ls_power(t, y, d=d)
    ff, pf, _ = psd_ref.fft_power(y, d)
    np.testing.assert_array_equal(f, ff)
    assert norm == d / (2 * np.pi) ** 0.5
    inner = slice(0, -1) if n % 2 == 0 else slice(None)          # the Nyquist frequency of an even n differs
    assert np.max(np.abs(p[inner] - pf[inner])) <= 1e-10 * pf.max()


def test_degenerate_limits_in_the_oracle():
    n, d = 1024, 60e-6
    t = np.arange(n) * d
    y = np.random.default_rng(0).normal(size=n)
    f, p, norm = ls_ref.ls_power(t, y, d=d, include_zero_freq=True)
    assert p[0] == 0 and np.all(np.isfinite(p))
    # Nyquist of an even, evenly sampled series: the fit onto the cosine column alone
    yc = y - y.mean()
    want = 0.5 * n * (np.mean(yc * (-1.0) ** np.arange(n))) ** 2 * norm
    assert abs(p[-1] - want) <= 1e-12 * want
    _, pc, _ = ls_ref.ls_power(t, np.full(n, 7.25), d=d, include_zero_freq=True)
    assert np.all(np.isfinite(pc)) and np.max(np.abs(pc)) < 1e-20


@pytest.mark.parametrize("n", [2, 3, 10, 11, 4096, 10007, 400001])
@pytest.mark.parametrize("d", [60e-6, 1.7642e-3, 0.1, 1.0 / 3.0])
def test_grid_is_rfftfreq_bit_for_bit(n, d):
    f, df = psd.ls_grid(n, d)
    np.testing.assert_array_equal(f, np.fft.rfftfreq(n, d))
    assert df == 1.0 / (n * d)


def test_series_layouts():
    t, y = _gapped(300, 5)
    s, lay = psd._ls_series(t, y, None)
    assert lay == "single" and len(s) == 1 and s[0][2] == np.median(np.diff(t))
    s, lay = psd._ls_series(t, np.stack([y, 2 * y]), None)
    assert lay == "batch" and len(s) == 2 and np.array_equal(s[1][0], t)
    s, lay = psd._ls_series(np.stack([t, t]), np.stack([y, y]), None)
    assert lay == "batch" and s[1][2] == s[0][2]
    s, lay = psd._ls_series(np.stack([t, t + 5.0]), np.stack([y, y]), 60e-6)     # explicit d: any rows
    assert lay == "batch" and s[0][2] == s[1][2] == 60e-6
    s, lay = psd._ls_series([(t, y), (t[:100], y[:100])], None, 1e-4)
    assert lay == "list" and [len(x[0]) for x in s] == [len(t), 100] and s[1][2] == 1e-4


def test_argument_validation():
    t, y = _gapped(300, 6)
    bad = y.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        psd._ls_series(t, bad, None)
    tb = t.copy()
    tb[3] = np.inf
    with pytest.raises(ValueError, match="NaN"):
        psd._ls_series(tb, y, None)
    with pytest.raises(ValueError):
        psd._ls_series(t[:1], y[:1], None)
    with pytest.raises(ValueError):
        psd._ls_series(t, y[:-1], None)
    with pytest.raises(ValueError):
        psd._ls_series(t[:-1], np.stack([y, y]), None)
    with pytest.raises(ValueError):
        psd._ls_series(t, y, -1.0)
    with pytest.raises(ValueError, match="median"):
        psd._ls_series(np.stack([t, 2 * t]), np.stack([y, y]), None)
    with pytest.raises(ValueError):
        psd._ls_series([(t, y[:-1])], None, None)
    with pytest.raises(ValueError):
        psd._ls_series([], None, None)
    with pytest.raises(ValueError):
        psd._ls_series(t, np.zeros((2, 3, 300)), None)
    # the public entry point validates before it touches a device
    with pytest.raises(ValueError, match="NaN"):
        psd.PowerSpectrum.from_lomb_scargle(t, bad)


def test_light_curve_detrend_still_refused():
    from tests.fake_units import FakeTime
    import types
    lc = types.SimpleNamespace(time=FakeTime(np.arange(10) / 1440.0, format="bkjd"), flux=np.zeros(10))
    with pytest.raises(NotImplementedError):
        psd.PowerSpectrum.from_light_curve(lc, method="lomb-scargle", detrend=True)
