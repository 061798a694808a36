"""GPU: the segmented detrend kernels at their entry points (gf_seg_median, gf_sigma_clip, gf_seg_compact,
gf_poly_normalise) and gadfly_amd.prepare_quarters / prepare_quarters_batch / PowerSpectrum.from_quarters against the
numpy restatement of tests/detrend_ref.py.

Flux bar: 1e-6 ppm absolute against the 80-bit restatement and against the float64 one -- the results are
1e6 (r - 1) with r of order one, so 1e-12 in r, two orders above what float64 routes differ from 80-bit on the CPU
(tests/test_detrend_host.py: 2e-10 .. 9e-9 ppm; the device itself measured 3.8e-9 and 6.9e-10 ppm).
Masks, counts, rounds, time axes and cadences are compared with ==.
"""
import numpy as np
import pytest

from tests import detrend_ref

pytestmark = pytest.mark.gpu

FLUX_BAR_PPM = 1e-6
MARGIN = 1e-9               # the restatement's thresholds must stay this far (relative) from every point
LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 5000]


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")


def _off(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def seg_median(hip, segments, masks=None):
    import torch
    lib = hip.load()
    S = len(segments)
    off, x = _dev(_off([len(s) for s in segments])), _dev(np.concatenate(segments), np.float64)
    keep = None if masks is None else _dev(np.concatenate(masks), np.uint8)
    med = torch.empty(S, dtype=torch.float64, device="cuda")
    hip.check(lib.gf_seg_median(S, hip.ptr(off), hip.ptr(x), hip.ptr(keep), 0, hip.ptr(med), hip.stream_handle()),
              "gf_seg_median")
    return med.cpu().numpy()


def sigma_clip(hip, segments, lo=5.0, hi=5.0, maxiters=5, times=None):
    import torch
    lib = hip.load()
    S = len(segments)
    off_h = _off([len(s) for s in segments])
    off, f = _dev(off_h), _dev(np.concatenate(segments), np.float64)
    t = None if times is None else _dev(np.concatenate(times), np.float64)
    keep = torch.empty(int(off_h[-1]), dtype=torch.uint8, device="cuda")
    kept = torch.empty(S, dtype=torch.int64, device="cuda")
    rounds = torch.empty(S, dtype=torch.int32, device="cuda")
    hip.check(lib.gf_sigma_clip(S, hip.ptr(off), hip.ptr(t), hip.ptr(f), lo, hi, maxiters, hip.ptr(keep),
                                hip.ptr(kept), hip.ptr(rounds), hip.stream_handle()), "gf_sigma_clip")
    keep_h = keep.cpu().numpy().astype(bool)
    return [keep_h[off_h[s]:off_h[s + 1]] for s in range(S)], kept.cpu().numpy(), rounds.cpu().numpy()


# ---------------------------------------------------------------------------------------------- median
def _median_data(kind, n, rng):
    if kind == "quantised":                 # many duplicates, both signs, +0 and -0
        x = np.round(rng.standard_normal(n) * 3.0)
        x[x == 0] *= rng.choice([-1.0, 1.0], int((x == 0).sum()))
        return x
    if kind == "negative":
        return -np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-3, 4, n)
    if kind == "mixed":
        return rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    return np.full(n, -7.25 if n % 2 else 3.5)          # "equal"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", ["quantised", "negative", "mixed", "equal"])
def test_median_equals_numpy(hip, kind, masked):
    rng = np.random.default_rng(LENGTHS.index(64) + len(kind) + 100 * masked)
    segs = [_median_data(kind, n, rng) for n in LENGTHS]
    masks = None
    if masked:
        masks = [rng.random(n) < 0.6 for n in LENGTHS]
        for m in masks:
            m[rng.integers(len(m))] = True
    want = np.array([np.median(x if masks is None else x[masks[i]]) for i, x in enumerate(segs)])
    got = seg_median(hip, segs, masks)
    assert np.all(got == want), (got, want)
    for i, x in enumerate(segs):            # each segment alone
        alone = seg_median(hip, [x], None if masks is None else [masks[i]])
        assert alone[0] == want[i], (LENGTHS[i], alone[0], want[i])


def test_median_of_nothing_is_nan_and_neighbours_are_untouched(hip):
    segs = [np.array([3.0, 1.0, 2.0]), np.array([5.0, 4.0]), np.array([9.0])]
    masks = [np.array([1, 1, 1], bool), np.array([0, 0], bool), np.array([1], bool)]
    got = seg_median(hip, segs, masks)
    assert got[0] == 2.0 and np.isnan(got[1]) and got[2] == 9.0


# ---------------------------------------------------------------------------------------------- clip
def _clip_flux(seed, n):
    rng = np.random.default_rng(1000 * seed + n)
    f = 2.3e5 * (1 + 3e-4 * rng.standard_normal(n))
    if n >= 5:
        k = max(1, n // 40)
        f[rng.choice(n, k, replace=False)] *= 1 + rng.choice([-1, 1], k) * rng.uniform(0.002, 0.05, k)
        f[rng.choice(n, max(1, n // 50), replace=False)] = np.nan
    return np.round(f, 1)


def _check_clip(hip, segs, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5, alone=False):
    want = [detrend_ref.sigma_clip(f, None, sigma, sigma_lower, sigma_upper, maxiters) for f in segs]
    margins = [w[2] for w in want]
    print("rounds", [w[1] for w in want], "least margin %.1e" % min(margins))
    assert min(margins) >= MARGIN            # the restatement's own masks do not hang on rounding
    if sigma is None:
        lo = hi = 1.0
        iters = 0
    else:
        lo = sigma if sigma_lower is None else sigma_lower
        hi = sigma if sigma_upper is None else sigma_upper
        iters = -1 if maxiters is None else maxiters
    groups = [[i] for i in range(len(segs))] if alone else [list(range(len(segs)))]
    for g in groups:
        keep, kept, rounds = sigma_clip(hip, [segs[i] for i in g], lo, hi, iters)
        for j, i in enumerate(g):
            np.testing.assert_array_equal(keep[j], want[i][0])
            assert kept[j] == want[i][0].sum() and rounds[j] == want[i][1], (len(segs[i]), rounds[j], want[i][1])
    return want


@pytest.mark.parametrize("seed", range(6))
def test_clip_equals_restatement(hip, seed):
    want = _check_clip(hip, [_clip_flux(seed, n) for n in LENGTHS])
    assert max(w[1] for w in want) >= 2 and all(1 <= w[1] <= 5 for w in want)


def test_clip_alone_capped_uncapped_asymmetric_and_off(hip):
    segs = [_clip_flux(0, n) for n in LENGTHS]
    full = _check_clip(hip, segs, alone=True)
    capped = _check_clip(hip, segs, maxiters=2)
    assert any(f[1] > 2 for f in full) and all(c[1] <= 2 for c in capped)       # the cap binds
    assert any(c[0].sum() > f[0].sum() for c, f in zip(capped, full))
    _check_clip(hip, segs, maxiters=None)
    asym = _check_clip(hip, segs, sigma_lower=3.0, sigma_upper=6.0)
    assert any(not np.array_equal(a[0], f[0]) for a, f in zip(asym, full))
    off = _check_clip(hip, segs, sigma=None)
    assert all(o[1] == 0 for o in off)


def test_clip_drops_rows_with_a_non_finite_time(hip):
    f = _clip_flux(1, 257)
    t = np.arange(257.0)
    t[[3, 200]] = [np.nan, np.inf]
    keep, kept, _ = sigma_clip(hip, [f], times=[t])
    want, _, margin = detrend_ref.sigma_clip(f, t)
    assert margin >= MARGIN and not want[3] and not want[200]
    np.testing.assert_array_equal(keep[0], want)
    assert kept[0] == want.sum()


# ---------------------------------------------------------------------------------------------- public API
def _quarter(rng, n, t0, cad, raw=True):
    """n cadences from t0 with 8 % missing and a run of 20 out; raw: flares, dips and NaNs in flux and time."""
    keep = rng.random(n) > 0.08
    a = int(rng.integers(n // 4, n // 2))
    keep[a:a + 20] = False
    keep[[0, -1]] = True
    t = (t0 + np.arange(n) * cad)[keep]
    x = (t - t.mean()) / (t.max() - t.min())
    f = 2.3e5 * (1 + 0.02 * (x + 0.7 * x ** 2 - 1.3 * x ** 3)) * (1 + 3e-4 * rng.standard_normal(t.size))
    if raw:
        m = t.size
        k = max(2, m // 60)
        f[rng.choice(m, k, replace=False)] *= 1 + rng.choice([-1, 1], k) * rng.uniform(0.01, 0.05, k)
        f[rng.choice(m, 3, replace=False)] = np.nan
        t[rng.choice(np.arange(1, m - 1), 2, replace=False)] = np.nan
    return t, f


def _stars(t0, raw=True, seed=5):
    """B = 3 stars with 1, 2 and 4 quarters of 300 .. 5000 points, gaps inside and between the quarters."""
    rng = np.random.default_rng(seed)
    cad = 0.0204
    shapes = [[1500], [300, 5000], [900, 333, 2049, 1024]]
    stars = []
    for lens in shapes:
        start, quarters = t0, []
        for n in lens:
            quarters.append(_quarter(rng, n, start, cad, raw))
            start += (n + int(rng.integers(30, 120))) * cad
        stars.append(quarters)
    return stars


def _reference(stars, normaliser, **kw):
    out, least = [], np.inf
    for quarters in stars:
        details = []
        out.append(detrend_ref.prepare_quarters(quarters, normaliser=normaliser, details=details, **kw))
        least = min([least] + [d[2] for d in details])
    return out, least


@pytest.mark.parametrize("fill", [True, False])
@pytest.mark.parametrize("order", [0, 3, 8])
@pytest.mark.parametrize("t0", [131.5, 2454964.5], ids=["bkjd", "jd"])
def test_prepare_quarters_batch_against_restatement(hip, t0, order, fill):
    import gadfly_amd
    stars = _stars(t0)
    want64, least = _reference(stars, "legendre", detrend_poly_order=order, fill=fill)
    want80, _ = _reference(stars, "longdouble", detrend_poly_order=order, fill=fill)
    assert least >= MARGIN
    got = gadfly_amd.prepare_quarters_batch(stars, detrend_poly_order=order, fill=fill)
    assert len(got) == 3
    worst64 = worst80 = 0.0
    for (t, f, cad), (t64, f64, cad64), (t80, f80, _) in zip(got, want64, want80):
        assert t.shape == t64.shape == f.shape
        np.testing.assert_array_equal(t, t64)
        np.testing.assert_array_equal(t, t80)
        assert cad == cad64
        worst64 = max(worst64, float(np.abs(f - f64).max()))
        worst80 = max(worst80, float(np.abs(f - f80).max()))
    print("t0=%s order=%d fill=%s: device flux within %.2e ppm of float64, %.2e ppm of 80-bit" % (
        t0, order, fill, worst64, worst80))
    assert worst64 <= FLUX_BAR_PPM and worst80 <= FLUX_BAR_PPM


def test_in_ppm_is_bit_identical_and_single_star_call(hip):
    import gadfly_amd
    stars = _stars(131.5)
    want, least = _reference(stars, "legendre", in_ppm=True)
    assert least >= MARGIN
    got = gadfly_amd.prepare_quarters_batch(stars, in_ppm=True)
    for (t, f, cad), (rt, rf, rcad) in zip(got, want):
        np.testing.assert_array_equal(t, rt)
        np.testing.assert_array_equal(f, rf)
        assert cad == rcad
    t, f, cad = gadfly_amd.prepare_quarters(stars[2], in_ppm=True, fill=False)
    rt, rf, rcad = detrend_ref.prepare_quarters(stars[2], in_ppm=True, fill=False)
    np.testing.assert_array_equal(t, rt)
    np.testing.assert_array_equal(f, rf)
    assert cad == rcad


@pytest.mark.parametrize("t0", [131.5, 2454964.5], ids=["bkjd", "jd"])
def test_clean_input_equals_stitch_quarters(hip, t0):
    import gadfly_amd
    for quarters in _stars(t0, raw=False):
        t, f, cad = gadfly_amd.prepare_quarters(quarters)
        rt, rf, rcad = gadfly_amd.stitch_quarters(quarters)
        np.testing.assert_array_equal(t, rt)
        assert cad == rcad
        assert np.abs(f - rf).max() <= FLUX_BAR_PPM


def test_batch_independence_and_repeatability(hip):
    import gadfly_amd
    stars = _stars(2454964.5, seed=9)
    batch = gadfly_amd.prepare_quarters_batch(stars, detrend_poly_order=5)
    again = gadfly_amd.prepare_quarters_batch(stars, detrend_poly_order=5)
    swapped = gadfly_amd.prepare_quarters_batch(stars[::-1], detrend_poly_order=5)[::-1]
    for b, quarters in enumerate(stars):
        alone = gadfly_amd.prepare_quarters(quarters, detrend_poly_order=5)
        for other in (again[b], swapped[b], alone):
            np.testing.assert_array_equal(batch[b][0], other[0])
            np.testing.assert_array_equal(batch[b][1], other[1])
            assert batch[b][2] == other[2]


def test_too_few_survivors_name_star_and_quarter(hip):
    import gadfly_amd
    t = 100.0 + np.arange(9) * 0.02
    f = np.array([1.0] * 8 + [2.0]) * 1e4           # nine finite rows pass the host check; the clip takes the last
    good = (t - 10.0, 1e4 + np.arange(9.0))
    with pytest.raises(ValueError, match="star 1, quarter 1: 8 points survive the clip, 9 are needed"):
        gadfly_amd.prepare_quarters_batch([[good], [good, (t, f)]], detrend_poly_order=8, sigma=3.0)


def test_ragged_result_feeds_the_batched_consumers(hip):
    import gadfly_amd
    from gadfly_amd.synth import solar_like_hyperparameters
    stars = _stars(131.5)
    pairs, cadences = gadfly_amd.prepare_quarters_batch(stars, fill=False, return_device=True)
    host = gadfly_amd.prepare_quarters_batch(stars, fill=False)
    assert all(t.is_cuda and f.is_cuda and t.shape == f.shape for t, f in pairs)
    for (t, f), c, (th, fh, ch) in zip(pairs, cadences, host):
        np.testing.assert_array_equal(t.cpu().numpy(), th)
        np.testing.assert_array_equal(f.cpu().numpy(), fh)
        assert c == ch
    day = 0.0864
    spectra = gadfly_amd.PowerSpectrum.from_lomb_scargle([(th * day, f) for (_, f), (th, _, _) in zip(pairs, host)])
    assert len(spectra) == 3 and all(np.all(np.isfinite(ps.power)) for ps in spectra)
    kernel = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(2), texp=60.0)
    ll = gadfly_amd.log_likelihood_batch([kernel] * 3, [th * day for th, _, _ in host], [fh for _, fh, _ in host],
                                         yerr=30.0)
    assert ll.shape == (3,) and np.all(np.isfinite(ll))
    filled, cad = gadfly_amd.prepare_quarters_batch(stars[:1], return_device=True)
    ps = gadfly_amd.PowerSpectrum.from_flux(filled[0][1], cad[0] * day)
    assert ps.power.shape == (len(filled[0][1]) // 2,) and np.all(np.isfinite(ps.power))


def test_from_quarters_equals_the_spectrum_of_its_own_preparation(hip):
    import gadfly_amd
    quarters = _stars(2454964.5)[1]
    day = 0.0864
    t, f, cad = gadfly_amd.prepare_quarters(quarters, detrend_poly_order=2)
    ps = gadfly_amd.PowerSpectrum.from_quarters(quarters, detrend_poly_order=2, name="star")
    want = gadfly_amd.PowerSpectrum.from_flux(f, cad * 86400.0 / gadfly_amd.units.SECONDS_PER_INVERSE_UHZ)
    np.testing.assert_array_equal(ps.frequency, want.frequency)
    np.testing.assert_array_equal(ps.power, want.power)
    assert ps.norm == want.norm and ps.name == "star"
    np.testing.assert_array_equal(ps.detrended_lc[0], t)
    np.testing.assert_array_equal(ps.detrended_lc[1], f)
    assert abs(86400.0 / gadfly_amd.units.SECONDS_PER_INVERSE_UHZ - day) < 1e-15
    tg, fg, _ = gadfly_amd.prepare_quarters(quarters, detrend_poly_order=2, fill=False)
    for ls_method in ("direct", "nufft"):
        ps = gadfly_amd.PowerSpectrum.from_quarters(quarters, method="lomb-scargle", detrend_poly_order=2,
                                                    ls_method=ls_method, include_zero_freq=True)
        want = gadfly_amd.PowerSpectrum.from_lomb_scargle(tg * 86400.0 / gadfly_amd.units.SECONDS_PER_INVERSE_UHZ, fg,
                                                          include_zero_freq=True, method=ls_method)
        np.testing.assert_array_equal(ps.frequency, want.frequency)
        np.testing.assert_array_equal(ps.power, want.power)
        np.testing.assert_array_equal(ps.detrended_lc[0], tg)
        np.testing.assert_array_equal(ps.detrended_lc[1], fg)


# ---------------------------------------------------------------------------------------------- the fit, raw
def poly_normalise(hip, ts, fs, order):
    import torch
    lib = hip.load()
    S = len(ts)
    off_h = _off([len(t) for t in ts])
    off, t, f = _dev(off_h), _dev(np.concatenate(ts), np.float64), _dev(np.concatenate(fs), np.float64)
    out = torch.empty_like(f)
    info = torch.empty(S, dtype=torch.int32, device="cuda")
    hip.check(lib.gf_poly_normalise(S, hip.ptr(off), hip.ptr(t), hip.ptr(f), order, hip.ptr(out), hip.ptr(info),
                                    hip.stream_handle()), "gf_poly_normalise")
    out_h = out.cpu().numpy()
    return [out_h[off_h[s]:off_h[s + 1]] for s in range(S)], info.cpu().numpy()


def test_a_non_positive_pivot_marks_its_segment_alone(hip):
    rng = np.random.default_rng(2)
    ts = [100.0 + np.arange(n) * 0.02 for n in (300, 9, 1025)]
    fs = [1e4 * (1 + 0.01 * rng.standard_normal(len(t))) for t in ts]
    good, info = poly_normalise(hip, ts, fs, 8)
    assert np.all(info == 0) and all(np.all(np.isfinite(g)) for g in good)
    planted = list(ts)
    planted[1] = np.full(9, 2454964.5)              # nine coincident stamps: u = 0, P_1 = 0, the second pivot is 0
    got, info = poly_normalise(hip, planted, fs, 8)
    assert info[0] == 0 and info[1] == 2 and info[2] == 0
    assert np.all(np.isnan(got[1]))
    np.testing.assert_array_equal(got[0], good[0])
    np.testing.assert_array_equal(got[2], good[2])
    got0, info0 = poly_normalise(hip, planted, fs, 0)    # order 0 needs no spread in time
    assert np.all(info0 == 0)
    np.testing.assert_allclose(got0[1], fs[1] / fs[1].mean(), rtol=1e-14)
