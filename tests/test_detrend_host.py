"""CPU: the numpy restatement of prepare_quarters (tests/detrend_ref.py) against the oracle's stitch_quarters and
against 80-bit arithmetic; the host-side ValueErrors of gadfly_amd.prepare_quarters; the argument checks of the
segmented entry points (status and message), none of which launches anything."""
import numpy as np
import pytest

import gadfly_amd
from gadfly_amd import _lib
from oracle import interp_ref
from tests import detrend_ref

FLUX_BAR_PPM = 1e-6         # results are 1e6 (r - 1), r of order one: 1e-12 in r


def make_quarter(rng, n, t0, cad, missing=0.1, trend=0.02):
    t = t0 + np.arange(n) * cad
    keep = rng.random(n) > missing
    keep[[0, -1]] = True
    t = t[keep]
    x = (t - t.mean()) / (t.max() - t.min())
    f = 2.3e5 * (1 + trend * (x + 0.7 * x ** 2 - 1.3 * x ** 3)) * (1 + 3e-4 * rng.standard_normal(t.size))
    return t, f


@pytest.mark.parametrize("t0", [131.5, 2454964.5])
@pytest.mark.parametrize("order", [0, 3, 8])
def test_restatement_equals_stitch_quarters_on_clean_input(t0, order):
    rng = np.random.default_rng(7)
    quarters = [make_quarter(rng, n, t0 + 95.0 * q, 0.0204) for q, n in enumerate((900, 300, 1500))]
    details = []
    t, f, cad = detrend_ref.prepare_quarters(quarters, order, details=details)
    assert all(mask.all() for mask, _, _ in details)            # clean: the clip removes nothing
    rt, rf, rcad = interp_ref.stitch_quarters(quarters, order)
    np.testing.assert_array_equal(t, rt)
    assert cad == rcad
    print("legendre float64 against numpy polyfit: %.2e ppm" % np.abs(f - rf).max())
    assert np.abs(f - rf).max() <= FLUX_BAR_PPM
    tn, fn, _ = detrend_ref.prepare_quarters(quarters, order, normaliser="numpy")
    np.testing.assert_array_equal(fn, rf)
    # in ppm already: only the clip and the fills act
    tp, fp, _ = detrend_ref.prepare_quarters(quarters, order, in_ppm=True)
    rtp, rfp, _ = interp_ref.stitch_quarters(quarters, order, in_ppm=True)
    np.testing.assert_array_equal(tp, rtp)
    np.testing.assert_array_equal(fp, rfp)


@pytest.mark.parametrize("n,t0,cad", [(4500, 131.5, 0.0204), (130000, 2454964.5, 1 / 1440.0),
                                      (300, 2454964.5, 0.0204), (40, 131.5, 0.0204)])
@pytest.mark.parametrize("order", [1, 3, 5, 8])
def test_float64_legendre_route_against_80_bit(n, t0, cad, order):
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(3 + n + order)
    t, f = make_quarter(rng, n, t0, cad)
    want = detrend_ref.normalise_longdouble(t, f, order)
    got = detrend_ref.normalise_legendre(t, f, order)
    ref = detrend_ref.normalise_numpy(t, f, order)
    P = detrend_ref.legendre_basis(t, order)
    cond = np.linalg.cond(P.T @ P)
    print("n=%d order=%d: legendre %.2e ppm, numpy %.2e ppm from 80-bit; cond %.1f" % (
        n, order, np.abs(got - want).max(), np.abs(ref - want).max(), cond))
    assert cond <= 2 * (2 * order + 1)      # the continuous basis: diag(2 / (2 j + 1)), i.e. 2 order + 1
    assert np.abs(got - want).max() <= FLUX_BAR_PPM / 10
    assert np.abs(ref - want).max() <= FLUX_BAR_PPM / 10


def test_clip_restatement_rounds_cap_and_asymmetry():
    rng = np.random.default_rng(11)
    f = 100.0 + rng.standard_normal(2000)
    f[::97] += 40.0
    f[5] = np.nan
    mask, rounds, margin = detrend_ref.sigma_clip(f)
    assert not mask[5] and not mask[::97].any() and mask.sum() >= 2000 - 30 and 2 <= rounds <= 5 and margin > 0
    capped, r1, _ = detrend_ref.sigma_clip(f, maxiters=1)
    assert r1 == 1 and capped.sum() >= mask.sum()
    free, r_free, _ = detrend_ref.sigma_clip(f, maxiters=None)
    assert r_free >= rounds and free.sum() <= mask.sum()
    upper, _, _ = detrend_ref.sigma_clip(f, sigma_lower=1e9, sigma_upper=5.0)
    np.testing.assert_array_equal(upper, mask)                  # all outliers lie above
    off, r0, _ = detrend_ref.sigma_clip(f, sigma=None)
    assert r0 == 0 and off.sum() == 1999


def _clean(n=50, t0=100.0):
    return t0 + np.arange(n) * 0.02, 1e4 + np.arange(n) * 0.1


@pytest.mark.parametrize("kwargs,match", [
    (dict(detrend_poly_order=9), "detrend_poly_order"),
    (dict(detrend_poly_order=-1), "detrend_poly_order"),
    (dict(detrend_poly_order=2.5), "detrend_poly_order"),
    (dict(sigma=0.0), "sigma_lower"),
    (dict(sigma=-3.0), "sigma_lower"),
    (dict(sigma_upper=0.0), "sigma_upper"),
    (dict(sigma=None, sigma_lower=3.0), "sigma_upper"),
    (dict(maxiters=0), "maxiters"),
    (dict(maxiters=-2), "maxiters"),
])
def test_options_out_of_range_raise_before_any_device_work(kwargs, match):
    with pytest.raises(ValueError, match=match):
        gadfly_amd.prepare_quarters([_clean()], **kwargs)


def test_input_errors_name_star_and_quarter():
    t, f = _clean()
    tb = t.copy()
    tb[10] = tb[9]
    with pytest.raises(ValueError, match="star 0, quarter 1: times must be strictly increasing"):
        gadfly_amd.prepare_quarters([(t, f), (tb + 10.0, f)])
    tn = t.copy()
    tn[10] = np.nan                                             # checked over the finite rows only
    fn = f.copy()
    fn[10] = np.nan
    for tq, fq in ((tn, f), (tb, fn)):                          # (passes the order check, then:)
        with pytest.raises(ValueError, match="star 1, quarter 1: starts at"):
            gadfly_amd.prepare_quarters_batch([[(t, f)], [(tq, fq), (t, f)]])
    t2 = np.concatenate([[t[-1]], t[-1] + 0.02 * np.arange(1, 50)])         # its first stamp is the previous last one
    with pytest.raises(ValueError, match="star 0, quarter 1: starts at .* before the previous quarter ends"):
        gadfly_amd.prepare_quarters([(t, f), (t2, f)])
    with pytest.raises(ValueError, match="star 2, quarter 0: 3 finite points, 4 are needed"):
        gadfly_amd.prepare_quarters_batch([[(t, f)], [(t, f)], [(t[:3], f[:3])]])
    f2 = f.copy()
    f2[2:] = np.nan
    with pytest.raises(ValueError, match="star 0, quarter 0: 2 finite points, 9 are needed"):
        gadfly_amd.prepare_quarters([(t, f2)], detrend_poly_order=8)
    with pytest.raises(ValueError, match="star 0, quarter 0: 1 finite points, 2 are needed"):
        gadfly_amd.prepare_quarters([(t[:1], f[:1])], detrend_poly_order=0)
    with pytest.raises(ValueError, match="dimension mismatch"):
        gadfly_amd.prepare_quarters([(t, f[:-1])])
    with pytest.raises(ValueError, match="no quarters"):
        gadfly_amd.prepare_quarters([])
    with pytest.raises(ValueError, match="no stars"):
        gadfly_amd.prepare_quarters_batch([])


def test_from_quarters_checks_its_method_and_keeps_from_light_curve_closed():
    with pytest.raises(ValueError, match="must be one of"):
        gadfly_amd.PowerSpectrum.from_quarters([_clean()], method="welch")
    with pytest.raises(TypeError):
        gadfly_amd.PowerSpectrum.from_quarters([_clean()], fill=False)
    import types
    lc = types.SimpleNamespace(time=np.arange(10) / 1440.0, flux=np.zeros(10))
    with pytest.raises(NotImplementedError, match="from_quarters"):
        gadfly_amd.PowerSpectrum.from_light_curve(lc, detrend=True)


Z, D = None, 4096            # NULL, and a non-null value that is never dereferenced: every case returns before a launch
CASES = [
    ("gf_seg_median", (0, D, D, Z, 0, D, Z), "gf_seg_median: no segments (S=0)"),
    ("gf_seg_median", (2, Z, D, Z, 0, D, Z), "gf_seg_median: null pointer"),
    ("gf_seg_median", (2, D, Z, Z, 0, D, Z), "gf_seg_median: null pointer"),
    ("gf_seg_median", (2, D, D, Z, 0, Z, Z), "gf_seg_median: null pointer"),
    ("gf_seg_median", (2, D, D, Z, 2, D, Z), "gf_seg_median: drop_last=2 must be 0 or 1"),
    ("gf_sigma_clip", (-1, D, Z, D, 5.0, 5.0, 5, D, D, D, Z), "gf_sigma_clip: no segments (S=-1)"),
    ("gf_sigma_clip", (1, D, Z, Z, 5.0, 5.0, 5, D, D, D, Z), "gf_sigma_clip: null pointer"),
    ("gf_sigma_clip", (1, D, Z, D, 5.0, 5.0, 5, Z, D, D, Z), "gf_sigma_clip: null pointer"),
    ("gf_sigma_clip", (1, D, Z, D, 5.0, 5.0, 5, D, Z, D, Z), "gf_sigma_clip: null pointer"),
    ("gf_sigma_clip", (1, D, Z, D, 5.0, 5.0, 5, D, D, Z, Z), "gf_sigma_clip: null pointer"),
    ("gf_sigma_clip", (1, D, Z, D, 0.0, 5.0, 5, D, D, D, Z),
     "gf_sigma_clip: sigma_lower=0 and sigma_upper=5 must be positive"),
    ("gf_sigma_clip", (1, D, Z, D, 5.0, float("nan"), -1, D, D, D, Z),
     "gf_sigma_clip: sigma_lower=5 and sigma_upper=nan must be positive"),
    ("gf_seg_compact", (0, D, D, D, D, D, D, D, Z), "gf_seg_compact: no segments (S=0)"),
    ("gf_seg_compact", (3, D, Z, D, D, D, D, D, Z), "gf_seg_compact: null pointer"),
    ("gf_seg_compact", (3, D, D, D, D, Z, D, D, Z), "gf_seg_compact: null pointer"),
    ("gf_seg_compact", (3, D, D, D, D, D, D, Z, Z), "gf_seg_compact: null pointer"),
    ("gf_seg_diff", (0, D, D, D, Z), "gf_seg_diff: no segments (S=0)"),
    ("gf_seg_diff", (1, D, D, Z, Z), "gf_seg_diff: null pointer"),
    ("gf_poly_normalise", (0, D, D, D, 3, D, D, Z), "gf_poly_normalise: no segments (S=0)"),
    ("gf_poly_normalise", (1, D, D, D, 9, D, D, Z), "gf_poly_normalise: order=9 must be in 0..8"),
    ("gf_poly_normalise", (1, D, D, D, -1, D, D, Z), "gf_poly_normalise: order=-1 must be in 0..8"),
    ("gf_poly_normalise", (1, D, D, Z, 3, D, D, Z), "gf_poly_normalise: null pointer"),
    ("gf_poly_normalise", (1, D, D, D, 3, D, Z, Z), "gf_poly_normalise: null pointer"),
    ("gf_seg_ppm", (0, D, D, D, D, Z), "gf_seg_ppm: no segments (S=0)"),
    ("gf_seg_ppm", (1, D, D, Z, D, Z), "gf_seg_ppm: null pointer"),
]


@pytest.mark.parametrize("name,args,message", CASES)
def test_entry_points_refuse_bad_arguments(name, args, message):
    lib = _lib.load()
    assert len(args) == len(_lib.SIGNATURES[name][1])
    assert getattr(lib, name)(*args) == -1
    assert lib.gf_last_error().decode() == message


def test_every_segmented_entry_point_has_a_case_and_the_unit_is_built():
    names = {"gf_seg_median", "gf_sigma_clip", "gf_seg_compact", "gf_seg_diff", "gf_poly_normalise", "gf_seg_ppm"}
    assert {c[0] for c in CASES} == names <= set(_lib.SIGNATURES)
    assert any(src.endswith("gadfly_detrend.hip") for src in _lib.SOURCES)
    assert _lib.GF_DETREND_MAX_ORDER == 8
