"""GPU: gadfly_amd.interpolate_missing_data_batch and the segmented gap-fill entry points (gf_interp_plan_seg,
gf_interp_fill_seg) against gadfly_amd.interpolate_missing_data on each series -- the function that
tests/test_gpu_interp.py pins to the reference's own stored outputs.  Every comparison is np.array_equal on times and
fluxes: a series' bits must not depend on whether it is filled alone or inside a batch.
"""
import collections

import numpy as np
import pytest

from tests.interp_cases import make_case

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048            # points per workgroup of the scan (SCAN_PER_WG), 256 per workgroup of the fill
# in this order the segments start at 0, 2048 (on a scan tile), 4097 (just past one), 6144 (on one), 6400 and 6912
# (on a tile of the fill), 6655 (just before one), 6914 and 6917 (inside)
LENGTHS = [2048, 2049, 2047, 256, 255, 257, 2, 3, 4097]
BKJD, JD = 131.5, 2454833.0
SHORT, LONG = 58.85 / 86400.0, 29.4 / 1440.0
PATTERNS = ["none", "every", "third", "first_5000", "last_5000"]


def same(got, want):
    return (got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and got[0].dtype == want[0].dtype == np.float64 and got[1].dtype == np.float64)


def single(t, f, **kw):
    import gadfly_amd
    return gadfly_amd.interpolate_missing_data(t, f, **kw)


def batch(ts, fs, **kw):
    import gadfly_amd
    return gadfly_amd.interpolate_missing_data_batch(ts, fs, **kw)


def shaped(n, pattern, t0, cad, seed):
    """n points on the grid t0 + m cad: no gap, one missing cadence in every interval, one in every third, or a
    single gap of 5000 cadences in the first or in the last interval."""
    step = np.ones(n - 1, dtype=np.int64)
    if pattern == "every":
        step[:] = 2
    elif pattern == "third":
        step[::3] = 2
    elif pattern == "first_5000":
        step[0] = 5001
    elif pattern == "last_5000":
        step[-1] = 5001
    m = np.concatenate([[0], np.cumsum(step)])
    rng = np.random.default_rng(seed)
    return t0 + m * cad, 1e4 + rng.standard_normal(n)


# ------------------------------------------------------------------------------------------- 1. the stored cases
@pytest.fixture(scope="module")
def plain_cases(hip):
    names = ["uniform_300", "complete_2049", "holes_5000", "jitter_5000"]
    series = [make_case(name)[:2] for name in names]
    return names, series, [single(t, f) for t, f in series]


@pytest.fixture(scope="module")
def cadence_cases(hip):
    names = ["uniform_300_cad", "holes_5000_cad", "jitter_5000_cad", "drift_10_cad", "drift_20000_cad"]
    series = [make_case(name) for name in names]
    return names, series, [single(t, f, **kw) for t, f, kw in series]


def test_stored_cases_without_cadence_numbers(plain_cases):
    names, series, want = plain_cases
    got = batch([t for t, _ in series], [f for _, f in series])
    assert len(got) == len(names)
    for name, g, w in zip(names, got, want):
        assert same(g, w), name


def test_stored_cases_with_cadence_numbers(cadence_cases):
    names, series, want = cadence_cases
    got = batch([t for t, _, _ in series], [f for _, f, _ in series], cadences=[kw["cadences"] for _, _, kw in series])
    for name, g, w in zip(names, got, want):
        assert same(g, w), name
    # the drifting grids put missing cadences past their neighbours' stamps: the case must not be a plain merge
    t, _, kw = series[names.index("drift_10_cad")]
    assert len(got[names.index("drift_10_cad")][0]) == kw["cadences"][-1] - kw["cadences"][0] + 1


# ---------------------------------------------------------------------------- 2. segment boundaries and scan tiles
@pytest.mark.parametrize("shift", range(len(PATTERNS)))
def test_boundaries_inside_on_and_past_a_tile(hip, shift):
    """Every length with every gap shape over the five cases; neighbours alternate between a BKJD axis at 29.4 min
    and a JD axis at 58.85 s, so a segment that read its neighbour's first time or cadence would be far off."""
    series = []
    for k, n in enumerate(LENGTHS):
        t0, cad = ((BKJD, LONG), (JD, SHORT))[k % 2]
        series.append(shaped(n, PATTERNS[(k + shift) % len(PATTERNS)], t0 + 3.0 * k, cad, seed=100 * shift + k))
    off = np.cumsum([0] + [len(t) for t, _ in series])[1:-1]
    assert {0, 1} < {int(o) % SCAN_TILE for o in off} and {0, 255} < {int(o) % 256 for o in off}
    want = [single(t, f) for t, f in series]
    got = batch([t for t, _ in series], [f for _, f in series])
    filled = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (LENGTHS[k], PATTERNS[(k + shift) % len(PATTERNS)])
        filled += len(g[0]) - len(series[k][0])
    assert filled >= 5000                   # at least one long gap was filled in every case


# ------------------------------------------------------------------------- 3. S = 1, permutations, repeatability
def test_one_series_permutations_and_repeats(plain_cases):
    names, series, want = plain_cases
    for (t, f), w in zip(series, want):
        (g,) = batch([t], [f])
        assert same(g, w)
    order = [2, 0, 3, 1]
    got = batch([series[k][0] for k in order], [series[k][1] for k in order])
    for k, g in zip(order, got):
        assert same(g, want[k]), names[k]
    again = batch([series[k][0] for k in order], [series[k][1] for k in order])
    for a, g in zip(again, got):
        assert same(a, g)


# -------------------------------------------------------------------------------------------- 4. device tensors
def test_device_inputs_and_outputs(plain_cases, cadence_cases):
    import torch
    for names, series, want, with_cad in (plain_cases + (False,), cadence_cases + (True,)):
        ts = [torch.as_tensor(s[0], device="cuda") for s in series]
        fs = [torch.as_tensor(s[1], device="cuda") for s in series]
        kw = {"cadences": [s[2]["cadences"] for s in series]} if with_cad else {}
        got = batch(ts, fs, return_device=True, **kw)
        storages = set()
        for name, (t, f), w in zip(names, got, want):
            assert t.is_cuda and f.is_cuda and t.dtype == f.dtype == torch.float64
            assert same((t.cpu().numpy(), f.cpu().numpy()), w), name
            storages |= {t.untyped_storage().data_ptr(), f.untyped_storage().data_ptr()}
        assert len(storages) == 1
        host = batch(ts, fs, **kw)                      # device in, numpy out
        for name, g, w in zip(names, host, want):
            assert same(g, w), name


def test_device_inputs_are_refused_after_the_read_back(hip):
    import torch
    t, f = shaped(300, "third", BKJD, LONG, seed=1)
    flat = torch.full((5,), 7.0, dtype=torch.float64, device="cuda")        # median spacing 0
    with pytest.raises(ValueError, match="series 1: the cadence is not a positive finite number"):
        batch([torch.as_tensor(t, device="cuda"), flat], [torch.as_tensor(f, device="cuda"), flat])
    bad = torch.as_tensor(np.array([0.0, 1.0, np.inf]), device="cuda")
    with pytest.raises(ValueError, match="times must be finite"):
        batch([bad], [bad])


# ------------------------------------------------------------------------------------- 5. the raw entry points
GUARD = 8
WORD, VALUE = -7777, -1.25e300


class Guarded:
    """A device buffer of n elements filled with a sentinel, GUARD more of it in front and behind."""

    def __init__(self, n, dtype, fill):
        import torch
        self.n, self.fill = n, fill
        self.all = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.use = self.all[GUARD:GUARD + n]

    def intact(self):
        h = self.all.cpu().numpy()
        return bool(np.all(h[:GUARD] == self.fill) and np.all(h[GUARD + self.n:] == self.fill))


def run_raw(hip, segs, dt, which):
    """segs: list of (t, f), possibly of no points.  -> (info, new_off, pieces); asserts what holds for every call"""
    import torch
    lib, p, st = hip.load(), hip.ptr, hip.stream_handle()
    S = len(segs)
    off_h = np.cumsum([0] + [len(t) for t, _ in segs]).astype(np.int64)
    total = int(off_h[-1])
    dev = lambda x, dtype: torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda")      # noqa: E731
    off, dt_d = dev(off_h, np.int64), dev(dt, np.float64)
    t = dev(np.concatenate([s[0] for s in segs]), np.float64)
    f = dev(np.concatenate([s[1] for s in segs]), np.float64)
    w = None if which is None else dev(which, np.uint8)
    words = int(lib.gf_interp_seg_work(total))
    assert words == -(-total // SCAN_TILE)
    plan, new_off = Guarded(total + 1, torch.int64, WORD), Guarded(S + 1, torch.int64, WORD)
    info, work = Guarded(S, torch.int32, WORD), Guarded(words, torch.int64, WORD)
    hip.check(lib.gf_interp_plan_seg(S, total, p(off), p(t), None, p(dt_d), p(w), p(plan.use), p(new_off.use),
                                     p(info.use), p(work.use), st), "gf_interp_plan_seg")
    new_off_h, plan_h = new_off.use.cpu().numpy(), plan.use.cpu().numpy()
    assert all(b.intact() for b in (plan, new_off, info, work))
    assert np.array_equal(new_off_h, plan_h[off_h]) and plan_h[0] == 0
    assert np.all(np.diff(plan_h) >= 1)
    n_out = int(new_off_h[-1])
    t_out, f_out = Guarded(n_out, torch.float64, VALUE), Guarded(n_out, torch.float64, VALUE)
    before = plan.all.clone()
    hip.check(lib.gf_interp_fill_seg(S, total, p(off), p(t), p(f), None, p(dt_d), p(w), p(plan.use), p(t_out.use),
                                     p(f_out.use), st), "gf_interp_fill_seg")
    assert t_out.intact() and f_out.intact() and torch.equal(before, plan.all)
    t_h, f_h = t_out.use.cpu().numpy(), f_out.use.cpu().numpy()
    assert not np.any(t_h == VALUE) and not np.any(f_h == VALUE)        # every output element was written
    pieces = [(t_h[new_off_h[s]:new_off_h[s + 1]], f_h[new_off_h[s]:new_off_h[s + 1]]) for s in range(S)]
    return info.use.cpu().numpy(), new_off_h, pieces


EMPTY = (np.zeros(0), np.zeros(0))


def raw_segments():
    a = shaped(300, "third", BKJD, LONG, seed=11)
    b = shaped(2049, "first_5000", JD, SHORT, seed=12)
    c = shaped(257, "last_5000", BKJD + 400.0, LONG, seed=13)
    d = shaped(2, "none", JD + 9.0, SHORT, seed=14)
    return [a, b, c, d]


def cadence_of(seg):
    return float(np.median(np.diff(seg[0]))) if len(seg[0]) > 1 else np.nan


def test_raw_empty_segments(hip):
    a, b, c, d = raw_segments()
    segs = [a, EMPTY, b, EMPTY, EMPTY, c, d, EMPTY]
    info, new_off, pieces = run_raw(hip, segs, [cadence_of(s) for s in segs], None)
    assert not info.any()
    for s, seg in enumerate(segs):
        if len(seg[0]) == 0:
            assert new_off[s] == new_off[s + 1]
        else:
            assert same(pieces[s], single(*seg)), s
    assert len(pieces[2][0]) == 2049 + 5000


def test_raw_which_mask_copies_the_unselected(hip):
    segs = raw_segments()
    dt = [np.nan, cadence_of(segs[1]), np.nan, cadence_of(segs[3])]
    info, new_off, pieces = run_raw(hip, segs, dt, [0, 1, 0, 1])
    assert not info.any()
    for s in (0, 2):
        assert same(pieces[s], segs[s])
    for s in (1, 3):
        assert same(pieces[s], single(*segs[s]))
    # and with an empty segment in the middle and at the end of the same mask
    segs = segs[:2] + [EMPTY] + segs[2:] + [EMPTY]
    info, new_off, pieces = run_raw(hip, segs, [np.nan, dt[1], np.nan, np.nan, dt[3], np.nan], [0, 1, 1, 0, 1, 1])
    assert not info.any()
    assert same(pieces[0], segs[0]) and same(pieces[3], segs[3])
    assert same(pieces[1], single(*segs[1])) and same(pieces[4], single(*segs[4]))


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_raw_unusable_cadence_flags_its_own_segment(hip, bad):
    segs = raw_segments()
    dt = [cadence_of(s) for s in segs]
    dt[2] = bad
    info, new_off, pieces = run_raw(hip, segs, dt, None)
    assert info.tolist() == [0, 0, 1, 0]
    assert same(pieces[2], segs[2])
    for s in (0, 1, 3):
        assert same(pieces[s], single(*segs[s]))


# ------------------------------------------------------------------- 6. prepare_quarters_batch fills in two calls
class Counting:
    def __init__(self, lib):
        self.lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def quarter(rng, n, start, cad=LONG):
    keep = rng.random(n) > 0.1
    keep[[0, -1]] = True
    t = (start + np.arange(n) * cad)[keep]
    f = 2.3e5 * (1 + 0.01 * (t - t.mean())) * (1 + 3e-4 * rng.standard_normal(t.size))
    f[rng.choice(t.size, 3, replace=False)] = np.nan
    return t, f


def test_prepare_quarters_batch_fills_in_two_calls(hip, monkeypatch):
    import gadfly_amd
    from gadfly_amd import detrend
    rng = np.random.default_rng(6)
    stars = [[quarter(rng, 300, BKJD + 10.0 * b + 7.0 * q) for q in range(nq)] for b, nq in enumerate((1, 2, 4))]
    want = gadfly_amd.prepare_quarters_batch(stars, fill=True)
    proxy = Counting(hip.load())
    monkeypatch.setattr(detrend._lib, "load", lambda: proxy)
    got = gadfly_amd.prepare_quarters_batch(stars, fill=True)
    calls = proxy.calls
    assert calls["gf_sigma_clip"] == 1                      # the proxy is the object the call went through
    assert calls["gf_interp_plan"] == 0 and calls["gf_interp_fill"] == 0
    assert 1 <= calls["gf_interp_plan_seg"] <= 2 and 1 <= calls["gf_interp_fill_seg"] <= 2
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2]
    for (t, f, cadence), star in zip(got, stars):
        assert 0.4 * cadence < np.diff(t).min() and np.diff(t).max() < 1.6 * cadence     # no cadence is missing
        assert star[0][0][0] <= t[0] and t[-1] <= star[-1][0][-1]       # (a NaN or clipped row may end a quarter)
        assert len(t) > sum(len(q[0]) for q in star)
