"""GPU: the fused sweeps through their raw C entry points, streamed mode, row by row (tests/fused_cases.py):
gf_loglike_fused (pivots d and z = L^-1 y) and gf_sample_fused (d and the draw L D^1/2 eps) against the float64 C oracle
at 1e-10 of the largest reference entry of the array -- every width 1..63 by column, every Jc = 1..31 lane-tiled, the
11 wide shapes on both sides of every dispatch line, every scaling block against every generator period on an axis
that takes every branch of the row generator, the block rule at its limit for both spans, rows that reset on their
own, tiles down to a last tile of one row, series of one to three rows, batch strides, diag = NULL, a failing pivot in
the first or a later tile, and a time axis 2e5 from zero.  t, y / eps and diag end in three NaN elements; every output
is one problem too long and pre-filled with a sentinel that must survive."""
import numpy as np
import pytest
import torch

from tests import fused_cases as fc
from tests import sweep_cases as sc
from tests import sweep_dev as sd

pytestmark = pytest.mark.gpu

AUTO, COLUMN, TILED, LONG_SPAN = 0, 1, 2, 0x200          # the GF_SWEEP_* constants of include/gadfly_hip.h
TOL = fc.TOL
PAD = 3                                                     # elements t, y / eps, diag must be readable past the end


def _variants(s):
    """The sweeps a structure can run: by column always, lane-tiled for Jr = 0; the wide kernels ignore the variant."""
    if s[0] + 2 * s[1] > 63:
        return (AUTO,)
    return (COLUMN, TILED) if s[0] == 0 else (COLUMN,)


def _padded(x, n):
    """(n,) or (B, n) on the device as rows of n + PAD elements, the pads NaN."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, n)
    buf = np.full((x.shape[0], n + PAD), np.nan)
    buf[:, :n] = x
    return sd.dev(buf.reshape(-1))


def _only(prob, b):
    """Problem b of a fused_cases.problem as a batch of one."""
    out = dict(prob, B=1)
    for k in ("real", "comp"):
        out[k] = prob[k][:, b:b + 1]
    for k in ("diag", "y", "eps", "diag_add", "cmax"):
        out[k] = prob[k][b:b + 1]
    return out


def _sweep(hip, prob, t, t_bs, diag, diag_bs, block, period, variant, tiles=None, sample=False, eps=None):
    """gf_loglike_fused (z = L^-1 y of prob["y"]) or gf_sample_fused (the draw from ``eps``, default prob["eps"]) on
    the coefficients of a fused_cases.problem: t (n,) with t_bs = 0 or (B, n) with t_bs = n + 3, diag likewise or None.
    tiles: None = one call; a tile length (the remainder comes last); or a list of (n_first, rows).  The state is
    zeroed before the first tile only.  Returns (d, z or draw, info): (B, n), (B, n), (B,) on the host; rows that no
    call wrote hold sweep_dev.SENTINEL."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, B = prob["Jr"], prob["Jc"], prob["B"]
    t = np.asarray(t)
    n = t.shape[-1]
    assert t_bs == (0 if t.ndim == 1 else n + PAD) and (diag is None or diag_bs == (0 if diag.ndim == 1 else n + PAD))
    real, comp = sd.dev(prob["real"]), sd.dev(prob["comp"])
    da, cm = sd.dev(prob["diag_add"]), sd.dev(prob["cmax"])
    td = _padded(t, n)
    dd = None if diag is None else _padded(diag, n)
    yd = _padded((prob["eps"] if eps is None else eps) if sample else prob["y"], n)
    bs = n + PAD
    wide = Jr + 2 * Jc > 63
    size = int(lib.gf_fused_state_size(Jr, Jc)) if wide else 64 * 64
    assert size > 0
    S = sd.zeroed_with_sentinel(B * size, size)
    F = None if wide else sd.zeroed_with_sentinel(B * 64, 64)
    info = sd.info_with_sentinel(B)
    out = sd.sentinel((B + 1) * bs) if sample else None
    if tiles is None:
        tiles = [(0, n)]
    elif isinstance(tiles, int):
        tiles = [(a, min(tiles, n - a)) for a in range(0, n, tiles)]
    fn = lib.gf_sample_fused if sample else lib.gf_loglike_fused
    parts = []
    for n0, rows in tiles:
        dt, zt = sd.sentinel((B + 1) * rows), sd.sentinel((B + 1) * rows)
        rc = fn(B, rows, n0, Jr, Jc, block, period, variant, p(real[0]), p(real[1]), p(comp[0]), p(comp[1]),
                p(comp[2]), p(comp[3]), p(da), p(cm), p(td), t_bs, p(dd), diag_bs, p(yd), bs, p(dt),
                p(out) if sample else p(zt), p(S), p(F), p(info), None)
        hip.check(rc, "gf_sample_fused" if sample else "gf_loglike_fused")
        parts.append((n0, rows, dt, zt))
    torch.cuda.synchronize()
    d, z = np.full((B, n), sd.SENTINEL), np.full((B, n), sd.SENTINEL)
    for n0, rows, dt, zt in parts:
        d[:, n0:n0 + rows] = sd.take(dt, B * rows, "d").reshape(B, rows)
        zh = sd.take(zt, 0 if sample else B * rows, "z")    # the sampling sweep leaves the tile-local z alone
        if not sample:
            z[:, n0:n0 + rows] = zh.reshape(B, rows)
    if sample:
        oh = sd.take(out, B * bs, "out").reshape(B, bs)
        assert np.all(oh[:, n:] == sd.SENTINEL), "out: written between the problems"
        z = oh[:, :n].copy()
    sd.take(S, B * size, "S_state")
    if F is not None:
        sd.take(F, B * 64, "F_state")
    return d, z, sd.take_info(info, B, "info")


def _run(hip, prob, t, block, period, variant, diag="own", **kw):
    """_sweep with the axis and the diagonal in their usual layouts: t (n,) shared or (B, n) own; diag "own" (B, n),
    "shared" (n,), "none"."""
    t = np.asarray(t)
    dg = fc.device_diag(prob, diag)
    return _sweep(hip, prob, t, 0 if t.ndim == 1 else t.shape[-1] + PAD, dg,
                  0 if dg is None or dg.ndim == 1 else dg.shape[-1] + PAD, block, period, variant, **kw)


def _against(got, refs, sample, what, worst):
    """d and z (or the draw) of every problem against the oracle's rows at TOL; every figure goes to ``worst`` first."""
    d, z, info = got
    assert not np.any(info), (what, info)
    for key, x in (("d", d), ("draw" if sample else "z", z)):
        errs = [sc.relerr(x[b], r[key]) for b, r in enumerate(refs)]
        worst.extend(errs)
        assert max(errs) <= TOL, (what, key, errs)


def _report(name, worst):
    print(f"{name}: {len(worst)} arrays, worst error {max(worst):.1e}")


# ---- 1. every narrow width -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", fc.NARROW, ids=fc.ident)
def test_every_narrow_width(hip, s):
    """B = 3 on the composite axis at block 64, periods 1 and 16, both entry points: k_factor3<R> and its sampling form
    by column at every W = 1..63; for Jr = 0 also k_factor7<R, false> and its sampling form; GF_SWEEP_AUTO gives the
    lane-tiled sweep's bits for Jr = 0 and the column sweep's elsewhere; GF_SWEEP_TILED with Jr > 0 is an error."""
    prob, refs, t = fc.problem(*s), fc.rows(*s), fc.composite_axis()
    worst = []
    for period in (1, 16):
        for sample in (False, True):
            got = {v: _run(hip, prob, t, 64, period, v, sample=sample) for v in (AUTO,) + _variants(s)}
            for v in _variants(s):
                _against(got[v], refs, sample, (period, sample, v), worst)
            same = got[TILED] if s[0] == 0 else got[COLUMN]
            assert all(np.array_equal(a, b) for a, b in zip(got[AUTO], same)), (period, sample)
    if s[0] > 0:
        for sample in (False, True):
            with pytest.raises(hip.GadflyHipError, match="GF_SWEEP_TILED"):
                _run(hip, prob, t, 64, 16, TILED, sample=sample)
    _report(fc.ident(s), worst)


# ---- 2. every wide shape ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", fc.WIDE, ids=fc.ident)
def test_every_wide_shape(hip, s):
    """B = 2 on the composite axis at block 64, periods 1 and 16, both entry points: k_factorw<TR, NW> and its sampling
    form on both sides of every line of dispatch_factorw; the state is gf_fused_state_size doubles per problem,
    F_state = NULL."""
    prob, refs, t = fc.problem(*s, B=2), fc.rows(*s, B=2), fc.composite_axis()
    worst = []
    for period in (1, 16):
        for sample in (False, True):
            _against(_run(hip, prob, t, 64, period, AUTO, sample=sample), refs, sample, (period, sample), worst)
    _report(fc.ident(s), worst)


def test_a_real_term_beyond_63_columns_is_an_error(hip):
    lib = hip.load()
    assert lib.gf_fused_supported(1, 31) == 1 and lib.gf_fused_supported(1, 32) == 0
    assert lib.gf_fused_supported(0, 88) == 1 and lib.gf_fused_supported(0, 89) == 0
    assert lib.gf_fused_state_size(1, 32) == -1
    prob = fc.problem(1, 32, B=2)
    for sample in (False, True):
        with pytest.raises(hip.GadflyHipError, match="unsupported"):
            _refused(hip, prob, sample)


def _refused(hip, prob, sample):
    """The raw call with W = 65, Jr = 1 and buffers of the narrow sizes: it must return before it touches any."""
    lib, p = hip.load(), hip.ptr
    n, B = prob["N"], prob["B"]
    real, comp = sd.dev(prob["real"]), sd.dev(prob["comp"])
    da, cm = sd.dev(prob["diag_add"]), sd.dev(prob["cmax"])
    td, yd = _padded(fc.composite_axis(), n), _padded(prob["y"], n)
    d, z = sd.sentinel((B + 1) * (n + PAD)), sd.sentinel((B + 1) * (n + PAD))
    S, F, info = sd.zeroed_with_sentinel(B * 4096, 4096), sd.zeroed_with_sentinel(B * 64, 64), sd.info_with_sentinel(B)
    fn = lib.gf_sample_fused if sample else lib.gf_loglike_fused
    rc = fn(B, n, 0, prob["Jr"], prob["Jc"], 64, 16, AUTO, p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]),
            p(comp[3]), p(da), p(cm), p(td), 0, None, 0, p(yd), n + PAD, p(d), p(z), p(S), p(F), p(info), None)
    torch.cuda.synchronize()
    sd.take(d, 0, "d")
    sd.take(z, 0, "z")
    hip.check(rc, "fused sweep")


# ---- 3. block x period -----------------------------------------------------------------------------------------------

GRID_CASES = [(s, v) for s in fc.GRID for v in _variants(s)]
GRID_IDS = [f"{fc.ident(s)}-{('auto', 'column', 'tiled')[v]}" for s, v in GRID_CASES]


@pytest.mark.parametrize("s,variant", GRID_CASES, ids=GRID_IDS)
def test_block_times_period_grid(hip, s, variant):
    """Every scaling block 1..64 against every generator period 1..64 on the composite axis (49 pairs): d and z; the
    draw on the seven pairs with block = period."""
    prob, refs, t = fc.problem(*s), fc.rows(*s), fc.composite_axis()
    worst = []
    for block in fc.BLOCKS:
        for period in fc.PERIODS:
            _against(_run(hip, prob, t, block, period, variant), refs, False, (block, period), worst)
        _against(_run(hip, prob, t, block, block, variant, sample=True), refs, True, (block, block), worst)
    _report(f"{fc.ident(s)} variant {variant}", worst)


def test_scaled_spans_are_the_ones_the_host_helper_assumes(hip):
    lib = hip.load()
    assert lib.gf_scaled_span(0) == fc.SPAN == 28.0 and lib.gf_scaled_span(1) == fc.SPAN_LONG == 128.0


# ---- 4. the block rule at its limit ----------------------------------------------------------------------------------

@pytest.mark.parametrize("s", fc.GRID, ids=fc.ident)
def test_block_rule_at_its_limit(hip, s):
    """Block 64, periods 1 and 64: the composite axis stretched to 0.98 of the rule 1.5 * 63 * cmax * cadence <= span
    for span 28 and, with GF_SWEEP_LONG_SPAN, for span 128 (W <= 63; an error for the wide structure); and the plain
    axis with a regular row at 0.98 and at 1.02 of the gap at which a row resets on its own."""
    prob = fc.problem(*s)
    worst = []
    for variant in _variants(s):
        for period in (1, 64):
            for name in ("stretch28", "gap098", "gap102"):
                got = _run(hip, prob, fc.axis(name, *s), 64, period, variant)
                _against(got, fc.rows(*s, name), False, (name, variant, period), worst)
            t = fc.axis("stretch128", *s)
            if s[0] + 2 * s[1] <= 63:
                got = _run(hip, prob, t, 64, period, variant | LONG_SPAN)
                _against(got, fc.rows(*s, "stretch128"), False, ("stretch128", variant, period), worst)
            else:
                with pytest.raises(hip.GadflyHipError, match="GF_SWEEP_LONG_SPAN"):
                    _run(hip, prob, t, 64, period, variant | LONG_SPAN)
    _report(fc.ident(s), worst)


@pytest.mark.parametrize("s", fc.GRID, ids=fc.ident)
def test_second_order_step_near_its_limit(hip, s):
    """Block 64, periods 16 and 64 on the jitter axis: every rotation step corrects a spacing that is off the cached
    one by 0.78..0.98 of the 2e-6 / wmax up to which RowGen::step does so -- to second order: a first-order step there
    leaves x^2 / 2 = 1.5e-12 per row, all of one sign, over up to 63 rows."""
    prob, refs, t = fc.problem(*s), fc.rows(*s, "jitter"), fc.axis("jitter", *s)
    worst = []
    for variant in _variants(s):
        for period in (16, 64):
            for sample in (False, True):
                _against(_run(hip, prob, t, 64, period, variant, sample=sample), refs, sample,
                         (variant, period, sample), worst)
    _report(fc.ident(s), worst)


# ---- 5. tiles --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", fc.GRID, ids=fc.ident)
def test_streamed_tiles(hip, s):
    """N = 385 at blocks 1, 8 and 64 in tiles of ``block``, 64 and 192 rows through S_state / F_state, the remainder
    last (one row where the tile length divides 384): every row of d, the tile-local z and the draw (by global row,
    stride eps_bs) against the oracle.  An n_first that is no multiple of the block is an error."""
    n = 385
    prob, refs, t = fc.problem(*s, n), fc.rows(*s, "composite", n), fc.composite_axis(n)
    worst = []
    for block in (1, 8, 64):
        for tile in sorted({block, 64, 192}):
            for sample in (False, True):
                _against(_run(hip, prob, t, block, 16, AUTO, tiles=tile, sample=sample), refs, sample,
                         (block, tile, sample), worst)
    for sample in (False, True):
        with pytest.raises(hip.GadflyHipError, match="multiple of block"):
            _run(hip, prob, t, 8, 16, AUTO, tiles=[(0, 4), (4, n - 4)], sample=sample)
    _report(fc.ident(s), worst)


@pytest.mark.parametrize("s", fc.GRID, ids=fc.ident)
def test_series_of_one_two_and_three_rows(hip, s):
    """N = 1, 2, 3 in one call: the sweeps read three elements ahead, into the NaN pads."""
    worst = []
    for n in (1, 2, 3):
        prob, refs, t = fc.problem(*s, n), fc.rows(*s, "composite", n), fc.composite_axis(n)
        for variant in _variants(s):
            for block in (1, 64):
                for sample in (False, True):
                    _against(_run(hip, prob, t, block, 16, variant, sample=sample), refs, sample,
                             (n, variant, block, sample), worst)
    _report(fc.ident(s), worst)


# ---- 6. batch layout -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", fc.LAYOUT, ids=fc.ident)
def test_batch_layout(hip, s):
    """A shared axis (t_bs = 0); own axes t (1 + b / 64) with stride N + 3; diag = NULL; a shared diagonal (diag_bs =
    0) -- d, z and the draw against the oracle, and every problem run alone (B = 1) gives the bits it gives inside the
    batch: one wave owns a problem."""
    prob = fc.problem(*s)
    worst = []
    for name, diag in (("composite", "own"), ("own", "own"), ("composite", "none"), ("composite", "shared")):
        T, refs = fc.axis(name, *s), fc.rows(*s, name, diag=diag)
        for sample in (False, True):
            got = _run(hip, prob, T, 64, 16, AUTO, diag=diag, sample=sample)
            _against(got, refs, sample, (name, diag, sample), worst)
            for b in range(prob["B"]):
                one = _only(prob, b)
                if diag == "shared":
                    one["diag"] = prob["diag"][0:1]
                alone = _run(hip, one, T[b] if T.ndim == 2 else T, 64, 16, AUTO,
                             diag="none" if diag == "none" else "own", sample=sample)
                assert all(np.array_equal(x[0], y[b]) for x, y in zip(alone, got)), (name, diag, sample, b)
    _report(fc.ident(s), worst)


# ---- 7. a failing pivot ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", fc.FAIL_ROWS)
@pytest.mark.parametrize("s", fc.FAIL, ids=fc.ident)
def test_failing_pivot(hip, s, r):
    """B = 2; problem 1's diagonal is -2 amp from row r on (r = 0; 100, inside a tile; 63 and 64, the last and the
    first row of 64-row tiles), in one call and in tiles of 64 rows, both entry points: info[1] is celerite2's 1-based
    global row, the rows in front of r are right, later tiles leave its rows alone, and problem 0 matches the oracle
    on every row."""
    prob, refs, t = fc.problem(*s, B=2), fc.rows(*s, B=2, fail=(1, r)), fc.composite_axis()
    dg = fc.device_diag(prob, "own", fail=(1, r))
    assert refs[1]["info"] == r + 1
    worst = []
    for tiles in (None, 64):
        for sample in (False, True):
            d, z, info = _sweep(hip, prob, t, 0, dg, fc.N + PAD, 64, 16, AUTO, tiles=tiles, sample=sample)
            what = (tiles, sample)
            assert list(info) == [0, r + 1], what
            for key, x in (("d", d), ("draw" if sample else "z", z)):
                errs = [sc.relerr(x[0], refs[0][key])] + ([sc.relerr(x[1, :r], refs[1][key])] if r else [])
                worst.extend(errs)
                assert max(errs) <= TOL, (what, key, errs)
                if tiles:
                    assert np.all(x[1, (r // tiles + 1) * tiles:] == sd.SENTINEL), (what, key)
    _report(f"{fc.ident(s)} r = {r}", worst)


# ---- 8. the far axis -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", fc.FAR, ids=fc.ident)
def test_far_axis(hip, s):
    """128 regular rows at t = 2.1e5 (phases of up to 3e8 rad, rounded to 3e-8 rad row by row as celerite2 rounds
    them), block 64, periods 1, 16 and 64: d, z and the draw against the C oracle ON THAT AXIS at TOL -- the oracle's
    rows on the same spacings near zero lie 5 TOL (d) and 50 TOL (z) away (test_fused_cases_host.py)."""
    n = fc.N_FAR
    prob, refs, (_, far) = fc.problem(*s, n), fc.rows(*s, "far", n), fc.far_axes()
    worst = []
    for variant in _variants(s):
        for period in (1, 16, 64):
            for sample in (False, True):
                got = _run(hip, prob, far, 64, period, variant, sample=sample)
                errs = [sc.relerr(got[0][b], refs[b]["d"]) for b in range(3)]
                print(f"{fc.ident(s)} variant {variant} period {period} sample {sample}: d "
                      + " ".join(f"{e:.1e}" for e in errs))
                _against(got, refs, sample, (variant, period, sample), worst)
    _report(fc.ident(s), worst)
