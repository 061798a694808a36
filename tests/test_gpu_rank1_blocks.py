"""GPU: the blocks of k_steady_rank1 at the raw entry point.  A block of 64 rows stages its d and z
in registers and stores them once, tests its pivots at the anchor and at its end, and runs as rows in front of the
anchor, the anchor row, rows behind it; blocks are counted from the tile's first row.  So every tiling moves the anchor
inside the block, the block's length and what is staged when the wave leaves: the results must not know.

  * tilings as explicit row lists: tiles that start at 0, 1, 31, 32 and 63 mod 64, last blocks of 1, 31, 33, 63 and 64
    rows, the tile of a switch at 1, 32 and 63 mod 64: d, z, header and ring and info are the one-tile run's bits,
    rows behind the switch row stay NaN; S_state, which a tile leaves only where it ends unswitched, is the bits of the
    run that reaches that row in one tile; acc in the acc form is the bits of the null-acc form + gf_reduce_tile_steady
    on the same tiles, and the one-tile run's to 1e-13 (each tile adds its own sum: tests/test_gpu_rank1.py's bound);
  * a failing row at block rows 0, 1, 62 and 63 with the block's anchor in front of it, behind it and on it (which of
    these is possible follows from the failing row mod 64, so seven walkers fail at rows 63, 64, 65, 100, 127, 128 and
    129): info, the rows in front, the ring and the counters are the one-tile run's bits, the rest stays NaN;
  * t and y behind a tile's last row are NaN (the block's loads are clamped to the tile): nothing changes."""
import numpy as np
import pytest

from tests.test_gpu_rank1 import _Raw, _route_evaluator, _stored
from tests.test_gpu_steady import _fast_terms, _series
from tests.test_gpu_steady_finish import N_FIN, T_FIN
from tests.test_gpu_steady_overlap import _spread_batch

pytestmark = pytest.mark.gpu
ST_SW, ST_VIOL = 0, 2   # slots of the steady buffer (include/gadfly_hip.h)
KEYS = ("d", "z", "steady", "info")


def _tiles(rows, N):
    """(n_first, rows) of the tiles with the given row counts; the last tile takes the rest of the N rows."""
    out, n0 = [], 0
    for r in rows:
        out.append((n0, r))
        n0 += r
    assert n0 < N
    return out + [(n0, N - n0)]


def _last_blocks(tiling):
    return {(rows - 1) % 64 + 1 for _, rows in tiling}


def _same(a, b, keys, what):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def _rows_behind_stay_nan(res, N):
    for b, n in enumerate(np.minimum(_stored(res), N)):
        assert np.all(np.isfinite(res["d"][b, :n])) and np.all(np.isfinite(res["z"][b, :n])), b
        assert np.all(np.isnan(res["d"][b, n:])) and np.all(np.isnan(res["z"][b, n:])), b


# --------------------------------------------------------------------------------------------------------------------
# tilings, on the batch whose walkers switch in tiles 0, 1, 2 and 0 of 4096 rows
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread(hip):
    t, y = _series(N_FIN, seed=29)
    hps, want = _spread_batch(30)
    ev, _ = _route_evaluator(hps, t, y, T_FIN)
    r = _Raw(ev, t)
    # a tile starts at a multiple of the generator block: block = 1 reaches every row (its gap threshold is 0, so
    # every block raises ST_VIOL, in every run alike; test_clamped_loads keeps block = 4 and a clean flag)
    one = r.run([(0, N_FIN)], block=1)
    sw = one["steady"][:, ST_SW].astype(np.int64)
    print(f"switch rows {sw.tolist()}")
    assert np.all(one["info"] == 0) and ((sw - 1) // T_FIN).tolist() == want and np.all((sw - 1) % 64 == 0)
    _rows_behind_stay_nan(one, N_FIN)
    return r, one, sw, {}


def _switch_tiling(sw, residue):
    """Cuts that put every switch anchor (row sw - 1, a multiple of 64) into a tile that starts at `residue` mod 64,
    128 rows or less in front of it; anchors too close to the one before share its tile."""
    cuts = []
    for a in sorted(set((sw - 1).tolist())):
        c = a - 128 + residue
        if c > (cuts[-1] if cuts else 0) + 64:
            cuts.append(c)
    return [c1 - c0 for c0, c1 in zip([0] + cuts[:-1], cuts)]


TILINGS = {
    "0-1-mod-64": lambda sw: [1, 63, 64, 65, 127, 129],
    "32-63-mod-64": lambda sw: [32, 31, 1],
    "31-mod-64": lambda sw: [31, 33, 95, 64],
    "switch-at-1": lambda sw: _switch_tiling(sw, 1),
    "switch-at-32": lambda sw: _switch_tiling(sw, 32),
    "switch-at-63": lambda sw: _switch_tiling(sw, 63),
}
STARTS = {"0-1-mod-64": {0, 1}, "32-63-mod-64": {0, 32, 63}, "31-mod-64": {0, 31}, "switch-at-1": {1},
          "switch-at-32": {32}, "switch-at-63": {63}}
LAST = {"0-1-mod-64": {1, 63, 64}, "32-63-mod-64": {1, 31, 32}, "31-mod-64": {31, 33, 64}}


def _state_reference(r, cache, c):
    """S_state of the run that reaches row c in one tile."""
    if c not in cache:
        cache[c] = r.run([(0, c)], block=1)["S_state"]
    return cache[c]


@pytest.mark.parametrize("name", list(TILINGS))
def test_tilings(spread, name):
    r, one, sw, cache = spread
    tiling = _tiles(TILINGS[name](sw), N_FIN)
    starts = {n0 % 64 for n0, _ in tiling}
    assert STARTS[name] <= starts and LAST.get(name, set()) <= _last_blocks(tiling), tiling
    # the tile each walker switches in, and where it starts
    tile_of = [max(n0 for n0, _ in tiling if n0 <= s - 1) for s in sw]
    if name.startswith("switch-at-"):
        want = int(name.split("-")[-1])
        hit = [b for b, n0 in enumerate(tile_of) if n0 > 0 and n0 % 64 == want]
        print(f"{name}: walkers {hit} switch in a tile that starts at {want} mod 64 (tile starts {tile_of})")
        assert len(hit) >= 2
    acc = r.run(tiling, block=1)                            # the acc form on every tile
    two = r.run(tiling, acc_from=None, block=1)             # the null-acc form + gf_reduce_tile_steady
    _same(one, acc, KEYS, name)
    _same(acc, two, KEYS + ("acc", "S_state"), name)
    _rows_behind_stay_nan(acc, N_FIN)
    err = np.abs(acc["acc"] - one["acc"]) / np.abs(one["acc"])
    print(f"{name}: acc against the one-tile run {err.max():.2e}")
    assert err.max() <= 1e-13
    for b, c in enumerate(tile_of):                         # the state the last unswitched tile left
        if c > 0:
            assert np.array_equal(acc["S_state"][b], _state_reference(r, cache, c)[b]), (name, b, c)
        else:
            assert not np.any(acc["S_state"][b]), (name, b)


def test_clamped_loads(spread):
    """Every tile sees a series that ends with it: t and y behind its last row are NaN, and y is one series per
    problem, cut at the tile's end, so that the next problem's slot comes next and is NaN as well (its rows in front of
    the tile, which no row of the tile reads).  The last block's loads of the rows behind the tile are clamped to the
    tile's last row: the same bits, and no spacing flagged."""
    r, one, sw, _ = spread
    torch, eng, B = r.torch, r.eng, r.B
    tiling = _tiles([4, 60, 64, 68, 124, 132], N_FIN)    # last blocks of 4, 60 and 64 rows
    want = r.run(tiling, block=4)
    _same(one, want, ("d", "z", "info"), "tiling")
    assert not np.any(want["steady"][:, ST_VIOL])
    t0 = eng.t.reshape(-1, eng.t.shape[-1])
    y0 = eng.y.reshape(-1, eng.y.shape[-1]).expand(B, -1)
    series = []
    for n0, rows in tiling:
        end = n0 + rows
        tc = torch.full((t0.shape[0], end + 128), float("nan"), **r.f64)
        tc[:, :end] = t0[:, :end]
        yc = torch.full((B + 1, end), float("nan"), **r.f64)            # batch stride = the tile's end; a spare slot
        yc[:B, n0:end] = y0[:, n0:end]
        series.append((tc, yc))
    got = _run_on(r, tiling, series)
    _same(want, got, KEYS + ("acc", "S_state"), "NaN behind the tile")


def _run_on(r, tiling, series):
    """_Raw.run's acc form with the engine's t and y replaced tile by tile (same strides' meaning: rows contiguous)."""
    torch, eng, lib, p, B, N = r.torch, r.eng, r.lib, r.p, r.B, r.N
    from tests.steady_raw import sweep_head
    steady = torch.zeros((B, int(lib.gf_steady_size())), **r.f64)
    acc = torch.full((B, 3), float("nan"), **r.f64)
    D = torch.full((B, N), float("nan"), **r.f64)
    Z = torch.full((B, N), float("nan"), **r.f64)
    eng.S_state.zero_()
    eng.info.zero_()
    for k, ((n0, rows), (tc, yc)) in enumerate(zip(tiling, series)):
        d = torch.full((B, rows), float("nan"), **r.f64)
        z = torch.full((B, rows), float("nan"), **r.f64)
        t_bs = 0 if tc.shape[0] == 1 else tc.shape[1]
        y_bs = 0 if yc.shape[0] == 1 else yc.shape[1]
        args = (*sweep_head(eng, rows, n0, d=p(d), z=p(z), block=4, t=p(tc), t_bs=t_bs, y=p(yc), y_bs=y_bs),
                p(steady), 0)
        st = lib.gf_steady_sweep_rank1(*args, p(acc), 1 if k == 0 else 0, p(r.dt), r.stream)
        r._lib.check(st, "gf_steady_sweep_rank1")
        D[:, n0:n0 + rows] = d
        Z[:, n0:n0 + rows] = z
    torch.cuda.synchronize()
    got = dict(acc=acc, steady=steady, info=eng.info, S_state=eng.S_state, d=D, z=Z)
    return {k: v.cpu().numpy().copy() for k, v in got.items()}


# --------------------------------------------------------------------------------------------------------------------
# a failing row anywhere in its block
# --------------------------------------------------------------------------------------------------------------------
#: walker 0 is positive definite; the others are tests/test_gpu_rank1.py's failing walker with a diagonal at which the
#: pivot turns negative at the named row (the recursion of tests/test_rank1_host.py on the host; each value lies in the
#: middle of its row's interval, 0.15 wide or more)
FAIL_DIAG = {63: -5952.44, 64: -5951.15, 65: -5949.92, 100: -5927.44, 127: -5921.20, 128: -5921.04, 129: -5920.885}
N_FAIL, ROWS_FAIL = 8192, 2048


@pytest.fixture(scope="module")
def failing(hip):
    import gadfly_amd
    t, y = _series(N_FAIL, seed=17)
    kernels = [gadfly_amd.StellarOscillatorKernel(_fast_terms(2, 0), texp=60.0)]
    kernels += [gadfly_amd.StellarOscillatorKernel(_fast_terms(2, 2), texp=60.0) for _ in FAIL_DIAG]
    diag = np.full((len(kernels), N_FAIL), 900.0)
    for b, v in enumerate(FAIL_DIAG.values()):
        diag[1 + b] = v
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag, tile_rows=1024)
    ev.engine.force_streaming = True
    ev.engine.RANK1_MIN_ROWS = 0
    r = _Raw(ev, t)
    one = r.run([(0, ROWS_FAIL)], block=1)          # (block = 1: a tile may start at any row, see `spread`)
    print(f"info {one['info'].tolist()}")
    assert one["info"].tolist() == [0] + [f + 1 for f in FAIL_DIAG]
    for b, f in enumerate(FAIL_DIAG):
        assert np.all(np.isfinite(one["d"][1 + b, :f])) and np.all(np.isnan(one["d"][1 + b, f:]))
        assert np.all(np.isfinite(one["z"][1 + b, :f])) and np.all(np.isnan(one["z"][1 + b, f:]))
    return r, one


def _fail_cases():
    """(failing row, block row, tile start, where the block's anchor lies) for every start that puts the row there."""
    out = []
    for f in FAIL_DIAG:
        for p in (0, 1, 62, 63):
            n0 = f - p - 64 if f - p > 64 else f - p
            if n0 < 1:
                continue
            ja = (64 - n0 % 64) % 64
            out.append((f, p, n0, "front" if ja < p else "behind" if ja > p else "on"))
    return out


def test_fail_cases_cover_the_block():
    seen = {(p, side) for _, p, _, side in _fail_cases()}
    assert {(0, "behind"), (0, "on"), (1, "front"), (1, "behind"), (62, "front"), (62, "behind"), (63, "front"),
            (63, "on")} <= seen, sorted(seen)


@pytest.mark.parametrize("f,p,n0,side", _fail_cases())
def test_failing_row(failing, f, p, n0, side):
    r, one = failing
    for acc_from in (0, None):
        got = r.run([(0, n0), (n0, ROWS_FAIL - n0)], acc_from=acc_from, block=1)
        _same(one, got, KEYS, (f, p, n0, side, acc_from))       # info, rows in front, NaN from the row on, ring, counters
