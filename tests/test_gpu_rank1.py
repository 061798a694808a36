"""GPU: the rank-one rows in front of the steady switch (gf_steady_sweep_rank1), at the raw entry point
and through BatchedLogLikelihood with `force_streaming`: the C oracle at 1e-8 on every instance edge and batch shape,
the route off on the same engine, tilings (the recursion does not know about tiles: d, z, switch rows and headers bit
for bit), the acc form against the null-acc form + gf_reduce_tile_steady bit for bit, a matrix that is not positive
definite, a gap the caller promised away, the conditioning guard, the argument errors.  The evaluator takes the route
from 32 768 rows on (StreamingBatch.RANK1_MIN_ROWS); the engines of this file lower that limit, so that the route runs
at shapes of a few seconds.  Measured on an MI355X: 9e-14 ... 1.2e-12 against the oracle, 8e-15 against the route off."""
import numpy as np
import pytest

from tests.random_cases import oracle_loglikes
from tests.steady_raw import sweep_head
from tests.test_gpu_steady import RTOL_LL, _evaluator, _fast_terms, _rel, _series
from tests.test_gpu_steady_finish import N_FIN, T_FIN
from tests.test_gpu_steady_overlap import _spread_batch
from tests.test_rank1_host import rank1_rows, rank1_switch_row
from tests.test_steady_host import FAST_TERM, _two_terms

pytestmark = pytest.mark.gpu
RTOL_OFF = 1e-10        # the route against the full rows on the same engine
ST_SW, ST_VIOL = 0, 2   # slots of the steady buffer (include/gadfly_hip.h)


def _route_evaluator(hps, t, y, tile_rows):
    """tests/test_gpu_steady.py's evaluator with the route's shortest series (StreamingBatch.RANK1_MIN_ROWS, 32 768
    rows) lowered on its own engine: the route runs at the small shapes of this file."""
    ev, coeffs = _evaluator(hps, t, y, tile_rows)
    ev.engine.RANK1_MIN_ROWS = 0
    return ev, coeffs


def _flagship(B):
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    return [jitter_hyperparameters(solar_like_hyperparameters(30), 1000 + i) for i in range(B)]


def _scaled(terms, k):
    return _two_terms(*[(s0 * (1.0 + 0.05 * k), nu, q) for s0, nu, q in terms])


#: name -> (hyperparameters per walker, N, cadence, tile rows, every walker switches / none does)
PARITY = {
    "flagship": (lambda: _flagship(8), 65536, 60.0, 8192, True),
    "W=2": (lambda: [_fast_terms(1, k) for k in range(3)], 16384, 60.0, 1024, True),
    "J=3": (lambda: [_fast_terms(3, k) for k in range(3)], 16384, 60.0, 1024, True),
    "W=62": (lambda: [_fast_terms(31, k) for k in range(3)], 16384, 60.0, 1024, True),
    "slow-a": (lambda: [_scaled(((50.0, 30.0, 3e4), (2.0, 3000.0, 2.0)), k) for k in range(2)], 65536, 60.0, 8192, True),
    "slow-b": (lambda: [_scaled(((1e4, 2.0, 50.0), (2.0, 3000.0, 5.0)), k) for k in range(2)], 65536, 60.0, 8192, True),
    "never-arms": (lambda: [_scaled(((1e-3, 5.0, 1e5), (2.0, 3000.0, 2.0)), k) for k in range(2)], 65536, 60.0, 8192,
                   False),
    "fast-240s": (lambda: [_scaled(FAST_TERM, k) for k in range(3)], 16384, 240.0, 1024, True),
    "B=1": (lambda: [_fast_terms(2)], 16384 + 37, 60.0, 4096, True),
    "B=65": (lambda: [_fast_terms(2, k) for k in range(65)], 8192 + 37, 60.0, 2048, True),
}


def _axis(N, cadence, seed):
    from gadfly_amd.synth import uniform_times
    _, y = _series(N, seed=seed)
    return uniform_times(N, cadence), y


@pytest.mark.parametrize("name", list(PARITY))
def test_oracle_parity(hip, name):
    make, N, cadence, T, switches = PARITY[name]
    t, y = _axis(N, cadence, 31)
    ev, coeffs = _route_evaluator(make(), t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    got = ev.evaluate()
    eng = ev.engine
    sw = eng.steady_switch_rows()
    rel = _rel(got, ref)
    print(f"{name}: largest error vs oracle {rel.max():.2e}, switch rows {sw.tolist()}")
    assert eng.rank1_used and eng.steady_used and eng.kernel_used == "fused"
    assert rel.max() <= RTOL_LL, rel.tolist()
    if switches:
        assert np.all((sw > 0) & (sw < N) & ((sw - 1) % 64 == 0)), sw.tolist()
    else:
        assert np.all(sw == -1)             # the recursion ran to the end of the series
    assert ev.steady_reruns == 0 and ev.guard_reruns == 0


def _host_switch_rows(coeffs, t, y):
    rows = []
    for co in coeffs:
        diag = np.full(len(t), 900.0) + float(co[6])
        sw0 = 0
        # the rule needs the rows up to the switch only: lengthen the stretch until it holds one
        for n in (4096, 16384, len(t)):
            n = min(n, len(t))
            dd, _, gains = rank1_rows(co[:6], t[:n], diag[:n], y[:n])
            sw0 = rank1_switch_row(dd, gains)
            if sw0 > 0 or n == len(t):
                break
        rows.append(sw0)
    return np.array(rows)


@pytest.mark.parametrize("batch", ["spread", "flagship"])
def test_against_the_route_off(hip, batch):
    if batch == "spread":
        N, T = N_FIN, T_FIN
        hps = _spread_batch(30)[0]
    else:
        N, T = 65536, 8192
        hps = _flagship(2)
    t, y = _series(N, seed=29)
    ev, coeffs = _route_evaluator(hps, t, y, T)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    got = ev.evaluate()
    sw = eng.steady_switch_rows()
    assert eng.rank1_used
    eng.steady_rank1 = False
    off = ev.evaluate()
    sw_off = eng.steady_switch_rows()
    assert eng.steady_used and not eng.rank1_used
    # the host restatement knows the cadence of the whole axis: on a stretch of a uniform axis it is the same
    host = _host_switch_rows(coeffs, t, y)
    print(f"{batch}: route on / off {_rel(got, off).max():.2e}; switch rows on {sw.tolist()}, off {sw_off.tolist()}, "
          f"host restatement {host.tolist()}")
    assert _rel(got, off).max() <= RTOL_OFF
    assert np.all(host > 0) and np.all(sw > 0) and np.all(sw - 1 <= host + 1024), (sw.tolist(), host.tolist())
    assert ev.steady_reruns == 0


def test_short_series_stay_on_the_full_rows_by_default(hip):
    """Below StreamingBatch.RANK1_MIN_ROWS the evaluator keeps the full rows (existing tests pin their bits there)."""
    from gadfly_amd.engine import StreamingBatch
    t, y = _series(N_FIN, seed=29)
    ev, _ = _evaluator(_spread_batch(3)[0], t, y, T_FIN)
    assert N_FIN < StreamingBatch.RANK1_MIN_ROWS <= 65536
    ev.evaluate()
    assert ev.engine.steady_used and not ev.engine.rank1_used


# --------------------------------------------------------------------------------------------------------------------
# the raw entry point
# --------------------------------------------------------------------------------------------------------------------
class _Raw:
    """gf_steady_sweep_rank1 on an evaluator's buffers; d, z and work of its own (a tile's), and the whole series'
    rows collected on the device behind every tile."""

    def __init__(self, ev, t):
        import torch
        from gadfly_amd import _lib
        self.torch, self._lib = torch, _lib
        eng = self.eng = ev.engine
        ev.auto_generator_period, eng.generator_period = False, 1
        ev.evaluate()                       # (packs the coefficients; its own result is not used)
        self.lib, self.p, self.B, self.N = eng.lib, _lib.ptr, eng.B, eng.N
        self.f64 = dict(dtype=torch.float64, device=eng.device)
        self.stream = torch.cuda.current_stream(eng.device).cuda_stream
        self.dt = torch.full((self.B,), (t[-1] - t[0]) / (len(t) - 1), **self.f64)

    def run(self, tiling, acc_from=0, block=None):
        """The tiles (n_first, rows) in order, with acc from tile `acc_from` on (None: never) and the null-acc form +
        gf_reduce_tile_steady in front of it.  d, z and acc are prefilled with NaN."""
        torch, eng, lib, p, B, N = self.torch, self.eng, self.lib, self.p, self.B, self.N
        steady = torch.zeros((B, int(lib.gf_steady_size())), **self.f64)
        acc = torch.full((B, 3), float("nan"), **self.f64)
        D = torch.full((B, N), float("nan"), **self.f64)
        Z = torch.full((B, N), float("nan"), **self.f64)
        eng.S_state.zero_()
        eng.info.zero_()
        over = {} if block is None else dict(block=block)
        for k, (n0, rows) in enumerate(tiling):
            assert rows > 0 and n0 + rows <= N
            d = torch.full((B, rows), float("nan"), **self.f64)
            z = torch.full((B, rows), float("nan"), **self.f64)
            args = (*sweep_head(eng, rows, n0, d=p(d), z=p(z), **over), p(steady), 0)
            init = 1 if k == 0 else 0
            if acc_from is not None and k >= acc_from:
                st = lib.gf_steady_sweep_rank1(*args, p(acc), init, p(self.dt), self.stream)
                self._lib.check(st, "gf_steady_sweep_rank1")
            else:
                st = lib.gf_steady_sweep_rank1(*args, None, init, p(self.dt), self.stream)
                self._lib.check(st, "gf_steady_sweep_rank1")
                work = torch.full((B * int(lib.gf_reduce_work(rows)),), float("nan"), **self.f64)
                st = lib.gf_reduce_tile_steady(B, rows, n0, p(d), p(z), p(steady), p(work), p(acc), init, self.stream)
                self._lib.check(st, "gf_reduce_tile_steady")
            D[:, n0:n0 + rows] = d
            Z[:, n0:n0 + rows] = z
        torch.cuda.synchronize()
        got = dict(acc=acc, steady=steady, info=eng.info, S_state=eng.S_state, d=D, z=Z)
        return {k: v.cpu().numpy().copy() for k, v in got.items()}


def _uniform(N, T):
    return [(n0, min(T, N - n0)) for n0 in range(0, N, T)]


def _stored(res):
    """Per problem the rows in front of its switch row (all rows where it has not switched)."""
    sw = res["steady"][:, ST_SW].astype(np.int64)
    return np.where(sw > 0, sw, res["d"].shape[1])


@pytest.fixture(scope="module")
def spread(hip):
    """The four-walker batch whose walkers switch in tiles 0, 1, 2 and 0 of T_FIN rows, and one run on those tiles."""
    t, y = _series(N_FIN, seed=29)
    hps, want = _spread_batch(30)
    ev, _ = _route_evaluator(hps, t, y, T_FIN)
    r = _Raw(ev, t)
    a = r.run(_uniform(N_FIN, T_FIN), block=4)
    sw = a["steady"][:, ST_SW].astype(np.int64)
    print(f"switch rows {sw.tolist()}")
    assert np.all(a["info"] == 0) and np.all(np.isfinite(a["acc"])) and ((sw - 1) // T_FIN).tolist() == want
    return r, a, sw


def _check_rows(res):
    """Rows in front of the switch row are finite, no row behind it was written."""
    lim = _stored(res)
    for b, n in enumerate(lim):
        assert np.all(np.isfinite(res["d"][b, :n])) and np.all(np.isfinite(res["z"][b, :n])), b
        assert np.all(np.isnan(res["d"][b, n:])) and np.all(np.isnan(res["z"][b, n:])), b


@pytest.mark.parametrize("tiles", ["300", "one", "switch-65-rows-in"])
def test_tilings_give_the_same_rows_and_headers(spread, tiles):
    r, a, sw = spread
    _check_rows(a)
    if tiles == "300":
        tiling = _uniform(N_FIN, 300)
    elif tiles == "one":
        tiling = [(0, N_FIN)]
    else:
        n0 = int(sw[1]) - 1 - 64            # walker 1's switch anchor is row 64 of a tile of 300 rows: 65 rows stored
        assert n0 > T_FIN and n0 % 64 == 0
        tiling = [(0, n0), (n0, 300), (n0 + 300, N_FIN - n0 - 300)]
    b = r.run(tiling, block=4)
    _check_rows(b)
    for key in ("d", "z", "steady", "info"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (tiles, key)
    err = np.abs(a["acc"] - b["acc"]) / np.abs(a["acc"])
    print(f"tiling {tiles}: acc agrees to {err.max():.2e}")
    assert err.max() <= 1e-13


@pytest.mark.parametrize("k", [1, 2, None])
def test_acc_form_gives_the_two_calls_bits(spread, k):
    """Tile k on with acc (the fixture: from tile 0 on), the tiles in front of it with the null-acc form and
    gf_reduce_tile_steady; None: the two calls on every tile."""
    r, a, _ = spread
    b = r.run(_uniform(N_FIN, T_FIN), acc_from=k, block=4)
    for key in ("acc", "steady", "info", "S_state", "d", "z"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (k, key)


@pytest.fixture(scope="module")
def failing(hip):
    """tests/test_gpu_steady.py::test_failing_walker_reports_its_row's batch: walker 2 is not positive definite."""
    import gadfly_amd
    N, T = 8192, 1024
    t, y = _series(N, seed=17)
    kernels = [gadfly_amd.StellarOscillatorKernel(_fast_terms(2, k0), texp=60.0) for k0 in range(4)]
    diag = np.full((4, N), 900.0)
    diag[2] = -0.5 * float(np.sum(kernels[2].get_device_coefficients()[2]))
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag, tile_rows=T)
    ev.engine.force_streaming = True
    ev.engine.RANK1_MIN_ROWS = 0
    return ev, t, N, T


def test_failing_walker(failing):
    ev, t, N, T = failing
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    out = ev.evaluate_device()
    info = eng.info.cpu().numpy().copy()
    sw = eng.steady_switch_rows()
    assert eng.rank1_used
    ev.resolve()
    got = out.cpu().numpy()
    eng.steady_rank1 = False
    out_off = ev.evaluate_device()
    info_off = eng.info.cpu().numpy().copy()
    assert eng.steady_used and not eng.rank1_used
    ev.resolve()
    off = out_off.cpu().numpy()
    eng.steady_rank1 = True
    print(f"info {info.tolist()} (route off {info_off.tolist()}), switch rows {sw.tolist()}")
    assert info[2] > 0 and np.array_equal(info, info_off)
    ok = [0, 1, 3]
    assert got[2] == -np.inf and np.all(sw[ok] > 0) and _rel(got[ok], off[ok]).max() <= RTOL_OFF
    # at the raw entry point it enters the later tiles failed: acc as the two calls leave it
    r = _Raw(ev, t)
    a = r.run(_uniform(N, T), acc_from=None)
    bad = int(a["info"][2])
    k_fail = (bad - 1) // T
    assert bad == info[2] and k_fail < N // T - 1
    for k in sorted({0, k_fail, k_fail + 1}):
        b = r.run(_uniform(N, T), acc_from=k)
        for key in ("acc", "steady", "info", "d", "z"):
            assert np.array_equal(a[key], b[key], equal_nan=True), (k, key)
    assert np.all(np.isnan(a["d"][2, bad - 1:]))        # the failing row and the rows behind it were not stored


def test_gap_that_was_promised_away(hip):
    """An axis with one gap in tile 1 of 512 rows, in front of any switch: at the raw entry point (arm_from = 0
    promised) every problem's flag is raised and the rows stay finite; the evaluator does not take the route."""
    N, row, T = 16384, 700, 512
    t, y = _series(N, seed=11)
    t = t.copy()
    t[row:] += 700 * 60e-6
    ev, _ = _route_evaluator([_fast_terms(2, k0) for k0 in range(4)], t, y, T)
    r = _Raw(ev, t)
    assert r.eng.steady_used and not r.eng.rank1_used and r.eng._steady_axis[0] == row
    a = r.run(_uniform(N, T)[:3])
    assert np.all(a["steady"][:, ST_VIOL] != 0.0) and np.all(a["info"] == 0)
    lim = np.minimum(_stored(a), 3 * T)     # (the recursion knows no stamps: a problem may switch behind the gap)
    assert np.all(lim > row)
    for b, n in enumerate(lim):
        assert np.all(np.isfinite(a["d"][b, :n])) and np.all(np.isfinite(a["z"][b, :n])), b
    assert np.all(np.isfinite(a["acc"]))


def test_conditioning_guard(hip):
    """One walker of three beyond RANK1_COND_LIMIT: resolve() repeats exactly that one, in the reference formulation."""
    from gadfly_amd.engine import StreamingBatch
    N = 16384
    t, y = _series(N, seed=23)
    hps = [_two_terms((s0, 2.0, 50.0), (2.0, 3000.0, 5.0)) for s0 in (1e4, 3e7, 2e4)]
    ev, _ = _route_evaluator(hps, t, y, 4096)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    out = ev.evaluate_device()
    assert eng.rank1_used
    cond = eng._rank1_conditions().cpu().numpy()
    viol = eng.steady_violations().cpu().numpy()
    print(f"max a / min d {cond.tolist()}")
    assert cond[1] > StreamingBatch.RANK1_COND_LIMIT > max(cond[0], cond[2])
    assert viol.tolist() == [False, True, False]
    first = out.cpu().numpy().copy()
    assert ev.resolve() == 1 and ev.steady_reruns == 1
    got = out.cpu().numpy()
    eng.steady_state = False
    ref = ev.evaluate()
    assert got[1] == ref[1] and np.array_equal(got[[0, 2]], first[[0, 2]])
    assert _rel(got, ref).max() <= RTOL_OFF


def test_argument_errors(spread):
    r, _, _ = spread
    eng, lib, p = r.eng, r.lib, r.p
    acc = r.torch.full((r.B, 3), float("nan"), **r.f64)
    steady = r.torch.zeros((r.B, int(lib.gf_steady_size())), **r.f64)

    def call(**over):
        v = dict(steady=p(steady), acc=p(acc), dt=p(r.dt), rows=64, n0=0, head={})
        v.update(over)
        head = sweep_head(eng, v["rows"], v["n0"], diag=None, diag_bs=0, **v["head"])
        return lib.gf_steady_sweep_rank1(*head, v["steady"], 0, v["acc"], 1, v["dt"], r.stream)

    for over, text in [(dict(dt=None), "null pointer"), (dict(steady=None), "null pointer"),
                       (dict(rows=0), "empty problem"), (dict(n0=-64), "n_first"),
                       (dict(head=dict(Jr=1)), "Jr = 0"), (dict(head=dict(variant=r._lib.GF_SWEEP_COLUMN)), "lane-tiled")]:
        assert call(**over) != 0, over
        msg = r._lib.last_error()
        assert msg.startswith("gf_steady_sweep_rank1:") and text in msg, msg
    r.torch.cuda.synchronize()
    assert np.all(np.isnan(acc.cpu().numpy()))                      # no launch went through
