"""GPU: the finishing launch over a window of switch rows (gf_steady_finish_window), the entry point
with which the tails of early switchers can be finished before the stragglers' (the evaluator does not: DESIGN.md 7 has
the measurement), on a batch whose walkers switch in different tiles (chosen with the rule on the oracle's factor):
windows that split the observed switch rows, in either order, against one gf_steady_finish -- acc and the whole steady
buffer bit for bit; sw == sw_lo is taken, sw == sw_hi is not; a window without a switch row touches nothing; the
argument errors."""
import numpy as np
import pytest

from tests.steady_raw import finish_head, sweep_head
from tests.test_gpu_steady import _evaluator, _series
from tests.test_gpu_steady_finish import N_FIN, T_FIN
from tests.test_steady_host import _switch_row, _two_terms

pytestmark = pytest.mark.gpu


def _spread_terms(J, tile, k0=0):
    """_fast_terms slowed down so that the factor reaches its steady state in tile `tile` (0, 1, 2) of T_FIN rows."""
    scale = (1.0, 0.1, 0.05)[tile]
    nu = np.geomspace(400.0, 4000.0, J) * scale
    return _two_terms(*[(2.0 + 0.1 * (k + k0), nu[k] * (1.0 + 0.01 * k0), 2.0 + (k % 4)) for k in range(J)])


def _spread_batch(J):
    """Four walkers: switches in tiles 0, 1, 2 and 0 of T_FIN rows."""
    return [_spread_terms(J, 0), _spread_terms(J, 1), _spread_terms(J, 2), _spread_terms(J, 0, k0=1)], [0, 1, 2, 0]


def _oracle_tiles(coeffs, t, T):
    """Tile of the row at which the rule (tests/test_steady_host.py) freezes the oracle's own factor, per kernel."""
    from oracle import cref
    tiles = []
    for co in coeffs:
        c, a, U, V = cref.get_matrices(co[:6], t, np.full(len(t), 900.0) + co[6])
        d, W, info = cref.factor(t, c, a, U, V)
        assert info == 0
        row, _, _ = _switch_row(t, np.asarray(co[5], dtype=np.float64), d, W)
        assert row > 0
        tiles.append(row // T)
    return tiles


# --------------------------------------------------------------------------------------------------------------------
# the raw entry point
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw(hip):
    """The tiles of one evaluation through gf_steady_sweep + gf_reduce_tile_steady on an evaluator's buffers, once;
    acc and the steady buffer in front of the finishing launches are kept, and run(layout) finishes a copy of them:
    layout None is one gf_steady_finish, a list of (sw_lo, sw_hi) that many gf_steady_finish_window calls."""
    import torch
    from gadfly_amd import _lib
    N, T, J = N_FIN, T_FIN, 30
    t, y = _series(N, seed=29)
    hps, want = _spread_batch(J)
    ev, coeffs = _evaluator(hps, t, y, T)
    assert _oracle_tiles(coeffs, t, T) == want
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    ev.evaluate()                           # (packs the coefficients; its own result is not used)
    lib, p, B = eng.lib, _lib.ptr, eng.B
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    f64 = dict(dtype=torch.float64, device=eng.device)
    steady0 = torch.zeros((B, int(lib.gf_steady_size())), **f64)
    acc0 = torch.full((B, 3), float("nan"), **f64)
    eng.S_state.zero_()
    eng.F_state.zero_()
    eng.info.zero_()
    eng.d.fill_(float("nan"))
    eng.z.fill_(float("nan"))
    for k, n0 in enumerate(range(0, N, T)):
        rows = min(T, N - n0)
        st = lib.gf_steady_sweep(*sweep_head(eng, rows, n0), p(steady0), 0, stream)
        _lib.check(st, "gf_steady_sweep")
        st = lib.gf_reduce_tile_steady(B, rows, n0, p(eng.d), p(eng.z), p(steady0), p(eng.work), p(acc0),
                                       1 if k == 0 else 0, stream)
        _lib.check(st, "gf_reduce_tile_steady")
    torch.cuda.synchronize()
    assert np.all(eng.info.cpu().numpy() == 0)
    sw = steady0[:, 0].cpu().numpy().astype(np.int64)

    def call(buf, acc, window, **over):
        head = finish_head(eng, N, buf, acc, **over)
        if window is None:
            return lib.gf_steady_finish(*head, stream)
        return lib.gf_steady_finish_window(*head, int(window[0]), int(window[1]), stream)

    def run(layout):
        steady, acc = steady0.clone(), acc0.clone()
        for window in ([None] if layout is None else layout):
            _lib.check(call(steady, acc, window), "finish")
        torch.cuda.synchronize()
        return acc.cpu().numpy(), steady.cpu().numpy()

    return dict(N=N, T=T, B=B, sw=sw, run=run, call=call, before=(acc0.cpu().numpy(), steady0.cpu().numpy()),
                buffers=lambda: (steady0.clone(), acc0.clone()), lib=_lib)


def _same(got, want):
    return np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True)


def test_raw_switch_rows_are_spread(raw):
    sw, T = raw["sw"], raw["T"]
    print(f"switch rows {sw.tolist()}")
    assert ((sw - 1) // T).tolist() == [0, 1, 2, 0] and len(set(sw.tolist())) >= 3


def test_raw_windows_give_the_single_launch_bit_for_bit(raw):
    N, sw, run = raw["N"], raw["sw"], raw["run"]
    one = run(None)
    assert np.all(np.isfinite(one[0])) and not _same(one, raw["before"])
    a, b, c = np.unique(sw)[[0, -2, -1]]    # a <= the early ones' rows < b < c
    assert a < b < c
    layouts = {
        "the window is everything": [(1, N + 1)],
        "zero is a legal lower end": [(0, N + 1)],
        "two, boundary between two switch rows": [(1, a + 1), (a + 1, N + 1)],
        "two, boundary on a problem's own switch row": [(1, b), (b, N + 1)],
        "three, boundaries on switch rows": [(1, b), (b, c), (c, N + 1)],
        "three, boundaries behind switch rows": [(1, a + 1), (a + 1, b + 1), (b + 1, N + 1)],
        "with an empty window in between": [(1, b), (b, b), (b, N + 1)],
    }
    for name, layout in layouts.items():
        for order in (layout, layout[::-1]):
            assert _same(run(order), one), (name, order)
    # sw == sw_lo is taken, sw == sw_hi is not: [b, c) finishes exactly the problem(s) switched at b
    part = run([(b, c)])
    took = sw == b
    assert took.any() and not took.all()
    assert np.array_equal(part[0][took], one[0][took]) and np.array_equal(part[1][took], one[1][took])
    assert _same((part[0][~took], part[1][~took]), (raw["before"][0][~took], raw["before"][1][~took]))


def test_raw_window_without_a_switch_row_touches_nothing(raw):
    N, sw, run = raw["N"], raw["sw"], raw["run"]
    u = np.unique(sw)
    holes = [(0, 1), (0, int(u[0])), (int(u[-1]) + 1, N + 1), (int(u[-1]) + 1, 2 ** 62), (5, 5)]
    holes += [(int(lo) + 1, int(hi)) for lo, hi in zip(u[:-1], u[1:]) if hi > lo + 1]
    assert len(holes) >= 6
    for hole in holes:
        assert _same(run([hole]), raw["before"]), hole


def test_raw_argument_errors(raw):
    lib, call, N = raw["lib"], raw["call"], raw["N"]
    steady, acc = raw["buffers"]()
    cases = [
        (dict(window=(-1, 5)), "0 <= sw_lo <= sw_hi"),
        (dict(window=(7, 6)), "0 <= sw_lo <= sw_hi"),
        (dict(window=(1, N + 1), B=0), "empty problem"),
        (dict(window=(1, N + 1), N=0), "empty problem"),
        (dict(window=(1, N + 1), Jr=1), "lane-tiled sweep only"),
        (dict(window=(1, N + 1), Jc=32), "lane-tiled sweep only"),
        (dict(window=(1, N + 1), block=3), "power of two"),
        (dict(window=(1, N + 1), ac=None), "null pointer"),
        (dict(window=(1, N + 1), info=None), "null pointer"),
        (dict(window=(5, 5), steady=None), "null pointer"),         # checked before the empty window returns
    ]
    for kw, text in cases:
        window = kw.pop("window")
        assert call(steady, acc, window, **kw) != 0, (window, kw)
        msg = lib.last_error()
        assert msg.startswith("gf_steady_finish_window:") and text in msg, msg
    assert call(steady, acc, (5, 5)) == 0
    import torch
    torch.cuda.synchronize()
    assert _same((acc.cpu().numpy(), steady.cpu().numpy()), raw["before"])      # no launch went through
