"""GPU: the streamed log-likelihood's steady route without stored tail rows (gf_steady_sweep + gf_reduce_tile_steady per
tile, one gf_steady_finish per evaluation): the narrowest, the flagship's and the widest instance
against the oracle and the plain sweep; d and z full of NaN before the evaluation (no row is read that was not written);
the raw entry points against the per-tile route (gf_loglike_steady + gf_reduce_tile) on the same buffers, slot by slot of
acc; a batch in which one walker never arms; a tail shorter than one block and a switch in the last tile."""
import numpy as np
import pytest

from tests.random_cases import oracle_loglikes
from tests.steady_raw import finish_head, sweep_head
from tests.test_gpu_steady import RTOL_LL, _evaluator, _fast_terms, _rel, _series
from tests.test_steady_host import GRID, LAG, COUNT, _switch_row, _two_terms

pytestmark = pytest.mark.gpu
B_FIN, N_FIN, T_FIN = 3, 16384 + 37, 4096       # four full tiles and one of 37 rows: a partial last block
RTOL_PLAIN = 1e-10      # the steady mode's whole share of the error budget


def _steady_and_plain(ev):
    """One evaluation on the steady route and one on the plain sweep at the same generator period."""
    eng = ev.engine
    got = ev.evaluate()
    sw, used = eng.steady_switch_rows(), int(eng.generator_period)
    assert eng.steady_used and eng.kernel_used == "fused"
    eng.steady_state = False
    ev.auto_generator_period, eng.generator_period = False, used
    plain = ev.evaluate()
    assert not eng.steady_used
    eng.steady_state = True
    return got, plain, sw


@pytest.mark.parametrize("J", [1, 30, 31])
def test_evaluator_against_oracle_and_plain_sweep(hip, J):
    N, T = N_FIN, T_FIN
    t, y = _series(N, seed=23)
    hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
    ev, coeffs = _evaluator(hps, t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    got, plain, sw = _steady_and_plain(ev)
    print(f"J = {J}: switch rows {sw.tolist()}, error vs oracle {_rel(got, ref).max():.2e} (plain sweep "
          f"{_rel(plain, ref).max():.2e}), steady vs plain {_rel(got, plain).max():.2e}")
    assert ev.engine.tile_rows == T
    # every switch inside a tile (the anchor is never a tile's first row), at least two tiles behind it
    assert np.all(sw > 0) and np.all((sw - 1) % T != 0) and np.all(sw < N - 2 * T), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert _rel(got, plain).max() <= RTOL_PLAIN
    assert ev.steady_reruns == 0


def test_stale_row_buffers_are_never_read(hip):
    """d and z hold NaN in every row before the evaluation: the bounded reductions read the rows the sweep instance
    stored in this evaluation only, so the values are those of an evaluator with clean buffers, bit for bit."""
    N, T = N_FIN, T_FIN
    t, y = _series(N, seed=23)
    hps = [_fast_terms(30, k0) for k0 in range(B_FIN)]
    out = []
    for fill in (False, True):
        ev, _ = _evaluator(hps, t, y, T)
        ev.auto_generator_period = False
        if fill:
            ev.engine.d.fill_(float("nan"))
            ev.engine.z.fill_(float("nan"))
        out.append(ev.evaluate())
        sw = ev.engine.steady_switch_rows()
        assert ev.engine.steady_used and np.all((sw > 0) & (sw < N - 2 * T)), sw.tolist()
    assert np.all(np.isfinite(out[0]))
    assert np.array_equal(out[0], out[1]), (out[0].tolist(), out[1].tolist())


def test_raw_entry_points_against_the_per_tile_route(hip):
    """gf_loglike_steady + gf_reduce_tile tile by tile, then gf_steady_sweep + gf_reduce_tile_steady tile by tile and
    one gf_steady_finish, on the evaluator's own buffers: acc's two sums agree to 1e-10 (the tail's block grid moves
    from the tiles' first rows to the switch row) and min d is the same number."""
    import torch
    from gadfly_amd import _lib
    N, T, J = N_FIN, T_FIN, 30
    t, y = _series(N, seed=29)
    hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
    ev, coeffs = _evaluator(hps, t, y, T)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    ev.evaluate()                           # (packs the coefficients; its own result is not used)
    lib, p, B = eng.lib, _lib.ptr, eng.B
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    f64 = dict(dtype=torch.float64, device=eng.device)

    def route(new):
        steady = torch.zeros((B, int(lib.gf_steady_size())), **f64)
        acc = torch.full((B, 3), float("nan"), **f64)
        eng.S_state.zero_()
        eng.F_state.zero_()
        eng.info.zero_()
        eng.d.fill_(float("nan"))
        eng.z.fill_(float("nan"))
        for k, n0 in enumerate(range(0, N, T)):
            rows = min(T, N - n0)
            sweep = lib.gf_steady_sweep if new else lib.gf_loglike_steady
            st = sweep(*sweep_head(eng, rows, n0), p(steady), 0, stream)
            _lib.check(st, "sweep")
            if new:
                st = lib.gf_reduce_tile_steady(B, rows, n0, p(eng.d), p(eng.z), p(steady), p(eng.work), p(acc),
                                               1 if k == 0 else 0, stream)
            else:
                st = lib.gf_reduce_tile(B, rows, p(eng.d), p(eng.z), p(eng.work), p(acc), 1 if k == 0 else 0, stream)
            _lib.check(st, "reduce")
        if new:
            st = lib.gf_steady_finish(*finish_head(eng, N, steady, acc), stream)
            _lib.check(st, "gf_steady_finish")
        torch.cuda.synchronize()
        assert np.all(eng.info.cpu().numpy() == 0)
        return acc.cpu().numpy(), steady.cpu().numpy()

    acc_old, hdr_old = route(False)
    acc_new, hdr_new = route(True)
    sw = hdr_new[:, 0].astype(np.int64)
    assert np.array_equal(hdr_old[:, :2], hdr_new[:, :2])           # the same switch rows and frozen pivots
    assert np.all(hdr_new[:, 2] == 0.0) and np.all((sw > 0) & (sw < N - 2 * T)), sw.tolist()
    for b in range(B):
        print(f"problem {b}: switch row {sw[b]}, sum log d {_rel(acc_new[b, 0], acc_old[b, 0]):.2e}, "
              f"sum z^2/d {_rel(acc_new[b, 1], acc_old[b, 1]):.2e}, min d {acc_new[b, 2]!r} / {acc_old[b, 2]!r}")
    assert np.all(np.isfinite(acc_new)) and np.all(np.isfinite(acc_old))
    assert _rel(acc_new[:, 0], acc_old[:, 0]).max() <= 1e-10
    assert _rel(acc_new[:, 1], acc_old[:, 1]).max() <= 1e-10
    assert np.array_equal(acc_new[:, 2], acc_old[:, 2])


def test_mixed_batch_one_walker_never_arms(hip):
    """Two fast walkers and the kernel of tests/test_steady_host.py::test_very_slow_weak_kernel_never_arms: the one
    that never arms goes through the bounded reductions with all its rows -- the plain sweep's bits --, the others
    through the finishing launch."""
    N, T = N_FIN, T_FIN
    t, y = _series(N, seed=37)
    hps = [_fast_terms(2, 0), _fast_terms(2, 1), _two_terms((1e-3, 5.0, 1e5), (2.0, 3000.0, 2.0))]
    ev, coeffs = _evaluator(hps, t, y, T)
    ev.auto_generator_period = False
    got, plain, sw = _steady_and_plain(ev)
    print(f"switch rows {sw.tolist()}, steady vs plain {_rel(got, plain).tolist()}")
    assert sw[2] == -1 and np.all(sw[:2] > 0) and np.all(sw[:2] < N - 2 * T), sw.tolist()
    assert got[2] == plain[2]
    assert _rel(got[:2], plain[:2]).max() <= RTOL_PLAIN
    assert ev.steady_reruns == 0


@pytest.mark.parametrize("case", ["tail shorter than one block", "switch in the last tile"])
def test_short_tail_and_switch_in_the_last_tile(hip, case):
    """Tiles of 1024 rows and an arm_from that puts the switch where the case needs it: the rule fills its ring at the
    16 anchors from arm_from on and counts 4 converged ones, so a factor that has long converged switches at the
    anchor arm_from + 19 * 64 (checked with the rule on the oracle's factor from arm_from on)."""
    from oracle import cref
    T = 1024
    if case == "tail shorter than one block":
        N, anchor = 4 * T, 4 * T - 64           # the tail: rows 4033 .. 4095, 63 of them
    else:
        N, anchor = 5 * T, 4 * T + 256          # the last tile's rows 4353 .. 5119: eleven blocks and 63 rows
    arm = anchor - (LAG + COUNT - 1) * GRID
    assert arm % GRID == 0 and anchor % T != 0
    t, y = _series(N, seed=41)
    hps = [_fast_terms(2, k0) for k0 in range(B_FIN)]
    ev, coeffs = _evaluator(hps, t, y, T)
    for co in coeffs:                           # the oracle's factor puts the switch at `anchor` under this arm_from
        c, a, U, V = cref.get_matrices(co[:6], t, np.full(N, 900.0) + co[6])
        d, W, info = cref.factor(t, c, a, U, V)
        assert info == 0
        row, _, _ = _switch_row(t[arm:], np.asarray(co[5], dtype=np.float64), d[arm:], W[arm:])
        assert arm + row == anchor, (arm, row, anchor)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    ev.engine._steady_axis = (arm, 0.0)
    got, plain, sw = _steady_and_plain(ev)
    print(f"{case}: switch rows {sw.tolist()} of {N}, error vs oracle {_rel(got, ref).max():.2e}, steady vs plain "
          f"{_rel(got, plain).max():.2e}")
    assert np.all(sw == anchor + 1), sw.tolist()
    if case == "tail shorter than one block":
        assert np.all((N - sw > 0) & (N - sw < 64))
    else:
        assert np.all(sw > N - T)
    assert _rel(got, ref).max() <= RTOL_LL
    assert _rel(got, plain).max() <= RTOL_PLAIN
    assert ev.steady_reruns == 0
