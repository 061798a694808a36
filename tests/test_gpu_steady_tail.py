"""GPU: the steady tail as a block filter (k_steady_tail behind the sweep instance of gf_loglike_steady, DESIGN.md
3.10): the narrowest, the flagship's and the widest instance with the switch inside a tile, later tiles entered in
the tail and a partial last block, against the oracle and against the plain sweep; the raw entry point tile by tile
(tail rows of z against the oracle's forward solve, d frozen); the violation flag from a stamp at the first, a
middle and the last row of a block and in the partial last block."""
import numpy as np
import pytest

from tests.random_cases import oracle_loglikes
from tests.steady_raw import sweep_head
from tests.test_gpu_steady import RTOL_LL, _evaluator, _fast_terms, _rel, _series

pytestmark = pytest.mark.gpu
N_TAIL, T_TAIL = 16384 + 37, 4096       # four full tiles and one of 37 rows: a partial last block


@pytest.mark.parametrize("J", [1, 30, 31])
def test_tail_kernel_instances_against_oracle_and_plain_sweep(hip, J):
    N, T = N_TAIL, T_TAIL
    t, y = _series(N, seed=23)
    hps = [_fast_terms(J, k0) for k0 in range(3)]
    ev, coeffs = _evaluator(hps, t, y, T)
    eng = ev.engine
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    got = ev.evaluate()
    sw = eng.steady_switch_rows()
    used = int(eng.generator_period)
    assert eng.steady_used and eng.kernel_used == "fused" and eng.tile_rows == T
    eng.steady_state = False
    ev.auto_generator_period, eng.generator_period = False, used
    plain = ev.evaluate()
    assert not eng.steady_used
    print(f"J = {J}, period {used}: switch rows {sw.tolist()}, error vs oracle {_rel(got, ref).max():.2e} (plain sweep "
          f"{_rel(plain, ref).max():.2e}), steady vs plain {_rel(got, plain).max():.2e}")
    assert np.all((sw > 0) & (sw < N)), sw.tolist()
    # the switch inside a tile (the anchor is never a tile's first row) and at least two tiles entered in the tail
    assert np.all((sw - 1) % T != 0) and np.all(sw < N - 2 * T), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert _rel(got, plain).max() <= 1e-10
    assert ev.steady_reruns == 0


def test_raw_entry_point_tile_by_tile(hip):
    """gf_loglike_steady on the evaluator's own buffers, one tile at a time: behind each problem's switch row z is the
    oracle's forward solve to 1e-9 max|z| and d is the frozen pivot of slot [1] on every row."""
    import torch
    from gadfly_amd import _lib
    from oracle import cref
    N, T, J = 8192, 2048, 2
    t, y = _series(N, seed=29)
    hps = [_fast_terms(J, k0) for k0 in range(3)]
    ev, coeffs = _evaluator(hps, t, y, T)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    ev.evaluate()                           # (packs the coefficients; its own result is not used)
    lib, p, B = eng.lib, _lib.ptr, eng.B
    steady = torch.zeros((B, int(lib.gf_steady_size())), dtype=torch.float64, device=eng.device)
    eng.S_state.zero_()
    eng.F_state.zero_()
    eng.info.zero_()
    z, d = np.empty((B, N)), np.empty((B, N))
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    for n0 in range(0, N, T):
        st = lib.gf_loglike_steady(*sweep_head(eng, T, n0), p(steady), 0, stream)
        _lib.check(st, "gf_loglike_steady")
        torch.cuda.synchronize()
        z[:, n0:n0 + T] = eng.z.reshape(-1)[:B * T].view(B, T).cpu().numpy()
        d[:, n0:n0 + T] = eng.d.reshape(-1)[:B * T].view(B, T).cpu().numpy()
    hdr = steady.cpu().numpy()
    assert np.all(eng.info.cpu().numpy() == 0) and np.all(hdr[:, 2] == 0.0)
    sw = hdr[:, 0].astype(np.int64)
    assert np.all((sw > 0) & (sw < N - 2 * T)), sw.tolist()
    for b in range(B):
        co = coeffs[b]
        c, a, U, V = cref.get_matrices(co[:6], t, np.full(N, 900.0) + co[6])
        dd, W, info = cref.factor(t, c, a, U, V)
        assert info == 0
        zz = cref.solve_lower(t, c, U, W, y)
        err = np.max(np.abs(z[b, sw[b]:] - zz[sw[b]:])) / np.max(np.abs(zz))
        print(f"problem {b}: switch row {sw[b]}, tail z error {err:.2e} max|z|, "
              f"d_inf against the oracle's last pivot {abs(hdr[b, 1] - dd[-1]) / dd[-1]:.2e}")
        assert err <= 1e-9
        assert np.all(d[b, sw[b]:] == hdr[b, 1])


@pytest.mark.parametrize("where", ["first row of a block", "row 31 of a block", "last row of a block",
                                   "partial last block"])
def test_one_moved_stamp_raises_the_flag(hip, where):
    """One stamp moved by 10 jthr (jthr = 2e-6 / wmax, the generator's own test) behind every problem's switch row,
    in a tile that is entered in the tail (its blocks start at the tile's first row for every problem): the flag of
    every problem, and resolve() repeats them all without the mode."""
    N, T = N_TAIL, T_TAIL
    off = {"first row of a block": 0, "row 31 of a block": 31, "last row of a block": 63}.get(where)
    row = 2 * T + 3 * 64 + off if off is not None else 4 * T + 20
    t, y = _series(N, seed=31)
    hps = [_fast_terms(2, k0) for k0 in range(3)]
    ev, coeffs = _evaluator(hps, t, y, T)
    wmax = float(ev.engine._pack.wmax)
    t = t.copy()
    t[row] += 10.0 * 2e-6 / wmax
    ev, coeffs = _evaluator(hps, t, y, T)
    eng = ev.engine
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    eng._steady_axis = (0, 0.0)             # (the evaluator's own axis scan would arm behind the moved stamp only)
    out = ev.evaluate_device()
    sw = eng.steady_switch_rows()
    viol = eng.steady_violations().cpu().numpy()
    assert eng.steady_used and np.all((sw > 0) & (sw < 2 * T)), sw.tolist()
    assert viol.all(), (viol.tolist(), sw.tolist())
    assert ev.resolve() == 3 and ev.steady_reruns == 3
    got = out.cpu().numpy()
    print(f"{where} (row {row}): switch rows {sw.tolist()}, after the repeat {_rel(got, ref).max():.2e} vs oracle")
    assert _rel(got, ref).max() <= RTOL_LL
