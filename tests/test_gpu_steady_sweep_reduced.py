"""GPU: the steady sweep that adds its own tile to acc (gf_steady_sweep_reduced) against the two calls
it stands for, gf_steady_sweep + gf_reduce_tile_steady, at the raw entry points -- bit for bit: acc (prefilled with
NaN, so `init` shows), the steady buffer, info, the handed-over state, and the rows d and z.

Route A runs the two calls on every tile; route B the two calls on the tiles in front of tile k and the one call from
tile k on.  On tests/test_gpu_steady_overlap.py's batch, whose four walkers switch in tiles 0, 1, 2 and 0 of 4096 rows
(J = 30, and J = 3), over N = 16384 + 37 rows -- the last tile has 37 --, k = 0, 1, 2; on tilings whose second tile has
300, 1000 and 4096 + 37 rows (one group of the reduction and not a full one; a length that is no multiple of 64 or
256; two groups, the second one of 37 rows); with a walker's switch inside a tile of 300 rows (fewer than 256 rows in
front of it); and on tests/test_gpu_steady.py's walker that is not positive definite, whose pivot fails inside a
reduced tile and which enters the later ones with info != 0."""
import numpy as np
import pytest

from tests.steady_raw import sweep_head
from tests.test_gpu_steady import _evaluator, _fast_terms, _series
from tests.test_gpu_steady_finish import N_FIN, T_FIN
from tests.test_gpu_steady_overlap import _oracle_tiles, _spread_batch

pytestmark = pytest.mark.gpu
KEYS = ("acc", "steady", "info", "S_state", "F_state", "d", "z")


def _uniform(N, T):
    return [(n0, min(T, N - n0)) for n0 in range(0, N, T)]


class _Raw:
    """The raw entry points on an evaluator's buffers; d, z and work of its own, sized for the longest tile."""

    def __init__(self, ev, max_rows):
        import torch
        from gadfly_amd import _lib
        self.torch, self._lib = torch, _lib
        eng = self.eng = ev.engine
        ev.auto_generator_period, eng.generator_period = False, 1
        ev.evaluate()                       # (packs the coefficients; its own result is not used)
        self.lib, self.p, self.B = eng.lib, _lib.ptr, eng.B
        self.f64 = dict(dtype=torch.float64, device=eng.device)
        self.max_rows = max_rows
        self.stream = torch.cuda.current_stream(eng.device).cuda_stream

    def run(self, tiling, reduced_from, arm_from=0):
        """The tiles (n_first, rows) in order; the one call from tile `reduced_from` on (None: never)."""
        torch, eng, lib, p, B = self.torch, self.eng, self.lib, self.p, self.B
        steady = torch.zeros((B, int(lib.gf_steady_size())), **self.f64)
        acc = torch.full((B, 3), float("nan"), **self.f64)
        d = torch.full((B * self.max_rows,), float("nan"), **self.f64)
        z = torch.full((B * self.max_rows,), float("nan"), **self.f64)
        work = torch.full((B * int(lib.gf_reduce_work(self.max_rows)),), float("nan"), **self.f64)
        eng.S_state.zero_()
        eng.F_state.zero_()
        eng.info.zero_()
        for k, (n0, rows) in enumerate(tiling):
            assert 0 < rows <= self.max_rows and n0 + rows <= eng.N
            args = (*sweep_head(eng, rows, n0, d=p(d), z=p(z)), p(steady), arm_from)
            init = 1 if k == 0 else 0
            if reduced_from is not None and k >= reduced_from:
                self._lib.check(lib.gf_steady_sweep_reduced(*args, p(acc), init, self.stream), "gf_steady_sweep_reduced")
            else:
                self._lib.check(lib.gf_steady_sweep(*args, self.stream), "gf_steady_sweep")
                self._lib.check(lib.gf_reduce_tile_steady(B, rows, n0, p(d), p(z), p(steady), p(work), p(acc), init,
                                                          self.stream), "gf_reduce_tile_steady")
        torch.cuda.synchronize()
        got = dict(acc=acc, steady=steady, info=eng.info, S_state=eng.S_state, F_state=eng.F_state, d=d, z=z)
        return {k: v.cpu().numpy().copy() for k, v in got.items()}


def _assert_same(got, want, what):
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


@pytest.fixture(scope="module")
def spread(hip):
    """raw(J): the four-walker batch on N_FIN rows and route A on tiles of T_FIN rows, once per J."""
    made = {}

    def raw(J):
        if J not in made:
            t, y = _series(N_FIN, seed=29)
            hps, want = _spread_batch(J)
            ev, coeffs = _evaluator(hps, t, y, T_FIN)
            r = _Raw(ev, T_FIN + 37)
            a = r.run(_uniform(N_FIN, T_FIN), None)
            sw = a["steady"][:, 0].astype(np.int64)
            print(f"J = {J}: switch rows {sw.tolist()}")
            assert np.all(a["info"] == 0) and np.all(np.isfinite(a["acc"]))
            if J == 30:
                assert _oracle_tiles(coeffs, t, T_FIN) == want and ((sw - 1) // T_FIN).tolist() == want
            made[J] = (r, a, sw)
        return made[J]

    return raw


@pytest.mark.parametrize("J", [30, 3])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_call_from_tile_k_on_gives_the_two_calls_bits(spread, J, k):
    r, a, sw = spread(J)
    b = r.run(_uniform(N_FIN, T_FIN), k)
    _assert_same(b, a, f"J = {J}, reduced from tile {k}")
    if J == 30:
        # tiles k .. 2 each hold a problem that switches inside them, and from tile 1 on problems that had switched
        assert np.all(sw % 64 == 1) and np.all((sw - 1) % T_FIN > 0)


@pytest.mark.parametrize("rows", [300, 1000, T_FIN + 37])
def test_tile_lengths_of_one_group_odd_rows_and_two_groups(spread, rows):
    r, _, sw = spread(30)
    tiling = [(0, T_FIN), (T_FIN, rows)]
    a = r.run(tiling, None)
    assert np.all(a["info"] == 0)
    stored = np.clip(np.where(a["steady"][:, 0] > 0, a["steady"][:, 0] - T_FIN, rows), 0, rows)
    print(f"second tile of {rows} rows: rows stored per problem {stored.tolist()}")
    assert (stored == rows).any() and (stored == 0).any()          # a whole tile, and a problem that had switched
    if rows > T_FIN:
        assert ((stored > 0) & (stored < rows)).any()               # and a switch inside it
    for k in (0, 1):
        _assert_same(r.run(tiling, k), a, f"second tile of {rows} rows, reduced from tile {k}")


def test_switch_inside_a_short_tile(spread):
    """Walker 1's switch row 65 rows into a tile of 300: fewer rows in front of it than one group of the reduction."""
    r, _, sw = spread(30)
    n0 = int(sw[1]) - 1 - 64
    assert n0 > T_FIN and n0 % 64 == 0
    tiling = [(0, n0), (n0, 300)]
    r2 = _Raw.__new__(_Raw)
    r2.__dict__.update(r.__dict__)
    r2.max_rows = n0
    a = r2.run(tiling, None)
    assert int(a["steady"][1, 0]) == int(sw[1]), (a["steady"][:, 0].tolist(), sw.tolist())
    for k in (0, 1):
        _assert_same(r2.run(tiling, k), a, f"switch 65 rows into a tile of 300, reduced from tile {k}")


def test_failing_problem_takes_what_the_reduction_takes(hip):
    """tests/test_gpu_steady.py::test_failing_walker_reports_its_row's batch: walker 2 is not positive definite.  Its
    pivot fails inside a tile and it enters the later ones with info != 0; acc (NaN or not) as the two calls leave it."""
    import gadfly_amd
    N, T = 8192, 1024
    t, y = _series(N, seed=17)
    kernels = [gadfly_amd.StellarOscillatorKernel(_fast_terms(2, k0), texp=60.0) for k0 in range(4)]
    diag = np.full((4, N), 900.0)
    diag[2] = -0.5 * float(np.sum(kernels[2].get_device_coefficients()[2]))
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag, tile_rows=T)
    ev.engine.force_streaming = True
    r = _Raw(ev, T)
    a = r.run(_uniform(N, T), None)
    bad = int(a["info"][2])
    print(f"info {a['info'].tolist()}, switch rows {a['steady'][:, 0].tolist()}, acc of the failing walker {a['acc'][2].tolist()}")
    assert bad > 0 and np.all(a["info"][[0, 1, 3]] == 0) and np.all(a["steady"][[0, 1, 3], 0] > 0)
    k_fail = (bad - 1) // T
    assert k_fail < N // T - 1                                      # tiles behind it: entered with info != 0
    for k in sorted({0, k_fail, k_fail + 1}):
        _assert_same(r.run(_uniform(N, T), k), a, f"failing walker, reduced from tile {k}")


def test_argument_errors(spread):
    r, a, _ = spread(3)
    eng, lib, p = r.eng, r.lib, r.p
    acc = r.torch.full((r.B, 3), float("nan"), **r.f64)
    steady = r.torch.zeros((r.B, int(lib.gf_steady_size())), **r.f64)

    def call(**over):
        v = dict(steady=p(steady), acc=p(acc), rows=64, n0=0)
        v.update(over)
        head = sweep_head(eng, v["rows"], v["n0"], diag=None, diag_bs=0)
        return lib.gf_steady_sweep_reduced(*head, v["steady"], 0, v["acc"], 1, r.stream)

    for over, text in [(dict(acc=None), "null pointer"), (dict(steady=None), "null pointer"),
                       (dict(rows=0), "empty problem"), (dict(n0=-64), "n_first")]:
        assert call(**over) != 0, over
        msg = r._lib.last_error()
        assert msg.startswith("gf_steady_sweep_reduced:") and text in msg, msg
    r.torch.cuda.synchronize()
    assert np.all(np.isnan(acc.cpu().numpy()))                      # no launch went through
