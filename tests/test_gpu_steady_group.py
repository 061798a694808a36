"""GPU: the group phase of the steady tail's finishing launch (k_steady_finish): u = H y of 16 blocks
at once on the matrix pipe.  The cases of tests/test_gpu_steady_instances.py (a) on the longer series of
tests/steady_group_cases.py -- a switch forced to ANCHOR, tiles of T rows, the oracle's exact rows as the reference
(tests/test_steady_group_host.py shows what that reference is worth there) -- with tails that cross the group
boundaries, at the narrowest instances, the flagship's and the widest, through the raw entry points:

  - what ONE finishing launch adds to acc, at tails of a lone partial block, exactly one group, a group and a row, a
    partial group of one block and of one block and a row, two groups, past two groups, and their neighbours;
  - the same bits from a repeated launch, from two disjoint windows, and whether the rows behind N hold the series'
    continuation or NaN (shared y and one y per problem): no operand load of the phase leaves the series;
  - the evaluator's own route at a group and a row and at the longest tail."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, ARM, B_FIN, RTOL_LL, SW, T, _evaluator, _rel, _run
from tests.steady_group_cases import J_GROUP, LONGEST_G, N_G, TAILS_G, case
from tests.steady_raw import finish_head, sweep_head
from tests.test_gpu_steady_instances import ULP_LOGD, _ulps
from tests.test_steady_tail_host import RTOL_Z

pytestmark = pytest.mark.gpu
REPEAT = 1089           # the tail whose launch runs twice: a group, a block and a row


@pytest.fixture(scope="module")
def raws(hip):
    """Per J, once: an evaluator on the long series with tiles of T rows, gf_steady_sweep + gf_reduce_tile_steady tile by
    tile, and the header and acc in front of the finishing launches; finish() is one launch on the engine's buffers,
    with another y on request."""
    import torch
    from gadfly_amd import _lib
    made = {}

    def get(J):
        if J in made:
            return made[J]
        c = case(J)
        ev, _ = _evaluator(c.hps, c.t, c.y, T)
        eng = ev.engine
        ev.auto_generator_period, eng.generator_period = False, 1
        ev.evaluate()                       # (packs the coefficients; its own result is not used)
        assert eng.B == B_FIN and eng.Jr == 0 and eng.Jc == J and eng.tile_rows == T
        lib, p, B = eng.lib, _lib.ptr, eng.B
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        f64 = dict(dtype=torch.float64, device=eng.device)
        eng.S_state.zero_()
        eng.F_state.zero_()
        eng.info.zero_()
        eng.d.fill_(float("nan"))
        eng.z.fill_(float("nan"))
        steady = torch.zeros((B, int(lib.gf_steady_size())), **f64)
        acc = torch.full((B, 3), float("nan"), **f64)
        for k, n0 in enumerate(range(0, N_G, T)):
            rows = min(T, N_G - n0)
            st = lib.gf_steady_sweep(*sweep_head(eng, rows, n0), p(steady), ARM, stream)
            _lib.check(st, "gf_steady_sweep")
            st = lib.gf_reduce_tile_steady(B, rows, n0, p(eng.d), p(eng.z), p(steady), p(eng.work), p(acc),
                                           1 if k == 0 else 0, stream)
            _lib.check(st, "gf_reduce_tile_steady")
        torch.cuda.synchronize()
        hdr = steady.cpu().numpy()
        assert np.all(eng.info.cpu().numpy() == 0)
        assert np.all(hdr[:, 0] == SW), hdr[:, 0].tolist()
        assert np.all(hdr[:, 2] == 0.0)

        def finish(N, hdr_, acc_, y=None, y_bs=None, window=None):
            head = finish_head(eng, N, hdr_, acc_, y=y, y_bs=y_bs)
            if window is None:
                _lib.check(lib.gf_steady_finish(*head, stream), "gf_steady_finish")
            else:
                _lib.check(lib.gf_steady_finish_window(*head, int(window[0]), int(window[1]), stream),
                           "gf_steady_finish_window")

        def fresh(n):
            """n headers as the sweep left them and n accs of (0, 0, +inf)"""
            return (steady.unsqueeze(0).repeat(n, 1, 1).contiguous(),
                    torch.tensor([0.0, 0.0, float("inf")], **f64).repeat(n, B, 1).contiguous())

        made[J] = dict(case=c, eng=eng, lib=lib, p=p, f64=f64, stream=stream, hdr=hdr, acc_front=acc, finish=finish,
                       fresh=fresh, check=_lib.check)
        return made[J]
    return get


@pytest.mark.parametrize("J", J_GROUP)
def test_finish_adds_the_tails_own_sums_across_groups(raws, J):
    """tests/test_gpu_steady_instances.py::test_finish_adds_the_tails_own_sums at the tails of TAILS_G: for each, one
    gf_steady_finish with N = ANCHOR + 1 + k on a fresh header and acc = (0, 0, +inf):
        acc[b][2] is the frozen pivot d_inf = steady[b][1], bit for bit, the flag stays down, the switch row stays;
        acc[b][0] is k log d_inf to ULP_LOGD ulp;
        |acc[b][1] - sum z_n^2 / d_n| <= 2 RTOL_Z max|z| sum |z_n| / d_inf + RTOL_Z sum z_n^2 / d_n.
    The launch of a tail of 1089 rows gives the same bits twice, and front + tail of the longest series through
    gf_loglike_finish is the oracle's log-likelihood to RTOL_LL."""
    import torch
    r = raws(J)
    c, eng, lib, p, B = r["case"], r["eng"], r["lib"], r["p"], B_FIN
    hdr = r["hdr"]
    dinf = hdr[:, 1].copy()
    derr = np.abs(dinf - c.d[:, ANCHOR]) / c.d[:, ANCHOR]
    assert derr.max() <= 1e-10, derr.tolist()            # the rule's own threshold (include/gadfly_hip.h)

    tails = list(TAILS_G) + [REPEAT]
    hdrs, accs = r["fresh"](len(tails))
    for i, k in enumerate(tails):
        r["finish"](ANCHOR + 1 + k, hdrs[i], accs[i])
    torch.cuda.synchronize()
    assert np.all(eng.info.cpu().numpy() == 0)
    got, after = accs.cpu().numpy(), hdrs.cpu().numpy()

    worst, worst_at, worst_ulp = 0.0, None, 0.0
    for i, k in enumerate(tails):
        for b in range(B):
            what = f"J = {J}, tail of {k} rows, problem {b}"
            assert got[i, b, 2] == dinf[b], what
            assert after[i, b, 2] == 0.0, what
            assert after[i, b, 0] == ANCHOR + 1 and after[i, b, 1] == dinf[b], what
            ulp = _ulps(got[i, b, 0], k * np.log(dinf[b]))
            s = c.sums[b]
            err = abs(got[i, b, 1] - s.z2d[k - 1])
            bar = 2.0 * RTOL_Z * c.zmax[b] * s.zabs[k - 1] / dinf[b] + RTOL_Z * s.z2d[k - 1]
            if err / bar > worst:
                worst, worst_at = err / bar, (k, b)
            worst_ulp = max(worst_ulp, ulp)
            print(f"{what}: sum z^2/d error / bar {err / bar:.1e}, k log d_inf {ulp:.1f} ulp")
            assert ulp <= ULP_LOGD, (what, got[i, b, 0], k * np.log(dinf[b]))
            assert err <= bar, (what, got[i, b, 1], s.z2d[k - 1], err / bar)
    assert np.array_equal(got[-1], got[tails.index(REPEAT)]), (got[-1].tolist(), got[tails.index(REPEAT)].tolist())
    assert np.array_equal(after[-1], after[tails.index(REPEAT)])

    last = tails.index(LONGEST_G)
    total = r["acc_front"].clone()
    total[:, :2] += accs[last, :, :2]
    total[:, 2] = torch.minimum(total[:, 2], accs[last, :, 2])
    out = torch.empty((B,), **r["f64"])
    r["check"](lib.gf_loglike_finish(B, N_G, p(total), p(eng.info), p(out), None, r["stream"]), "gf_loglike_finish")
    torch.cuda.synchronize()
    ll = _rel(out.cpu().numpy(), c.loglike).max()
    print(f"J = {J:2d} (ROWS = {(2 * J + 3) // 4 * 4:2d}): tail sum z^2/d error / bar {worst:.1e} at a tail of "
          f"{worst_at[0]} rows (problem {worst_at[1]}), k log d_inf {worst_ulp:.1f} ulp, front + tail against the "
          f"oracle {ll:.1e}")
    assert ll <= RTOL_LL


@pytest.mark.parametrize("shared", [True, False], ids=["shared-y", "y-per-problem"])
@pytest.mark.parametrize("J", J_GROUP)
def test_rows_behind_the_series_are_never_read(raws, J, shared):
    """A y buffer longer than N: acc and the header are bit-identical whether the rows from N on hold the series'
    continuation or NaN, at every tail of TAILS_G -- with one y for all problems (batch stride 0) and with one per
    problem.  An operand load of the group phase (or a look-ahead) that is not clamped to row N - 1 reads a NaN into
    a column of U, a row of z and the sum."""
    import torch
    r = raws(J)
    c, B = r["case"], B_FIN
    y = torch.tensor(c.y, **r["f64"])
    if not shared:
        y = y.unsqueeze(0).repeat(B, 1).contiguous()
    y_bs = 0 if shared else N_G
    tails = [k for k in TAILS_G if k < LONGEST_G]
    res = []
    for poison in (False, True):
        hdrs, accs = r["fresh"](len(tails))
        ys = []
        for i, k in enumerate(tails):
            yk = y
            if poison:
                yk = y.clone()
                yk[..., ANCHOR + 1 + k:] = float("nan")
                ys.append(yk)                   # (alive until the launches are through)
            r["finish"](ANCHOR + 1 + k, hdrs[i], accs[i], y=yk, y_bs=y_bs)
        torch.cuda.synchronize()
        res.append((accs.cpu().numpy(), hdrs.cpu().numpy()))
    assert np.all(np.isfinite(res[0][0][..., :2])) and np.all(res[0][0][..., 1] > 0.0)
    for i, k in enumerate(tails):
        assert np.array_equal(res[0][0][i], res[1][0][i]), (J, k, res[0][0][i].tolist(), res[1][0][i].tolist())
        assert np.array_equal(res[0][1][i], res[1][1][i]), (J, k)


@pytest.mark.parametrize("J", J_GROUP)
def test_two_windows_give_the_single_launch(raws, J):
    """gf_steady_finish_window over two disjoint windows that cover [1, N], in either order, against one
    gf_steady_finish on the longest tail, bit for bit: the groups of a problem start at its own switch row, whichever
    launch takes it."""
    import torch
    r = raws(J)
    layouts = [None, [(1, SW), (SW, N_G + 1)], [(SW, N_G + 1), (1, SW)], [(1, SW + 1), (SW + 1, N_G + 1)],
               [(SW + 1, N_G + 1), (0, SW + 1)]]
    hdrs, accs = r["fresh"](len(layouts))
    for i, layout in enumerate(layouts):
        for window in ([None] if layout is None else layout):
            r["finish"](N_G, hdrs[i], accs[i], window=window)
    torch.cuda.synchronize()
    got, after = accs.cpu().numpy(), hdrs.cpu().numpy()
    assert np.all(np.isfinite(got[0])) and np.all(got[0][:, 1] > 0.0)
    for i, layout in enumerate(layouts[1:], start=1):
        assert np.array_equal(got[i], got[0]), (J, layout)
        assert np.array_equal(after[i], after[0]), (J, layout)


@pytest.mark.parametrize("J", J_GROUP)
def test_evaluator_route_across_groups(hip, J):
    """BatchedLogLikelihood.evaluate() with the switch forced to ANCHOR (tests/steady_cases.py::_run: against the oracle
    at RTOL_LL and against the plain sweep at RTOL_PLAIN) at a tail of a group and a row and at the longest tail."""
    c = case(J)
    for tail in (1025, LONGEST_G):
        _run(c.hps, c.t, c.y, tail, f"J = {J}, tail of {tail} rows")
