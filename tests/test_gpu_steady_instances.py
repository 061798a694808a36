"""GPU: every instance of the steady tail's three kernels -- the STEADY instance of k_factor7,
k_steady_tail<ROWS> and k_steady_finish<ROWS>, ROWS = 4 ceil(2 J / 4) = 4, 8, .. 64 -- at J = 1 .. 31 terms: both
parities of every instance's padding, the instances whose term slots are a multiple of the z phase's group of six
(ROWS = 12, 24, 36, 48, 60) and the eleven that end in a remainder group.  The cases are tests/steady_cases.py's (a
switch forced to row 3968, tiles of 1024 rows, the oracle's exact rows as the reference;
tests/test_steady_instances_host.py shows what that reference is worth), and the kernels are reached through the
documented entry points alone: steady[b][0 .. 2], acc[b][0 .. 2], d, z.

  (a) what ONE finishing launch adds to acc, for every tail of 1 .. 193 rows, against the tail's own sums on the
      oracle's rows -- not diluted by the ~3969 swept rows in front of the switch, as every whole-series total is;
  (b) the rows k_steady_tail stores, tile by tile, against the oracle's forward solve;
  (c) the evaluator's own route at the shortest and the longest tail."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, ARM, B_FIN, J_ALL, LONGEST, N_LONG, RTOL_LL, SW, T, _evaluator, _rel, _run, case
from tests.steady_raw import finish_head, sweep_head
from tests.test_steady_tail_host import RTOL_Z

pytestmark = pytest.mark.gpu
REPEAT = 129            # the tail whose launch runs twice: two full blocks and a row
ULP_LOGD = 4            # acc[b][0]: one rounding of the product k * log d_inf and a device log of up to 2 ulp


@pytest.fixture(scope="module")
def raws(hip):
    """Per J, once: an evaluator on the longest series with tiles of T rows, one evaluate() to pack its coefficients,
    and the arguments of the raw entry points on the engine's own buffers."""
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
        lib, p = eng.lib, _lib.ptr
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        f64 = dict(dtype=torch.float64, device=eng.device)

        def start():
            eng.S_state.zero_()
            eng.F_state.zero_()
            eng.info.zero_()
            eng.d.fill_(float("nan"))
            eng.z.fill_(float("nan"))
            return torch.zeros((eng.B, int(lib.gf_steady_size())), **f64)

        def sweep(entry, steady, n0, rows):
            st = entry(*sweep_head(eng, rows, n0), p(steady), ARM, stream)
            _lib.check(st, "sweep")

        def finish(N, steady, acc):
            st = lib.gf_steady_finish(*finish_head(eng, N, steady, acc), stream)
            _lib.check(st, "gf_steady_finish")

        made[J] = dict(case=c, ev=ev, eng=eng, lib=lib, p=p, f64=f64, stream=stream, start=start, sweep=sweep,
                       finish=finish, check=_lib.check)
        return made[J]
    return get


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


@pytest.mark.parametrize("J", J_ALL)
def test_finish_adds_the_tails_own_sums(raws, J):
    """gf_steady_sweep + gf_reduce_tile_steady tile by tile on the longest series, once; then, for EVERY tail of
    k = 1 .. 193 rows, one gf_steady_finish with N = ANCHOR + 1 + k on a fresh copy of the header and acc = (0, 0, +inf).
    The launch reads rows < N only and the header does not depend on the rows behind the switch, so each is the
    finishing launch of an evaluation of the first N rows, alone, and acc is what it adds:
        acc[b][2] is the frozen pivot d_inf = steady[b][1], bit for bit, the flag stays down, the switch row stays;
        acc[b][0] is k log d_inf to ULP_LOGD ulp;
        |acc[b][1] - sum z_n^2 / d_n| <= 2 RTOL_Z max|z| sum |z_n| / d_inf + RTOL_Z sum z_n^2 / d_n,
    the per-row bar of tests/test_gpu_steady_tail.py (RTOL_Z of max |z| over the whole series) carried to the sum: with
    z~ = z + e, |e| <= RTOL_Z max|z|, the sum of z~^2 moves by at most 2 max|e| sum |z_n| (e^2 is below the rounding),
    and d_inf for d_n by far less than the second term (the host file's tail-share cap, 1e-11).  The launch of a tail of
    129 rows gives the same bits twice, and front + tail of the longest series through gf_loglike_finish is the oracle's
    log-likelihood to RTOL_LL."""
    import torch
    r = raws(J)
    c, eng, lib, p, B = r["case"], r["eng"], r["lib"], r["p"], B_FIN
    steady = r["start"]()
    acc = torch.full((B, 3), float("nan"), **r["f64"])
    for k, n0 in enumerate(range(0, N_LONG, T)):
        rows = min(T, N_LONG - n0)
        r["sweep"](lib.gf_steady_sweep, steady, n0, rows)
        st = lib.gf_reduce_tile_steady(B, rows, n0, p(eng.d), p(eng.z), p(steady), p(eng.work), p(acc),
                                       1 if k == 0 else 0, r["stream"])
        r["check"](st, "gf_reduce_tile_steady")
    torch.cuda.synchronize()
    acc_front, hdr0 = acc.clone(), steady.clone()
    hdr = hdr0.cpu().numpy()
    assert np.all(eng.info.cpu().numpy() == 0)
    assert np.all(hdr[:, 0] == ANCHOR + 1), hdr[:, 0].tolist()
    assert np.all(hdr[:, 2] == 0.0)
    dinf = hdr[:, 1].copy()
    derr = np.abs(dinf - c.d[:, ANCHOR]) / c.d[:, ANCHOR]
    assert derr.max() <= 1e-10, derr.tolist()            # the rule's own threshold (include/gadfly_hip.h)

    # every tail in a header and an acc of its own, the repeat in the last slot; one synchronisation for all of them
    tails = list(range(1, LONGEST + 1)) + [REPEAT]
    hdrs = hdr0.unsqueeze(0).repeat(len(tails), 1, 1).contiguous()
    accs = torch.tensor([0.0, 0.0, float("inf")], **r["f64"]).repeat(len(tails), B, 1).contiguous()
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
            assert ulp <= ULP_LOGD, (what, got[i, b, 0], k * np.log(dinf[b]))
            assert err <= bar, (what, got[i, b, 1], s.z2d[k - 1], err / bar)
    assert np.array_equal(got[-1], got[REPEAT - 1]), (got[-1].tolist(), got[REPEAT - 1].tolist())

    total = acc_front.clone()
    total[:, :2] += accs[LONGEST - 1, :, :2]
    total[:, 2] = torch.minimum(total[:, 2], accs[LONGEST - 1, :, 2])
    out = torch.empty((B,), **r["f64"])
    r["check"](lib.gf_loglike_finish(B, N_LONG, p(total), p(eng.info), p(out), None, r["stream"]), "gf_loglike_finish")
    torch.cuda.synchronize()
    ll = _rel(out.cpu().numpy(), c.loglike).max()
    print(f"J = {J:2d} (ROWS = {(2 * J + 3) // 4 * 4:2d}): tail sum z^2/d error / bar {worst:.1e} at a tail of "
          f"{worst_at[0]} rows (problem {worst_at[1]}), k log d_inf {worst_ulp:.1f} ulp, d_inf against the oracle's "
          f"pivot {derr.max():.1e}, front + tail against the oracle {ll:.1e}")
    assert ll <= RTOL_LL


@pytest.mark.parametrize("J", J_ALL)
def test_tail_kernel_rows(raws, J):
    """gf_loglike_steady tile by tile on the longest series, d and z full of NaN in front of every tile: the tail, rows
    3969 .. 4161, ends tile 3 with one full block and 63 rows and enters tile 4 with one full block and 2 rows.  Behind
    the switch row z is the oracle's forward solve to RTOL_Z max|z| and d the frozen pivot of slot [1] on every row;
    the rows in front of it are finite; the flag stays down."""
    import torch
    r = raws(J)
    c, eng, lib, B = r["case"], r["eng"], r["lib"], B_FIN
    steady = r["start"]()
    z, d = np.empty((B, N_LONG)), np.empty((B, N_LONG))
    for n0 in range(0, N_LONG, T):
        rows = min(T, N_LONG - n0)
        eng.d.fill_(float("nan"))
        eng.z.fill_(float("nan"))
        r["sweep"](lib.gf_loglike_steady, steady, n0, rows)
        torch.cuda.synchronize()
        z[:, n0:n0 + rows] = eng.z.reshape(-1)[:B * rows].view(B, rows).cpu().numpy()
        d[:, n0:n0 + rows] = eng.d.reshape(-1)[:B * rows].view(B, rows).cpu().numpy()
    hdr = steady.cpu().numpy()
    assert np.all(eng.info.cpu().numpy() == 0)
    assert np.all(hdr[:, 0] == SW), hdr[:, 0].tolist()
    assert np.all(hdr[:, 2] == 0.0)
    assert np.all(np.isfinite(z[:, :SW])) and np.all(np.isfinite(d[:, :SW]))
    errs = []
    for b in range(B):
        errs.append(np.max(np.abs(z[b, SW:] - c.z[b, SW:])) / c.zmax[b])
        assert np.all(d[b, SW:] == hdr[b, 1]), (J, b)
    print(f"J = {J:2d} (ROWS = {(2 * J + 3) // 4 * 4:2d}): tail z error {max(errs):.2e} max|z|")
    assert max(errs) <= RTOL_Z, (J, errs)


@pytest.mark.parametrize("J", J_ALL)
def test_evaluator_route(hip, J):
    """BatchedLogLikelihood.evaluate() with the switch forced to ANCHOR, as tests/test_gpu_steady_fold.py runs it, at
    the shortest and the longest tail: the engine reaches the same instances with its own arguments."""
    c = case(J)
    for tail in (1, LONGEST):
        _run(c.hps, c.t, c.y, tail, f"J = {J}, tail of {tail} rows")
