"""GPU: the four-row state step of the steady tail's finishing block (k_steady_finish / k_steady_chunk)
through the raw entry points, on the cases of tests/steady_cases.py: the switch forced to row 3968, series of at most
4162 rows, tiles of 1024 rows.

tests/test_gpu_steady_instances.py bars the sums a finishing launch adds at every tail of 1 .. 193 rows and every J;
what it cannot see is the state update of the LAST full block, whose result no row behind it reads.  This file checks
the END STATE the launch leaves in the header, (s_r, s_i) at words 72 and 104, at tails of 64, 65, 96, 127, 128, 129,
192 and 193 rows (one to three full blocks, with and without a partial block behind them, whose rolled loop takes
four-row trips and then single rows) and J = 1, 2, 15, 29, 30, 31.

Reference: the frozen row form in longdouble (tests/steady_cases.py::row_form, restated here so that it returns the
state), run from what the header itself holds in front of the launch -- the state at the switch row, the gain G, the
cadence Delta -- and the kernel's coefficients, on the series' own rows.  Distance: max over the terms of |s - s_ref|,
over max |s_ref|.

Bar: the parent commit's library (two-row steps, lambda^32 by squarings in double), loaded through GADFLY_SO, measured
on exactly these cases against this reference: worst distance 1.05e-15 (J = 29, a tail of 127 rows; per J = 1, 2, 15,
29, 30, 31: 4.02e-16, 7.72e-16, 6.57e-16, 1.05e-15, 8.11e-16, 9.87e-16).  BAR = 4 x 1.05e-15 = 4.2e-15: the cases differ
in J and the four-row form has fewer roundings on the chain, not more.  This tree measures 8.49e-16, 6.35e-16, 5.18e-16,
1.01e-15, 8.73e-16 and 9.87e-16 (J = 31, ROWS = 64, keeps the two-row step and the parent's bits).

Further: the launch of 129 rows twice, bit for bit; one chunked launch (gf_steady_finish_chunked, 16-block chunks) on
the 2113-row tail of tests/steady_group_cases.py at J = 2 and 30 against the one-wave launch, within
tests/test_gpu_steady_chunk.py's bars; two disjoint windows against one launch, bit for bit."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, ARM, B_FIN, N_LONG, SW, T, _evaluator, case
from tests.steady_group_cases import LONGEST_G, N_G
from tests.steady_raw import finish_head, sweep_head
from tests.test_gpu_steady_chunk import _against_plain, _chunked
from tests.test_gpu_steady_group import raws  # noqa: F401  (the module fixture of the raw entry points, long series)

pytestmark = pytest.mark.gpu
TAILS = (64, 65, 96, 127, 128, 129, 192, 193)
REPEAT = 129
J_CASES = (1, 2, 15, 29, 30, 31)
PARENT_WORST = 1.05e-15     # the parent commit's library on these cases against this reference (docstring)
BAR = 4.0 * PARENT_WORST
ST_DT, ST_GR, ST_GI, ST_SR, ST_SI = 6, 8, 40, 72, 104      # the header's words (gadfly_hip.hip)


def _row_form_state(alpha, expo, G, s, ytail):
    """tests/steady_cases.py::row_form in longdouble, returning the state behind the last row of ytail."""
    cld = np.clongdouble
    alpha, G, s = alpha.astype(cld), G.astype(cld), s.astype(cld)
    lam = np.exp(-expo.astype(cld))
    for yn in ytail:
        x = lam * s
        zn = np.longdouble(yn) - np.sum((alpha * x).real)
        s = x + G * zn
    return s


def _header_frozen(hdr_b, co, J):
    """What the launch starts from, read from a problem's header and coefficients."""
    ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in co[2:6])
    assert len(ac) == J
    return dict(alpha=ac + 1j * bc, expo=(cc + 1j * dc) * hdr_b[ST_DT],
                G=hdr_b[ST_GR:ST_GR + J] + 1j * hdr_b[ST_GI:ST_GI + J],
                s=hdr_b[ST_SR:ST_SR + J] + 1j * hdr_b[ST_SI:ST_SI + J])


@pytest.mark.parametrize("J", J_CASES)
def test_end_state_against_the_longdouble_row_form(hip, J):
    import torch
    from gadfly_amd import _lib
    c = case(J)
    ev, _ = _evaluator(c.hps, c.t, c.y, T)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    ev.evaluate()                           # (packs the coefficients; its own result is not used)
    assert eng.B == B_FIN and eng.Jr == 0 and eng.Jc == J and eng.tile_rows == T
    lib, p, B = eng.lib, _lib.ptr, eng.B
    stream = torch.cuda.current_stream(eng.device).cuda_stream
    f64 = dict(dtype=torch.float64, device=eng.device)
    eng.S_state.zero_()
    eng.F_state.zero_()
    eng.info.zero_()
    steady = torch.zeros((B, int(lib.gf_steady_size())), **f64)
    acc = torch.full((B, 3), float("nan"), **f64)
    for k, n0 in enumerate(range(0, N_LONG, T)):
        rows = min(T, N_LONG - n0)
        _lib.check(lib.gf_steady_sweep(*sweep_head(eng, rows, n0), p(steady), ARM, stream), "gf_steady_sweep")
        _lib.check(lib.gf_reduce_tile_steady(B, rows, n0, p(eng.d), p(eng.z), p(steady), p(eng.work), p(acc),
                                             1 if k == 0 else 0, stream), "gf_reduce_tile_steady")
    torch.cuda.synchronize()
    hdr0 = steady.cpu().numpy()
    assert np.all(eng.info.cpu().numpy() == 0)
    assert np.all(hdr0[:, 0] == SW) and np.all(hdr0[:, 2] == 0.0), hdr0[:, :3].tolist()

    tails = list(TAILS) + [REPEAT]
    hdrs = steady.unsqueeze(0).repeat(len(tails), 1, 1).contiguous()
    accs = torch.tensor([0.0, 0.0, float("inf")], **f64).repeat(len(tails), B, 1).contiguous()
    for i, k in enumerate(tails):
        _lib.check(lib.gf_steady_finish(*finish_head(eng, ANCHOR + 1 + k, hdrs[i], accs[i]), stream),
                   "gf_steady_finish")
    torch.cuda.synchronize()
    assert np.all(eng.info.cpu().numpy() == 0)
    after, got = hdrs.cpu().numpy(), accs.cpu().numpy()
    assert np.all(after[:, :, 2] == 0.0) and np.all(after[:, :, 0] == SW)
    rep = TAILS.index(REPEAT)
    assert np.array_equal(after[-1], after[rep]) and np.array_equal(got[-1], got[rep])

    worst, worst_at = 0.0, None
    for b in range(B):
        fz = _header_frozen(hdr0[b], c.coeffs[b], J)
        for i, k in enumerate(TAILS):
            ref = _row_form_state(fz["alpha"], fz["expo"], fz["G"], fz["s"], c.y[SW:SW + k])
            s = (after[i, b, ST_SR:ST_SR + J] + 1j * after[i, b, ST_SI:ST_SI + J]).astype(np.clongdouble)
            dist = float(np.max(np.abs(s - ref)) / np.max(np.abs(ref)))
            if dist > worst:
                worst, worst_at = dist, (k, b)
            # the slots behind the kernel's terms stay zero
            assert not after[i, b, ST_SR + J:ST_SI].any() and not after[i, b, ST_SI + J:ST_SI + 32].any(), (J, k, b)
    print(f"J = {J:2d} (ROWS = {(2 * J + 3) // 4 * 4:2d}): end state against the longdouble row form {worst:.2e} of "
          f"max |s| at a tail of {worst_at[0]} rows (problem {worst_at[1]}); bar {BAR:.2e}")
    assert worst <= BAR, (J, worst, worst_at)


@pytest.mark.parametrize("J", (2, 30))
def test_chunked_launch_and_two_windows_on_the_long_tail(raws, J):  # noqa: F811
    """tests/steady_group_cases.py's tail of 2113 rows (two chunks of 16 blocks, a block and a row): the chunked launch
    against the one-wave launch within tests/test_gpu_steady_chunk.py's bars -- M, the block's own code on unit
    states, follows the four-row step --, and two launches over disjoint windows against one, bit for bit."""
    import torch
    r = raws(J)
    hd, ac = r["fresh"](3)
    r["finish"](N_G, hd[0], ac[0])
    ws = _chunked(r, N_G, hd[1], ac[1])
    r["finish"](N_G, hd[2], ac[2], window=(1, SW))              # holds nobody
    r["finish"](N_G, hd[2], ac[2], window=(SW, N_G + 1))        # holds everybody
    torch.cuda.synchronize()
    assert ws is not None
    a, h = ac.cpu().numpy(), hd.cpu().numpy()
    assert np.all(np.isfinite(a[0])) and np.all(a[0][:, 1] > 0.0)
    _against_plain(f"J = {J}, tail of {LONGEST_G} rows", a[0], a[1], h[0], h[1])
    assert np.array_equal(a[2], a[0]) and np.array_equal(h[2], h[0])
