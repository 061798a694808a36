"""GPU: random walker batches through the batched evaluator at the settings the product runs -- the generator period
it calibrates itself (up to 64), the vectorised coefficient pack (`pack_parameters`), every walker with its own
coefficients, time axes near zero, on BKJD and crossing QMODE_PHASE inside the first tile or chunk, the streamed and
the automatic (time-parallel) route -- against the C oracle at 1e-8.  Each seed asserts the route and the period the
oracle's condition predicts for it; test_random_cases_host.py checks that these seeds include periods of 32 / 64 on
the BKJD and the crossing axes and on the time-parallel route.  Problems: tests/random_cases.batch_problem;
skip rule: random_cases.float64_limit (oracle-side only)."""
import numpy as np
import pytest

from tests.random_cases import (batch_problem, expected_route, float64_limit, oracle_problems, product_period,
                                sho_kernels, wmax)

pytestmark = pytest.mark.gpu
RTOL_LL = 1e-8


@pytest.mark.parametrize("seed", range(300, 332))
def test_random_walker_batch(hip, seed):
    import gadfly_amd
    prob = batch_problem(seed)
    S0, w0, Q, delta = prob["S0"], prob["w0"], prob["Q"], prob["delta"]
    t, y, du, B, N = prob["t"], prob["y"], prob["diag_user"], prob["B"], prob["N"]
    kernels = [sho_kernels(S0[i], w0[i], Q[i], delta) for i in range(2)]
    coeffs = [[k.get_device_coefficients() for k in ks] for ks in kernels]
    orc = [oracle_problems(coeffs[i], t, du, y) for i in range(2)]
    for i in range(2):                  # (both proposals' values are checked)
        why = float64_limit(coeffs[i], t, du, y, orc[i])
        if why:
            pytest.skip(why)
    if prob["kind"] == "qcross":       # walker 0 of the checked proposal crosses the threshold in its first 60 rows
        ph = wmax(coeffs[1][0]) * np.abs(t)
        assert ph[0] < 4.0e6 < ph[59]
    ev = gadfly_amd.BatchedLogLikelihood(kernels[0], t, y, yerr=prob["yerr"], tile_rows=prob["tile"])
    eng = ev.engine
    eng.force_streaming = prob["route"] == "stream"
    tp, two_exp = expected_route(prob)
    assert eng._fused_ok() and eng.B == B and eng.W <= 60
    # 1. first proposal: one synchronous evaluation calibrates the period from the measured condition
    ll0 = ev.evaluate()
    pd0 = orc[0]["info"] == 0
    dmin, amax = ev._last_cond
    dmin, amax = float(dmin.min()), float(amax.max())
    cond = amax / dmin
    per = int(eng.generator_period)
    tag = (seed, prob["kind"], prob["route"], prob["J"], prob["n_over"], B, N, prob["tile"], eng._pack.block, per, cond)
    assert eng._tp_used == tp and (tp or eng.kernel_used == "fused"), tag
    if pd0.all():
        cond_ref = float(np.max([m[1].max() for m in orc[0]["mats"]]) / np.min([d.min() for d in orc[0]["d"]]))
        assert per == eng.period_for_condition(cond), tag
        assert per <= eng.period_for_condition(cond_ref), (tag, cond_ref)       # never longer than the truth allows
        # ... and not shorter than the oracle's condition gives (a two-sweep estimate is at most 1.5 x the truth):
        # the period this seed is meant to run at (random_cases.batch_calibration) is the one it runs at
        per_min = product_period(coeffs[0], t, cond_ref * (eng.TWO_SWEEP_MARGIN if two_exp else 1.0 + 1e-4))
        assert per >= per_min, (tag, cond_ref, per_min)
        if not two_exp:
            # (an estimate: where rotation steps run short of qmode at phases near QMODE_PHASE, the rows differ from
            # the oracle's rounded-phase rows by up to half an ulp of the phase -- the smallest pivot moves by up to
            # that quantum times the condition: 1.8e-6 at 2.3e5 on seed 318)
            assert abs(cond - cond_ref) <= 1e-4 * cond_ref, (tag, cond_ref)
        ref0 = orc[0]["ref"]
        assert np.all(np.abs(ll0 - ref0) <= RTOL_LL * np.abs(ref0)), (tag, ll0, ref0)
    # 2. second proposal through the vectorised pack, asynchronously, then the accuracy guard
    out = ev.evaluate_device(ev.pack_parameters(S0[1], w0[1], Q[1], delta))
    assert eng.generator_period == per and eng._tp_used == tp, tag
    two = eng._two_sweep_used
    assert two == two_exp, tag
    # the accuracy guard's flags: only the flagged walkers are repeated with exact rows, and a walker the oracle puts
    # well inside the guard's bound (a factor 2) is not flagged -- its value below IS a value at period `per`
    flags = [f for o, f, _, _ in ev._unresolved if o is out]
    flag = flags[0].cpu().numpy() if flags else np.zeros(B, bool)
    assert ev.resolve() == int(flag.sum()), tag
    ref, info = orc[1]["ref"], orc[1]["info"]
    if per > 1:
        coef = eng.generator_error_coefficient(per) * (eng.TWO_SWEEP_MARGIN if two else 1.0)
        amax1 = np.array([m[1].max() for m in orc[1]["mats"]])
        dmin1 = np.array([d.min() for d in orc[1]["d"]])
        clear = (info == 0) & (2.0 * coef * amax1 <= ev.generator_target * dmin1)
        assert not flag[clear].any(), (tag, flag, clear)
    got = out.cpu().numpy()
    for i in range(B):
        if info[i] != 0:
            assert got[i] == -np.inf, (tag, two, i, got[i], info[i])
        else:
            assert abs(got[i] - ref[i]) <= RTOL_LL * abs(ref[i]), (tag, two, i, got[i], ref[i])
