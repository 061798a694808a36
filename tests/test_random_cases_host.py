"""Host: the shared random-problem generators and skip rule of tests/random_cases.py (no GPU)."""
import numpy as np
import pytest

from tests import random_cases as rc


def _axis_ok(t):
    return np.all(np.isfinite(t)) and np.all(np.diff(t) > 0)


@pytest.mark.parametrize("seed", [0, 7, 301, 322])
def test_generators_are_deterministic_with_sorted_distinct_axes(seed):
    for gen in (rc.narrow_problem, rc.batch_problem, rc.wide_problem):
        a, b = gen(seed), gen(seed)
        for k, v in a.items():
            if k != "rng":
                assert np.array_equal(np.asarray(v), np.asarray(b[k])) if k != "kernel" else \
                    all(np.array_equal(x, y) for x, y in zip(v.get_device_coefficients(), b[k].get_device_coefficients()))
        assert _axis_ok(a["t"]) and len(a["t"]) == len(a["y"]) == len(a["diag_user"])


def test_batch_problems_cover_the_product_settings():
    seen = set()
    for seed in range(300, 332):
        p = rc.batch_problem(seed)
        assert 2 <= p["B"] <= 12 and 1 <= p["J"] <= 30 and 300 <= p["N"] <= 12000 and p["S0"].shape == (2, p["B"], p["J"])
        # every term stays on its side of Q = 1/2 in both proposals (one overdamped pattern per batch)
        over = p["Q"] < 0.5
        assert np.all(over == over[0, 0][None, None, :]) and over[0, 0].sum() == p["n_over"]
        seen |= {p["kind"], p["route"]}
        if p["N"] % 64 in (1, 63):
            seen.add("k*tile+-1")
    assert seen >= set(rc.AXES) | {"stream", "auto", "k*tile+-1"}
    from gadfly_amd.engine import _coeff_pack, _complexify_pack
    for seed in range(400, 416):
        p = rc.wide_problem(seed)
        coeffs = [k.get_device_coefficients() for k in rc.sho_kernels(p["S0"], p["w0"], p["Q"], p["delta"])]
        Jr, Jc = _coeff_pack(coeffs)[:2]
        # the kernel's celerite width: two real columns per overdamped term, a complex pair per underdamped one
        assert Jr == 2 * p["n_over"] and Jr + 2 * Jc == 2 * p["J"]
        # the width the fused wide sweep runs at: every real column rewritten as a complex pair
        Jr2, Jc2 = _complexify_pack(*_coeff_pack(coeffs))[:2] if Jr else (Jr, Jc)
        assert Jr2 == 0 and 64 <= 2 * Jc2 == 2 * p["J"] + 2 * p["n_over"] <= 176


def test_batch_seeds_reach_the_long_periods_on_every_axis_and_route():
    """The periods the batched evaluator calibrates on the seeds of test_gpu_random_batched.py, predicted from the
    oracle's condition through the engine's own period rule (random_cases.batch_calibration; the GPU test asserts that
    the device reaches at least that period).  A generator change must not silently drop the settings the test is
    there for: periods of 32 / 64 on the BKJD axis and on the QMODE_PHASE-crossing one (there, only a period > 1 runs
    rotation steps in a tile that starts below the threshold), and the time-parallel route -- two-sweep among it --
    at those periods."""
    long = dict(bkjd=0, qcross=0, tp=0, two=0)
    tp_seeds = 0
    for seed in range(300, 332):
        p = rc.batch_problem(seed)
        tp, two, per = rc.batch_calibration(p)
        tp_seeds += tp and p["J"] >= 3
        if per is not None and per >= 32:
            long[p["kind"]] = long.get(p["kind"], 0) + 1
            long["tp"] += tp
            long["two"] += two
    assert long["bkjd"] >= 2 and long["qcross"] >= 2 and long["tp"] >= 3 and long["two"] >= 2, long
    assert tp_seeds >= 6, tp_seeds


def test_qmode_crossing_axis_crosses_in_the_first_rows():
    hits = 0
    for seed in range(300, 400):
        p = rc.batch_problem(seed)
        if p["kind"] != "qcross":
            continue
        co = rc.sho_kernels(p["S0"][1][:1], p["w0"][1][:1], p["Q"][1][:1], p["delta"])[0].get_device_coefficients()
        ph = rc.wmax(co) * np.abs(p["t"])
        r = int(np.argmax(ph > rc.QMODE_PHASE))
        assert ph[0] < rc.QMODE_PHASE and 1 <= r < 60 and ph[r - 1] <= rc.QMODE_PHASE < ph[r]
        hits += 1
    assert hits >= 5


def test_skip_rule_keeps_well_conditioned_problems():
    """C vs 80-bit on small problems: where the condition is modest the two agree far inside C_VS_80 (so the rule,
    which runs the 80-bit recurrence only beyond COND_80, skips nothing it should keep) -- on a zero-based and on a
    BKJD axis (the 80-bit rows take cos / sin of the same float64 phases)."""
    from gadfly_amd import StellarOscillatorKernel
    from gadfly_amd.synth import solar_like_hyperparameters, uniform_times
    N = 600
    co = StellarOscillatorKernel(solar_like_hyperparameters(6), texp=60.0).get_device_coefficients()
    y = np.random.default_rng(3).normal(size=N) * 50.0
    du = np.full(N, 900.0)
    for off in (0.0, rc.BKJD0):
        t = uniform_times(N, 60.0) + off
        orc = rc.oracle_problems([co], t, du, y)
        assert orc["info"][0] == 0 and orc["cond"][0] < rc.COND_80
        ll80 = rc.loglike80([co], t, [du + co[6]], y)
        assert abs(ll80[0] - orc["ref"][0]) <= 1e-12 * abs(ll80[0])
        assert rc.float64_limit([co], t, du, y, orc) is None
    # a problem beyond the bar by its condition alone (narrow seed 102: 4e8) is skipped, whatever the GPU would say
    p = rc.narrow_problem(102)
    co = p["kernel"].get_device_coefficients()
    assert "conditioning" in rc.float64_limit([co], p["t"], p["diag_user"], p["y"])


def test_loglike80_matches_the_sequential_oracle():
    from oracle import seq
    p = rc.narrow_problem(104)
    co = p["kernel"].get_device_coefficients()
    t, y, d = p["t"][:400], p["y"][:400], p["diag_user"][:400] + co[6]
    ld = np.longdouble
    c, a, U, V = seq.celerite_matrices(co[:6], t, d, dtype=ld)
    dl, Wl, info = seq.factor(t.astype(ld), c, a, U, V)
    zl = seq.solve_lower(t.astype(ld), c, U, Wl, y.astype(ld))
    ref = float(-0.5 * (np.sum(np.log(dl)) + len(t) * np.log(2 * ld(np.pi))) - 0.5 * np.sum(zl * zl / dl))
    assert info == 0 and abs(rc.loglike80([co, co], t, [d, d], y)[1] - ref) <= 1e-13 * abs(ref)
