"""GPU: random WIDE kernels (J 32-88 SHO terms, W = 64 ... 176; some with overdamped terms, which the fused wide
sweep takes as degenerate complex ones) for two walkers with different coefficients, through every wide route --
streamed fused sweep, the block-scaled rows without fusion (`scaled_wide`), three- and two-sweep time-parallel
evaluation -- at exact rows and at the period the product's rule gives for the measured condition, against the C
oracle at 1e-8; and the stored time-parallel `WideFactor` of one series on the chunk-parallel solve paths at 1e-6.
Problems: tests/random_cases.wide_problem; skip rule: random_cases.float64_limit (oracle-side only).
tools/random_sweep_more.py wide runs this function over any seed range."""
import numpy as np
import pytest

from tests.random_cases import float64_limit, oracle_problems, relmax, sho_kernels, wide_problem

pytestmark = pytest.mark.gpu
RTOL_LL, TOL_VEC = 1e-8, 1e-6


def _close(ll, ref, what):
    rel = np.abs(np.asarray(ll) - ref) / np.abs(ref)
    assert np.all(rel <= RTOL_LL), (what, rel.tolist(), np.asarray(ll).tolist(), ref.tolist())


@pytest.mark.parametrize("seed", range(400, 416))
def test_random_wide_kernel(hip, seed):
    import torch
    from gadfly_amd.engine import StreamingBatch, WideFactor
    from oracle import cref
    prob = wide_problem(seed)
    t, y, du, N, L, rng = prob["t"], prob["y"], prob["diag_user"], prob["N"], prob["chunk_len"], prob["rng"]
    coeffs = [k.get_device_coefficients() for k in sho_kernels(prob["S0"], prob["w0"], prob["Q"], prob["delta"])]
    orc = oracle_problems(coeffs, t, du, y)
    eng = StreamingBatch(coeffs, t, y, diag=du, tile_rows=1024)
    tag = (seed, prob["kind"], prob["J"], prob["n_over"], eng.W, N, L)
    assert eng._wide_ok() and not eng._fused_ok() and 64 <= eng.W <= 176, tag
    if np.any(orc["info"] != 0):
        # not positive definite: the streamed sweep stops at the oracle's failing row
        eng.generator_period = 1
        ll = eng.log_likelihood().cpu().numpy()
        bad = orc["info"] != 0
        assert np.all(ll[bad] == -np.inf) and np.array_equal(eng.info.cpu().numpy()[bad], orc["info"][bad]), tag
        return
    why = float64_limit(coeffs, t, du, y, orc)
    if why:
        pytest.skip(why)
    ref = orc["ref"]
    eng.generator_period = 1
    _close(eng.log_likelihood().cpu().numpy(), ref, (tag, "streamed", 1))
    assert eng.kernel_used == "fused-wide"
    cond = eng.condition_estimate()
    cond_ref = float(max(m[1].max() for m in orc["mats"]) / min(d.min() for d in orc["d"]))
    assert abs(cond - cond_ref) <= 1e-6 * cond_ref, (tag, cond, cond_ref)
    per = eng.period_for_condition(cond)
    tag = tag + (per, cond)
    for period in sorted({1, per}):
        eng.generator_period = period
        _close(eng.log_likelihood().cpu().numpy(), ref, (tag, "streamed", period))
        assert eng.kernel_used == "fused-wide"
        for two in (False, True):
            eng.two_sweep = two
            ll = eng.log_likelihood_time_parallel(chunk_len=L).cpu().numpy()
            assert eng._last_wide_tp and eng._two_sweep_used == two and eng._wide_tp["nch"] > 1, tag
            _close(ll, ref, (tag, "two-sweep" if two else "three-sweep", period))
        eng.two_sweep = False
    # the same rows, block-scaled, without fusion (no generator period there: rows built exactly)
    sw = StreamingBatch(coeffs, t, y, diag=du, tile_rows=1024, allow_fused=False)
    assert (sw.scaled_wide or (sw.scaled and sw.W == 64)) and not sw._wide_ok(), tag
    _close(sw.log_likelihood().cpu().numpy(), ref, (tag, "scaled_wide"))
    # the stored factor of ONE series, time-parallel, on the chunk-parallel solves
    one = StreamingBatch(coeffs[:1], t, y, diag=du)
    one.generator_period = per
    fac = WideFactor(one, time_parallel=True, chunk_len=L)
    assert fac.time_parallel and fac.nch > 1, tag
    _close(fac.reduce(True)[0].cpu().numpy(), ref[:1], (tag, "WideFactor"))
    c, a, U, V = orc["mats"][0]
    d_ref, W_ref = orc["d"][0], orc["W"][0]
    Y = rng.normal(size=(N, 3))
    Yd = torch.as_tensor(Y).cuda().reshape(1, N, 3)
    ai_ref = cref.solve_upper(t, c, U, W_ref, cref.solve_lower(t, c, U, W_ref, Y) / d_ref[:, None])
    dt_ref = cref.matmul_lower(t, c, U, W_ref, Y * np.sqrt(d_ref)[:, None])
    assert relmax(fac.apply_inverse(Yd[:, :, :1].contiguous())[0].cpu().numpy(), ai_ref[:, :1]) < TOL_VEC, tag
    assert relmax(fac.apply_inverse(Yd)[0].cpu().numpy(), ai_ref) < TOL_VEC, tag
    assert relmax(fac.dot_tril(Yd[:, :, :1].contiguous())[0].cpu().numpy(), dt_ref[:, :1]) < TOL_VEC, tag
