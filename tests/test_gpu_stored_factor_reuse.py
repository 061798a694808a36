"""GPU: a stored scaled factor whose owner has swept again before the factor's first solve.  ScaledFactor builds its
chunk transitions lazily, at the first solve, from the rows r of the final pass -- which live in the owner's row
buffer.  An evaluation of OTHER coefficients on the same chunking refills that buffer, and the factor must then
rebuild r = w~ d from its own rows (the generation check of ScaledFactor._ensure_transitions) instead of chaining its
chunks with another factor's transitions."""
import numpy as np
import pytest

from tests import util
from tests.random_cases import oracle_problems, relmax

pytestmark = pytest.mark.gpu
TOL_VEC = 1e-6


def test_stored_factor_survives_a_later_evaluation_of_its_owner(hip):
    import torch
    import gadfly_amd
    from gadfly_amd.engine import StreamingBatch
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    from oracle import cref
    prob = util.solar_problem(20, 6000)
    t, y, du = prob["t"], prob["y"], prob["diag_user"]
    N = len(t)
    co = prob["kernel"].get_device_coefficients()
    other = gadfly_amd.StellarOscillatorKernel(jitter_hyperparameters(solar_like_hyperparameters(20), 7, frac=0.3),
                                               texp=60.0).get_device_coefficients()
    eng = StreamingBatch([co], t, y, diag=du)
    eng.generator_period = 1
    L, nch = eng._tp_chunking(None)             # the chunking evaluate(time_parallel=True) takes by itself
    assert nch > 1
    fac = eng.stored_factor(chunk_len=L)
    assert fac.nch == nch and not fac._phi_ready
    rows, gen = eng._tp["r"], eng._tp_generation
    eng.use_coefficients(eng.pack_coefficients([other]))
    eng.evaluate(time_parallel=True)
    # the owner's row buffer now holds the rows of another factor
    assert eng._tp_used and eng._tp["r"] is rows and eng._tp_generation != gen
    orc = oracle_problems([co], t, du, y)
    c, a, U, V = orc["mats"][0]
    d_ref, W_ref = orc["d"][0], orc["W"][0]
    Y = np.random.default_rng(4).normal(size=(N, 3))
    Yd = torch.as_tensor(Y).cuda().reshape(1, N, 3)
    ai_ref = cref.solve_upper(t, c, U, W_ref, cref.solve_lower(t, c, U, W_ref, Y) / d_ref[:, None])
    assert relmax(fac.apply_inverse(Yd)[0].cpu().numpy(), ai_ref) < TOL_VEC
    assert fac._phi_ready
    dt_ref = cref.matmul_lower(t, c, U, W_ref, Y * np.sqrt(d_ref)[:, None])
    assert relmax(fac.dot_tril(Yd)[0].cpu().numpy(), dt_ref) < TOL_VEC
    # and the owner's own evaluation of the other coefficients is right as well
    ref2, info2 = cref.loglike(other[:6], t, du + other[6], y)
    ll2 = float(eng.log_likelihood_time_parallel(chunk_len=L)[0])
    assert info2 == 0 and abs(ll2 - ref2) <= 1e-8 * abs(ref2)
