"""GPU: the benchmark headline's configuration, scaled down -- 64 walkers of the 30-term solar-like kernel at 60 s,
each with its own coefficients (+-10 % jitter, seeds 1000 + id), N = 3 * 8192 + 1 rows, the streamed sweep on the
long scaling span (block 64) at the generator period the evaluator calibrates (64), proposals handed over as (B, J)
arrays through `pack_parameters` and `evaluate_device` + `resolve` -- every walker against the C oracle at 1e-8, on
the zero-based axis and on the same axis moved to BKJD (RowGen::qmode on).  Then one walker of a proposal is made
badly conditioned: the accuracy guard must repeat exactly that one with exact rows and leave the others' period-64
values alone, bit for bit."""
import numpy as np
import pytest

from tests.random_cases import BKJD0, oracle_loglikes, sho_kernels

pytestmark = pytest.mark.gpu
RTOL_LL = 1e-8
B, J, N = 64, 30, 3 * 8192 + 1


def _proposal(base, step):
    """Hyperparameter sets of one proposal (jitter_hyperparameters, as bench.walker_proposals draws them) and
    their (B, J) arrays."""
    from gadfly_amd.synth import jitter_hyperparameters
    hps = [jitter_hyperparameters(base, 1000 + step * B + e) for e in range(B)]
    return hps, tuple(np.array([[p["hyperparameters"][k] for p in hp] for hp in hps]) for k in ("S0", "w0", "Q"))


def _coeffs(hps):
    import gadfly_amd
    return [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0).get_device_coefficients() for hp in hps]


def _check_route(eng):
    assert eng.kernel_used == "fused" and not eng._tp_used
    assert eng._pack.stream_block == 64 and eng.generator_period == 64


@pytest.mark.parametrize("axis", ["zero", "bkjd"])
def test_headline_configuration_against_the_oracle(hip, axis):
    import gadfly_amd
    from gadfly_amd.synth import solar_like_hyperparameters, uniform_times
    base = solar_like_hyperparameters(J)
    t = uniform_times(N, 60.0) + (BKJD0 if axis == "bkjd" else 0.0)
    rng = np.random.Generator(np.random.PCG64(12345))
    y = np.cumsum(rng.normal(size=N)) * 5.0 + 30.0 * rng.normal(size=N)
    du = np.full(N, 900.0)
    hps0, _ = _proposal(base, 0)
    kernels = [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0) for hp in hps0]
    delta = kernels[0].delta
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=30.0)
    eng = ev.engine
    eng.force_streaming = True
    assert (eng._pack.dmax * eng._tmax > 4.0e6) == (axis == "bkjd")          # qmode on the BKJD axis only
    ev.evaluate()                                                            # warm-up
    cond, period = ev.calibrate()
    assert period == 64 and eng._pack.stream_block == 64, (cond, period)
    outs, refs = [], []
    for step in (1, 2):
        hps, arr = _proposal(base, step)
        outs.append(ev.evaluate_device(ev.pack_parameters(*arr, delta)))
        _check_route(eng)
        refs.append(oracle_loglikes(_coeffs(hps), t, du, y))
    assert ev.resolve() == 0                    # nothing was repeated: the values below ARE period-64 values
    for step, (out, (ref, info)) in enumerate(zip(outs, refs), 1):
        got = out.cpu().numpy()
        assert np.all(info == 0)
        rel = np.abs(got - ref) / np.abs(ref)
        assert rel.max() <= RTOL_LL, (axis, step, int(rel.argmax()), float(rel.max()))
    # a planted ill-conditioned walker (amplitudes x 1e6, frequencies x 0.03: condition ~ 1e5) in proposal 2
    hps, (S0, w0, Q) = _proposal(base, 2)
    S0, w0 = S0.copy(), w0.copy()
    S0[3] *= 1e6
    w0[3] *= 0.03
    hot = ev.evaluate_device(ev.pack_parameters(S0, w0, Q, delta))
    _check_route(eng)
    unguarded = hot.clone()
    assert ev.resolve() == 1
    got = hot.cpu().numpy()
    same = np.arange(B) != 3
    plain = outs[1].cpu().numpy()
    assert np.array_equal(got[same], unguarded.cpu().numpy()[same])
    assert np.array_equal(got[same], plain[same])            # the other walkers: the period-64 values of step 2
    co3 = sho_kernels(S0[3:4], w0[3:4], Q[3:4], delta)[0].get_device_coefficients()
    ref3, info3 = oracle_loglikes([co3], t, du, y)
    assert info3[0] == 0 and abs(got[3] - ref3[0]) <= RTOL_LL * abs(ref3[0]), (got[3], ref3[0])
    assert eng.generator_period == 64
