"""GPU: the steady mode of the streamed lane-tiled sweep (gf_loglike_steady) through
BatchedLogLikelihood with `force_streaming`, against the C oracle at 1e-8: the flagship kernel, the narrowest and
the widest instance with the switch inside a tile, series too short to arm, a gap, inputs that never arm (bit for
bit the plain sweep), the violation flag and its repeat, a matrix that is not positive definite."""
import numpy as np
import pytest

from tests.random_cases import BKJD0, oracle_loglikes
from tests.test_steady_host import _two_terms

pytestmark = pytest.mark.gpu
RTOL_LL = 1e-8


def _series(N, seed=12345):
    from gadfly_amd.synth import uniform_times
    rng = np.random.Generator(np.random.PCG64(seed))
    return uniform_times(N, 60.0), np.cumsum(rng.normal(size=N)) * 5.0 + 30.0 * rng.normal(size=N)


def _fast_terms(J, k0=0):
    """J well-damped SHO terms between 400 and 4000 uHz: their factor reaches its steady state within ~1500 rows
    (tests/test_steady_host.py's rule on the oracle's factor), so short series exercise the switch."""
    nu = np.geomspace(400.0, 4000.0, J) if J > 1 else [3000.0]
    return _two_terms(*[(2.0 + 0.1 * (k + k0), nu[k] * (1.0 + 0.01 * k0), 2.0 + (k % 4)) for k in range(J)])


def _evaluator(hps, t, y, tile_rows, yerr=30.0, steady=True):
    import gadfly_amd
    kernels = [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0) for hp in hps]
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, yerr=yerr, tile_rows=tile_rows)
    ev.engine.force_streaming = True
    ev.engine.steady_state = steady
    return ev, [k.get_device_coefficients() for k in kernels]


def _rel(got, ref):
    return np.abs(np.asarray(got) - ref) / np.abs(ref)


@pytest.fixture(scope="module")
def flagship():
    """8 jittered walkers of the 30-term solar-like kernel at N = 65 536 and their oracle values (computed once)."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    N = 65536
    t, y = _series(N)
    hps = [jitter_hyperparameters(solar_like_hyperparameters(30), 1000 + i) for i in range(8)]
    import gadfly_amd
    coeffs = [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0).get_device_coefficients() for hp in hps]
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    return hps, t, y, ref


@pytest.mark.parametrize("period", ["calibrated", 1])
def test_flagship_walkers_switch_and_match_the_oracle(hip, flagship, period):
    hps, t, y, ref = flagship
    N = len(t)
    ev, _ = _evaluator(hps, t, y, 8192)
    eng = ev.engine
    if period == "calibrated":
        ev.evaluate()                       # (the evaluator picks its generator period from this one)
        ev.calibrate()
    else:
        ev.auto_generator_period, eng.generator_period = False, 1
    used = int(eng.generator_period)
    got = ev.evaluate()
    sw = eng.steady_switch_rows()
    assert eng.steady_used and eng.kernel_used == "fused"
    eng.steady_state = False
    ev.auto_generator_period, eng.generator_period = False, used
    plain = ev.evaluate()
    assert not eng.steady_used
    rel = _rel(got, ref)
    print(f"period {used}: switch rows {sw.tolist()}, error vs oracle {rel.max():.2e} (plain sweep "
          f"{_rel(plain, ref).max():.2e}), steady vs plain {_rel(got, plain).max():.2e}")
    assert rel.max() <= RTOL_LL, (rel.tolist(), sw.tolist())
    assert np.all((sw > 0) & (sw < N)), sw.tolist()
    assert ev.steady_reruns == 0


@pytest.mark.parametrize("J", [1, 31])
def test_instance_edges_switch_inside_a_tile(hip, J):
    """W = 2 and W = 62 (the 4-row and the 64-row instance): the switch falls inside a tile of 1024 rows and the
    frozen state crosses several tile boundaries."""
    N, T = 8192, 1024
    t, y = _series(N, seed=7)
    hps = [_fast_terms(J, k0) for k0 in range(3)]
    ev, coeffs = _evaluator(hps, t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    got = ev.evaluate()
    sw = ev.engine.steady_switch_rows()
    print(f"J = {J}: switch rows {sw.tolist()}, error vs oracle {_rel(got, ref).max():.2e}")
    assert ev.engine.steady_used and ev.engine.tile_rows == T
    # (sw = the switch anchor + 1: the anchor itself must not be a tile's first row)
    assert np.all(sw > 0) and np.all((sw - 1) % T != 0) and np.all(sw < N - 3 * T), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert ev.steady_reruns == 0


def test_scaling_block_below_64(hip):
    """A 240 s cadence with a fast term: the streamed sweep's scaling block is 16, block resets arrive every 16 rows,
    and the rule still looks at the 64-row grid over a lag of 1024 rows (no switch before row 19 * 64 + 1)."""
    import gadfly_amd
    from gadfly_amd.synth import uniform_times
    from tests.test_steady_host import FAST_TERM
    N, T = 8192, 1024
    _, y = _series(N, seed=19)
    t = uniform_times(N, 240.0)
    hps = [_two_terms(*[(s0 * (1.0 + 0.05 * k), nu, q) for s0, nu, q in FAST_TERM]) for k in range(3)]
    ev, coeffs = _evaluator(hps, t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    got = ev.evaluate()
    sw = ev.engine.steady_switch_rows()
    print(f"block {ev.engine._pack.stream_block}: switch rows {sw.tolist()}, error vs oracle {_rel(got, ref).max():.2e}")
    assert ev.engine.steady_used and ev.engine._pack.stream_block == 16
    assert np.all(sw >= 19 * 64 + 1) and np.all((sw - 1) % 64 == 0) and np.all(sw < N - 3 * T), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert ev.steady_reruns == 0


def _bitwise_pair(hps, t, y, tile_rows, yerr=30.0):
    ev, coeffs = _evaluator(hps, t, y, tile_rows, yerr=yerr)
    ev.auto_generator_period = False
    got = ev.evaluate()
    used, sw = ev.engine.steady_used, ev.engine.steady_switch_rows()
    ev.engine.steady_state = False
    plain = ev.evaluate()
    return got, plain, used, sw, coeffs


def test_short_series_never_arms_and_is_bit_identical(hip):
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    t, y = _series(4096)
    hps = [jitter_hyperparameters(solar_like_hyperparameters(30), 1000 + i) for i in range(4)]
    got, plain, used, sw, _ = _bitwise_pair(hps, t, y, 1024)
    assert used and np.all(sw == -1)        # the steady entry point ran, and stayed on full rows
    assert np.array_equal(got, plain)


def _gapped(N=16384, row=5000):
    t, y = _series(N, seed=11)
    t = t.copy()
    t[row:] += 700 * 60e-6                   # one gap of 700 cadences
    return t, y


def test_gap_arms_only_behind_it(hip):
    N, row = 16384, 5000
    t, y = _gapped(N, row)
    hps = [_fast_terms(2, k0) for k0 in range(4)]
    ev, coeffs = _evaluator(hps, t, y, 2048)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    got = ev.evaluate()
    sw = ev.engine.steady_switch_rows()
    print(f"gap at {row}: switch rows {sw.tolist()}, error vs oracle {_rel(got, ref).max():.2e}")
    assert ev.engine.steady_used and ev.engine._steady_axis[0] == row
    assert np.all(sw > row) and np.all(sw < N), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert ev.steady_reruns == 0 and not bool(ev.engine.steady_violations().any())


@pytest.mark.parametrize("case", ["yerr-per-row", "bkjd"])
def test_inputs_that_never_arm_are_bit_identical(hip, case):
    N = 16384
    t, y = _series(N, seed=13)
    yerr = 30.0
    if case == "yerr-per-row":
        yerr = np.random.Generator(np.random.PCG64(5)).uniform(20.0, 40.0, N)
    else:
        t = t + BKJD0
    hps = [_fast_terms(2, k0) for k0 in range(4)]
    got, plain, used, sw, _ = _bitwise_pair(hps, t, y, 2048, yerr=yerr)
    assert not used and np.all(sw == -1)
    assert np.array_equal(got, plain)


def test_violation_flag_and_repeat(hip):
    """gf_loglike_steady told that it may arm from row 0 on an axis with a gap (the evaluator's own axis scan
    overridden): the walkers switch before the gap, the tail meets it, the flag is raised for exactly those, and
    resolve() repeats them without the mode."""
    N, row = 16384, 5000
    t, y = _gapped(N, row)
    hps = [_fast_terms(2, k0) for k0 in range(4)]
    ev, coeffs = _evaluator(hps, t, y, 2048)
    eng = ev.engine
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    eng._steady_axis = (0, 0.0)             # arm_from = 0
    out = ev.evaluate_device()
    sw = eng.steady_switch_rows()
    viol = eng.steady_violations().cpu().numpy()
    assert eng.steady_used and np.all((sw > 0) & (sw < row)), sw.tolist()
    assert np.array_equal(viol, sw > 0) and viol.all()
    assert ev.resolve() == 4 and ev.steady_reruns == 4
    got = out.cpu().numpy()
    print(f"after the repeat: error vs oracle {_rel(got, ref).max():.2e}")
    assert _rel(got, ref).max() <= RTOL_LL
    assert eng.steady_state                 # (switched off for the repeats only)


def test_failing_walker_reports_its_row(hip):
    """One walker of four is not positive definite (a constant negative diagonal): -inf and the oracle's row, with the
    steady entry point running; the others switch and match."""
    import gadfly_amd
    N = 8192
    t, y = _series(N, seed=17)
    hps = [_fast_terms(2, k0) for k0 in range(4)]
    kernels = [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0) for hp in hps]
    coeffs = [k.get_device_coefficients() for k in kernels]
    diag = np.full((4, N), 900.0)
    diag[2] = -0.5 * float(np.sum(coeffs[2][2]))         # minus half the kernel's variance
    refs = [oracle_loglikes([co], t, dg, y) for co, dg in zip(coeffs, diag)]
    info = np.array([int(r[1][0]) for r in refs])
    assert info[2] > 0 and np.all(info[[0, 1, 3]] == 0)
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y, diag=diag, tile_rows=1024)
    ev.engine.force_streaming = True
    out = ev.evaluate_device()
    sw = ev.engine.steady_switch_rows()
    assert ev.engine.steady_used and int(ev.engine.info[2]) == info[2]
    ev.resolve()                            # (the accuracy guard may repeat the failing walker: -inf either way)
    got = out.cpu().numpy()
    assert got[2] == -np.inf and int(ev.engine.info[2]) == info[2]
    ok = [0, 1, 3]
    assert np.all(sw[ok] > 0)
    assert _rel(got[ok], np.array([refs[i][0][0] for i in ok])).max() <= RTOL_LL
