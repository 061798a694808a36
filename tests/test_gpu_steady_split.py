"""GPU: the finishing launch's state update on both half-waves (restated in numpy in
tests/test_steady_finish_host.py): tails of 1, 2, 31, 32, 33, 63, 64 and 65 rows behind a forced switch -- a last block
of every shape the split has: the lower half-wave alone (even, odd, exactly full), one and two rows on the upper one,
both full, and a second block of one row -- against the oracle and the plain sweep.  What is compared are whole-series
totals: the ~3969 swept rows in front of the switch dilute whatever the tail adds (a tail of one row is 1/4000 of both
sums).  The tail's own sums, per finishing launch and at every instance: tests/test_gpu_steady_instances.py."""
import numpy as np
import pytest

from tests.random_cases import oracle_loglikes
from tests.test_gpu_steady import RTOL_LL, _evaluator, _fast_terms, _rel, _series
from tests.test_gpu_steady_finish import B_FIN, RTOL_PLAIN, _steady_and_plain
from tests.test_steady_host import GRID, LAG, COUNT, _switch_row

pytestmark = pytest.mark.gpu
T, ANCHOR = 1024, 4 * 1024 - 128            # tiles of 1024 rows; the sweep freezes at row 3968, the tail starts at 3969
ARM = ANCHOR - (LAG + COUNT - 1) * GRID


@pytest.fixture(scope="module")
def longest():
    """The series of the longest tail, its kernels' coefficients, and the check (once) that the rule puts the switch
    at ANCHOR on the oracle's factor under this arm_from; the shorter series are its first rows."""
    import gadfly_amd
    from oracle import cref
    N = ANCHOR + 1 + 65
    t, y = _series(N, seed=43)
    hps = [_fast_terms(2, k0) for k0 in range(B_FIN)]
    for hp in hps:
        co = gadfly_amd.StellarOscillatorKernel(hp, texp=60.0).get_device_coefficients()
        c, a, U, V = cref.get_matrices(co[:6], t, np.full(N, 900.0) + co[6])
        d, W, info = cref.factor(t, c, a, U, V)
        assert info == 0
        row, _, _ = _switch_row(t[ARM:], np.asarray(co[5], dtype=np.float64), d[ARM:], W[ARM:])
        assert ARM + row == ANCHOR
    return hps, t, y


@pytest.mark.parametrize("tail", [1, 2, 31, 32, 33, 63, 64, 65])
def test_tail_lengths_around_the_half_and_the_full_block(hip, longest, tail):
    hps, t, y = longest
    N = ANCHOR + 1 + tail
    t, y = t[:N], y[:N]
    ev, coeffs = _evaluator(hps, t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    ev.engine._steady_axis = (ARM, 0.0)
    got, plain, sw = _steady_and_plain(ev)
    print(f"tail of {tail} rows: switch rows {sw.tolist()} of {N}, error vs oracle {_rel(got, ref).max():.2e}, "
          f"steady vs plain {_rel(got, plain).max():.2e}")
    assert np.all(sw == ANCHOR + 1) and np.all(N - sw == tail), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert _rel(got, plain).max() <= RTOL_PLAIN
    assert ev.steady_reruns == 0
