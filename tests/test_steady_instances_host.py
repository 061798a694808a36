"""Host side of tests/test_gpu_steady_instances.py: on the inputs of tests/steady_cases.py -- J = 1 .. 31 terms, every
instance of the steady tail's kernels -- the C oracle's exact rows behind the forced switch are a valid reference for
the frozen filter.  The rule puts the switch at ANCHOR for all three kernels of every J, and the frozen row form of
tests/test_steady_tail_host.py, started from the oracle's state at ANCHOR and run in longdouble, agrees with the exact
rows (cref.factor, cref.solve_lower) far below the device tests' bars:

    tail z                                          <= 1e-11 max|z|         (measured: 7.0e-13 at worst)
    sum z^2 / d_inf against sum z_n^2 / d_n         <= 1e-11 relative       (1.0e-12), at tails of 1, 2, 65 and 193 rows
    tail * log d_inf against sum log d_n            <= 1e-12 relative       (1.3e-13), at the same tails

These caps are conditions on the reference, not measurements of a device: about ten times what was measured, and they keep
the bars of the device tests (RTOL_Z = 1e-9 per row) at least a hundred times above what the reference contributes.
Should another libm move a value past a cap, the series' seed changes, not the cap."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, B_FIN, J_ALL, LONGEST, N_LONG, SW, TAILS_HOST, _fast_terms, _series
from tests.steady_cases import frozen_state, oracle_rows, row_form, tail_sums

CAP_Z, CAP_SHARE, CAP_LOGD = 1e-11, 1e-11, 1e-12


@pytest.fixture(scope="module")
def series():
    return _series(N_LONG, seed=47)


@pytest.mark.parametrize("J", J_ALL)
def test_exact_rows_are_a_reference_for_the_frozen_filter(series, J):
    t, y = series
    worst = dict(z=0.0, z64=0.0, share=0.0, logd=0.0, drift=0.0)
    for k0 in range(B_FIN):
        rows = oracle_rows(_fast_terms(J, k0), t, y)    # (asserts info == 0 and the switch at ANCHOR)
        d, z, dinf = rows.d, rows.z, rows.dinf
        sums = tail_sums(d, z)
        ks = np.array(TAILS_HOST)
        logd = np.abs(ks * np.log(np.longdouble(dinf)) - sums.logd[ks - 1]) / np.abs(sums.logd[ks - 1])
        worst["logd"] = max(worst["logd"], float(logd.max()))
        worst["drift"] = max(worst["drift"], float(np.max(np.abs(d[SW:] - dinf)) / dinf))
        assert logd.max() <= CAP_LOGD, (J, k0, logd.tolist())
        fz = frozen_state(rows, t)
        zl = row_form(fz, y[SW:])
        assert len(zl) == LONGEST
        zmax = np.max(np.abs(z))
        ez = float(np.max(np.abs(zl - z[SW:])) / zmax)
        e64 = float(np.max(np.abs(row_form(fz, y[SW:], dtype=np.complex128) - zl)) / zmax)
        share = np.cumsum(zl * zl)[ks - 1] / np.longdouble(dinf)
        es = np.abs(share - sums.z2d[ks - 1]) / sums.z2d[ks - 1]
        worst["z"], worst["z64"] = max(worst["z"], ez), max(worst["z64"], e64)
        worst["share"] = max(worst["share"], float(es.max()))
        assert ez <= CAP_Z, (J, k0, ez)
        assert es.max() <= CAP_SHARE, (J, k0, es.tolist())
    print(f"J = {J}: switch at {ANCHOR}; tail z {worst['z']:.1e} max|z| (float64 row form {worst['z64']:.1e}), "
          f"tail share {worst['share']:.1e}, tail log d {worst['logd']:.1e}, pivot drift {worst['drift']:.1e}")
