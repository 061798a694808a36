"""GPU: the folded block of the finishing launch (z = H y + Q s with H y formed a block ahead, DESIGN.md 3.10;
restated in numpy in tests/test_steady_fold_host.py), built as tests/test_gpu_steady_split.py builds its cases: a
forced switch, tiles of 1024 rows, against the oracle and the plain sweep.  Tails of 1, 64, 65, 127, 128, 129 and 193
rows behind the switch: no full block at all, the partial block takes the set-up's u and every load ahead is clamped to
the last row; exactly one full block, whose look-ahead u has no block to go to and is dropped; a one-row partial block
that takes its predecessor's u; a partial block of 63 rows behind a full one; two full blocks, the second on the u and
the y the first one formed and loaded; two and a row; three and a row, the load two blocks ahead unclamped once.  The
narrowest, the flagship's and the widest instance at a tail of 129 rows.  And at the raw entry points: two launches over
disjoint windows of switch rows against one launch, on a batch whose problems switch in different tiles."""
import numpy as np
import pytest

from tests.random_cases import oracle_loglikes
from tests.test_gpu_steady import RTOL_LL, _evaluator, _fast_terms, _rel, _series
from tests.test_gpu_steady_finish import B_FIN, RTOL_PLAIN, _steady_and_plain
from tests.test_gpu_steady_overlap import raw  # noqa: F401  (the fixture: one evaluation's tiles at the raw entry points)
from tests.test_gpu_steady_split import ANCHOR, ARM, T
from tests.test_steady_host import _switch_row

pytestmark = pytest.mark.gpu
LONGEST = 193


def _case(J):
    """The series of the longest tail, J-term kernels and their coefficients, and the check (once) that the rule puts
    the switch at ANCHOR on the oracle's factor under this arm_from; the shorter series are its first rows."""
    import gadfly_amd
    from oracle import cref
    N = ANCHOR + 1 + LONGEST
    t, y = _series(N, seed=47)
    hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
    for hp in hps:
        co = gadfly_amd.StellarOscillatorKernel(hp, texp=60.0).get_device_coefficients()
        c, a, U, V = cref.get_matrices(co[:6], t, np.full(N, 900.0) + co[6])
        d, W, info = cref.factor(t, c, a, U, V)
        assert info == 0
        row, _, _ = _switch_row(t[ARM:], np.asarray(co[5], dtype=np.float64), d[ARM:], W[ARM:])
        assert ARM + row == ANCHOR
    return hps, t, y


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(J):
        if J not in made:
            made[J] = _case(J)
        return made[J]
    return get


def _run(hps, t, y, tail, what):
    N = ANCHOR + 1 + tail
    t, y = t[:N], y[:N]
    ev, coeffs = _evaluator(hps, t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    ev.engine._steady_axis = (ARM, 0.0)
    got, plain, sw = _steady_and_plain(ev)
    print(f"{what}: switch rows {sw.tolist()} of {N}, error vs oracle {_rel(got, ref).max():.2e}, "
          f"steady vs plain {_rel(got, plain).max():.2e}")
    assert np.all(sw == ANCHOR + 1) and np.all(N - sw == tail), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert _rel(got, plain).max() <= RTOL_PLAIN
    assert ev.steady_reruns == 0


@pytest.mark.parametrize("tail", [1, 64, 65, 127, 128, 129, LONGEST])
def test_tail_lengths_around_one_two_and_three_blocks(hip, cases, tail):
    hps, t, y = cases(2)
    _run(hps, t, y, tail, f"tail of {tail} rows")


@pytest.mark.parametrize("J", [1, 30, 31])
def test_instances_at_two_blocks_and_a_row(hip, cases, J):
    hps, t, y = cases(J)
    _run(hps, t, y, 129, f"J = {J}, tail of 129 rows")


def test_two_windows_give_the_single_launch(raw):  # noqa: F811
    """gf_steady_finish_window over [1, b) and [b, N + 1), b a problem's own switch row, in either order: acc as one
    gf_steady_finish leaves it, bit for bit -- a problem's values do not depend on the launch that takes it."""
    N, sw, run = raw["N"], raw["sw"], raw["run"]
    assert len(set(((sw - 1) // raw["T"]).tolist())) >= 3, sw.tolist()     # the problems switch in different tiles
    one = run(None)
    assert np.all(np.isfinite(one[0]))
    b = int(np.unique(sw)[-2])
    for layout in ([(1, b), (b, N + 1)], [(b, N + 1), (1, b)]):
        two = run(layout)
        assert np.array_equal(two[0], one[0]), (layout, two[0].tolist(), one[0].tolist())
        assert np.array_equal(two[1], one[1], equal_nan=True)
