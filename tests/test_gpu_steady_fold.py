"""GPU: the folded block of the finishing launch (z = H y + Q s with H y formed a block ahead, DESIGN.md 3.10;
restated in numpy in tests/test_steady_fold_host.py), built as tests/test_gpu_steady_split.py builds its cases: a
forced switch, tiles of 1024 rows, against the oracle and the plain sweep.  Tails of 1, 64, 65, 127, 128, 129 and 193
rows behind the switch: no full block at all, the partial block takes the set-up's u and every load ahead is clamped to
the last row; exactly one full block, whose look-ahead u has no block to go to and is dropped; a one-row partial block
that takes its predecessor's u; a partial block of 63 rows behind a full one; two full blocks, the second on the u and
the y the first one formed and loaded; two and a row; three and a row, the load two blocks ahead unclamped once.  The
narrowest, the flagship's and the widest instance at a tail of 129 rows.  And at the raw entry points: two launches over
disjoint windows of switch rows against one launch, on a batch whose problems switch in different tiles.  The tail
tests compare whole-series totals, in which the ~3969 swept rows in front of the switch dilute whatever the tail adds;
the tail's own sums, per finishing launch, for every tail of 1 .. 193 rows and at every instance (J = 1 .. 31):
tests/test_gpu_steady_instances.py, on the cases of tests/steady_cases.py (which this file shares)."""
import numpy as np
import pytest

from tests.steady_cases import LONGEST, _case, _run
from tests.test_gpu_steady_overlap import raw  # noqa: F401  (the fixture: one evaluation's tiles at the raw entry points)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(J):
        if J not in made:
            made[J] = _case(J)
        return made[J]
    return get


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
