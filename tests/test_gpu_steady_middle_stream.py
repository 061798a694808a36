"""GPU: the middle window's chunked launch on a stream of its own, at the evaluator, on the pattern of
tests/test_gpu_steady_windows3.py: 512 walkers of tests/test_gpu_steady_overlap.py's kinds, which switch in tiles 0, 1
and 2 of 4096 rows, on the rank-one rows, behind one feedback -- split behind tile 0, middle window's end behind tile 1
-- so that the early launch stands behind tile 0's reduction on one side stream, the middle launch behind tile 1's sweep
on another, beside it, and the last launch behind the last tile.  Batches whose problems switch in other windows than
that feedback said run behind it: every problem is finished exactly once (a tail missed or taken twice shows at the
size of the tail's sum), the problems on the early window have the one launch's bits, the others agree with it to the
chunked route's 1e-12; with the piece switched off the values are the same bits."""
import numpy as np
import pytest

from tests.test_gpu_steady import _evaluator, _rel, _series
from tests.test_gpu_steady_chunk import CHUNK_BLOCKS, RTOL_BUILDS
from tests.test_gpu_steady_finish import N_FIN, T_FIN
from tests.test_gpu_steady_overlap import _spread_terms

pytestmark = pytest.mark.gpu
J, B = 30, 512
#: (earliest, all but B/8, all but B/64, latest) switch rows of the feedback: windows [1, 4097) early, [4097, 8193) in
#: the middle, [8193, ...) behind the last tile
FEEDBACK = [1729.0, 1729.0, 5761.0, 10241.0]
CUTS = [T_FIN + 1, 2 * T_FIN + 1]


def _batch(tiles):
    """B walkers, walker b of kind tiles[b % len(tiles)] with one of four variants."""
    return [_spread_terms(J, tiles[b % len(tiles)], k0=(b // len(tiles)) % 4) for b in range(B)]


BATCHES = {
    "as the feedback said": (0, 0, 0, 0, 0, 1, 1, 2),
    "rotated": (2, 1, 1, 0),
    "all early": (0,),
    "all in the middle": (1,),
    "all late": (2,),
}


@pytest.fixture(scope="module")
def batch(hip):
    import gadfly_amd
    import torch
    t, y = _series(N_FIN, seed=29)
    ev, _ = _evaluator(_batch(BATCHES["as the feedback said"]), t, y, T_FIN)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    eng._steady_chunk_blocks = CHUNK_BLOCKS
    eng.RANK1_MIN_ROWS = 0                  # the rank-one rows in front of the switch, as on long series
    eng.time_factor = True
    assert eng.B >= eng.STEADY_MIDDLE_MIN_B and eng.steady_middle_stream

    def kernels(hps):
        return [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0) for hp in hps]

    def reference(hps):
        eng.steady_overlap = False
        ref = ev.evaluate(kernels(hps))
        sw = eng.steady_switch_rows().copy()
        assert eng.steady_used and eng.rank1_used and np.all(sw > 0)
        assert not eng.steady_violations().cpu().numpy().any()
        return ref, sw

    def behind_the_feedback(hps):
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        eng.steady_overlap, eng.finish_events = True, []
        eng._steady_feedback = (torch.tensor(FEEDBACK, dtype=torch.float64), done)
        got = ev.evaluate(kernels(hps))
        assert (eng._steady_split, eng._steady_mid) == (T_FIN, 2 * T_FIN)
        return got, eng.steady_switch_rows().copy(), len(eng.finish_events)

    return dict(eng=eng, reference=reference, behind=behind_the_feedback)


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_problem_is_finished_once(batch, name):
    eng = batch["eng"]
    hps = _batch(BATCHES[name])
    ref, sw_ref = batch["reference"](hps)
    got, sw, launches = batch["behind"](hps)
    window = np.searchsorted(CUTS, sw, side="right")
    counts = np.bincount(window, minlength=3).tolist()
    e = _rel(got, ref)
    print(f"{name}: problems per window {counts}, against the one launch {e.max():.2e}")
    assert launches == 3 and np.array_equal(sw, sw_ref)
    assert eng._finish_mid_side is not None and eng._finish_mid_side != eng._finish_side
    if name == "as the feedback said":
        assert min(counts) > 0
    elif name.startswith("all"):
        assert max(counts) == B
    early = window == 0
    assert np.array_equal(got[early], ref[early])           # the one-wave window launch is the one launch's code
    assert e.max() <= RTOL_BUILDS, (name, e.max())


def test_the_shared_stream_gives_the_same_bits(batch):
    """steady_middle_stream off: the middle launch behind the early one on its stream; each problem's launch is the
    same code on either schedule."""
    eng = batch["eng"]
    hps = _batch(BATCHES["as the feedback said"])
    got, sw, launches = batch["behind"](hps)
    eng.steady_middle_stream = False
    try:
        old, sw_old, launches_old = batch["behind"](hps)
    finally:
        del eng.steady_middle_stream
    assert eng.steady_middle_stream and (launches, launches_old) == (3, 3) and np.array_equal(sw, sw_old)
    assert np.array_equal(got, old)
