"""GPU: the overlapped finishing schedule with a middle window at the evaluator -- the early switchers'
tails in one-wave launches behind the split's tile, the middle window's in chunks on the same side stream behind tile
k_m's sweep, the last ones' in chunks behind the last tile, and behind the split the sweeps that add their own tiles to
acc (gf_steady_sweep_reduced).  On tests/test_gpu_steady_overlap.py's batch, whose walkers switch in tiles 0, 1, 2 and 0
of 4096 rows, with the boundaries forced so that each window holds a problem, chunks of 16 blocks as in
tests/test_gpu_steady_chunk.py, and that file's bound between the chunked and the one-wave routes."""
import numpy as np
import pytest

from tests.test_gpu_steady import _evaluator, _rel, _series
from tests.test_gpu_steady_chunk import CHUNK_BLOCKS, RTOL_BUILDS
from tests.test_gpu_steady_finish import N_FIN, T_FIN
from tests.test_gpu_steady_overlap import _spread_batch, _spread_terms

pytestmark = pytest.mark.gpu
J = 30


def _kernels(hps):
    import gadfly_amd
    return [gadfly_amd.StellarOscillatorKernel(hp, texp=60.0) for hp in hps]


@pytest.fixture(scope="module")
def batch(hip):
    """The evaluator, and per set of hyperparameters the one-launch schedule's values and switch rows (computed once)."""
    t, y = _series(N_FIN, seed=29)
    hps, _ = _spread_batch(J)
    ev, _ = _evaluator(hps, t, y, T_FIN)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    eng.STEADY_OVERLAP_MIN_B, eng.STEADY_MIDDLE_MIN_B, eng._steady_chunk_blocks = 1, 1, CHUNK_BLOCKS
    eng.time_factor = True
    refs = {}

    def reference(name, hps_):
        if name not in refs:
            eng.steady_overlap = False
            ref = ev.evaluate(_kernels(hps_))
            sw = eng.steady_switch_rows().copy()
            assert eng.steady_used and np.all(sw > 0) and not eng.steady_violations().cpu().numpy().any()
            refs[name] = (ref, sw)
        return refs[name]

    def overlapped(hps_, split, mid, feedback=None):
        """One evaluation on the overlapped schedule with forced boundaries, or behind the given feedback scalars."""
        import torch
        eng.steady_overlap, eng.finish_events = True, []
        if feedback is None:
            eng._steady_feedback, eng._steady_split, eng._steady_mid = None, split, mid
        else:
            done = torch.cuda.Event()
            done.record()
            done.synchronize()
            eng._steady_feedback = (torch.tensor(feedback, dtype=torch.float64), done)
        got = ev.evaluate(_kernels(hps_))
        return got, eng.steady_switch_rows().copy(), len(eng.finish_events)

    return dict(ev=ev, eng=eng, hps=hps, reference=reference, overlapped=overlapped)


def test_three_windows_each_with_a_problem(batch):
    eng, hps = batch["eng"], batch["hps"]
    ref, sw0 = batch["reference"]("spread", hps)
    assert ((sw0 - 1) // T_FIN).tolist() == [0, 1, 2, 0]
    got, sw, launches = batch["overlapped"](hps, T_FIN, 2 * T_FIN)
    e = _rel(got, ref)
    print(f"switch rows {sw.tolist()}: three windows against the one launch {e.tolist()}")
    assert np.array_equal(sw, sw0) and launches == 3
    assert eng._steady_mid_ws is not None and eng._steady_mid_ws[1] == CHUNK_BLOCKS
    assert e.max() <= RTOL_BUILDS
    early = sw <= T_FIN
    assert np.array_equal(got[early], ref[early])           # the one-wave window launch is the one launch's code
    # the sweeps' own sums behind the split are the separate reduction's bits
    eng.steady_sweep_reduces = False
    try:
        two_calls, _, launches = batch["overlapped"](hps, T_FIN, 2 * T_FIN)
    finally:
        eng.steady_sweep_reduces = True
    assert launches == 3 and np.array_equal(two_calls, got)


@pytest.mark.parametrize("mid", ["the split's own tile", "the last tile", "beyond the series", "no multiple of the tile"])
def test_unusable_middle_gives_the_two_launch_schedule(batch, mid):
    eng, hps = batch["eng"], batch["hps"]
    ntiles = (N_FIN + T_FIN - 1) // T_FIN
    mid_end = {"the split's own tile": T_FIN, "the last tile": ntiles * T_FIN, "beyond the series": (ntiles + 3) * T_FIN,
               "no multiple of the tile": 2 * T_FIN + 64}[mid]
    two, sw, launches = batch["overlapped"](hps, T_FIN, 0)
    assert launches == 2
    got, sw2, launches = batch["overlapped"](hps, T_FIN, mid_end)
    assert launches == 2 and np.array_equal(sw2, sw) and np.array_equal(got, two)


def test_small_batches_take_no_middle_window(batch):
    eng, hps = batch["eng"], batch["hps"]
    keep = eng.STEADY_MIDDLE_MIN_B
    eng.STEADY_MIDDLE_MIN_B = type(eng).STEADY_MIDDLE_MIN_B
    try:
        assert eng.B < eng.STEADY_MIDDLE_MIN_B
        _, _, launches = batch["overlapped"](hps, T_FIN, 2 * T_FIN)
    finally:
        eng.STEADY_MIDDLE_MIN_B = keep
    assert launches == 2


def test_switch_rows_outside_the_predicted_windows(batch):
    """One feedback -- the spread batch's own switch rows -- and evaluations whose problems switch elsewhere: every
    problem is finished exactly once (a tail missed or taken twice shows at the size of the tail's sum)."""
    eng, hps = batch["eng"], batch["hps"]
    _, sw0 = batch["reference"]("spread", hps)
    feedback = [float(sw0.min()), float(np.sort(sw0)[1]), float(np.sort(sw0)[2]), float(sw0.max())]
    others = {
        "spread": hps,
        "rotated": [hps[2], hps[0], hps[1], hps[3]],
        "all early": [_spread_terms(J, 0, k0=k0) for k0 in range(4)],
        "all late": [_spread_terms(J, 2, k0=k0) for k0 in range(4)],
    }
    for name, hps_ in others.items():
        ref, sw_ref = batch["reference"](name, hps_)
        got, sw, launches = batch["overlapped"](hps_, None, None, feedback=feedback)
        assert (eng._steady_split, eng._steady_mid) == (T_FIN, 2 * T_FIN), name
        windows = np.searchsorted([T_FIN + 1, 2 * T_FIN + 1], sw, side="right")
        e = _rel(got, ref)
        print(f"{name}: switch rows {sw.tolist()} in windows {windows.tolist()}, against the one launch {e.max():.2e}")
        assert launches == 3 and np.array_equal(sw, sw_ref), name
        assert e.max() <= RTOL_BUILDS, (name, e.tolist())
    assert (np.searchsorted([T_FIN + 1, 2 * T_FIN + 1], batch["reference"]("rotated", others["rotated"])[1], side="right")
            .tolist() == [2, 0, 1, 0])
