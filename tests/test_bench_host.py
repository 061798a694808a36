"""CPU: bench.py's host side -- the walkers' proposals it builds in one pass are, value for value, the
hyperparameters jitter_hyperparameters gives (the benchmark's inputs), and the legs beyond the headline
are behind --full."""
import sys

import numpy as np

import bench
from gadfly_amd.core import Hyperparameters
from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters


def _per_walker(base, seeds):
    return [np.array([[p["hyperparameters"][k] for p in jitter_hyperparameters(base, s)] for s in seeds])
            for k in ("S0", "w0", "Q")]


def test_walker_proposals_are_jitter_hyperparameters_bit_for_bit():
    base = solar_like_hyperparameters(30)
    # seeds of the first and a later step, and of rank 1 (bench.py: 1000 + rank * 1000003 + step * E + e)
    seeds = [1000 + i for i in (0, 1, 977, 2047, 2048, 5 * 2048 + 1954, 1000003, 1000003 + 4 * 2048 + 7)]
    got = bench.walker_proposals(base, seeds)
    for g, w in zip(got, _per_walker(base, seeds)):
        assert g.dtype == w.dtype == np.float64 and g.shape == w.shape == (len(seeds), 30)
        assert g.tobytes() == w.tobytes()


def test_walker_proposals_keep_the_q_floor():
    # Q = 0.5 and 0.52: the jitter (+-10 %) takes them below 0.5 for some seeds, where the floor holds them
    base = Hyperparameters([dict(hyperparameters=dict(S0=1.0, w0=100.0, Q=q), metadata={}) for q in (0.5, 0.52, 3.0)])
    seeds = list(range(1000, 1064))
    got = bench.walker_proposals(base, seeds)
    want = _per_walker(base, seeds)
    assert np.any(want[2] == 0.5) and np.any(want[2][:, 1] > 0.5)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1", "--full"])
    assert bench.parse().full is True
