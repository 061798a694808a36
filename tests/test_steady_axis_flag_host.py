"""Host: where the streamed engine sets GF_SWEEP_AXIS_PROVEN on its finishing launches (StreamingBatch._finish_variant,
_steady_axis_proven, _finish_launch).  No device: a bare StreamingBatch on CPU tensors, the engine's own
axis scan, and a stub library that records the `variant` each finishing launch is handed.

The bit is set exactly where the scan proves BOTH of the tail's tests for every spacing behind arm_from:
  - off the cadence: 2 jit + (roundings) < 2e-6 / wmax;
  - a gap: cad_max + jit < 1.5 dt_med and block > 1 (the pack's block is the largest with (block - 1) 1.5 cmax dt_med
    <= span, so the kernel's threshold gap / cmax_b is at least 1.5 dt_med)."""
import types

import numpy as np
import pytest
import torch

from gadfly_amd import _lib
from gadfly_amd.engine import CoefficientPack, StreamingBatch

N, B, J = 4096, 2, 3
CADENCE = 60e-6
FINISH_VARIANT_SLOT = 5         # B, N, Jr, Jc, block, variant, ... (include/gadfly_hip.h)


class _StubLib:
    """Records (name, variant) of every finishing launch; every call succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gf_steady_finish"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args[FINISH_VARIANT_SLOT]))
            return 0
        return call


def _engine(t, wmax=2.0e4, block=64, stream_block=0, dt_med=None):
    f64 = torch.float64
    eng = object.__new__(StreamingBatch)
    eng.torch, eng.device, eng.lib = torch, torch.device("cpu"), _StubLib()
    eng.B, eng.N, eng.Jr, eng.Jc = B, t.shape[-1], 0, J
    eng.t = torch.tensor(np.atleast_2d(t), dtype=f64)
    eng.y = torch.zeros((1, eng.N), dtype=f64)
    eng.diag = None
    eng.info = torch.zeros((B,), dtype=torch.int32)
    eng._steady = torch.zeros((B, 8), dtype=f64)
    eng.acc = torch.zeros((B, 3), dtype=f64)
    eng._tmax = float(np.max(np.abs(t)))
    eng._dt_med = float(np.median(np.diff(np.atleast_2d(t)[0]))) if dt_med is None else dt_med
    eng._steady_axis, eng._steady_cad_max, eng._steady_scanned, eng.steady_axis_proven = None, None, None, True
    pack = CoefficientPack(torch.zeros((2, B, 1), dtype=f64), torch.zeros((4, B, J), dtype=f64),
                           torch.zeros((B,), dtype=f64), torch.zeros((B, 2 * J), dtype=f64), torch.ones((B,), dtype=f64),
                           block, wmax, stream_block, wmax)
    return eng, pack


def _variants(eng, pack, block, variant):
    """The variant each of the three finishing entry points is handed behind a sweep with (block, variant)."""
    stream = types.SimpleNamespace(cuda_stream=0)
    fv = eng._finish_variant(pack, block, variant)
    eng._finish_launch("gf_steady_finish", stream, pack, block, fv)
    eng._finish_launch("gf_steady_finish_window", stream, pack, block, fv, 1, 100)
    eng._finish_launch("gf_steady_finish_chunked", stream, pack, block, fv, 1, 100, 16, None)
    names = [c[0] for c in eng.lib.calls]
    assert names == ["gf_steady_finish", "gf_steady_finish_window", "gf_steady_finish_chunked"]
    got = {c[1] for c in eng.lib.calls}
    assert len(got) == 1
    eng.lib.calls.clear()
    return got.pop()


PROVEN = _lib.GF_SWEEP_AXIS_PROVEN


def test_the_bit_is_none_of_the_sweeps_bits():
    assert PROVEN == 0x400
    assert PROVEN & (_lib.GF_SWEEP_ZERO_START | _lib.GF_SWEEP_LONG_SPAN | 0xff) == 0


def test_regular_axis_sets_the_bit_on_every_finishing_launch():
    t = np.arange(N) * CADENCE
    eng, pack = _engine(t)
    arm, jit = eng._steady_axis_scan()
    assert arm == 0 and jit < 1e-6 / pack.wmax and eng._steady_arm_from.__func__ is StreamingBatch._steady_arm_from
    assert _variants(eng, pack, 64, _lib.GF_SWEEP_AUTO) == PROVEN
    # the long span's block goes with the long span's bit: both stay
    eng2, pack2 = _engine(t, block=16, stream_block=64)
    eng2._steady_axis_scan()
    assert _variants(eng2, pack2, 64, _lib.GF_SWEEP_LONG_SPAN) == PROVEN | _lib.GF_SWEEP_LONG_SPAN
    # switched off: the kernel's own tests
    eng.steady_axis_proven = False
    assert _variants(eng, pack, 64, _lib.GF_SWEEP_AUTO) == 0


def test_no_scan_no_bit():
    """An axis planted without the scan, or over its result (tests that force arm_from), carries no proof."""
    eng, pack = _engine(np.arange(N) * CADENCE)
    eng._steady_axis = (0, 0.0)
    assert _variants(eng, pack, 64, 0) == 0
    eng._steady_axis = None
    eng._steady_axis_scan()
    assert _variants(eng, pack, 64, 0) == PROVEN
    eng._steady_axis = (0, 0.0)
    assert _variants(eng, pack, 64, 0) == 0


def test_jitter_inside_the_arming_limit_but_not_twice_inside():
    """_steady_arm_from arms for jit < 1e-6 / wmax; the proof needs 2 jit < 2e-6 / wmax with the roundings of the
    frozen cadence and of the differences on top: the same limit, reached from below.  A jitter of 0.99 of the limit
    keeps the bit; one a rounding below the limit (armed, but the roundings are not covered) loses it.  (The scan
    itself leaves only spacings within 8 ulp of the largest stamp behind arm_from, so the figures are planted.)"""
    wmax = 2.0e4
    lim = 1e-6 / wmax
    eng, pack = _engine(np.arange(N) * CADENCE, wmax=wmax)
    arm, jit = eng._steady_axis_scan()
    assert arm == 0 and jit <= 8.0 * 2.0 ** -52 * eng._tmax
    eng._steady_axis = eng._steady_scanned = (0, 0.99 * lim)
    assert _variants(eng, pack, 64, 0) == PROVEN
    eng._steady_axis = eng._steady_scanned = (0, float(np.nextafter(lim, 0.0)))     # armed (jit < lim) ...
    assert eng._steady_axis[1] < lim
    assert _variants(eng, pack, 64, 0) == 0                     # ... but 2 jit + roundings is not below 2e-6 / wmax
    eng._steady_axis = eng._steady_scanned = (0, lim)
    assert _variants(eng, pack, 64, 0) == 0


def test_gap_bound_that_cannot_be_shown_leaves_the_bit_off():
    """The series starts on a cadence of 60 us and ends on one of 96 us: regular behind the change (jitter zero, well
    inside _steady_arm_from's limit), but the final cadence is 1.6 medians -- the host's bound on the kernel's gap
    threshold, 1.5 dt_med, does not cover it.  So is every axis under block = 1 (gap = 0: every row a reset)."""
    n, n1 = 2 * N, 3 * N // 2
    t = np.concatenate([np.arange(n1) * CADENCE, (n1 - 1) * CADENCE + np.arange(1, n - n1 + 1) * 1.6 * CADENCE])
    eng, pack = _engine(t)
    arm, jit = eng._steady_axis_scan()
    assert 0 < arm < n and n - arm >= StreamingBatch.STEADY_MIN_ROWS
    assert jit < 1e-6 / pack.wmax                   # the steady mode would arm
    assert eng._dt_med == pytest.approx(CADENCE) and eng._steady_cad_max == pytest.approx(1.6 * CADENCE)
    assert _variants(eng, pack, 64, 0) == 0
    # the same axis with a median that covers its final cadence (a caller's axis_stats): shown
    eng2, pack2 = _engine(t, dt_med=1.2 * CADENCE)
    eng2._steady_axis_scan()
    assert _variants(eng2, pack2, 64, 0) == PROVEN
    # block = 1, and a block that is not the pack's
    eng3, pack3 = _engine(np.arange(N) * CADENCE, block=1)
    eng3._steady_axis_scan()
    assert _variants(eng3, pack3, 1, 0) == 0
    eng4, pack4 = _engine(np.arange(N) * CADENCE, block=32)
    eng4._steady_axis_scan()
    assert _variants(eng4, pack4, 64, 0) == 0 and _variants(eng4, pack4, 32, 0) == PROVEN
