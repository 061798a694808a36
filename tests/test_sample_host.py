"""CPU: the algebra the sampling sweeps implement (tests/sample_ref.py) against the oracle's matmul_lower after
factor, the centring rule, the sampler's host-side validation, and the presence of gf_sample_fused in the C-ABI."""
import os
import re

import numpy as np
import pytest

import gadfly_amd
from gadfly_amd import _lib
from oracle import seq
from tests import sample_ref, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", ["solar6", "mixed", "overdamped"])
def test_draw_column_recurrence_is_matmul_lower_after_factor(case):
    prob = {"solar6": lambda: util.solar_problem(J=6, N=3000),
            "mixed": lambda: util.generic_problem("mixed", 700),
            "overdamped": lambda: util.generic_problem("overdamped", 300)}[case]()
    c, a, U, V = util.oracle_matrices(prob, seq)
    t = prob["t"]
    eps = np.random.default_rng(11).normal(size=len(t))
    d, Wm, info = seq.factor(t, c, a, U, V)
    assert info == 0
    ref = seq.matmul_lower(t, c, U, Wm, eps * np.sqrt(d))
    got, d2, info2 = sample_ref.draw(t, c, a, U, V, eps)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print(f"{case}: recurrence vs matmul_lower after factor: {err:.2e}")
    assert info2 == 0
    assert err <= 1e-12
    assert np.max(np.abs(d2 - d) / d) <= 1e-12


def test_draw_recurrence_reports_the_failing_row():
    prob = util.generic_problem("mixed", 200)
    c, a, U, V = util.oracle_matrices(prob, seq)
    a = a.copy()
    a[57] = -1.0
    _, _, info = seq.factor(prob["t"], c, a, U, V)
    out, _, info2 = sample_ref.draw(prob["t"], c, a, U, V, np.ones(len(a)))
    assert info == info2 == 58 and np.all(np.isfinite(out[:57])) and np.all(np.isnan(out[57:]))


@pytest.mark.parametrize("size", [None, 3])
def test_centering_rule(size):
    import torch
    from gadfly_amd.batch import _center_draws
    rng = np.random.default_rng(5)
    B, N = 4, 37
    x = rng.normal(size=(B, N) if size is None else (B, size, N)) + 3.0
    got = _center_draws(torch.from_numpy(x.copy()), size).numpy()
    want = np.stack([sample_ref.center(x[b], size) for b in range(B)])
    assert got.shape == x.shape
    assert np.max(np.abs(got - want)) <= 1e-14
    # the statement itself: what the reference does to its (N,) / (size, N) result
    for b in range(B):
        r = x[b].copy()
        r -= r.mean(axis=0 if r.ndim == 2 else None)
        assert np.array_equal(r, want[b])


def _kernels(B, J=6):
    from gadfly_amd.synth import solar_like_hyperparameters
    return [gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0) for _ in range(B)]


def test_validation_happens_on_the_host():
    """Each of these is refused before any device call (no GPU here, and none is asked for)."""
    ks = _kernels(3)
    t = np.arange(50.0) * 6e-5
    with pytest.raises(ValueError, match="must be sorted"):
        gadfly_amd.BatchedSampler(ks, t[::-1])
    with pytest.raises(ValueError, match="only one of"):
        gadfly_amd.BatchedSampler(ks, t, yerr=1.0, diag=np.ones(50))
    with pytest.raises(ValueError, match="dimension mismatch"):
        gadfly_amd.BatchedSampler(ks, t, yerr=np.ones(49))
    with pytest.raises(ValueError, match="dimension mismatch"):
        gadfly_amd.BatchedSampler(ks, np.tile(t, (2, 1)))
    s = gadfly_amd.BatchedSampler(ks, t, yerr=1.0)
    assert (s.B, s.N) == (3, 50)
    for bad in (np.zeros((3, 51)), np.zeros((2, 50)), np.zeros((3, 2, 50))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            s.sample_device(normals=bad)
    with pytest.raises(ValueError, match="dimension mismatch"):
        s.sample_device(normals=np.zeros((3, 50)), size=2)
    # ragged: a list of the wrong length, series that are not sorted, normals that do not follow the lengths
    ragged = [t[:40], t[:50]]
    with pytest.raises(ValueError, match="dimension mismatch"):
        gadfly_amd.BatchedSampler(ks, ragged)
    with pytest.raises(ValueError, match="must be sorted"):
        gadfly_amd.BatchedSampler(ks[:2], [t[:40][::-1], t[:50]])
    with pytest.raises(ValueError, match="dimension mismatch"):
        gadfly_amd.BatchedSampler(ks[:2], ragged, yerr=[np.ones(40)])
    r = gadfly_amd.BatchedSampler(ks[:2], ragged, yerr=[np.ones(40), 2.0 * np.ones(50)], mean=[1.0, 2.0])
    assert list(r.rows) == [40, 50] and r.N == 50
    with pytest.raises(ValueError, match="dimension mismatch"):
        r.sample_device(normals=[np.zeros(40), np.zeros(49)])
    with pytest.raises(ValueError, match="dimension mismatch"):
        r.sample_device(normals=np.zeros((2, 50)))
    # kernels of different term structures do not make a batch
    from gadfly_amd.synth import solar_like_hyperparameters
    odd = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(7), texp=60.0)
    with pytest.raises(ValueError, match="term structure"):
        gadfly_amd.BatchedSampler(ks[:2] + [odd], t)


def test_gf_sample_fused_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "gadfly_hip.h")).read()
    assert re.search(r"\bint\s+gf_sample_fused\s*\(", header)
    assert "gf_sample_fused" in _lib.SIGNATURES
    # gf_loglike_fused's argument list, eps where y stands and out where z stands
    assert _lib.SIGNATURES["gf_sample_fused"] == _lib.SIGNATURES["gf_loglike_fused"]
    assert "BatchedSampler" in gadfly_amd.batch.__all__ and callable(gadfly_amd.sample_batch)
    _lib.build()
    lib = _lib.load()
    # argument errors are status codes: W = 65 with a real term has no fused sweep, and a batch needs a stride
    st = lib.gf_sample_fused(1, 16, 0, 1, 32, 8, 1, 0, *([None] * 8), None, 0, None, 0, None, 0,
                             *([None] * 5), None)
    assert st < 0 and b"width" in lib.gf_last_error()
    st = lib.gf_sample_fused(2, 16, 0, 0, 6, 8, 1, 0, *([None] * 8), None, 0, None, 0, None, 0,
                             *([None] * 5), None)
    assert st < 0 and b"gf_sample_fused" in lib.gf_last_error()
