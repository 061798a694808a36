#!/usr/bin/env python
"""Two more randomized sweeps (development, next to tools/random_sweep.py):
  jd    FIRST COUNT   tests/test_gpu_random.py::test_random_problem with every time axis moved to t + 2.12e5 (a JD-based
                      axis: phases far beyond 4e6 rad, the row generator's rounded-phase steps -- RowGen::qmode -- on)
  wide  FIRST COUNT   tests/test_gpu_random_wide.py::test_random_wide_kernel (random WIDE kernels, W = 64 ... 176, two
                      walkers each: streamed, scaled_wide, three-sweep and two-sweep time-parallel evaluation -- the
                      latter with the pivot-sign check of every chunk: a false alarm shows up as a non-finite value --
                      and the stored WideFactor's chunk-parallel solves) over any seed range"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_random as T  # noqa: E402
from gadfly_amd import _lib as hip  # noqa: E402

what, first, count = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
hip.require_device()
bad, skipped = [], 0

if what == "jd":
    base = T._problem

    def moved(seed):
        p = base(seed)
        p["t"] = p["t"] + 2.12e5
        return p

    T._problem = moved
    for seed in range(first, first + count):
        try:
            T.test_random_problem(hip, seed)
        except pytest.skip.Exception:
            skipped += 1
        except Exception as e:      # noqa: BLE001
            bad.append(seed)
            print("FAIL", seed, repr(e)[:300], flush=True)
        if (seed - first) % 50 == 49:
            print(f"... {seed - first + 1} seeds, {len(bad)} failures, {skipped} skipped", flush=True)
else:
    import test_gpu_random_wide as TW
    for seed in range(first, first + count):
        try:
            TW.test_random_wide_kernel(hip, seed)
        except pytest.skip.Exception:
            skipped += 1
        except Exception as e:      # noqa: BLE001
            bad.append(seed)
            print("FAIL", seed, repr(e)[:300], flush=True)
        if (seed - first) % 25 == 24:
            print(f"... {seed - first + 1} seeds, {len(bad)} failures, {skipped} skipped", flush=True)
print(f"{what}: {count} seeds from {first}: {len(bad)} failures, {skipped} skipped")
sys.exit(1 if bad else 0)
