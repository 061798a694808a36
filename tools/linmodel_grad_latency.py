#!/usr/bin/env python
"""Latency of BatchedLogLikelihood.linear_value_and_grad, profile and marginal, on the two legs of
tools/linmodel_latency.py, in one process: one JSON line per shape and mode, medians of `--reps` calls after one warm-up.

  (a) 64 stars, N = 74 800, J = 20, seventeen quarters with a cubic each (R = 68);
  (b) walkers B = 2048, N = 1e5, J = 30, one quarter with a cubic (R = 4).

Per call: the HIP-event time of every stage (gram, residual, grad, and for the marginal mode solve, product, quadform;
`stage_ms`), their sum `device_ms`, and the wall time of the whole call with its host work `call_ms` (the fit on the
host and the chain rule to S0, w0, Q included).
GATE: the route the package offered before is central differences through fit_linear, 6 J evaluations per gradient:
`fd_ms` = 6 J times fit_linear's wall time, measured here in the same process.  The call must beat it by more than
1.2 x (`gate_ok`; the tool exits 1 otherwise).  Reported without a gate: the ratio to value_and_grad on the same batch
(`vs_value_and_grad`, wall time over wall time) and gf_quadform_grad's share of the device time (`quadform_share`).
`--shapes a` runs a subset, `--out` appends the lines to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd.batch import sho_coefficient_pack  # noqa: E402
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times  # noqa: E402

SHAPES = {"a": (64, 74_800, 20, 17), "b": (2048, 100_000, 30, 1)}
ORDER = 3
FLOOR = 1.2


def wall_ms(fn, reps):
    """(median wall time in ms over `reps` calls of fn() after one warm-up, device idle before and after each; what
    fn returned for every timed call)."""
    fn()
    torch.cuda.synchronize()
    ms, outs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        outs.append(fn())
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), outs


def measure(name, reps):
    B, N, J, S = SHAPES[name]
    rng = np.random.default_rng(33)
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
    terms = kern.term.terms if hasattr(kern, "term") else kern.terms
    S0, w0, Q = (np.tile(np.array([[getattr(tm, k) for tm in terms]]), (B, 1)) for k in ("S0", "w0", "Q"))
    S0 = S0 * (1.0 + 0.1 * rng.uniform(size=(B, 1)))        # B different kernels of one term structure
    delta = float(kern.delta)
    t = uniform_times(N, 60.0)
    breaks = np.linspace(0, N, S + 1).astype(np.int64)
    A = gadfly_amd.quarter_polynomial_basis(t, breaks, ORDER)
    R = A.shape[1]
    y = 100.0 * rng.normal(size=(B, N)) + (A @ rng.normal(size=R))[None, :]
    ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
    pk = sho_coefficient_pack(S0, w0, Q, delta)
    fit_ms, _ = wall_ms(lambda: ev.fit_linear(A, pk), reps)
    vg_ms, _ = wall_ms(lambda: ev.value_and_grad(S0, w0, Q, delta), reps)
    vg_device_ms = float(ev.last_grad_device_ms)
    fd_ms = 6 * J * fit_ms
    lines = []
    for marginal in (False, True):
        def call():
            ev.linear_value_and_grad(A, S0, w0, Q, delta, marginal=marginal)
            return dict(ev.last_linear_grad_ms)
        call_ms, stages = wall_ms(call, reps)
        stage_ms = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        device_ms = float(sum(stage_ms.values()))
        lines.append(dict(
            tool="linmodel_grad_latency", shape=name, mode="marginal" if marginal else "profile", B=B, N=N, J=J, R=R,
            reps=reps, call_ms=call_ms, device_ms=device_ms, stage_ms=stage_ms, fit_linear_ms=fit_ms, fd_ms=fd_ms,
            speedup_over_fd=fd_ms / call_ms, gate_floor=FLOOR, gate_ok=bool(fd_ms / call_ms > FLOOR),
            value_and_grad_ms=vg_ms, value_and_grad_device_ms=vg_device_ms, vs_value_and_grad=call_ms / vg_ms,
            quadform_share=stage_ms.get("quadform", 0.0) / device_ms,
            grad_groups=int(ev.last_linear_grad_plan[1]), device=torch.cuda.get_device_name(0)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ok = True
    for name in args.shapes.split(","):
        for rec in measure(name, args.reps):
            ok &= rec["gate_ok"]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
