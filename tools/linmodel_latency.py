#!/usr/bin/env python
"""Latency of BatchedLogLikelihood.linear_gram_device against the route it replaces, in one process:
one JSON line per shape, medians of `--reps` calls after one warm-up, HIP events around each route.

  (a) 64 stars, N = 74 800, J = 20, seventeen quarters with a cubic each (R = 68);
  (b) walkers B = 2048, N = 1e5, J = 30, one quarter with a cubic (R = 4).

gram_ms: linear_gram_device(A) -- one forward sweep, the products summed on the device;
solve_ms: apply_inverse_device([A | y]) and the torch product [A | y]^T alpha -- forward sweep, recompute, backward
sweep per block of right-hand sides, (B, R + 1, N) doubles written.  speedup = solve_ms / gram_ms; agreement: the
largest difference of the two Gram matrices over sqrt(G_ii G_jj).  `--shapes a` runs a subset, `--out` appends the
lines to a file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times  # noqa: E402

SHAPES = {"a": (64, 74_800, 20, 17), "b": (2048, 100_000, 30, 1)}
ORDER = 3


def device_ms(fn, reps):
    """Median over `reps` calls of the HIP-event time around fn(), after one warm-up; the last result."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), out


def measure(name, reps):
    B, N, J, S = SHAPES[name]
    rng = np.random.default_rng(33)
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
    t = uniform_times(N, 60.0)
    breaks = np.linspace(0, N, S + 1).astype(np.int64)
    A = gadfly_amd.quarter_polynomial_basis(t, breaks, ORDER)
    R = A.shape[1]
    y = 100.0 * rng.normal(size=(B, N)) + (A @ rng.normal(size=R))[None, :]
    ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
    Ad = torch.as_tensor(A, device="cuda")
    yd = torch.as_tensor(y, device="cuda")
    rhs = torch.cat([Ad.T[None].expand(B, R, N), yd[:, None, :]], dim=1).contiguous()         # (B, R + 1, N)

    def new():
        return ev.linear_gram_device(A)[0]              # (the upload of A is inside the events)

    def old():
        alpha = ev.apply_inverse_device(rhs)
        return torch.matmul(rhs, alpha.transpose(1, 2))

    gram_ms, g = device_ms(new, reps)
    plan = ev.last_linear_plan
    solve_ms, go = device_ms(old, reps)
    g, go = g.cpu().numpy(), go.cpu().numpy()
    d = np.sqrt(np.einsum("bii->bi", g))
    diff = float(np.max(np.abs(g - go) / (d[:, :, None] * d[:, None, :])))
    return dict(tool="linmodel_latency", shape=name, B=B, N=N, J=J, R=R, reps=reps, gram_ms=gram_ms,
                solve_ms=solve_ms, speedup=solve_ms / gram_ms, agreement=diff,
                gram_workspace_bytes=int(plan[0]), gram_groups=int(plan[1]),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for name in args.shapes.split(","):
        line = json.dumps(measure(name, args.reps))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
