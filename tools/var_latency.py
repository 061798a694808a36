#!/usr/bin/env python
"""Latency of BatchedLogLikelihood.predict_device(return_var=True): one JSON line per leg, medians of
`--reps` calls after one warm-up, HIP events around each launch -- (a) walkers B = 2048, N = 1e5, J = 30 at the
observed times; (b) cfg3-shaped B = 256, N = 65 000, J = 20 on a grid that lost 10 % of its cadences, the M = 7222
queries filling them; (c) one star B = 1, N = 1e5, J = 30 at the observed times.  `--shapes a,c` runs a subset.

mean_device_ms: the launches of predict_device() without return_var on the same batch (gf_solve_batch, and
gf_predict_batch_at in leg b): the route the means have had since DESIGN.md 3.9 / 3.11;
var_device_ms: the launches of predict_device(return_var=True) (gf_var_batch in gf_solve_batch's place);
var_over_mean their ratio (the arithmetic suggests about 2: four forward-row equivalents per row against two);
var_api_ms: the call and a device synchronise, wall time.

`--loop Q` adds the per-kernel route at Q queries: GaussianProcess(kernel_b, t, yerr).predict(y, t*, return_var=True)
one kernel at a time (one right-hand side per query through the stored factor), wall time per problem (median over
`--loop-problems` problems after one warm-up), against predict(t=t*, return_var=True) of the whole batch at the same Q
queries, results on the host as numpy: loop_scaled_ms = per problem times B, speedup_over_loop their ratio."""
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
from gadfly_amd.terms import SHOTerm, TermConvolution, TermSum  # noqa: E402

SHAPES = {"a": (2048, 100_000, 30), "b": (256, 65_000, 20), "c": (1, 100_000, 30)}


def kernel_of(S0, w0, Q, delta):
    return TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q)) for s, w, q in zip(S0, w0, Q)]),
                           delta)


def walkers(B, J, rng):
    """(kernel, S0, w0, Q (B, J), delta): proposals around the solar-like kernel's own parameters (Q untouched)."""
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
    base = [np.array([[getattr(tm, k) for tm in kern.term.terms]]) for k in ("S0", "w0", "Q")]
    S0, w0 = (np.repeat(b, B, axis=0) * np.exp(0.05 * rng.normal(size=(B, J))) for b in base[:2])
    return kern, S0, w0, np.repeat(base[2], B, axis=0), float(kern.delta)


def timed(ev, reps, **kw):
    """Medians over `reps` calls (after one warm-up) of the device time of predict_device(**kw)'s launches and of the
    call's wall time with a synchronise; whether every result is finite; the workspace plan."""
    dev, wall, finite = [], [], True
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.predict_device(**kw)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ev.last_predict_device_ms)
        finite = all(bool(torch.isfinite(x).all()) for x in (out if isinstance(out, tuple) else (out,)))
        del out
    return float(np.median(dev[1:])), float(np.median(wall[1:])), finite, ev.last_predict_plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=0, help="queries of the per-kernel loop leg (0 skips it)")
    ap.add_argument("--loop-problems", type=int, default=4)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(2024))
    for name in args.shapes.split(","):
        B, N, J = SHAPES[name]
        kern, S0, w0, Q, delta = walkers(B, J, rng)
        ts = None
        if name == "b":                                 # a grid that lost 10 % of its cadences: fill them
            grid = uniform_times(int(round(N / 0.9)), 60.0)
            keep = np.zeros(len(grid), dtype=bool)
            keep[rng.choice(len(grid), size=N, replace=False)] = True
            t, ts = grid[keep], grid[~keep]
        else:
            t = uniform_times(N, 60.0)
        y = 100.0 * rng.normal(size=N)
        ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
        pack = sho_coefficient_pack(S0, w0, Q, delta)
        kw = dict(pack_or_kernels=pack) if ts is None else dict(pack_or_kernels=pack, t=ts)
        m_dev, m_api, m_fin, _ = timed(ev, args.reps, **kw)
        v_dev, v_api, v_fin, plan = timed(ev, args.reps, return_var=True, **kw)
        rec = dict(leg="var_" + name, B=B, N=N, M=0 if ts is None else len(ts), J=J, W=2 * J,
                   mean_device_ms=round(m_dev, 2), var_device_ms=round(v_dev, 2), var_over_mean=round(v_dev / m_dev, 2),
                   mean_api_ms=round(m_api, 2), var_api_ms=round(v_api, 2), finite=m_fin and v_fin,
                   workspace_bytes=int(plan[0]), groups=int(plan[1]), group_size=int(plan[2]), reps=args.reps)
        if ts is not None:
            rec["var_at_share_ms"] = round(ev.last_predict_at_ms, 2)
        print(json.dumps(rec), flush=True)
        if args.loop > 0:
            q = np.sort(rng.uniform(t[0], t[-1], args.loop))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.predict(pack, t=q, return_var=True)
            batch_ms = (time.perf_counter() - t0) * 1e3
            walls = []
            for b in range(args.loop_problems + 1):     # (the first problem warms up and is dropped)
                i = b % B
                kb = kernel_of(S0[i], w0[i], Q[i], delta)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gp = gadfly_amd.GaussianProcess(kb, t=t, yerr=30.0, device="cuda:0")
                gp.predict(y, t=q, return_var=True)
                walls.append(time.perf_counter() - t0)
                del gp
            per = float(np.median(walls[1:])) * 1e3
            print(json.dumps(dict(leg="var_loop_" + name, B=B, N=N, M=args.loop, J=J, batch_numpy_ms=round(batch_ms, 2),
                                  loop_problems=args.loop_problems, loop_ms_per_problem=round(per, 2),
                                  loop_scaled_ms=round(per * B, 1),
                                  speedup_over_loop=round(per * B / batch_ms, 2))), flush=True)
        del ev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
