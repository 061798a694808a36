#!/usr/bin/env python
"""Latency of BatchedLogLikelihood.sample_conditional_device: one JSON line per leg and size, medians
of `--reps` calls after one warm-up, HIP events around the launches.

Leg b (DESIGN.md 3.11's): B = 256, N = 65 000, J = 20 on a grid that lost 10 % of its cadences, the M = 7222 queries
filling them, size in 1, 4, 16.  sweeps / assembly / solve / at: the parts of the call, each between HIP events
(last_conditional_ms); device_ms: their sum; api_ms: the whole call and a synchronise, wall time.  loop_ms: what the
package could do for the same draws without the R-right-hand-side kernels -- per draw one BatchedSampler sweep on the
union axis (between HIP events), the residual as the evaluator's data and a fresh predict_device(t=...) on it
(gf_solve_batch + gf_predict_batch_at, each with its own factorisation: last_predict_device_ms) --, summed;
loop_api_ms its wall time; speedup = loop_ms / device_ms.

Leg w (walkers): B = 2048, N = 1e5, J = 30 at the observed stamps, size 1 and 4: the solve's device time, and the time
per extra right-hand side against the first, (solve_4 - solve_1) / 3 / solve_1 (a block always carries its RB columns,
so this is small by construction) and against gf_solve_batch's one right-hand side on the same batch,
(solve_4 - solve_batch) / 3 / solve_batch.
`--legs b,w` and `--sizes 1,4,16` pick a subset."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd import conddraw  # noqa: E402
from gadfly_amd.batch import sho_coefficient_pack  # noqa: E402
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times  # noqa: E402
from gadfly_amd.terms import SHOTerm, TermConvolution, TermSum  # noqa: E402


def walkers(B, J, rng):
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
    base = [np.array([[getattr(tm, k) for tm in kern.term.terms]]) for k in ("S0", "w0", "Q")]
    S0, w0 = (np.repeat(b, B, axis=0) * np.exp(0.05 * rng.normal(size=(B, J))) for b in base[:2])
    return kern, S0, w0, np.repeat(base[2], B, axis=0), float(kern.delta)


def between_events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def new_route(ev, pack, ts, size, reps):
    whole, parts, finite = [], [], True
    for i in range(reps + 1):
        ms, out = between_events(lambda: ev.sample_conditional_device(pack, t=ts, size=size, seed=i))
        whole.append(ms)
        parts.append(dict(ev.last_conditional_ms))
        parts[-1]["device_ms"] = sum(parts[-1].values())
        finite = bool(torch.isfinite(out).all())
        del out
    med = lambda xs: round(float(np.median(xs[1:])), 2)      # noqa: E731
    return med(whole), {k: med([p[k] for p in parts]) for k in parts[0]}, finite


def old_loop(kernels, pack, t, ts, yerr, y, size, reps):
    """size x (one sampler sweep on the union axis + a fresh predict_device(t=...) on the residual), on an evaluator
    of its own whose data are per problem."""
    ev = gadfly_amd.BatchedLogLikelihood(kernels, t, np.tile(y, (len(kernels), 1)), yerr=yerr)
    ax = conddraw.union_axes(t, ts)
    sampler = gadfly_amd.BatchedSampler(kernels, ax.u[0])
    dev = ev.engine.device
    orow = torch.as_tensor(ax.obs_rows[0], device=dev)
    qrow = torch.as_tensor(ax.query_rows[0], device=dev)
    yd = torch.as_tensor(y, device=dev)
    B, N = ev.B, len(t)

    def run():
        out, dev_ms, pairs = [], 0.0, []
        for _ in range(size):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            w = sampler.sample_device(include_mean=False, center=False)
            e1.record()
            pairs.append((e0, e1))
            eta = torch.randn((B, N), dtype=torch.float64, device=dev)
            ev.engine.set_y(yd[None, :] - w[:, orow] - yerr * eta)
            out.append(w[:, qrow] + ev.predict_device(pack, t=ts, include_mean=False))
            dev_ms += ev.last_predict_device_ms
        torch.cuda.synchronize()
        return dev_ms + sum(a.elapsed_time(b) for a, b in pairs)

    ms, wall = [], []
    for _ in range(reps + 1):
        w_ms, d_ms = between_events(run)
        ms.append(d_ms)
        wall.append(w_ms)
    return round(float(np.median(ms[1:])), 2), round(float(np.median(wall[1:])), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="b,w")
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(2024))
    for leg in args.legs.split(","):
        if leg == "b":
            B, N, J = 256, 65_000, 20
            kern, S0, w0, Q, delta = walkers(B, J, rng)
            grid = uniform_times(int(round(N / 0.9)), 60.0)
            keep = np.zeros(len(grid), dtype=bool)
            keep[rng.choice(len(grid), size=N, replace=False)] = True
            t, ts = grid[keep], grid[~keep]
            y = 100.0 * rng.normal(size=N)
            ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
            host = sho_coefficient_pack(S0, w0, Q, delta)
            kernels = [TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q))
                                                 for s, w, q in zip(S0[b], w0[b], Q[b])]), delta) for b in range(B)]
            for size in (int(s) for s in args.sizes.split(",")):
                dev_ms, parts, finite = new_route(ev, host, ts, size, args.reps)
                loop_ms, loop_api = old_loop(kernels, host, t, ts, 30.0, y, size, args.reps)
                print(json.dumps(dict(leg="cond_b", B=B, N=N, M=len(ts), J=J, W=2 * J, size=size, api_ms=dev_ms,
                                      **parts, loop_ms=loop_ms, loop_api_ms=loop_api,
                                      speedup=round(loop_ms / parts["device_ms"], 2), finite=finite,
                                      rhs_block=int(ev.engine.lib.gf_solve_batch_rhs_block(2 * J)),
                                      workspace_bytes=int(ev.last_predict_plan[0]), groups=int(ev.last_predict_plan[1]),
                                      reps=args.reps)), flush=True)
        elif leg == "w":
            B, N, J = 2048, 100_000, 30
            kern, S0, w0, Q, delta = walkers(B, J, rng)
            t = uniform_times(N, 60.0)
            y = 100.0 * rng.normal(size=N)
            ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
            pack = sho_coefficient_pack(S0, w0, Q, delta)
            rec = {}
            for size in (1, 4):
                dev_ms, parts, finite = new_route(ev, pack, None, size, args.reps)
                rec[size] = parts["solve"]
                print(json.dumps(dict(leg="cond_w", B=B, N=N, J=J, W=2 * J, size=size, api_ms=dev_ms, **parts,
                                      finite=finite, workspace_bytes=int(ev.last_predict_plan[0]),
                                      groups=int(ev.last_predict_plan[1]), reps=args.reps)), flush=True)
            one = []
            for _ in range(args.reps + 1):              # gf_solve_batch on the same batch: one right-hand side
                ev.predict_device(pack)
                one.append(ev.last_predict_device_ms)
            one = round(float(np.median(one[1:])), 2)
            print(json.dumps(dict(leg="cond_w_ratio", solve_batch_ms=one, solve_1_ms=rec[1], solve_4_ms=rec[4],
                                  extra_rhs_over_first=round((rec[4] - rec[1]) / 3.0 / rec[1], 3),
                                  extra_rhs_over_solve_batch=round((rec[4] - one) / 3.0 / one, 3))), flush=True)
        del ev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
