#!/usr/bin/env python
"""Latency of BatchedLogLikelihood.predict_device: one JSON line per leg and variant, medians of 5 calls
-- (a) walkers B = 2048, N = 1e5, J = 30; (b) cfg3-shaped B = 256, N = 65 000, J = 20; (c) one star B = 1, N = 1e5,
J = 30 -- each without and with a component (the first third of the terms).  `--shapes a,c` runs a subset, `--reps`
sets the count, `--loop` the number of problems of the per-kernel loop (0 skips it).

predict_device_ms: the gf_solve_batch launches alone (HIP events around each, summed over the groups);
predict_api_ms: predict_device() and a device synchronise, wall time (coefficient pack and upload included);
predict_numpy_ms: predict(), the results copied to the host as numpy, wall time of one call (what the loop returns);
evaluate_device_ms: HIP events around evaluate_device(pack_parameters(...)) at generator_period = 1 on the same batch;
loop_ms_per_problem: GaussianProcess(kernel_b, t, yerr).predict(y[, kernel=sub]) one kernel at a time, wall time
per problem (median over `--loop` problems after one warm-up); loop_scaled_ms = that times B; speedup_over_loop =
loop_scaled_ms / predict_numpy_ms.

`--at a,b` measures prediction at new times instead, one JSON line per leg: (a) the walkers with a query
at every mid-cadence, M = N; (b) the cfg3-shaped batch on a grid that lost 10 % of its cadences, the queries filling
them.  solve_device_ms: the gf_solve_batch launches of predict_device(t=...) (HIP events, summed over the groups);
at_device_ms: the gf_predict_batch_at launch that follows them; at_over_solve their ratio; each a median of `--reps`
calls, without and with a component."""
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


def median_ms(fn, reps):
    """Medians of (wall ms, value fn returns) over `reps` calls after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts, vs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        vs.append(fn())
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.median(vs))


def device_span(fn):
    """fn() enqueued between two HIP events: their elapsed time in ms."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_of(S0, w0, Q, delta, first=None):
    return TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q))
                                     for s, w, q in list(zip(S0, w0, Q))[:first]]), delta)


def walkers(B, J, rng):
    """(kernel, S0, w0, Q (B, J), delta): proposals around the solar-like kernel's own parameters (Q untouched: every
    proposal keeps its overdamped terms)."""
    kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
    terms = kern.term.terms
    base = [np.array([[getattr(tm, k) for tm in terms]]) for k in ("S0", "w0", "Q")]
    S0, w0 = (np.repeat(b, B, axis=0) * np.exp(0.05 * rng.normal(size=(B, J))) for b in base[:2])
    return kern, S0, w0, np.repeat(base[2], B, axis=0), float(kern.delta)


def at_legs(names, reps, rng):
    for name in names:
        B, N, J = SHAPES[name]
        kern, S0, w0, Q, delta = walkers(B, J, rng)
        if name == "a":                                 # a query between every two cadences and one past the end
            t = uniform_times(N, 60.0)
            ts = t + 30e-6
        else:                                           # a grid that lost 10 % of its cadences: fill them
            grid = uniform_times(int(round(N / 0.9)), 60.0)
            keep = np.zeros(len(grid), dtype=bool)
            keep[rng.choice(len(grid), size=N, replace=False)] = True
            t, ts = grid[keep], grid[~keep]
        y = 100.0 * rng.normal(size=N)
        first = J // 3
        ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
        pack = sho_coefficient_pack(S0, w0, Q, delta)
        sub = sho_coefficient_pack(S0[:, :first], w0[:, :first], Q[:, :first], delta)
        for comp in (False, True):
            solve, at, wall = [], [], []
            for r in range(reps + 1):                   # (the first call warms up and is dropped)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mu = ev.predict_device(pack, kernel=sub if comp else None, t=ts)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                at.append(ev.last_predict_at_ms)
                solve.append(ev.last_predict_device_ms - at[-1])
                finite = bool(torch.isfinite(mu).all())
                del mu
            s_ms, a_ms = float(np.median(solve[1:])), float(np.median(at[1:]))
            print(json.dumps(dict(leg="at_" + name, B=B, N=N, M=len(ts), J=J, W=2 * J,
                                  component_W=2 * first if comp else 0, solve_device_ms=round(s_ms, 2),
                                  at_device_ms=round(a_ms, 2), at_over_solve=round(a_ms / s_ms, 3),
                                  predict_api_ms=round(float(np.median(wall[1:])), 2), finite=finite,
                                  groups=int(ev.last_predict_plan[1]), reps=reps)), flush=True)
        del ev
        torch.cuda.empty_cache()


WIDE_SHAPES = {"w1": (256, 65_000, 86), "w2": (64, 20_000, 40), "w3": (1, 100_000, 86)}


def wide_legs(names, reps, nloop, rng, grad_reps=3):
    """predict_device(wide=True) on a grid that lost 10 % of its cadences, one JSON line per shape:
    solve_device_ms, the gf_solve_batch_wide launches (HIP events, summed over the groups, median of `reps`);
    predict_numpy_ms, predict(wide=True) as numpy, wall time of one call; the loop it replaces, GaussianProcess(kernel_b,
    t, yerr).predict(y) one kernel at a time, construction included, over `nloop` problems and scaled to B; at_device_ms
    and at_share, the gf_predict_batch_at launches of predict_device(t=the lost cadences, wide=True) and their share of
    that call's device time; grad_device_ms, value_and_grad(wide=True) on the same batch (median of `grad_reps`)."""
    for name in names:
        B, N, J = WIDE_SHAPES[name]
        kern, S0, w0, Q, delta = walkers(B, J, rng)
        grid = uniform_times(int(round(N / 0.9)), 60.0)
        keep = np.zeros(len(grid), dtype=bool)
        keep[rng.choice(len(grid), size=N, replace=False)] = True
        t, ts = grid[keep], grid[~keep]
        y = 100.0 * rng.normal(size=N)
        ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
        pack = sho_coefficient_pack(S0, w0, Q, delta)

        def run_predict():
            ev.predict_device(pack, wide=True)
            return ev.last_predict_device_ms

        api, dev = median_ms(run_predict, reps)
        ws, groups, group_size = ev.last_predict_plan
        rec = dict(shape=name, B=B, N=N, J=J, W=2 * J, solve_device_ms=round(dev, 2), predict_api_ms=round(api, 2),
                   us_per_row=round(1e3 * dev / (groups * N), 3), workspace_bytes=int(ws), groups=int(groups),
                   group_size=int(group_size), reps=reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mu = ev.predict(pack, wide=True)
        rec["predict_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["finite"] = bool(np.all(np.isfinite(mu)))
        if nloop > 0:
            walls, worst = [], 0.0
            for b in range(nloop + 1):                          # (the first problem warms up and is dropped)
                i = b % B
                kb = kernel_of(S0[i], w0[i], Q[i], delta)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gp = gadfly_amd.GaussianProcess(kb, t=t, yerr=30.0, device="cuda:0")
                m1 = gp.predict(y)
                walls.append(time.perf_counter() - t0)
                worst = max(worst, float(np.max(np.abs(m1 - mu[i])) / np.max(np.abs(m1))))
                del gp
            per = float(np.median(walls[1:])) * 1e3
            rec.update(loop_problems=nloop, loop_ms_per_problem=round(per, 2), loop_scaled_ms=round(per * B, 1),
                       speedup_over_loop=round(per * B / rec["predict_numpy_ms"], 2),
                       speedup_device_over_loop=round(per * B / dev, 2), worst_against_loop=float(f"{worst:.2e}"))
        del mu
        solve, at = [], []
        for r in range(reps + 1):                               # (the first call warms up and is dropped)
            out = ev.predict_device(pack, t=ts, wide=True)
            at.append(ev.last_predict_at_ms)
            solve.append(ev.last_predict_device_ms - at[-1])
            del out
        s_ms, a_ms = float(np.median(solve[1:])), float(np.median(at[1:]))
        rec.update(M=len(ts), at_solve_device_ms=round(s_ms, 2), at_device_ms=round(a_ms, 2),
                   at_share=round(a_ms / (a_ms + s_ms), 4))
        if grad_reps > 0:
            def run_grad():
                ev.value_and_grad(S0, w0, Q, delta, wide=True)
                return ev.last_grad_device_ms

            _, g_ms = median_ms(run_grad, grad_reps)
            rec.update(grad_device_ms=round(g_ms, 2), grad_over_solve=round(g_ms / dev, 2))
        print(json.dumps(rec), flush=True)
        del ev
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=16)
    ap.add_argument("--at", default="", help="legs of the prediction at new times (a, b) to measure instead")
    ap.add_argument("--wide", default="", help="shapes of the wide route (w1, w2, w3) to measure instead")
    ap.add_argument("--grad-reps", type=int, default=3, help="value_and_grad(wide=True) calls of a wide shape (0: none)")
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(2024))
    if args.wide:
        return wide_legs(args.wide.split(","), args.reps, args.loop, rng, args.grad_reps)
    if args.at:
        return at_legs(args.at.split(","), args.reps, rng)
    for name in args.shapes.split(","):
        B, N, J = SHAPES[name]
        kern, S0, w0, Q, delta = walkers(B, J, rng)
        t = uniform_times(N, 60.0)
        y = 100.0 * rng.normal(size=N)
        first = J // 3
        ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
        ev.auto_generator_period = False
        ev.engine.generator_period = 1
        run_ev = lambda: ev.evaluate_device(ev.pack_parameters(S0, w0, Q, delta))       # noqa: E731
        _, ev_dev = median_ms(lambda: device_span(run_ev), args.reps)
        ev.resolve()
        pack = sho_coefficient_pack(S0, w0, Q, delta)
        sub = sho_coefficient_pack(S0[:, :first], w0[:, :first], Q[:, :first], delta)
        nloop = min(args.loop, max(B, 1)) if B > 1 else args.loop
        for comp in (False, True):
            def run_predict():
                ev.predict_device(pack, kernel=sub if comp else None)
                return ev.last_predict_device_ms

            api, dev = median_ms(run_predict, args.reps)
            ws, groups, group_size = ev.last_predict_plan
            rec = dict(shape=name, B=B, N=N, J=J, W=2 * J, component_W=2 * first if comp else 0,
                       predict_device_ms=round(dev, 2), predict_api_ms=round(api, 2),
                       evaluate_device_ms=round(ev_dev, 3), ratio_to_evaluate=round(dev / ev_dev, 2),
                       workspace_bytes=int(ws), groups=int(groups), group_size=int(group_size), reps=args.reps)
            # the whole call as the loop's caller sees it: results on the host as numpy (one call)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.predict(pack, kernel=sub if comp else None)
            rec["predict_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            if nloop > 0:
                walls = []
                for b in range(nloop + 1):                      # (the first problem warms up and is dropped)
                    i = b % B
                    kb = kernel_of(S0[i], w0[i], Q[i], delta)
                    sb = kernel_of(S0[i], w0[i], Q[i], delta, first) if comp else None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    gp = gadfly_amd.GaussianProcess(kb, t=t, yerr=30.0, device="cuda:0")
                    gp.predict(y, kernel=sb)
                    walls.append(time.perf_counter() - t0)
                    del gp
                per = float(np.median(walls[1:])) * 1e3
                rec.update(loop_problems=nloop, loop_ms_per_problem=round(per, 2), loop_scaled_ms=round(per * B, 1),
                           speedup_over_loop=round(per * B / rec["predict_numpy_ms"], 2))
            print(json.dumps(rec), flush=True)
        del ev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
