#!/usr/bin/env python
"""Latency of BatchedLogLikelihood.value_and_grad against evaluate() on the same batch: one JSON line
per shape, medians of 5 calls -- (a) walkers B = 2048, N = 1e5, J = 30; (b) cfg3-shaped B = 256, N = 65 000, J = 20;
(c) one star B = 1, N = 1e5, J = 30; (d) one star B = 1, N = 1e6, J = 30 (not in the default set: its one-wave leg
takes about ten seconds a call).  `--shapes a,c` runs a subset, `--reps` sets the count.  `--time-parallel` adds, for
the shapes b, c and d, the legs of the time-parallel route (value_and_grad(..., time_parallel=True)) in
the same session: a line with route = "time_parallel" at the default chunk length and, for (c), one per chunk length
of `--grid` (speedup = the one-wave route's grad_device_ms of this session over the leg's).

grad_device_ms: the gf_loglike_grad launches alone (HIP events around each, summed over the groups);
grad_api_ms: the whole call as a caller sees it (coefficient pack, launches, copies, the host chain rule);
evaluate_device_ms: HIP events around evaluate_device(pack_parameters(...)) (pack upload and every kernel);
evaluate_api_ms: the same with the copy of the result to the host, wall time.

Wide kernels (`--shapes w1,w2,w3`): (w1) B = 256, N = 65 000, the 86-term solar kernel; (w2) B = 1,
N = 1e5, the same kernel; (w3) B = 64, N = 20 000, J = 40.  value_and_grad(..., wide=True) against the central
difference it replaces, 6 J calls of evaluate_device(pack_parameters(...)) on the same evaluator between one pair of
HIP events: both series whole, their medians and spreads (max - min), the ratio, and margin_over_spread =
(fd_device_ms - grad_device_ms) / max(spread).  `--loop-reps` sets the count of the 6 J loops (default: `--reps`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd.synth import solar_like_hyperparameters, uniform_times  # noqa: E402

SHAPES = {"a": (2048, 100_000, 30), "b": (256, 65_000, 20), "c": (1, 100_000, 30), "d": (1, 1_000_000, 30),
          "w1": (256, 65_000, 86), "w2": (1, 100_000, 86), "w3": (64, 20_000, 40)}


def wide_shape(name, ev, S0, w0, Q, delta, reps, loop_reps):
    """One wide shape: the gradient call against 6 J evaluations, one JSON line."""
    B, N, J = SHAPES[name]
    run_ev = lambda: ev.evaluate_device(ev.pack_parameters(S0, w0, Q, delta))       # noqa: E731
    grads, apis = [], []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        ev.value_and_grad(S0, w0, Q, delta, wide=True)
        torch.cuda.synchronize()
        if i:                                          # (the first call warms up)
            grads.append(ev.last_grad_device_ms)
            apis.append((time.perf_counter() - t0) * 1e3)
        print(f"# {name}: gradient call {i}: {ev.last_grad_device_ms:.1f} ms", file=sys.stderr, flush=True)
    ws, groups, group_size = ev.last_grad_plan
    device_span(run_ev)
    one = [device_span(run_ev) for _ in range(3)]
    loops = []
    for i in range(loop_reps):
        loops.append(device_span(lambda: [run_ev() for _ in range(6 * J)]))
        print(f"# {name}: loop of {6 * J} evaluations {i}: {loops[-1]:.1f} ms", file=sys.stderr, flush=True)
    g, f = float(np.median(grads)), float(np.median(loops))
    spread = max(max(grads) - min(grads), max(loops) - min(loops))
    print(json.dumps(dict(shape=name, route="wide", B=B, N=N, J=J, W=2 * J, seg=int(ev.last_grad_seg),
                          grad_device_ms=round(g, 2), grad_api_ms=round(float(np.median(apis)), 2),
                          fd_evaluations=6 * J, fd_device_ms=round(f, 2), ratio=round(f / g, 2),
                          grad_series_ms=[round(x, 2) for x in grads], fd_series_ms=[round(x, 2) for x in loops],
                          spread_ms=round(spread, 2), margin_over_spread=round((f - g) / max(spread, 1e-9), 1),
                          evaluate_device_ms=round(float(np.median(one)), 3), workspace_bytes=int(ws),
                          groups=int(groups), group_size=int(group_size), reps=reps, loop_reps=loop_reps)),
          flush=True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=None)
    ap.add_argument("--time-parallel", action="store_true")
    ap.add_argument("--grid", default="64,128,256,512,1024,2048")
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(2024))
    for name in args.shapes.split(","):
        B, N, J = SHAPES[name]
        kern = gadfly_amd.StellarOscillatorKernel(solar_like_hyperparameters(J), texp=60.0)
        terms = kern.term.terms
        base = [np.array([[getattr(tm, k) for tm in terms]]) for k in ("S0", "w0", "Q")]
        # proposals around the kernel's own parameters (Q untouched: every proposal keeps its overdamped terms)
        S0, w0 = (np.repeat(b, B, axis=0) * np.exp(0.05 * rng.normal(size=(B, J))) for b in base[:2])
        Q = np.repeat(base[2], B, axis=0)
        t = uniform_times(N, 60.0)
        y = 100.0 * rng.normal(size=N)
        ev = gadfly_amd.BatchedLogLikelihood([kern] * B, t, y, yerr=30.0)
        delta = float(kern.delta)
        if name.startswith("w"):
            wide_shape(name, ev, S0, w0, Q, delta, args.reps, args.loop_reps or args.reps)
            continue
        run_ev = lambda: ev.evaluate_device(ev.pack_parameters(S0, w0, Q, delta))       # noqa: E731
        ev_api, _ = median_ms(lambda: run_ev().cpu(), args.reps)
        _, ev_dev = median_ms(lambda: device_span(run_ev), args.reps)

        def run_grad():
            ev.value_and_grad(S0, w0, Q, delta)
            return ev.last_grad_device_ms

        gr_api, gr_dev = median_ms(run_grad, args.reps)
        ws, groups, group_size = ev.last_grad_plan
        print(json.dumps(dict(shape=name, B=B, N=N, J=J, W=2 * J, grad_device_ms=round(gr_dev, 2),
                              grad_api_ms=round(gr_api, 2), evaluate_device_ms=round(ev_dev, 3),
                              evaluate_api_ms=round(ev_api, 3), device_ratio=round(gr_dev / ev_dev, 2),
                              api_ratio=round(gr_api / ev_api, 2), workspace_bytes=int(ws), groups=int(groups),
                              group_size=int(group_size), reps=args.reps)), flush=True)
        if not args.time_parallel or name == "a":
            continue
        ll1, g1 = ev.value_and_grad(S0, w0, Q, delta)
        for L in [None] + ([int(x) for x in args.grid.split(",") if x] if name == "c" else []):

            def run_tp():
                ev.value_and_grad(S0, w0, Q, delta, time_parallel=True, chunk_len=L)
                return ev.last_grad_device_ms

            tp_api, tp_dev = median_ms(run_tp, args.reps)
            ll, g = ev.value_and_grad(S0, w0, Q, delta, time_parallel=True, chunk_len=L)
            ws, groups, group_size = ev.last_grad_plan
            scaled = max(float(np.max(np.abs(th * (g[k] - g1[k]))) / max(1.0, float(np.max(np.abs(th * g1[k])))))
                         for k, th in (("S0", S0), ("w0", w0), ("Q", Q)))
            print(json.dumps(dict(shape=name, route="time_parallel", B=B, N=N, J=J, W=2 * J,
                                  chunk_len=int(ev.last_grad_chunk_len), default_chunk_len=L is None,
                                  chunks=-(-N // int(ev.last_grad_chunk_len)), grad_device_ms=round(tp_dev, 3),
                                  grad_api_ms=round(tp_api, 2), one_wave_device_ms=round(gr_dev, 2),
                                  speedup=round(gr_dev / tp_dev, 1), reruns=int(ev.last_grad_reruns),
                                  ll_rel_vs_one_wave=float(np.max(np.abs(ll - ll1) / np.abs(ll1))),
                                  grad_scaled_vs_one_wave=scaled, workspace_bytes=int(ws), groups=int(groups),
                                  group_size=int(group_size), reps=args.reps)), flush=True)


if __name__ == "__main__":
    main()
