#!/usr/bin/env python
"""Latency of BatchedSampler.sample_device against evaluate_device() of a BatchedLogLikelihood on the same kernels,
axis and generator period, and against the loop over single-kernel draws it replaces: one JSON line
per leg, HIP events, medians of 5 calls --
  (a) B = 2048, N = 1e5, J = 30, 60 s cadence;   (b) B = 256 stars from for_star (W = 172), N = 65 000, 58.85 s;
  (c) (b) on stamps 1765 s apart (same kernels); (d) B = 512, N = 2e5, J = 40 (cfg4's shape).
`--legs a,c` runs a subset, `--reps` sets the count, `--loop` the problems of the single-kernel loop (16).

sample_ms:          sample_device(normals=<device tensor>, center=False, include_mean=False) at exact rows (period 1,
                    the default): the copy of eps into the padded buffer, the sweeps, min d, the NaN mask;
sample_randn_ms:    sample_device(seed=...) -- the same plus torch.randn for the block and the centring;
evaluate_ms:        evaluate_device() of the evaluator, streamed sweep (the same arithmetic), same period;
evaluate_auto_ms:   the evaluator's own route (time-parallel for small batches of long series), same period;
loop_ms:            GaussianProcess(kernel_b, t, yerr).sample_device(rng="device") over `--loop` problems, wall time
                    with a synchronisation per draw as a caller sees it, scaled to B;
rule_*:             legs a, b: the same with the evaluator's period rule instead (period from the measured max a / min d).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters  # noqa: E402

LEGS = {"a": (2048, 100_000, 30, 60.0), "b": (256, 65_000, None, 58.85), "c": (256, 65_000, None, 1765.0),
        "d": (512, 200_000, 40, 60.0)}


def device_ms(fn, reps):
    """Median HIP-event time of fn() over `reps` calls after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def kernels_of(B, J, cadence):
    if J is not None:
        base = solar_like_hyperparameters(J)
        return [gadfly_amd.StellarOscillatorKernel(jitter_hyperparameters(base, 1000 + i), texp=cadence)
                for i in range(B)]
    stars = []
    for i in range(16):                     # sixteen different stars, repeated over the batch
        f = i / 15.0
        hp = gadfly_amd.Hyperparameters.for_star(0.9 + 0.4 * f, 0.95 + 0.85 * f, 5500.0 + 700.0 * f, 0.75 + 3.5 * f,
                                                 bandpass="SOHO VIRGO", quiet=True)
        stars.append(gadfly_amd.StellarOscillatorKernel(hp, texp=cadence))
    return [stars[i % 16] for i in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=16)
    args = ap.parse_args()
    for name in args.legs.split(","):
        B, N, J, cadence = LEGS[name]
        # (the kernels keep their short-cadence exposure in leg c: a reset on every row is what it is about)
        kernels = kernels_of(B, J, 58.85 if J is None else cadence)
        W = len(kernels[0])
        t = np.arange(N) * cadence * 1e-6
        s = gadfly_amd.BatchedSampler(kernels, t, yerr=30.0)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        eps = torch.randn((B, N), dtype=torch.float64, device="cuda", generator=gen)
        draw = lambda: s.sample_device(normals=eps, center=False, include_mean=False)       # noqa: E731
        rec = dict(leg=name, B=B, N=N, W=W, cadence_s=cadence, reps=args.reps)
        rec["sample_ms"] = round(device_ms(draw, args.reps), 3)
        rec["route"] = s.engine.kernel_used
        rec["sample_randn_ms"] = round(device_ms(lambda: s.sample_device(seed=3), args.reps), 3)
        y = draw()
        rec["failed_problems"] = int(np.count_nonzero(s.last_info))
        ev = gadfly_amd.BatchedLogLikelihood(kernels, t, y.cpu().numpy(), yerr=30.0)
        del y

        def evaluate(period, streamed):
            ev.engine.generator_period = period
            ev.engine.force_streaming = streamed
            return device_ms(ev.evaluate_device, args.reps)

        rec["evaluate_ms"] = round(evaluate(1, True), 3)
        rec["evaluate_auto_ms"] = round(evaluate(1, False), 3)
        ev.resolve()
        rec["ratio"] = round(rec["sample_ms"] / rec["evaluate_ms"], 3)
        if name in ("a", "b"):
            s.auto_generator_period = True
            draw()
            draw()                          # (calibrated on the first call's conditioning)
            rec["rule_sample_ms"] = round(device_ms(draw, args.reps), 3)
            rec["rule_period"] = int(s.engine.generator_period)
            rec["rule_evaluate_ms"] = round(evaluate(rec["rule_period"], True), 3)
            ev.resolve()
            rec["rule_ratio"] = round(rec["rule_sample_ms"] / rec["rule_evaluate_ms"], 3)
            rec["rule_reruns"] = int(s.guard_reruns)
            s.auto_generator_period = False
        del ev
        torch.cuda.empty_cache()
        # the parent's way: one GaussianProcess per kernel, a stored factor built and thrown away per draw
        n = min(args.loop, B)
        gadfly_amd.GaussianProcess(kernels[0], t=t, yerr=30.0).sample_device(rng="device")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(n):
            gadfly_amd.GaussianProcess(kernels[b], t=t, yerr=30.0).sample_device(rng="device")
            torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / n * 1e3
        rec["loop_ms_per_problem"] = round(per, 3)
        rec["loop_ms"] = round(per * B, 1)
        rec["loop_over_sample"] = round(per * B / rec["sample_randn_ms"], 1)
        print(json.dumps(rec), flush=True)
        del s, eps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
