#!/usr/bin/env python
"""Device time of SpectralLikelihood: value only and value plus gradients, one JSON line per
(shape, objective), medians of `--reps` calls after a warm-up -- (a) walkers B = 2048, M = 5e5, J = 30;
(b) B = 256, M = 5e5, gadfly's 86-term solar kernel.  `--shapes a` runs a subset, `--out FILE` appends the lines to a
file (profiles/..._spectral_latency.jsonl).

value_ms / grad_ms: HIP events around the gf_spectral_like launches (SpectralLikelihood.last_device_ms), parameters
uploaded before, nothing copied back inside the span.
share_of_fp64_vector_peak: the kernel's own FP64 vector instructions per (frequency, term) pair -- 10 for the value
(2 add, 2 mul, 2 fma, the reciprocal's estimate and 4 fma), 15 more with gradients (the pair recomputed, 5 for the
three sums) -- times the pairs, over 39.3e12 instructions/s (78.6 TFLOP/s at two flops per FMA).
torch_value_ms / torch_grad_ms: the same objective written in plain torch on the device, chunked over M (what a user
can write today), forward only / forward and autograd backward per chunk, `--torch-reps` calls."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd.synth import solar_like_hyperparameters  # noqa: E402

SHAPES = {"a": (2048, 500_000, 30), "b": (256, 500_000, 86)}
DT = 60.0e-6
PEAK_FP64_INSTR = 78.6e12 / 2
INSTR_VALUE, INSTR_GRAD = 10, 25


def kernel_of(J):
    if J == 86:
        hp = gadfly_amd.Hyperparameters.for_star(1, 1, 5777, 1, bandpass="SOHO VIRGO", quiet=True)
    else:
        hp = solar_like_hyperparameters(J)
    return gadfly_amd.StellarOscillatorKernel(hp, texp=60.0)


def torch_objective(objective, S0, w0, Q, delta, floor, omega, power, weight, chunk, grad):
    """-sum n (ln S + P / S) or -1/2 sum ((P - S) / e)^2 per problem in plain torch, `chunk` frequencies at a time;
    with `grad` each chunk's sum is differentiated at once (the graph of one chunk alive at a time)."""
    total = torch.zeros(S0.shape[0], dtype=torch.float64, device=S0.device)
    a, b, q = S0[:, :, None], w0[:, :, None], Q[:, :, None]
    for s in range(0, omega.shape[0], chunk):
        w = omega[None, None, s:s + chunk]
        x = (w - b) * (w + b)
        terms = np.sqrt(2 / np.pi) * a * b ** 4 / (x * x + w * w * b * b / (q * q))
        arg = 0.5 * delta[:, None] * omega[None, s:s + chunk]
        sinc = torch.where(arg == 0, torch.ones_like(arg), torch.sin(arg) / torch.where(arg == 0, 1.0, arg))
        S = sinc * sinc * terms.sum(1) + floor[:, None]
        P, n = power[None, s:s + chunk], weight[None, s:s + chunk]
        use = torch.isfinite(P) & torch.isfinite(n) & (n > 0)
        add = n * (torch.log(S) + P / S) if objective == "whittle" else 0.5 * ((P - S) / n) ** 2
        part = -torch.where(use, add, 0.0).sum(1)
        if grad:
            part.sum().backward()
        total += part.detach()
    return total


def span_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--objectives", default="whittle,chi2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--torch-chunk", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(2025))
    for name in args.shapes.split(","):
        B, M, J = SHAPES[name]
        kern = kernel_of(J)
        S0, w0, Q, delta = gadfly_amd.spectral.kernel_parameters([kern])
        freq = np.fft.rfftfreq(2 * M, DT)[1:]
        floor = float(gadfly_amd.spectral.white_floor(30.0, DT))
        S = kern.get_psd(2 * np.pi * freq) + floor
        # walkers around the kernel's own parameters
        pars = [np.repeat(v, B, axis=0) * np.exp(0.05 * rng.normal(size=(B, J))) for v in (S0, w0, Q)]
        for objective in args.objectives.split(","):
            if objective == "whittle":
                ps = gadfly_amd.PowerSpectrum(freq, S * rng.exponential(size=M))
            else:
                ps = gadfly_amd.PowerSpectrum(freq, S * (1.0 + 0.1 * rng.normal(size=M)), error=0.1 * S)
            sl = gadfly_amd.SpectralLikelihood(ps, objective=objective)
            call = (*pars, float(delta[0]), floor)
            times = {}
            for key, grad in (("value", False), ("grad", True)):
                out = sl.run_device(*call, grad=grad)                   # warm-up
                torch.cuda.synchronize()
                ms = []
                for _ in range(args.reps):
                    out = sl.run_device(*call, grad=grad)
                    ms.append(sl.last_device_ms)
                times[key] = float(np.median(ms))
                times[key + "_ll0"] = float(out["ll"][0])
            dev = sl.power_device.device
            t = [torch.as_tensor(v, device=dev) for v in pars]
            td = torch.full((B,), float(delta[0]), dtype=torch.float64, device=dev)
            tf = torch.full((B,), floor, dtype=torch.float64, device=dev)
            tw = torch.ones(M, dtype=torch.float64, device=dev) if sl._weights is None else \
                torch.as_tensor(sl._weights[0], device=dev)
            tom, tp = torch.as_tensor(sl.omega, device=dev), sl.power_device[0]
            for key, grad in (("torch_value", False), ("torch_grad", True)):
                ms = []
                for _ in range(args.torch_reps + 1):
                    if grad:
                        lv = [v.clone().requires_grad_(True) for v in t + [tf]]
                        run = lambda: torch_objective(objective, *lv[:3], td, lv[3], tom, tp, tw,     # noqa: E731
                                                      args.torch_chunk, True)
                    else:
                        run = lambda: torch_objective(objective, *t, td, tf, tom, tp, tw,             # noqa: E731
                                                      args.torch_chunk, False)
                    with torch.set_grad_enabled(grad):
                        dt_ms, ll = span_ms(run)
                    ms.append(dt_ms)
                times[key] = float(np.median(ms[1:]))               # (the first call is the warm-up)
                times[key + "_ll0"] = float(ll[0])
            pairs = float(B) * M * J
            ws, groups, group = sl.last_plan
            line = dict(shape=name, objective=objective, B=B, M=M, J=J, value_ms=round(times["value"], 3),
                        grad_ms=round(times["grad"], 3), grad_over_value=round(times["grad"] / times["value"], 2),
                        value_share_of_fp64_vector_peak=round(
                            pairs * INSTR_VALUE / PEAK_FP64_INSTR / (times["value"] * 1e-3), 3),
                        grad_share_of_fp64_vector_peak=round(
                            pairs * INSTR_GRAD / PEAK_FP64_INSTR / (times["grad"] * 1e-3), 3),
                        fp64_instr_per_pair=[INSTR_VALUE, INSTR_GRAD], pairs=pairs,
                        torch_value_ms=round(times["torch_value"], 1), torch_grad_ms=round(times["torch_grad"], 1),
                        torch_value_over_value=round(times["torch_value"] / times["value"], 1),
                        torch_grad_over_grad=round(times["torch_grad"] / times["grad"], 1),
                        ll0=times["value_ll0"], ll0_grad_call=times["grad_ll0"], torch_ll0=times["torch_value_ll0"],
                        tile=gadfly_amd._lib.load().gf_spectral_tile(), workspace_bytes=int(ws), groups=int(groups),
                        group_size=int(group), reps=args.reps, torch_reps=args.torch_reps,
                        torch_chunk=args.torch_chunk)
            text = json.dumps(line)
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(text + "\n")


if __name__ == "__main__":
    main()
