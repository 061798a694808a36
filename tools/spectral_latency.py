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
can write today), forward only / forward and autograd backward per chunk, `--torch-reps` calls.

`--legs fisher` times SpectralLikelihood.fisher_device the same way (fisher_ms: HIP events around the
gf_spectral_fisher launches) on the shapes a, b and c (B = 256, M = 200: a binned spectrum, J = 30), against
torch_fisher_ms -- the Jacobian built `--torch-chunk` frequencies at a time in plain torch and `baddbmm` for
A diag(v) A^T -- and against the matrix pipe's issue bound: T (T + 1) / 2 MFMAs per four frequencies and problem,
T = 3 ceil(J / 16) + 1 parameter tiles, 83 cycles each per SIMD (tools/microbench/mfma_f64_rate.hip) on 1024 SIMDs at
2.4 GHz; kernel_mfma_bound_ms is the same for the MFMAs the kernel really issues (9 per pair of term tiles, 6 on the
diagonal).  `--legs fit` times a `--fit-iterations`-iteration SpectralLikelihood.fit of the shapes a and c end to end
(wall clock around the call, the host algebra included)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd.synth import solar_like_hyperparameters  # noqa: E402

SHAPES = {"a": (2048, 500_000, 30), "b": (256, 500_000, 86), "c": (256, 200, 30)}
MFMA_CYCLES, SIMDS, CLOCK_HZ = 83.0, 1024, 2.4e9
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


def torch_fisher(objective, S0, w0, Q, delta, floor, omega, power, weight, chunk):
    """sum_k v_k grad S grad S^T per problem in plain torch: the (B, P, chunk) Jacobian of `chunk` frequencies at a
    time, then baddbmm."""
    B, J = S0.shape
    F = torch.zeros((B, 3 * J + 1, 3 * J + 1), dtype=torch.float64, device=S0.device)
    a, b, q = S0[:, :, None], w0[:, :, None], Q[:, :, None]
    a1 = np.sqrt(2 / np.pi) * b ** 4
    for s in range(0, omega.shape[0], chunk):
        w = omega[None, None, s:s + chunk]
        x = (w - b) * (w + b)
        r = 1.0 / (x * x + w * w * b * b / (q * q))
        arg = 0.5 * delta[:, None] * omega[None, s:s + chunk]
        sinc = torch.where(arg == 0, torch.ones_like(arg), torch.sin(arg) / torch.where(arg == 0, 1.0, arg))
        dS0 = (sinc * sinc)[:, None, :] * a1 * r
        term = a * dS0
        S = term.sum(1) + floor[:, None]
        dQ = term * (2 * w * w * b * b / q ** 3) * r
        dw = term * (4 / b + (4 * b * x - 2 * w * w * b / (q * q)) * r)
        A = torch.cat([dS0, dw, dQ, torch.ones_like(S)[:, None, :]], dim=1)
        P, n = power[None, s:s + chunk], weight[None, s:s + chunk]
        use = torch.isfinite(P) & torch.isfinite(n) & (n > 0)
        v = torch.where(use, n / (S * S) if objective == "whittle" else 1.0 / (n * n), 0.0)
        F = torch.baddbmm(F, A * v[:, None, :], A.transpose(1, 2))
    return F


def mfma_bound_ms(B, M, J, own):
    """The matrix pipe's issue time of the rank updates: every tile pair of the triangle, or the kernel's own count."""
    tj = (J + 15) // 16
    t = 3 * tj + 1
    per_step = (6 * tj + 9 * tj * (tj - 1) // 2) if own else t * (t + 1) // 2
    return per_step * np.ceil(M / 4) * B * MFMA_CYCLES / (SIMDS * CLOCK_HZ) * 1e3


def fisher_legs(args, name, objective, sl, call, B, M, J, legs):
    """The Fisher and fit lines of one (shape, objective)."""
    import time
    lines = []
    if "fisher" in legs:
        F = sl.fisher_device(*call)                                     # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            F = sl.fisher_device(*call)
            ms.append(sl.last_device_ms)
        fisher_ms = float(np.median(ms))
        ws, groups, group = sl.last_plan
        dev = sl.power_device.device
        t = [torch.as_tensor(v, device=dev) for v in call[:3]]
        td = torch.full((B,), call[3], dtype=torch.float64, device=dev)
        tf = torch.full((B,), call[4], dtype=torch.float64, device=dev)
        tw = torch.ones(M, dtype=torch.float64, device=dev) if sl._weights is None else \
            torch.as_tensor(sl._weights[0], device=dev)
        tom, tp = torch.as_tensor(sl.omega, device=dev), sl.power_device[0]
        tms = []
        with torch.no_grad():
            for _ in range(args.torch_reps + 1):
                dt_ms, Ft = span_ms(lambda: torch_fisher(objective, *t, td, tf, tom, tp, tw, args.torch_chunk))
                tms.append(dt_ms)
        torch_ms = float(np.median(tms[1:]))
        scale = torch.sqrt(torch.diagonal(Ft, dim1=1, dim2=2))
        differ = float(((F - Ft).abs() / (scale[:, :, None] * scale[:, None, :])).max())
        bound, own = mfma_bound_ms(B, M, J, False), mfma_bound_ms(B, M, J, True)
        lines.append(dict(leg="fisher", shape=name, objective=objective, B=B, M=M, J=J, fisher_ms=round(fisher_ms, 3),
                          torch_fisher_ms=round(torch_ms, 1), torch_over_fisher=round(torch_ms / fisher_ms, 1),
                          mfma_issue_bound_ms=round(bound, 3), fisher_over_bound=round(fisher_ms / bound, 2),
                          kernel_mfma_bound_ms=round(own, 3), fisher_over_kernel_bound=round(fisher_ms / own, 2),
                          largest_difference_from_torch_over_sqrt_diagonals=differ,
                          slab=gadfly_amd._lib.load().gf_spectral_fisher_slab(), workspace_bytes=int(ws),
                          groups=int(groups), group_size=int(group), reps=args.reps, torch_reps=args.torch_reps,
                          torch_chunk=args.torch_chunk))
        del F, Ft
    if "fit" in legs and name in ("a", "c"):
        start = [v * 1.05 for v in call[:3]] + [call[3], call[4] * 1.05]
        sl.fit(*start, max_iter=1)                                      # warm-up
        sec = []
        for _ in range(max(1, args.reps if name == "c" else 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = sl.fit(*start, max_iter=args.fit_iterations)
            torch.cuda.synchronize()
            sec.append(time.perf_counter() - t0)
        lines.append(dict(leg="fit", shape=name, objective=objective, B=B, M=M, J=J, iterations=args.fit_iterations,
                          fit_s=round(float(np.median(sec)), 3), converged=int(fit.converged.sum()),
                          largest_iterations=int(fit.iterations.max()), cov_ok=int(fit.cov_ok.sum()), reps=len(sec)))
    return lines


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
    ap.add_argument("--legs", default="value", help="value, fisher, fit (comma separated)")
    ap.add_argument("--fit-iterations", type=int, default=20)
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
            legs = args.legs.split(",")
            for line in fisher_legs(args, name, objective, sl, call, B, M, J, legs):
                text = json.dumps(line)
                print(text, flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(text + "\n")
            if "value" not in legs:
                continue
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
