#!/usr/bin/env python
"""Lomb-Scargle power spectra (gf_ls_power) at the sizes of real photometry: (a) three Kepler short-cadence
quarters (~3.7e5 points at 58.85 s, with gaps), (b) a full short-cadence light curve (~1.5e6 points), (c) 256
long-cadence series of 7.1e4 points (four years at 29.4 min).  Per case: the API call end to end
(PowerSpectrum.from_lomb_scargle, host arrays in, host power out), the native call alone on device events,
(point, frequency) pairs per second, and the share of the per-pair peak: VALU_PER_PAIR vector instructions
per pair (the sum pass' inner loop from a host compile) at 78.6 TF FP64 vector, i.e.
39.3e12 lane-instructions per second.  --method nufft times the non-uniform FFT route (gf_lsfft_*, a torch sort and
hipFFT between them; device events around the whole device part, the upload of the time axis and offsets included)
at the same cases and at (d) 4.4e6 points; --method both runs the two routes side by side on the same inputs
(medians of 5) with the worst difference of their powers; --crossover sweeps n for the size below which the
direct sum wins.  Usage: python tools/ls_latency.py [--method direct|nufft|both] [--crossover] [case ...]
(default: --method direct a b c)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd import _lib, psd  # noqa: E402

VALU_PER_PAIR = 225 / 16            # k_ls_sum<16>: 225 VALU per point and 16 frequencies
PEAK_LANE_INSTR = 78.6e12 / 2       # FP64 vector: one FMA (2 flops) per lane-instruction


def gapped_axis(n_target, cadence_s, seed, gaps):
    """Times [1/uHz] of n_target samples at cadence_s with `gaps` data gaps of 1-3 % each and 1 % lost cadences."""
    rng = np.random.default_rng(seed)
    n = int(n_target * (1 + 0.03 * gaps + 0.02))
    keep = np.ones(n, bool)
    for a in rng.integers(0, n, gaps):
        keep[a:a + int(n * rng.uniform(0.01, 0.03))] = False
    keep[rng.integers(0, n, n // 100)] = False
    t = np.flatnonzero(keep)[:n_target] * cadence_s / 1e6
    assert len(t) == n_target
    return t + 2454833.0 * 0.0864                     # a JD-based axis, as from_light_curve passes it


CASES = {
    "a": dict(label="3 Kepler SC quarters", n=370_000, R=1, cadence=58.85, gaps=3),
    "b": dict(label="full Kepler SC light curve", n=1_500_000, R=1, cadence=58.85, gaps=17),
    "c": dict(label="256 Kepler LC series, 4 yr", n=71_000, R=256, cadence=1765.5, gaps=17),
    "d": dict(label="20 s cadence, 3 yr (nufft only)", n=4_400_000, R=1, cadence=20.0, gaps=17),
}
REPS = 5


def median_ms(call, reps=REPS):
    """Median device time of `call` over `reps` event pairs, after one warm-up call."""
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms)), [round(x, 3) for x in ms]


def case_inputs(c):
    t = gapped_axis(c["n"], c["cadence"], 1, c["gaps"])
    rng = np.random.default_rng(2)
    flux = 100 * rng.normal(size=(c["R"], c["n"])) if c["R"] > 1 else 100 * rng.normal(size=c["n"])
    return t, flux


def api_wall(t, flux, method, reps=3):
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, flux, method=method)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    return ps, [round(w * 1e3, 2) for w in wall]


def direct_call(t, flux):
    """The launches from_lomb_scargle(method="direct") makes, on buffers made once: (call, out [R, M])."""
    lib, p = _lib.load(), _lib.ptr
    flux2 = np.ascontiguousarray(np.atleast_2d(flux))
    R, n = flux2.shape
    series, _ = psd._ls_series(t, flux, None)
    _, df = psd.ls_grid(n, series[0][2])
    norm = series[0][2] / (2 * np.pi) ** 0.5
    M = n // 2
    pt = np.arange(R + 1, dtype=np.int64) * n
    oo = np.arange(R + 1, dtype=np.int64) * M
    groups = psd._ls_groups(lib, np.full(R, n, np.int64), np.full(R, M, np.int64))
    g = max(b - a for a, b in groups)
    s_max = lib.gf_ls_segments(n)
    dev = torch.device("cuda")
    meta_i = torch.as_tensor(np.concatenate([pt[:g + 1], oo[:g + 1]]), device=dev)
    meta_d = torch.as_tensor(np.array([df] * g + [norm] * g), device=dev)
    t_d = torch.as_tensor(np.tile(t, g), device=dev)
    y_all = torch.as_tensor(flux2.reshape(-1), device=dev)
    work = torch.empty(int(lib.gf_ls_work(g * n, g * M, s_max)), dtype=torch.float64, device=dev)
    out = torch.empty(R * M, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        for a, b in groups:
            k = b - a
            _lib.check(lib.gf_ls_power(k, n, k * n, k * M, s_max, 1, p(meta_i), p(meta_i[g + 1:]), p(meta_d),
                                       p(meta_d[g:]), p(t_d), p(y_all[a * n:]),
                                       p(work), p(out[a * M:]), st), "gf_ls_power")
    return call, out.view(R, M)


def nufft_call(t, flux):
    """The device part of from_lomb_scargle(method="nufft") on a flux uploaded once: (call, out [R, M], info)."""
    lib = _lib.load()
    series, _ = psd._ls_series(t, flux, None)
    R, n = len(series), len(t)
    grids = [psd.ls_grid(n, dr) for _, _, dr in series]
    norms = [dr / (2 * np.pi) ** 0.5 for _, _, dr in series]
    outs = np.full(R, n // 2, np.int64)
    out_off = np.arange(R + 1, dtype=np.int64) * (n // 2)
    pt_all = np.arange(R + 1, dtype=np.int64) * n
    dev = torch.device("cuda")
    y_all = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(flux)).reshape(-1), device=dev)
    out = torch.empty(int(out_off[-1]), dtype=torch.float64, device=dev)
    n_f = int(lib.gf_lsfft_grid(n))
    groups = psd._lsfft_groups([n_f] * R, [id(tr) for tr, _, _ in series])

    def call():
        psd._ls_nufft(lib, series, grids, norms, outs, out_off, pt_all, 1, y_all, out, dev)
    return call, out.view(R, n // 2), dict(fine_grid=n_f, groups=len(groups),
                                           series_per_group=max(b - a for a, b in groups))


def run_nufft(key, compare):
    c = CASES[key]
    t, flux = case_inputs(c)
    ps, wall = api_wall(t, flux, "nufft")
    call, out, info = nufft_call(t, flux)
    ms, all_ms = median_ms(call)
    assert np.array_equal(out.cpu().numpy(), np.asarray(ps.power).reshape(out.shape)), "device part differs from the API's"
    line = dict(case=key, label=c["label"], method="nufft", R=c["R"], n=c["n"], frequencies=out.shape[1], **info,
                api_wall_ms=wall, device_ms=round(ms, 3), device_ms_all=all_ms)
    if compare:
        dcall, dout = direct_call(t, flux)
        dms, dall = median_ms(dcall)
        a, b = out.cpu().numpy(), dout.cpu().numpy()
        err = np.abs(a - b)
        top = b.max(axis=-1, keepdims=True)
        big = b > 1e-10 * top
        r, k = np.unravel_index(np.argmax(err / top), err.shape)
        inner = (err / top)[:, :-1]                  # without the grid's last frequency (Nyquist of an even n)
        line.update(direct_device_ms=round(dms, 3), direct_device_ms_all=dall, speedup=round(dms / ms, 1),
                    worst_diff_over_max=float((err / top).max()), worst_at=[int(r), int(k)],
                    worst_diff_over_max_inner=float(inner.max()),
                    outside_direct_bar=int(np.count_nonzero(err > 1e-10 * top + 1e-8 * b)),   # rtol 1e-8, atol 1e-10 max
                    worst_relative_diff=float((err[big] / b[big]).max()),
                    worst_relative_diff_inner=float((err[:, :-1][big[:, :-1]] / b[:, :-1][big[:, :-1]]).max()))
    return line


def crossover():
    """Both routes on one series of n points (device events, medians of 5): the n below which the direct sum wins."""
    rows = []
    for n in (1000, 2000, 4000, 8000, 16000, 32000, 64000, 128000):
        t = gapped_axis(n, 58.85, 1, 3)
        flux = 100 * np.random.default_rng(2).normal(size=n)
        fast, _, _ = nufft_call(t, flux)
        direct, _ = direct_call(t, flux)
        rows.append(dict(n=n, nufft_ms=round(median_ms(fast)[0], 3), direct_ms=round(median_ms(direct)[0], 3)))
    wins = [r["n"] for r in rows if r["nufft_ms"] < r["direct_ms"]]
    return dict(case="crossover", rows=rows, nufft_wins_from_n=min(wins) if wins else None)


def run(key):
    c = CASES[key]
    t, flux = case_inputs(c)
    n, R, M = c["n"], c["R"], c["n"] // 2
    ps, wall = api_wall(t, flux, "direct")
    # the native call alone (the same launches from_lomb_scargle makes), on device events
    lib = _lib.load()
    call, out = direct_call(t, flux)
    groups = psd._ls_groups(lib, np.full(R, n, np.int64), np.full(R, M, np.int64))
    ms_dev, all_ms = median_ms(call)
    assert np.array_equal(out.cpu().numpy(), np.asarray(ps.power).reshape(R, M)), "native call differs from the API's"
    pairs = float(R) * n * M
    rate = pairs / (ms_dev * 1e-3)
    peak = PEAK_LANE_INSTR / VALU_PER_PAIR
    return dict(case=key, label=c["label"], method="direct", R=R, n=n, frequencies=M, launches=len(groups),
                series_per_launch=max(b - a for a, b in groups), segments=lib.gf_ls_segments(n), pairs=pairs,
                api_wall_ms=wall, device_ms=round(ms_dev, 3), device_ms_all=all_ms, pairs_per_s=rate,
                valu_per_pair=round(VALU_PER_PAIR, 3), peak_pairs_per_s=peak, fraction_of_peak=round(rate / peak, 3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--method", choices=("direct", "nufft", "both"), default="direct")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    _lib.require_device()
    for key in (args.cases or ([] if args.crossover else ["a", "b", "c"])):
        if args.method == "direct":
            print(json.dumps(run(key)), flush=True)
        else:
            print(json.dumps(run_nufft(key, compare=args.method == "both" and key != "d")), flush=True)
    if args.crossover:
        print(json.dumps(crossover()), flush=True)
