#!/usr/bin/env python
"""Lomb-Scargle power spectra (gf_ls_power) at the sizes of real photometry: (a) three Kepler short-cadence
quarters (~3.7e5 points at 58.85 s, with gaps), (b) a full short-cadence light curve (~1.5e6 points), (c) 256
long-cadence series of 7.1e4 points (four years at 29.4 min).  Per case: the API call end to end
(PowerSpectrum.from_lomb_scargle, host arrays in, host power out), the native call alone on device events,
(point, frequency) pairs per second, and the share of the per-pair peak: VALU_PER_PAIR vector instructions
per pair (the sum pass' inner loop from a host compile) at 78.6 TF FP64 vector, i.e.
39.3e12 lane-instructions per second.  Usage: python tools/ls_latency.py [case ...]  (default: a b c)"""
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
}


def run(key):
    c = CASES[key]
    t = gapped_axis(c["n"], c["cadence"], 1, c["gaps"])
    rng = np.random.default_rng(2)
    flux = 100 * rng.normal(size=(c["R"], c["n"])) if c["R"] > 1 else 100 * rng.normal(size=c["n"])
    torch.cuda.synchronize()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        ps = gadfly_amd.PowerSpectrum.from_lomb_scargle(t, flux)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    # the native call alone (the same launch from_lomb_scargle makes), on device events
    lib, p = _lib.load(), _lib.ptr
    n, R = c["n"], c["R"]
    series, _ = psd._ls_series(t, flux, None)
    freq, df = psd.ls_grid(n, series[0][2])
    M = n // 2 + 1 - 1
    pt = np.arange(R + 1, dtype=np.int64) * n
    oo = np.arange(R + 1, dtype=np.int64) * M
    groups = psd._ls_groups(lib, np.full(R, n, np.int64), np.full(R, M, np.int64))
    g = max(b - a for a, b in groups)                 # series per launch (every series has n points here)
    s_max = lib.gf_ls_segments(n)
    dev = torch.device("cuda")
    meta_i = torch.as_tensor(np.concatenate([pt[:g + 1], oo[:g + 1]]), device=dev)
    meta_d = torch.as_tensor(np.array([df] * g + [ps.norm] * g), device=dev)
    t_d = torch.as_tensor(np.tile(t, g), device=dev)
    y_all = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(flux)).reshape(-1), device=dev)
    work = torch.empty(int(lib.gf_ls_work(g * n, g * M, s_max)), dtype=torch.float64, device=dev)
    out = torch.empty(R * M, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        for a, b in groups:
            k = b - a
            _lib.check(lib.gf_ls_power(k, n, k * n, k * M, s_max, 1, p(meta_i), p(meta_i[g + 1:]), p(meta_d),
                                       p(meta_d[g:]), p(t_d), p(y_all[a * n:]),
                                       p(work), p(out[a * M:]), st), "gf_ls_power")
    call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 3
    ev[0].record()
    for _ in range(reps):
        call()
    ev[1].record()
    torch.cuda.synchronize()
    ms_dev = ev[0].elapsed_time(ev[1]) / reps
    assert np.array_equal(out.view(R, M).cpu().numpy(), np.asarray(ps.power).reshape(R, M)), \
        "native call differs from the API's"
    pairs = float(R) * n * M
    rate = pairs / (ms_dev * 1e-3)
    peak = PEAK_LANE_INSTR / VALU_PER_PAIR
    return dict(case=key, label=c["label"], R=R, n=n, frequencies=M, launches=len(groups), series_per_launch=g,
                segments=s_max, pairs=pairs, api_wall_ms=[round(w * 1e3, 2) for w in wall],
                device_ms=round(ms_dev, 3), pairs_per_s=rate, valu_per_pair=round(VALU_PER_PAIR, 3),
                peak_pairs_per_s=peak, fraction_of_peak=round(rate / peak, 3))


if __name__ == "__main__":
    _lib.require_device()
    for key in (sys.argv[1:] or ["a", "b", "c"]):
        print(json.dumps(run(key)), flush=True)
