#!/usr/bin/env python
"""prepare_quarters_batch against the loop it replaces (stitch_quarters per star, polynomial fit and medians in numpy
on the host), and the device time of each stage.  Legs:
  a   64 stars x 17 long-cadence quarters of about 4 400 points
  b   one short-cadence star, 17 quarters of about 1.3e5 points
The raw quarters carry NaNs and outliers; the host loop gets the same quarters already cleaned (the rows the device
clip keeps), since stitch_quarters leaves cleaning to the caller.  Times: medians of `reps` runs after a warm-up, wall
clock around work that ends in a device synchronise, and HIP events around the same work.  One JSON line per leg.
Usage: python tools/detrend_latency.py [a|b|all] [reps]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import gadfly_amd  # noqa: E402
from gadfly_amd import _lib, detrend  # noqa: E402


def make_star(rng, quarters, n, cad, t0=131.5):
    out, start = [], t0
    for _ in range(quarters):
        keep = rng.random(n) > 0.1
        keep[[0, -1]] = True
        t = (start + np.arange(n) * cad)[keep]
        x = (t - t.mean()) / (t.max() - t.min())
        f = 2.3e5 * (1 + 0.02 * (x + 0.7 * x ** 2 - 1.3 * x ** 3)) * (1 + 3e-4 * rng.standard_normal(t.size))
        k = t.size // 60
        f[rng.choice(t.size, k, replace=False)] *= 1 + rng.choice([-1, 1], k) * rng.uniform(0.01, 0.05, k)
        f[rng.choice(t.size, t.size // 100, replace=False)] = np.nan
        out.append((t, f))
        start += (n + 150) * cad
    return out


def measure(fn, reps):
    """(median wall ms, median HIP-event ms) of fn(), which enqueues on the current stream"""
    fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - w0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return round(statistics.median(wall), 3), round(statistics.median(dev), 3)


def stages(stars, order, reps):
    """The stages of prepare_quarters_batch one by one on resident data: {stage: [wall ms, event ms]}, and the rows
    the clip keeps (per quarter)."""
    lib, p = _lib.load(), _lib.ptr
    ts = [t for q in stars for t, _ in q]
    fs = [f for q in stars for _, f in q]
    S, B = len(ts), len(stars)
    off_h = detrend._offsets([len(t) for t in ts])
    d = detrend._Device(torch.device("cuda", torch.cuda.current_device()))
    st = d.st
    t0, f0, off0 = (torch.as_tensor(a, device=d.dev) for a in (np.concatenate(ts), np.concatenate(fs), off_h))
    keep, meta, rounds = d.empty(off_h[-1], torch.uint8), d.empty(2 * S + 1, torch.int64), d.empty(S, torch.int32)
    t1, f1, off1 = d.empty(off_h[-1]), d.empty(off_h[-1]), meta[S:]
    out = {}
    out["clip"] = measure(lambda: lib.gf_sigma_clip(S, p(off0), p(t0), p(f0), 5.0, 5.0, 5, p(keep), p(meta), p(rounds),
                                                    st), reps)
    out["compact"] = measure(lambda: lib.gf_seg_compact(S, p(off0), p(keep), p(t0), p(f0), p(off1), p(t1), p(f1), st),
                             reps)
    out["cadence"] = measure(lambda: d.cadence(S, off1, t1), reps)
    off1_h, dt1 = off1.cpu().numpy(), d.cadence(S, off1, t1)
    t1, f1 = t1[:int(off1_h[-1])], f1[:int(off1_h[-1])]
    out["fill_quarters"] = measure(lambda: d.fill(off1_h, off1, t1, f1, dt1), reps)
    off2_h, off2, t2, f2 = d.fill(off1_h, off1, t1, f1, dt1)
    normed, info = torch.empty_like(f2), d.empty(S, torch.int32)
    out["poly_normalise"] = measure(lambda: lib.gf_poly_normalise(S, p(off2), p(t2), p(f2), order, p(normed), p(info),
                                                                  st), reps)
    ppm = torch.empty_like(normed)

    def to_ppm():
        med = d.median(S, off2, normed)
        lib.gf_seg_ppm(S, p(off2), p(normed), p(med), p(ppm), st)
    out["median_ppm"] = measure(to_ppm, reps)
    off3_h = off2_h[detrend._offsets([len(q) for q in stars])]
    off3 = torch.as_tensor(off3_h, device=d.dev)

    def stitch():
        return d.fill(off3_h, off3, t2, ppm, d.cadence(B, off3, t2))
    out["fill_stitched"] = measure(stitch, reps)
    keep_h = keep.cpu().numpy().astype(bool)
    return {k: list(v) for k, v in out.items()}, [keep_h[off_h[s]:off_h[s + 1]] for s in range(S)], \
        {"rounds_max": int(rounds.max()), "segments": S, "points": int(off_h[-1]), "filled_points": int(off2_h[-1])}


def leg(name, n_stars, n, cad, reps, order=3, quarters=17):
    rng = np.random.default_rng(17)
    stars = [make_star(rng, quarters, n, cad) for _ in range(n_stars)]
    api = measure(lambda: gadfly_amd.prepare_quarters_batch(stars, detrend_poly_order=order), reps)
    got = gadfly_amd.prepare_quarters_batch(stars, detrend_poly_order=order)
    per_stage, masks, shape = stages(stars, order, reps)
    clean, s = [], 0
    for star in stars:
        clean.append([(t[masks[s + i]], f[masks[s + i]]) for i, (t, f) in enumerate(star)])
        s += len(star)
    host = measure(lambda: [gadfly_amd.stitch_quarters(q, order) for q in clean], reps)
    want = [gadfly_amd.stitch_quarters(q, order) for q in clean]
    same_t = all(np.array_equal(g[0], w[0]) and g[2] == w[2] for g, w in zip(got, want))
    worst = max(float(np.abs(g[1] - w[1]).max()) for g, w in zip(got, want))
    print(json.dumps({"leg": name, "stars": n_stars, "quarters": quarters, "order": order, **shape,
                      "api_wall_ms": api[0], "api_event_ms": api[1], "host_loop_wall_ms": host[0],
                      "speedup_wall": round(host[0] / api[0], 2), "stages_wall_event_ms": per_stage,
                      "time_axis_equal": same_t, "flux_max_diff_ppm": worst, "reps": reps}), flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    _lib.require_device()
    if which in ("a", "all"):
        leg("a_64_stars_long_cadence", 64, 4400, 0.0204, reps)
    if which in ("b", "all"):
        leg("b_1_star_short_cadence", 1, 130000, 1.0 / 1440.0, reps)
