"""Seeded random problems shared by the randomized GPU tests and tools/random_sweep*.py, and the ONE rule that
decides which of them lie beyond float64 at the 1e-8 bar.

The rule (`float64_limit`) looks at oracle-side quantities only -- never at a GPU result:
  * the condition max(a) / min(d) of the C recurrence above COND_MAX = 1e7, or
  * the plain-C recurrence and the 80-bit one disagreeing by more than C_VS_80 = 1e-9 (relative).
A 2000-seed sweep of test_gpu_random.py had two cases at conditions of 4e7 and 1e8 where C was 1.7e-9 from the 80-bit
value and the GPU, with exact generator rows, at 1.4e-8 / 9e-9; a 5000-seed sweep one at 2.4e7 where C happened to land
4e-10 from the 80-bit result while every GPU path, the unscaled celerite recurrence included, sat at 1.5e-8: rounding
of the inputs times the condition, not an implementation defect.
The 80-bit recurrence costs ~0.1 ms per row and walker (numpy on long doubles); it only runs for problems whose
C-side condition exceeds COND_80 = 1e4.  Below that the two recurrences agree to ~1e-12 (the C recurrence's
rounding grows with the condition: 4e-10 ... 1.7e-9 at 2e7 ... 1e8), so the comparison cannot fire there --
tests/test_random_cases_host.py checks both on well-conditioned problems.
"""
import numpy as np

COND_MAX = 1.0e7
C_VS_80 = 1.0e-9
COND_80 = 1.0e4
BKJD0 = 2454833.0 * 0.0864          # Time(0, format='bkjd') in units of 1e6 s: 2.12e5
#: StreamingBatch.QMODE_PHASE (RowGen::qmode): restated so that the generators need no device
QMODE_PHASE = 4.0e6
AXES = ("uniform", "jitter", "gaps", "bkjd", "qcross")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---------------------------------------------------------------------------------------------------------------
# the oracle side


def loglike80(coeffs, t, diags, y):
    """80-bit log-likelihoods of B problems on ONE time axis (coefficient tuples of the same width, one diagonal
    each): the recurrence of oracle.seq.factor / solve_lower on the generator rows of float64 phases, vectorised
    over the problems.  Returns (B,) floats, -inf where a pivot is not positive."""
    from oracle import seq
    ld = np.longdouble
    mats = [seq.celerite_matrices(co[:6], t, dg, dtype=ld) for co, dg in zip(coeffs, diags)]
    t = np.asarray(t, dtype=np.float64)
    for co, m in zip(coeffs, mats):
        # the phases as celerite2 (and the C oracle, and the kernels) form them: theta = fl(d t), ONE float64
        # multiply, whose cos / sin are then taken in 80 bits.  An 80-bit product would be a different matrix on a
        # time axis far from zero (half an ulp of 5e9 rad is 5e-7 rad), not a more accurate evaluation of this one
        Jr, ac, bc = len(co[0]), np.asarray(co[2], dtype=ld), np.asarray(co[3], dtype=ld)
        theta = (t[:, None] * np.asarray(co[5], dtype=np.float64)[None, :]).astype(ld)
        cs, sn = np.cos(theta), np.sin(theta)
        m[2][:, Jr::2], m[2][:, Jr + 1::2] = ac * cs + bc * sn, ac * sn - bc * cs
        m[3][:, Jr::2], m[3][:, Jr + 1::2] = cs, sn
    c = np.stack([m[0] for m in mats])
    a = np.stack([m[1] for m in mats])
    U = np.stack([m[2] for m in mats])
    V = np.stack([m[3] for m in mats])
    tl, yl = np.asarray(t, dtype=ld), np.asarray(y, dtype=ld)
    B, N, W = U.shape
    S = np.zeros((B, W, W), dtype=ld)
    F = np.zeros((B, W), dtype=ld)
    d = a[:, 0].copy()
    ok = d > 0
    Wn = V[:, 0] / d[:, None]
    z = np.full(B, yl[0])
    logd, quad = np.log(np.where(ok, d, 1)), z * z / np.where(ok, d, 1)
    for n in range(1, N):
        p = np.exp(c * (tl[n - 1] - tl[n]))
        S = p[:, :, None] * p[:, None, :] * (S + d[:, None, None] * Wn[:, :, None] * Wn[:, None, :])
        F = p * (F + Wn * z[:, None])
        tmp = np.einsum("bi,bij->bj", U[:, n], S)
        d = a[:, n] - np.einsum("bi,bi->b", tmp, U[:, n])
        ok &= d > 0
        dd = np.where(ok, d, 1)
        Wn = (V[:, n] - tmp) / dd[:, None]
        z = yl[n] - np.einsum("bi,bi->b", U[:, n], F)
        logd += np.log(dd)
        quad += z * z / dd
    ll = -0.5 * (logd + N * np.log(2 * ld(np.pi))) - 0.5 * quad
    return np.where(ok, ll.astype(np.float64), -np.inf)


def oracle_problems(coeffs, t, diag_user, y):
    """C-oracle view of B problems on one axis: dict(ref (B,), info (B,), cond (B,), d [B x (N,)], mats [B x
    (c, a, U, V)]).  cond = max(a) / min(d) per problem (inf where the factorisation fails)."""
    from oracle import cref, seq
    out = dict(ref=[], info=[], cond=[], d=[], W=[], mats=[])
    for co in coeffs:
        ref, info = cref.loglike(co[:6], t, diag_user + co[6], y)
        c, a, U, V = seq.celerite_matrices(co[:6], t, diag_user + co[6])
        d, Wm, _ = cref.factor(t, c, a, U, V)
        out["ref"].append(ref)
        out["info"].append(info)
        out["cond"].append(float(a.max() / d.min()) if info == 0 else float("inf"))
        out["d"].append(d)
        out["W"].append(Wm)
        out["mats"].append((c, a, U, V))
    for k in ("ref", "info", "cond"):
        out[k] = np.asarray(out[k])
    return out


def oracle_loglikes(coeffs, t, diag_user, y):
    """(ref (B,), info (B,)) of the C oracle for many problems on one axis, on a few threads (the C call releases the
    interpreter lock)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    from oracle import cref
    cref.lib()
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        res = list(ex.map(lambda co: cref.loglike(co[:6], t, diag_user + co[6], y), coeffs))
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def float64_limit(coeffs, t, diag_user, y, orc=None):
    """The skip rule: None, or the reason why one of these problems (those whose factorisation the oracle
    completes) is beyond float64 at the 1e-8 bar.  Oracle-side quantities only (module docstring)."""
    orc = oracle_problems(coeffs, t, diag_user, y) if orc is None else orc
    pd = orc["info"] == 0
    if not pd.any():
        return None
    cond = float(orc["cond"][pd].max())
    if cond > COND_MAX:
        return f"conditioning {cond:.1e}: beyond float64 at 1e-8"
    hot = [i for i in range(len(coeffs)) if pd[i] and orc["cond"][i] > COND_80]
    if hot:
        ll80 = loglike80([coeffs[i] for i in hot], t, [diag_user + coeffs[i][6] for i in hot], y)
        ref = orc["ref"][hot]
        rel = np.abs(ref - ll80) / np.abs(ll80)
        if not np.all(rel <= C_VS_80):
            return f"C vs 80-bit {float(rel.max()):.1e} at conditioning {cond:.1e}: beyond float64 at 1e-8"
    return None


def relmax(x, ref):
    return float(np.max(np.abs(np.asarray(x) - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


# ---------------------------------------------------------------------------------------------------------------
# problem generators


def narrow_problem(seed):
    """test_gpu_random.py's problem: J 1-30 SHO terms (up to 3 overdamped), random cadence pattern (uniform,
    jittered, gaps, clusters), noise level; the seed fixes everything."""
    from gadfly_amd.terms import SHOTerm, TermSum, TermConvolution
    rng = _rng(seed)
    J = int(rng.integers(1, 31))
    n_over = int(rng.integers(0, min(J, 3) + 1)) if rng.random() < 0.4 else 0
    terms = []
    for j in range(J):
        w0 = float(np.exp(rng.uniform(np.log(0.5), np.log(3000.0))))
        Q = float(rng.uniform(0.05, 0.45)) if j < n_over else float(np.exp(rng.uniform(np.log(0.5), np.log(300.0))))
        S0 = float(np.exp(rng.uniform(-2, 4)))
        terms.append(SHOTerm(S0=S0, w0=w0, Q=Q))
    dt = float(np.exp(rng.uniform(np.log(2e-5), np.log(2e-3))))          # cadence in 1e6 s
    N = int(rng.integers(40, 5000))
    kind = rng.choice(["uniform", "jitter", "gaps", "clusters"])
    t = np.arange(N) * dt
    if kind == "jitter":
        t = t + rng.uniform(-0.3, 0.3, N) * dt
    elif kind == "gaps":
        keep = np.ones(N, bool)
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, N - 1)); keep[a:a + int(rng.integers(1, max(2, N // 8)))] = False
        keep[0] = True
        t = t[keep]
    elif kind == "clusters":
        t = np.sort(rng.uniform(0, N * dt, N))
        t = np.unique(np.round(t / (dt * 1e-3)) * (dt * 1e-3))            # no exact duplicates
    t = np.sort(t)
    N = len(t)
    kernel = TermConvolution(TermSum(*terms), float(rng.uniform(0.1, 1.0)) * dt)
    yerr = 0.0 if rng.random() < 0.2 else float(np.exp(rng.uniform(-3, 2)))
    amp = float(np.sqrt(kernel.get_value(np.zeros(1))[0]))
    y = amp * rng.normal(size=N) + np.cumsum(rng.normal(size=N)) * 0.1 * amp
    return dict(kernel=kernel, t=t, y=y, diag_user=np.full(N, yerr ** 2), rng=rng, kind=kind, J=J)


def sho_kernels(S0, w0, Q, delta):
    """One exposure-integrated SHO-sum kernel object per row of the (B, J) arrays (the per-object path that
    `BatchedLogLikelihood.pack_parameters` vectorises)."""
    from gadfly_amd.terms import SHOTerm, TermSum, TermConvolution
    return [TermConvolution(TermSum(*[SHOTerm(S0=float(s), w0=float(w), Q=float(q)) for s, w, q in zip(*row)]),
                            float(delta)) for row in zip(S0, w0, Q)]


def wmax(co):
    """Largest rate max(c, |d|) of one coefficient tuple: what RowGen::init multiplies |t| of a tile's or chunk's
    first row with to decide qmode."""
    return float(max(np.max(co[1], initial=0.0), np.max(co[4], initial=0.0), np.max(np.abs(co[5]), initial=0.0)))


def _base_terms(rng, J, n_over):
    """(S0, w0, Q) of J terms, the first n_over overdamped; Q kept far enough from 1/2 that a jitter of 30 % leaves
    every term on its side (sho_coefficient_pack needs one overdamped pattern per batch)."""
    w0 = np.exp(rng.uniform(np.log(0.5), np.log(3000.0), J))
    S0 = np.exp(rng.uniform(-2, 4, J))
    Q = np.exp(rng.uniform(np.log(0.75), np.log(300.0), J))
    Q[:n_over] = rng.uniform(0.05, 0.33, n_over)
    return S0, w0, Q


def _walkers(rng, base, B):
    """(S0, w0, Q) arrays (B, J): every parameter of every walker scaled by a log-uniform factor within +-frac,
    frac drawn per walker from 2 ... 30 %."""
    frac = rng.uniform(0.02, 0.30, B)[:, None]
    out = []
    for v in base:
        f = np.exp(rng.uniform(np.log1p(-frac), np.log1p(frac), (B, len(v))))
        out.append(v[None, :] * f)
    return tuple(out)


def _axis(rng, N, dt, kind, w_cross=None):
    """A sorted time axis of N distinct stamps: uniform, jittered (+-0.3 cadence), gapped (1-3 gaps of 2-500
    cadences), moved to BKJD, or moved so that w_cross * t crosses QMODE_PHASE between rows r0 - 1 and r0 < 60 (the
    first tile or chunk of any route)."""
    t = np.arange(N) * dt
    if kind == "jitter":
        t = t + rng.uniform(-0.3, 0.3, N) * dt
    elif kind == "gaps":
        for _ in range(int(rng.integers(1, 4))):
            t[int(rng.integers(1, N)):] += int(rng.integers(2, 500)) * dt
    elif kind == "bkjd":
        t = t + BKJD0
    elif kind == "qcross":
        r0 = int(rng.integers(1, min(60, N - 1)))
        t = t + (QMODE_PHASE / w_cross - t[r0] + 0.5 * dt)
    return t


TILES = (64, 128, 320, 1024, 4096, 8192)


def batch_problem(seed):
    """A walker batch at the batched evaluator's settings: a base kernel of J 1-30 SHO terms (a shared overdamped
    pattern), exposure 0.1-1 cadence; B = 2-12 walkers around it for TWO proposals (S0, w0, Q of shape (2, B, J));
    an axis of AXES; a route ("stream": force_streaming, "auto": the evaluator's own choice -- time-parallel at
    N >= 8192, which 60 % of the "auto" seeds get); N 300-12 000 otherwise (40 % of those at k tile +- 1);
    tile_rows.  Half of the seeds have white noise of 5-100 % of the kernel's amplitude: conditions of at most a few
    hundred, where the product calibrates the longest periods (32 and 64) on every axis, the BKJD and the
    QMODE_PHASE-crossing ones included (random_cases_host checks that such seeds exist); the others a noise level
    independent of the amplitude, mostly badly conditioned problems at short periods."""
    rng = _rng(seed)
    J = int(rng.integers(1, 31))
    n_over = int(rng.integers(1, min(J, 3) + 1)) if rng.random() < 0.35 else 0
    base = _base_terms(rng, J, n_over)
    B = int(rng.integers(2, 13))
    props = [_walkers(rng, base, B) for _ in range(2)]
    S0, w0, Q = (np.stack([p[i] for p in props]) for i in range(3))
    assert np.all((Q < 0.5) == (base[2] < 0.5)[None, None, :])
    dt = float(np.exp(rng.uniform(np.log(2e-5), np.log(2e-3))))
    delta = float(rng.uniform(0.1, 1.0)) * dt
    tile = int(rng.choice(TILES))
    route = str(rng.choice(["stream", "auto"]))
    if route == "auto" and rng.random() < 0.6:
        N = int(rng.integers(8192, 12001))
    elif rng.random() < 0.4:
        T = max(64, tile // 64 * 64)
        k = int(rng.integers(max(1, -(-301 // T)), max(2, 11999 // T + 1)))
        N = min(max(k * T + int(rng.choice([-1, 1])), 300), 12000)
    else:
        N = int(rng.integers(300, 12001))
    kind = str(rng.choice(AXES))
    co_cross = sho_kernels(S0[1][:1], w0[1][:1], Q[1][:1], delta)[0].get_device_coefficients()
    t = _axis(rng, N, dt, kind, w_cross=wmax(co_cross))
    amp = float(np.sqrt(np.sum(base[0] * base[1] * base[2])))
    if rng.random() < 0.5:
        yerr = amp * float(np.exp(rng.uniform(np.log(0.05), 0.0)))
    else:
        yerr = 0.0 if rng.random() < 0.15 else float(np.exp(rng.uniform(-2, 2)))
    y = amp * rng.normal(size=N) + np.cumsum(rng.normal(size=N)) * 0.1 * amp
    return dict(S0=S0, w0=w0, Q=Q, delta=delta, t=t, y=y, yerr=yerr, diag_user=np.full(N, yerr ** 2), tile=tile,
                route=route, kind=kind, J=J, B=B, N=N, n_over=n_over, rng=rng)


def expected_route(prob):
    """(time-parallel, two-sweep) of the first evaluation of a batch_problem: what BatchedLogLikelihood.evaluate picks
    (engine.evaluate: time-parallel for the automatic route at N >= 8192; two sweeps where the pack is positive
    semi-definite by construction -- batch._exposure_resolved)."""
    from gadfly_amd.batch import _exposure_resolved
    t = prob["t"]
    tp = prob["route"] == "auto" and prob["N"] >= 8192
    return tp, tp and _exposure_resolved(prob["delta"], float(np.min(np.diff(t))), float(np.max(np.abs(t))))


def product_period(coeffs, t, cond):
    """The generator period StreamingBatch.period_for_condition picks for the condition `cond` of a batch with these
    coefficients on this axis: the engine's own formulas (GEN_ERR * period + the phase-quantum term), evaluated on the
    host -- so that coverage of the long periods can be checked without a device."""
    from gadfly_amd.engine import StreamingBatch as SB

    class _Host:
        GEN_ERR, PHASE_ERR, QMODE_PHASE = SB.GEN_ERR, SB.PHASE_ERR, SB.QMODE_PHASE
        phase_quantum = SB.phase_quantum
        phase_error_coefficient = SB.phase_error_coefficient
        generator_error_coefficient = SB.generator_error_coefficient
        period_for_condition = SB.period_for_condition

    h = _Host()
    h.N, h._tmax = len(t), float(np.max(np.abs(t)))
    h._pack = (None,) * 6 + (max(float(np.max(np.abs(co[5]), initial=0.0)) for co in coeffs),)
    return h.period_for_condition(cond)


def batch_calibration(prob, orc0=None):
    """(time-parallel, two-sweep, period) the batched evaluator reaches on a batch_problem after its first evaluation,
    predicted from the oracle: the condition max(a) / min(d) over the walkers of proposal 0 (times the two-sweep
    margin 1.5, StreamingBatch.TWO_SWEEP_MARGIN, where that route runs) through product_period.  period None where
    the oracle's factorisation fails."""
    from gadfly_amd.engine import StreamingBatch as SB
    coeffs = [k.get_device_coefficients() for k in sho_kernels(prob["S0"][0], prob["w0"][0], prob["Q"][0], prob["delta"])]
    orc0 = oracle_problems(coeffs, prob["t"], prob["diag_user"], prob["y"]) if orc0 is None else orc0
    tp, two = expected_route(prob)
    if np.any(orc0["info"] != 0):
        return tp, two, None
    cond = max(m[1].max() for m in orc0["mats"]) / min(d.min() for d in orc0["d"])
    return tp, two, product_period(coeffs, prob["t"], cond * (SB.TWO_SWEEP_MARGIN if two else 1.0))


def grad_problem(seed):
    """test_gpu_grad_random.py's problem: B = 2-6 walkers around a base kernel of J 1-30 SHO terms (a shared overdamped
    pattern; W = 2J <= 60, the gradient kernel's one-wave range), exposure 0.1-1 cadence, N = 40-1500 rows on an axis of
    AXES (the QMODE_PHASE-crossing one placed by walker 0's rates), white noise of 5-100 % of the kernel's amplitude:
    well conditioned by construction (test_grad_host.py checks max(a) / min(d) <= 1e4 for every walker), so no seed
    and no walker is ever skipped."""
    rng = _rng(seed)
    J = int(rng.integers(1, 31))
    n_over = int(rng.integers(1, min(J, 3) + 1)) if rng.random() < 0.35 else 0
    base = _base_terms(rng, J, n_over)
    B = int(rng.integers(2, 7))
    S0, w0, Q = _walkers(rng, base, B)
    assert np.all((Q < 0.5) == (base[2] < 0.5)[None, :])
    dt = float(np.exp(rng.uniform(np.log(2e-5), np.log(2e-3))))
    delta = float(rng.uniform(0.1, 1.0)) * dt
    N = int(rng.integers(40, 1501))
    kind = str(rng.choice(AXES))
    co = sho_kernels(S0[:1], w0[:1], Q[:1], delta)[0].get_device_coefficients()
    t = _axis(rng, N, dt, kind, w_cross=wmax(co))
    amp = float(np.sqrt(np.sum(base[0] * base[1] * base[2])))
    yerr = amp * float(np.exp(rng.uniform(np.log(0.05), 0.0)))
    y = amp * rng.normal(size=N) + np.cumsum(rng.normal(size=N)) * 0.1 * amp
    return dict(S0=S0, w0=w0, Q=Q, delta=delta, t=t, y=y, yerr=yerr, diag_user=np.full(N, yerr ** 2), kind=kind,
                J=J, B=B, N=N, n_over=n_over, rng=rng)


def wide_problem(seed):
    """A wide kernel (J 32-88 SHO terms, W = 64 ... 176 after the overdamped terms' complexification; 40 % of the
    seeds with 1-3 overdamped terms) and TWO walkers with different coefficients (+-2 ... 30 %) on a uniform,
    jittered or gapped axis of 1500-4000 rows."""
    rng = _rng(seed)
    n_over = int(rng.integers(1, 4)) if rng.random() < 0.4 else 0
    J = int(rng.integers(32, 89 - n_over))
    base = _base_terms(rng, J, n_over)
    S0, w0, Q = _walkers(rng, base, 2)
    dt = float(np.exp(rng.uniform(np.log(2e-5), np.log(2e-3))))
    delta = float(rng.uniform(0.1, 1.0)) * dt
    N = int(rng.integers(1500, 4001))
    kind = str(rng.choice(["uniform", "jitter", "gaps"]))
    t = _axis(rng, N, dt, kind)
    yerr = 0.0 if rng.random() < 0.2 else float(np.exp(rng.uniform(-3, 2)))
    amp = float(np.sqrt(np.sum(base[0] * base[1] * base[2])))
    y = amp * rng.normal(size=N) + np.cumsum(rng.normal(size=N)) * 0.1 * amp
    L = int(rng.choice([192, 256, 640, 1024]))
    return dict(S0=S0, w0=w0, Q=Q, delta=delta, t=t, y=y, diag_user=np.full(N, yerr ** 2), kind=kind, J=J, N=N,
                n_over=n_over, chunk_len=L, rng=rng)
