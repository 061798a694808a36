"""Cases of the fused sweeps (gf_loglike_fused, gf_sample_fused) in streamed mode, shared by
tests/test_fused_cases_host.py and tests/test_gpu_fused_rows.py.  Host only: numpy and the oracle, no device import.

Problems are tests.grad_cases.edge_problem's coefficients and data on axes built here.  The device is handed
``diag`` (the observational noise), ``diag_add[b] = amp_b + 0.01 amp_b`` (what include/gadfly_hip.h calls diag_add: the
sum of the amplitudes plus a diagonal shift, here a nonzero one per problem) and ``cmax[b]`` = the largest decay rate;
the reference diagonal handed to oracle/seq.py (which adds the amplitudes itself) is ``diag + 0.01 amp_b``.  Conditions
max(a) / min(d) of 8..16.  References are the float64 C oracle (oracle/cref.py) on oracle/seq.py's float64 matrices --
celerite2's statement, phases theta_n = fl(d t_n) included: on stretched and far axes the 80-bit form of oracle/seq.py
takes sin / cos of UNROUNDED phases and is another function of t."""
import functools

import numpy as np

from oracle import cref, seq
from tests import grad_cases as gc
from tests import sweep_cases as sc

TOL = sc.TOL                        # 1e-10 of the largest reference entry of the array: d, z and draws
DT = gc.DT
N = 384                             # six scaling blocks of 64 rows
SHIFT = 2454833.0 * 0.0864          # a JD-based time axis in the library's units
SPAN, SPAN_LONG = 28.0, 128.0       # gf_scaled_span(0), gf_scaled_span(1)  (test_gpu_fused_rows.py compares them)
N_FAR = 128                         # the regular rows of the composite axis

#: every W = 1..63 as (W % 2, W // 2), the all-real structures W = 3, 4, 5, 63 and three mixed ones (W = 32, 63, 62):
#: k_factor3<R> and k_factor3<R, true>, R = 4..64, both pad parities of each R
NARROW = tuple((W % 2, W // 2) for W in range(1, 64)) + ((3, 0), (4, 0), (5, 0), (63, 0), (2, 15), (3, 30), (4, 29))
#: Jr = 0, Jc = 1..31: k_factor7<R, false> and k_factor7<R, false, true>, R = 4..64, both pad parities of each R
TILED = tuple(s for s in NARROW if s[0] == 0)
#: both sides of every line of dispatch_factorw (W = 64..176): its 11 shapes (TR, NW)
WIDE = tuple((0, Jc) for Jc in (32, 33, 40, 41, 47, 48, 49, 56, 57, 63, 64, 65, 72, 73, 79, 80, 81, 88))
GRID = ((1, 0), (0, 1), (1, 15), (0, 31), (1, 31), (0, 44))
FAR = ((1, 0), (0, 1), (0, 16), (0, 31), (3, 30), (0, 44))
LAYOUT = ((1, 15), (0, 31))
FAIL = ((1, 15), (0, 31), (0, 44))
FAIL_ROWS = (0, 63, 64, 100)
BLOCKS = PERIODS = (1, 2, 4, 8, 16, 32, 64)
#: axes of the GRID structures (test_gpu_fused_rows.py's block rule): name -> span the stretch is made for
STRETCHES = {"stretch28": SPAN, "stretch128": SPAN_LONG, "gap098": SPAN, "gap102": SPAN}


def ident(s):
    return f"W{s[0] + 2 * s[1]}-{s[0]}r{s[1]}c"


def rows_of(W):
    """R of k_factor3<R> / k_factor7<R>: the width rounded up to a multiple of four."""
    return (W + 3) // 4 * 4


def wide_shape(W):
    """(TR, NW) of k_factorw, restated from wide_shape in gadfly_hip.hip (the instance table only)."""
    return (W + 15) // 16 * 4, (W + 1 + 31) // 32


# ---- axes ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def composite_axis(n=N):
    """One axis that holds every row kind of RowGen::advance, built from steps of DT (step k leads to row k):
    rows 0..127 regular; 128..191 each step times 1 + 2e-6 u, u uniform in +-1; 192..255 cadence 2 DT; a gap of 400 DT
    in front of row 270; row 300 late by 0.3 DT (steps 1.3 DT, 0.7 DT); 320.. steps jittered by +-20 %."""
    rng = np.random.default_rng(384)
    m = max(n, N)
    step = np.full(m, DT)
    step[128:192] *= 1.0 + 2e-6 * rng.uniform(-1.0, 1.0, 64)
    step[192:256] = 2.0 * DT
    step[270] = 400.0 * DT
    step[300], step[301] = 1.3 * DT, 0.7 * DT
    step[320:] *= 1.0 + 0.2 * rng.uniform(-1.0, 1.0, m - 320)
    step[0] = 0.0
    t = np.cumsum(step)
    t[:128] = np.arange(128) * DT
    t = t[:n].copy()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def plain_axis(n=N):
    """The regular cadence DT with the composite's one gap of 400 DT in front of row 270: the axis of the gap pair (on
    it a stretch decides for every row but one whether it resets on its own)."""
    step = np.full(n, DT)
    step[0] = 0.0
    if n > 270:
        step[270] = 400.0 * DT
    t = np.cumsum(step)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def far_axes():
    """(near, far): the regular rows of the composite axis moved by SHIFT, and the same stamps moved back -- the
    regular rows rounded to the far axis' grid (half an ulp of SHIFT: 1.5e-11), so that far - SHIFT == near and
    near + SHIFT == far hold exactly and both axes describe the same spacings."""
    far = composite_axis()[:N_FAR] + SHIFT
    near = far - SHIFT
    for x in (far, near):
        x.setflags(write=False)
    return near, far


def jitter_axis(prob, n=N):
    """The regular cadence with every step from row 3 on times 1 + e u, |u| in 0.8..1 with a random sign and e such
    that wmax * DT * e is 0.98 of the limit 2e-6 up to which RowGen::step corrects a spacing to second order, for the
    largest wmax of the structure: every rotation step takes the second-order branch with |x| of 0.78..0.98 of its
    limit (rows 1, 2 are regular: they set the cached spacing)."""
    rng = np.random.default_rng(2)
    e = 0.98 * 2e-6 / (float(np.max(prob["wmax"])) * DT)
    step = np.full(n, DT)
    step[0] = 0.0
    step[3:] *= 1.0 + e * rng.uniform(0.8, 1.0, n - 3) * rng.choice([-1.0, 1.0], n - 3)
    return np.cumsum(step)


def stretched(t, prob, frac, span):
    """The axis times the factor that makes 1.5 * 63 * cmax * DT = frac * span for the largest cmax of the structure:
    at block 64 the rule ``1.5 (block - 1) cmax cadence <= span`` used to the fraction frac."""
    return t * (frac * span / (1.5 * 63.0 * float(np.max(prob["cmax"])) * DT))


def gap_stretched(t, prob, frac, span):
    """The axis times the factor that makes cmax * DT = frac * span / 63 for the largest cmax: a regular row of that
    problem is frac of the gap that makes a row reset on its own at block 64."""
    return t * (frac * span / (63.0 * float(np.max(prob["cmax"])) * DT))


def axis(name, Jr, Jc, n=N, B=3):
    """Named axes, (n,) shared or (B, n) per problem: composite; own (composite * (1 + b / 64)); stretch28 /
    stretch128 (composite, the block rule at 0.98 of either span); gap098 / gap102 (plain, a regular row at 0.98 /
    1.02 of the reset gap); jitter (second-order steps near their limit); near / far."""
    if name == "composite":
        return composite_axis(n)
    if name == "own":
        return composite_axis(n)[None, :] * (1.0 + np.arange(B) / 64.0)[:, None]
    if name in ("near", "far"):
        assert n == N_FAR
        return far_axes()[name == "far"]
    prob = problem(Jr, Jc, n, B)
    if name == "jitter":
        return jitter_axis(prob, n)
    if name in ("stretch28", "stretch128"):
        return stretched(composite_axis(n), prob, 0.98, STRETCHES[name])
    assert name in ("gap098", "gap102"), name
    return gap_stretched(plain_axis(n), prob, 0.98 if name == "gap098" else 1.02, SPAN)


# ---- problems --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def problem(Jr, Jc, n=N, B=3):
    """grad_cases.edge_problem(Jr, Jc, n, B) without its axis, with what the fused entry points take: real, comp,
    diag (B, n), y, eps (B, n), amp, shift = 0.01 amp, diag_add = amp + shift, cmax, wmax (B,)."""
    p = gc.edge_problem(Jr, Jc, n, B)
    amp = p["diag_add"]
    cr, cc, dc = p["real"][1, :, :Jr], p["comp"][2, :, :Jc], p["comp"][3, :, :Jc]
    rates = np.concatenate([cr, cc], axis=1)
    out = dict(Jr=Jr, Jc=Jc, N=n, B=B, real=p["real"], comp=p["comp"], diag=p["diag"], y=p["y"], amp=amp,
               shift=0.01 * amp, diag_add=amp + 0.01 * amp, cmax=np.max(rates, axis=1),
               wmax=np.max(np.concatenate([rates, np.abs(dc)], axis=1), axis=1),
               eps=np.random.default_rng([7, Jr, Jc, n]).normal(size=(B, n)),
               co=tuple(gc.coefficients(p, b) for b in range(B)))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def device_diag(prob, mode="own", fail=None):
    """The ``diag`` argument of the entry points: own (B, n); shared (n,) -- problem 0's for all; none: None.  fail =
    (b, r): problem b's rows from r on hold -2 amp_b, a diagonal no pivot survives."""
    if mode == "none":
        return None
    if mode == "shared":
        return prob["diag"][0]
    diag = np.array(prob["diag"])
    if fail is not None:
        b, r = fail
        diag[b, r:] = -2.0 * prob["amp"][b]
    return diag


@functools.lru_cache(maxsize=None)
def rows(Jr, Jc, axis_name="composite", n=N, B=3, diag="own", fail=None):
    """The float64 C oracle's rows of every problem on a named axis, computed once and shared (read-only): tuple of
    dicts t, a, d, z = L^-1 y, draw = L D^1/2 eps, info.  With a failing pivot (info = its 1-based row) d, z and draw
    hold the rows in front of it."""
    prob = problem(Jr, Jc, n, B)
    T = axis(axis_name, Jr, Jc, n, B)
    dg = device_diag(prob, diag, fail)
    out = []
    for b in range(B):
        t = T[b] if T.ndim == 2 else T
        noise = 0.0 if dg is None else dg[b] if dg.ndim == 2 else dg
        c, a, U, V = seq.celerite_matrices(prob["co"][b], t, noise + prob["shift"][b])
        d, Wm, info = cref.factor(t, c, a, U, V)
        m = n if info == 0 else info - 1
        r = dict(t=t, a=a, info=info, d=d[:m], z=np.zeros(0), draw=np.zeros(0))
        if m:
            r["z"] = cref.solve_lower(t[:m], c, U[:m], Wm[:m], prob["y"][b, :m])
            r["draw"] = cref.matmul_lower(t[:m], c, U[:m], Wm[:m], prob["eps"][b, :m] * np.sqrt(d[:m]))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return tuple(out)


def rows_80bit(Jr, Jc, axis_name, b=0, n=N, B=3):
    """(d, z) of problem b from oracle/seq.py in np.longdouble throughout, the matrix build included (its phases
    d t are 80-bit products, not celerite2's rounded ones)."""
    prob = problem(Jr, Jc, n, B)
    T = axis(axis_name, Jr, Jc, n, B)
    t = np.asarray(T[b] if T.ndim == 2 else T, dtype=np.longdouble)
    c, a, U, V = seq.celerite_matrices(prob["co"][b], t, prob["diag"][b] + prob["shift"][b], dtype=np.longdouble)
    d, Wm, info = seq.factor(t, c, a, U, V)
    assert info == 0
    return d, seq.solve_lower(t, c, U, Wm, np.asarray(prob["y"][b], dtype=np.longdouble))


# ---- the generator's row kinds ---------------------------------------------------------------------------------------

KINDS = ("anchor", "sub_anchor", "exact", "refresh", "first_order", "second_order")


def row_kinds(t, wmax, cmax, block, period, span=SPAN):
    """Which branch of RowGen::advance (gadfly_hip.hip) every row of t takes, counted: anchor (block reset or a gap),
    sub_anchor (exact phasor on the cached spacing), exact (a row on another spacing; ``refresh`` counts those of them
    that re-cache the multiplier, so the other five kinds add up to len(t)), first_order and second_order rotation
    steps.  A restatement of RowGen::peek / advance that exists ONLY to prove that the inputs reach every branch --
    never a reference for values.  Its constants (2e-6 and 1.4e-9 over wmax, the phase bound 4e6 of qmode, the spans
    28 / 128 over block - 1) DUPLICATE the kernel's: a change there must be repeated here."""
    t = np.asarray(t, dtype=np.float64)
    gthr = (span / (block - 1) if block > 1 else 0.0) / cmax
    jthr = 2e-6 / wmax
    qmode = wmax * abs(t[0]) > 4.0e6
    jthr1 = 0.0 if qmode else 1.4e-9 / wmax
    count = dict.fromkeys(KINDS, 0)
    t_m1, dt_ref, dt_last = t[0], -1.0, -2.0
    for g, tn in enumerate(t):
        dt = tn - t_m1
        ddt = dt - dt_ref
        t_m1 = tn
        if (g & (block - 1)) == 0 or dt > gthr:
            count["anchor"] += 1
        elif (g & (period - 1)) != 0 and abs(ddt) < jthr:
            count["first_order" if abs(ddt) < jthr1 else "second_order"] += 1
        elif abs(ddt) < jthr:
            count["sub_anchor"] += 1
        else:
            count["exact"] += 1
            if abs(dt - dt_last) < jthr:
                count["refresh"] += 1
                dt_ref = dt
            dt_last = dt
    assert sum(count[k] for k in KINDS if k != "refresh") == len(t)
    return count
