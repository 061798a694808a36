"""Shared cases of the steady tail's instance tests (not a conftest): the series of the longest tail
behind a forced switch -- tests/test_gpu_steady_split.py's ANCHOR, ARM and tiles of T rows --, J-term kernels for every
J = 1 .. 31 (ROWS = 4 ceil(2 J / 4) = 4, 8, .. 64: every instance of the STEADY sweep, k_steady_tail and k_steady_finish,
at both parities of its padding), the C oracle's exact rows d, z on that series, and the sums of a tail of k rows on
those rows.  tests/test_steady_instances_host.py shows that on these inputs the exact rows are a reference for the
frozen filter three orders of magnitude below the bars of tests/test_gpu_steady_instances.py."""
import functools
from types import SimpleNamespace

import numpy as np

from tests.random_cases import oracle_loglikes
from tests.test_gpu_steady import RTOL_LL, _evaluator, _fast_terms, _rel, _series
from tests.test_gpu_steady_finish import B_FIN, RTOL_PLAIN, _steady_and_plain
from tests.test_gpu_steady_split import ANCHOR, ARM, T
from tests.test_steady_host import _switch_row
from tests.test_steady_tail_host import LAG_ROWS

LONGEST = 193           # rows of the longest tail: three blocks and a row
SW = ANCHOR + 1         # the first tail row, as steady[b][0] counts it
N_LONG = SW + LONGEST
J_ALL = tuple(range(1, 32))
TAILS_HOST = (1, 2, 65, LONGEST)


def oracle_rows(hp, t, y):
    """One kernel on the series: the oracle's factor and forward solve, and the rule's switch row under arm_from = ARM
    (asserted to be ANCHOR, with info == 0).  Returns d, W, z, the derotated gain and the pivot at ANCHOR, and the
    kernel's coefficients."""
    import gadfly_amd
    from oracle import cref
    co = gadfly_amd.StellarOscillatorKernel(hp, texp=60.0).get_device_coefficients()
    c, a, U, V = cref.get_matrices(co[:6], t, np.full(len(t), 900.0) + co[6])
    d, W, info = cref.factor(t, c, a, U, V)
    assert info == 0
    row, gain, dinf = _switch_row(t[ARM:], np.asarray(co[5], dtype=np.float64), d[ARM:], W[ARM:])
    assert ARM + row == ANCHOR, (ARM, row, ANCHOR)
    assert dinf == d[ANCHOR]
    z = cref.solve_lower(t, c, U, W, y)
    return SimpleNamespace(co=co, c=c, d=d, W=W, z=z, gain=gain, dinf=dinf)


def frozen_state(rows, t):
    """What the frozen filter starts from at ANCHOR (tests/test_steady_tail_host.py::_frozen with the switch where
    arm_from = ARM puts it): alpha, lambda's exponent (c + i d) Delta, G and the folded derotated state."""
    co, sw = rows.co, ANCHOR
    ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in co[2:6])
    F = np.zeros(rows.W.shape[1])
    for n in range(sw + 1):                 # celerite's F just after row sw, that row's update folded
        if n:
            F *= np.exp(-rows.c * (t[n] - t[n - 1]))
        F += rows.W[n] * rows.z[n]
    s = np.exp(-1j * dc * t[sw]) * (F[0::2] + 1j * F[1::2])
    delta = (t[sw] - t[sw - LAG_ROWS]) / LAG_ROWS
    return dict(alpha=ac + 1j * bc, expo=(cc + 1j * dc) * delta, G=rows.gain, s=s)


def row_form(fz, ytail, dtype=np.clongdouble):
    """The frozen row form x = lambda s; z_n = y_n - sum_k Re(alpha_k x_k); s = x + G z_n over ytail, in `dtype`."""
    real = np.longdouble if dtype is np.clongdouble else np.float64
    alpha, G, s = fz["alpha"].astype(dtype), fz["G"].astype(dtype), fz["s"].astype(dtype)
    lam = np.exp(-fz["expo"].astype(dtype))
    out = np.empty(len(ytail), dtype=real)
    for i, yn in enumerate(ytail):
        x = lam * s
        out[i] = real(yn) - np.sum((alpha * x).real)
        s = x + G * out[i]
    return out


def tail_sums(d, z, sw=SW, longest=LONGEST):
    """On the oracle's rows, for the tails of k = 1 .. longest rows behind row sw (entry k - 1: the rows sw .. sw + k - 1),
    from one pass: sum log d_n, sum z_n^2 / d_n, sum |z_n|."""
    dd, zz = d[sw:sw + longest].astype(np.longdouble), z[sw:sw + longest].astype(np.longdouble)
    assert len(dd) == longest
    return SimpleNamespace(logd=np.cumsum(np.log(dd)).astype(np.float64),
                           z2d=np.cumsum(zz * zz / dd).astype(np.float64),
                           zabs=np.cumsum(np.abs(zz)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def case(J):
    """The series of the longest tail, B_FIN kernels of J terms with their device coefficients, and per problem the
    oracle's d, z and log-likelihood on that series, max |z| over the whole series and the tails' sums; the shorter
    series are its first rows.  Computed once per J and shared: nobody writes to it."""
    t, y = _series(N_LONG, seed=47)
    hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
    rows = [oracle_rows(hp, t, y) for hp in hps]
    coeffs = [r.co for r in rows]
    ll, info = oracle_loglikes(coeffs, t, np.full(N_LONG, 900.0), y)
    assert np.all(info == 0)
    d, z = np.stack([r.d for r in rows]), np.stack([r.z for r in rows])
    for a in (d, z, ll):
        a.setflags(write=False)
    return SimpleNamespace(J=J, hps=hps, t=t, y=y, coeffs=coeffs, d=d, z=z, loglike=ll, zmax=np.max(np.abs(z), axis=1),
                           sums=[tail_sums(d[b], z[b]) for b in range(B_FIN)])


def _case(J):
    """tests/test_gpu_steady_fold.py's view of case(J): the kernels and the series."""
    c = case(J)
    return c.hps, c.t, c.y


def _run(hps, t, y, tail, what):
    """The evaluator's own route on the first ANCHOR + 1 + tail rows, switch forced to ANCHOR: against the oracle and
    against the plain sweep."""
    N = ANCHOR + 1 + tail
    t, y = t[:N], y[:N]
    ev, coeffs = _evaluator(hps, t, y, T)
    ref, info = oracle_loglikes(coeffs, t, np.full(N, 900.0), y)
    assert np.all(info == 0)
    ev.engine._steady_axis = (ARM, 0.0)
    got, plain, sw = _steady_and_plain(ev)
    print(f"{what}: switch rows {sw.tolist()} of {N}, error vs oracle {_rel(got, ref).max():.2e}, "
          f"steady vs plain {_rel(got, plain).max():.2e}")
    assert np.all(sw == ANCHOR + 1) and np.all(N - sw == tail), sw.tolist()
    assert _rel(got, ref).max() <= RTOL_LL
    assert _rel(got, plain).max() <= RTOL_PLAIN
    assert ev.steady_reruns == 0
