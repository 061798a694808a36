"""Host side of the four-row state step of the steady tail's finishing block (k_steady_finish / k_steady_chunk,
DESIGN.md 3.10), restated in numpy float64 on the C oracle's own factor: the folded block z = u + Q s of
tests/test_steady_fold_host.py, then the state over the block's rows as the kernel now takes them --
    s <- lambda^4 s + (lambda^3 G z_j + lambda^2 G z_j+1 + lambda G z_j+2 + G z_j+3),
eight trips on the rows 0 .. 31 from the incoming state, eight on the rows 32 .. 63 from a zero state, joined by
lambda^32 (four more squarings of lambda^2) -- beside the two-row split of tests/test_steady_finish_host.py on the
same blocks.

The reference is the frozen row form in longdouble (tests/steady_cases.py::row_form, restated here so that it takes
the float64 lambda the block forms use, bit for bit, and returns the state behind marked rows too): never the device.
The four-row form has half the roundings on the chain from block to block, so it may lie no farther from the
reference than the two-row form does on the same case, times 2 for the reordering: asserted for the state behind 1,
2, 16 and 240 blocks and for the sum of z^2 -- per row slot of a block first, as the lanes sum it -- over the 240 blocks."""
import numpy as np
import pytest

from tests.test_steady_finish_host import _advance_split
from tests.test_steady_fold_host import L, _tables
from tests.test_steady_host import _two_terms
from tests.test_steady_tail_host import _frozen, _problem

BLOCKS = (1, 2, 16, 240)    # the states compared: behind a block, two, a group of the launch, and a long tail
FACTOR = 2.0                # the four-row form's distance from the reference against the two-row form's own
N = 65536


def _row_form_ld(fz, ytail, marks):
    """tests/steady_cases.py::row_form in longdouble on fz's own float64 lambda, G, alpha and state: z of every row of
    ytail and the state behind the rows listed in `marks` (counts of rows)."""
    ld, cld = np.longdouble, np.clongdouble
    alpha, lam, G, s = (fz[k].astype(cld) for k in ("alpha", "lam", "G", "s"))
    z, states = np.empty(len(ytail), dtype=ld), {}
    for i, yn in enumerate(ytail):
        x = lam * s
        z[i] = ld(yn) - np.sum((alpha * x).real)
        s = x + G * z[i]
        if i + 1 in marks:
            states[i + 1] = s.copy()
    return z, states


def _advance_four(lam, G, s, zb):
    """A full block's state update as the kernel runs it: both halves in trips of four rows, then the join.  The
    kernel's set-up forms lambda^4, lambda^32 and lambda^k G in double-double and rounds each once; here they come from
    longdouble powers, rounded once."""
    ll, gl = lam.astype(np.clongdouble), G.astype(np.clongdouble)
    lam4, lam32, lG, l2G, l3G = ((ll ** 4).astype(np.complex128), (ll ** 32).astype(np.complex128),
                                 (ll * gl).astype(np.complex128), (ll ** 2 * gl).astype(np.complex128),
                                 (ll ** 3 * gl).astype(np.complex128))
    halves = []
    for h, sh in ((0, s), (1, np.zeros_like(s))):
        for t in range(8):
            j = 32 * h + 4 * t
            w = l3G * zb[j] + (l2G * zb[j + 1] + (lG * zb[j + 2] + G * zb[j + 3]))
            sh = lam4 * sh + w
        halves.append(sh)
    return lam32 * halves[0] + halves[1]


def _blocks(fz, ytail, advance):
    """240 folded blocks z = u + Q s from fz's state under one form of the state update: the states behind the
    blocks of BLOCKS and the sum of z^2 as the lanes form it."""
    lam, G, s = fz["lam"], fz["G"], fz["s"].copy()
    H, _, Q = _tables(fz)
    lanes, states = np.zeros(L), {}
    for b in range(BLOCKS[-1]):
        zb = H @ ytail[L * b:L * (b + 1)] + Q @ np.concatenate([s.real, s.imag])
        lanes += zb * zb
        s = advance(lam, G, s, zb)
        if b + 1 in BLOCKS:
            states[b + 1] = s.copy()
    return states, float(np.sum(lanes))


def _case(hp):
    coeffs, t, diag, y, _ = _problem(hp, N)
    fz = _frozen(coeffs, t, diag, y)
    rows = L * BLOCKS[-1]
    assert 0 < fz["sw"] and fz["sw"] + 1 + rows <= N, fz["sw"]
    ytail = y[fz["sw"] + 1:fz["sw"] + 1 + rows]
    zl, sl = _row_form_ld(fz, ytail, {L * b for b in BLOCKS})
    lanes = np.zeros(L, dtype=np.longdouble)
    for r in range(L):
        lanes[r] = np.sum(zl[r::L] * zl[r::L])
    return fz, ytail, sl, np.sum(lanes)


def _distances(fz, ytail, sl, ql, advance):
    states, q = _blocks(fz, ytail, advance)
    out = {}
    for b in BLOCKS:
        ref = sl[L * b]
        out[f"state behind {b} blocks"] = float(np.max(np.abs(states[b].astype(np.clongdouble) - ref))
                                                / np.max(np.abs(ref)))
    out["sum of z^2"] = float(abs(np.longdouble(q) - ql) / ql)
    return out


def _compare(hp, what):
    fz, ytail, sl, ql = _case(hp)
    two = _distances(fz, ytail, sl, ql, _advance_split)
    four = _distances(fz, ytail, sl, ql, _advance_four)
    for key in two:
        print(f"{what}, switch row {fz['sw']}, {key}: two-row split {two[key]:.2e}, four-row split {four[key]:.2e} "
              f"from the longdouble row form")
    for key in two:
        assert four[key] <= FACTOR * two[key], (what, key, four[key], two[key])


def test_four_row_step_on_the_flagship_walker():
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    _compare(jitter_hyperparameters(solar_like_hyperparameters(30), 1000), "flagship walker")


@pytest.mark.parametrize("terms", [((50.0, 30.0, 3e4), (2.0, 3000.0, 2.0)), ((1e4, 2.0, 50.0), (2.0, 3000.0, 5.0))])
def test_four_row_step_on_the_slow_two_term_kernels(terms):
    _compare(_two_terms(*terms), f"two terms {terms}")
