"""Host side of the folded block of the steady tail's finishing launch (k_steady_finish), restated in
numpy on the C oracle's own factor: with C the block's p coefficients (p = y + C s), the present block form runs
z = H (y + C s); the folded form runs z = u + Q s with Q = H C built by applying H to the coefficient columns and
u = H y formed one block ahead, then the same state update split over the two half-waves.  Both are compared with the
row form (tests/test_steady_tail_host.py) in what the launch keeps: the sum of z^2 -- per row slot of a block first, as
the lanes sum it -- and the state behind the last row.  The folded form may err at most 4 times as much as the present
block form on the same case (one more rounding layer), or 1e-13 relative, whichever is larger."""
import numpy as np
import pytest

from tests.test_gpu_steady import _fast_terms
from tests.test_steady_finish_host import _advance_split
from tests.test_steady_tail_host import _frozen, _impulse_response, _problem

L = 64
FLOOR = 1e-13           # relative; below it the two forms are not told apart
FACTOR = 4.0            # the folded form's error against the present block form's


def _row_form(fz, y):
    """z of the rows sw + 1 .. N - 1 one by one, and the state behind the last of them."""
    alpha, lam, G, s = fz["alpha"], fz["lam"], fz["G"], fz["s"].copy()
    z = np.empty(len(y) - fz["sw"] - 1)
    for i, yn in enumerate(y[fz["sw"] + 1:]):
        x = lam * s
        z[i] = yn - np.sum((alpha * x).real)
        s = x + G * z[i]
    return z, s


def _tables(fz):
    """H (lower-triangular Toeplitz of the impulse response), C with p = y + C (s_r, s_i), and Q = H C column by
    column, as the kernel's set-up builds it."""
    alpha, lam = fz["alpha"], fz["lam"]
    h = _impulse_response(fz, L)
    H = np.zeros((L, L))
    for m in range(L):
        H += np.diag(np.full(L - m, h[m]), -m)
    coef = alpha[None, :] * lam[None, :] ** np.arange(1, L + 1)[:, None]        # [row in block][term]
    C = np.concatenate([-coef.real, coef.imag], axis=1)                         # Re(coef s) = Re s_r - Im s_i
    Q = np.stack([H @ C[:, k] for k in range(C.shape[1])], axis=1)
    return H, C, Q


def _block_form(fz, y, fold):
    """Blocks of 64 rows from the switch row on.  Returns (sum of z^2 as the lanes form it, final state)."""
    lam, G, s = fz["lam"], fz["G"], fz["s"].copy()
    H, C, Q = _tables(fz)
    first, N = fz["sw"] + 1, len(y)
    last = N - 1

    def block_y(b0):                            # rows b0 .. b0 + 63, clamped to the last row as the kernel's loads are
        return y[np.minimum(np.arange(b0, b0 + L), last)]

    lanes = np.zeros(L)
    u = H @ block_y(first) if fold else None                # the prologue's u
    for b0 in range(first, N, L):
        lim = min(L, N - b0)
        sv = np.concatenate([s.real, s.imag])
        if fold:
            zb = u + Q @ sv
            u = H @ block_y(b0 + L)             # the next block's, from the data alone (dropped behind the last block)
        else:
            zb = H @ (block_y(b0) + C @ sv)
        lanes[:lim] += zb[:lim] ** 2
        s = _advance_split(lam, G, s, zb[:lim])
    return float(np.sum(lanes)), s


def _compare(fz, y, what):
    zr, sr = _row_form(fz, y)
    lanes = np.bincount(np.arange(len(zr)) % L, weights=zr * zr, minlength=L)
    q_row = float(np.sum(lanes))
    smax = np.max(np.abs(sr))
    err = {}
    for name, fold in (("block", False), ("folded", True)):
        q, s = _block_form(fz, y, fold)
        err[name] = (abs(q - q_row) / q_row, np.max(np.abs(s - sr)) / smax)
    print(f"{what}: sum z^2 block {err['block'][0]:.2e} folded {err['folded'][0]:.2e}; "
          f"state block {err['block'][1]:.2e} folded {err['folded'][1]:.2e}")
    for i, quantity in enumerate(("sum z^2", "state")):
        bound = max(FACTOR * err["block"][i], FLOOR)
        assert err["folded"][i] <= bound, (what, quantity, err["folded"][i], bound)


@pytest.fixture(scope="module", params=[1, 30, 31])
def fast(request):
    """J well-damped terms (tests/test_gpu_steady.py's kernels): the oracle's factor freezes within a few thousand rows."""
    J = request.param
    coeffs, t, diag, y, _ = _problem(_fast_terms(J), 8192)
    fz = _frozen(coeffs, t, diag, y)
    assert 1024 < fz["sw"] < 8192 - 130, fz["sw"]
    return J, fz, y


@pytest.mark.parametrize("tail", [1, 63, 64, 65, 128, 129])
def test_folded_block_against_the_row_form(fast, tail):
    """Tails of: one row; a partial block alone; exactly one block (its look-ahead is dropped); a one-row second block;
    two full blocks; two and a row."""
    J, fz, y = fast
    _compare(fz, y[:fz["sw"] + 1 + tail], f"J = {J}, tail of {tail} rows")


def test_folded_block_on_the_headline_workload():
    """The benchmark's kind of series (red plus white noise at the headline's amplitudes, its generator) under the flagship
    walker's hyperparameters, a few thousand rows behind the switch: the cancellation of H y against Q s is the
    workload's."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    N = 36864
    coeffs, t, diag, y, _ = _problem(jitter_hyperparameters(solar_like_hyperparameters(30), 1000), N)
    fz = _frozen(coeffs, t, diag, y)
    assert 0 < fz["sw"] < N - 4000 and (N - fz["sw"] - 1) % L != 0
    _compare(fz, y, f"flagship walker, switch row {fz['sw']}, tail of {N - fz['sw'] - 1} rows")
