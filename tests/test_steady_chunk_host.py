"""Host side of the chunked finishing launch of the steady tail (gf_steady_finish_chunked), restated in
numpy on the C oracle's own factor.  Behind the switch a 64-row block is linear and time-invariant in the state:
z = u + Q s, s' = M s + K u with one real 2J x 2J matrix M per problem, so a chunk of n = 2^k blocks that starts from
s_in ends in  s_out = M^n s_in + s_out0,  s_out0 the end state of the same chunk started from zero.  The launch runs
    pass A: chunk 0 from the true state; every later chunk but the last from zero (its s_out0);
    scan:   P = M^n by k squarings, M column by column from the block body on unit states with u = 0;
            s_in[1] = s_out[0],  s_in[c + 1] = s_out0[c] + P s_in[c];
    pass B: the chunks 1 .. last again, from their true s_in, summing z^2;
and adds the chunks' sums in chunk order.  It is compared with the row form in what the launch keeps -- the sum of z^2
and the state behind the last row -- under the fold test's own rule: it may err at most FACTOR times as much as the
sequential folded block form on the same case, or FLOOR relative, whichever is larger.  The correction by P is of
order one on these inputs: with P = 0 the flagship and the slow walker miss the bar."""
import numpy as np
import pytest

from tests.test_gpu_steady import _fast_terms
from tests.test_steady_finish_host import _advance_split
from tests.test_steady_fold_host import FACTOR, FLOOR, L, _block_form, _row_form, _tables
from tests.test_steady_tail_host import _frozen, _problem

CHUNK_BLOCKS = 16
CHUNK = CHUNK_BLOCKS * L


def _vec(s):
    return np.concatenate([s.real, s.imag])


def _cplx(v):
    J = len(v) // 2
    return v[:J] + 1j * v[J:]


def _block(fz, Q, s, u, lim=L):
    """The folded block body: z = u + Q s, then the state over the block's first `lim` rows on both half-waves."""
    zb = u + Q @ _vec(s)
    return zb, _advance_split(fz["lam"], fz["G"], s, zb[:lim])


def _block_map(fz, Q):
    """M, column by column: the block body on the 2J unit states with u = 0 -- the arithmetic of the blocks themselves."""
    J2 = 2 * len(fz["lam"])
    M = np.empty((J2, J2))
    for j in range(J2):
        e = np.zeros(J2)
        e[j] = 1.0
        M[:, j] = _vec(_block(fz, Q, _cplx(e), np.zeros(L))[1])
    return M


def _chunk_power(M, blocks):
    assert blocks >= 1 and blocks & (blocks - 1) == 0
    P = M
    while blocks > 1:
        P, blocks = P @ P, blocks // 2
    return P


def _chunk_rows(fz, y, H, Q, s, r_lo, r_hi):
    """Blocks of 64 rows over [r_lo, r_hi) from the state s: (the lanes' sums of z^2, the end state).  y is clamped to
    the series' last row as the kernel's loads are; a partial block can only be the series' last."""
    lanes, last = np.zeros(L), len(y) - 1
    for b0 in range(r_lo, r_hi, L):
        lim = min(L, r_hi - b0)
        zb, s = _block(fz, Q, s, H @ y[np.minimum(np.arange(b0, b0 + L), last)], lim)
        lanes[:lim] += zb[:lim] ** 2
    return float(np.sum(lanes)), s


def _chunked_form(fz, y, chunk=CHUNK, zero_P=False):
    """(sum of z^2 as the launch adds it, final state, ||P||_2, chunks)."""
    H, _, Q = _tables(fz)
    first, N = fz["sw"] + 1, len(y)
    nch = max(1, -(-(N - first) // chunk))
    lo = [first + c * chunk for c in range(nch)]
    hi = [min(r + chunk, N) for r in lo]
    P = _chunk_power(_block_map(fz, Q), chunk // L)
    if zero_P:
        P = np.zeros_like(P)
    zero = np.zeros_like(fz["s"])
    # pass A
    q, s_end = [0.0] * nch, [None] * nch
    q[0], s_end[0] = _chunk_rows(fz, y, H, Q, fz["s"].copy(), lo[0], hi[0])
    for c in range(1, nch - 1):
        _, s_end[c] = _chunk_rows(fz, y, H, Q, zero, lo[c], hi[c])
    # scan and pass B
    s_in = s_end[0]
    for c in range(1, nch):
        q[c], s_fin = _chunk_rows(fz, y, H, Q, s_in, lo[c], hi[c])
        if c < nch - 1:
            s_in = s_end[c] + _cplx(P @ _vec(s_in))
    if nch == 1:
        s_fin = s_end[0]
    total = 0.0
    for c in range(nch):
        total += q[c]
    return total, s_fin, float(np.linalg.norm(P, 2)), nch


def _compare(fz, y, what, zero_P=False):
    zr, sr = _row_form(fz, y)
    q_row = float(np.sum(np.bincount(np.arange(len(zr)) % L, weights=zr * zr, minlength=L)))
    smax = np.max(np.abs(sr))
    qs, ss = _block_form(fz, y, True)
    seq = (abs(qs - q_row) / q_row, np.max(np.abs(ss - sr)) / smax)
    qc, sc, normP, nch = _chunked_form(fz, y, zero_P=zero_P)
    got = (abs(qc - q_row) / q_row, np.max(np.abs(sc - sr)) / smax)
    print(f"{what}: {nch} chunks, |P| {normP:.3g}; sum z^2 sequential {seq[0]:.2e} chunked {got[0]:.2e}; "
          f"state sequential {seq[1]:.2e} chunked {got[1]:.2e}")
    for i, quantity in enumerate(("sum z^2", "state")):
        bound = max(FACTOR * seq[i], FLOOR)
        assert got[i] <= bound, (what, quantity, got[i], bound)


@pytest.fixture(scope="module", params=[1, 30, 31])
def fast(request):
    """J well-damped terms (tests/test_gpu_steady.py's kernels): the oracle's factor freezes within a few thousand rows."""
    J = request.param
    coeffs, t, diag, y, _ = _problem(_fast_terms(J), 12288)
    fz = _frozen(coeffs, t, diag, y)
    assert 1024 < fz["sw"] < 12288 - 3 * CHUNK - L - 1, fz["sw"]
    return J, fz, y


@pytest.mark.parametrize("tail", [CHUNK, CHUNK + 1, 3 * CHUNK + L])
def test_chunked_form_against_the_row_form(fast, tail):
    """Tails of exactly one chunk (no pass B); a chunk and a row (the last chunk is one row); three chunks and a block
    (two chunks from zero, two corrections by P)."""
    J, fz, y = fast
    _compare(fz, y[:fz["sw"] + 1 + tail], f"J = {J}, tail of {tail} rows")


@pytest.fixture(scope="module")
def flagship():
    """The benchmark's kind of series under the flagship walker's hyperparameters (seed 1000), N = 40 960."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    N = 40960
    coeffs, t, diag, y, _ = _problem(jitter_hyperparameters(solar_like_hyperparameters(30), 1000), N)
    fz = _frozen(coeffs, t, diag, y)
    assert 0 < fz["sw"] < N - 8 * CHUNK
    return fz, y


@pytest.fixture(scope="module")
def slow():
    """The slowest of the jitter seeds 1000 .. 1047 (seed 1027, switch row 54 144): three chunks, a block and a row
    behind its switch row."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    N = 54144 + 1 + 3 * CHUNK + L + 1
    coeffs, t, diag, y, _ = _problem(jitter_hyperparameters(solar_like_hyperparameters(30), 1027), N)
    fz = _frozen(coeffs, t, diag, y)
    assert fz["sw"] == 54144, fz["sw"]
    return fz, y


def test_chunked_form_on_the_headline_workload(flagship):
    fz, y = flagship
    _compare(fz, y, f"flagship walker, switch row {fz['sw']}, tail of {len(y) - fz['sw'] - 1} rows")


def test_chunked_form_on_the_slowest_walker(slow):
    fz, y = slow
    _compare(fz, y, f"slow walker, switch row {fz['sw']}, tail of {len(y) - fz['sw'] - 1} rows")


@pytest.mark.parametrize("which", ["flagship", "slow"])
def test_the_inputs_see_the_correction(which, request):
    """With P = 0 (the chunks joined without the correction) the same comparison fails: |P| is of order 1 to 100 at
    16-block chunks, so the bar tests the scan and not only the passes."""
    fz, y = request.getfixturevalue(which)
    with pytest.raises(AssertionError):
        _compare(fz, y, f"{which} walker with P = 0", zero_P=True)
