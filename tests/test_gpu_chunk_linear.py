"""GPU: gf_chunk_linear (k_lin1, k_linR7<ROWS, NODOT>, k_mmR_mfma<MT, NODOT, NWV>) through its raw C entry point, on the
synthetic stored rows of tests/lin_ref.py (pinned without the device by tests/test_lin_ref_host.py), both passes, with
the start states of the final pass taken from the 80-bit reference: the sweep kernels alone, no combine.

Error of a problem: max |device - reference| / max(1, max |reference|) over its rows (local pass: over the leading W
rows of all its F_state slots).  Its bar: the larger of 100 x the error of the same recurrence in plain float64
(tests/lin_ref.py with dtype = float64) on that problem and W eps gamma, gamma = max(1, max |Z_ref| / max |input|).

Measured on an MI355X (pytest -s prints the error closest to its bar per kind of comparison): see CHANGELOG.md,
round 28."""
import numpy as np
import pytest
import torch

from tests import lin_cases as C
from tests import lin_dev as D
from tests import lin_ref as R

pytestmark = pytest.mark.gpu
NAMES = {R.LOWER: "lower", R.UPPER: "upper", R.MATMUL: "matmul"}


def both_passes(hip, worst, cs, dr, mode, Rn, Rmax, scales=(0, 1), what=()):
    """Local pass against the zero-start end states, final pass (reference start states) against the sequential
    sweep, for R = Rn right-hand sides of the case's Rmax; layout checks: F_state rows >= W exactly zero or untouched,
    the guards around Z and F_state untouched, the local pass writes no row of Z."""
    W, N, L, _ = cs
    B, nch = dr.B, D.nchunks(N, L)
    ref, ref64 = C.sweep_ref(cs, mode, Rmax), C.sweep_ref(cs, mode, Rmax, np.float64)
    Y = D.dev(ref["Y"][:, :, :Rn])
    for s in scales:
        yin = R.scaled_input(mode, dr.host, ref["Y"][:, :, :Rn], s, np.float64)
        gam = C.gamma(ref["Z"][s][..., :Rn], yin)
        tag = what + (W, L, NAMES[mode], Rn, s)
        Z, F = D.Guarded(B * N * Rn), D.Guarded(B * nch * 64 * Rn)
        D.linear(hip, mode, dr, L, Rn, s, 0, Y, Z.t, F.t)
        assert np.all(Z.host() == D.SENTINEL), ("the local pass wrote Z", tag)
        lead, rest = R.unpack_states(F.host(), B, nch, W, Rn)
        assert np.all((rest == 0.0) | (rest == D.SENTINEL)), ("a state row beyond W holds a number", tag)
        D.judge(worst, "local " + NAMES[mode], tag, lead, ref["loc"][s][..., :Rn], ref64["loc"][s][..., :Rn], 1, W, gam)
        F = D.Guarded(B * nch * 64 * Rn, R.pack_states(ref["starts"][s][..., :Rn]))
        D.linear(hip, mode, dr, L, Rn, s, 1, Y, Z.t, F.t)
        F.host()
        got = Z.host().reshape(B, N, Rn)
        D.judge(worst, "final " + NAMES[mode], tag, got, ref["Z"][s][..., :Rn], ref64["Z"][s][..., :Rn], 0, W, gam)


@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_every_width(hip, cls):
    """W = 1 ... 63 (every ROWS = 4 ceil(W / 4) of k_linR7, every MT of k_mmR_mfma on both sides of its tiles), the
    three modes, R = 1 (k_lin1), 3 (k_linR7), 16 and 40 (matmul: k_mmR_mfma, one and two waves), B = 3 problems of
    different rows, N = 333 in chunks of 64 (the last of 13 rows), input scaling off and on."""
    worst = C.Worst()
    for W in C.CLASSES[cls]:
        cs = C.width_case(W)
        dr = D.DevRows(C.rows_of(cs))
        for mode in C.MODES:
            for Rn in (1, 3, 16, 40):
                both_passes(hip, worst, cs, dr, mode, Rn, 40)
    worst.report(f"widths {cls}")


@pytest.mark.parametrize("W", C.EDGE_WIDTHS)
def test_chunk_lengths(hip, W):
    """chunk_len = 1 ... 129 around k_lin1's ring (24) and scalar blocks (64), k_linR7's fetch-ahead (3) and
    k_mmR_mfma's blocks (16): two chunks and a ragged last one of a single row; R = 1, 3, 16, input scaling on."""
    worst = C.Worst()
    for L in C.CHUNK_LENS:
        cs = C.chunk_len_case(W, L)
        dr = D.DevRows(C.rows_of(cs))
        for mode in C.MODES:
            for Rn in (1, 3, 16):
                both_passes(hip, worst, cs, dr, mode, Rn, 16, scales=(1,))
    worst.report(f"W = {W}")


@pytest.mark.parametrize("W", [5, 33, 63])
def test_right_hand_side_counts(hip, W):
    """R = 2 ... 65: the k_linR7 / k_mmR_mfma switch (15 | 16), one and two waves (32 | 33), ragged tiles of 16 and
    32, a second tile (64 | 65); N = 150 in chunks of 64."""
    worst = C.Worst()
    cs = C.rhs_case(W)
    dr = D.DevRows(C.rows_of(cs))
    for mode in C.MODES:
        for Rn in C.RHS_COUNTS:
            both_passes(hip, worst, cs, dr, mode, Rn, 65, scales=(1,))
    worst.report(f"W = {W}")


@pytest.mark.parametrize("W", [7, 33])
def test_reset_positions(hip, W):
    """Reset rows off the grid: one at every offset 0 ... 15 of a 16-row block (k_mmR_mfma cuts the block there),
    three in a row, on the first and on the last row of a chunk, spans of exactly 0 -- and no reset at all."""
    worst = C.Worst()
    for k, cs in enumerate(C.reset_cases(W)):
        dr = D.DevRows(C.rows_of(cs))
        for mode in C.MODES:
            for Rn in (1, 3, 16, 40):
                both_passes(hip, worst, cs, dr, mode, Rn, 40, what=("resets" if k == 0 else "none",))
    worst.report(f"W = {W}")


@pytest.mark.parametrize("W", [13, 48])
def test_invariances(hip, W):
    """Z aliasing Y, a second run and every problem alone give the bits of the batch."""
    cs = C.width_case(W)
    rows = C.rows_of(cs)
    _, N, L, _ = cs
    nch = D.nchunks(N, L)
    dr = D.DevRows(rows)
    for mode in C.MODES:
        for Rn in (1, 3, 16):
            ref = C.sweep_ref(cs, mode, 40)
            Yh = ref["Y"][:, :, :Rn]
            F0 = R.pack_states(ref["starts"][1][..., :Rn]).reshape(3, nch, 64 * Rn)

            def run(d, sel, alias=False):
                B = len(sel)
                Y = D.Guarded(B * N * Rn, Yh[sel])
                loc = D.Guarded(B * nch * 64 * Rn, 0.0)
                D.linear(hip, mode, d, L, Rn, 1, 0, Y.t, Y.t, loc.t)
                assert np.array_equal(Y.host(), Yh[sel].reshape(-1)), "the local pass wrote its rows"
                F = D.Guarded(B * nch * 64 * Rn, F0[sel])
                Z = Y if alias else D.Guarded(B * N * Rn)
                D.linear(hip, mode, d, L, Rn, 1, 1, Y.t, Z.t, F.t)
                return loc.host().reshape(B, -1), Z.host().reshape(B, -1)

            loc, Z = run(dr, [0, 1, 2])
            for kw in (dict(), dict(alias=True)):
                loc2, Z2 = run(dr, [0, 1, 2], **kw)
                assert np.array_equal(loc, loc2) and np.array_equal(Z, Z2), (mode, Rn, kw)
            for b in range(3):
                loc1, Z1 = run(D.DevRows(rows, [b]), [b])
                assert np.array_equal(loc1[0], loc[b]) and np.array_equal(Z1[0], Z[b]), (mode, Rn, b)


def test_refusals_return_before_any_launch(hip):
    """mode 3, W = 0 / 64, R = 0, B = 0, N = 0, bad chunkings and null pointers: a non-zero status, a message, and no
    output touched."""
    lib, p = hip.load(), hip.ptr
    cs = C.width_case(13)
    dr = D.DevRows(C.rows_of(cs))
    N, Rn = 333, 3
    Y, Z, F = D.Guarded(3 * N * Rn), D.Guarded(3 * N * Rn), D.Guarded(3 * 6 * 64 * Rn)

    def call(mode=0, B=3, N=N, L=64, nch=6, W=13, Rn=Rn, c=dr.c, Ut=dr.Ut, Wt=dr.Wt, d=dr.d, de=dr.de, Y=Y.t, Z=Z.t,
             F=F.t):
        return lib.gf_chunk_linear(mode, B, N, L, nch, W, Rn, 1, 1, p(c), p(Ut), p(Wt), p(d), p(de), p(Y), p(Z), p(F),
                                   None)

    bad = [dict(mode=3), dict(mode=-1), dict(W=0), dict(W=64), dict(Rn=0), dict(B=0), dict(N=0), dict(L=0),
           dict(nch=0), dict(nch=5), dict(nch=7), dict(L=32), dict(L=67, nch=6)]
    bad += [{k: None} for k in ("c", "Ut", "Wt", "d", "de", "Y", "Z", "F")]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    for x in (Y, Z, F):
        assert np.all(x.host() == D.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
