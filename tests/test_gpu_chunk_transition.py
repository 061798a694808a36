"""GPU: gf_chunk_transition (k_phi<ROWS>, k_phi7<ROWS>) and gf_scaled_propagator through their raw C entry points
against tests/lin_ref.py in 80 bits, then the whole chain of a stored factor's sweep -- local pass, the device's Phi,
combine (plain and two-level), final pass -- against the sequential 80-bit sweep, on synthetic rows and on the rows of
real factors (engine.ScaledFactor).

Bar per problem: the larger of 100 x the error of the same recurrence in float64 and W eps gamma; gamma = the largest
element of the reference (maps) or max(1, max |Z_ref| / max |input|) (sweeps).  Measured errors: CHANGELOG.md,
round 28."""
import functools

import numpy as np
import pytest
import torch

from tests import grad_cases as gc
from tests import lin_cases as C
from tests import lin_dev as D
from tests import lin_ref as R

pytestmark = pytest.mark.gpu
AUTO, COLUMN, TILED = 0, 1, 2
NAN = float("nan")


def structure(W):
    """(Jr, Jc) with Jr + 2 Jc = W: one real term for odd widths (column sweep only), complex terms otherwise."""
    return W % 2, W // 2


def padded(x, n, tail):
    a = np.full((n + D.TAIL,) + x.shape[2:], tail)
    a[:n] = x.reshape((n,) + x.shape[2:])
    return D.dev(a)


def transition(hip, cs, variant, first=0, count=None, tail=None, bad=(), fill=NAN):
    """gf_chunk_transition on a case: (Phi [B * nch][4096], G, m [B * nch][64]) on the host, pre-filled with ``fill``;
    row arrays padded by eight rows of zeros (d: ones), or of ``tail``."""
    W, N, L, _ = cs
    rows = C.rows_of(cs)
    B, nch = rows["c"].shape[0], D.nchunks(N, L)
    count = nch if count is None else count
    dr = D.DevRows(rows, tail=tail)
    r, dbar, zbar = C.map_inputs(cs, bad)
    rd = padded(r, B * N, 0.0 if tail is None else tail)
    dd = padded(dbar, B * N, 1.0 if tail is None else tail)
    zd = padded(zbar, B * N, 1.0 if tail is None else tail)
    Phi, G, m = D.Guarded(B * nch * 4096, fill), D.Guarded(B * nch * 4096, fill), D.Guarded(B * nch * 64, fill)
    Jr, Jc = structure(W)
    p = hip.ptr
    rc = hip.load().gf_chunk_transition(B, N, L, nch, first, count, Jr, Jc, variant, p(dr.c), p(dr.de), p(dd), p(zd),
                                        p(rd), p(dr.Ut), p(Phi.t), p(G.t), p(m.t), None)
    hip.check(rc, "gf_chunk_transition")
    torch.cuda.synchronize()
    return Phi.host().reshape(B * nch, 4096), G.host().reshape(B * nch, 4096), m.host().reshape(B * nch, 64)


def check_maps(worst, what, cs, got, bad=()):
    """Phi, G, m of every chunk against the reference; beyond the width: Phi holds ones on the diagonal
    W <= j < ROWS = 4 ceil(W / 4) and zeros elsewhere, G and m zeros (include/gadfly_hip.h)."""
    W, N, L, _ = cs
    B, nch = 3, D.nchunks(N, L)
    ref, ref64 = C.map_ref(cs, R.LD, bad), C.map_ref(cs, np.float64, bad)
    Phi, G, m = got
    tail = R.pack_maps(np.zeros((1, 1, W, W)))[0]
    for name, slots, k in (("Phi", Phi, 0), ("G", G, 1)):
        full = R.unpack_maps(slots, B, nch)
        gam = [max(1.0, float(np.max(np.abs(ref[k][:, b])))) for b in range(B)]
        D.judge(worst, name, what, full[:, :, :W, :W], ref[k], ref64[k], 1, W, gam)
        out = slots.reshape(-1, 64, 64).copy()
        out[:, :W, :W] = 0.0
        want = tail if name == "Phi" else np.zeros(4096)
        assert np.array_equal(out.reshape(-1, 4096), np.broadcast_to(want, (B * nch, 4096))), (name, "beyond W", what)
    assert np.array_equal(G.reshape(-1, 64, 64), G.reshape(-1, 64, 64).transpose(0, 2, 1)), ("G not symmetric", what)
    assert not m[:, W:].any(), ("m beyond W", what)
    gam = [max(1.0, float(np.max(np.abs(ref[2][:, b])))) for b in range(B)]
    D.judge(worst, "m", what, m.reshape(B, nch, 64)[:, :, :W].transpose(1, 0, 2), ref[2], ref64[2], 1, W, gam)


@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_every_width(hip, cls):
    """W = 1 ... 63 with GF_SWEEP_COLUMN (k_phi<ROWS>; Jr = W mod 2), every even W also with GF_SWEEP_TILED and
    GF_SWEEP_AUTO (k_phi7<ROWS>); B = 3, N = 333 in chunks of 64; r = w~ d, dbar = d, zbar random."""
    worst = C.Worst()
    for W in C.CLASSES[cls]:
        cs = C.width_case(W)
        col = transition(hip, cs, COLUMN)
        check_maps(worst, (W, "column"), cs, col)
        if W % 2 == 0:
            for v, name in ((TILED, "tiled"), (AUTO, "auto")):
                got = transition(hip, cs, v)
                check_maps(worst, (W, name), cs, got)
            assert all(np.array_equal(a, b) for a, b in zip(got, transition(hip, cs, TILED))), "auto is not tiled"
    worst.report(f"widths {cls}")


@pytest.mark.parametrize("W", C.TRANSITION_WIDTHS)
def test_chunkings_resets_and_rows_without_a_pivot(hip, W):
    """One chunk of N = 1 ... 65 rows, chunks of 128, a ragged last chunk of one row, reset rows at every offset of a
    16-row block / in a row / on a chunk's first and last row; then rows with dbar <= 0 (0 and -1.5): they add nothing
    to G, m and the pending update."""
    worst = C.Worst()
    variants = (COLUMN,) if W % 2 else (COLUMN, TILED)
    for cs in C.transition_cases(W):
        for v in variants:
            check_maps(worst, (cs[1], cs[2], v), cs, transition(hip, cs, v))
    cs = C.width_case(W)
    for v in variants:
        check_maps(worst, ("rows without a pivot", v), cs, transition(hip, cs, v, bad=C.BAD_ROWS), C.BAD_ROWS)
    worst.report(f"W = {W}")


@pytest.mark.parametrize("W", C.TRANSITION_WIDTHS)
def test_chunk_ranges_and_padding_rows(hip, W):
    """Only the chunks of the range are written (the others keep their NaN), with the bits of the full call; the
    eight rows the sweep fetches past the end of its row arrays hold zeros (d = 1) or NaN: identical bits."""
    cs = C.width_case(W)
    nch = 6
    for v in (COLUMN,) if W % 2 else (COLUMN, TILED):
        full = transition(hip, cs, v)
        for first, count in ((1, nch - 2), (0, nch), (2, 1), (nch - 1, 1), (0, 0)):
            got = transition(hip, cs, v, first, count)
            inside = np.zeros((3, nch), dtype=bool)
            inside[:, first:first + count] = True
            for a, b in zip(got, full):
                assert np.array_equal(a[inside.reshape(-1)], b[inside.reshape(-1)]), (v, first, count)
                assert np.all(np.isnan(a[~inside.reshape(-1)])), (v, first, count)
        nan_tail = transition(hip, cs, v, tail=NAN)
        assert all(np.array_equal(a, b) for a, b in zip(nan_tail, full)), ("NaN in the padding rows", v)


def test_transition_refusals(hip):
    lib, p = hip.load(), hip.ptr
    cs = C.width_case(34)
    dr = D.DevRows(C.rows_of(cs))
    out = [D.Guarded(3 * 6 * 4096), D.Guarded(3 * 6 * 4096), D.Guarded(3 * 6 * 64)]
    base = dict(B=3, N=333, L=64, nch=6, first=0, count=6, Jr=0, Jc=17, v=TILED, c=dr.c, de=dr.de, d=dr.d, z=dr.d,
                r=dr.Wt, Ut=dr.Ut, Phi=out[0].t, G=out[1].t, m=out[2].t)
    bad = [dict(B=0), dict(N=0), dict(Jc=0), dict(Jr=2, Jc=31), dict(L=32), dict(L=96, nch=4), dict(nch=5),
           dict(nch=7), dict(first=-1), dict(count=-1), dict(first=3, count=4), dict(v=3), dict(Jr=2, Jc=16, v=TILED)]
    bad += [{k: None} for k in ("c", "de", "d", "z", "r", "Ut", "Phi", "G", "m")]
    for kw in bad:
        a = dict(base, **kw)
        rc = lib.gf_chunk_transition(a["B"], a["N"], a["L"], a["nch"], a["first"], a["count"], a["Jr"], a["Jc"], a["v"],
                                     p(a["c"]), p(a["de"]), p(a["d"]), p(a["z"]), p(a["r"]), p(a["Ut"]), p(a["Phi"]),
                                     p(a["G"]), p(a["m"]), None)
        assert rc != 0 and hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(np.all(o.host() == D.SENTINEL) for o in out)


@pytest.mark.parametrize("W,ld", [(1, 2), (63, 64), (64, 96), (172, 192)])
def test_scaled_propagator(hip, W, ld):
    """P [B][N][ld]: ones off the reset rows, exp(-c_j de) on them (de = 0: ones), ones in the columns >= W; the
    guards around P stay; refused arguments."""
    lib, p = hip.load(), hip.ptr
    B, N = 2, 70
    rng = np.random.default_rng([W, ld])
    c = rng.uniform(0.01, 2.0, (B, W))
    de = np.full((B, N), -1.0)
    at = np.arange(0, N, 7)
    de[:, at] = rng.uniform(0.0, 1.0, (B, len(at)))
    de[:, at[1::3]] = 0.0
    cd, ded = D.dev(c), D.dev(de)
    P = D.Guarded(B * N * ld)
    hip.check(lib.gf_scaled_propagator(B, N, W, ld, p(cd), p(ded), p(P.t), None), "gf_scaled_propagator")
    torch.cuda.synchronize()
    got = P.host().reshape(B, N, ld)
    assert np.all(got[:, :, W:] == 1.0) and np.all(got[de <= 0.0] == 1.0)

    def ref(dtype):
        e = np.exp(-c.astype(dtype)[:, None, :] * np.maximum(de, 0.0).astype(dtype)[:, :, None])
        return np.where((de >= 0)[:, :, None], e, dtype(1.0))

    worst = C.Worst()
    D.judge(worst, "P", (W, ld), got[:, :, :W], ref(R.LD), ref(np.float64), 0, W, 1.0)
    worst.report(f"W = {W}")
    for kw in (dict(B=0), dict(N=0), dict(W=0), dict(ld=W - 1), dict(c=None), dict(de=None), dict(P=None)):
        a = dict(dict(B=B, N=N, W=W, ld=ld, c=cd, de=ded, P=P.t), **kw)
        rc = lib.gf_scaled_propagator(a["B"], a["N"], a["W"], a["ld"], p(a["c"]), p(a["de"]), p(a["P"]), None)
        assert rc != 0, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert np.array_equal(P.host().reshape(B, N, ld), got)


@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_chain(hip, cls):
    """Local pass -> Phi from gf_chunk_transition, called as ScaledFactor._ensure_transitions calls it (r = w~ d,
    dbar = zbar = d, every chunk; column sweep for odd widths, the tiled one for even) -> combine, plain and two-level
    (seg_len = 2; matmul: its diagonal combine) -> final pass, against the sequential 80-bit sweep: every
    W = 1 ... 63, the three modes, R = 1, 3, 16, input scaling on; F_state zeroed as the header asks."""
    worst = C.Worst()
    lib, p = hip.load(), hip.ptr
    B = 3
    for W in C.CLASSES[cls]:
        cs = C.width_case(W)
        _, N, L, _ = cs
        nch = D.nchunks(N, L)
        rows = C.rows_of(cs)
        dr = D.DevRows(rows)
        Jr, Jc = structure(W)
        rd = padded(C.map_inputs(cs)[0], B * N, 0.0)
        Phi, G, m = (torch.empty((B * nch, n), dtype=torch.float64, device="cuda") for n in (4096, 4096, 64))
        rc = lib.gf_chunk_transition(B, N, L, nch, 0, nch, Jr, Jc, AUTO, p(dr.c), p(dr.de), p(dr.d), p(dr.d), p(rd),
                                     p(dr.Ut), p(Phi), p(G), p(m), None)
        hip.check(rc, "gf_chunk_transition")
        nseg = -(-nch // 2)
        Psi = torch.empty((B * nseg, 4096), dtype=torch.float64, device="cuda")
        hip.check(lib.gf_chunk_segment_transitions(B, nch, 2, p(Phi), p(Psi), None, None, None),
                  "gf_chunk_segment_transitions")
        for mode in C.MODES:
            ref, ref64 = C.sweep_ref(cs, mode, 40), C.sweep_ref(cs, mode, 40, np.float64)
            for Rn in (1, 3, 16):
                Y = D.dev(ref["Y"][:, :, :Rn])
                yin = R.scaled_input(mode, rows, ref["Y"][:, :, :Rn], 1, np.float64)
                gam = C.gamma(ref["Z"][1][..., :Rn], yin)
                for two in ((False,) if mode == R.MATMUL else (False, True)):
                    F = D.Guarded(B * nch * 64 * Rn, 0.0)
                    D.linear(hip, mode, dr, L, Rn, 1, 0, Y, Y, F.t)
                    if mode == R.MATMUL:
                        Dw = torch.empty((B * nch, 64), dtype=torch.float64, device="cuda")
                        rc = lib.gf_chunk_linear_combine(mode, B, N, L, nch, W, Rn, p(dr.c), p(dr.de), None, p(Dw),
                                                         p(F.t), None)
                    elif two:
                        V = torch.empty((B * nseg, 64 * Rn), dtype=torch.float64, device="cuda")
                        rc = lib.gf_chunk_linear_combine_seg(mode, B, nch, 2, Rn, p(Phi), p(Psi), None, None, p(F.t),
                                                             p(V), None)
                    else:
                        rc = lib.gf_chunk_linear_combine(mode, B, nch, 1, nch, W, Rn, None, None, p(Phi), None, p(F.t),
                                                         None)
                    hip.check(rc, "combine")
                    torch.cuda.synchronize()
                    lead, _ = R.unpack_states(F.host(), B, nch, W, Rn)      # (the final pass leaves end states there)
                    Z = D.Guarded(B * N * Rn)
                    D.linear(hip, mode, dr, L, Rn, 1, 1, Y, Z.t, F.t)
                    tag = (W, mode, Rn, "two-level" if two else "plain")
                    D.judge(worst, "start states", tag, lead, ref["starts"][1][..., :Rn], ref64["starts"][1][..., :Rn],
                            1, W, gam)
                    D.judge(worst, "Z", tag, Z.host().reshape(B, N, Rn), ref["Z"][1][..., :Rn], ref64["Z"][1][..., :Rn],
                            0, W, gam)
    worst.report(f"widths {cls}")


@functools.lru_cache(maxsize=None)
def real_reference(key, dtype):
    """lower, upper, apply_inverse and dot_tril of the rows in _REAL[key] by the sequential recurrence, R = 16."""
    rows, Y = _REAL[key]
    lower = R.sweep(R.LOWER, rows, Y.astype(dtype), dtype=dtype)[0]
    return dict(solve_lower=lower, solve_upper=R.sweep(R.UPPER, rows, Y.astype(dtype), dtype=dtype)[0],
                apply_inverse=R.sweep(R.UPPER, rows, R.scaled_input(R.UPPER, rows, lower, 1, dtype), dtype=dtype)[0],
                dot_tril=R.sweep(R.MATMUL, rows, R.scaled_input(R.MATMUL, rows, Y, 1, dtype), dtype=dtype)[0])


_REAL = {}


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (0, 6), (3, 5), (0, 31)])
def test_real_factors(hip, Jr, Jc):
    """The rows of a real stored factor (two problems of grad_cases.edge_problem, N = 1300, stored_factor(chunk_len =
    128): 11 chunks, the last of 20 rows) copied to the host: solve_lower, solve_upper, apply_inverse and dot_tril of
    engine.ScaledFactor against the sequential 80-bit recurrences ON THOSE ROWS, R = 1, 5, 16 -- the tight bar for the
    path tests/test_gpu_parity.py::test_scaled_factor_sweeps holds at 1e-6 against the factorisation's oracle.  Errors
    relative to the largest element of the reference (no floor of 1: apply_inverse returns values of 1e-4)."""
    from gadfly_amd.engine import StreamingBatch
    N, B, W = 1300, 2, Jr + 2 * Jc
    prob = gc.edge_problem(Jr, Jc, N)
    eng = StreamingBatch([gc.coefficients(prob, b) + (0.0,) for b in range(B)], prob["t"], prob["y"][0],
                         diag=prob["diag"][0])
    fac = eng.stored_factor(chunk_len=128)
    assert fac.nch == 11 and fac.chunk_len == 128
    host = lambda x, *s: x.reshape(-1, *s)[:B * N].reshape(B, N, *s).cpu().numpy().copy()      # noqa: E731
    rows = dict(c=fac.c.cpu().numpy().reshape(B, W), Ut=host(fac.Ut, 64), Wt=host(fac.Wt, 64), d=host(fac.d),
                de=host(fac.de))
    assert np.all(rows["d"] > 0) and np.all(np.isfinite(rows["Ut"][:, :, :W])) and np.any(rows["de"][:, 1:] >= 0)
    Y = np.random.default_rng([Jr, Jc]).normal(size=(B, N, 16))
    _REAL[(Jr, Jc)] = (rows, Y)
    ref, ref64 = real_reference((Jr, Jc), R.LD), real_reference((Jr, Jc), np.float64)
    worst = C.Worst()
    for name in ("solve_lower", "solve_upper", "apply_inverse", "dot_tril"):
        for Rn in (1, 5, 16):
            got = getattr(fac, name)(D.dev(Y[:, :, :Rn])).cpu().numpy()
            yin = Y[:, :, :Rn] * np.sqrt(rows["d"])[:, :, None] if name == "dot_tril" else Y[:, :, :Rn]
            D.judge(worst, name, (Rn,), got, ref[name][..., :Rn], ref64[name][..., :Rn], 0, W,
                    C.gamma(ref[name][..., :Rn], yin), floor=0.0)
    worst.report(f"(Jr, Jc) = ({Jr}, {Jc})")
