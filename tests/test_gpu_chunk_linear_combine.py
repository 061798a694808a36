"""GPU: the combines of the stored factor's sweeps through their raw C entry points -- gf_chunk_linear_combine
(k_lincombine<0>; matmul: k_chunk_decay, k_lincombine_mm), gf_chunk_linear_combine_seg (k_lincombine<1|2>,
k_lincombine_R<1|2>), gf_chunk_segment_transitions (k_segment_transition, k_transpose64) -- against the 80-bit scans of
tests/lin_ref.py.  The maps are random contractions (spectral norm 0.9) in the leading W x W of their 64 x 64 slots,
with what gf_chunk_transition leaves beyond the width (ones on the diagonal W <= j < 4 ceil(W / 4), zeros elsewhere:
include/gadfly_hip.h); the local end states are random: nothing here depends on a sweep.  The two-level combine gets
the device's own Psi (gf_chunk_segment_transitions, held to the 80-bit products in its own test below).

Bar per problem: the larger of 100 x the error of the same scan in float64 and W eps gamma, gamma = max(1, largest
start state / largest local state) (maps: the largest element of the reference).  The F_state contract of
include/gadfly_hip.h is pinned by test_f_state_contract.  Measured errors: CHANGELOG.md, round 28."""
import functools

import numpy as np
import pytest
import torch

from tests import lin_cases as C
from tests import lin_dev as D
from tests import lin_ref as R

pytestmark = pytest.mark.gpu
NCH = (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 100)
RHS = (1, 2, 15, 16, 17, 63, 64, 65)
NMAX, RMAX, B = 100, 65, 3


def rhs_of(nch):
    """Every chunk count runs R = 1 and 16 (the two segment-scan kernels); nch = 5 and 33 run every R = 1 ... 65."""
    return RHS if nch in (5, 33) else (1, 16)


def seg_lens(nch):
    return sorted({1, 2, 5, max(1, nch - 1), nch, nch + 3})


@functools.lru_cache(maxsize=None)
def family(W):
    """100 maps and local end states of B = 3 problems: Phi [100][B][W][W] (contractions), loc [100][B][W][65]."""
    rng = np.random.default_rng([W, 28])
    Phi = np.array([[R.contraction(rng, W) for _ in range(B)] for _ in range(NMAX)])
    return Phi, rng.normal(size=(NMAX, B, W, RMAX))


@functools.lru_cache(maxsize=None)
def scan_ref(W, mode, nch, dtype=R.LD):
    """The start states of the first nch chunks, for as many right-hand sides as that count runs."""
    Phi, loc = family(W)
    return R.scan(mode, Phi[:nch].astype(dtype), loc[:nch, :, :, :max(rhs_of(nch))].astype(dtype))


@functools.lru_cache(maxsize=None)
def dev_family(W):
    Phi, loc = family(W)
    return (D.dev(R.pack_maps(Phi).reshape(B, NMAX, 4096)), D.dev(R.pack_states(loc).reshape(B, NMAX, 64, RMAX)))


def plain(hip, mode, W, nch, Rn, Phi, F):
    rc = hip.load().gf_chunk_linear_combine(mode, B, nch, 1, nch, W, Rn, None, None, hip.ptr(Phi), None, hip.ptr(F),
                                            None)
    hip.check(rc, "gf_chunk_linear_combine")


def segments(hip, nch, seg_len, Phi, transposes, nb=B):
    """(Psi, PhiT, PsiT) guarded device arrays of gf_chunk_segment_transitions."""
    nseg = -(-nch // seg_len)
    Psi = D.Guarded(nb * nseg * 4096)
    PhiT, PsiT = (D.Guarded(nb * nch * 4096), D.Guarded(nb * nseg * 4096)) if transposes else (None, None)
    rc = hip.load().gf_chunk_segment_transitions(nb, nch, seg_len, hip.ptr(Phi), hip.ptr(Psi.t),
                                                 hip.ptr(PhiT.t) if transposes else None,
                                                 hip.ptr(PsiT.t) if transposes else None, None)
    hip.check(rc, "gf_chunk_segment_transitions")
    return Psi, PhiT, PsiT


def two_level(hip, mode, nch, seg_len, Rn, Phi, seg, F):
    Psi, PhiT, PsiT = seg
    nseg = -(-nch // seg_len)
    V = D.Guarded(B * nseg * 64 * Rn, float("nan"))
    p = hip.ptr
    rc = hip.load().gf_chunk_linear_combine_seg(mode, B, nch, seg_len, Rn, p(Phi), p(Psi.t),
                                                None if PhiT is None else p(PhiT.t),
                                                None if PsiT is None else p(PsiT.t), p(F), p(V.t), None)
    hip.check(rc, "gf_chunk_linear_combine_seg")
    torch.cuda.synchronize()
    V.host()


@pytest.mark.parametrize("mode", [R.LOWER, R.UPPER])
@pytest.mark.parametrize("W", [13, 63])
def test_plain_and_two_level_combine(hip, W, mode):
    """nch = 1 ... 9, 31, 32, 33, 100 (k_lincombine's unroll by four with three chunks prefetched: every remainder,
    every prefetch that runs off the end), seg_len = 1, 2, 5, nch - 1, nch, nch + 3 (one chunk per segment, a ragged
    last segment, one segment), with and without the transposes, B = 3.  Every chunk count runs R = 1 and 16 (the two
    segment-scan kernels); nch = 5 and 33 run every R = 1 ... 65 (ragged tiles of k_lincombine_R, a second tile)."""
    worst = C.Worst()
    Phi_all, loc_all = dev_family(W)
    _, loc_h = family(W)
    for nch in NCH:
        Phi = Phi_all[:, :nch].contiguous()
        segs = {(sl, tr): segments(hip, nch, sl, Phi, tr) for sl in seg_lens(nch) for tr in (False, True)}
        ref, ref64 = scan_ref(W, mode, nch), scan_ref(W, mode, nch, np.float64)
        for Rn in rhs_of(nch):
            loc = loc_all[:, :nch, :, :Rn].contiguous().reshape(-1)
            want, want64 = ref[..., :Rn], ref64[..., :Rn]
            gam = [max(1.0, float(np.max(np.abs(want[:, b])) / np.max(np.abs(loc_h[:nch, b, :, :Rn]))))
                   for b in range(B)]

            def run(call, what):
                F = D.Guarded(B * nch * 64 * Rn)
                F.t.copy_(loc)
                call(F.t)
                torch.cuda.synchronize()
                lead, rest = R.unpack_states(F.host(), B, nch, W, Rn)
                assert not rest.any(), ("a state row beyond W holds a number", what)
                D.judge(worst, what[0], what[1:], lead, want, want64, 1, W, gam)
                return lead

            got = run(lambda F: plain(hip, mode, W, nch, Rn, Phi, F), ("plain", nch, Rn))
            e64 = D.errors(want64, want, 1)
            for (sl, tr), seg in segs.items():
                two = run(lambda F: two_level(hip, mode, nch, sl, Rn, Phi, seg, F),
                          ("two-level" + (", transposes" if tr else ""), nch, sl, Rn))
                apart = D.errors(two, got, 1)
                for b in range(B):       # against each other: within the two bars
                    worst.add("two-level against plain", (nch, sl, Rn, tr, b), float(apart[b]),
                              2 * C.bar(float(e64[b]), W, gam[b]))
    worst.report(f"W = {W}, mode {mode}")


@pytest.mark.parametrize("W", [1, 13, 60, 63])
def test_segment_transitions(hip, W):
    """Psi_s = Phi_{e-1} ... Phi_b against the 80-bit products, nch = 1, 7, 33, every seg_len; beyond the width Psi
    keeps what the Phi slots hold there, to the bit; the transposes are exact transposes; one transpose output
    without the other is refused."""
    worst = C.Worst()
    Phi_h, _ = family(W)
    Phi_all, _ = dev_family(W)
    tail = R.pack_maps(np.zeros((1, 1, W, W)))[0]
    for nch in (1, 7, 33):
        Phi = Phi_all[:, :nch].contiguous()
        for sl in seg_lens(nch):
            nseg = -(-nch // sl)
            Psi, PhiT, PsiT = segments(hip, nch, sl, Phi, True)
            torch.cuda.synchronize()
            P = R.unpack_maps(Psi.host(), B, nseg)
            ref = R.segment_transitions(Phi_h[:nch].astype(R.LD), sl)
            ref64 = R.segment_transitions(Phi_h[:nch], sl)
            D.judge(worst, "Psi", (nch, sl), P[:, :, :W, :W], ref, ref64, 1, W,
                    [max(1.0, float(np.max(np.abs(ref[:, b])))) for b in range(B)])
            full = Psi.host().reshape(B * nseg, 4096).copy()
            full.reshape(-1, 64, 64)[:, :W, :W] = 0.0
            assert np.array_equal(full, np.broadcast_to(tail, full.shape)), ("beyond the width", nch, sl)
            assert np.array_equal(R.unpack_maps(PsiT.host(), B, nseg), P.transpose(0, 1, 3, 2)), (nch, sl)
            assert np.array_equal(R.unpack_maps(PhiT.host(), B, nch),
                                  R.unpack_maps(Phi.cpu().numpy(), B, nch).transpose(0, 1, 3, 2)), (nch, sl)
            alone = segments(hip, nch, sl, Phi, False)[0]
            torch.cuda.synchronize()
            assert np.array_equal(alone.host(), Psi.host()), "Psi depends on the transposes being asked for"
    worst.report(f"W = {W}")
    lib, p = hip.load(), hip.ptr
    Phi = Phi_all[:, :7].contiguous()
    out = [D.Guarded(B * 7 * 4096) for _ in range(3)]
    for kw in (dict(PhiT=None), dict(PsiT=None), dict(Phi=None), dict(Psi=None), dict(nb=0), dict(nch=0), dict(sl=0)):
        a = dict(nb=B, nch=7, sl=2, Phi=Phi, Psi=out[0].t, PhiT=out[1].t, PsiT=out[2].t)
        a.update(kw)
        rc = lib.gf_chunk_segment_transitions(a["nb"], a["nch"], a["sl"], p(a["Phi"]), p(a["Psi"]), p(a["PhiT"]),
                                              p(a["PsiT"]), None)
        assert rc != 0 and hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(np.all(o.host() == D.SENTINEL) for o in out)


@pytest.mark.parametrize("W", [1, 13, 63])
def test_matmul_combine(hip, W):
    """GF_MATMUL_LOWER: k_chunk_decay's D = exp(-c sum of the chunk's spans > 0) against the reference (spans of
    exactly 0 and the markers -1 add nothing; ones beyond W), the diagonal scan against the reference and, to the bit,
    against gf_chunk_diag_scan on the same D.  Chunks of 64 and 16 rows (6 and 21 chunks, ragged ends) and 100
    chunks of 3 rows (k_lincombine_mm splits more than 64 chunks over its segments); R = 1, 15, 16, 17, 64."""
    worst = C.Worst()
    lib, p = hip.load(), hip.ptr
    for N, L in ((333, 64), (333, 16), (300, 3)):
        cs = C.case(W, N, L, block=16, resets=(5, 6, 70), key=5)
        rows = C.rows_of(cs)
        dr = D.DevRows(rows)
        nch = D.nchunks(N, L)
        Dref, Dref64 = R.chunk_decay(rows, L), R.chunk_decay(rows, L, np.float64)
        rng = np.random.default_rng([W, N, L])
        loc_h = rng.normal(size=(nch, B, W, 64))
        for Rn in (1, 15, 16, 17, 64):
            loc = R.pack_states(loc_h[..., :Rn])
            F, Dw = D.Guarded(B * nch * 64 * Rn, loc), D.Guarded(B * nch * 64)
            rc = lib.gf_chunk_linear_combine(R.MATMUL, B, N, L, nch, W, Rn, p(dr.c), p(dr.de), None, p(Dw.t), p(F.t),
                                             None)
            hip.check(rc, "gf_chunk_linear_combine")
            torch.cuda.synchronize()
            Dd = Dw.host().reshape(B, nch, 64)
            assert np.all(Dd[:, :, W:] == 1.0), "D beyond the width"
            D.judge(worst, "D", (N, L, Rn), Dd[:, :, :W].transpose(1, 0, 2), Dref, Dref64, 1, W, 1.0)
            lead, rest = R.unpack_states(F.host(), B, nch, W, Rn)
            assert not rest.any()
            want = R.diag_scan(Dref, loc_h[..., :Rn].astype(R.LD))
            want64 = R.diag_scan(Dref64, loc_h[..., :Rn])
            gam = [max(1.0, float(np.max(np.abs(want[:, b])) / np.max(np.abs(loc_h[:, b, :, :Rn])))) for b in range(B)]
            D.judge(worst, "diagonal scan", (N, L, Rn), lead, want, want64, 1, W, gam)
            F2 = D.Guarded(B * nch * 64 * Rn, loc)
            hip.check(lib.gf_chunk_diag_scan(B, nch, 64, Rn, p(Dw.t), p(F2.t), None), "gf_chunk_diag_scan")
            torch.cuda.synchronize()
            assert np.array_equal(F2.host(), F.host()), ("gf_chunk_diag_scan on the same D", N, L, Rn)
    worst.report(f"W = {W}")


@pytest.mark.parametrize("W", [1, 13, 60, 61, 63])
def test_f_state_contract(hip, W):
    """include/gadfly_hip.h, gf_chunk_linear: what F_state must hold before the local pass.  The local pass writes the
    state rows i < ROWS = 4 ceil(W / 4) of every slot (all 64 for R = 1; 16 ceil(W / 16) for GF_MATMUL_LOWER with
    R >= 16) and the solves' combines multiply all 64 rows of every slot by the rows of Phi, so 0 x NaN reaches every
    start state: for the solves with R > 1 the caller zeroes the rows ROWS .. 63 of every slot; everything else may
    hold anything.  Pinned both ways: NaN everywhere gives the bits of a zeroed F_state where the header asks for
    nothing, NaN in Z where it asks for zeros; NaN in the rows below ROWS and zeros from ROWS on always gives the bits
    of a zeroed F_state.  Plain and two-level combine (seg_len = 2)."""
    cs = C.width_case(W)
    _, N, L, _ = cs
    nch, rows_w = D.nchunks(N, L), R.rows_of_width(W)
    dr = D.DevRows(C.rows_of(cs))
    Phi = D.dev(R.pack_maps(C.map_ref(cs, np.float64)[0]))
    seg = segments(hip, nch, 2, Phi, False)
    lib, p = hip.load(), hip.ptr
    for mode in C.MODES:
        for Rn in (1, 3, 16):
            Y = D.dev(R.rhs(W, N, Rn))

            def run(fill, two):
                F = D.Guarded(B * nch * 64 * Rn, fill)
                D.linear(hip, mode, dr, L, Rn, 1, 0, Y, Y, F.t)
                if mode == R.MATMUL:
                    Dw = D.Guarded(B * nch * 64)
                    rc = lib.gf_chunk_linear_combine(mode, B, N, L, nch, W, Rn, p(dr.c), p(dr.de), None, p(Dw.t),
                                                     p(F.t), None)
                    hip.check(rc, "gf_chunk_linear_combine")
                elif two:
                    two_level(hip, mode, nch, 2, Rn, Phi, seg, F.t)
                else:
                    plain(hip, mode, W, nch, Rn, Phi, F.t)
                Z = D.Guarded(B * N * Rn)
                D.linear(hip, mode, dr, L, Rn, 1, 1, Y, Z.t, F.t)
                return Z.host(), F.host().reshape(B * nch, 64, Rn)[:, :W]

            contract = np.full((B * nch, 64, Rn), np.nan)
            contract[:, rows_w:] = 0.0
            for two in ((False,) if mode == R.MATMUL else (False, True)):
                Z0, F0 = run(0.0, two)
                assert np.all(np.isfinite(Z0))
                Zc, Fc = run(contract, two)
                assert np.array_equal(Zc, Z0) and np.array_equal(Fc, F0), ("contract", mode, Rn, two)
                Zn, Fn = run(float("nan"), two)
                needs_zeros = mode != R.MATMUL and Rn > 1 and rows_w < 64
                if needs_zeros:
                    assert np.any(np.isnan(Zn)), ("the header asks for zeros that nothing needs", mode, Rn, two)
                else:
                    assert np.array_equal(Zn, Z0) and np.array_equal(Fn, F0), ("NaN everywhere", mode, Rn, two)
