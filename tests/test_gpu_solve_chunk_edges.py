"""GPU: chunk mode of the general-width sweeps -- gf_solve_chunk (k_solve_vec with a (problem, chunk) grid),
gf_solve_chunk_rhs (k_solve_rhs) and gf_chunk_diag_scan -- through the raw C entry points with B = 2 problems of
different coefficients, at chunk lengths that leave a last chunk of one row, a full one and a single chunk.  The true
start state of every chunk comes from the float64 oracle's sequential sweep (tests/sweep_cases.true_chunk_states); the
bar is 1e-10 of the largest reference entry."""
import numpy as np
import pytest
import torch

from tests import sweep_cases as sc
from tests.sweep_dev import SENTINEL, Factor, dev, sentinel, solve, solve_chunk, take

pytestmark = pytest.mark.gpu

WIDTHS = (17, 64, 65, 128, 193, 256)
N = 70
CHUNK_LENS = (1, 7, 8, 9, 35, 69, 70)
B = 2


def _factor(W):
    return Factor(sc.reference(*sc.structure_of(W), N, B))


def _true_states(mode, fac, Y, scaled, L):
    """(Z (B, N, R), start, end (B, nch, W, R)) of the oracle."""
    Z, start, end = [], [], []
    for b, ref in enumerate(fac.refs):
        Zb = sc.sweep_reference(mode, ref, Y[b], scaled).reshape(N, -1)
        s, e = sc.true_chunk_states(mode, ref, sc.carried_input(mode, ref, Y[b], scaled), Zb, L)
        Z.append(Zb), start.append(s), end.append(e)
    return np.array(Z), np.array(start), np.array(end)


@pytest.mark.parametrize("R", [1, 2, 65])
@pytest.mark.parametrize("W", WIDTHS)
def test_solves_from_the_true_start_states(hip, W, R):
    """GF_SOLVE_LOWER and GF_SOLVE_UPPER, with and without the scale; R = 1 is gf_solve_chunk, R = 2 and 65 (a second,
    one-lane tile of right-hand sides) gf_solve_chunk_rhs.  store = 1 from the true start states gives the oracle's Z;
    store = 0 from the same states leaves in every slot the true start state of the next chunk in sweep direction and
    writes no Z row."""
    fac = _factor(W)
    Y = np.stack([sc.rhs(N, R, seed=10 + b) for b in range(B)])
    worst, bad = dict(Z=0.0, state=0.0), []
    for mode in (sc.LOWER, sc.UPPER):
        for scaled in (False, True):
            for L in CHUNK_LENS:
                Zref, start, end = _true_states(mode, fac, Y, scaled, L)
                Z, _ = solve_chunk(hip, mode, fac, Y, scaled, L, start, 1, multi=R > 1)
                Zn, left = solve_chunk(hip, mode, fac, Y, scaled, L, start, 0, multi=R > 1)
                assert np.all(Zn == SENTINEL), (mode, scaled, L)
                for b in range(B):
                    ez, es = sc.relerr(Z[b], Zref[b]), sc.relerr(left[b], end[b])
                    worst["Z"], worst["state"] = max(worst["Z"], ez), max(worst["state"], es)
                    if not (ez <= sc.TOL and es <= sc.TOL):
                        bad.append((mode, scaled, L, b, ez, es))
    print(f"gf_solve_chunk{'_rhs' if R > 1 else ''} W = {W}, R = {R}: Z {worst['Z']:.1e}, states {worst['state']:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("R", [1, 2, 64])
@pytest.mark.parametrize("W", WIDTHS)
def test_matmul_lower_protocol_on_the_device(hip, W, R):
    """GF_MATMUL_LOWER: local pass from zero states (store = 0), gf_chunk_diag_scan with D = the product of each
    chunk's propagator rows, final pass (store = 1): Z equals the oracle at 1e-10, and unchunked gf_solve at twice
    that; the scanned states are the true start states."""
    lib, p = hip.load(), hip.ptr
    fac = _factor(W)
    ld = fac.ld
    Y = np.stack([sc.rhs(N, R, seed=20 + b) for b in range(B)])
    Yd = dev(Y)
    worst, bad = dict(Z=0.0, state=0.0), []
    for scaled in (False, True):
        whole = solve(hip, sc.MATMUL, fac, Y, scaled)
        sd = p(fac.d) if scaled else None
        for L in CHUNK_LENS:
            Zref, start, _ = _true_states(sc.MATMUL, fac, Y, scaled, L)
            nch = start.shape[1]
            D = dev(np.stack([sc.pad(sc.chunk_decays(ref, L), ld, 1.0) for ref in fac.refs]))      # (B, nch, ld)
            F = sentinel((B * nch + 1) * ld * R)
            F[:B * nch * ld * R] = 0.0
            Z = sentinel((B + 1) * N * R)

            def sweep(store):
                if R > 1:
                    rc = lib.gf_solve_chunk_rhs(sc.MATMUL, B, N, L, nch, W, ld, R, p(fac.U), p(fac.Wm), p(fac.P), sd,
                                                p(Yd), p(Z), p(F), store, None)
                else:
                    rc = lib.gf_solve_chunk(sc.MATMUL, B, N, L, nch, W, ld, p(fac.U), p(fac.Wm), p(fac.P), sd, p(Yd),
                                            p(Z), p(F), store, None)
                hip.check(rc, "gf_solve_chunk")

            sweep(0)
            torch.cuda.synchronize()
            assert bool(torch.all(Z == SENTINEL))
            hip.check(lib.gf_chunk_diag_scan(B, nch, ld, R, p(D), p(F), None), "gf_chunk_diag_scan")
            torch.cuda.synchronize()
            states = take(F, B * nch * ld * R, "F_state").reshape(B, nch, ld, R)
            sweep(1)
            torch.cuda.synchronize()
            Zh = take(Z, B * N * R, "Z").reshape(B, N, R)
            assert not np.any(states[:, :, W:])
            for b in range(B):
                ez = max(sc.relerr(Zh[b], Zref[b]), 0.5 * sc.relerr(Zh[b], whole[b]))
                es = sc.relerr(states[b, :, :W], start[b]) if nch > 1 else float(np.max(np.abs(states[b])))
                worst["Z"], worst["state"] = max(worst["Z"], ez), max(worst["state"], es)
                if not (ez <= sc.TOL and es <= sc.TOL):
                    bad.append((scaled, L, b, ez, es))
    print(f"matmul_lower in chunks W = {W}, R = {R}: Z {worst['Z']:.1e}, states {worst['state']:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("rows", [1, 17, 256])
def test_chunk_diag_scan_against_numpy(hip, rows):
    """R in {1, 16, 17, 64} (a tile of 16 right-hand sides full, one over, four tiles) and 1 to 130 chunks (64
    segments of one chunk, of up to three with empty ones at the end), B = 2."""
    lib, p = hip.load(), hip.ptr
    worst = 0.0
    for R in (1, 16, 17, 64):
        for nch in (1, 2, 9, 64, 65, 130):
            rng = np.random.default_rng([rows, R, nch])
            D = rng.uniform(0.2, 1.0, (B, nch, rows))
            loc = rng.normal(size=(B, nch, rows, R))
            F = sentinel((B * nch + 1) * rows * R)
            F[:B * nch * rows * R] = dev(loc).reshape(-1)
            hip.check(lib.gf_chunk_diag_scan(B, nch, rows, R, p(dev(D)), p(F), None), "gf_chunk_diag_scan")
            torch.cuda.synchronize()
            got = take(F, B * nch * rows * R, "F_state").reshape(B, nch, rows, R)
            for b in range(B):
                want = sc.diag_scan(D[b], loc[b])
                assert not np.any(got[b, 0])
                err = sc.relerr(got[b], want) if nch > 1 else 0.0
                worst = max(worst, err)
                assert err <= sc.TOL, (R, nch, b, err)
    print(f"gf_chunk_diag_scan rows = {rows}: worst {worst:.1e}")


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    fac = _factor(17)
    R = 2
    Y = dev(np.stack([sc.rhs(N, R) for _ in range(B)]))
    nmax = 12
    Z, F = sentinel(B * N * R), sentinel(B * nmax * fac.ld * R)

    def chunk(L, nch, multi):
        if multi:
            return lib.gf_solve_chunk_rhs(sc.LOWER, B, N, L, nch, fac.W, fac.ld, R, p(fac.U), p(fac.Wm), p(fac.P),
                                          None, p(Y), p(Z), p(F), 1, None)
        return lib.gf_solve_chunk(sc.LOWER, B, N, L, nch, fac.W, fac.ld, p(fac.U), p(fac.Wm), p(fac.P), None, p(Y),
                                  p(Z), p(F), 1, None)

    for multi in (False, True):
        for L, nch in ((7, 9), (9, 7), (7, 11), (10, 8), (0, 1), (70, 0)):      # too few rows covered; an empty chunk
            assert chunk(L, nch, multi) < 0 and "chunking" in hip.last_error(), (L, nch, multi)
    D = sentinel(B * nmax * fac.ld)
    assert lib.gf_chunk_diag_scan(B, nmax, fac.ld, 65, p(D), p(F), None) < 0 and hip.last_error()
    # B * nch > 65535 in the multi-right-hand-side form: 65536 problems of one row and one chunk, buffers of full size
    Bm, ld = 65536, 16
    big = [torch.ones(Bm * ld, dtype=torch.float64, device="cuda") for _ in range(3)]
    Yb, Zb, Fb = (torch.ones(Bm * R, dtype=torch.float64, device="cuda"), sentinel(Bm * R), sentinel(Bm * ld * R))
    rc = lib.gf_solve_chunk_rhs(sc.LOWER, Bm, 1, 1, 1, 1, ld, R, p(big[0]), p(big[1]), p(big[2]), None, p(Yb), p(Zb),
                                p(Fb), 1, None)
    assert rc < 0 and "65535" in hip.last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.all(x == SENTINEL)) for x in (Z, F, D, Zb, Fb))
