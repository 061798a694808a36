"""GPU: the generic sweep kernels through their raw C entry points at every instance boundary up to W = 256
(tests/sweep_cases.py): gf_build_matrices against oracle/seq.py; gf_factor (k_factor's eight instances, one-shot and
streamed through S_state / F_state, the failing pivot) and gf_solve (k_solve_vec<1..4> in its six mode / scale forms,
k_solve_rhs's eight instances) against oracle/cref.py in float64 at 1e-10 of the largest reference entry, at every
length around the depth-8 row rings; gf_reduce_tile + gf_loglike_finish against numpy.  Every output is one problem
too long and pre-filled with a sentinel that must survive."""
import numpy as np
import pytest
import torch

from oracle import cref
from tests import grad_cases as gc
from tests import sweep_cases as sc
from tests.sweep_dev import INFO_SENTINEL, SENTINEL, Factor, dev, sentinel, solve, stack, take

pytestmark = pytest.mark.gpu

MODES = ((sc.LOWER, "solve_lower"), (sc.UPPER, "solve_upper"), (sc.MATMUL, "matmul_lower"))
# generator rows and propagators are a sincos / an exp and two products each: a few units of the last place of the
# largest entry of the row (|a| + |b| against max |U|, below 3 for these terms) -- 1e-13 leaves two orders
TOL_BUILD = 1e-13


def _ids(s):
    return f"W{s[0] + 2 * s[1]}-{s[0]}r{s[1]}c"


# ---- gf_build_matrices -----------------------------------------------------------------------------------------

def _build(hip, prob, t, t_bs, diag, diag_bs, N, n_first=0, want_a=True, want_P=True):
    """One gf_build_matrices call on the coefficients of a grad_cases.edge_problem: dict a, U, V, P (host, None where
    not asked for)."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, B = prob["Jr"], prob["Jc"], prob["B"]
    ld = sc.leading_dim(Jr + 2 * Jc)
    real, comp = dev(prob["real"]), dev(prob["comp"])       # (2, B, max(Jr, 1)), (4, B, max(Jc, 1))
    da, td = dev(prob["diag_add"]), dev(t)
    dd = None if diag is None else dev(diag)
    a = sentinel((B + 1) * N) if want_a else None
    U, V = sentinel((B + 1) * N * ld), sentinel((B + 1) * N * ld)
    P = sentinel((B + 1) * N * ld) if want_P else None
    rc = lib.gf_build_matrices(B, N, n_first, Jr, Jc, ld, p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]),
                               p(comp[3]), p(da), p(td), t_bs, p(dd), diag_bs, p(a), p(U), p(V), p(P), None)
    hip.check(rc, "gf_build_matrices")
    torch.cuda.synchronize()
    out = dict(a=None if a is None else take(a, B * N, "a").reshape(B, N))
    for k, x in (("U", U), ("V", V), ("P", P)):
        out[k] = None if x is None else take(x, B * N * ld, k).reshape(B, N, ld)
    return out


@pytest.mark.parametrize("Jr,Jc", sc.STRUCTURES, ids=[_ids(s) for s in sc.STRUCTURES])
def test_build_matrices(hip, Jr, Jc):
    """N = 9, B = 3: U, V, a, P against oracle/seq.py on a shared axis and on per-problem axes (strides 0 and N + 2),
    shared and per-problem diagonals; pad columns exactly 0 (1 for P); a, P, diag = NULL; a tile of rows 3..8 equals
    those rows of the whole-series call to the bit, its first propagator row (which needs t[2]) included."""
    N, B, W = 9, 3, Jr + 2 * Jc
    prob = gc.edge_problem(Jr, Jc, N, B)
    worst = 0.0
    for own in (False, True):
        refs = sc.reference(Jr, Jc, N, B, own_axes=own)
        if own:
            t = np.full((B, N + 2), np.nan)
            t[:, :N] = stack(refs, "t")
            t_bs = N + 2
        else:
            t, t_bs = refs[0]["t"], 0
        got = _build(hip, prob, t, t_bs, prob["diag"], N, N)
        for k, fill in (("U", 0.0), ("V", 0.0), ("P", 1.0)):
            assert np.all(got[k][:, :, W:] == fill), (k, own)
            for b in range(B):
                err = sc.relerr(got[k][b, :, :W], refs[b][k])
                worst = max(worst, err)
                assert err <= TOL_BUILD, (k, own, b, err)
        err = sc.relerr(got["a"], stack(refs, "a"))
        worst = max(worst, err)
        assert err <= TOL_BUILD, ("a", own, err)
        assert np.all(got["P"][:, 0] == 1.0)
        # a, P = NULL: U and V do not change; diag = NULL: a = diag_add alone; a shared diagonal (stride 0)
        part = _build(hip, prob, t, t_bs, prob["diag"], N, N, want_a=False, want_P=False)
        assert part["a"] is None and part["P"] is None
        assert np.array_equal(part["U"], got["U"]) and np.array_equal(part["V"], got["V"])
        null = _build(hip, prob, t, t_bs, None, 0, N)
        assert np.array_equal(null["a"], np.repeat(prob["diag_add"][:, None], N, axis=1))
        assert all(np.array_equal(null[k], got[k]) for k in ("U", "V", "P"))
        shared = _build(hip, prob, t, t_bs, prob["diag"][1], 0, N)
        assert np.array_equal(shared["a"], prob["diag"][1][None, :] + prob["diag_add"][:, None])
        # rows 3..8 as a tile
        tile = _build(hip, prob, t, t_bs, prob["diag"], N, 6, n_first=3)
        assert np.array_equal(tile["a"], got["a"][:, 3:])
        assert all(np.array_equal(tile[k], got[k][:, 3:]) for k in ("U", "V", "P"))
    print(f"gf_build_matrices W = {W} ({Jr}, {Jc}): worst {worst:.1e}")


# ---- gf_factor ---------------------------------------------------------------------------------------------------

def _factor(hip, fac, a, y, y_bs, tiles=None, want_W=True, want_z=True, stop_after=None):
    """gf_factor on the device rows of ``fac`` (U, V, P) with the host diagonal a (B, N) and right-hand side y ((N,)
    shared or (B, N); None = no forward solve): one shot, or streamed through S_state / F_state in ``tiles`` (row
    counts).  Returns dict d, W, z (host; rows a failed problem never reached hold the sentinel), info."""
    lib, p = hip.load(), hip.ptr
    B, N, W, ld = fac.B, fac.N, fac.W, fac.ld
    ad = dev(a)
    yd = None if y is None else dev(y)
    want_z = want_z and y is not None
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    info[:B] = 0
    out = dict(d=np.full((B, N), SENTINEL), W=np.full((B, N, ld), SENTINEL) if want_W else None,
               z=np.full((B, N), SENTINEL) if want_z else None)
    streamed = tiles is not None
    S = F = None
    if streamed:
        S = torch.zeros((B + 1) * int(lib.gf_state_size(W)), dtype=torch.float64, device="cuda")
        F = torch.zeros((B + 1) * int(lib.gf_state_cols(W)), dtype=torch.float64, device="cuda")
        S[B * int(lib.gf_state_size(W)):] = SENTINEL
        F[B * int(lib.gf_state_cols(W)):] = SENTINEL
    n0 = 0
    for T in (tiles if streamed else [N]):
        sl = slice(n0, n0 + T)
        at, Ut, Vt, Pt = (x[:, sl].contiguous() for x in (ad, fac.U, fac.V, fac.P))
        yp = None if yd is None else p(yd[..., n0:])
        d, z = sentinel((B + 1) * T), (sentinel((B + 1) * T) if want_z else None)
        Wm = sentinel((B + 1) * T * ld) if want_W else None
        rc = lib.gf_factor(B, T, n0, W, ld, p(at), p(Ut), p(Vt), p(Pt), yp, y_bs, p(d), p(Wm), p(z), p(S), p(F),
                           p(info), None)
        hip.check(rc, "gf_factor")
        torch.cuda.synchronize()
        out["d"][:, sl] = take(d, B * T, "d").reshape(B, T)
        if want_W:
            out["W"][:, sl] = take(Wm, B * T * ld, "W").reshape(B, T, ld)
        if want_z:
            out["z"][:, sl] = take(z, B * T, "z").reshape(B, T)
        n0 += T
    assert n0 == N
    ih = info.cpu().numpy()
    assert ih[B] == INFO_SENTINEL
    if streamed:
        assert S[-1].item() == SENTINEL and F[-1].item() == SENTINEL
    out["info"] = ih[:B]
    return out


def _tiles(N):
    """1, 8 and the remaining rows."""
    t = [1, min(8, N - 1), N - 1 - min(8, N - 1)]
    return [x for x in t if x > 0]


@pytest.mark.parametrize("Jr,Jc", sc.STRUCTURES, ids=[_ids(s) for s in sc.STRUCTURES])
def test_factor(hip, Jr, Jc):
    """N in {1, 2, 9, 70}, B = 3: d, W, z against oracle/cref.py at 1e-10; without y, without W, with a shared y;
    streamed in tiles of 1, 8 and the rest against the same bar (the hand-over folds the pending update with an FMA
    the loop does not use: no bit identity)."""
    W, B = Jr + 2 * Jc, 3
    worst = dict(d=0.0, W=0.0, z=0.0)
    bad = []

    def compare(tag, N, got, refs, zref):
        assert np.all(got["info"] == 0), (tag, N, got["info"])
        errs = dict(d=sc.relerr(got["d"], stack(refs, "d")))
        if got["W"] is not None:
            assert not np.any(got["W"][:, :, W:]), (tag, N)
            errs["W"] = max(sc.relerr(got["W"][b, :, :W], refs[b]["W"]) for b in range(B))
        if got["z"] is not None:
            errs["z"] = max(sc.relerr(got["z"][b], zref[b]) for b in range(B))
        for k, e in errs.items():
            worst[k] = max(worst[k], e)
            if not e <= sc.TOL:
                bad.append((tag, N, k, e))

    for N in (1, 2, 9, 70):
        refs = sc.reference(Jr, Jc, N, B)
        fac = Factor(refs)
        a, y, z = stack(refs, "a"), stack(refs, "y"), stack(refs, "z")
        base = _factor(hip, fac, a, y, N)
        compare("one-shot", N, base, refs, z)
        noy = _factor(hip, fac, a, None, 0)
        assert noy["z"] is None and np.array_equal(noy["d"], base["d"]) and np.array_equal(noy["W"], base["W"])
        now = _factor(hip, fac, a, y, N, want_W=False)
        assert now["W"] is None and np.array_equal(now["d"], base["d"]) and np.array_equal(now["z"], base["z"])
        zs = [cref.solve_lower(r["t"], r["c"], r["U"], r["W"], y[1]) for r in refs]
        compare("shared y", N, _factor(hip, fac, a, y[1], 0), refs, zs)
        compare("streamed", N, _factor(hip, fac, a, y, N, tiles=_tiles(N)), refs, z)
    print(f"gf_factor W = {W} ({Jr}, {Jc}): d {worst['d']:.1e}, W {worst['W']:.1e}, z {worst['z']:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", sc.STRUCTURES, ids=[_ids(s) for s in sc.STRUCTURES])
def test_factor_failing_pivot_in_a_streamed_tile(hip, Jr, Jc):
    """N = 70 in tiles of 1, 8 and 61 rows; problem 1 of three gets a negative diagonal at row 4, inside the second
    tile: info[1] is the oracle's 1-based global row, problems 0 and 2 equal the clean streamed run to the bit, and
    problem 1's rows from the failing one on -- the whole third tile among them -- are never written."""
    N, B = 70, 3
    refs = sc.reference(Jr, Jc, N, B)
    fac = Factor(refs)
    a, y = stack(refs, "a"), stack(refs, "y")
    clean = _factor(hip, fac, a, y, N, tiles=_tiles(N))
    a2 = a.copy()
    a2[1, 4] = -1e6
    r = refs[1]
    _, _, info = cref.factor(r["t"], r["c"], a2[1], r["U"], r["V"])
    assert info == 5
    got = _factor(hip, fac, a2, y, N, tiles=_tiles(N))
    assert list(got["info"]) == [0, info, 0]
    for k in ("d", "W", "z"):
        assert np.array_equal(got[k][[0, 2]], clean[k][[0, 2]]), k
        assert np.array_equal(got[k][1, :info - 1], clean[k][1, :info - 1]), k
        assert np.all(got[k][1, info - 1:] == SENTINEL), k


# ---- gf_solve ----------------------------------------------------------------------------------------------------

def _solve_cases(hip, fac, R, worst, bad, tag):
    """The three modes, with and without the scale, on B problems: the oracle at 1e-10, Z aliasing Y for the solves,
    every problem alone -- same bits."""
    B, N = fac.B, fac.N
    Y = np.stack([sc.rhs(N, R, seed=b) for b in range(B)])
    for mode, name in MODES:
        for scaled in (False, True):
            got = solve(hip, mode, fac, Y, scaled)
            for b in range(B):
                err = sc.relerr(got[b], sc.sweep_reference(mode, fac.refs[b], Y[b], scaled))
                worst[name] = max(worst[name], err)
                if not err <= sc.TOL:
                    bad.append((tag, name, scaled, N, R, b, err))
                one = solve(hip, mode, fac.only(b), Y[b:b + 1], scaled)
                assert np.array_equal(one[0], got[b]), (tag, name, scaled, N, R, b)
            if mode != sc.MATMUL:
                assert np.array_equal(solve(hip, mode, fac, Y, scaled, inplace=True), got), (tag, name, scaled, N, R)


@pytest.mark.parametrize("Jr,Jc", sc.STRUCTURES, ids=[_ids(s) for s in sc.STRUCTURES])
def test_solve_every_length(hip, Jr, Jc):
    """Every length of sweep_cases.LENGTHS with R = 1 (k_solve_vec) and R = 3 (k_solve_rhs), B = 3."""
    worst, bad = {n: 0.0 for _, n in MODES}, []
    for N in sc.LENGTHS:
        fac = Factor(sc.reference(Jr, Jc, N))
        for R in (1, 3):
            _solve_cases(hip, fac, R, worst, bad, "lengths")
    print(f"gf_solve W = {Jr + 2 * Jc} ({Jr}, {Jc}), R = 1, 3: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("W", [16, 65, 129, 256])
def test_solve_right_hand_side_tiles(hip, W):
    """R in {2, 63, 64, 65, 130} at N = 17: a tile of 64 right-hand sides short, full, one over, and three tiles."""
    worst, bad = {n: 0.0 for _, n in MODES}, []
    fac = Factor(sc.reference(*sc.structure_of(W), 17))
    for R in (2, 63, 64, 65, 130):
        _solve_cases(hip, fac, R, worst, bad, "tiles")
    print(f"gf_solve W = {W}, R = 2 .. 130: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert not bad, bad


def test_matmul_lower_in_place_is_refused(hip):
    lib, p = hip.load(), hip.ptr
    fac = Factor(sc.reference(1, 8, 9))
    for R in (1, 3):
        buf = sentinel(fac.B * fac.N * R)
        rc = lib.gf_solve(sc.MATMUL, fac.B, fac.N, fac.W, fac.ld, R, p(fac.U), p(fac.Wm), p(fac.P), None, p(buf),
                          p(buf), None)
        assert rc < 0 and "in place" in hip.last_error()
        torch.cuda.synchronize()
        assert bool(torch.all(buf == SENTINEL))


# ---- gf_reduce_tile + gf_loglike_finish -----------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_reduce_tile_and_loglike_finish(hip, N):
    """acc = {sum log d, sum z^2 / d, min d} against numpy (sums of at most 514 terms of either sign in a fixed tree:
    1e-12 of the sum of their magnitudes), accumulation of a second tile with init = 0, z = NULL, and the finish with
    a failed problem."""
    lib, p = hip.load(), hip.ptr
    B = 3
    rng = np.random.default_rng([5, N])
    d, z = rng.uniform(0.05, 30.0, (2, B, N)), rng.normal(size=(2, B, N)) * 3.0
    work = torch.full((B * int(lib.gf_reduce_work(N)) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    acc = sentinel((B + 1) * 3)
    dd, zd = dev(d), dev(z)

    def reduce(k, zp, init):
        hip.check(lib.gf_reduce_tile(B, N, p(dd[k]), zp, p(work), p(acc), init, None), "gf_reduce_tile")
        torch.cuda.synchronize()
        return take(acc, B * 3, "acc").reshape(B, 3)

    def close(got, terms):
        return np.all(np.abs(got - terms.sum(axis=-1)) <= 1e-12 * np.abs(terms).sum(axis=-1))

    one = reduce(0, p(zd[0]), 1)
    assert close(one[:, 0], np.log(d[0])) and close(one[:, 1], z[0] ** 2 / d[0])
    assert np.array_equal(one[:, 2], d[0].min(axis=1))
    two = reduce(1, p(zd[1]), 0)
    assert close(two[:, 0], np.log(np.concatenate([d[0], d[1]], axis=1)))
    assert close(two[:, 1], np.concatenate([z[0] ** 2 / d[0], z[1] ** 2 / d[1]], axis=1))
    assert np.array_equal(two[:, 2], np.minimum(d[0].min(axis=1), d[1].min(axis=1)))
    noz = reduce(0, None, 1)
    assert np.array_equal(noz[:, 0], one[:, 0]) and np.all(noz[:, 1] == 0.0) and np.array_equal(noz[:, 2], one[:, 2])

    reduce(0, p(zd[0]), 1)
    info = torch.tensor([0, 7, 0, INFO_SENTINEL], dtype=torch.int32, device="cuda")
    out, logdet = sentinel(B + 1), sentinel(B + 1)
    hip.check(lib.gf_loglike_finish(B, N, p(acc), p(info), p(out), p(logdet), None), "gf_loglike_finish")
    torch.cuda.synchronize()
    out, logdet = take(out, B, "out"), take(logdet, B, "logdet")
    assert out[1] == -np.inf and logdet[1] == -np.inf
    want = -0.5 * (one[:, 0] + N * np.log(2.0 * np.pi)) - 0.5 * one[:, 1]
    for b in (0, 2):
        # (three terms, each rounded once or twice)
        assert logdet[b] == one[b, 0] and abs(out[b] - want[b]) <= 1e-15 * (abs(one[b, 0]) + 2 * N + one[b, 1])
