"""CPU: pins the helpers of tests/sweep_cases.py -- the float64 C oracle against the 80-bit recurrence on these very
problems, the true chunk states and the numpy restatement of the chunked sweeps against the unchunked oracle, the
restated chunking of the conditional mean and the row patterns its query sets claim."""
import numpy as np
import pytest

from oracle import cref, seq
from tests import sweep_cases as sc


@pytest.mark.parametrize("Jr,Jc,N", [(1, 8, 70), (1, 64, 300), (0, 128, 600)])
def test_c_oracle_is_within_1e13_of_the_80_bit_recurrence(Jr, Jc, N):
    """oracle/cref.py in float64 against oracle/seq.py in np.longdouble on the SAME float64 matrices: d, W, the three
    sweeps and the conditional mean within 1e-13 of the largest entry (measured: 1.6e-14 worst, for W; 2e-15 for d,
    the sweeps and the conditional mean)."""
    ref = sc.reference(Jr, Jc, N, B=1)[0]
    assert ref["info"] == 0
    ld_ = np.longdouble
    t, c, a, U, V = (np.asarray(ref[k], dtype=ld_) for k in ("t", "c", "a", "U", "V"))
    d, Wm, info = seq.factor(t, c, a, U, V)
    assert info == 0
    Y = sc.rhs(N, 2)
    t1 = sc.query_set("full", ref["t"], 1)
    _, _, U1, V1 = seq.celerite_matrices(ref["co"], t1, np.zeros(len(t1)))
    alpha = Y[:, 0]
    mu = seq.predict_mean_at(t, c, U, V, alpha.astype(ld_), t1.astype(ld_), U1.astype(ld_), V1.astype(ld_))
    errs = dict(
        d=sc.relerr(ref["d"], d), W=sc.relerr(ref["W"], Wm),
        lower=sc.relerr(cref.solve_lower(ref["t"], ref["c"], ref["U"], ref["W"], Y), seq.solve_lower(t, c, U, Wm, Y)),
        upper=sc.relerr(cref.solve_upper(ref["t"], ref["c"], ref["U"], ref["W"], Y), seq.solve_upper(t, c, U, Wm, Y)),
        matmul=sc.relerr(cref.matmul_lower(ref["t"], ref["c"], ref["U"], ref["W"], Y),
                         seq.matmul_lower(t, c, U, Wm, Y)),
        mean=sc.relerr(sc.general_matmul_reference(ref, t1, alpha)[0], mu))
    print(f"W = {Jr + 2 * Jc}, N = {N}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v <= 1e-13 for v in errs.values()), errs


def test_every_structure_is_positive_definite_and_names_its_width():
    widths = [Jr + 2 * Jc for Jr, Jc in sc.STRUCTURES]
    assert widths == [1, 2, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 255, 256, 256]
    for Jr, Jc in sc.STRUCTURES:
        for N in (9, 70):
            for r in sc.reference(Jr, Jc, N):
                assert r["info"] == 0 and np.min(r["d"]) > 0
                assert np.max(r["a"]) / np.min(r["d"]) < 100.0


@pytest.mark.parametrize("mode", [sc.LOWER, sc.UPPER, sc.MATMUL])
@pytest.mark.parametrize("Jr,Jc,N", [(1, 8, 17), (1, 32, 70)])
def test_chunked_sweeps_from_the_true_states_reproduce_the_oracle(mode, Jr, Jc, N):
    """Chunk lengths 1, 7, 8 and N, one right-hand side and three, with and without the scale: every chunk swept in
    numpy from its true start state gives the oracle's rows and leaves the next chunk's start state."""
    ref = sc.reference(Jr, Jc, N)[1]
    for R in (1, 3):
        for scaled in (False, True):
            Y = sc.rhs(N, R)
            Yin = sc.carried_input(mode, ref, Y, scaled)
            Z = sc.sweep_reference(mode, ref, Y, scaled).reshape(N, R)
            for L in (1, 7, 8, N):
                start, end = sc.true_chunk_states(mode, ref, Yin, Z, L)
                ch = sc.chunks_of(N, L)
                assert start.shape == (len(ch), Jr + 2 * Jc, R)
                order = range(len(ch))
                for k in order:
                    a, e = ch[k]
                    Zk, endk = sc.chunk_sweep(mode, ref, Yin, a, e, start[k])
                    assert sc.relerr(Zk, Z[a:e]) <= 1e-13 * max(1.0, np.max(np.abs(Z)) / np.max(np.abs(Z[a:e])))
                    assert sc.relerr(endk, end[k]) <= 1e-13
                    nxt = k - 1 if mode == sc.UPPER else k + 1
                    if 0 <= nxt < len(ch):
                        assert np.array_equal(end[k], start[nxt])
                first = len(ch) - 1 if mode == sc.UPPER else 0
                assert not np.any(start[first])


def test_diag_scan_of_local_passes_gives_the_true_states_of_the_product():
    """GF_MATMUL_LOWER's protocol in numpy: local passes from zero, the diagonal scan with the chunks' decays, and
    the true start states come out."""
    N, R = 70, 2
    ref = sc.reference(1, 32, N)[0]
    Y = sc.rhs(N, R)
    Z = sc.sweep_reference(sc.MATMUL, ref, Y, False)
    for L in (1, 7, 9, 35, 69, 70):
        ch = sc.chunks_of(N, L)
        loc = np.array([sc.chunk_sweep(sc.MATMUL, ref, Y, a, e, np.zeros((65, R)))[1] for a, e in ch])
        start, _ = sc.true_chunk_states(sc.MATMUL, ref, Y, Z, L)
        assert sc.relerr(sc.diag_scan(sc.chunk_decays(ref, L), loc), start) <= 1e-13 or not np.any(start)


def test_chunking_and_query_sets():
    assert sc.gmm_chunking(1, 511) == (1, 511) and sc.gmm_chunking(1, 512) == (2, 256)
    assert sc.gmm_chunking(1, 513) == (2, 257) and sc.gmm_chunking(1, 769) == (3, 257)
    assert sc.gmm_chunking(5, 1024) == (4, 256) and sc.gmm_chunking(600, 520) == (1, 520)
    assert sc.gmm_work(1, 10, 511, 65) == 20 and sc.gmm_work(5, 7, 1024, 129) == 70 + 3 * 10 * 4 * 256
    for B, N in ((1, 1), (3, 9), (1, 513), (1, 769), (5, 1024)):
        t = sc.reference(0, 1, N, B=1)[0]["t"]
        nch, L = sc.gmm_chunking(B, N)
        ch = sc.chunks_of(N, L)
        assert len(ch) == nch
        full = sc.query_set("full", t, B)
        q = sc.qidx_of(t, full)
        assert np.all(np.diff(full) >= 0) and q[0] == 0 and q[1] == 0 and q[-1] == N and q[-3] == N
        assert np.count_nonzero(full == t[0]) >= 1 and np.count_nonzero(full == t[-1]) >= 1
        assert np.max(np.unique(full, return_counts=True)[1]) >= 3
        for a, e in ch[:-1]:
            # on the last row of a chunk and strictly after it: qidx = e (the next chunk's a); on the next row: e + 1
            assert np.count_nonzero(q == e) >= 2 and np.count_nonzero(q == e + 1) >= 1
            assert t[e - 1] in full and t[e] in full
        assert np.all(sc.qidx_of(t, sc.query_set("all_before", t, B)) == 0)
        assert np.all(sc.qidx_of(t, sc.query_set("all_after", t, B)) == N)
        assert len(sc.query_set("M1", t, B)) == 1
        one = sc.qidx_of(t, sc.query_set("one_chunk_only", t, B))
        a, e = ch[min(1, nch - 1)]
        if e - a >= 2:                  # inside for both directions: a + 1 <= qidx <= e - 1
            assert np.all((one >= a + 1) & (one <= e - 1)) and one[0] == a + 1 and one[-1] == e - 1
