"""GPU: gf_chunk_combine (k_combine<32|48|64>) and gf_chunk_combine_tree (k_tree_compose / k_tree_top / k_tree_apply)
through their raw C entry points, on W x W maps in 64 x 64 slots, against the 80-bit start states of tests/lft_ref.py
(pinned without the device by tests/test_lft_ref_host.py).  Both entry points get the same inputs.

Error of a problem: max |device - reference| over the leading W x W (and W) of all its slots, divided by
max(1, max |reference|) for the synthetic family (lft.random_maps: non-symmetric Phi, |X| ~ 4) and by max |reference|
of that array for the real family (the plain-coordinate maps gf_loglike_grad_chunked hands over: |X| ~ 1e-5,
G = sum h h^T / D positive semi-definite, I - X G with eigenvalues down to 0.02).  Its bar: the larger of 100 x the
error of float64 oracle/lft.py on that same problem against the same reference, and W eps kappa with kappa the largest
cond(I - X G) along the chain -- the backward-error scale of a pivoted W x W elimination; the factor 100 allows for
the kernels' looser pivot choice (32-bit keys) and their own association.  Slot 0 is exactly zero, and whatever lies
outside the leading W x W of an output slot is exactly zero or still the sentinel.

Measured on an MI355X (largest error of a class; the error closest to its bar is printed with that bar, pytest -s):
synthetic family, sequential / tree: W = 1-16 1.1e-15 / 1.0e-15 (bars from 3.7e-15), 17-32 2.9e-15 / 3.1e-15
(bars ~ 1e-13), 33-48 5.5e-15 / 6.1e-15 (~ 1e-12), 49-63 8.6e-15 / 7.9e-15 (~ 2.5e-12), W = 64 6.2e-15 / 7.8e-15
(5.4e-12); real family: 3.1e-14 sequential ((0, 31), 100 chunks of one row; bar 1.9e-12), 5.1e-14 tree ((3, 30), 100
chunks; bar 2.0e-12).  No case came nearer than a factor 15 to its bar ((1, 0), W = 1, tree at 7 chunks: 2.1e-16
against 3.7e-15)."""
import functools

import numpy as np
import pytest
import torch

from tests import grad_cases as gc
from tests import lft_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77                  # what every output holds before a call: no result of these problems
EPS = float(np.finfo(np.float64).eps)
CLASSES = {"1-16": range(1, 17), "17-32": range(17, 33), "33-48": range(33, 49), "49-63": range(49, 64)}
#: both sides of every 16-column tile and of the three LDS sizes (32 | 33, 48 | 49), the smallest, the largest
EDGE_WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
SEQ_COUNTS = (1, 2, 3, 4, 7, 8, 13)
#: P = 2, 4, 4, 8, 8, 8, 16, 16, 16, 32, 64: no padding (2, 4, 8, 16), one slot (3, 7), almost half (5, 9, 17, 33);
#: at P = 2 the up-sweep has no level at all
TREE_COUNTS = (2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 33)
REAL_STRUCTURES = gc.STRUCTURES + ((1, 24), (0, 24))
#: chunks: 13 (last of 5 rows), 8, 100 (one row each), 4 (last of one row)
REAL_SHAPES = ((197, 16), (64, 8), (100, 1), (13, 4))


def pow2(nch):
    """The power of two P with P / 2 < nch <= P (at least 2)."""
    return max(2, 1 << (nch - 1).bit_length())


def pack(cases, nch):
    """Phi, G, m, S (nominal end X), F (nominal end Y) of the first nch chunks of every problem, slots [b * nch + c]."""
    maps = [M for c in cases for M in c["maps"][:nch]]
    return dict(Phi=R.pack_matrices([M[0] for M in maps]), G=R.pack_matrices([M[1] for M in maps]),
                m=R.pack_vectors([M[4] for M in maps]), S=R.pack_matrices([M[2] for M in maps]),
                F=R.pack_vectors([M[3] for M in maps]))


def _dev(x, extra=0):
    """x on the device, ``extra`` sentinel slots behind it."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    t = torch.full((x.shape[0] + extra, x.shape[1]), SENTINEL, dtype=torch.float64, device="cuda")
    t[:x.shape[0]] = torch.from_numpy(x)
    return t


def seq_call(hip, W, B, nch, a):
    """gf_chunk_combine on the packed arrays ``a``: (S_state, F_state) after the call; one sentinel slot behind every
    array, inputs included, must survive."""
    lib, p = hip.load(), hip.ptr
    d = {k: _dev(v, 1) for k, v in a.items()}
    rc = lib.gf_chunk_combine(B, nch, W, p(d["Phi"]), p(d["G"]), p(d["m"]), p(d["S"]), p(d["F"]), None)
    hip.check(rc, "gf_chunk_combine")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in d.items()}
    n = B * nch
    assert all(np.all(v[n:] == SENTINEL) for v in out.values())
    for k in ("Phi", "G", "m"):                         # const inputs
        assert np.array_equal(out[k][:n], a[k], equal_nan=True), k
    return out["S"][:n], out["F"][:n]


def tree_call(hip, W, B, nch, a, P=None, work_extra=0, work_fill=float("nan")):
    """gf_chunk_combine_tree on the packed arrays ``a`` (the map arrays may be overwritten: copies): (Xst, Yst),
    pre-filled with the sentinel, one slot more than the call may write; the workspace holds ``work_fill`` (NaN:
    nothing may be read before it is written)."""
    lib, p = hip.load(), hip.ptr
    P = pow2(nch) if P is None else P
    d = {k: _dev(v) for k, v in a.items()}
    n = B * nch
    Xst = torch.full((n + 1, 4096), SENTINEL, dtype=torch.float64, device="cuda")
    Yst = torch.full((n + 1, 64), SENTINEL, dtype=torch.float64, device="cuda")
    need = int(lib.gf_chunk_combine_tree_work(B, P, nch))
    work = torch.full((max(need, 8) + work_extra,), work_fill, dtype=torch.float64, device="cuda")
    rc = lib.gf_chunk_combine_tree(B, P, nch, W, p(d["Phi"]), p(d["G"]), p(d["m"]), p(d["S"]), p(d["F"]), p(Xst),
                                   p(Yst), p(work), None)
    hip.check(rc, "gf_chunk_combine_tree")
    torch.cuda.synchronize()
    X, Y = Xst.cpu().numpy(), Yst.cpu().numpy()
    assert np.all(X[n:] == SENTINEL) and np.all(Y[n:] == SENTINEL)
    return X[:n], Y[:n]


def state_errors(X, Y, cases, nch, real):
    """Per problem (error, bar) of the device's slots X [B * nch][4096], Y [B * nch][64], after the layout checks:
    slot 0 exactly zero, everything outside the leading W x W (W) exactly zero or still the sentinel."""
    W = cases[0]["W"]
    lead, rest = R.unpack_matrices(X, W)
    assert np.all((rest == 0.0) | (rest == SENTINEL)), "an output slot holds a number outside its leading W x W"
    tail = Y[:, W:]
    assert np.all((tail == 0.0) | (tail == SENTINEL)), "an output vector holds a number beyond W"
    out = []
    for b, c in enumerate(cases):
        gx, gy = lead[b * nch:(b + 1) * nch], Y[b * nch:(b + 1) * nch, :W]
        assert not gx[0].any() and not gy[0].any(), "slot 0 is not exactly zero"
        rx, ry = (np.array([s[k] for s in c["starts"][:nch]]) for k in (0, 1))
        ox, oy = (np.array([s[k] for s in c["starts64"][:nch]]) for k in (0, 1))
        floor = 0.0 if real else 1.0
        if nch == 1:
            out.append((0.0, 0.0))
            continue
        err = max(R.scaled_error(gx, rx, floor), R.scaled_error(gy, ry, floor))
        e64 = max(R.scaled_error(ox, rx, floor), R.scaled_error(oy, ry, floor))
        out.append((err, max(100.0 * e64, W * EPS * max(c["conds"][:nch]))))
    return out


class Worst:
    """The error closest to (or furthest beyond) its bar and the largest error of a test, per kind of call."""

    def __init__(self):
        self.seen, self.largest, self.bad = {}, {}, []

    def add(self, key, what, pairs):
        for b, (err, bar) in enumerate(pairs):
            self.largest[key] = max(self.largest.get(key, 0.0), err)
            cur = self.seen.get(key)
            if cur is None or err / max(bar, 1e-300) > cur[0] / max(cur[1], 1e-300):
                self.seen[key] = (err, bar, what, b)
            if not err <= bar:
                self.bad.append((key, what, b, err, bar))

    def report(self, title):
        for key, (err, bar, what, b) in self.seen.items():
            print(f"{title} {key}: worst error {err:.2e} against its bar {bar:.2e} at {what}, problem {b}; "
                  f"largest error {self.largest[key]:.2e}")
        assert not self.bad, self.bad


def both_entry_points(hip, worst, cases, seq_counts, tree_counts, real, what):
    W, B = cases[0]["W"], len(cases)
    for nch in seq_counts:
        S, F = seq_call(hip, W, B, nch, pack(cases, nch))
        worst.add("sequential", what + (nch,), state_errors(S, F, cases, nch, real))
    for nch in tree_counts:
        X, Y = tree_call(hip, W, B, nch, pack(cases, nch))
        worst.add("tree", what + (nch,), state_errors(X, Y, cases, nch, real))


@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_width(hip, cls):
    """W = 1 ... 63, B = 3 problems of different maps, nch = 5 (sequential) and nch = 9 (tree: P = 16, padded)."""
    worst = Worst()
    for W in CLASSES[cls]:
        cases = [R.synthetic_case(W, 9, b) for b in range(3)]
        both_entry_points(hip, worst, cases, (5,), (9,), False, (W,))
    worst.report(f"widths {cls}")


@pytest.mark.parametrize("W", EDGE_WIDTHS)
def test_chunk_counts(hip, W):
    """Sequential nch = 1, 2, 3, 4, 7, 8, 13; tree nch = 2 ... 33 (P = 2 ... 64, with and without padding); B = 2."""
    worst = Worst()
    cases = [R.synthetic_case(W, 33, b) for b in range(2)]
    both_entry_points(hip, worst, cases, SEQ_COUNTS, TREE_COUNTS, False, (W,))
    worst.report(f"W = {W}")


def test_width_64(hip):
    """The combines take the full slot, W = 64 (k_combine<64> and the tree's <64> instances with compile-time bounds;
    gf_chunk_corrections stops at 63): held to the same bar."""
    worst = Worst()
    both_entry_points(hip, worst, [R.synthetic_case(64, 9, b) for b in range(2)], (5,), (8, 9), False, (64,))
    worst.report("W = 64")


@pytest.mark.parametrize("Jr,Jc", REAL_STRUCTURES)
def test_real_plain_coordinate_maps(hip, Jr, Jc):
    """The nominal-pass maps of two problems of grad_cases.edge_problem in plain coordinates, 13, 8, 100 and 4 chunks
    (last chunks of 5, 8, 1 and 1 rows), against the 80-bit SEQUENTIAL states; both entry points at every count."""
    worst = Worst()
    for N, L in REAL_SHAPES:
        cases = [R.real_case(Jr, Jc, N, L, b) for b in range(2)]
        nch = len(cases[0]["maps"])
        both_entry_points(hip, worst, cases, (nch,), (nch,), True, (N, L))
    worst.report(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}")


@functools.lru_cache(maxsize=None)
def _cases(W, nch, B=3):
    return [R.synthetic_case(W, nch, b) for b in range(B)]


@pytest.mark.parametrize("W", [5, 17, 40, 63])
def test_chunk_0_map_in_both_calling_forms(hip, W):
    """The gradient hands over the true map of chunk 0, the engine zeros for its Phi, G, m: the same start states --
    to the bit from the sequential combine (which skips that solve), within the bar from the tree."""
    for nch in (5, 8, 9):
        cases = _cases(W, 9)
        a = pack(cases, nch)
        z = {k: v.copy() for k, v in a.items()}
        for b in range(len(cases)):
            for k in ("Phi", "G", "m"):
                z[k][b * nch] = 0.0
        S, F = seq_call(hip, W, len(cases), nch, a)
        Sz, Fz = seq_call(hip, W, len(cases), nch, z)
        assert np.array_equal(S, Sz) and np.array_equal(F, Fz), nch
        worst = Worst()
        worst.add("tree, zeros for chunk 0", (W, nch),
                  state_errors(*tree_call(hip, W, len(cases), nch, z), cases, nch, False))
        worst.report(f"W = {W}")


@pytest.mark.parametrize("W", [5, 17, 40, 63])
def test_last_chunk_map_is_never_used(hip, W):
    """Phi, G, m and the nominal end state of the LAST chunk filled with NaN: every slot keeps its bits (callers do
    not sweep the last chunk's transition at all).  nch = 5, 8 (P = nch), 9 and 13 (padded)."""
    for nch in (2, 5, 8, 9, 13):
        cases = _cases(W, 13)
        a = pack(cases, nch)
        nans = [tuple(np.full_like(x, np.nan) for x in M) for M in cases[0]["maps"][:1]]
        n = pack([dict(maps=c["maps"][:nch - 1] + nans) for c in cases], nch)      # (slots stay zero beyond W)
        S, F = seq_call(hip, W, len(cases), nch, a)
        Sn, Fn = seq_call(hip, W, len(cases), nch, n)
        assert np.array_equal(S, Sn) and np.array_equal(F, Fn), ("sequential", nch)
        X, Y = tree_call(hip, W, len(cases), nch, a)
        Xn, Yn = tree_call(hip, W, len(cases), nch, n)
        assert np.array_equal(X, Xn) and np.array_equal(Y, Yn), ("tree", nch)


@pytest.mark.parametrize("W", [17, 40, 63])
def test_call_conventions(hip, W):
    """Two calls give identical bits; problem b alone has the bits it has in the batch; an over-long workspace and a
    zero-filled against a NaN-filled one change nothing."""
    for nch in (5, 9):
        cases = _cases(W, 9)
        B = len(cases)
        a = pack(cases, nch)
        S, F = seq_call(hip, W, B, nch, a)
        S2, F2 = seq_call(hip, W, B, nch, a)
        assert np.array_equal(S, S2) and np.array_equal(F, F2)
        X, Y = tree_call(hip, W, B, nch, a)
        for kw in (dict(), dict(work_extra=1234), dict(work_fill=0.0), dict(work_extra=7, work_fill=3.5)):
            X2, Y2 = tree_call(hip, W, B, nch, a, **kw)
            assert np.array_equal(X, X2) and np.array_equal(Y, Y2), kw
        for b in range(B):
            one = pack(cases[b:b + 1], nch)
            S1, F1 = seq_call(hip, W, 1, nch, one)
            assert np.array_equal(S1, S[b * nch:(b + 1) * nch]) and np.array_equal(F1, F[b * nch:(b + 1) * nch]), b
            X1, Y1 = tree_call(hip, W, 1, nch, one)
            assert np.array_equal(X1, X[b * nch:(b + 1) * nch]) and np.array_equal(Y1, Y[b * nch:(b + 1) * nch]), b


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    B, nch, P, W = 2, 5, 8, 17
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    Phi, G, S, X = (f(B * 8 * 4096) for _ in range(4))
    m, F, Y = (f(B * 8 * 64) for _ in range(3))
    work = f(int(lib.gf_chunk_combine_tree_work(B, 8, 5)))

    def seq(B=B, nch=nch, W=W, Phi=Phi, S=S):
        return lib.gf_chunk_combine(B, nch, W, p(Phi), p(G), p(m), p(S), p(F), None)

    def tree(B=B, P=P, nch=nch, W=W, G=G, X=X, work=work):
        return lib.gf_chunk_combine_tree(B, P, nch, W, p(Phi), p(G), p(m), p(S), p(F), p(X), p(Y), p(work), None)

    for kw in (dict(W=0), dict(W=65), dict(B=0), dict(nch=0), dict(Phi=None), dict(S=None)):
        assert seq(**kw) != 0, kw
        assert hip.last_error(), kw
    for kw in (dict(W=0), dict(W=65), dict(B=0), dict(G=None), dict(X=None), dict(work=None), dict(P=6), dict(P=1),
               dict(nch=4), dict(nch=9)):                    # nch = P / 2, nch = P + 1
        assert tree(**kw) != 0, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool(torch.all(x == SENTINEL)) for x in (Phi, G, S, X, m, F, Y, work))


def test_workspace_formula():
    """gf_chunk_combine_tree_work(B, P, nch) = B (P - nch) (4 * 4096 + 3 * 64) + 8 doubles; -1 for nch > P."""
    from gadfly_amd import _lib
    lib = _lib.load()
    for B, P, nch in ((1, 2, 2), (3, 16, 9), (2, 64, 33), (7, 8, 8), (1, 128, 100), (5, 4, 3)):
        assert lib.gf_chunk_combine_tree_work(B, P, nch) == B * (P - nch) * (4 * 4096 + 3 * 64) + 8, (B, P, nch)
    assert lib.gf_chunk_combine_tree_work(1, 8, 9) == -1 and lib.gf_chunk_combine_tree_work(0, 8, 5) == -1
