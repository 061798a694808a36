"""GPU: gf_chunk_corrections (k_corr_small + k_corr_finish_small) through its raw C entry point against
tests/lft_ref.corrections in 80 bits, and, for real maps, against the sequential recurrence's own sums (sum log D and
sum z^2 / D from the true start state minus the same from the zero state, tests/lft_ref.real_maps).

Inputs: the 80-bit true start states rounded to float64 and the maps' G, m, in 64 x 64 slots [b * nch + c]; slots
outside the chunk range hold NaN.  acc is [B + 1][3], (10.0, -3.0, 0.25) in every row: row B and column 2 (min d) must
come back untouched, and the values are judged as acc holds them (10 + the sum of log det(I - X G) over the range,
-3 + the sum of the quadratic forms), error |value - ref| / max(1, |ref|) per problem with the reference summed the
same way.  Bar: the larger of 100 x the error of a plain float64 evaluation (numpy.linalg, tests/lft_ref.corrections64)
of the same sums against the same reference, and W eps kappa, kappa the largest cond(I - X G) of the range.

Measured on an MI355X (largest error of a class; the error closest to its bar is printed with that bar, pytest -s):
synthetic family W = 1-16 1.5e-15 (bar 1.2e-14), 17-32 3.8e-14 (2.0e-13, W = 20: the nearest any case came to its
bar, a factor 5), 33-48 2.9e-14 (7.8e-13), 49-63 2.7e-14 (2.2e-12), the ranges at W = 61 6.0e-14 (5.7e-12); real
family 3.8e-15 against the 80-bit formulas and 3.9e-15 against the recurrence's own sums (bars from 2.7e-14);
rank-deficient X 1.2e-15 (an early chunk, bar 6.2e-13) and 1.7e-14 (rank 2 at W = 48, bar 9.6e-12)."""
import functools

import numpy as np
import pytest
import torch

from tests import lft_ref as R
from tests.test_gpu_chunk_combine import CLASSES, EPS, REAL_SHAPES, REAL_STRUCTURES, SENTINEL, Worst

pytestmark = pytest.mark.gpu

LD = R.LD
PREFILL = (10.0, -3.0, 0.25)


def pack(cases, nch):
    """X, Y (the true start states, rounded to float64), G, m of the first nch chunks of every problem."""
    st = [s for c in cases for s in c["starts"][:nch]]
    maps = [M for c in cases for M in c["maps"][:nch]]
    return dict(X=R.pack_matrices([s[0] for s in st]), Y=R.pack_vectors([s[1] for s in st]),
                G=R.pack_matrices([M[1] for M in maps]), m=R.pack_vectors([M[4] for M in maps]))


def corr_call(hip, W, B, nch, first, count, a, work_fill=float("nan")):
    """gf_chunk_corrections on the packed arrays ``a`` with every slot outside the range replaced by NaN: acc [B][3]
    after the call (row B, the sentinel row, and column 2 checked here)."""
    lib, p = hip.load(), hip.ptr
    d = {}
    for k, v in a.items():
        v = v.reshape(B, nch, -1).copy()
        v[:, :max(first, 0)] = np.nan
        v[:, max(first + count, 0):] = np.nan
        d[k] = torch.from_numpy(v.reshape(B * nch, -1)).cuda()
    acc = torch.tensor([PREFILL] * (B + 1), dtype=torch.float64, device="cuda")
    need = int(lib.gf_chunk_corrections_work(B, nch))
    work = torch.full((need + 5,), work_fill, dtype=torch.float64, device="cuda")
    rc = lib.gf_chunk_corrections(B, nch, W, first, count, p(d["X"]), p(d["Y"]), p(d["G"]), p(d["m"]), p(acc),
                                  p(work), None)
    hip.check(rc, "gf_chunk_corrections")
    torch.cuda.synchronize()
    out = acc.cpu().numpy()
    assert tuple(out[B]) == PREFILL and np.all(out[:, 2] == PREFILL[2])
    tail = work[need:].cpu().numpy()                    # nothing is written behind the workspace
    assert np.array_equal(tail, np.full(5, work_fill), equal_nan=True)
    return out[:B]


@functools.lru_cache(maxsize=None)
def _chunk_values(kind, key, c):
    """((log det, quadratic form) in 80 bits, the same in float64) of chunk c of a case, on the float64 inputs."""
    case = R.synthetic_case(*key) if kind == "synthetic" else R.real_case(*key)
    X, Y = (np.asarray(x, dtype=np.float64) for x in case["starts"][c])
    M = case["maps"][c]
    ld, q, sg = R.corrections(X, Y, M[1], M[4])
    assert sg == 1
    return (ld, q), R.corrections64(X, Y, M[1], M[4])


def judge(acc, kind, keys, first, count, recurrence=False):
    """Per problem (error, bar) of acc [B][3] over the chunk range; ``recurrence``: against the sequential
    recurrence's own differences instead of the 80-bit formulas."""
    out = []
    for b, key in enumerate(keys):
        case = R.synthetic_case(*key) if kind == "synthetic" else R.real_case(*key)
        vals = [_chunk_values(kind, key, c) for c in range(first, first + count)]
        err, e64 = 0.0, 0.0
        for k in (0, 1):
            if recurrence:
                ref = LD(PREFILL[k]) + sum((case["dld"], case["dqd"])[k][first:first + count], LD(0.0))
            else:
                ref = LD(PREFILL[k]) + sum((v[0][k] for v in vals), LD(0.0))
            f64 = PREFILL[k]
            for v in vals:
                f64 = f64 + v[1][k]
            scale = max(LD(1.0), abs(ref))
            err = max(err, float(abs(LD(acc[b][k]) - ref) / scale))
            e64 = max(e64, float(abs(LD(f64) - ref) / scale))
        kappa = max(case["conds"][first:first + count], default=1.0)
        out.append((err, max(100.0 * e64, case["W"] * EPS * kappa)))
    return out


@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_width(hip, cls):
    """W = 1 ... 63 (every boundary of the kernel's rounding of W to 4: 4 | 5, ..., 60 | 61 -- from 61 on it opts in
    to more than 64 KB of LDS -- and 63), B = 3 problems, nch = 4, the engine's range (1, nch - 1)."""
    worst = Worst()
    for W in CLASSES[cls]:
        keys = [(W, 4, b) for b in range(3)]
        a = pack([R.synthetic_case(*k) for k in keys], 4)
        worst.add("corrections", (W,), judge(corr_call(hip, W, 3, 4, 1, 3, a), "synthetic", keys, 1, 3))
    worst.report(f"widths {cls}")


@pytest.mark.parametrize("Jr,Jc", REAL_STRUCTURES)
def test_real_plain_coordinate_maps(hip, Jr, Jc):
    """The edge problems' maps and true start states at 13, 8, 100 and 4 chunks, B = 2, the ranges (1, nch - 1) and
    (0, nch): against the 80-bit formulas and against the recurrence's own differences."""
    worst = Worst()
    W = Jr + 2 * Jc
    for N, L in REAL_SHAPES:
        keys = [(Jr, Jc, N, L, b) for b in range(2)]
        cases = [R.real_case(*k) for k in keys]
        nch = len(cases[0]["maps"])
        a = pack(cases, nch)
        for first, count in ((1, nch - 1), (0, nch)):
            acc = corr_call(hip, W, 2, nch, first, count, a)
            worst.add("80-bit formulas", (N, L, first, count), judge(acc, "real", keys, first, count))
            worst.add("recurrence sums", (N, L, first, count), judge(acc, "real", keys, first, count, True))
    worst.report(f"(Jr, Jc) = ({Jr}, {Jc}), W = {W}")


@pytest.mark.parametrize("W", [5, 17, 48, 61])
def test_chunk_ranges(hip, W):
    """nch = 5: (1, nch - 1), (0, nch), (2, 1), (nch - 1, 1); (0, 0) leaves acc bit-identical.  The slots outside a
    range hold NaN (corr_call)."""
    nch, keys = 5, [(W, 5, b) for b in range(3)]
    a = pack([R.synthetic_case(*k) for k in keys], nch)
    worst = Worst()
    for first, count in ((1, nch - 1), (0, nch), (2, 1), (nch - 1, 1)):
        acc = corr_call(hip, W, 3, nch, first, count, a)
        worst.add("corrections", (W, first, count), judge(acc, "synthetic", keys, first, count))
    worst.report(f"W = {W}")
    for first in (0, 3, nch):
        assert np.array_equal(corr_call(hip, W, 3, nch, first, 0, a), np.array([PREFILL] * 3)), first
    # two calls, and a zero-filled workspace against the NaN-filled one: identical bits
    base = corr_call(hip, W, 3, nch, 1, nch - 1, a)
    assert np.array_equal(base, corr_call(hip, W, 3, nch, 1, nch - 1, a))
    assert np.array_equal(base, corr_call(hip, W, 3, nch, 1, nch - 1, a, work_fill=0.0))
    # problem b alone
    for b in range(3):
        one = corr_call(hip, W, 1, nch, 1, nch - 1, {k: v[b * nch:(b + 1) * nch] for k, v in a.items()})
        assert np.array_equal(one[0], base[b]), b


def test_rank_deficient_states(hip):
    """X of numerical rank far below W: the start state of chunk 1 of a series in chunks of 8 rows and of 1 row at
    W = 63 (rank <= 8, rank 1), and the synthetic family at rank 2, W = 17 and 48.  The values come from the pivoted
    elimination of I - X G, not from the truncated Cholesky factor: the same bar."""
    worst = Worst()
    for N, L in ((64, 8), (100, 1)):
        keys = [(3, 30, N, L, b) for b in range(2)]
        cases = [R.real_case(*k) for k in keys]
        nch = len(cases[0]["maps"])
        assert np.linalg.matrix_rank(np.asarray(cases[0]["starts"][1][0], dtype=np.float64)) <= L
        acc = corr_call(hip, 63, 2, nch, 1, 1, pack(cases, nch))
        worst.add("early chunk", (N, L), judge(acc, "real", keys, 1, 1))
    for W in (17, 48):
        keys = [(W, 4, b, 2) for b in range(3)]
        cases = [R.synthetic_case(*k) for k in keys]
        assert np.linalg.matrix_rank(np.asarray(cases[0]["starts"][1][0], dtype=np.float64)) == 2
        acc = corr_call(hip, W, 3, 4, 1, 3, pack(cases, 4))
        worst.add("rank 2", (W,), judge(acc, "synthetic", keys, 1, 3))
    worst.report("rank-deficient X")


def _rounded(f):
    return dict(maps=[tuple(np.asarray(x, dtype=np.float64) for x in M) for M in f["maps"]], starts=f["starts"])


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (0, 31)])
@pytest.mark.parametrize("nrows", [1, 2])
def test_non_positive_pivot_gives_nan(hip, Jr, Jc, nrows):
    """tests/lft_ref.planted_failure (pinned by tests/test_lft_ref_host.py): N = 197 in 13 chunks of 16 rows, problem
    1 of 3 has one non-positive true pivot (the first row of chunk 3; det(I - X G) < 0) or two (both in chunk 6;
    det(I - X G) > 0, a parity check would pass it) under a healthy nominal pass.  acc[1][0:2] are NaN, problems 0
    and 2 keep the bits of the healthy call; the failing chunk alone gives NaN, the chunks before it the healthy
    values."""
    W, nch = Jr + 2 * Jc, 13
    keys = [(Jr, Jc, 197, 16, b) for b in range(3)]
    healthy = [R.real_case(*k) for k in keys]
    f = R.planted_failure(Jr, Jc, nrows)
    ch = f["chunk"]
    a = pack([healthy[0], _rounded(f), healthy[2]], nch)
    base = corr_call(hip, W, 3, nch, 1, nch - 1, pack(healthy, nch))
    assert np.all(np.isfinite(base))
    got = corr_call(hip, W, 3, nch, 1, nch - 1, a)
    assert np.all(np.isnan(got[1, :2])), got
    assert np.array_equal(got[[0, 2]], base[[0, 2]])
    one = corr_call(hip, W, 3, nch, ch, 1, a)
    assert np.all(np.isnan(one[1, :2])) and np.all(np.isfinite(one[[0, 2]])), one
    before = corr_call(hip, W, 3, nch, 1, ch - 1, a)
    assert np.array_equal(before, corr_call(hip, W, 3, nch, 1, ch - 1, pack(healthy, nch)))
    worst = Worst()
    worst.add("chunks before the failing one", (ch,), judge(before, "real", keys, 1, ch - 1))
    worst.report(f"(Jr, Jc) = ({Jr}, {Jc})")


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    B, nch, W = 2, 5, 17
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    X, G = f(B * nch * 4096), f(B * nch * 4096)
    Y, m = f(B * nch * 64), f(B * nch * 64)
    acc, work = f(3 * B), f(int(lib.gf_chunk_corrections_work(B, nch)))

    def call(B=B, nch=nch, W=W, first=1, count=nch - 1, X=X, acc=acc, work=work):
        return lib.gf_chunk_corrections(B, nch, W, first, count, p(X), p(Y), p(G), p(m), p(acc), p(work), None)

    for kw in (dict(W=0), dict(W=64), dict(first=1, count=nch), dict(first=nch, count=1), dict(first=-1, count=2),
               dict(count=-1), dict(B=1, nch=65536, first=0, count=1), dict(B=256, nch=256, first=0, count=1),
               dict(B=0), dict(nch=0, first=0, count=0), dict(X=None), dict(acc=None), dict(work=None)):
        assert call(**kw) == -1, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool(torch.all(x == SENTINEL)) for x in (X, G, Y, m, acc, work))


def test_workspace_formula():
    """gf_chunk_corrections_work(B, nch) = B nch (3 * 64^2 + 18 * 64 + 1) doubles."""
    from gadfly_amd import _lib
    lib = _lib.load()
    for B, nch in ((1, 1), (3, 4), (2, 100), (64, 1023), (1, 65535)):
        assert lib.gf_chunk_corrections_work(B, nch) == B * nch * (3 * 64 * 64 + 18 * 64 + 1), (B, nch)
    assert lib.gf_chunk_corrections_work(0, 4) == -1 and lib.gf_chunk_corrections_work(4, 0) == -1
