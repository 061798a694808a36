"""TEST INFRASTRUCTURE: the cases of tests/test_gpu_chunk_linear.py, test_gpu_chunk_linear_combine.py and
test_gpu_chunk_transition.py on the synthetic family of tests/lin_ref.py, with their cached 80-bit references and
float64 restatements; tests/test_lin_ref_host.py asserts the conditioning of every one of them without a device."""
import functools

import numpy as np

from tests import lin_ref as R

EPS = float(np.finfo(np.float64).eps)
MODES = (R.LOWER, R.UPPER, R.MATMUL)
CLASSES = {f"{a}-{min(a + 7, 63)}": range(a, min(a + 8, 64)) for a in range(1, 64, 8)}
#: both sides of k_mmR_mfma's tiles (16 | 17, 32 | 33, 48 | 49), of ROWS = 4, 60 and 64, the smallest, the largest
EDGE_WIDTHS = (1, 3, 4, 5, 16, 17, 32, 33, 48, 49, 60, 61, 63)
#: k_lin1's ring of 24 rows and scalar blocks of 64, k_linR7's fetch three rows ahead, k_mmR_mfma's blocks of 16
CHUNK_LENS = (1, 2, 3, 4, 15, 16, 17, 23, 24, 25, 31, 33, 63, 64, 65, 127, 128, 129)
RHS_COUNTS = (2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65)
#: a reset at every offset 0 .. 15 of a 16-row block (rows 16 k + k), three in a row (100 .. 102), on the first
#: (64, 128) and on the last (63, 127) row of a chunk of 64
RESET_ROWS = tuple(sorted({16 * k + k % 16 for k in range(17)} | {100, 101, 102, 63, 64, 127, 128}))

# a case: (W, N, L, kwargs of lin_ref.synthetic as a sorted tuple of items)


def case(W, N, L, **kw):
    return (W, N, L, tuple(sorted(kw.items())))


def rows_of(cs):
    W, N, L, kw = cs
    return R.synthetic(W, N, **dict(kw))


def width_case(W):
    return case(W, 333, 64)


def chunk_len_case(W, L):
    """Two chunks of L rows and a ragged last one of a single row."""
    return case(W, 2 * L + 1, L, key=L)


def rhs_case(W):
    return case(W, 150, 64, key=1)


def reset_cases(W):
    return (case(W, 280, 64, grid=False, resets=RESET_ROWS, key=2), case(W, 280, 64, grid=False, key=3))


TRANSITION_WIDTHS = (5, 34)
BAD_ROWS = (0, 17, 63, 64, 200)      # rows without a pivot (dbar <= 0): a chunk's first and last row among them


def transition_cases(W):
    """The chunkings of the transition sweep: a single chunk of 1 ... 65 rows, chunks of 128 rows, a ragged last chunk
    of one row, and the reset rows of reset_cases."""
    return ([case(W, N, 128, key=6) for N in (1, 7, 15, 16, 17, 63, 65)]
            + [case(W, 333, 128, key=6), case(W, 129, 64, key=6), reset_cases(W)[0]])


def linear_cases():
    """Every (case, R) the sweeps run on the device."""
    for W in TRANSITION_WIDTHS:
        for cs in transition_cases(W):
            yield cs, 3
    for W in range(1, 64):
        yield width_case(W), 40
    for W in EDGE_WIDTHS:
        for L in CHUNK_LENS:
            yield chunk_len_case(W, L), 16
    for W in (5, 33, 63):
        yield rhs_case(W), 65
    for W in (7, 33):
        for cs in reset_cases(W):
            yield cs, 40


@functools.lru_cache(maxsize=None)
def sweep_ref(cs, mode, Rmax, dtype=R.LD):
    """dict(Z [2][B][N][R], starts, loc [2][nch][B][W][R]) of a case with Rmax right-hand sides, unscaled (0) and
    scaled (1) input: the two inputs run side by side as 2 Rmax columns of one sweep."""
    W, N, L, _ = cs
    rows = rows_of(cs)
    Y = R.rhs(W, N, Rmax, key=dict(cs[3]).get("key", 0))
    Yc = np.concatenate([R.scaled_input(mode, rows, Y, s, dtype) for s in (0, 1)], axis=2)
    Z, starts = R.sequential(mode, rows, Yc, L, dtype)
    loc = R.local_states(mode, rows, Yc, L, dtype)
    cut = lambda x: np.stack([x[..., :Rmax], x[..., Rmax:]])         # noqa: E731
    return dict(Y=Y, Z=cut(Z), starts=cut(starts), loc=cut(loc))


@functools.lru_cache(maxsize=None)
def map_inputs(cs, bad=()):
    """(r, dbar, zbar) [B][N][64], [B][N], [B][N] of a case's transition sweep, float64: r = w~ d as the engine forms
    it (ScaledFactor._ensure_transitions: one float64 product), dbar = d with the rows ``bad`` set to 0, -1.5, 0, ...
    (rows without a pivot), zbar ~ N(0, 1)."""
    rows = rows_of(cs)
    r = rows["Wt"] * rows["d"][:, :, None]
    dbar = rows["d"].copy()
    for k, n in enumerate(bad):
        dbar[:, n] = -1.5 * (k % 2)
    zbar = np.stack([np.random.default_rng([cs[0], b, 9]).normal(size=cs[1]) for b in range(dbar.shape[0])])
    return r, dbar, zbar


@functools.lru_cache(maxsize=None)
def map_ref(cs, dtype=R.LD, bad=()):
    """(Phi, G, m) [nch][B]... of lin_ref.transitions on a case with the rows of map_inputs."""
    r, dbar, zbar = map_inputs(cs, bad)
    return R.transitions(rows_of(cs), cs[2], r=r, dbar=dbar, zbar=zbar, dtype=dtype)


def gamma(ref, Y):
    """The reference's own amplification max(1, max |Z| / max |Y|), per problem [B]."""
    B = Y.shape[0]
    return np.array([max(1.0, float(np.max(np.abs(ref[b])) / np.max(np.abs(Y[b])))) for b in range(B)])


def bar(e64, W, g):
    """The larger of 100 x the float64 restatement's error and W eps gamma."""
    return max(100.0 * e64, W * EPS * g)


class Worst:
    """The error closest to (or furthest beyond) its bar and the largest error of a test, per kind of comparison."""

    def __init__(self):
        self.seen, self.largest, self.bad = {}, {}, []

    def add(self, key, what, err, limit):
        self.largest[key] = max(self.largest.get(key, 0.0), err)
        cur = self.seen.get(key)
        if cur is None or err / max(limit, 1e-300) > cur[0] / max(cur[1], 1e-300):
            self.seen[key] = (err, limit, what)
        if not err <= limit:
            self.bad.append((key, what, err, limit))

    def report(self, title):
        for key, (err, limit, what) in self.seen.items():
            print(f"{title} {key}: worst error {err:.2e} against its bar {limit:.2e} at {what}; "
                  f"largest error {self.largest[key]:.2e}")
        assert not self.bad, self.bad[:20]
