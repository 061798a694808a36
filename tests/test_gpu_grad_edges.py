"""GPU: gf_loglike_grad through its raw C entry point at the shapes where it can go wrong (tests/grad_cases.py) --
every width at a boundary of its three instances (k_grad<16>, <32>, <64>; odd widths, which no SHO kernel has), every
length at an edge of its ceil(sqrt(N))-row segments -- against the numpy reverse pass and dense autograd
(tests/grad_ref.py); its calling conventions (strides, diag = NULL, workspace, output layout, batch independence), the
failing pivot at the first and last rows of a segment, and its argument checks."""
import math

import numpy as np
import pytest
import torch

from oracle import cref
from tests import grad_cases as gc
from tests.grad_ref import loglike_grad

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77                  # what every output holds before a call: no result of these problems
INFO_SENTINEL = -77
KEYS = ("ll", "real", "comp", "diag_add", "mean", "info")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _bs(a):
    """Batch stride in elements of a host array: 0 for a shared (N,) one, the row length of a (B, S) one."""
    return 0 if a.ndim == 1 else a.shape[1]


def grad_call(hip, Jr, Jc, real, comp, diag_add, t, y, diag, N, work_extra=0, work_fill=0.0):
    """One gf_loglike_grad call on host arrays: real (2, B, max(Jr, 1)), comp (4, B, max(Jc, 1)), diag_add (B,);
    t, y, diag (N,) shared or (B, S >= N) per problem, diag may be None (NULL).  The workspace holds ``work_fill`` on
    entry and is ``work_extra`` doubles per problem larger than gf_grad_work asks.  Every output is allocated one
    problem too long and pre-filled with a sentinel: nothing beyond the B problems may be written, nor the pad column
    of g_real (Jr = 0) or g_comp (Jc = 0).  Returns dict(ll, real (2, B, Jr), comp (4, B, Jc), diag_add, mean, info)."""
    lib, p = hip.load(), hip.ptr
    B, lr, lc = real.shape[1], max(Jr, 1), max(Jc, 1)
    assert real.shape == (2, B, lr) and comp.shape == (4, B, lc) and diag_add.shape == (B,)
    per = int(lib.gf_grad_work(N, Jr + 2 * Jc))
    assert per > 0
    per += work_extra
    work = torch.full((B * per,), work_fill, dtype=torch.float64, device="cuda")
    rd, cd, ad, td, yd = _dev(real), _dev(comp), _dev(diag_add), _dev(t), _dev(y)
    dd = None if diag is None else _dev(diag)
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    ll, g_real, g_comp, g_diag, g_mean = f(B + 1), f(2 * (B + 1) * lr), f(4 * (B + 1) * lc), f(B + 1), f(B + 1)
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_loglike_grad(B, N, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]), p(ad),
                             p(td), _bs(t), p(dd), 0 if diag is None else _bs(diag), p(yd), _bs(y), p(work), per,
                             p(ll), p(g_real), p(g_comp), p(g_diag), p(g_mean), p(info), None)
    hip.check(rc, "gf_loglike_grad")
    torch.cuda.synchronize()
    ll, g_real, g_comp, g_diag, g_mean, info = (x.cpu().numpy() for x in (ll, g_real, g_comp, g_diag, g_mean, info))
    for x in (ll, g_diag, g_mean):
        assert x[B] == SENTINEL
    assert info[B] == INFO_SENTINEL
    assert np.all(g_real[2 * B * lr:] == SENTINEL) and np.all(g_comp[4 * B * lc:] == SENTINEL)
    if Jr == 0:
        assert np.all(g_real == SENTINEL)
    if Jc == 0:
        assert np.all(g_comp == SENTINEL)
    return dict(ll=ll[:B], real=g_real[:2 * B * lr].reshape(2, B, lr)[:, :, :Jr],
                comp=g_comp[:4 * B * lc].reshape(4, B, lc)[:, :, :Jc], diag_add=g_diag[:B], mean=g_mean[:B],
                info=info[:B])


def _identical(a, b, rows=slice(None)):
    """Two results agree to the bit (NaN = NaN) on the problems ``rows``."""
    return all(np.array_equal(a[k][..., rows, :] if a[k].ndim == 3 else a[k][rows],
                              b[k][..., rows, :] if b[k].ndim == 3 else b[k][rows], equal_nan=True) for k in KEYS)


def _errors(prob, b, got, ll, g):
    """[log L relative, six scaled adjoint errors, mean, diag_add] of problem b of a device result against (ll, g)."""
    co = gc.coefficients(prob, b)
    dev = dict(ar=got["real"][0, b], cr=got["real"][1, b], ac=got["comp"][0, b], bc=got["comp"][1, b],
               cc=got["comp"][2, b], dc=got["comp"][3, b])
    adj = [gc.scaled_error(c, dev[k], g[k]) for k, c in zip(gc.NAMES, co)]
    adj += [abs(got[k][b] - g[k]) / max(1.0, abs(g[k])) for k in ("mean", "diag_add")]
    return abs(got["ll"][b] - ll) / abs(ll), max(adj)


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_edge_shapes_match_both_oracles(hip, Jr, Jc):
    """B = 3 problems of different coefficients, data and diagonals (stride N) on a shared axis (stride 0) at every
    length of grad_cases.LENGTHS: log L to 1e-9 and every adjoint to 1e-7 (scaled) of the float64 numpy pass, and of
    dense autograd for problem 0.  The two references agree to 1.4e-12 at these shapes (test_grad_host.py), so the
    bars rest on the kernel alone."""
    bad, worst = [], [0.0, 0.0, 0.0, 0.0]
    for N in gc.LENGTHS:
        prob = gc.edge_problem(Jr, Jc, N)
        got = grad_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"],
                        prob["diag"], N)
        assert np.all(got["info"] == 0), (N, got["info"])
        for b in range(prob["B"]):
            ll, g = loglike_grad(prob["t"], prob["y"][b], prob["diag"][b], Jr, Jc, *gc.coefficients(prob, b),
                                 prob["diag_add"][b])
            errs = list(_errors(prob, b, got, ll, g))
            if b == 0:
                errs += list(_errors(prob, 0, got, *gc.dense_grad(prob, 0)))
            worst = [max(w, e) for w, e in zip(worst, errs + [0.0] * (4 - len(errs)))]
            if any(e > bar for e, bar in zip(errs, (1e-9, 1e-7, 1e-9, 1e-7))):
                bad.append((N, b, errs))
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: numpy pass log L {worst[0]:.1e}, adjoints {worst[1]:.1e}; "
          f"dense autograd log L {worst[2]:.1e}, adjoints {worst[3]:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", [(0, 8), (1, 16), (1, 31)])
def test_call_conventions(hip, Jr, Jc):
    """N = 101 (K = 11, a last segment of two rows) and N = 13 (K = 4, a last segment of one row)."""
    for N in (101, 13):
        prob = gc.edge_problem(Jr, Jc, N)
        B = prob["B"]
        real, comp, da = prob["real"], prob["comp"], prob["diag_add"]
        t, y, diag = prob["t"], prob["y"][0], prob["diag"][0]
        base = grad_call(hip, Jr, Jc, real, comp, da, t, y, diag, N)
        assert np.all(base["info"] == 0) and np.all(np.isfinite(base["ll"]))
        assert all(np.all(np.isfinite(base[k])) for k in KEYS)
        # t, y, diag shared (stride 0) against B copies at a stride of N + 3 (the three pad elements are never read)
        wide = [np.full((B, N + 3), np.nan) for _ in range(3)]
        for w, x in zip(wide, (t, y, diag)):
            w[:, :N] = x
        assert _identical(base, grad_call(hip, Jr, Jc, real, comp, da, *wide, N)), N
        # a workspace 17 doubles per problem longer than asked and full of NaN against a zeroed minimal one: nothing is
        # read before it is written, and the stride is the caller's
        assert _identical(base, grad_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, work_extra=17,
                                          work_fill=float("nan"))), N
        # the same problems alone
        for b in range(B):
            one = grad_call(hip, Jr, Jc, real[:, b:b + 1], comp[:, b:b + 1], da[b:b + 1], t, y, diag, N)
            assert all(np.array_equal(one[k][..., 0, :] if one[k].ndim == 3 else one[k][0],
                                      base[k][..., b, :] if base[k].ndim == 3 else base[k][b]) for k in KEYS), (N, b)
        # diag = NULL against an array of zeros (the white noise folded into diag_add: positive definite without diag)
        da2 = da * 1.05
        null = grad_call(hip, Jr, Jc, real, comp, da2, t, y, None, N)
        assert np.all(null["info"] == 0)
        assert _identical(null, grad_call(hip, Jr, Jc, real, comp, da2, t, y, np.zeros(N), N)), N


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (0, 31)])
def test_failing_pivot_at_segment_edges(hip, Jr, Jc):
    """N = 101: segments of K = 11 rows.  One problem of three loses positive definiteness from row r on -- the first
    row, both sides of a segment boundary (10 | 11), the last row of a segment (98), the first row of the last
    segment (99), the last row (100): info is the C oracle's failing row, log L is -inf, every gradient of that
    problem NaN, and its neighbours do not notice."""
    N = 101
    prob = gc.edge_problem(Jr, Jc, N)
    args = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"])
    base = grad_call(hip, *args, prob["diag"], N)
    assert np.all(base["info"] == 0)
    for r in (0, 10, 11, 98, 99, 100):
        diag = prob["diag"].copy()
        diag[1, r:] = -1e6
        got = grad_call(hip, *args, diag, N)
        # (the C oracle adds sum a to the diagonal itself: diag_add of these problems)
        _, info = cref.loglike(gc.coefficients(prob, 1), prob["t"], diag[1], prob["y"][1])
        assert info >= r + 1 and got["info"][1] == info, (r, got["info"], info)
        assert got["ll"][1] == -np.inf
        for k in ("real", "comp"):
            assert np.all(np.isnan(got[k][:, 1])), (r, k)
        assert np.isnan(got["diag_add"][1]) and np.isnan(got["mean"][1])
        assert _identical(got, base, rows=[0, 2]), r


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    N, B = 50, 2
    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")      # noqa: E731
    real, comp, da, t, y = f(2, B, 1), f(4, B, 32), f(B), f(N), f(N)
    work = f(B * int(lib.gf_grad_work(N, 63)))
    out = [torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for n in (B, 2 * B, 4 * B * 32, B, B)]
    info = torch.full((B,), INFO_SENTINEL, dtype=torch.int32, device="cuda")

    def call(N=N, Jr=0, Jc=8, work_bs=None, y=y):
        wb = int(lib.gf_grad_work(N, Jr + 2 * Jc)) if work_bs is None else work_bs
        return lib.gf_loglike_grad(B, N, Jr, Jc, p(real[0]), p(real[1]), p(comp[0]), p(comp[1]), p(comp[2]),
                                   p(comp[3]), p(da), p(t), 0, None, 0, p(y), 0, p(work), wb, *[p(o) for o in out],
                                   p(info), None)

    assert call(Jc=32, work_bs=int(lib.gf_grad_work(N, 63))) == -3 and "63" in hip.last_error()
    need = int(lib.gf_grad_work(N, 16))
    for kw in (dict(work_bs=need - 1), dict(N=0, work_bs=need), dict(y=None)):
        assert call(**kw) == -1, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out) and bool(torch.all(info == INFO_SENTINEL))


def test_workspace_size_formula():
    """gf_grad_work(N, W) = nseg (WM + 4) 64 + K (WM + 8) 64 doubles with K = ceil(sqrt(N)) exactly -- also where
    N is beyond 2^53 or sqrt's rounding could put K off by one (k^2 and k^2 +- 1 at k = 2^20 + 1 and at
    k = 94906267, whose square is above 2^53)."""
    from gadfly_amd import _lib
    lib = _lib.load()
    assert 94906267 ** 2 - 1 > 2 ** 53                 # not every N there is a double
    lengths = [1, 2, 4, 5, 16, 17, 10 ** 5]
    for k in (2 ** 20 + 1, 94906267):
        lengths += [k * k - 1, k * k, k * k + 1]
    for N in lengths:
        K = math.isqrt(N - 1) + 1
        assert (K - 1) ** 2 < N <= K * K
        nseg = -(-N // K)
        for W, WM in ((1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (63, 64)):
            assert lib.gf_grad_work(N, W) == nseg * (WM + 4) * 64 + K * (WM + 8) * 64, (N, W)
        assert lib.gf_grad_work(N, 64) == 0 and lib.gf_grad_work(N, 0) == 0
    assert lib.gf_grad_work(0, 8) == 0
