"""GPU: gf_loglike_grad_chunked through its raw C entry point at the shapes where it can go wrong --
every width at a boundary of the three kernel instances (tests/grad_cases.STRUCTURES), chunk counts 1, 2, 3, 4, 5, 7, 8, 9,
13, 77 and 100, one row per chunk, last chunks of one row, a single chunk -- against the numpy sequential pass and
dense autograd (tests/grad_ref.py); its calling conventions (strides, diag = NULL, a dirty and over-long workspace,
output layout, batch independence), the failing pivot at the edges of a chunk, and its argument checks."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import cref
from tests import grad_cases as gc
from tests.grad_ref import loglike_grad
from tests.test_gpu_grad_edges import (INFO_SENTINEL, KEYS, SENTINEL, _bs, _dev, _errors, _identical, grad_call)

pytestmark = pytest.mark.gpu

#: (N, chunk_len) -> chunks: 13 (last of 5 rows), 4, 100 (one row each), 2 (last of one row), 8 (all full), 9;
#: 1 (one row), 2 (one row each), 3 (last of one row), 4 (last of one row), 5, 1 (chunk_len = N), 7.  Up to 7 chunks
#: the start states come from the sequential combine, from 8 on from the tree (8: no padding; 9, 13, 100: padding)
SHAPES = ((197, 16), (197, 50), (100, 1), (101, 100), (64, 8), (300, 37),
          (1, 1), (2, 1), (5, 2), (13, 4), (10, 2), (197, 197), (56, 8))


def tp_call(hip, Jr, Jc, real, comp, diag_add, t, y, diag, N, L, work_extra=0, work_fill=float("nan")):
    """One gf_loglike_grad_chunked call on host arrays, as tests/test_gpu_grad_edges.grad_call: every output one
    problem too long and pre-filled with a sentinel; the workspace holds ``work_fill`` (NaN: nothing may be read before
    it is written) and is ``work_extra`` doubles per problem longer than gf_grad_chunked_work asks."""
    lib, p = hip.load(), hip.ptr
    B, lr, lc = real.shape[1], max(Jr, 1), max(Jc, 1)
    assert real.shape == (2, B, lr) and comp.shape == (4, B, lc) and diag_add.shape == (B,)
    per = int(lib.gf_grad_chunked_work(N, Jr + 2 * Jc, L))
    assert per > 0
    per += work_extra
    work = torch.full((B * per,), work_fill, dtype=torch.float64, device="cuda")
    rd, cd, ad, td, yd = _dev(real), _dev(comp), _dev(diag_add), _dev(t), _dev(y)
    dd = None if diag is None else _dev(diag)
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    ll, g_real, g_comp, g_diag, g_mean = f(B + 1), f(2 * (B + 1) * lr), f(4 * (B + 1) * lc), f(B + 1), f(B + 1)
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_loglike_grad_chunked(B, N, L, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]),
                                     p(ad), p(td), _bs(t), p(dd), 0 if diag is None else _bs(diag), p(yd), _bs(y),
                                     p(work), per, p(ll), p(g_real), p(g_comp), p(g_diag), p(g_mean), p(info), None)
    hip.check(rc, "gf_loglike_grad_chunked")
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


@functools.lru_cache(maxsize=None)
def _numpy_pass(Jr, Jc, N, b):
    """The sequential float64 pass of problem b of edge_problem(Jr, Jc, N): computed once, shared, never changed."""
    prob = gc.edge_problem(Jr, Jc, N)
    return loglike_grad(prob["t"], prob["y"][b], prob["diag"][b], Jr, Jc, *gc.coefficients(prob, b),
                        prob["diag_add"][b])


def _check_shapes(hip, Jr, Jc, shapes):
    bad, worst = [], [0.0, 0.0, 0.0, 0.0]
    for N, L in shapes:
        prob = gc.edge_problem(Jr, Jc, N)
        got = tp_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"], prob["diag"],
                      N, L)
        assert np.all(got["info"] == 0), (N, L, got["info"])
        for b in range(prob["B"]):
            errs = list(_errors(prob, b, got, *_numpy_pass(Jr, Jc, N, b)))
            if b == 0:
                errs += list(_errors(prob, 0, got, *gc.dense_grad(prob, 0)))
            worst = [max(w, e) for w, e in zip(worst, errs + [0.0] * (4 - len(errs)))]
            if any(not e <= bar for e, bar in zip(errs, (1e-9, 1e-7, 1e-9, 1e-7))):
                bad.append((N, L, b, errs))
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: numpy pass log L {worst[0]:.1e}, adjoints {worst[1]:.1e}; "
          f"dense autograd log L {worst[2]:.1e}, adjoints {worst[3]:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", gc.STRUCTURES)
def test_edge_shapes_match_both_oracles(hip, Jr, Jc):
    """B = 3 problems of different coefficients, data and diagonals on a shared axis at every (N, chunk_len) of SHAPES:
    log L to 1e-9 and every adjoint to 1e-7 (scaled) of the float64 numpy sequential pass, and of dense autograd for
    problem 0 (the project's bars for the one-wave route; the chunked algebra itself sits 2.7e-13 from the sequential
    pass in numpy, tests/test_grad_tp_host.py)."""
    _check_shapes(hip, Jr, Jc, SHAPES)


def test_many_chunks_not_a_power_of_two(hip):
    """N = 1000 in chunks of 13 rows: 77 chunks, the last of 12 rows -- more than a wave's worth for the flag kernel's
    strided search, and a long way for both scans."""
    _check_shapes(hip, 0, 8, ((1000, 13),))


@pytest.mark.parametrize("Jr,Jc", [(0, 8), (1, 16), (1, 31)])
def test_call_conventions(hip, Jr, Jc):
    """(197, 16): 13 chunks; (13, 4): a last chunk of one row."""
    for N, L in ((197, 16), (13, 4)):
        prob = gc.edge_problem(Jr, Jc, N)
        B = prob["B"]
        real, comp, da = prob["real"], prob["comp"], prob["diag_add"]
        t, y, diag = prob["t"], prob["y"][0], prob["diag"][0]
        base = tp_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, L)
        assert np.all(base["info"] == 0)
        assert all(np.all(np.isfinite(base[k])) for k in KEYS)
        # two calls give identical bits
        assert _identical(base, tp_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, L)), N
        # t, y, diag shared (stride 0) against B copies at a stride of N + 3 (the three pad elements are never read)
        wide = [np.full((B, N + 3), np.nan) for _ in range(3)]
        for w, x in zip(wide, (t, y, diag)):
            w[:, :N] = x
        assert _identical(base, tp_call(hip, Jr, Jc, real, comp, da, *wide, N, L)), N
        # another work_bs, and a zeroed workspace against the NaN-filled one
        assert _identical(base, tp_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, L, work_extra=17,
                                        work_fill=0.0)), N
        # the same problems alone
        for b in range(B):
            one = tp_call(hip, Jr, Jc, real[:, b:b + 1], comp[:, b:b + 1], da[b:b + 1], t, y, diag, N, L)
            assert all(np.array_equal(one[k][..., 0, :] if one[k].ndim == 3 else one[k][0],
                                      base[k][..., b, :] if base[k].ndim == 3 else base[k][b]) for k in KEYS), (N, b)
        # diag = NULL against an array of zeros
        da2 = da * 1.05
        null = tp_call(hip, Jr, Jc, real, comp, da2, t, y, None, N, L)
        assert np.all(null["info"] == 0)
        assert _identical(null, tp_call(hip, Jr, Jc, real, comp, da2, t, y, np.zeros(N), N, L)), N
        # a chunk length beyond N means one chunk
        assert _identical(tp_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, N),
                          tp_call(hip, Jr, Jc, real, comp, da, t, y, diag, N, N + 40)), N


@pytest.mark.parametrize("Jr,Jc", [(2, 7), (0, 31)])
def test_failing_pivot_at_chunk_edges(hip, Jr, Jc):
    """N = 197 in 13 chunks of 16 rows.  One problem of three loses positive definiteness from row r on: the first
    row, inside and the last row of chunk 0 (0, 5, 15), the first and the last row of a later chunk (32, 47), inside
    one (100), the first and the last row of the short last chunk (192, 196).  info is the one-wave route's and the C
    oracle's failing row, log L is -inf, every gradient of that problem NaN, and its neighbours keep their bits."""
    N, L = 197, 16
    prob = gc.edge_problem(Jr, Jc, N)
    args = (Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"])
    base = tp_call(hip, *args, prob["diag"], N, L)
    assert np.all(base["info"] == 0)
    for r in (0, 5, 15, 32, 47, 100, 192, 196):
        diag = prob["diag"].copy()
        diag[1, r:] = -1e6
        got = tp_call(hip, *args, diag, N, L)
        one = grad_call(hip, *args, diag, N)
        _, info = cref.loglike(gc.coefficients(prob, 1), prob["t"], diag[1], prob["y"][1])
        assert info >= r + 1 and got["info"][1] == info == one["info"][1], (r, got["info"], one["info"], info)
        assert got["ll"][1] == -np.inf
        for k in ("real", "comp"):
            assert np.all(np.isnan(got[k][:, 1])), (r, k)
        assert np.isnan(got["diag_add"][1]) and np.isnan(got["mean"][1])
        assert _identical(got, base, rows=[0, 2]), r


def test_argument_checks_return_before_any_launch(hip):
    lib, p = hip.load(), hip.ptr
    N, B, L = 50, 2, 8
    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")      # noqa: E731
    real, comp, da, t, y = f(2, B, 1), f(4, B, 32), f(B), f(N), f(N)
    work = f(B * int(lib.gf_grad_chunked_work(N, 63, L)))
    out = [torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda") for n in (B, 2 * B, 4 * B * 32, B, B)]
    info = torch.full((B,), INFO_SENTINEL, dtype=torch.int32, device="cuda")

    def call(N=N, L=L, Jr=0, Jc=8, work_bs=None, y=y):
        wb = int(lib.gf_grad_chunked_work(N, Jr + 2 * Jc, L)) if work_bs is None else work_bs
        return lib.gf_loglike_grad_chunked(B, N, L, Jr, Jc, p(real[0]), p(real[1]), p(comp[0]), p(comp[1]),
                                           p(comp[2]), p(comp[3]), p(da), p(t), 0, None, 0, p(y), 0, p(work), wb,
                                           *[p(o) for o in out], p(info), None)

    assert call(Jc=32, work_bs=int(lib.gf_grad_chunked_work(N, 63, L))) == -3 and "63" in hip.last_error()
    need = int(lib.gf_grad_chunked_work(N, 16, L))
    for kw in (dict(work_bs=need - 1), dict(N=0, work_bs=need), dict(L=0, work_bs=need), dict(y=None)):
        assert call(**kw) == -1, kw
        assert hip.last_error(), kw
    torch.cuda.synchronize()
    assert all(bool(torch.all(o == SENTINEL)) for o in out) and bool(torch.all(info == INFO_SENTINEL))


def test_workspace_and_chunk_rule():
    """gf_grad_chunked_work(N, W, L) = nch (3 * 4096 + 3 * 64 + 512 + nseg (WM + 4) 64 + K (WM + 8) 64) + 64 doubles
    with nch = ceil(N / L), K = ceil(sqrt(L)), nseg = ceil(L / K), L held to N -- and, from 8 chunks on, the tree
    combine's states and padding slots, nch (4096 + 64) + (P - nch) (4 * 4096 + 3 * 64) + 8 with P the power of two
    not below nch; gf_grad_chunk_len gives a length whose chunk count is at most max(1, 1024 / B) and at most
    ceil(N / 64)."""
    from gadfly_amd import _lib
    lib = _lib.load()
    for N, L in ((1, 1), (5, 2), (197, 16), (197, 500), (197, 29), (197, 25), (10 ** 5, 98), (10 ** 6, 1000)):
        Le = min(L, N)
        K = math.isqrt(Le - 1) + 1
        nseg, nch = -(-Le // K), -(-N // Le)
        P = 1 << (nch - 1).bit_length()
        tree = nch * (4096 + 64) + (P - nch) * (4 * 4096 + 3 * 64) + 8 if nch >= 8 else 0
        assert P // 2 < nch <= P or nch == 1
        for W, WM in ((1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (63, 64)):
            want = nch * (3 * 4096 + 3 * 64 + 512 + nseg * (WM + 4) * 64 + K * (WM + 8) * 64) + 64 + tree
            assert lib.gf_grad_chunked_work(N, W, L) == want, (N, W, L)
        assert lib.gf_grad_chunked_work(N, 64, L) == 0 and lib.gf_grad_chunked_work(N, 8, 0) == 0
    assert lib.gf_grad_chunked_work(0, 8, 4) == 0
    for B, N in ((1, 10 ** 5), (1, 10 ** 6), (64, 4096), (2048, 1000), (1, 50), (3, 197)):
        L = lib.gf_grad_chunk_len(B, N, 60)
        nch = -(-N // L)
        assert 1 <= L <= N and nch <= max(1, 1024 // B) and nch <= -(-N // 64), (B, N, L)
    assert lib.gf_grad_chunk_len(1, 100, 64) == 0 and lib.gf_grad_chunk_len(0, 100, 8) == 0
