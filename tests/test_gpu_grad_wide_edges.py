"""GPU: gf_loglike_grad_wide through its raw C entry point at the shapes where it can go wrong --
both sides of the boundaries of its three instances (W = 64 | 65, 128 | 129), the 86-term default kernel's width, the
largest width and an odd one beside it, lengths at the edges of the segments and every segment rule at N = 101 --
against the float64 numpy reverse pass and dense autograd (tests/grad_ref.py), against the one-wave kernel where both
run, bit-identity across the segment length and the batch, a workspace full of NaN, and the failing pivot."""
import functools

import numpy as np
import pytest
import torch

from tests import grad_cases as gc
from tests.grad_ref import loglike_grad

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
INFO_SENTINEL = -77
KEYS = ("ll", "real", "comp", "diag_add", "mean", "info")

#: W = 2, 17, 63 (narrow); 64, 64, 65 and 128, 128, 129: both sides of the instance boundaries, with and without real
#: terms; 172 and 176: the 86-term default kernel, bare and with four real terms; 192, the largest, and 191 beside it
STRUCTURES = ((0, 1), (1, 8), (3, 30), (0, 32), (2, 31), (1, 32), (0, 64), (2, 63), (1, 64), (0, 86), (4, 86), (0, 96),
              (1, 95))
LENGTHS = (1, 2, 3, 5, 17, 101, 197)
SEGS = (1, 2, 7, 50, 101, 1000)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def wide_call(hip, prob, seg=0, rows=slice(None), diag=None):
    """One gf_loglike_grad_wide call on the problems ``rows`` of a grad_cases.edge_problem (shared t, per-problem y and
    diag) at ``seg`` rows per segment.  The workspace is full of NaN on entry and every output is one problem too long
    and pre-filled with a sentinel, as in tests/test_gpu_grad_edges.py."""
    lib, p = hip.load(), hip.ptr
    Jr, Jc, N = prob["Jr"], prob["Jc"], prob["N"]
    real, comp, da = prob["real"][:, rows], prob["comp"][:, rows], prob["diag_add"][rows]
    y, dg = prob["y"][rows], (prob["diag"] if diag is None else diag)[rows]
    B, lr, lc = real.shape[1], max(Jr, 1), max(Jc, 1)
    per = int(lib.gf_grad_wide_work(N, Jr + 2 * Jc, seg))
    assert per > 0
    work = torch.full((B * per,), float("nan"), dtype=torch.float64, device="cuda")
    rd, cd, ad, td, yd, dd = _dev(real), _dev(comp), _dev(da), _dev(prob["t"]), _dev(y), _dev(dg)
    f = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")      # noqa: E731
    ll, g_real, g_comp, g_diag, g_mean = f(B + 1), f(2 * (B + 1) * lr), f(4 * (B + 1) * lc), f(B + 1), f(B + 1)
    info = torch.full((B + 1,), INFO_SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.gf_loglike_grad_wide(B, N, seg, Jr, Jc, p(rd[0]), p(rd[1]), p(cd[0]), p(cd[1]), p(cd[2]), p(cd[3]),
                                  p(ad), p(td), 0, p(dd), N, p(yd), N, p(work), per, p(ll), p(g_real), p(g_comp),
                                  p(g_diag), p(g_mean), p(info), None)
    hip.check(rc, "gf_loglike_grad_wide")
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


def _same(a, ia, b, ib):
    """Problem ia of result a and problem ib of result b agree to the bit (NaN = NaN)."""
    return all(np.array_equal(a[k][..., ia, :] if a[k].ndim == 3 else a[k][ia],
                              b[k][..., ib, :] if b[k].ndim == 3 else b[k][ib], equal_nan=True) for k in KEYS)


def _errors(prob, b, got, ll, g):
    """(log L relative, the largest of the six scaled adjoint errors and of mean, diag_add) of problem b."""
    co = gc.coefficients(prob, b)
    dev = dict(ar=got["real"][0, b], cr=got["real"][1, b], ac=got["comp"][0, b], bc=got["comp"][1, b],
               cc=got["comp"][2, b], dc=got["comp"][3, b])
    adj = [gc.scaled_error(c, dev[k], g[k]) for k, c in zip(gc.NAMES, co)]
    adj += [abs(got[k][b] - g[k]) / max(1.0, abs(g[k])) for k in ("mean", "diag_add")]
    return abs(got["ll"][b] - ll) / abs(ll), max(adj)


@functools.lru_cache(maxsize=None)
def _references(Jr, Jc, N):
    """(problem, [(ll, g) of the float64 numpy pass per problem], (ll, g) of dense autograd of problem 0 or None)."""
    prob = gc.edge_problem(Jr, Jc, N)
    ref = [loglike_grad(prob["t"], prob["y"][b], prob["diag"][b], Jr, Jc, *gc.coefficients(prob, b),
                        prob["diag_add"][b]) for b in range(prob["B"])]
    return prob, ref, (gc.dense_grad(prob, 0) if N <= 101 else None)


@pytest.mark.parametrize("Jr,Jc", STRUCTURES)
def test_edge_shapes_match_both_oracles(hip, Jr, Jc):
    """B = 3 at every length of LENGTHS and the default segments: log L to 1e-9 and every adjoint to 1e-7 (scaled) of
    the float64 numpy pass, and for N <= 101 of dense autograd for problem 0."""
    bad, worst = [], [0.0, 0.0, 0.0, 0.0]
    for N in LENGTHS:
        prob, ref, dense = _references(Jr, Jc, N)
        got = wide_call(hip, prob)
        assert np.all(got["info"] == 0), (N, got["info"])
        for b in range(prob["B"]):
            errs = list(_errors(prob, b, got, *ref[b]))
            if b == 0 and dense is not None:
                errs += list(_errors(prob, 0, got, *dense))
            worst = [max(w, e) for w, e in zip(worst, errs + [0.0] * (4 - len(errs)))]
            if any(e > bar for e, bar in zip(errs, (1e-9, 1e-7, 1e-9, 1e-7))):
                bad.append((N, b, errs))
    print(f"(Jr, Jc) = ({Jr}, {Jc}), W = {Jr + 2 * Jc}: numpy pass log L {worst[0]:.1e}, adjoints {worst[1]:.1e}; "
          f"dense autograd log L {worst[2]:.1e}, adjoints {worst[3]:.1e}")
    assert not bad, bad


@pytest.mark.parametrize("Jr,Jc", STRUCTURES)
def test_segment_rules_and_batch_independence(hip, Jr, Jc):
    """N = 101 at 1, 2, 7, 50, 101 and 1000 rows per segment: the bars against both references, every output equal to
    the bit over all the segment rules, and problem 1 alone (B = 1) and as the last of two (B = 2) with the bits it has
    among three."""
    N = 101
    prob, ref, dense = _references(Jr, Jc, N)
    base = wide_call(hip, prob)
    assert np.all(base["info"] == 0)
    for seg in SEGS:
        got = wide_call(hip, prob, seg=seg)
        for b in range(prob["B"]):
            e = _errors(prob, b, got, *ref[b])
            assert e[0] <= 1e-9 and e[1] <= 1e-7, (seg, b, e)
            assert _same(got, b, base, b), (seg, b)
        e = _errors(prob, 0, got, *dense)
        assert e[0] <= 1e-9 and e[1] <= 1e-7, (seg, e)
    assert _same(wide_call(hip, prob, rows=slice(1, 2)), 0, base, 1)
    assert _same(wide_call(hip, prob, rows=slice(0, 2)), 1, base, 1)
    assert _same(wide_call(hip, prob, rows=slice(1, 3), seg=7), 0, base, 1)


@pytest.mark.parametrize("Jr,Jc", [s for s in STRUCTURES if s[0] + 2 * s[1] <= 63])
def test_narrow_widths_match_the_one_wave_kernel(hip, Jr, Jc):
    """W <= 63 against gf_loglike_grad on the same problems: log L to 1e-12, adjoints to 1e-10 scaled."""
    from tests.test_gpu_grad_edges import grad_call
    worst = [0.0, 0.0]
    for N in LENGTHS:
        prob, _, _ = _references(Jr, Jc, N)
        got = wide_call(hip, prob)
        one = grad_call(hip, Jr, Jc, prob["real"], prob["comp"], prob["diag_add"], prob["t"], prob["y"], prob["diag"],
                        N)
        for b in range(prob["B"]):
            g = dict(ar=one["real"][0, b], cr=one["real"][1, b], ac=one["comp"][0, b], bc=one["comp"][1, b],
                     cc=one["comp"][2, b], dc=one["comp"][3, b], mean=one["mean"][b], diag_add=one["diag_add"][b])
            e = _errors(prob, b, got, one["ll"][b], g)
            worst = [max(w, x) for w, x in zip(worst, e)]
    print(f"(Jr, Jc) = ({Jr}, {Jc}): against the one-wave kernel log L {worst[0]:.1e}, adjoints {worst[1]:.1e}")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-10, worst


@pytest.mark.parametrize("Jr,Jc", [(1, 8), (1, 32), (4, 86)])
def test_failing_pivot_between_healthy_problems(hip, Jr, Jc):
    """N = 101 (segments of 11 rows): problem 1 of three loses positive definiteness from row r on -- the first row,
    both sides of a segment boundary, the last row: log L is -inf, info the 1-based failing row, every gradient of
    that problem NaN, and its neighbours have the bits of a call without it."""
    N = 101
    prob, _, _ = _references(Jr, Jc, N)
    base = wide_call(hip, prob)
    for r in (0, 10, 11, 100):
        diag = prob["diag"].copy()
        diag[1, r:] = -1e9                 # (far below diag_add = sum a of the widest structure)
        got = wide_call(hip, prob, diag=diag)
        assert got["info"][1] == r + 1 and got["info"][0] == 0 and got["info"][2] == 0, (r, got["info"])
        assert got["ll"][1] == -np.inf
        for k in ("real", "comp"):
            assert np.all(np.isnan(got[k][:, 1])), (r, k)
        assert np.isnan(got["diag_add"][1]) and np.isnan(got["mean"][1])
        assert _same(got, 0, base, 0) and _same(got, 2, base, 2), r
