"""CPU: what the wide gradient route's device tests rest on -- the references agree with each other
at the wide shapes, the shape queries of gf_loglike_grad_wide, and its argument checks by status, all of which return
before any launch (the pointers are dummies, as in tests/test_abi_errors_host.py)."""
import ctypes
import functools

import numpy as np
import pytest

from gadfly_amd import _lib
from tests import grad_cases as gc
from tests.grad_ref import loglike_grad

D = ctypes.c_void_p(0x1000)         # never dereferenced: every case below is refused before a launch
Z = None


@functools.lru_cache(maxsize=None)
def _passes(Jr, Jc, N):
    prob = gc.edge_problem(Jr, Jc, N)
    args = (prob["t"], prob["y"][0], prob["diag"][0], Jr, Jc, *gc.coefficients(prob, 0), prob["diag_add"][0])
    return prob, loglike_grad(*args), loglike_grad(*args, dtype=np.longdouble), gc.dense_grad(prob, 0)


def _gap(prob, a, b):
    """(log L relative, largest scaled adjoint / mean / diag_add difference) between two references of problem 0."""
    (lla, ga), (llb, gb) = a, b
    adj = [gc.scaled_error(c, np.asarray(ga[k], dtype=np.float64), np.asarray(gb[k], dtype=np.float64))
           for k, c in zip(gc.NAMES, gc.coefficients(prob, 0))]
    adj += [abs(float(ga[k]) - float(gb[k])) / max(1.0, abs(float(gb[k]))) for k in ("mean", "diag_add")]
    return abs(float(lla) - float(llb)) / abs(float(llb)), max(adj)


@pytest.mark.parametrize("Jr,Jc", [(1, 32), (0, 86), (4, 86)])
@pytest.mark.parametrize("N", [17, 101])
def test_references_agree_at_wide_shapes(Jr, Jc, N):
    """The float64 numpy pass, the 80-bit pass and dense autograd agree to 1e-10 in log L and in every adjoint: the
    device bars (1e-9, 1e-7) rest on the kernel alone."""
    prob, f64, f80, dense = _passes(Jr, Jc, N)
    gaps = [_gap(prob, f64, f80), _gap(prob, f64, dense), _gap(prob, f80, dense)]
    print(f"(Jr, Jc) = ({Jr}, {Jc}), N = {N}: " + ", ".join(f"({a:.1e}, {b:.1e})" for a, b in gaps))
    assert max(max(g) for g in gaps) <= 1e-10, gaps


def test_shape_queries():
    lib = _lib.load()
    wmax = lib.gf_grad_wide_max_width()
    assert wmax >= 176
    for N, W, seg in ((0, 8, 0), (-1, 8, 0), (10, 0, 0), (10, -3, 0), (10, wmax + 1, 0), (10, 8, -1)):
        assert lib.gf_grad_wide_work(N, W, seg) == 0, (N, W, seg)
    assert lib.gf_grad_wide_seg(0, 8) == 0 and lib.gf_grad_wide_seg(10, 0) == 0
    assert lib.gf_grad_wide_seg(10, wmax + 1) == 0
    for W in (1, 63, 64, 65, 128, 129, 172, 176, wmax):
        for seg in (0, 1, 7, 255, 10 ** 6):
            sizes = [lib.gf_grad_wide_work(N, W, seg) for N in (1, 2, 3, 16, 17, 100, 101, 1000, 65000, 10 ** 5)]
            assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (W, seg, sizes)
        for N in (1, 2, 3, 4, 5, 17, 101, 197, 65000, 10 ** 5, 2 ** 40 + 1):
            K = lib.gf_grad_wide_seg(N, W)
            assert 1 <= K <= N and (K - 1) ** 2 < N <= K * K, (N, W, K)
            # 0 means the default, values above N mean N
            assert lib.gf_grad_wide_work(N, W, 0) == lib.gf_grad_wide_work(N, W, K)
            assert lib.gf_grad_wide_work(N, W, N + 5) == lib.gf_grad_wide_work(N, W, N)
    # the same instance serves a range of widths: its workspace does not depend on the width within it
    assert lib.gf_grad_wide_work(101, 65, 0) == lib.gf_grad_wide_work(101, 128, 0)
    assert lib.gf_grad_wide_work(101, 129, 0) == lib.gf_grad_wide_work(101, wmax, 0)
    assert lib.gf_grad_wide_work(101, 64, 0) < lib.gf_grad_wide_work(101, 65, 0) < lib.gf_grad_wide_work(101, 129, 0)


def _args(B=2, N=50, seg=0, Jr=1, Jc=8, work_bs=None, null=None, p=D):
    """The call's arguments with dummy pointers; ``null``: the index of the one pointer argument that is NULL."""
    lib = _lib.load()
    if work_bs is None:
        work_bs = lib.gf_grad_wide_work(N, Jr + 2 * Jc, seg)
    a = [B, N, seg, Jr, Jc] + [p] * 7 + [p, 0, p, 0, p, 0, p, work_bs] + [p] * 6 + [Z]
    if null is not None:
        a[null] = Z
    return a


#: ar cr ac bc cc dc diag_add t y work ll g_real g_comp g_diag g_mean info (diag may be NULL: index 14 is not listed)
REQUIRED = (5, 6, 7, 8, 9, 10, 11, 12, 16, 18, 20, 21, 22, 23, 24, 25)


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    wmax = lib.gf_grad_wide_max_width()
    assert len(_args()) == len(_lib.SIGNATURES["gf_loglike_grad_wide"][1])
    for kw in (dict(B=0), dict(N=0), dict(N=-4), dict(seg=-1), dict(Jr=-1), dict(Jc=-1), dict(Jr=0, Jc=0)):
        assert lib.gf_loglike_grad_wide(*_args(work_bs=1 << 40, **kw)) == -1, kw
        assert "bad shape" in _lib.last_error(), kw
    need = lib.gf_grad_wide_work(50, 17, 0)
    assert lib.gf_loglike_grad_wide(*_args(work_bs=need - 1)) == -1
    assert "work_bs" in _lib.last_error() and str(need) in _lib.last_error()
    need7 = lib.gf_grad_wide_work(50, 17, 7)
    assert need7 != need and lib.gf_loglike_grad_wide(*_args(seg=7, work_bs=need7 - 1)) == -1
    for i in REQUIRED:
        assert lib.gf_loglike_grad_wide(*_args(null=i)) == -1, i
        assert "null pointer" in _lib.last_error(), i
    # (without real terms ar and cr may be NULL, without complex ones ac .. dc: these pass the pointer check and are
    # not run here)
    for Jr, Jc in ((wmax + 1, 0), (1, wmax // 2), (wmax - 1, 1)):
        assert Jr + 2 * Jc == wmax + 1
        assert lib.gf_loglike_grad_wide(*_args(Jr=Jr, Jc=Jc, work_bs=1 << 40)) == -3, (Jr, Jc)
        assert str(wmax) in _lib.last_error()
    assert lib.gf_loglike_grad_wide(*_args(Jr=0, Jc=2 ** 30, work_bs=1 << 40)) == -3      # (no overflow of Jr + 2 Jc)


def test_host_refusals_of_the_python_route():
    """check_width names the route to take, and the wide route's own limit."""
    from gadfly_amd import grad
    wmax = grad.wide_max_width()
    grad.check_width(63)
    grad.check_width(wmax, wide=True)
    with pytest.raises(NotImplementedError, match="63"):
        grad.check_width(64)
    with pytest.raises(NotImplementedError, match="63.*wide=True"):
        grad.check_width(64, hint=True)
    with pytest.raises(NotImplementedError, match=str(wmax)):
        grad.check_width(wmax + 1, wide=True)
    per, group, ngroups = grad.workspace_plan(101, 172, 5, cap_bytes=1, wide=True)
    assert per == _lib.load().gf_grad_wide_work(101, 172, 0) and (group, ngroups) == (1, 5)
    assert grad.workspace_plan(101, 172, 5, wide=True, seg=7)[0] == _lib.load().gf_grad_wide_work(101, 172, 7)
    with pytest.raises(NotImplementedError):
        grad.workspace_plan(101, 172, 5)
