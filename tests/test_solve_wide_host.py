"""CPU: the host side of the wide conditional-mean route -- the width checks' texts, the workspace
plan, the shape queries of gf_solve_batch_wide and its argument checks by status, all of which return before any launch
(the pointers are dummies, as in tests/test_grad_wide_host.py), and the cut of a coefficient pack into groups of whole
terms."""
import ctypes

import numpy as np
import pytest

from gadfly_amd import _lib, predict

D = ctypes.c_void_p(0x1000)         # never dereferenced: every case below is refused before a launch
Z = None


def test_check_width_texts():
    wmax = _lib.load().gf_solve_wide_max_width()
    assert wmax == 192
    predict.check_width(63)
    predict.check_width(63, wide=True)
    predict.check_width(wmax, wide=True)
    with pytest.raises(NotImplementedError) as e:
        predict.check_width(172)
    assert str(e.value) == ("batched conditional means take celerite widths W <= 63 (one wave per problem); "
                            "this kernel has W = 172")
    with pytest.raises(NotImplementedError) as e:
        predict.check_width(64, "the component")
    assert str(e.value).endswith("the component has W = 64")
    with pytest.raises(NotImplementedError, match=f"wide=True.*W <= {wmax}.*this kernel has W = {wmax + 1}"):
        predict.check_width(wmax + 1, wide=True)
    with pytest.raises(NotImplementedError, match=f"{wmax}.*the component has W = 194"):
        predict.check_width(194, "the component", wide=True)


def test_workspace_plan_of_the_wide_route():
    lib = _lib.load()
    per, group, ngroups = predict.workspace_plan(101, 172, 5, cap_bytes=1, wide=True)
    assert per == lib.gf_solve_wide_work(101, 172, 0) and (group, ngroups) == (1, 5)
    assert predict.workspace_plan(101, 172, 5, wide=True, seg=7)[0] == lib.gf_solve_wide_work(101, 172, 7)
    assert predict.workspace_plan(101, 172, 5, wide=True)[1:] == (5, 1)
    assert predict.workspace_plan(101, 17, 5, wide=True)[0] == lib.gf_solve_wide_work(101, 17, 0)
    with pytest.raises(NotImplementedError, match="W = 172"):
        predict.workspace_plan(101, 172, 5)
    with pytest.raises(NotImplementedError, match="192"):
        predict.workspace_plan(101, 193, 5, wide=True)


def _formula(N, W, K):
    """The workspace the header documents: checkpoints of (NC + 4) RT, one segment of staged rows at 3 RT, z and D."""
    rt = 64 if W <= 64 else 128 if W <= 128 else 192
    return -(-N // K) * (rt + 4) * rt + K * 3 * rt + 2 * (-(-N // 64) * 64)


def test_shape_queries():
    lib = _lib.load()
    wmax = lib.gf_solve_wide_max_width()
    for N, W, seg in ((0, 8, 0), (-1, 8, 0), (10, 0, 0), (10, -3, 0), (10, wmax + 1, 0), (10, 8, -1)):
        assert lib.gf_solve_wide_work(N, W, seg) == 0, (N, W, seg)
    for N, W in ((0, 8), (-1, 8), (10, 0), (10, -3), (10, wmax + 1)):
        assert lib.gf_solve_wide_seg(N, W) == 0, (N, W)
    for W in (1, 63, 64, 65, 128, 129, 172, 176, wmax):
        for N in (1, 2, 3, 4, 5, 17, 101, 197, 65000, 10 ** 5, 2 ** 40 + 1):
            K = lib.gf_solve_wide_seg(N, W)
            assert 1 <= K <= N, (N, W, K)
            # 0 means the default, values above N mean N, and the default is a minimum of the documented sum
            assert lib.gf_solve_wide_work(N, W, 0) == lib.gf_solve_wide_work(N, W, K) == _formula(N, W, K)
            assert lib.gf_solve_wide_work(N, W, N + 5) == lib.gf_solve_wide_work(N, W, N) == _formula(N, W, N)
            for other in (1, 2, 7, 100, 1000, N):
                k = min(other, N)
                assert lib.gf_solve_wide_work(N, W, other) == _formula(N, W, k)
                # (the rule balances N / K checkpoints against K staged rows: 2 sqrt(N CK RS) at the least for any
                # length; rounding N / K up adds one checkpoint at the most, rounding K up one staged row)
                rt = 64 if W <= 64 else 128 if W <= 128 else 192
                assert _formula(N, W, K) <= _formula(N, W, k) + (rt + 4) * rt + 3 * rt, (N, W, K, k)
    # the same instance serves a range of widths: its workspace does not depend on the width within it
    assert lib.gf_solve_wide_work(101, 65, 0) == lib.gf_solve_wide_work(101, 128, 0)
    assert lib.gf_solve_wide_work(101, 129, 0) == lib.gf_solve_wide_work(101, wmax, 0)
    assert lib.gf_solve_wide_work(101, 64, 0) < lib.gf_solve_wide_work(101, 65, 0) < lib.gf_solve_wide_work(101, 129, 0)


def _args(B=2, N=50, Jr=1, Jc=8, seg=0, work_bs=None, null=None, p=D, strides=(0, 0, 0)):
    """The call's arguments with dummy pointers; ``null``: the index of the one pointer argument that is NULL."""
    lib = _lib.load()
    if work_bs is None:
        work_bs = lib.gf_solve_wide_work(N, Jr + 2 * Jc, seg)
    a = [B, N, Jr, Jc] + [p] * 7 + [p, strides[0], p, strides[1], p, strides[2], seg, p, work_bs] + [p] * 4 + [Z]
    if null is not None:
        a[null] = Z
    return a


#: ar cr ac bc cc dc diag_add t y work ll info (diag, alpha and mu may be NULL: 13, 20 and 21 are not listed)
REQUIRED = (4, 5, 6, 7, 8, 9, 10, 11, 15, 18, 22, 23)


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    wmax = lib.gf_solve_wide_max_width()
    assert len(_args()) == len(_lib.SIGNATURES["gf_solve_batch_wide"][1])
    for kw in (dict(B=0), dict(B=-2), dict(N=0), dict(N=-4), dict(seg=-1), dict(Jr=-1), dict(Jc=-1),
               dict(Jr=0, Jc=0)):
        assert lib.gf_solve_batch_wide(*_args(work_bs=1 << 40, **kw)) == -1, kw
        assert "bad shape" in _lib.last_error(), kw
    for strides in ((49, 0, 0), (0, -1, 0), (0, 0, 7)):
        assert lib.gf_solve_batch_wide(*_args(strides=strides)) == -1, strides
        assert "stride" in _lib.last_error(), strides
    need = lib.gf_solve_wide_work(50, 17, 0)
    assert lib.gf_solve_batch_wide(*_args(work_bs=need - 1)) == -1
    assert "work_bs" in _lib.last_error() and str(need) in _lib.last_error()
    need7 = lib.gf_solve_wide_work(50, 17, 7)
    assert need7 != need and lib.gf_solve_batch_wide(*_args(seg=7, work_bs=need7 - 1)) == -1
    for i in REQUIRED:
        assert lib.gf_solve_batch_wide(*_args(null=i)) == -1, i
        assert "null pointer" in _lib.last_error(), i
    for Jr, Jc in ((wmax + 1, 0), (1, wmax // 2), (wmax - 1, 1)):
        assert Jr + 2 * Jc == wmax + 1
        assert lib.gf_solve_batch_wide(*_args(Jr=Jr, Jc=Jc, work_bs=1 << 40)) == -3, (Jr, Jc)
        assert str(wmax) in _lib.last_error()
    assert lib.gf_solve_batch_wide(*_args(Jr=0, Jc=2 ** 30, work_bs=1 << 40)) == -3       # (no overflow of Jr + 2 Jc)


@pytest.mark.parametrize("Jr,Jc", [(0, 86), (4, 86), (63, 0), (64, 0), (1, 95), (1, 31), (3, 30)])
def test_term_groups(Jr, Jc):
    """Every term exactly once and in order, widths <= 63, no complex term split (a group holds whole terms only), and
    a pack that fits comes back as one group holding the same arrays."""
    B = 3
    rng = np.random.default_rng(5)
    real, comp = rng.normal(size=(2, B, max(Jr, 1))), rng.normal(size=(4, B, max(Jc, 1)))
    groups = predict.term_groups(Jr, Jc, real, comp)
    if Jr + 2 * Jc <= 63:
        assert len(groups) == 1
        g = groups[0]
        assert g[:2] == (Jr, Jc) and g[2] is real and g[3] is comp
        return
    assert len(groups) >= -(-(Jr + 2 * Jc) // 63)
    seen_complex = False
    for jr, jc, r, c in groups:
        assert jr >= 0 and jc >= 0 and 1 <= jr + 2 * jc <= 63
        assert r.shape == (2, B, max(jr, 1)) and c.shape == (4, B, max(jc, 1))
        assert not (seen_complex and jr), "a real term behind a complex one"
        seen_complex = seen_complex or jc > 0
    assert sum(g[0] for g in groups) == Jr and sum(g[1] for g in groups) == Jc
    assert np.array_equal(np.concatenate([g[2][:, :, :g[0]] for g in groups], axis=2), real[:, :, :Jr])
    assert np.array_equal(np.concatenate([g[3][:, :, :g[1]] for g in groups], axis=2), comp[:, :, :Jc])
    # groups are as full as whole terms allow: no more of them than a greedy cut needs
    assert len(groups) <= -(-Jr // 63) + -(-Jc // 31)
    # a narrower cut is honoured too
    for jr, jc, _, _ in predict.term_groups(Jr, Jc, real, comp, max_width=16):
        assert 1 <= jr + 2 * jc <= 16
