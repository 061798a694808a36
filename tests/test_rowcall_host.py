"""CPU: the host side the one-wave batch calls share (gadfly_amd/rowcall.py) -- the group plan against hand values,
the validation of the query axes and of a stacked pack, and every message word for word (the strings are the ones
predict.py and grad.py raised when each held its own copy of this code)."""
import numpy as np
import pytest

from gadfly_amd import _lib, grad, predict, rowcall


def _raises(exc, text, fn, *args, **kw):
    with pytest.raises(exc) as err:
        fn(*args, **kw)
    assert str(err.value) == text


def test_group_plan_against_hand_values():
    per, B = 1000, 5                                     # 8000 bytes per problem
    for cap, want in ((0, (1, 5)), (7999, (1, 5)), (8000, (1, 5)), (15999, (1, 5)), (16000, (2, 3)), (23999, (2, 3)),
                      (24000, (3, 2)), (32000, (4, 2)), (39999, (4, 2)), (40000, (5, 1)), (10 ** 12, (5, 1))):
        assert rowcall.group_plan(per, B, cap, "none") == (per,) + want, cap
    assert rowcall.group_plan(7, 1, 1 << 34, "none") == (7, 1, 1)
    for per in (0, -1):
        _raises(ValueError, "no workspace of this kind", rowcall.group_plan, per, B, 1 << 34, "no workspace of this kind")


def test_public_plans_are_the_library_size_and_the_group_plan():
    lib = _lib.load()
    N, W, B, M = 130, 4, 5, 65
    sizes = ((predict.workspace_plan, (N, W, B), lib.gf_solve_batch_work(N, W, 0)),
             (predict.variance_plan, (N, W, B, M), lib.gf_var_batch_work(N, W, M, 0)),
             (predict.variance_plan, (N, W, B, 0), lib.gf_var_batch_work(N, W, 0, 0)),
             (grad.workspace_plan, (N, W, B), lib.gf_grad_work(N, W)))
    for plan, args, per in sizes:
        assert per > 0
        assert plan(*args) == (per, 5, 1)                              # the default cap: one group
        assert plan(*args, cap_bytes=8 * per - 1) == (per, 1, 5)       # below one problem: still one per group
        assert plan(*args, cap_bytes=2 * 8 * per) == (per, 2, 3)       # exactly two problems
        assert plan(*args, cap_bytes=3 * 8 * per - 1) == (per, 2, 3)
        assert plan(*args, cap_bytes=8 * 8 * per) == (per, 5, 1)       # above the batch
    assert predict.workspace_plan(N, W, B, seg=1) == (lib.gf_solve_batch_work(N, W, 1), 5, 1)
    _raises(ValueError, "no solve workspace for N = 0, W = 4, seg = 0", predict.workspace_plan, 0, W, B)
    _raises(ValueError, "no variance workspace for N = 0, W = 4, M = 3, seg = 0", predict.variance_plan, 0, W, B, 3)
    _raises(ValueError, "no gradient workspace for N = 0, W = 4", grad.workspace_plan, 0, W, B)
    # the two width checks word theirs differently
    wide = ("batched conditional means take celerite widths W <= 63 (one wave per problem); this kernel has W = 64",
            "gradients take celerite widths W <= 63 (one wave per problem); this kernel has W = 64")
    _raises(NotImplementedError, wide[0], predict.workspace_plan, N, 64, B)
    _raises(NotImplementedError, wide[0], predict.variance_plan, N, 64, B)
    _raises(NotImplementedError, wide[1], grad.workspace_plan, N, 64, B)
    _raises(NotImplementedError, "batched conditional means take celerite widths W <= 63 (one wave per problem); "
            "the component has W = 70", predict.check_width, 70, "the component")


def test_query_axes_validation():
    B, N, M = 3, 10, 7
    check = rowcall.check_query_axes
    assert check(B, N, (M,)) == (M, None, None) == check(B, N, (1, M)) == check(B, N, (B, M))
    assert check(B, N, None, empty_ok=True) == (0, None, None)
    m, nobs, nq = check(B, N, (B, M), nobs=[10, 0, 3], nq=np.array([7, 0, 1], dtype=np.int32))
    assert m == M and nobs.dtype == nq.dtype == np.int64 and nobs.flags.c_contiguous
    assert nobs.tolist() == [10, 0, 3] and nq.tolist() == [7, 0, 1]
    for empty_ok in (False, True):
        for shape in ((), (2, 3, 4), (2, M), (4, M), (B, M, 1)):       # wrong rank, wrong leading dimension
            _raises(ValueError, f"query times of shape {shape} for a batch of 3 problems", check, B, N, shape,
                    empty_ok=empty_ok)
        for kw in (dict(nq=[7, 8, 1]), dict(nobs=[10, -1, 3]), dict(nobs=[11, 1, 3]), dict(nq=[0, -1, 0]),
                   dict(nq=[1, 2]), dict(nobs=[[1, 2, 3]]), dict(nq=5)):
            _raises(ValueError, "dimension mismatch", check, B, N, (B, M), empty_ok=empty_ok, **kw)
    # M = 0: "no queries" on the variance side (then no problem may count any), an error on the predict-at side
    assert check(B, N, (0,), empty_ok=True) == (0, None, None) == check(B, N, (B, 0), empty_ok=True)
    assert check(B, N, (0,), nq=[0, 0, 0], empty_ok=True)[2].tolist() == [0, 0, 0]
    _raises(ValueError, "dimension mismatch", check, B, N, (0,), nq=[0, 1, 0], empty_ok=True)
    _raises(ValueError, "dimension mismatch", check, B, N, None, nq=[0, 1, 0], empty_ok=True)
    _raises(ValueError, "query times of shape (1, 0) for a batch of 3 problems", check, B, N, (0,))
    _raises(ValueError, "query times of shape (3, 0) for a batch of 3 problems", check, B, N, (B, 0))


def test_check_pack_batch_message_and_home():
    assert grad.check_pack_batch is rowcall.check_pack_batch and "check_pack_batch" in grad.__all__
    real, comp, diag_add = np.zeros((2, 5, 2)), np.zeros((4, 5, 1)), np.zeros(5)
    rowcall.check_pack_batch(5, 2, 1, real, comp, diag_add)
    rowcall.check_pack_batch(5, 2, 0, real, comp, diag_add)            # no complex terms: one padding column
    _raises(ValueError, "coefficient pack of shapes ((2, 4, 2), (4, 5, 1), (5,)) does not match the batch of 5 "
            "problems (expected ((2, 5, 2), (4, 5, 1), (5,)))", rowcall.check_pack_batch, 5, 2, 1, real[:, :4], comp,
            diag_add)
    _raises(ValueError, "coefficient pack of shapes ((2, 5, 2), (4, 5, 1), (4,)) does not match the batch of 5 "
            "problems (expected ((2, 5, 2), (4, 5, 1), (5,)))", rowcall.check_pack_batch, 5, 2, 1, real, comp,
            diag_add[:4])
