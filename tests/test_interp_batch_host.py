"""CPU: what gadfly_amd.interpolate_missing_data_batch and the segmented gap-fill entry points (gf_interp_seg_work,
gf_interp_plan_seg, gf_interp_fill_seg) refuse, before anything reaches a device.

The dummy address `D` is never dereferenced: every case below that carries it also carries a NULL required pointer,
a bad S or a bad total, which the entry points refuse before they launch.  As in tests/test_abi_errors_host.py those
cases run only where there is no device, where a mistaken launch is a -2 status and a failed assertion.
"""
import ctypes

import numpy as np
import pytest

from gadfly_amd import _lib

D = ctypes.c_void_p(0x1000)
Z = None

# required pointers by position; cadences and which may be NULL
PLAN_REQUIRED = {2: "off", 3: "t", 5: "dt", 7: "plan", 8: "new_off", 9: "info", 10: "work"}
FILL_REQUIRED = {2: "off", 3: "t", 4: "f", 6: "dt", 8: "plan", 9: "t_out", 10: "f_out"}


def plan_args(S=3, total=100, null=()):
    args = [S, total] + [D] * 9 + [Z]
    args[4] = args[6] = Z                   # cadences, which
    for k in null:
        args[k] = Z
    return tuple(args)


def fill_args(S=3, total=100, null=()):
    args = [S, total] + [D] * 9 + [Z]
    args[5] = args[7] = Z                   # cadences, which
    for k in null:
        args[k] = Z
    return tuple(args)


ALL_NULL = tuple(range(2, 11))

NO_POINTER_CASES = [
    ("gf_interp_plan_seg", plan_args(S=0, null=ALL_NULL), "gf_interp_plan_seg: no segments (S=0)"),
    ("gf_interp_plan_seg", plan_args(S=-2, null=ALL_NULL), "gf_interp_plan_seg: no segments (S=-2)"),
    ("gf_interp_plan_seg", plan_args(total=-1, null=ALL_NULL), "gf_interp_plan_seg: negative length (total=-1)"),
    ("gf_interp_plan_seg", plan_args(null=ALL_NULL), "gf_interp_plan_seg: null pointer"),
    ("gf_interp_fill_seg", fill_args(S=0, null=ALL_NULL), "gf_interp_fill_seg: no segments (S=0)"),
    ("gf_interp_fill_seg", fill_args(total=-5, null=ALL_NULL), "gf_interp_fill_seg: negative length (total=-5)"),
    ("gf_interp_fill_seg", fill_args(null=ALL_NULL), "gf_interp_fill_seg: null pointer"),
    ("gf_interp_fill_seg", fill_args(total=0, null=ALL_NULL), "gf_interp_fill_seg: null pointer"),
]

DUMMY_POINTER_CASES = (
    [("gf_interp_plan_seg", plan_args(S=0), "gf_interp_plan_seg: no segments (S=0)"),
     ("gf_interp_plan_seg", plan_args(total=-1), "gf_interp_plan_seg: negative length (total=-1)"),
     ("gf_interp_fill_seg", fill_args(S=0), "gf_interp_fill_seg: no segments (S=0)"),
     ("gf_interp_fill_seg", fill_args(total=-1), "gf_interp_fill_seg: negative length (total=-1)")]
    + [("gf_interp_plan_seg", plan_args(null=(k,)), "gf_interp_plan_seg: null pointer") for k in PLAN_REQUIRED]
    + [("gf_interp_fill_seg", fill_args(null=(k,)), "gf_interp_fill_seg: null pointer") for k in FILL_REQUIRED]
)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _run(lib, cases):
    for name, args, text in cases:
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
        assert getattr(lib, name)(*args) == -1, (name, args, lib.gf_last_error())
        assert _lib.last_error() == text, (name, args)
        assert name in _lib.last_error()


def test_bad_shapes_and_all_null(lib):
    _run(lib, NO_POINTER_CASES)


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="dummy addresses: only where nothing can launch")
def test_each_null_required_pointer(lib):
    assert len(DUMMY_POINTER_CASES) == 4 + len(PLAN_REQUIRED) + len(FILL_REQUIRED)
    _run(lib, DUMMY_POINTER_CASES)


def test_work_size(lib):
    assert lib.gf_interp_seg_work(-1) == -1
    assert _lib.last_error() == "gf_interp_seg_work: negative length (total=-1)"
    assert lib.gf_interp_seg_work(0) == 0
    # one word per 2048 points, as gf_interp_work: the two share their scan
    for total in (1, 2047, 2048, 2049, 1 << 21, (1 << 33) + 1):
        assert lib.gf_interp_seg_work(total) == lib.gf_interp_work(total) == -(-total // 2048)


# ---------------------------------------------------------------------------------- interpolate_missing_data_batch
@pytest.fixture()
def no_device(monkeypatch):
    """Any step past the host checks fails the test, with or without a device."""
    def reached():
        raise AssertionError("the device was reached before the input was refused")
    monkeypatch.setattr(_lib, "require_device", reached)


def _good(n=10, t0=0.0):
    return t0 + np.arange(n) * 0.5, np.linspace(1.0, 2.0, n)


def test_batch_refuses_before_the_device(no_device):
    from gadfly_amd import interpolate_missing_data_batch as batch
    t, f = _good()
    with pytest.raises(ValueError, match="no series"):
        batch([], [])
    with pytest.raises(ValueError, match="one length"):
        batch([t, t], [f])
    with pytest.raises(ValueError, match="one length"):
        batch([t, t], [f, f], cadences=[np.arange(10)])
    with pytest.raises(ValueError, match="series 1: 1 points"):
        batch([t, t[:1], t], [f, f[:1], f])
    with pytest.raises(ValueError, match="series 2: dimension mismatch"):
        batch([t, t, t], [f, f, f[:-1]])
    with pytest.raises(ValueError, match="series 0: dimension mismatch"):
        batch([t.reshape(2, 5), t], [f.reshape(2, 5), f])
    with pytest.raises(ValueError, match="series 1: dimension mismatch"):
        batch([t, t], [f, f], cadences=[np.arange(10), np.arange(9)])
    late = t.copy()
    late[4] = late[3]
    with pytest.raises(ValueError, match="series 1: times must be strictly increasing"):
        batch([t, late], [f, f])
    open_end = t.copy()
    open_end[-1] = np.inf
    with pytest.raises(ValueError, match="series 1: times must be finite"):
        batch([t, open_end], [f, f])
    back = t.copy()
    back[-1] = back[0] - 1.0
    with pytest.raises(ValueError, match="series 0: times must be strictly increasing"):
        batch([back], [f])


def test_batch_reaches_the_device_check_on_good_input(no_device):
    """The fixture's tripwire itself: good input gets past the host checks."""
    from gadfly_amd import interpolate_missing_data_batch as batch
    t, f = _good()
    with pytest.raises(AssertionError, match="the device was reached"):
        batch([t, t + 100.0], [f, f])
    with pytest.raises(AssertionError, match="the device was reached"):
        batch([t], [f], cadences=[np.arange(10)])


def test_exported():
    import gadfly_amd
    assert gadfly_amd.interpolate_missing_data_batch is gadfly_amd.interp.interpolate_missing_data_batch
    for name in ("gf_interp_seg_work", "gf_interp_plan_seg", "gf_interp_fill_seg"):
        assert name in _lib.SIGNATURES
