"""GPU: GF_SWEEP_AXIS_PROVEN, the bit of the finishing launches' `variant` with which the caller vouches for the tail's
spacing tests (include/gadfly_hip.h), through the raw entry points on the set-up of
tests/test_gpu_steady_group.py: the series of tests/steady_group_cases.py, the switch forced to ANCHOR, a tail of 2113
rows (two groups of 16 blocks, a block and a row), J = 1, 2, 15, 29, 30, 31.

  - On the regular axis gf_steady_finish, gf_steady_finish_window (two disjoint windows) and gf_steady_finish_chunked
    (chunks of 16 and of 32 blocks) give the same bits with the bit as without: acc, the whole header (state, h, flag).
  - One time stamp moved off the cadence inside the tail: without the bit the launch raises steady[b][2]; with it the
    flag stays down and acc is finite.  That is the contract -- the caller promised what its axis does not keep --, a
    data condition and no fault.
  - The argument checks refuse what they refused, in the same words, whether the bit is set or not."""
import numpy as np
import pytest

from tests.steady_cases import B_FIN, SW
from tests.steady_group_cases import N_G
from tests.steady_raw import finish_head, sweep_options
from tests.test_gpu_steady_group import raws  # noqa: F401  (the module fixture of the raw entry points, long series)

pytestmark = pytest.mark.gpu
J_CASES = (1, 2, 15, 29, 30, 31)
I64_MAX = (1 << 63) - 1
ST_VIOL = 2


def _variant(r, proven):
    from gadfly_amd import _lib
    return sweep_options(r["eng"])[1] | (_lib.GF_SWEEP_AXIS_PROVEN if proven else 0)


def _launch(r, name, hdr_, acc_, proven, *tail, **over):
    """One finishing launch by name on the long series; returns the status (the caller checks it)."""
    head = finish_head(r["eng"], N_G, hdr_, acc_, variant=_variant(r, proven), **over)
    return getattr(r["lib"], name)(*head, *tail, r["stream"])


def _chunk_ws(r, chunk_blocks):
    import torch
    return torch.full((r["eng"].B, int(r["lib"].gf_steady_chunk_size(N_G, chunk_blocks))), float("nan"), **r["f64"])


def _all_entry_points(r, hd, ac, proven, **over):
    """Slot 0: one launch; 1: two windows; 2, 3: chunked at 16 and 32 blocks.  Returns what must stay alive."""
    keep = [_chunk_ws(r, 16), _chunk_ws(r, 32)]
    chk = r["check"]
    chk(_launch(r, "gf_steady_finish", hd[0], ac[0], proven, **over), "gf_steady_finish")
    for window in ((1, SW), (SW, N_G + 1)):
        chk(_launch(r, "gf_steady_finish_window", hd[1], ac[1], proven, *window, **over), "gf_steady_finish_window")
    for i, cb in ((2, 16), (3, 32)):
        chk(_launch(r, "gf_steady_finish_chunked", hd[i], ac[i], proven, 0, I64_MAX, cb, r["p"](keep[i - 2]), **over),
            "gf_steady_finish_chunked")
    return keep


@pytest.mark.parametrize("J", J_CASES)
def test_the_bit_changes_no_bit_on_a_regular_axis(raws, J):  # noqa: F811
    import torch
    r = raws(J)
    hd0, ac0 = r["fresh"](4)
    hd1, ac1 = r["fresh"](4)
    keep = [_all_entry_points(r, hd0, ac0, False), _all_entry_points(r, hd1, ac1, True)]
    torch.cuda.synchronize()
    assert keep and np.all(r["eng"].info.cpu().numpy() == 0)
    a0, a1, h0, h1 = ac0.cpu().numpy(), ac1.cpu().numpy(), hd0.cpu().numpy(), hd1.cpu().numpy()
    assert np.all(np.isfinite(a0)) and np.all(a0[..., 1] > 0.0)
    assert np.all(h0[..., ST_VIOL] == 0.0) and np.all(h0[..., 0] == SW)
    assert not np.array_equal(h0[0, :, 72:136], r["hdr"][:, 72:136])       # (the launches did run: the state moved)
    for i, what in enumerate(("one launch", "two windows", "chunks of 16 blocks", "chunks of 32 blocks")):
        assert np.array_equal(a1[i], a0[i]), (J, what, a0[i].tolist(), a1[i].tolist())
        assert np.array_equal(h1[i], h0[i]), (J, what)
    assert np.array_equal(a0[1], a0[0]) and np.array_equal(h0[1], h0[0])    # (windows: the one launch's bits)


@pytest.mark.parametrize("J", (2, 30))
def test_a_spacing_off_the_cadence_is_the_callers_with_the_bit(raws, J):  # noqa: F811
    import torch
    r = raws(J)
    eng, p = r["eng"], r["p"]
    t = eng.t.clone()
    row = SW + 1100                                 # inside the tail's second group
    cadence = float(t[0, -1] - t[0, -2])
    t[:, row] += 0.25 * cadence                     # two spacings off the frozen cadence, by far more than 2e-6 / wmax
    over = dict(t=p(t), t_bs=eng._bs(t))
    hd0, ac0 = r["fresh"](4)
    hd1, ac1 = r["fresh"](4)
    keep = [_all_entry_points(r, hd0, ac0, False, **over), _all_entry_points(r, hd1, ac1, True, **over)]
    torch.cuda.synchronize()
    assert keep and np.all(eng.info.cpu().numpy() == 0)
    a1, h0, h1 = ac1.cpu().numpy(), hd0.cpu().numpy(), hd1.cpu().numpy()
    assert np.all(h0[..., ST_VIOL] == 1.0), h0[..., ST_VIOL].tolist()      # the kernel's own test finds it
    assert np.all(h1[..., ST_VIOL] == 0.0), h1[..., ST_VIOL].tolist()      # the caller's word is taken
    assert np.all(np.isfinite(a1)) and np.all(np.isfinite(h1))
    # ... and with the bit no time stamp is read at all: the values are those of the regular axis
    hd2, ac2 = r["fresh"](4)
    keep.append(_all_entry_points(r, hd2, ac2, True))
    torch.cuda.synchronize()
    assert np.array_equal(a1, ac2.cpu().numpy()) and np.array_equal(h1, hd2.cpu().numpy())


def test_argument_checks_refuse_in_the_same_words(raws):  # noqa: F811
    from gadfly_amd import _lib
    r = raws(2)
    hd, ac = r["fresh"](1)
    ws = _chunk_ws(r, 16)
    before = (hd.clone(), ac.clone())
    cases = [("gf_steady_finish", (), dict(B=0)),
             ("gf_steady_finish", (), dict(N=0)),
             ("gf_steady_finish", (), dict(Jr=1)),
             ("gf_steady_finish", (), dict(Jc=32)),
             ("gf_steady_finish", (), dict(block=3)),
             ("gf_steady_finish", (), dict(t=None)),
             ("gf_steady_finish", (), dict(acc=None)),
             ("gf_steady_finish_window", (5, 4), {}),
             ("gf_steady_finish_window", (-1, 4), {}),
             ("gf_steady_finish_chunked", (0, I64_MAX, 15, r["p"](ws)), {}),
             ("gf_steady_finish_chunked", (0, I64_MAX, 8, r["p"](ws)), {}),
             ("gf_steady_finish_chunked", (0, I64_MAX, 16, None), {}),
             ("gf_steady_finish_chunked", (4, 3, 16, r["p"](ws)), {})]
    for name, tail, over in cases:
        said = []
        for proven in (False, True):
            head = finish_head(r["eng"], N_G, hd[0], ac[0], **{"variant": _variant(r, proven), **over})
            st = getattr(r["lib"], name)(*head, *tail, r["stream"])
            assert st == -1, (name, tail, over, proven, st)
            said.append(_lib.last_error())
        assert said[0] == said[1] and name in said[0], (name, tail, over, said)
    import torch
    torch.cuda.synchronize()
    assert torch.equal(hd, before[0]) and torch.equal(ac, before[1])
    # the bit belongs to the finishing launches: the sweeps refuse it as an unknown variant
    from tests.steady_raw import sweep_head
    eng = r["eng"]
    head = sweep_head(eng, 64, 0, variant=_variant(r, True))
    st = r["lib"].gf_loglike_fused(*head, r["stream"])
    assert st == -1 and "variant" in _lib.last_error()
    assert B_FIN == eng.B
