"""Host: the streamed engine's named coefficient pack and its argument builders (gadfly_amd.engine.CoefficientPack,
sweep_options, sweep_head, finish_head, kernel_and_series) against the binding's own table of the C ABI,
`_lib.SIGNATURES` -- no device: CPU float64 tensors stand in for the buffers, nothing is launched.  A slot that moves,
goes missing or changes its type shows here instead of as a wrong number on a GPU."""
import ctypes

import pytest
import torch

from gadfly_amd import _lib
from gadfly_amd.batch import _Pack
from gadfly_amd.engine import CoefficientPack, finish_head, kernel_and_series, sweep_head, sweep_options

FIELDS = ("real", "comp", "diag_add", "c", "cmax", "block", "dmax", "stream_block", "wmax")
B, N, T, JR, JC = 3, 200, 64, 1, 2
STREAM = 0x5000

#: entry point -> what follows the shared head in front of the stream; a name stands for that buffer's pointer (_tail)
SWEEP_TAILS = {
    "gf_loglike_fused": (),
    "gf_sample_fused": (),
    "gf_loglike_steady": ("steady", 128),
    "gf_steady_sweep": ("steady", 128),
    "gf_steady_sweep_reduced": ("steady", 128, "acc", 1),
}
FINISH_TAILS = {
    "gf_steady_finish": (),
    "gf_steady_finish_window": (1, 65),
    "gf_steady_finish_chunked": (1, 65, 16, "ws"),
}


def _pack(stream_block=0):
    f64 = torch.float64
    return CoefficientPack(torch.rand((2, B, JR), dtype=f64), torch.rand((4, B, JC), dtype=f64),
                           torch.rand((B,), dtype=f64), torch.rand((B, JR + 2 * JC), dtype=f64),
                           torch.rand((B,), dtype=f64), 8, 3.5, stream_block, 4.5)


@pytest.fixture(scope="module")
def buffers():
    f64 = torch.float64
    buf = dict(t=torch.rand((1, N), dtype=f64), diag=torch.rand((B, N), dtype=f64), y=torch.rand((B, N), dtype=f64),
               d=torch.empty((B, T), dtype=f64), z=torch.empty((B, T), dtype=f64),
               S_state=torch.empty((B, 4096), dtype=f64), F_state=torch.empty((B, 64), dtype=f64),
               info=torch.zeros((B,), dtype=torch.int32), steady=torch.zeros((B, 256), dtype=f64),
               acc=torch.empty((B, 3), dtype=f64), ws=torch.empty((B, 512), dtype=f64))
    return buf


def _tail(tail, buf):
    return tuple(buf[v].data_ptr() if isinstance(v, str) else v for v in tail)


def _sweep(pack, buf, **over):
    a = dict(buf, **over)
    return sweep_head(pack, B, T, 2 * T, JR, JC, 8, 4, 2, a["t"], a["diag"], a["y"], a["d"], a["z"], a["S_state"],
                      a["F_state"], a["info"], y_bs=a.get("y_bs"))


def _check_types(name, args):
    """len(args) is the signature's; a pointer slot holds an int or None, an integer slot an int."""
    argtypes = _lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes), (name, len(args), len(argtypes))
    for i, (v, ty) in enumerate(zip(args, argtypes)):
        if ty is ctypes.c_void_p:
            assert v is None or type(v) is int, (name, i, v)
        else:
            assert ty in (ctypes.c_int, ctypes.c_int64) and type(v) is int, (name, i, ty, v)


def test_pack_is_a_named_nine_tuple():
    assert CoefficientPack._fields == FIELDS
    pack = _pack()
    assert isinstance(pack, tuple) and len(pack) == 9
    assert all(a is b for a, b in zip(pack[:5], (pack.real, pack.comp, pack.diag_add, pack.c, pack.cmax)))
    real, comp, diag_add, c, cmax, block, dmax, stream_block, wmax = pack
    assert (block, dmax, stream_block, wmax) == (8, 3.5, 0, 4.5) == pack[5:]
    assert pack[6] is pack.dmax and pack[8] is pack.wmax


def test_batch_pack_keeps_the_names_and_takes_psd_safe():
    pack = _pack(stream_block=16)
    pk = _Pack(*pack)
    assert isinstance(pk, CoefficientPack) and pk._fields == FIELDS and pk == pack
    assert pk.comp is pack.comp and pk.stream_block == 16 and pk[:5] == pack[:5]
    assert pk.psd_safe is False
    pk.psd_safe = True
    assert pk.psd_safe is True and _Pack(*pack).psd_safe is False and _Pack._make(pack).psd_safe is False


def test_sweep_options():
    for variant in (_lib.GF_SWEEP_AUTO, _lib.GF_SWEEP_TILED, _lib.GF_SWEEP_TILED | _lib.GF_SWEEP_ZERO_START):
        assert sweep_options(_pack(stream_block=0), variant) == (8, variant)
        assert sweep_options(_pack(stream_block=16), variant) == (16, variant | _lib.GF_SWEEP_LONG_SPAN)


@pytest.mark.parametrize("name", sorted(SWEEP_TAILS))
def test_sweep_head_fills_the_signature(buffers, name):
    head = _sweep(_pack(), buffers)
    assert len(head) == 27
    _check_types(name, head + _tail(SWEEP_TAILS[name], buffers) + (STREAM,))


@pytest.mark.parametrize("name", sorted(FINISH_TAILS))
def test_finish_head_fills_the_signature(buffers, name):
    b = buffers
    head = finish_head(_pack(), B, N, 0, JC, 8, 2, b["t"], b["y"], b["info"], b["steady"], b["acc"])
    assert len(head) == 18
    _check_types(name, head + _tail(FINISH_TAILS[name], b) + (STREAM,))


def test_chunk_sweep_arguments_fill_the_signature(buffers):
    """gf_chunk_sweep as the time-parallel routes call it: its own eleven sizes and options, the 14 arguments the fused
    heads carry in slots 8 .. 21 (the same code), nine outputs with None for the rows not kept."""
    b, pack = buffers, _pack()
    series = kernel_and_series(pack, b["t"], None, b["y"])
    assert series == _sweep(pack, b, diag=None)[8:22]
    outputs = (b["d"].data_ptr(), b["z"].data_ptr(), None, None, None, None, b["S_state"].data_ptr(), None,
               b["info"].data_ptr())
    _check_types("gf_chunk_sweep", (B, N, 64, 4, 0, 4, JR, JC, 8, 4, _lib.GF_SWEEP_ZERO_START) + series + outputs
                 + (STREAM,))


def test_sweep_head_slots(buffers):
    b, pack = buffers, _pack()
    head = _sweep(pack, b)
    assert head[:8] == (B, T, 2 * T, JR, JC, 8, 4, 2)
    assert head[8:14] == (pack.real[0].data_ptr(), pack.real[1].data_ptr(), pack.comp[0].data_ptr(),
                          pack.comp[1].data_ptr(), pack.comp[2].data_ptr(), pack.comp[3].data_ptr())
    assert head[14:16] == (pack.diag_add.data_ptr(), pack.cmax.data_ptr())
    assert head[16:18] == (b["t"].data_ptr(), 0)                    # a shared axis: stride 0
    assert head[18:20] == (b["diag"].data_ptr(), N)
    assert head[20:22] == (b["y"].data_ptr(), N)
    assert head[22:] == tuple(b[k].data_ptr() for k in ("d", "z", "S_state", "F_state", "info"))
    assert len({v for v in head[8:] if v not in (0, N)}) == 16      # sixteen different buffers


def test_sweep_head_overrides_and_missing_diagonal(buffers):
    b, pack = buffers, _pack()
    eps = torch.rand((B, N + 8), dtype=torch.float64)[:, :N]         # rows further apart than the shape says
    out, info = torch.empty_like(b["y"]), torch.zeros((B,), dtype=torch.int32)
    head = _sweep(pack, b, diag=None, y=eps, z=out, info=info, y_bs=N + 8)
    assert head[18:20] == (None, 0)
    assert head[20:22] == (eps.data_ptr(), N + 8)
    assert head[23] == out.data_ptr() and head[26] == info.data_ptr()
    _check_types("gf_sample_fused", head + (STREAM,))
    shared = _sweep(pack, b, diag=b["diag"][:1], y=b["y"][:1])
    assert shared[19] == 0 and shared[21] == 0


def test_finish_head_slots(buffers):
    b, pack = buffers, _pack()
    head = finish_head(pack, B, N, 0, JC, 16, 0x202, b["t"], b["y"], b["info"], b["steady"], b["acc"])
    assert head[:6] == (B, N, 0, JC, 16, 0x202)
    assert head[6:11] == tuple(pack.comp[k].data_ptr() for k in range(4)) + (pack.cmax.data_ptr(),)
    assert head[11:15] == (b["t"].data_ptr(), 0, b["y"].data_ptr(), N)
    assert head[15:] == (b["info"].data_ptr(), b["steady"].data_ptr(), b["acc"].data_ptr())


@pytest.mark.parametrize("stream_block", [0, 16])
def test_raw_entry_helper_states_the_same_lists(buffers, stream_block):
    """tests/steady_raw.py restates both heads from the header on its own; on a stand-in engine of CPU tensors the two
    statements give the same lists, and a slot named in a keyword is replaced, the builders' own N and steady included."""
    from types import SimpleNamespace

    from gadfly_amd.engine import StreamingBatch
    from tests import steady_raw
    b, pack = buffers, _pack(stream_block)
    eng = SimpleNamespace(_pack=pack, sweep_variant=_lib.GF_SWEEP_TILED, B=B, Jr=JR, Jc=JC, _bs=StreamingBatch._bs,
                          **{k: b[k] for k in ("t", "y", "d", "z", "S_state", "F_state", "info")}, diag=None)
    block, variant = sweep_options(pack, eng.sweep_variant)
    assert steady_raw.sweep_options(eng) == (block, variant)
    assert steady_raw.sweep_head(eng, T, 2 * T) == sweep_head(
        pack, B, T, 2 * T, JR, JC, block, 1, variant, b["t"], None, b["y"], b["d"], b["z"], b["S_state"], b["F_state"],
        b["info"])
    assert steady_raw.finish_head(eng, N, b["steady"], b["acc"]) == finish_head(
        pack, B, N, JR, JC, block, variant, b["t"], b["y"], b["info"], b["steady"], b["acc"])
    over = steady_raw.finish_head(eng, N, b["steady"], b["acc"], B=0, N=0, block=3, ac=None, steady=None)
    assert over[:2] == (0, 0) and over[4] == 3 and over[6] is None and over[16] is None
    assert steady_raw.sweep_head(eng, T, 0, d=7, diag=None, diag_bs=0)[18:23] == (None, 0, b["y"].data_ptr(), N, 7)
