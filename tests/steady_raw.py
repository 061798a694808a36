"""The argument lists of the steady family's raw entry points on an engine's own buffers, for the tests that call the
library directly (tests/test_gpu_steady_*.py).

The order is restated here from include/gadfly_hip.h, slot by slot under the header's own argument names, and the
coefficient pack is read by field name: nothing below calls the engine's builders (gadfly_amd.engine.sweep_head /
finish_head), so these tests stay a second, independent statement of the ABI.  A keyword argument named after a slot
replaces that slot's value (an argument-error test passes B=0, N=0, ac=None, ...: the builders' own parameters are
positional-only, so that every slot name is free for it)."""
from gadfly_amd import _lib

#: gf_loglike_fused / gf_loglike_steady / gf_steady_sweep / gf_steady_sweep_reduced / gf_sample_fused, up to `info`
SWEEP_SLOTS = ("B", "N", "n_first", "Jr", "Jc", "block", "gen_period", "variant",
               "ar", "cr", "ac", "bc", "cc", "dc", "diag_add", "cmax",
               "t", "t_bs", "diag", "diag_bs", "y", "y_bs", "d", "z", "S_state", "F_state", "info")
#: gf_steady_finish / gf_steady_finish_window / gf_steady_finish_chunked, up to `acc`
FINISH_SLOTS = ("B", "N", "Jr", "Jc", "block", "variant", "ac", "bc", "cc", "dc", "cmax",
                "t", "t_bs", "y", "y_bs", "info", "steady", "acc")


def sweep_options(eng):
    """(block, variant) of the engine's streamed sweep: the long scaling span where its pack allows one."""
    pack, variant = eng._pack, int(eng.sweep_variant)
    if pack.stream_block:
        return pack.stream_block, variant | _lib.GF_SWEEP_LONG_SPAN
    return pack.block, variant


def _slots(names, values, over):
    assert len(names) == len(values) and set(over) <= set(names), sorted(set(over) - set(names))
    slots = dict(zip(names, values))
    slots.update(over)
    return tuple(slots[k] for k in names)


def sweep_head(eng, rows, n_first, /, gen_period=1, **over):
    """The 27 arguments B ... info of a sweep of `rows` rows from row `n_first` on the engine's buffers."""
    p, pack = _lib.ptr, eng._pack
    block, variant = sweep_options(eng)
    return _slots(SWEEP_SLOTS, (
        eng.B, rows, n_first, eng.Jr, eng.Jc, block, gen_period, variant,
        p(pack.real[0]), p(pack.real[1]), p(pack.comp[0]), p(pack.comp[1]), p(pack.comp[2]), p(pack.comp[3]),
        p(pack.diag_add), p(pack.cmax),
        p(eng.t), eng._bs(eng.t), p(eng.diag), 0 if eng.diag is None else eng._bs(eng.diag), p(eng.y), eng._bs(eng.y),
        p(eng.d), p(eng.z), p(eng.S_state), p(eng.F_state), p(eng.info)), over)


def finish_head(eng, N, steady, acc, /, y=None, y_bs=None, **over):
    """The 18 arguments B ... acc of a finishing launch over the first N rows, on the header `steady` and `acc`; with
    `y`, that tensor and its batch stride `y_bs` in place of the engine's own series."""
    p, pack = _lib.ptr, eng._pack
    block, variant = sweep_options(eng)
    return _slots(FINISH_SLOTS, (
        eng.B, N, eng.Jr, eng.Jc, block, variant,
        p(pack.comp[0]), p(pack.comp[1]), p(pack.comp[2]), p(pack.comp[3]), p(pack.cmax),
        p(eng.t), eng._bs(eng.t), p(eng.y if y is None else y), eng._bs(eng.y) if y is None else y_bs,
        p(eng.info), p(steady), p(acc)), over)
