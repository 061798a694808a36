"""GPU: the chunked finishing launch of the steady tail (gf_steady_finish_chunked) -- the tail of a
problem in chunks of 16 blocks side by side: pass A, P = M^16, pass B, the chunks' sums in chunk order -- and the
overlapped finishing schedule of the evaluator that uses it.

Against gf_steady_finish on a copy of the same fresh header with acc = (0, 0, +inf) (tests/test_gpu_steady_group.py's
set-up: the series of tests/steady_group_cases.py, the switch forced to ANCHOR): acc[b][0] and acc[b][2] bit for bit
(one product, one minimum), acc[b][1] within RTOL_BUILDS = 1e-12 relative (the project's bound between two builds'
outputs), the header's end state within the bar of tests/test_steady_chunk_host.py -- there both forms lie within
max(FACTOR e_seq, FLOOR) of the row form and e_seq <= 2.3e-15 on these kernels, so the two device forms are asked to
agree to FLOOR = 1e-13 of max |s| --, and acc[b][1] against the oracle's own tail sums at
tests/test_gpu_steady_group.py's bar.  tests/test_steady_chunk_host.py shows without a device that the flagship inputs
used below see the correction by P (|P| ~ 100 at 16-block chunks)."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, ARM, B_FIN, J_ALL, SW, T, _fast_terms, _rel
from tests.steady_group_cases import J_GROUP, LONGEST_G, N_G, series
from tests.steady_raw import finish_head
from tests.test_gpu_steady import _evaluator, _series
from tests.test_gpu_steady_group import raws  # noqa: F401  (the module fixture of the raw entry points)
from tests.test_steady_fold_host import FLOOR
from tests.test_steady_tail_host import RTOL_Z

pytestmark = pytest.mark.gpu
CHUNK_BLOCKS = 16
CHUNK = 64 * CHUNK_BLOCKS
RTOL_BUILDS = 1e-12
I64_MAX = (1 << 63) - 1
# no second chunk; exactly one chunk; a chunk and a row; two chunks; two and a row; three chunks, the last one a block
# and a row -- and the neighbours below
TAILS = (1, 64, 1023, 1024, 1025, 2047, 2048, 2049, LONGEST_G)


def _chunked(r, N, hdr_, acc_, y=None, y_bs=None, window=(0, I64_MAX), ws=None):
    """One gf_steady_finish_chunked on the buffers of tests/test_gpu_steady_group.py::raws; returns the workspace."""
    import torch
    from gadfly_amd import _lib
    eng, lib, p = r["eng"], r["lib"], r["p"]
    if ws is None:
        ws = torch.full((eng.B, int(lib.gf_steady_chunk_size(N, CHUNK_BLOCKS))), float("nan"), **r["f64"])
    head = finish_head(eng, N, hdr_, acc_, y=y, y_bs=y_bs)
    st = lib.gf_steady_finish_chunked(*head, int(window[0]), int(window[1]), CHUNK_BLOCKS, p(ws), r["stream"])
    _lib.check(st, "gf_steady_finish_chunked")
    return ws


def _state(hdr):
    """(s_r, s_i) of the header: ST_SR = 72, ST_SI = 104, 32 each."""
    return hdr[..., 72:136]


def _against_plain(what, plain, chunk, hdr_plain, hdr_chunk):
    assert np.array_equal(chunk[..., 0], plain[..., 0]), (what, chunk[..., 0].tolist(), plain[..., 0].tolist())
    assert np.array_equal(chunk[..., 2], plain[..., 2]), what
    e1 = (np.abs(chunk[..., 1] - plain[..., 1]) / np.abs(plain[..., 1])).max()
    sp, sc = _state(hdr_plain), _state(hdr_chunk)
    es = (np.abs(sc - sp).max(axis=-1) / np.abs(sp).max(axis=-1)).max()
    print(f"{what}: chunked against one wave, sum z^2/d {e1:.2e}, end state {es:.2e} of max |s|")
    assert e1 <= RTOL_BUILDS, (what, e1)
    assert es <= FLOOR, (what, es)
    rest = np.ones(hdr_plain.shape[-1], dtype=bool)
    rest[72:136] = False
    rest[5] = False                                 # ST_HOK, ST_H: the one-wave launch keeps h in the header
    rest[136:200] = False
    assert np.array_equal(hdr_chunk[..., rest], hdr_plain[..., rest]), what


@pytest.mark.parametrize("J", J_GROUP)
def test_chunked_launch_against_the_one_wave_launch(raws, J):  # noqa: F811
    import torch
    r = raws(J)
    c, B = r["case"], B_FIN
    hp, ap = r["fresh"](len(TAILS))
    hc, ac = r["fresh"](len(TAILS) + 1)
    keep = []
    for i, k in enumerate(TAILS):
        r["finish"](ANCHOR + 1 + k, hp[i], ap[i])
        keep.append(_chunked(r, ANCHOR + 1 + k, hc[i], ac[i]))
    keep.append(_chunked(r, N_G, hc[-1], ac[-1]))               # the longest tail a second time
    torch.cuda.synchronize()
    plain, chunk, hdp, hdc = ap.cpu().numpy(), ac.cpu().numpy(), hp.cpu().numpy(), hc.cpu().numpy()
    assert TAILS[-1] == LONGEST_G
    assert np.array_equal(chunk[-1], chunk[-2]) and np.array_equal(hdc[-1], hdc[-2])
    dinf = r["hdr"][:, 1]
    for i, k in enumerate(TAILS):
        what = f"J = {J}, tail of {k} rows"
        assert np.all(hdc[i, :, 2] == 0.0) and np.all(hdc[i, :, 0] == SW), what
        _against_plain(what, plain[i], chunk[i], hdp[i], hdc[i])
        if k <= CHUNK:                              # one chunk: the one-wave launch's own additions
            assert np.array_equal(chunk[i], plain[i]), what
            assert np.array_equal(_state(hdc[i]), _state(hdp[i])), what
        for b in range(B):
            s = c.sums[b]
            err = abs(chunk[i, b, 1] - s.z2d[k - 1])
            bar = 2.0 * RTOL_Z * c.zmax[b] * s.zabs[k - 1] / dinf[b] + RTOL_Z * s.z2d[k - 1]
            assert err <= bar, (what, b, err / bar)


@pytest.mark.parametrize("J", J_ALL)
def test_every_instance_on_a_three_chunk_tail(hip, J):
    """All 16 ROWS instances at both parities of the padding (Jc = 1 .. 31), tests/steady_cases.py's kernels on the
    long series: two chunks, a block and a row behind the forced switch, through the evaluator's two schedules."""
    t, y = series()
    hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
    ev, _ = _evaluator(hps, t, y, T)
    eng = ev.engine
    ev.auto_generator_period, eng.generator_period = False, 1
    eng._steady_axis = (ARM, 0.0)
    eng.steady_overlap = False
    ref = ev.evaluate()
    sw, viol = eng.steady_switch_rows(), eng.steady_violations().cpu().numpy()
    assert np.all(sw == SW), sw.tolist()
    eng.steady_overlap, eng.STEADY_OVERLAP_MIN_B, eng._steady_chunk_blocks = True, 1, CHUNK_BLOCKS
    eng._steady_feedback, eng._steady_split = None, (SW - 1) // T * T       # every problem behind the split
    got = ev.evaluate()
    assert eng._steady_chunk_ws is not None and eng._steady_chunk_ws[1] == CHUNK_BLOCKS
    assert np.array_equal(eng.steady_switch_rows(), sw)
    assert np.array_equal(eng.steady_violations().cpu().numpy(), viol) and not viol.any()
    e = _rel(got, ref).max()
    print(f"J = {J:2d} (ROWS = {(2 * J + 3) // 4 * 4:2d}): chunked route against the one launch {e:.2e}")
    assert e <= RTOL_BUILDS


def test_rows_behind_the_series_and_problems_outside_the_window(raws):  # noqa: F811
    """Rows >= N poisoned with NaN: the same bits.  A window that does not hold the switch row: header and acc
    untouched, bit for bit.  Two disjoint windows, one chunked and one plain, in both orders: the chunked launch's
    values when it holds the problems, the plain launch's bits when that one does."""
    import torch
    r = raws(30)
    c = r["case"]
    k = 2049
    N = ANCHOR + 1 + k
    y = torch.tensor(c.y, **r["f64"])
    yp = y.clone()
    yp[N:] = float("nan")
    hd, ac = r["fresh"](7)
    h0, a0 = hd[6].clone(), ac[6].clone()
    keep = [_chunked(r, N, hd[0], ac[0], y=y, y_bs=0), _chunked(r, N, hd[1], ac[1], y=yp, y_bs=0)]
    r["finish"](N, hd[2], ac[2])
    keep.append(_chunked(r, N, hd[3], ac[3], window=(1, SW)))           # chunked holds nobody, plain everybody
    r["finish"](N, hd[3], ac[3], window=(SW, N + 1))
    r["finish"](N, hd[4], ac[4], window=(1, SW))                        # the other way round, plain first
    keep.append(_chunked(r, N, hd[4], ac[4], window=(SW, N + 1)))
    keep.append(_chunked(r, N, hd[5], ac[5], window=(SW, N + 1)))       # chunked first
    r["finish"](N, hd[5], ac[5], window=(1, SW))
    keep.append(_chunked(r, N, hd[6], ac[6], window=(SW + 1, I64_MAX)))  # outside
    keep.append(_chunked(r, N, hd[6], ac[6], window=(0, SW)))
    torch.cuda.synchronize()
    a, h = ac.cpu().numpy(), hd.cpu().numpy()
    assert np.all(np.isfinite(a[0])) and np.all(a[0][:, 1] > 0.0)
    assert np.array_equal(a[0], a[1]) and np.array_equal(h[0], h[1])
    assert np.array_equal(a[3], a[2]) and np.array_equal(h[3], h[2])
    assert np.array_equal(a[4], a[0]) and np.array_equal(h[4], h[0])
    assert np.array_equal(a[5], a[0]) and np.array_equal(h[5], h[0])
    assert np.array_equal(a[6], a0.cpu().numpy()) and np.array_equal(h[6], h0.cpu().numpy())


@pytest.fixture(scope="module")
def walkers():
    """Flagship walkers (the 30-term solar-like kernel, jitter seeds 1000 and the slowest, 1027, among them) on the
    benchmark's kind of series, and their switch rows on the device."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    N = 65536
    t, y = _series(N)
    hps = [jitter_hyperparameters(solar_like_hyperparameters(30), s) for s in (1000, 1001, 1002, 1027)]
    ev, _ = _evaluator(hps, t, y, 8192)
    ev.auto_generator_period = False
    ev.engine.steady_overlap = False
    ev.evaluate()
    sw = ev.engine.steady_switch_rows()
    assert np.all(sw > 0) and sw.max() > 50000, sw.tolist()
    return hps, t, y, sw


def _two_schedules(ev, split, chunk_blocks):
    """(one launch, the overlapped schedule with the given split): values, violations, switch rows."""
    eng = ev.engine
    ev.auto_generator_period = False
    eng.steady_overlap = False
    ref = ev.evaluate()
    sw, viol = eng.steady_switch_rows(), eng.steady_violations().cpu().numpy()
    eng.steady_overlap, eng.STEADY_OVERLAP_MIN_B, eng._steady_chunk_blocks = True, 1, chunk_blocks
    if split is not None:
        eng._steady_feedback, eng._steady_split = None, split
    eng.time_factor, eng.finish_events = True, []
    got = ev.evaluate()
    assert np.array_equal(eng.steady_switch_rows(), sw)
    assert np.array_equal(eng.steady_violations().cpu().numpy(), viol)
    return ref, got, sw, len(eng.finish_events)


def test_chunks_whose_correction_is_of_order_one(hip, walkers):
    """The evaluator's route on flagship walkers, every problem on the chunked route at 16-block chunks, on a series
    that ends three chunks and 65 rows behind the latest switch row: |P| ~ 100 there
    (tests/test_steady_chunk_host.py); with P zeroed in a copy of the library this comparison gave 2.0e-4
    (CHANGELOG)."""
    hps, t, y, sw0 = walkers
    N = int(sw0.max()) + 3 * CHUNK + 65
    ev, _ = _evaluator(hps, t[:N], y[:N], 8192)
    ref, got, sw, launches = _two_schedules(ev, (int(sw0.min()) - 1) // 8192 * 8192, CHUNK_BLOCKS)
    assert np.array_equal(sw, sw0) and launches == 2
    e = _rel(got, ref)
    print(f"switch rows {sw.tolist()} of {N}: chunked route against the one launch {e.tolist()}")
    assert e.max() <= RTOL_BUILDS


def test_overlapped_schedule_on_a_mixed_batch(hip, walkers):
    """Some problems per route: the early switchers through gf_steady_finish_window on the side stream behind the tile
    of the split, the others through the chunked launch behind the last tile."""
    hps, t, y, sw0 = walkers
    split = (int(np.sort(sw0)[1]) - 1) // 8192 * 8192 + 8192
    assert 0 < np.sum(sw0 <= split) < len(sw0), (sw0.tolist(), split)
    ev, _ = _evaluator(hps, t, y, 8192)
    ref, got, sw, launches = _two_schedules(ev, split, None)
    e = _rel(got, ref)
    print(f"switch rows {sw.tolist()}, split {split}: overlapped schedule against the one launch {e.tolist()}")
    assert launches == 2 and e.max() <= RTOL_BUILDS
    early = sw <= split
    assert np.array_equal(got[early], ref[early])           # the window launch is the one launch's code


def test_feedback_sets_the_split(hip):
    """B = 64 flagship walkers (jitter seeds 1000 .. 1063, the slowest one among them): the second evaluation takes its
    split from the first one's switch rows -- all but B / 8 in front of it -- without being told, finishes the early
    switchers beside the later tiles and the others in chunks (chunk_blocks from N), and agrees with the one launch."""
    from gadfly_amd.synth import jitter_hyperparameters, solar_like_hyperparameters
    N, B = 65536, 64
    t, y = _series(N)
    hps = [jitter_hyperparameters(solar_like_hyperparameters(30), 1000 + i) for i in range(B)]
    ev, _ = _evaluator(hps, t, y, 8192)
    ref, got, sw, launches = _two_schedules(ev, None, None)
    split = ev.engine._steady_split
    behind = int(np.sum(sw > split))
    print(f"switch rows {sw.min()} .. {sw.max()}, split {split}, {behind} problems behind it, {launches} finishing "
          f"launches, against the one launch {_rel(got, ref).max():.2e}")
    assert split > 0 and 0 < behind <= B // 8 and launches == 2
    assert _rel(got, ref).max() <= RTOL_BUILDS
