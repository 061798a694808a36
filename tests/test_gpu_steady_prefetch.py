"""GPU: where the finishing block takes y from (k_steady_finish / k_steady_chunk), at the end of a
series.  The group phase reads the rows of 16 blocks at once, in operand layout, every index clamped to the series'
last row; a look-ahead of those rows a group ahead through an LDS image was measured in round 38 and not kept (DESIGN.md
7) -- this file is the check such a form has to pass, and pins the clamp of the present one for both kinds of instance
(with and without GF_SWEEP_AXIS_PROVEN).  Through the raw entry points, on a series of tests/steady_cases.py's kind
(seed 47, the switch forced to ANCHOR, tiles of T rows) that is long enough for three groups and 17 rows behind the
switch row; J = 1, 2, 15, 29, 30, 31.

Tails of 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049 and 3 * 1024 + 17 rows -- the group boundary, the clamp
and the last partial group --, each on a y tensor that is EXACTLY N = switch row + tail long: every index of the last
group beyond row N - 1 is clamped to it, and one that is not reads outside the tensor.

Reference: the frozen row form in longdouble (tests/steady_cases.py::row_form), run from what the header holds in front
of the launch (state, gain, cadence) on the tail's own rows.  Bars: those of tests/test_gpu_steady_instances.py --
acc[b][2] = d_inf bit for bit, acc[b][0] = k log d_inf to ULP_LOGD ulp, |acc[b][1] - sum z^2 / d_inf| <= 2 RTOL_Z max|z|
sum |z| / d_inf + RTOL_Z sum z^2 / d_inf with max |z| over the tail's own rows (not larger than that file's, which
takes it over the whole series) -- and those of tests/test_gpu_steady_chunk.py between the chunked launch and the
one-wave launch (_against_plain).  Two windows against one launch bit for bit.  A NaN one row behind the series' last
row, in a buffer one row longer, reaches no output: the same bits as from the exact buffer."""
import numpy as np
import pytest

from tests.steady_cases import ANCHOR, ARM, B_FIN, SW, T, _evaluator, _fast_terms, _series, row_form
from tests.steady_raw import finish_head, sweep_head, sweep_options
from tests.test_gpu_steady_chunk import _against_plain
from tests.test_gpu_steady_instances import ULP_LOGD, _ulps
from tests.test_steady_tail_host import RTOL_Z

pytestmark = pytest.mark.gpu
J_CASES = (1, 2, 15, 29, 30, 31)
TAILS = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 17)
LONGEST_P = TAILS[-1]
N_P = SW + LONGEST_P
I64_MAX = (1 << 63) - 1
ST_DT, ST_GR, ST_GI, ST_SR, ST_SI = 6, 8, 40, 72, 104      # the header's words (gadfly_hip.hip)


@pytest.fixture(scope="module")
def long_raws(hip):
    """Per J, once: an evaluator on the series of N_P rows, gf_steady_sweep + gf_reduce_tile_steady tile by tile, the
    header in front of the finishing launches, and the longdouble row form's z on the longest tail from that header."""
    import torch
    from gadfly_amd import _lib
    made = {}

    def get(J):
        if J in made:
            return made[J]
        t, y = _series(N_P, seed=47)
        hps = [_fast_terms(J, k0) for k0 in range(B_FIN)]
        ev, coeffs = _evaluator(hps, t, y, T)
        eng = ev.engine
        ev.auto_generator_period, eng.generator_period = False, 1
        ev.evaluate()                       # (packs the coefficients; its own result is not used)
        assert eng.B == B_FIN and eng.Jr == 0 and eng.Jc == J and eng.tile_rows == T
        lib, p, B = eng.lib, _lib.ptr, eng.B
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        f64 = dict(dtype=torch.float64, device=eng.device)
        eng.S_state.zero_()
        eng.F_state.zero_()
        eng.info.zero_()
        steady = torch.zeros((B, int(lib.gf_steady_size())), **f64)
        acc = torch.full((B, 3), float("nan"), **f64)
        for k, n0 in enumerate(range(0, N_P, T)):
            rows = min(T, N_P - n0)
            _lib.check(lib.gf_steady_sweep(*sweep_head(eng, rows, n0), p(steady), ARM, stream), "gf_steady_sweep")
            _lib.check(lib.gf_reduce_tile_steady(B, rows, n0, p(eng.d), p(eng.z), p(steady), p(eng.work), p(acc),
                                                 1 if k == 0 else 0, stream), "gf_reduce_tile_steady")
        torch.cuda.synchronize()
        hdr = steady.cpu().numpy()
        assert np.all(eng.info.cpu().numpy() == 0)
        assert np.all(hdr[:, 0] == SW) and np.all(hdr[:, 2] == 0.0), hdr[:, :3].tolist()
        zref = []
        for b in range(B):
            ac, bc, cc, dc = (np.asarray(v, dtype=np.float64) for v in coeffs[b][2:6])
            fz = dict(alpha=ac + 1j * bc, expo=(cc + 1j * dc) * hdr[b, ST_DT],
                      G=hdr[b, ST_GR:ST_GR + J] + 1j * hdr[b, ST_GI:ST_GI + J],
                      s=hdr[b, ST_SR:ST_SR + J] + 1j * hdr[b, ST_SI:ST_SI + J])
            zref.append(row_form(fz, y[SW:N_P]))
        zref = np.stack(zref)
        zref.setflags(write=False)
        ydev = torch.tensor(y, **f64)

        def fresh(n):
            return (steady.unsqueeze(0).repeat(n, 1, 1).contiguous(),
                    torch.tensor([0.0, 0.0, float("inf")], **f64).repeat(n, B, 1).contiguous())

        def variant(proven):
            return sweep_options(eng)[1] | (_lib.GF_SWEEP_AXIS_PROVEN if proven else 0)

        def finish(k, hdr_, acc_, proven, ybuf, window=None):
            """One launch over the first SW + k rows with y = ybuf (shared by the problems)."""
            head = finish_head(eng, SW + k, hdr_, acc_, y=ybuf, y_bs=0, variant=variant(proven))
            if window is None:
                _lib.check(lib.gf_steady_finish(*head, stream), "gf_steady_finish")
            else:
                _lib.check(lib.gf_steady_finish_window(*head, int(window[0]), int(window[1]), stream),
                           "gf_steady_finish_window")

        def chunked(k, hdr_, acc_, proven, ybuf, chunk_blocks=16):
            ws = torch.full((B, int(lib.gf_steady_chunk_size(SW + k, chunk_blocks))), float("nan"), **f64)
            head = finish_head(eng, SW + k, hdr_, acc_, y=ybuf, y_bs=0, variant=variant(proven))
            _lib.check(lib.gf_steady_finish_chunked(*head, 0, I64_MAX, chunk_blocks, p(ws), stream),
                       "gf_steady_finish_chunked")
            return ws

        made[J] = dict(eng=eng, hdr=hdr, zref=zref, y=ydev, fresh=fresh, finish=finish, chunked=chunked)
        return made[J]
    return get


def _exact(r, k):
    """y of the first SW + k rows in a tensor of exactly that length."""
    return r["y"][:SW + k].clone()


@pytest.mark.parametrize("proven", [False, True], ids=["tested", "proven"])
@pytest.mark.parametrize("J", J_CASES)
def test_tails_on_series_that_end_with_them(long_raws, J, proven):
    import torch
    r = long_raws(J)
    B, hdr, zref = B_FIN, r["hdr"], r["zref"]
    dinf = hdr[:, 1]
    n = len(TAILS)
    hp, ap = r["fresh"](n)              # one wave per problem
    hc, ac = r["fresh"](n)              # chunks of 16 blocks
    hw, aw = r["fresh"](n)              # two windows
    hn, an = r["fresh"](n)              # one row more, a NaN in it
    keep = []
    for i, k in enumerate(TAILS):
        yk = _exact(r, k)
        assert yk.shape == (SW + k,) and yk.is_contiguous()
        yn = torch.cat([yk, torch.full((1,), float("nan"), dtype=yk.dtype, device=yk.device)])
        keep += [yk, yn]
        r["finish"](k, hp[i], ap[i], proven, yk)
        keep.append(r["chunked"](k, hc[i], ac[i], proven, yk))
        r["finish"](k, hw[i], aw[i], proven, yk, window=(SW, SW + k + 1))       # holds everybody
        r["finish"](k, hw[i], aw[i], proven, yk, window=(1, SW))                # holds nobody
        r["finish"](k, hn[i], an[i], proven, yn)
    torch.cuda.synchronize()
    assert np.all(r["eng"].info.cpu().numpy() == 0)
    plain, chunk, hdp, hdc = ap.cpu().numpy(), ac.cpu().numpy(), hp.cpu().numpy(), hc.cpu().numpy()
    assert np.all(np.isfinite(plain)) and np.all(np.isfinite(hdp))
    assert np.array_equal(aw.cpu().numpy(), plain) and np.array_equal(hw.cpu().numpy(), hdp)
    assert np.array_equal(an.cpu().numpy(), plain) and np.array_equal(hn.cpu().numpy(), hdp)
    worst, worst_at, worst_ulp = 0.0, None, 0.0
    for i, k in enumerate(TAILS):
        what = f"J = {J}, {'proven' if proven else 'tested'}, tail of {k} rows"
        assert np.all(hdp[i, :, 2] == 0.0) and np.all(hdp[i, :, 0] == SW), what
        assert np.all(hdc[i, :, 2] == 0.0) and np.all(hdc[i, :, 0] == SW), what
        _against_plain(what, plain[i], chunk[i], hdp[i], hdc[i])
        if k <= 1024:                               # one chunk: the one-wave launch's own additions
            assert np.array_equal(chunk[i], plain[i]) and np.array_equal(hdc[i, :, 72:136], hdp[i, :, 72:136]), what
        for b in range(B):
            z = zref[b, :k]
            zmax, zabs = float(np.max(np.abs(z))), float(np.sum(np.abs(z)))
            z2d = float(np.sum(z * z) / np.longdouble(dinf[b]))
            assert plain[i, b, 2] == dinf[b], (what, b)
            ulp = _ulps(plain[i, b, 0], k * np.log(dinf[b]))
            err = abs(plain[i, b, 1] - z2d)
            bar = 2.0 * RTOL_Z * zmax * zabs / dinf[b] + RTOL_Z * z2d
            if err / bar > worst:
                worst, worst_at = err / bar, (k, b)
            worst_ulp = max(worst_ulp, ulp)
            assert ulp <= ULP_LOGD, (what, b, plain[i, b, 0], k * np.log(dinf[b]))
            assert err <= bar, (what, b, plain[i, b, 1], z2d, err / bar)
            errc = abs(chunk[i, b, 1] - z2d)
            assert errc <= bar, (what, b, "chunked", errc / bar)
    print(f"J = {J:2d} (ROWS = {(2 * J + 3) // 4 * 4:2d}), {'proven' if proven else 'tested'}: sum z^2/d against the "
          f"longdouble row form, error / bar {worst:.1e} at a tail of {worst_at[0]} rows (problem {worst_at[1]}), "
          f"k log d_inf {worst_ulp:.1f} ulp")


@pytest.mark.parametrize("J", (2, 30))
def test_proven_and_tested_instances_agree_bit_for_bit(long_raws, J):
    """The two kinds of instance on the exact buffers, one wave and chunks of 16 and of 32 blocks."""
    import torch
    r = long_raws(J)
    res, keep = [], []
    for proven in (False, True):
        hd, ac = r["fresh"](3 * len(TAILS))
        for i, k in enumerate(TAILS):
            yk = _exact(r, k)
            keep.append(yk)
            r["finish"](k, hd[3 * i], ac[3 * i], proven, yk)
            keep.append(r["chunked"](k, hd[3 * i + 1], ac[3 * i + 1], proven, yk, 16))
            keep.append(r["chunked"](k, hd[3 * i + 2], ac[3 * i + 2], proven, yk, 32))
        torch.cuda.synchronize()
        res.append((ac.cpu().numpy(), hd.cpu().numpy()))
    assert np.all(np.isfinite(res[0][0]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
