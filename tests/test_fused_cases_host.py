"""CPU: pins what tests/fused_cases.py claims -- the float64 C oracle against the 80-bit recurrence on these axes, the
health of every problem that tests/test_gpu_fused_rows.py runs, the row kinds that the composite axis and its stretches
reach in RowGen::advance, that the far axis tells rounded phases from exact ones, and that the structure lists reach
every kernel instance."""
import numpy as np
import pytest

from tests import fused_cases as fc
from tests import sweep_cases as sc


@pytest.mark.parametrize("s", [(1, 0), (0, 1), (1, 15), (0, 31), (1, 31), (0, 44), (0, 88)], ids=fc.ident)
def test_c_oracle_against_the_80_bit_recurrence(s):
    """d and z of the float64 C oracle against oracle/seq.py in np.longdouble throughout (W = 1, 2, 31, 62, 63, 88,
    176), relative to the largest entry: within 1e-13 on the composite axis (measured 4e-15 worst), within 1e-11 on
    the stretched ones (measured 5e-13 worst).  The distance on the stretched axes is not the C oracle's error: the
    80-bit build takes sin / cos of the 80-bit product d t, celerite2 -- and the C oracle -- of the product rounded
    to float64, half an ulp of a phase of up to a few thousand radians there."""
    Jr, Jc = s
    worst = {}
    for name, bound in (("composite", 1e-13), ("stretch28", 1e-11), ("stretch128", 1e-11), ("gap102", 1e-11)):
        ref = fc.rows(Jr, Jc, name)[0]
        d, z = fc.rows_80bit(Jr, Jc, name)
        worst[name] = (sc.relerr(ref["d"], d), sc.relerr(ref["z"], z))
        assert max(worst[name]) <= bound, (name, worst[name])
    print(fc.ident((Jr, Jc)) + ": " + ", ".join(f"{k} d {v[0]:.1e} z {v[1]:.1e}" for k, v in worst.items()))


def _healthy(refs, what):
    for r in refs:
        assert r["info"] == 0 and np.min(r["d"]) > 0, what
        assert np.max(r["a"]) / np.min(r["d"]) < 100.0, (what, np.max(r["a"]) / np.min(r["d"]))
    return max(np.max(r["a"]) / np.min(r["d"]) for r in refs), min(np.max(r["a"]) / np.min(r["d"]) for r in refs)


def test_every_problem_is_positive_definite_with_a_condition_below_100():
    """Every (structure, axis, diagonal) that the GPU module runs; on the composite axis the conditions max(a) / min(d)
    are 7.8..15.9 at the widths 1, 2, 31, 62, 63, 88, 176."""
    for s in fc.NARROW:
        _healthy(fc.rows(*s), s)
    for s in fc.WIDE:
        _healthy(fc.rows(*s, B=2), s)
    for s in fc.GRID:
        for name in ("stretch28", "gap098", "gap102") + (("stretch128",) if s[0] + 2 * s[1] <= 63 else ()):
            _healthy(fc.rows(*s, name), (s, name))
        _healthy(fc.rows(*s, "composite", 385), (s, 385))
        for n in (1, 2, 3):
            _healthy(fc.rows(*s, "composite", n), (s, n))
    for s in fc.LAYOUT:
        for name, diag in (("own", "own"), ("composite", "shared")):
            _healthy(fc.rows(*s, name, diag=diag), (s, name, diag))
    for s in fc.FAR:
        for name in ("near", "far"):
            _healthy(fc.rows(*s, name, fc.N_FAR), (s, name))
    for s in ((1, 0), (0, 1), (1, 15), (0, 31), (1, 31), (0, 44), (0, 88)):
        hi, lo = _healthy(fc.rows(*s), s)
        assert 7.0 <= lo and hi <= 17.0, (s, lo, hi)


def test_without_a_diagonal_the_problems_stay_positive_definite():
    """diag = NULL leaves the shift 0.01 amp alone on the kernel's diagonal: conditions of 69..73, below 100 as
    everywhere else."""
    for s in fc.LAYOUT:
        for r in fc.rows(*s, diag="none"):
            cond = np.max(r["a"]) / np.min(r["d"])
            assert r["info"] == 0 and cond < 100.0, (s, cond)


def test_failing_pivots_fail_where_the_diagonal_turns():
    for s in fc.FAIL:
        for r in fc.FAIL_ROWS:
            refs = fc.rows(*s, B=2, fail=(1, r))
            assert refs[0]["info"] == 0 and refs[1]["info"] == r + 1
            assert len(refs[1]["d"]) == len(refs[1]["z"]) == len(refs[1]["draw"]) == r
            if r:
                good = fc.rows(*s, B=2)[1]
                assert np.array_equal(refs[1]["d"], good["d"][:r]) and np.array_equal(refs[1]["z"], good["z"][:r])


def test_row_kinds_of_the_composite_axis():
    """At block 64 every branch of RowGen::advance is taken at least 3 times at the periods 16 and 64 (3 is what the
    axis is built for: its three changes of cadence re-cache the multiplier once each); period 1 takes no rotation
    step; block 1 makes every row an anchor."""
    t = fc.composite_axis()
    prob = fc.problem(0, 31)
    for b in range(3):
        wmax, cmax = prob["wmax"][b], prob["cmax"][b]
        k16 = fc.row_kinds(t, wmax, cmax, 64, 16)
        k64 = fc.row_kinds(t, wmax, cmax, 64, 64)
        print(f"problem {b}: period 16 {k16}, period 64 {k64}")
        assert k16["anchor"] == 7 and k16["sub_anchor"] == 15 and k16["exact"] == 71 and k16["refresh"] == 3
        assert k16["first_order"] + k16["second_order"] == 291 and k16["first_order"] >= 231
        assert k64["anchor"] == 7 and k64["sub_anchor"] == 0 and k64["exact"] == 71 and k64["refresh"] == 3
        for k in (k16, k64):
            assert all(k[kind] >= 3 for kind in fc.KINDS if not (k is k64 and kind == "sub_anchor")), k
        k1 = fc.row_kinds(t, wmax, cmax, 64, 1)
        assert k1["first_order"] == k1["second_order"] == 0 and k1["anchor"] == 7
        assert fc.row_kinds(t, wmax, cmax, 1, 16)["anchor"] == fc.N
    # period 64 at block 64 has no sub-anchor of its own: the periods 2 .. 32 of the grid have
    assert fc.row_kinds(t, prob["wmax"][0], prob["cmax"][0], 64, 32)["sub_anchor"] >= 3


def test_row_kinds_of_the_stretched_axes():
    """The gap pair: with a regular row at 0.98 of the reset gap only the block rows and the one gap reset (7 anchors),
    at 1.02 every row of the problem with the largest cmax resets on its own (384 anchors).  The 0.98-stretches of the
    block rule keep rows of every kind (the 63 rows of the doubled cadence now reset on their own)."""
    for s in fc.GRID:
        prob = fc.problem(*s)
        b = int(np.argmax(prob["cmax"]))
        wmax, cmax = prob["wmax"][b], prob["cmax"][b]
        assert fc.row_kinds(fc.axis("gap098", *s), wmax, cmax, 64, 16)["anchor"] == 7
        assert fc.row_kinds(fc.axis("gap102", *s), wmax, cmax, 64, 16)["anchor"] == fc.N
        for name, span in (("stretch28", fc.SPAN), ("stretch128", fc.SPAN_LONG)):
            t = fc.axis(name, *s)
            assert np.isclose(1.5 * 63 * cmax * (t[1] - t[0]), 0.98 * span, rtol=1e-12)
            k = fc.row_kinds(t, wmax, cmax, 64, 16, span)
            assert k["anchor"] == 7 + 63 and k["exact"] >= 3 and k["refresh"] >= 1, (s, name, k)
            assert k["sub_anchor"] >= 3, (s, name, k)
            assert k["first_order"] + k["second_order"] >= 100, (s, name, k)


def test_row_kinds_of_the_jitter_axis():
    """Every rotation step is a second-order one, for the problem with the largest wmax at 0.78..0.98 of the limit."""
    for s in fc.GRID:
        prob = fc.problem(*s)
        t = fc.axis("jitter", *s)
        x = np.abs(np.diff(t)[2:] - fc.DT) * np.max(prob["wmax"])
        assert 0.78 * 2e-6 < np.min(x) and np.max(x) < 0.981 * 2e-6
        for b in range(3):
            k = fc.row_kinds(t, prob["wmax"][b], prob["cmax"][b], 64, 64)
            assert k["second_order"] == fc.N - 6 - 2 and k["exact"] == 2 and k["first_order"] == 0, (s, b, k)
        for r in fc.rows(*s, "jitter"):
            assert r["info"] == 0 and np.max(r["a"]) / np.min(r["d"]) < 100.0


def test_the_far_axis_tells_rounded_phases_from_exact_ones():
    """far - SHIFT is the near axis exactly, so both describe the same spacings; what differs is celerite2's phase
    fl(d t), rounded at up to 3e8 rad on the far axis.  On structures with complex terms the C oracle's rows on the two axes
    differ -- in the problem where they differ most, every problem is asserted on the device -- by at least 5 TOL in
    d and 50 TOL in z (measured 9e-10..1.3e-9 and 8e-9..1.6e-8): a sweep that ignored the rounded phases fails at TOL.
    All-real structures have no phase: the rows agree to the bit.  The rounding jitter of the far grid (1.5e-11) lies
    between the two step thresholds: qmode runs with the second-order step."""
    near, far = fc.far_axes()
    assert np.array_equal(far - fc.SHIFT, near) and np.array_equal(near + fc.SHIFT, far)
    assert np.max(np.abs(near - fc.composite_axis()[:fc.N_FAR])) <= 0.5 * np.spacing(fc.SHIFT)
    for s in fc.FAR + ((0, 1), (0, 16), (0, 31), (1, 31)):
        prob = fc.problem(*s, fc.N_FAR)
        a, b = fc.rows(*s, "near", fc.N_FAR), fc.rows(*s, "far", fc.N_FAR)
        dd = max(sc.relerr(x["d"], y["d"]) for x, y in zip(a, b))
        dz = max(sc.relerr(x["z"], y["z"]) for x, y in zip(a, b))
        if s[1] == 0:
            assert dd == 0.0 and dz == 0.0
            continue
        print(f"{fc.ident(s)}: near - far d {dd:.1e}, z {dz:.1e}")
        assert dd >= 5 * fc.TOL and dz >= 50 * fc.TOL, (s, dd, dz)
        assert np.all(prob["wmax"] * fc.SHIFT > 4e6)
        for bb in range(3):
            k = fc.row_kinds(far, prob["wmax"][bb], prob["cmax"][bb], 64, 16)
            kn = fc.row_kinds(near, prob["wmax"][bb], prob["cmax"][bb], 64, 16)
            assert k["first_order"] == 0 and k["second_order"] >= 100 and kn["second_order"] >= 50, (s, k, kn)


def test_the_structure_lists_reach_every_instance():
    """16 row counts R of k_factor3 (any terms) and of k_factor7 (Jr = 0), each at both pad parities -- a width that
    fills R and one that leaves pad rows --, and the 11 shapes of k_factorw on both sides of every dispatch line."""
    assert [s[0] + 2 * s[1] for s in fc.NARROW[:63]] == list(range(1, 64))
    for group, widths in ((fc.NARROW, range(1, 64)), (fc.TILED, range(2, 64, 2))):
        hit = {}
        for s in group:
            hit.setdefault(fc.rows_of(s[0] + 2 * s[1]), set()).add(s[0] + 2 * s[1])
        assert sorted(hit) == list(range(4, 65, 4))
        for R, ws in hit.items():
            assert {w for w in widths if fc.rows_of(w) == R} <= ws
    assert [s[1] for s in fc.TILED] == list(range(1, 32))
    shapes = [fc.wide_shape(2 * Jc) for _, Jc in fc.WIDE]
    assert sorted(set(shapes)) == [(16, 3), (20, 3), (24, 3), (24, 4), (28, 4), (32, 4), (32, 5), (36, 5), (40, 5),
                                   (40, 6), (44, 6)]
    assert all(shapes.count(x) >= 1 for x in shapes) and shapes[0] == (16, 3) and shapes[-1] == (44, 6)
    for s in fc.GRID + fc.FAR + fc.LAYOUT + fc.FAIL:
        assert s in fc.NARROW or s in fc.WIDE or s == (0, 44) or s == (0, 16)
