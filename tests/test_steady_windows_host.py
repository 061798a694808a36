"""Host: the window arithmetic of the overlapped finishing schedule as pure functions of the feedback
-- gadfly_amd.engine.steady_boundaries, steady_windows, steady_chunk_blocks, steady_final_chunk_blocks: the windows are
disjoint and cover every switch row 1 .. N whatever the feedback, the boundaries are ends of tiles in the order the
schedule needs, chunk sizes are powers of two >= 16 that keep their promise, and degenerate feedback gives fewer
launches, never a hole."""
import itertools

import pytest

from gadfly_amd.engine import (STEADY_SW_MAX, steady_boundaries, steady_chunk_blocks, steady_final_chunk_blocks,
                               steady_windows)

SERIES = [(1_000_000, 8192), (65536, 8192), (16384 + 37, 4096), (4096, 4096), (100, 64), (8192 * 3 + 1, 8192)]


def _rows(N, T):
    """Feedback rows worth trying: 0 (unknown), the ends and starts of tiles, the series' ends and beyond."""
    r = {0, 1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, N // 2, N - T, N - 1, N, N + 1, N + 5 * T}
    return sorted(v for v in r if v >= 0)


def _check_cover(windows, N):
    assert windows[0][0] == 1 and windows[-1][1] == STEADY_SW_MAX > N + 1
    for (lo, hi), (lo2, _) in zip(windows, windows[1:]):
        assert lo < hi == lo2                       # disjoint, no hole, none empty
    assert all(lo < hi for lo, hi in windows)
    for sw in (1, 2, N // 2, N - 1, N):             # every switch row in exactly one window
        assert sum(lo <= sw < hi for lo, hi in windows) == 1


@pytest.mark.parametrize("N,T", SERIES)
def test_windows_are_a_disjoint_cover_for_any_feedback(N, T):
    ntiles = (N + T - 1) // T
    seen = set()
    for most, mid, latest in itertools.product(_rows(N, T), repeat=3):
        split, mid_end = steady_boundaries(N, T, most, mid, latest)
        windows = steady_windows(split, mid_end)
        seen.add(len(windows))
        _check_cover(windows, N)
        assert split % T == 0 and mid_end % T == 0
        if split:
            k_e = split // T - 1
            assert 0 <= k_e < ntiles - 1 and most <= split < latest and split - most < T
        else:
            assert mid_end == 0 and len(windows) == 1
        if mid_end:
            k_m = mid_end // T - 1
            assert split // T - 1 < k_m < ntiles - 1 and mid <= mid_end < latest and mid_end - mid < T
            assert windows == [(1, split + 1), (split + 1, mid_end + 1), (mid_end + 1, STEADY_SW_MAX)]
    assert seen == ({1, 2, 3} if ntiles >= 3 else {1, 2} if ntiles == 2 else {1})


def test_the_headline():
    """Round 21's switch rows: all but B/8 switch in tiles 3 and 4, all but B/64 by tile 6, the last one in tile 8."""
    N, T = 1_000_000, 8192
    assert steady_boundaries(N, T, 38000, 55000, 72577) == (5 * T, 7 * T)
    assert steady_windows(5 * T, 7 * T) == [(1, 40961), (40961, 57345), (57345, STEADY_SW_MAX)]
    assert steady_chunk_blocks(N, 8) == 2048                        # 8 chunks of 2048 blocks
    cb = steady_final_chunk_blocks(N, 2048, 1024)
    assert cb == 512 and -(-N // (64 * cb)) == 31                   # 32 problems x 31 chunks <= 1024 SIMDs


def test_degenerate_feedback():
    N, T = 1_000_000, 8192
    assert steady_boundaries(N, T, 0, 0, 0) == (0, 0)               # nothing switched: one launch
    assert steady_boundaries(N, T, 0, 0, 5000) == (0, 0)            # fewer than B - B/8 switched at all
    assert steady_boundaries(N, T, 100, 200, 300) == (0, 0)         # everything in one tile
    assert steady_boundaries(N, T, 100, 200, T) == (0, 0)           # ... up to its last row
    assert steady_boundaries(N, T, 100, 200, T + 1) == (T, 0)       # the latest one tile on: the middle is the split's
    assert steady_boundaries(N, T, 100, 0, 5 * T) == (T, 0)         # fewer than B - B/64 switched: no middle
    assert steady_boundaries(N, T, 100, 3 * T, 3 * T) == (T, 0)     # nobody expected behind the middle
    assert steady_boundaries(N, T, 100, 3 * T, 3 * T + 1) == (T, 3 * T)
    assert steady_boundaries(N, T, 100, N + 5 * T, N + 6 * T) == (T, 0)     # k_m beyond the series
    assert steady_boundaries(N, T, N + T, N + 5 * T, N + 6 * T) == (0, 0)
    last = (N - 1) // T                                             # k_m the last tile: unusable
    assert steady_boundaries(N, T, 100, last * T + 5, N) == (T, 0)
    assert steady_boundaries(N, T, 100, last * T, N) == (T, last * T)
    assert steady_boundaries(N, T, last * T, last * T + 1, N) == (last * T, 0)
    assert steady_boundaries(N, T, last * T + 1, last * T + 2, N) == (0, 0)     # the split's own tile the last one
    assert steady_windows(0, 0) == [(1, STEADY_SW_MAX)] and steady_windows(0, 3 * T) == [(1, STEADY_SW_MAX)]


@pytest.mark.parametrize("N", [1, 63, 64, 1024, 1025, 16384 + 37, 65536, 1_000_000, 10_000_000])
def test_chunk_blocks_are_powers_of_two_that_keep_their_promise(N):
    for chunks in (1, 2, 8, 31, 32, 1024, 0, -3):
        cb = steady_chunk_blocks(N, chunks)
        want = max(chunks, 1)
        assert cb >= 16 and cb & (cb - 1) == 0
        assert -(-N // (64 * cb)) <= want                           # at most that many chunks
        assert cb == 16 or -(-N // (64 * (cb // 2))) > want         # and no smaller power of two does
    for B, simds in ((2048, 1024), (64, 1024), (1, 1024), (4096, 1024), (100_000, 1024), (2048, 4), (2048, 0)):
        cb = steady_final_chunk_blocks(N, B, simds)
        assert cb >= 16 and cb & (cb - 1) == 0
        problems, chunks = max(1, B // 64), -(-N // (64 * cb))
        assert problems * chunks <= simds or chunks == 1            # (more problems than SIMDs: one chunk each)
        assert cb == steady_chunk_blocks(N, max(1, simds // problems))
