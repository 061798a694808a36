// Shared between the translation units of libgadfly_hip.so; NOT part of the C-ABI (hidden visibility).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/gadfly_hip.h"

// records the message gf_last_error() returns (thread-local) and returns `code`
__attribute__((visibility("hidden"), format(printf, 2, 3)))
int gf_internal_error(int code, const char *fmt, ...);

// hipGetLastError() -> 0, or -2 with the message recorded
__attribute__((visibility("hidden")))
int gf_internal_check_launch(const char *what);

// opt a set of kernels in to `bytes` (> 64 KB) of dynamic LDS on the device the stream belongs to; remembered per
// (which, device).  false if the attribute could not be set.
__attribute__((visibility("hidden")))
bool gf_internal_lds_opt_in(int which, hipStream_t st, const void *const *funcs, int nfuncs, size_t bytes);

// ---- host-side helpers of the entry points (every unit its own copy) ----
static inline int check_launch(const char *what) { return gf_internal_check_launch(what); }

// Kernels that exist per value of an int template argument: dispatch_among calls f with
// std::integral_constant<int, V> for the V that equals v, and says whether there was one.
template <int... V, class F>
constexpr bool dispatch_among(int v, F &&f) {
    return ((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}
// the one-wave kernels' row count: the width rounded up to a multiple of 4 (the ladder is written here alone)
template <class F>
constexpr bool dispatch_rows(int rows, F &&f) {
    return dispatch_among<4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64>(rows, f);
}
// A wrong instance for a width is a fault on the device, not a failed assertion: every multiple of 4 in 4 .. 64
// selects the instance of that many rows, and no other count (0, 2 and 68 among them) selects any.
constexpr bool dispatch_rows_exact() {
    for (int rows = -4; rows <= 72; ++rows) {
        int got = -1;
        dispatch_rows(rows, [&](auto r) { got = decltype(r)::value; });
        if (got != ((rows >= 4 && rows <= 64 && rows % 4 == 0) ? rows : -1)) return false;
    }
    return true;
}
static_assert(dispatch_rows_exact(), "dispatch_rows: rows must select the instance R == rows, in 4, 8, .., 64 only");

// Argument checks the entry points share: 0, or -1 with "<who>: ..." recorded.
static inline int check_block(const char *who, int block) {
    if (block < 1 || block > 64 || (block & (block - 1)))
        return gf_internal_error(-1, "%s: block=%d must be a power of two in 1..64", who, block);
    return 0;
}
static inline int check_n_first(const char *who, int64_t n_first, int block) {        // (behind check_block)
    if (n_first < 0 || (n_first % block) != 0)
        return gf_internal_error(-1, "%s: n_first=%lld must be a non-negative multiple of block=%d", who,
                                 (long long)n_first, block);
    return 0;
}
// nch chunks of chunk_len rows cover the N rows, none of them empty; more than one chunk: chunk_len is a multiple
// of `quantum` (the sweeps: their scaling block; the transitions: 64; 1: any length)
static inline int check_chunking(const char *who, int64_t N, int64_t chunk_len, int nch, int quantum) {
    if (nch < 1 || chunk_len < 1 || (nch > 1 && (chunk_len % quantum) != 0) || (int64_t)nch * chunk_len < N
        || (int64_t)(nch - 1) * chunk_len >= N)
        return gf_internal_error(-1, "%s: bad chunking (chunk_len=%lld, nch=%d)", who, (long long)chunk_len, nch);
    return 0;
}
static inline int check_chunk_range(const char *who, int chunk_first, int chunk_count, int nch) {
    if (chunk_first < 0 || chunk_count < 0 || chunk_first + chunk_count > nch)
        return gf_internal_error(-1, "%s: bad chunk range (first=%d, count=%d)", who, chunk_first, chunk_count);
    return 0;
}
static inline int check_ld(const char *who, int W, int ld) {
    if (ld < W || (ld & 15))
        return gf_internal_error(-1, "%s: ld=%d must be a multiple of 16 and >= W=%d", who, ld, W);
    return 0;
}
static inline int check_width_ld(const char *who, int W, int ld) {
    if (W < 1 || W > GF_MAX_WIDTH)
        return gf_internal_error(-1, "%s: width %d unsupported (max %d)", who, W, GF_MAX_WIDTH);
    return check_ld(who, W, ld);
}
