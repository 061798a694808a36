// gadfly_detrend.hip -- raw observing quarters to detrended ppm series, S segments (star x quarter) per launch
//
// Reference being replaced: the detrend=True branch of PowerSpectrum.from_light_curve (gadfly/psd.py:482-535):
// per quarter remove_nans().remove_outliers() (a sigma clip about the median), a polynomial in time divided out,
// 1e6 (f / median - 1).  The segments live in concatenated arrays with an int64 offset table off [S + 1]; one
// workgroup owns one segment and every element of a segment is always handled by the same thread, so a segment's
// result is a function of its own data alone:
//   k_seg_median      exact median (the value numpy.median returns): radix select on order-preserving 64-bit keys,
//                     8 passes of 8 bits with an integer histogram in LDS; an even count averages the two middle ones
//   k_sigma_clip      all rounds of the clip in one launch: median, mean, population std, mask, early stop
//   k_seg_count / k_seg_scan / k_seg_compact   stable compaction of (t, f) by the mask, with new offsets
//   k_seg_diff        t[i + 1] - t[i] inside each segment (the cadence is its median)
//   k_poly_normalise  least-squares Legendre fit on u = (t - mid) / half: Gram matrix and right-hand side in a fixed
//                     order, Cholesky on chip, f / fit
//   k_seg_ppm         1e6 (x / median - 1)
// No floating-point atomics: every sum is per-thread strided, then a wave shuffle tree, then the waves in order.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"

#pragma clang fp contract(off)      // numpy rounds every product and sum on its own (no FMA)

namespace {

constexpr int DT_THREADS = 1024;            // the select, clip and copy kernels
constexpr int DT_WAVES = DT_THREADS / 64;
constexpr int DT_FIT_THREADS = 256;         // k_poly_normalise keeps 54 running sums per thread in registers
constexpr int DT_FIT_WAVES = DT_FIT_THREADS / 64;
constexpr int DT_K = GF_DETREND_MAX_ORDER + 1;          // Legendre polynomials P_0 .. P_8
constexpr int DT_GRAM = DT_K * (DT_K + 1) / 2;          // upper triangle of the Gram matrix
constexpr int DT_SUMS = DT_GRAM + DT_K;                 // ... and the right-hand side

typedef unsigned long long u64;

// order-preserving key of a finite double (-0 and +0 share a key)
__device__ __forceinline__ u64 key_of(double x) {
    const u64 b = (u64)__double_as_longlong(x + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct BlockScratch {
    u64 hist[256];
    u64 scan[256];
    double redd[DT_WAVES];
    u64 redu[DT_WAVES];
    int sel_bin;
    u64 sel_before;
};

// Sums over the workgroup in a fixed order (lanes by a shuffle tree, then the waves in order); all threads get it.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < WAVES; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ u64 block_count(u64 v, u64 *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
    for (int w = 0; w < DT_WAVES; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ u64 block_min(u64 v, u64 *red) {
    for (int o = 32; o > 0; o >>= 1) { const u64 u = __shfl_down(v, o, 64); v = u < v ? u : v; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = ~0ull;
    for (int w = 0; w < DT_WAVES; ++w) s = red[w] < s ? red[w] : s;
    return s;
}

// The key of rank r (0-based, r < the number of kept elements) among the kept elements i in [0, n):
// key_at(i, &k) says whether element i is kept and gives its key.  Called by all DT_THREADS threads.
template <class KeyAt>
__device__ u64 block_select(KeyAt key_at, int64_t n, u64 r, BlockScratch &sh) {
    const int tid = threadIdx.x;
    u64 prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();
        if (tid < 256) sh.hist[tid] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += DT_THREADS) {
            u64 k;
            if (!key_at(i, k)) continue;
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8)))
                atomicAdd(&sh.hist[(k >> shift) & 255], 1ull);
        }
        __syncthreads();
        if (tid < 256) sh.scan[tid] = sh.hist[tid];
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const u64 u = (tid < 256 && tid >= o) ? sh.scan[tid - o] : 0;
            __syncthreads();
            if (tid < 256) sh.scan[tid] += u;
            __syncthreads();
        }
        if (tid < 256) {
            const u64 incl = sh.scan[tid], before = incl - sh.hist[tid];
            if (before <= r && r < incl) { sh.sel_bin = tid; sh.sel_before = before; }
        }
        __syncthreads();
        prefix |= (u64)sh.sel_bin << shift;
        r -= sh.sel_before;
    }
    return prefix;
}

// numpy.median of the m kept elements: the middle one, or (a + b) / 2 of the two middle ones; NaN if none
template <class KeyAt>
__device__ double block_median(KeyAt key_at, int64_t n, u64 m, BlockScratch &sh) {
    if (m == 0) return __longlong_as_double(0x7ff8000000000000ll);
    const u64 klo = block_select(key_at, n, (m - 1) / 2, sh);
    if (m & 1) return value_of(klo);
    u64 n_le = 0, next = ~0ull;                 // rank m / 2 holds klo again, or the smallest key above it
    for (int64_t i = threadIdx.x; i < n; i += DT_THREADS) {
        u64 k;
        if (!key_at(i, k)) continue;
        if (k <= klo) ++n_le;
        else if (k < next) next = k;
    }
    n_le = block_count(n_le, sh.redu);
    next = block_min(next, sh.redu);
    const u64 khi = (n_le >= m / 2 + 1) ? klo : next;
    return (value_of(klo) + value_of(khi)) / 2.0;
}

__global__ __launch_bounds__(DT_THREADS) void k_seg_median(const int64_t *__restrict__ off,
                                                           const double *__restrict__ x,
                                                           const uint8_t *__restrict__ keep, const int drop_last,
                                                           double *__restrict__ med) {
    __shared__ BlockScratch sh;
    const int s = blockIdx.x;
    const int64_t b = off[s];
    int64_t n = off[s + 1] - b - drop_last;
    if (n < 0) n = 0;
    auto key_at = [&](int64_t i, u64 &k) {
        if (keep && !keep[b + i]) return false;
        k = key_of(x[b + i]);
        return true;
    };
    u64 m = (u64)n;
    if (keep) {
        u64 c = 0;
        for (int64_t i = threadIdx.x; i < n; i += DT_THREADS) c += keep[b + i] ? 1 : 0;
        m = block_count(c, sh.redu);
    }
    const double v = block_median(key_at, n, m, sh);
    if (threadIdx.x == 0) med[s] = v;
}

// Element b + i is read and written by thread i % DT_THREADS alone, in every pass: no pass waits for another
// thread's global store.
__global__ __launch_bounds__(DT_THREADS) void k_sigma_clip(const int64_t *__restrict__ off,
                                                           const double *__restrict__ t,
                                                           const double *__restrict__ f, const double sigma_lower,
                                                           const double sigma_upper, const int maxiters,
                                                           uint8_t *__restrict__ keep, int64_t *__restrict__ kept,
                                                           int *__restrict__ rounds) {
    __shared__ BlockScratch sh;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t b = off[s], n = off[s + 1] - b;
    u64 c = 0;
    for (int64_t i = tid; i < n; i += DT_THREADS) {
        const bool k = isfinite(f[b + i]) && (!t || isfinite(t[b + i]));
        keep[b + i] = k ? 1 : 0;
        c += k ? 1 : 0;
    }
    u64 m = block_count(c, sh.redu);
    auto key_at = [&](int64_t i, u64 &k) {
        if (!keep[b + i]) return false;
        k = key_of(f[b + i]);
        return true;
    };
    int r = 0;
    while (m > 0 && (maxiters < 0 || r < maxiters)) {
        ++r;
        const double med = block_median(key_at, n, m, sh);
        double a = 0.0;
        for (int64_t i = tid; i < n; i += DT_THREADS)
            if (keep[b + i]) a += f[b + i];
        const double mean = block_sum<DT_WAVES>(a, sh.redd) / (double)m;
        a = 0.0;
        for (int64_t i = tid; i < n; i += DT_THREADS)
            if (keep[b + i]) { const double d = f[b + i] - mean; a += d * d; }
        const double sd = sqrt(block_sum<DT_WAVES>(a, sh.redd) / (double)m);
        const double lo = med - sigma_lower * sd, hi = med + sigma_upper * sd;
        u64 gone = 0;
        for (int64_t i = tid; i < n; i += DT_THREADS)
            if (keep[b + i] && !(f[b + i] >= lo && f[b + i] <= hi)) { keep[b + i] = 0; ++gone; }
        gone = block_count(gone, sh.redu);
        if (gone == 0) break;
        m -= gone;
    }
    if (tid == 0) { kept[s] = (int64_t)m; rounds[s] = r; }
}

__global__ __launch_bounds__(DT_THREADS) void k_seg_count(const int64_t *__restrict__ off,
                                                          const uint8_t *__restrict__ keep,
                                                          int64_t *__restrict__ new_off) {
    __shared__ u64 red[DT_WAVES];
    const int s = blockIdx.x;
    const int64_t b = off[s], n = off[s + 1] - b;
    u64 c = 0;
    for (int64_t i = threadIdx.x; i < n; i += DT_THREADS) c += keep[b + i] ? 1 : 0;
    c = block_count(c, red);
    if (threadIdx.x == 0) new_off[s] = (int64_t)c;
}

// exclusive scan of v[0 .. S) in place, the total to v[S] (one workgroup, any S)
__global__ __launch_bounds__(256) void k_seg_scan(const int S, int64_t *__restrict__ v) {
    __shared__ int64_t part[256];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += 256) {
        const int i = s0 + (int)threadIdx.x;
        const int64_t mine = (i < S) ? v[i] : 0;
        part[threadIdx.x] = mine;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int64_t u = ((int)threadIdx.x >= o) ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += u;
            __syncthreads();
        }
        if (i < S) v[i] = carry + part[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 0) carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) v[S] = carry;
}

__global__ __launch_bounds__(DT_THREADS) void k_seg_compact(const int64_t *__restrict__ off,
                                                            const uint8_t *__restrict__ keep,
                                                            const double *__restrict__ t,
                                                            const double *__restrict__ f,
                                                            const int64_t *__restrict__ new_off,
                                                            double *__restrict__ t_out, double *__restrict__ f_out) {
    __shared__ int wsum[DT_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t b = off[s], n = off[s + 1] - b, ob = new_off[s], room = new_off[s + 1] - ob;
    int64_t base = 0;
    for (int64_t i0 = 0; i0 < n; i0 += DT_THREADS) {
        const int64_t i = i0 + tid;
        const bool k = i < n && keep[b + i];
        const u64 bal = __ballot(k);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int j = 0; j < DT_WAVES; ++j) { const int cw = wsum[j]; before += (j < w) ? cw : 0; total += cw; }
        const int64_t o = base + before + rank;
        if (k && o < room) { t_out[ob + o] = t[b + i]; f_out[ob + o] = f[b + i]; }   // (room: the mask as counted)
        base += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(DT_THREADS) void k_seg_diff(const int64_t *__restrict__ off,
                                                         const double *__restrict__ t, double *__restrict__ d) {
    const int s = blockIdx.x;
    const int64_t b = off[s], n = off[s + 1] - b;
    for (int64_t i = threadIdx.x; i + 1 < n; i += DT_THREADS) d[b + i] = t[b + i + 1] - t[b + i];
    if (threadIdx.x == 0 && n > 0) d[b + n - 1] = 0.0;
}

__device__ __forceinline__ void legendre(const double u, double *P) {
    P[0] = 1.0;
    P[1] = u;
#pragma unroll
    for (int j = 1; j + 1 < DT_K; ++j) P[j + 1] = ((double)(2 * j + 1) * u * P[j] - (double)j * P[j - 1]) / (double)(j + 1);
}

__global__ __launch_bounds__(DT_FIT_THREADS) void k_poly_normalise(const int64_t *__restrict__ off,
                                                                   const double *__restrict__ t,
                                                                   const double *__restrict__ f, const int order,
                                                                   double *__restrict__ out, int *__restrict__ info) {
    __shared__ double part[DT_FIT_WAVES][DT_SUMS];
    __shared__ double sums[DT_SUMS];
    __shared__ double L[DT_K][DT_K];
    __shared__ double coef[DT_K];
    __shared__ int bad;
    const int s = blockIdx.x, tid = threadIdx.x, K = order + 1;
    const int64_t b = off[s], n = off[s + 1] - b;
    if (n <= 0) {
        if (tid == 0) info[s] = 1;
        return;
    }
    const double t0 = t[b], tl = t[b + n - 1];
    const double mid = 0.5 * (t0 + tl), half = 0.5 * (tl - t0);
    double acc[DT_SUMS];
#pragma unroll
    for (int q = 0; q < DT_SUMS; ++q) acc[q] = 0.0;
    for (int64_t i = tid; i < n; i += DT_FIT_THREADS) {
        const double u = (half != 0.0) ? (t[b + i] - mid) / half : 0.0, y = f[b + i];
        double P[DT_K];
        legendre(u, P);
        int q = 0;
#pragma unroll
        for (int a = 0; a < DT_K; ++a)
#pragma unroll
            for (int c = a; c < DT_K; ++c) acc[q++] += P[a] * P[c];
#pragma unroll
        for (int a = 0; a < DT_K; ++a) acc[DT_GRAM + a] += P[a] * y;
    }
#pragma unroll
    for (int q = 0; q < DT_SUMS; ++q) {
        double v = acc[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0) part[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < DT_SUMS) {
        double v = 0.0;
        for (int w = 0; w < DT_FIT_WAVES; ++w) v += part[w][tid];
        sums[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        // Cholesky G = L L^T of the leading K x K block, then L z = rhs, L^T c = z
        int fail = 0;
        for (int j = 0; j < K && !fail; ++j) {
            for (int i = j; i < K; ++i) {
                double v = sums[j * DT_K - j * (j - 1) / 2 + (i - j)];          // G[j][i], j <= i
                for (int p = 0; p < j; ++p) v -= L[i][p] * L[j][p];
                if (i == j) {
                    if (!(v > 0.0)) { fail = j + 1; break; }
                    L[j][j] = sqrt(v);
                } else {
                    L[i][j] = v / L[j][j];
                }
            }
        }
        if (!fail) {
            double z[DT_K];
            for (int i = 0; i < K; ++i) {
                double v = sums[DT_GRAM + i];
                for (int p = 0; p < i; ++p) v -= L[i][p] * z[p];
                z[i] = v / L[i][i];
            }
            for (int i = K - 1; i >= 0; --i) {
                double v = z[i];
                for (int p = i + 1; p < K; ++p) v -= L[p][i] * coef[p];
                coef[i] = v / L[i][i];
            }
        }
        for (int i = fail ? 0 : K; i < DT_K; ++i) coef[i] = 0.0;
        bad = fail;
        info[s] = fail;
    }
    __syncthreads();
    const int fail = bad;
    double c[DT_K];
#pragma unroll
    for (int a = 0; a < DT_K; ++a) c[a] = coef[a];
    for (int64_t i = tid; i < n; i += DT_FIT_THREADS) {
        if (fail) { out[b + i] = __longlong_as_double(0x7ff8000000000000ll); continue; }
        const double u = (half != 0.0) ? (t[b + i] - mid) / half : 0.0;
        double P[DT_K];
        legendre(u, P);
        double fit = 0.0;
#pragma unroll
        for (int a = 0; a < DT_K; ++a) fit += c[a] * P[a];
        out[b + i] = f[b + i] / fit;
    }
}

__global__ __launch_bounds__(DT_THREADS) void k_seg_ppm(const int64_t *__restrict__ off, const double *x,
                                                        const double *__restrict__ med, double *out) {   // (out may be x)
    const int s = blockIdx.x;
    const int64_t b = off[s], n = off[s + 1] - b;
    const double m = med[s];
    for (int64_t i = threadIdx.x; i < n; i += DT_THREADS) out[b + i] = 1e6 * (x[b + i] / m - 1.0);
}

int check_segments(const char *who, int S) {
    if (S < 1) return gf_internal_error(-1, "%s: no segments (S=%d)", who, S);
    return 0;
}

}  // namespace

extern "C" {

int gf_seg_median(int S, const int64_t *off, const double *x, const uint8_t *keep, int drop_last, double *med,
                  void *stream) {
    if (int st = check_segments("gf_seg_median", S)) return st;
    if (!off || !x || !med) return gf_internal_error(-1, "gf_seg_median: null pointer");
    if (drop_last < 0 || drop_last > 1)
        return gf_internal_error(-1, "gf_seg_median: drop_last=%d must be 0 or 1", drop_last);
    hipLaunchKernelGGL(k_seg_median, dim3(S), dim3(DT_THREADS), 0, (hipStream_t)stream, off, x, keep, drop_last, med);
    return check_launch("gf_seg_median");
}

int gf_sigma_clip(int S, const int64_t *off, const double *t, const double *f, double sigma_lower,
                  double sigma_upper, int maxiters, uint8_t *keep, int64_t *kept, int *rounds, void *stream) {
    if (int st = check_segments("gf_sigma_clip", S)) return st;
    if (!off || !f || !keep || !kept || !rounds) return gf_internal_error(-1, "gf_sigma_clip: null pointer");
    if (maxiters != 0 && !(sigma_lower > 0.0 && sigma_upper > 0.0))
        return gf_internal_error(-1, "gf_sigma_clip: sigma_lower=%g and sigma_upper=%g must be positive",
                                 sigma_lower, sigma_upper);
    hipLaunchKernelGGL(k_sigma_clip, dim3(S), dim3(DT_THREADS), 0, (hipStream_t)stream, off, t, f, sigma_lower,
                       sigma_upper, maxiters, keep, kept, rounds);
    return check_launch("gf_sigma_clip");
}

int gf_seg_compact(int S, const int64_t *off, const uint8_t *keep, const double *t, const double *f,
                   int64_t *new_off, double *t_out, double *f_out, void *stream) {
    if (int st = check_segments("gf_seg_compact", S)) return st;
    if (!off || !keep || !t || !f || !new_off || !t_out || !f_out)
        return gf_internal_error(-1, "gf_seg_compact: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_seg_count, dim3(S), dim3(DT_THREADS), 0, st, off, keep, new_off);
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(256), 0, st, S, new_off);
    hipLaunchKernelGGL(k_seg_compact, dim3(S), dim3(DT_THREADS), 0, st, off, keep, t, f, new_off, t_out, f_out);
    return check_launch("gf_seg_compact");
}

int gf_seg_diff(int S, const int64_t *off, const double *t, double *d, void *stream) {
    if (int st = check_segments("gf_seg_diff", S)) return st;
    if (!off || !t || !d) return gf_internal_error(-1, "gf_seg_diff: null pointer");
    hipLaunchKernelGGL(k_seg_diff, dim3(S), dim3(DT_THREADS), 0, (hipStream_t)stream, off, t, d);
    return check_launch("gf_seg_diff");
}

int gf_poly_normalise(int S, const int64_t *off, const double *t, const double *f, int order, double *normed,
                      int *info, void *stream) {
    if (int st = check_segments("gf_poly_normalise", S)) return st;
    if (order < 0 || order > GF_DETREND_MAX_ORDER)
        return gf_internal_error(-1, "gf_poly_normalise: order=%d must be in 0..%d", order, GF_DETREND_MAX_ORDER);
    if (!off || !t || !f || !normed || !info) return gf_internal_error(-1, "gf_poly_normalise: null pointer");
    hipLaunchKernelGGL(k_poly_normalise, dim3(S), dim3(DT_FIT_THREADS), 0, (hipStream_t)stream, off, t, f, order,
                       normed, info);
    return check_launch("gf_poly_normalise");
}

int gf_seg_ppm(int S, const int64_t *off, const double *x, const double *med, double *out, void *stream) {
    if (int st = check_segments("gf_seg_ppm", S)) return st;
    if (!off || !x || !med || !out) return gf_internal_error(-1, "gf_seg_ppm: null pointer");
    hipLaunchKernelGGL(k_seg_ppm, dim3(S), dim3(DT_THREADS), 0, (hipStream_t)stream, off, x, med, out);
    return check_launch("gf_seg_ppm");
}

}  // extern "C"
