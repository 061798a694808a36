// gadfly_lsfft.hip -- the floating-mean Lomb-Scargle periodogram of R gapped series through a non-uniform FFT
//
// Reference being replaced: PowerSpectrum._lomb_scargle (gadfly/psd.py:589-601), as gadfly_ls.hip does by the
// exact direct sum (n^2 / 2 pair evaluations); this unit reaches the same seven sums in O(n log n).
// With w = 1/n, y' centred, t' = t - t_0 and x = frac(t' df) (df = 1/(n d): every exponential has period n d in t'),
//     F_1(k) = sum_j e^{2 pi i k x_j}  (k = 0 ... 2 [n/2]),     F_y(k) = sum_j y'_j e^{2 pi i k x_j}  (k = 0 ... [n/2])
//     C, S = Re, Im F_1(k)/n;  CC = (1 + Re F_1(2k)/n)/2;  CS = Im F_1(2k)/(2n);  SS = 1 - CC;  YC, YS = Re, Im F_y(k)/n
// and the power follows as in k_ls_finish (same formula, same degenerate limits).  F_1 and F_y are type-1
// non-uniform transforms with real strengths: spread onto a fine grid of n_f cells with
//     phi(z) = exp(beta (sqrt(1 - z^2) - 1)),  z = (cell - x n_f) / (w/2),  w = 16,  beta = 2.30 w
// over the 16 cells floor(x n_f) - 7 ... floor(x n_f) + 8 (wrapping round the ends), F(k) = conj(rfft(grid))[k]
// (hipFFT, by the caller), divided by phi^(k) = w int_0^1 phi(z) cos(pi w k z / n_f) dz (64 Gauss-Legendre nodes).
// Series that share a time axis share its wrap, its sort and its grid of ones (`axis`).  Kernels:
//   k_lsfft_wrap    per axis: u = frac(t' df) n_f and the sort key (first cell of the axis' grid + floor(u))
//   k_lsfft_sum     per series: the sums of y - y_0 over min(64, ceil(n / 16384)) segments (a function of n alone)
//   k_lsfft_center  y' = (y - y_0) - mean (centred on the first value, then the mean, as k_ls_prep does)
//   (the caller sorts the keys: a stable integer sort)
//   k_lsfft_starts  per-cell start offsets into the sorted points (a binary search per cell)
//   k_lsfft_spread  one thread per fine-grid cell gathers the points of the 16 cells of its window in sorted order
//   (the caller transforms the grids)
//   k_lsfft_finish  deconvolution, the seven sums, the degenerate-limit rule, the scaled power
// No floating-point atomics: a cell's sum runs over the sorted points in one fixed order.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"

namespace {

constexpr int LSFFT_W = 16;                     // kernel width in fine-grid cells (fixed: DESIGN.md 3.6)
constexpr int LSFFT_HALF = LSFFT_W / 2;
constexpr int LSFFT_SIGMA = 2;                  // oversampling
constexpr double LSFFT_BETA = 2.30 * LSFFT_W;
constexpr int LSFFT_QUAD = 64;                  // Gauss-Legendre nodes on [0, 1]
constexpr int LSFFT_THREADS = 256;
constexpr int LSFFT_MAX_SEGMENTS = 64;          // partial sums of the mean per series
constexpr int64_t LSFFT_SEGMENT_POINTS = 16384;
constexpr double LSFFT_ZERO_TOL = 1e-10;        // as gadfly_ls.hip: lambda = C^ + S^ <= this
constexpr double LSFFT_RANK_TOL = 1e-10;        // det <= this * lambda^2
constexpr double PI = 3.141592653589793;

__host__ __device__ inline int64_t lsfft_grid(int64_t n) {
    int64_t m = 2 * (2 * (n / 2) + 1) * LSFFT_SIGMA + 2 * LSFFT_W;
    for (;; ++m) {
        int64_t r = m;
        while (r % 2 == 0) r /= 2;
        while (r % 3 == 0) r /= 3;
        while (r % 5 == 0) r /= 5;
        if (r == 1) return m;
    }
}

__host__ __device__ inline int lsfft_segments(int64_t n) {
    const int64_t s = (n + LSFFT_SEGMENT_POINTS - 1) / LSFFT_SEGMENT_POINTS;
    return (int)(s < 1 ? 1 : s > LSFFT_MAX_SEGMENTS ? LSFFT_MAX_SEGMENTS : s);
}

__device__ inline double lsfft_phi(double z) {
    const double s = fma(-z, z, 1.0);
    return exp(LSFFT_BETA * (sqrt(s > 0.0 ? s : 0.0) - 1.0));
}

__global__ __launch_bounds__(LSFFT_THREADS) void k_lsfft_wrap(const int64_t *__restrict__ ax_off,
                                                              const int64_t *__restrict__ cell_off,
                                                              const double *__restrict__ df_,
                                                              const double *__restrict__ t,
                                                              int64_t *__restrict__ key, double *__restrict__ u) {
    const int a = blockIdx.y;
    const int64_t b = ax_off[a], n = ax_off[a + 1] - b;
    const int64_t c0 = cell_off[a], nf = cell_off[a + 1] - c0;
    const double t0 = t[b], df = df_[a];
    for (int64_t i = (int64_t)blockIdx.x * LSFFT_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * LSFFT_THREADS) {
        const double q = (t[b + i] - t0) * df;  // cycles of the grid's period, rounded once
        double x = q - floor(q);                // exact for q >= 0
        if (x >= 1.0) x -= 1.0;                 // (a tiny negative q)
        const double uu = x * (double)nf;
        int64_t m = (int64_t)uu;
        if (m > nf - 1) m = nf - 1;             // x n_f rounded up to n_f: the last cell, u = n_f
        if (m < 0) m = 0;                       // (a non-finite time: the key stays a cell of this grid)
        key[b + i] = c0 + m;
        u[b + i] = uu;
    }
}

// sums of y - y_0 over the S = lsfft_segments(n) equal segments of a series (S depends on n alone): part[r][s]
__global__ __launch_bounds__(LSFFT_THREADS) void k_lsfft_sum(const int64_t *__restrict__ pt_off,
                                                             const double *__restrict__ y,
                                                             double *__restrict__ part) {
    __shared__ double red[LSFFT_THREADS];
    const int r = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
    const int64_t b = pt_off[r], n = pt_off[r + 1] - b;
    const int S = lsfft_segments(n);
    if (seg >= S) return;                       // whole workgroup
    const int64_t L = (n + S - 1) / S, i0 = seg * L, i1 = (i0 + L < n) ? i0 + L : n;
    const double y0 = y[b];
    // centred on the first value: a constant series is exactly zero after centring
    double acc = 0.0;
    for (int64_t i = i0 + tid; i < i1; i += LSFFT_THREADS) acc += y[b + i] - y0;
    red[tid] = acc;
    __syncthreads();
    for (int h = LSFFT_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) part[(int64_t)r * LSFFT_MAX_SEGMENTS + seg] = red[0];
}

// y' = (y - y_0) - mean, the mean from the segments' sums in order
__global__ __launch_bounds__(LSFFT_THREADS) void k_lsfft_center(const int64_t *__restrict__ pt_off,
                                                                const double *__restrict__ y,
                                                                const double *__restrict__ part,
                                                                double *__restrict__ yc) {
    const int r = blockIdx.y;
    const int64_t b = pt_off[r], n = pt_off[r + 1] - b;
    const int S = lsfft_segments(n);
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += part[(int64_t)r * LSFFT_MAX_SEGMENTS + s];
    const double mean = sum / (double)n, y0 = y[b];
    for (int64_t i = (int64_t)blockIdx.x * LSFFT_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * LSFFT_THREADS)
        yc[b + i] = (y[b + i] - y0) - mean;
}

// start[c] = number of sorted keys < c, c = 0 ... cells: a binary search per cell (neighbouring cells read the
// same keys); whatever the keys hold, every start lies in [0, n]
__global__ __launch_bounds__(LSFFT_THREADS) void k_lsfft_starts(int64_t n, int64_t cells,
                                                                const int64_t *__restrict__ skey,
                                                                int64_t *__restrict__ start) {
    const int64_t c = (int64_t)blockIdx.x * LSFFT_THREADS + threadIdx.x;
    if (c > cells) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (skey[mid] < c) lo = mid + 1; else hi = mid;
    }
    start[c] = lo;
}

struct SpreadSums {
    double y, one;
};

// the sorted points i0 <= i < i1, seen from cell position cc (the cell, shifted by +-n_f across the wrap)
__device__ inline void lsfft_gather(int64_t i0, int64_t i1, double cc, const int64_t *__restrict__ perm,
                                    const double *__restrict__ u, const double *__restrict__ yc, int64_t yo,
                                    SpreadSums &acc) {
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t p = perm[i];
        const double ph = lsfft_phi((cc - u[p]) * (1.0 / LSFFT_HALF));
        acc.one += ph;
        acc.y = fma(ph, yc[yo + p], acc.y);
    }
}

__global__ __launch_bounds__(LSFFT_THREADS) void k_lsfft_spread(const int64_t *__restrict__ ax_off,
                                                                const int64_t *__restrict__ cell_off,
                                                                const int64_t *__restrict__ pt_off,
                                                                const int64_t *__restrict__ axis,
                                                                const int64_t *__restrict__ gy_off,
                                                                const int64_t *__restrict__ g1_off,
                                                                const int64_t *__restrict__ start,
                                                                const int64_t *__restrict__ perm,
                                                                const double *__restrict__ u,
                                                                const double *__restrict__ yc,
                                                                double *__restrict__ grid) {
    const int r = blockIdx.y;
    const int64_t a = axis[r];
    const int64_t base = cell_off[a], nf = cell_off[a + 1] - base;
    const int64_t c = (int64_t)blockIdx.x * LSFFT_THREADS + threadIdx.x;
    if (c >= nf) return;
    // point p of the axis (an index into the concatenated axes) is point p - ax_off[a] of series r
    const int64_t yo = pt_off[r] - ax_off[a];
    const int64_t *st = start + base;
    // cell c receives the points whose own cell m has m - 7 <= c <= m + 8: the 16 cells c - 8 ... c + 7
    const int64_t lo = c - LSFFT_HALF, hi = c + LSFFT_HALF;
    SpreadSums acc = {0.0, 0.0};
    if (lo < 0) lsfft_gather(st[lo + nf], st[nf], (double)(c + nf), perm, u, yc, yo, acc);
    lsfft_gather(st[lo < 0 ? 0 : lo], st[hi > nf ? nf : hi], (double)c, perm, u, yc, yo, acc);
    if (hi > nf) lsfft_gather(st[0], st[hi - nf], (double)(c - nf), perm, u, yc, yo, acc);
    grid[gy_off[r] + c] = acc.y;
    if (g1_off[r] >= 0) grid[g1_off[r] + c] = acc.one;
}

__device__ inline double lsfft_phi_hat(double ak, const double *qz, const double *qa) {
    double s = 0.0;
#pragma unroll 8
    for (int q = 0; q < LSFFT_QUAD; ++q) s = fma(qa[q], cos(ak * qz[q]), s);
    return s;
}

__global__ __launch_bounds__(LSFFT_THREADS) void k_lsfft_finish(const int64_t *__restrict__ pt_off,
                                                                const int64_t *__restrict__ out_off,
                                                                const int64_t *__restrict__ axis,
                                                                const int64_t *__restrict__ cell_off,
                                                                const int64_t *__restrict__ sy_off,
                                                                const int64_t *__restrict__ s1_off,
                                                                const double *__restrict__ norm_,
                                                                const double *__restrict__ quad, int first,
                                                                const double2 *__restrict__ spec,
                                                                double *__restrict__ power) {
    __shared__ double qz[LSFFT_QUAD], qa[LSFFT_QUAD];
    const int r = blockIdx.y;
    if (threadIdx.x < LSFFT_QUAD) {             // node z_q and w * weight_q * phi(z_q)
        const double z = quad[threadIdx.x];
        qz[threadIdx.x] = z;
        qa[threadIdx.x] = (double)LSFFT_W * quad[LSFFT_QUAD + threadIdx.x] * lsfft_phi(z);
    }
    __syncthreads();
    const int64_t n = pt_off[r + 1] - pt_off[r], M = n / 2 + 1;
    const int64_t a = axis[r], nf = cell_off[a + 1] - cell_off[a];
    const double alpha = PI * LSFFT_W / (double)nf;
    const double2 *sy = spec + sy_off[r], *s1 = spec + s1_off[r];
    const int64_t ob = out_off[r], cnt = M - first;
    const double w = 1.0 / (double)n;
    for (int64_t i = (int64_t)blockIdx.x * LSFFT_THREADS + threadIdx.x; i < cnt;
         i += (int64_t)gridDim.x * LSFFT_THREADS) {
        const int64_t k = first + i;
        const double h1 = w / lsfft_phi_hat(alpha * (double)k, qz, qa);
        const double h2 = w / lsfft_phi_hat(alpha * (double)(2 * k), qz, qa);
        const double2 g1 = s1[k], g2 = s1[2 * k], gy = sy[k];      // F = conj(rfft)
        const double C = g1.x * h1, Sn = -g1.y * h1;
        const double CC = 0.5 * (1.0 + g2.x * h2), CS = -0.5 * g2.y * h2;
        const double YC = gy.x * h1, YS = -gy.y * h1;
        const double SS = 1.0 - CC;
        const double Ch = CC - C * C, Sh = SS - Sn * Sn, Xh = CS - C * Sn;
        const double lam = Ch + Sh, det = Ch * Sh - Xh * Xh;
        double P;
        if (!(lam > LSFFT_ZERO_TOL)) {
            P = 0.0;
        } else if (!(det > LSFFT_RANK_TOL * lam * lam)) {
            const double u0 = (Ch >= Sh) ? Ch : Xh, u1 = (Ch >= Sh) ? Xh : Sh;
            const double uv = u0 * YC + u1 * YS;
            P = 0.5 * (double)n * (uv * uv / (u0 * u0 + u1 * u1)) / lam;
        } else {
            P = 0.5 * (double)n * (Sh * YC * YC - 2.0 * Xh * YC * YS + Ch * YS * YS) / det;
        }
        power[ob + i] = P * norm_[r];
    }
}

bool lsfft_bad_counts(int A, int R) { return A < 1 || R < 1 || A > 65535 || R > 65535 || A > R; }

}  // namespace

extern "C" {

int64_t gf_lsfft_grid(int64_t n) { return n < 2 ? -1 : lsfft_grid(n); }

int64_t gf_lsfft_part(int R) { return R < 1 ? 0 : (int64_t)R * LSFFT_MAX_SEGMENTS; }

int gf_lsfft_prepare(int A, int R, int64_t n_max, const int64_t *ax_off, const int64_t *cell_off, const double *df,
                     const int64_t *pt_off, const double *t, const double *y, int64_t *key, double *u, double *yc,
                     double *part, void *stream) {
    if (lsfft_bad_counts(A, R) || n_max < 2)
        return gf_internal_error(-1, "gf_lsfft_prepare: bad shape (A=%d, R=%d, n_max=%lld; 1 <= A <= R <= 65535)", A, R,
                                 (long long)n_max);
    if (!ax_off || !cell_off || !df || !pt_off || !t || !y || !key || !u || !yc || !part)
        return gf_internal_error(-1, "gf_lsfft_prepare: null pointer");
    hipStream_t st = (hipStream_t)stream;
    int64_t blocks = (n_max + LSFFT_THREADS - 1) / LSFFT_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_lsfft_wrap, dim3((unsigned)blocks, A), dim3(LSFFT_THREADS), 0, st, ax_off, cell_off, df, t,
                       key, u);
    hipLaunchKernelGGL(k_lsfft_sum, dim3(lsfft_segments(n_max), R), dim3(LSFFT_THREADS), 0, st, pt_off, y, part);
    hipLaunchKernelGGL(k_lsfft_center, dim3((unsigned)blocks, R), dim3(LSFFT_THREADS), 0, st, pt_off, y,
                       (const double *)part, yc);
    return gf_internal_check_launch("gf_lsfft_prepare");
}

int gf_lsfft_spread(int A, int R, int64_t n_axes, int64_t cells, int64_t nf_max, const int64_t *ax_off,
                    const int64_t *cell_off, const int64_t *pt_off, const int64_t *axis, const int64_t *gy_off,
                    const int64_t *g1_off, const int64_t *skey, const int64_t *perm, const double *u, const double *yc,
                    int64_t *start, double *grid, void *stream) {
    if (lsfft_bad_counts(A, R) || n_axes < 2 || nf_max < lsfft_grid(2) || cells < nf_max ||
        nf_max > ((int64_t)1 << 38))
        return gf_internal_error(-1, "gf_lsfft_spread: bad shape (A=%d, R=%d, n_axes=%lld, cells=%lld, nf_max=%lld)", A, R,
                                 (long long)n_axes, (long long)cells, (long long)nf_max);
    if (!ax_off || !cell_off || !pt_off || !axis || !gy_off || !g1_off || !skey || !perm || !u || !yc || !start || !grid)
        return gf_internal_error(-1, "gf_lsfft_spread: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t sb = (cells + 1 + LSFFT_THREADS - 1) / LSFFT_THREADS;
    if (sb > 0x7fffffff) return gf_internal_error(-1, "gf_lsfft_spread: too many cells (%lld)", (long long)cells);
    hipLaunchKernelGGL(k_lsfft_starts, dim3((unsigned)sb), dim3(LSFFT_THREADS), 0, st, n_axes, cells, skey, start);
    const int64_t blocks = (nf_max + LSFFT_THREADS - 1) / LSFFT_THREADS;
    hipLaunchKernelGGL(k_lsfft_spread, dim3((unsigned)blocks, R), dim3(LSFFT_THREADS), 0, st, ax_off, cell_off, pt_off,
                       axis, gy_off, g1_off, (const int64_t *)start, perm, u, yc, grid);
    return gf_internal_check_launch("gf_lsfft_spread");
}

int gf_lsfft_finish(int R, int64_t n_max, int first, const int64_t *pt_off, const int64_t *out_off, const int64_t *axis,
                    const int64_t *cell_off, const int64_t *sy_off, const int64_t *s1_off, const double *norm,
                    const double *quad, const double *spec, double *power, void *stream) {
    if (R < 1 || R > 65535 || n_max < 2 || first < 0 || first > 1)
        return gf_internal_error(-1, "gf_lsfft_finish: bad shape (R=%d, n_max=%lld, first=%d)", R, (long long)n_max, first);
    if (!pt_off || !out_off || !axis || !cell_off || !sy_off || !s1_off || !norm || !quad || !spec || !power)
        return gf_internal_error(-1, "gf_lsfft_finish: null pointer");
    if (reinterpret_cast<uintptr_t>(spec) & 15)
        return gf_internal_error(-1, "gf_lsfft_finish: the transforms must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int64_t blocks = (n_max / 2 + 1 + LSFFT_THREADS - 1) / LSFFT_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_lsfft_finish, dim3((unsigned)blocks, R), dim3(LSFFT_THREADS), 0, st, pt_off, out_off, axis,
                       cell_off, sy_off, s1_off, norm, quad, first, reinterpret_cast<const double2 *>(spec), power);
    return gf_internal_check_launch("gf_lsfft_finish");
}

}  // extern "C"
