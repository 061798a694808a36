// gadfly_ls.hip -- the exact floating-mean Lomb-Scargle periodogram ("psd" normalisation) of R gapped series
//
// Reference being replaced: PowerSpectrum._lomb_scargle (gadfly/psd.py:589-601), i.e. astropy's
// LombScargle(time, flux, normalization='psd').power(rfftfreq(n, d)) * d / sqrt(2 pi), defaults dy=None,
// fit_mean=True, center_data=True, nterms=1.  Per series (w = 1/n, y centred, t' = t - t_0):
//     C = sum w c, S = sum w s, CC = sum w c^2, CS = sum w c s, YC = sum w y c, YS = sum w y s, SS = 1 - CC
//     C^ = CC - C^2, S^ = SS - S^2, X^ = CS - C S,  lambda = C^ + S^,  det = C^ S^ - X^2
//     P = (n/2) (S^ YC^2 - 2 X^ YC YS + C^ YS^2) / det                              (general frequency)
//     P = (n/2) (u.v)^2 / lambda,  u the unit vector of the surviving column      (det <= GF_LS_RANK_TOL lambda^2)
//     P = 0                                                                        (lambda <= GF_LS_ZERO_TOL)
// power = P * norm.  Three kernels:
//   k_ls_prep   one workgroup per series: the mean of y - y_0 (fixed-shape reduction), and the per-point table
//               (t', y', cos 2 pi df t', sin 2 pi df t') with every phase reduced in cycles (p - rint(p))
//   k_ls_sum    (frequency tile, time segment, series): each thread owns K consecutive frequencies; per point one
//               exact sincos at its first frequency, then rotations by the point's (cos, sin) of 2 pi df t'; the
//               points are staged through LDS (a broadcast read); per-segment partial sums to the workspace
//   k_ls_finish the segments' partial sums in a fixed order, the degenerate-limit rule, the scaled power
// No floating-point atomics: every sum has one fixed association, whatever the batch around a series.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"

#define FM_INLINE static __device__ __forceinline__
#include "fastmath.h"

namespace {

constexpr int LS_K = 16;                    // frequencies per thread (k_ls_sum)
constexpr int LS_THREADS = 256;
constexpr int LS_TILE = LS_K * LS_THREADS;  // frequencies per workgroup
constexpr int LS_STAGE = LS_THREADS;        // points per LDS stage
constexpr int LS_PREP_THREADS = 1024;
constexpr int LS_MAX_SEGMENTS = 32;
constexpr int64_t LS_SEGMENT_POINTS = 8192; // a series gets ceil(n / 8192) segments, at most 32
constexpr double GF_LS_ZERO_TOL = 1e-10;    // lambda = C^ + S^ <= this (of its maximum 1): both columns constant
constexpr double GF_LS_RANK_TOL = 1e-10;    // det <= this * lambda^2: one column is a multiple of the other
constexpr double TWO_PI = 6.283185307179586;

__host__ __device__ inline int ls_segments(int64_t n) {
    const int64_t s = (n + LS_SEGMENT_POINTS - 1) / LS_SEGMENT_POINTS;
    return (int)(s < 1 ? 1 : s > LS_MAX_SEGMENTS ? LS_MAX_SEGMENTS : s);
}

__device__ inline void ls_sincos_cycles(double p, double *s, double *c) {
    const double frac = p - rint(p);        // exact: |frac| <= 1/2 cycle
    fm_sincos(TWO_PI * frac, s, c);
}

__global__ __launch_bounds__(LS_PREP_THREADS) void k_ls_prep(const int64_t *__restrict__ pt_off,
                                                             const double *__restrict__ df_,
                                                             const double *__restrict__ t,
                                                             const double *__restrict__ y,
                                                             double4 *__restrict__ tab) {
    __shared__ double red[LS_PREP_THREADS];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int64_t b = pt_off[r], n = pt_off[r + 1] - b;
    const double t0 = t[b], y0 = y[b], df = df_[r];
    // centred on the first value: a constant series is exactly zero after centring
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += LS_PREP_THREADS) acc += y[b + i] - y0;
    red[tid] = acc;
    __syncthreads();
    for (int h = LS_PREP_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double mean = red[0] / (double)n;
    for (int64_t i = tid; i < n; i += LS_PREP_THREADS) {
        const double tp = t[b + i] - t0;
        double sd, cd;
        ls_sincos_cycles(df * tp, &sd, &cd);
        tab[b + i] = make_double4(tp, (y[b + i] - y0) - mean, cd, sd);
    }
}

// part [LS_MAX_SEGMENTS... S_max][6][out_total]: C, S, CC, CS, YC, YS of segment s at output index o
template <int K>
__global__ __launch_bounds__(LS_THREADS) void k_ls_sum(const int64_t *__restrict__ pt_off,
                                                       const int64_t *__restrict__ out_off,
                                                       const double *__restrict__ df_, int first,
                                                       int64_t out_total, const double4 *__restrict__ tab,
                                                       double *__restrict__ part) {
    __shared__ double4 pts[LS_STAGE];
    const int r = blockIdx.z, seg = blockIdx.y, tid = threadIdx.x;
    const int64_t b = pt_off[r], n = pt_off[r + 1] - b, M = n / 2 + 1;
    const int S = ls_segments(n);
    const int64_t k_begin = first + (int64_t)blockIdx.x * (K * LS_THREADS);
    if (seg >= S || k_begin >= M) return;           // whole workgroup: the conditions hold per block
    const int64_t L = (n + S - 1) / S, i0 = seg * L, i1 = (i0 + L < n) ? i0 + L : n;
    const int64_t k0 = k_begin + (int64_t)tid * K;
    const double df = df_[r];
    const double f0 = (double)k0 * df;              // rfftfreq's value of frequency k0
    double aC[K], aS[K], aCC[K], aCS[K], aYC[K], aYS[K];
#pragma unroll
    for (int q = 0; q < K; ++q) aC[q] = aS[q] = aCC[q] = aCS[q] = aYC[q] = aYS[q] = 0.0;
    for (int64_t base = i0; base < i1; base += LS_STAGE) {
        const int cnt = (int)((i1 - base < LS_STAGE) ? i1 - base : LS_STAGE);
        __syncthreads();
        if (tid < cnt) pts[tid] = tab[b + base + tid];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double4 p = pts[j];
            double s, c;
            ls_sincos_cycles(f0 * p.x, &s, &c);
#pragma unroll
            for (int q = 0; q < K; ++q) {
                aC[q] += c;
                aS[q] += s;
                aCC[q] = fma(c, c, aCC[q]);
                aCS[q] = fma(c, s, aCS[q]);
                aYC[q] = fma(p.y, c, aYC[q]);
                aYS[q] = fma(p.y, s, aYS[q]);
                if (q + 1 < K) {                    // to frequency k0 + q + 1: rotate by 2 pi df t'
                    const double cn = fma(c, p.z, -s * p.w);
                    s = fma(s, p.z, c * p.w);
                    c = cn;
                }
            }
        }
    }
    const int64_t ob = out_off[r] - first;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        if (k0 + q >= M) break;
        double *o = part + ((int64_t)seg * 6) * out_total + ob + k0 + q;
        o[0] = aC[q];
        o[out_total] = aS[q];
        o[2 * out_total] = aCC[q];
        o[3 * out_total] = aCS[q];
        o[4 * out_total] = aYC[q];
        o[5 * out_total] = aYS[q];
    }
}

__global__ __launch_bounds__(256) void k_ls_finish(const int64_t *__restrict__ pt_off,
                                                   const int64_t *__restrict__ out_off,
                                                   const double *__restrict__ norm_, int first,
                                                   int64_t out_total, const double *__restrict__ part,
                                                   double *__restrict__ power) {
    const int r = blockIdx.y;
    const int64_t n = pt_off[r + 1] - pt_off[r], M = n / 2 + 1;
    const int S = ls_segments(n);
    const int64_t ob = out_off[r], cnt = M - first;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * 256) {
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int q = 0; q < 6; ++q) v[q] += part[((int64_t)s * 6 + q) * out_total + ob + i];
        const double w = 1.0 / (double)n;
        const double C = v[0] * w, Sn = v[1] * w, CC = v[2] * w, CS = v[3] * w, YC = v[4] * w, YS = v[5] * w;
        const double SS = 1.0 - CC;
        const double Ch = CC - C * C, Sh = SS - Sn * Sn, Xh = CS - C * Sn;
        const double lam = Ch + Sh, det = Ch * Sh - Xh * Xh;
        double P;
        if (!(lam > GF_LS_ZERO_TOL)) {
            P = 0.0;
        } else if (!(det > GF_LS_RANK_TOL * lam * lam)) {
            const double u0 = (Ch >= Sh) ? Ch : Xh, u1 = (Ch >= Sh) ? Xh : Sh;
            const double uv = u0 * YC + u1 * YS;
            P = 0.5 * (double)n * (uv * uv / (u0 * u0 + u1 * u1)) / lam;
        } else {
            P = 0.5 * (double)n * (Sh * YC * YC - 2.0 * Xh * YC * YS + Ch * YS * YS) / det;
        }
        power[ob + i] = P * norm_[r];
    }
}

}  // namespace

extern "C" {

int gf_ls_segments(int64_t n) { return n < 2 ? -1 : ls_segments(n); }

int64_t gf_ls_work(int64_t n_total, int64_t out_total, int S_max) {
    if (n_total < 2 || out_total < 1 || S_max < 1 || S_max > LS_MAX_SEGMENTS) return 0;
    return 4 * n_total + 6 * (int64_t)S_max * out_total;
}

int gf_ls_power(int R, int64_t n_max, int64_t n_total, int64_t out_total, int S_max, int first,
                const int64_t *pt_off, const int64_t *out_off, const double *df, const double *norm,
                const double *t, const double *y, double *work, double *power, void *stream) {
    if (R < 1 || n_max < 2 || n_total < 2 || out_total < 1 || first < 0 || first > 1)
        return gf_internal_error(-1, "gf_ls_power: bad shape (R=%d, n_max=%lld, n_total=%lld, out_total=%lld, first=%d)",
                                 R, (long long)n_max, (long long)n_total, (long long)out_total, first);
    if (R > 65535) return gf_internal_error(-1, "gf_ls_power: more than 65535 series (R=%d)", R);
    if (S_max < ls_segments(n_max) || S_max > LS_MAX_SEGMENTS)
        return gf_internal_error(-1, "gf_ls_power: S_max=%d does not cover n_max=%lld (needs %d, at most %d)",
                                 S_max, (long long)n_max, ls_segments(n_max), LS_MAX_SEGMENTS);
    if (!pt_off || !out_off || !df || !norm || !t || !y || !work || !power)
        return gf_internal_error(-1, "gf_ls_power: null pointer");
    hipStream_t st = (hipStream_t)stream;
    double4 *tab = reinterpret_cast<double4 *>(work);
    double *part = work + 4 * n_total;
    if (reinterpret_cast<uintptr_t>(work) & 31)
        return gf_internal_error(-1, "gf_ls_power: the workspace must be 32-byte aligned");
    hipLaunchKernelGGL(k_ls_prep, dim3(R), dim3(LS_PREP_THREADS), 0, st, pt_off, df, t, y, tab);
    const int64_t tiles = (n_max / 2 + 1 + LS_TILE - 1) / LS_TILE;
    hipLaunchKernelGGL(k_ls_sum<LS_K>, dim3((unsigned)tiles, S_max, R), dim3(LS_THREADS), 0, st, pt_off, out_off, df,
                       first, out_total, (const double4 *)tab, part);
    int64_t blocks = (n_max / 2 + 1 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_ls_finish, dim3((unsigned)blocks, R), dim3(256), 0, st, pt_off, out_off, norm, first,
                       out_total, (const double *)part, power);
    return gf_internal_check_launch("gf_ls_power");
}

}  // extern "C"
