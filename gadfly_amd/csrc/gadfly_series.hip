// gadfly_series.hip -- light-curve preparation around the Gaussian process: power spectra and gap filling
//
// What is replaced: what the reference does in numpy / scipy around its FFT (PowerSpectrum._fft and the binning of
// gadfly/psd.py, scipy.stats.binned_statistic) and its interpolation of missing cadences (gadfly/interp.py).  The
// transform itself is hipFFT's.
//   k_psd_power, k_psd_bin     |X|^2 * norm of a spectrum, and its means and errors over frequency bins
//   k_interp_*                 a plan (count, scan, offsets) and a fill (points, missing) of the cadences a series lacks
//   k_interp_*_seg             the same plan and fill for many series at once, over one offset table

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"

namespace {

// ------------------------------------------------------------------------------------
// Power spectra of light curves / prior draws and their binning: the step
// after `sample` in the reference's own hot-path test (gadfly/tests/test_core.py:29-34).  The
// transform itself is hipFFT's (a plain library FFT); these two kernels are what the reference
// does around it in numpy / scipy.binned_statistic.
// ------------------------------------------------------------------------------------
// power[r][k] = |X[r][first + k]|^2 * norm      (PowerSpectrum._fft, psd.py:566-587)
// X interleaved complex [R][M]; re*re + im*im without contraction, as numpy forms it.
__global__ void __launch_bounds__(256)
k_psd_power(const int64_t M, const int64_t Mout, const int64_t first, const double norm,
            const double2 *__restrict__ spec, double *__restrict__ power) {
#pragma clang fp contract(off)      // plain operators under this pragma: HIP's __dmul_rn / __dadd_rn wrappers still contract
    const size_t r = blockIdx.y;
    const double2 *X = spec + r * (size_t)M + first;
    double *P = power + r * (size_t)Mout;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < Mout; k += (int64_t)gridDim.x * 256) {
        const double2 v = X[k];
        P[k] = (v.x * v.x + v.y * v.y) * norm;
    }
}

// sum over the 256 threads of a workgroup, result in every thread (fixed shape: deterministic)
__device__ __forceinline__ double wg_sum256(double v, double *red) {
    v = wave_sum(v);
    __syncthreads();                                // red may still be read from the last call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per (bin, series): the bin's points are the contiguous range [start[b], start[b+1])
// of the ascending frequency axis x.  bin_power_spectrum's two statistics (psd.py:186-227):
//   stat = trapz(y, x) / (x_last - x_first)                          (one point: y itself)
//   err  = std(y) / sqrt(n) * mean(x) / (x_last - x_first) / constant (one point: y itself)
// and NaN for an empty bin (scipy.stats.binned_statistic's value for a failing statistic).
__global__ void __launch_bounds__(256)
k_psd_bin(const int64_t M, const int nb, const double *__restrict__ x,
          const double *__restrict__ power, const int64_t *__restrict__ start,
          const double constant, double *__restrict__ stat, double *__restrict__ err) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const size_t r = blockIdx.y;
    const int64_t s = start[b], e = start[b + 1], n = e - s;
    const double *y = power + r * (size_t)M;
    double *st = stat + r * (size_t)nb + b, *er = err + r * (size_t)nb + b;
    if (n <= 0) {
        if (threadIdx.x == 0) { *st = __builtin_nan(""); *er = __builtin_nan(""); }
        return;
    }
    const double span = x[e - 1] - x[s];
    if (n == 1 || !(span > 0.0)) {
        if (threadIdx.x == 0) { *st = y[s]; *er = y[s]; }
        return;
    }
    double tz = 0.0, sy = 0.0, sx = 0.0;
    for (int64_t i = s + threadIdx.x; i < e; i += 256) {
        const double yi = y[i], xi = x[i];
        sy += yi;
        sx += xi;
        if (i + 1 < e) tz += (x[i + 1] - xi) * (yi + y[i + 1]) * 0.5;
    }
    tz = wg_sum256(tz, red);
    sy = wg_sum256(sy, red);
    sx = wg_sum256(sx, red);
    const double mean = sy / (double)n;
    double ss = 0.0;
    for (int64_t i = s + threadIdx.x; i < e; i += 256) {
        const double dv = y[i] - mean;
        ss = fma(dv, dv, ss);
    }
    ss = wg_sum256(ss, red);
    if (threadIdx.x == 0) {
        *st = tz / span;
        *er = sqrt(ss / (double)n) / sqrt((double)n) * (sx / (double)n) / span / constant;
    }
}

// ------------------------------------------------------------------------------------
// Light-curve ingestion: fill the missing cadences of an otherwise evenly
// sampled series by linear interpolation -- interpolate_missing_data (gadfly/interp.py:6-60), what
// the reference runs before every FFT power spectrum (psd.py:495, :531).  Times ascending.
//   cadence index c_i = rint((t_i - t_0) / dt)  (or the given cadence numbers, minus the first);
//   after point i the indices c_i + 1 .. c_{i+1} - 1 are missing: grid time x = t_0 + index * dt,
//   flux np.interp(x, t, f) = slope * (x - t_j) + f_j on the interval that holds x,
// each product and sum rounded on its own, as numpy forms them (bit-identical results).
// Steps: counts (1 + gap) per point, an exclusive scan, then the merge by time (below).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t cadence_index(const double *t, const int64_t *cad, int64_t i,
                                                 double t0, double dt) {
#pragma clang fp contract(off)
    return cad ? (cad[i] - cad[0]) : (int64_t)rint((t[i] - t0) / dt);
}

constexpr int SCAN_PER_WG = 2048;       // elements per 256-thread workgroup (8 per thread)

// 1 + number of cadences missing after point i of a series of N points (its last point: 1)
__device__ __forceinline__ int64_t interp_count(const int64_t N, const double *t, const int64_t *cad,
                                                const double t0, const double dt, const int64_t i) {
    if (i + 1 >= N) return 1;
    const int64_t gap = cadence_index(t, cad, i + 1, t0, dt) - cadence_index(t, cad, i, t0, dt) - 1;
    return gap > 0 ? 1 + gap : 1;
}

// The scan of one workgroup's SCAN_PER_WG counts: thread x holds 8 neighbours, loc[k] = sum of its counts before the
// k-th and run = their sum; -> the sum over the threads before x (the workgroup's total: part[255])
__device__ __forceinline__ int64_t interp_scan_wg(int64_t *part, const int64_t run) {
    part[threadIdx.x] = run;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {           // Hillis-Steele inclusive scan of the 256 partials
        const int64_t v = (threadIdx.x >= (unsigned)off) ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    return part[threadIdx.x] - run;
}

// counts[i] = 1 + number of cadences missing after point i; block_sums[wg] = sum over the workgroup's
// SCAN_PER_WG elements; offsets[i] = exclusive scan of counts WITHIN the workgroup
__global__ void __launch_bounds__(256)
k_interp_count(const int64_t N, const double *__restrict__ t, const int64_t *__restrict__ cad,
               const double t0, const double dt, int64_t *__restrict__ offsets,
               int64_t *__restrict__ block_sums) {
    __shared__ int64_t part[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_WG + (int64_t)threadIdx.x * 8;
    int64_t loc[8], run = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t i = base + k;
        const int64_t cnt = (i < N) ? interp_count(N, t, cad, t0, dt, i) : 0;
        loc[k] = run;
        run += cnt;
    }
    const int64_t before = interp_scan_wg(part, run);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (base + k < N) offsets[base + k] = before + loc[k];
    if (threadIdx.x == 255) block_sums[blockIdx.x] = part[255];
}

// exclusive scan of the block sums in place (one workgroup, any count); total -> offsets[N]
__global__ void __launch_bounds__(256)
k_interp_scan_top(const int64_t nblocks, const int64_t N, int64_t *__restrict__ block_sums,
                  int64_t *__restrict__ offsets) {
    __shared__ int64_t part[256];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nblocks; b0 += 256) {
        const int64_t i = b0 + threadIdx.x;
        const int64_t v = (i < nblocks) ? block_sums[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int64_t u = (threadIdx.x >= (unsigned)off) ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += u;
            __syncthreads();
        }
        if (i < nblocks) block_sums[i] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[N] = carry;
}

__global__ void __launch_bounds__(256)
k_interp_offsets(const int64_t N, const int64_t *__restrict__ block_sums, int64_t *__restrict__ offsets) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) offsets[i] += block_sums[i / SCAN_PER_WG];
}

// The filled series is the reference's merge BY TIME of the input points and the missing cadences'
// grid times t_0 + m dt (interp.py:56-59).  With cadence numbers given, dt is a median and the grid
// drifts against the (e.g. barycentric) time stamps, so a missing cadence's grid time need not lie
// between its neighbours' time stamps: positions come from ranks, not from the gap a cadence sits in.
//   input point i   -> i + #{missing m : x_m <  t_i}
//   missing cadence -> (its rank among the missing) + #{i : t_i <= x_m}      (ties: input points first)
__device__ __forceinline__ double grid_time(const double t0, const int64_t m, const double dt) {
#pragma clang fp contract(off)
    return t0 + (double)m * dt;
}

// The two fill rules for point i of ONE series of N points (t, f, cad start at its first point; t0 = t[0]).
// offs[j] - obase = j + (number of cadences missing before point j), j = 0 .. N: the series' own scan (obase = 0)
// or its stretch of a scan over many series, obase = offs[0].  t_out, f_out start at the series' first output.
// G[i] = offs[i] - obase - i = number of missing cadences before point i's gap
__device__ __forceinline__ void interp_point(const int64_t N, const double *__restrict__ t,
                                             const double *__restrict__ f, const int64_t *__restrict__ cad,
                                             const double t0, const double dt, const int64_t *__restrict__ offs,
                                             const int64_t obase, const int64_t i, double *__restrict__ t_out,
                                             double *__restrict__ f_out) {
    const double ti = t[i];
    // M = smallest cadence index whose grid time is >= t_i (monotone in m: settle it exactly)
    int64_t M = (int64_t)floor((ti - t0) / dt) - 1;
    while (grid_time(t0, M, dt) >= ti) --M;
    while (grid_time(t0, M, dt) < ti) ++M;
    // j = last input point with cadence index < M; missing below M = G[j] + those of j's gap below M
    int64_t lo = 0, hi = N;                         // first point with index >= M
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cadence_index(t, cad, mid, t0, dt) < M) lo = mid + 1; else hi = mid;
    }
    int64_t before = 0;
    if (lo > 0) {
        const int64_t j = lo - 1;
        const int64_t gap = offs[j + 1] - offs[j] - 1;
        int64_t part = M - cadence_index(t, cad, j, t0, dt) - 1;
        part = part < 0 ? 0 : (part > gap ? gap : part);
        before = (offs[j] - obase - j) + part;
    }
    t_out[i + before] = ti;
    f_out[i + before] = f[i];
}

// the cadences missing after point i (one thread fills the whole gap)
__device__ __forceinline__ void interp_missing(const int64_t N, const double *__restrict__ t,
                                               const double *__restrict__ f, const int64_t *__restrict__ cad,
                                               const double t0, const double dt, const int64_t G, const int64_t gap,
                                               const int64_t i, double *__restrict__ t_out,
                                               double *__restrict__ f_out) {
#pragma clang fp contract(off)      // numpy rounds the product and the sum separately (no FMA)
    const int64_t ci = cadence_index(t, cad, i, t0, dt);
    int64_t p = i + 1;                              // #{points with t <= x}: grows with k, starts near i
    for (int64_t k = 1; k <= gap; ++k) {
        const double x = grid_time(t0, ci + k, dt);
        if (p > 0 && t[p - 1] > x) {                // the grid has drifted back past point p-1: search below
            int64_t lo = 0, hi = p - 1;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (t[mid] <= x) lo = mid + 1; else hi = mid; }
            p = lo;
        }
        while (p < N && t[p] <= x) ++p;
        // np.interp: clamped outside the series, the sample itself on a knot, else the chord
        double v;
        if (p == 0) v = f[0];
        else if (p == N) v = f[N - 1];
        else {
            const int64_t j = p - 1;
            const double slope = (f[j + 1] - f[j]) / (t[j + 1] - t[j]);
            v = slope * (x - t[j]) + f[j];
        }
        const int64_t o = (G + k - 1) + p;
        t_out[o] = x;
        f_out[o] = v;
    }
}

__global__ void __launch_bounds__(256)
k_interp_points(const int64_t N, const double *__restrict__ t, const double *__restrict__ f,
                const int64_t *__restrict__ cad, const double t0, const double dt,
                const int64_t *__restrict__ offsets, double *__restrict__ t_out, double *__restrict__ f_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    interp_point(N, t, f, cad, t0, dt, offsets, 0, i, t_out, f_out);
}

__global__ void __launch_bounds__(256)
k_interp_missing(const int64_t N, const double *__restrict__ t, const double *__restrict__ f,
                 const int64_t *__restrict__ cad, const double t0, const double dt,
                 const int64_t *__restrict__ offsets, double *__restrict__ t_out, double *__restrict__ f_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t G = offsets[i] - i, gap = offsets[i + 1] - offsets[i] - 1;
    if (gap <= 0) return;
    interp_missing(N, t, f, cad, t0, dt, G, gap, i, t_out, f_out);
}

// ------------------------------------------------------------------------------------
// The same plan and fill over S series at once (gf_interp_plan_seg / gf_interp_fill_seg): segment s owns the
// elements off[s] .. off[s + 1] - 1 of the concatenated arrays.  The structure stays flat -- one count per point, ONE
// int64 scan over the whole concatenation, one thread per point and per gap -- so a single series of 2e6 points is as
// parallel as 1000 of 2000; each point finds its segment by a binary search of off and then applies the per-point
// rules above to its segment's own stretch (first time, first cadence number, searches, ranks: all local), so a
// segment's bits depend on its own data alone.  A segment that is not selected, or whose dt is not a positive
// finite number, counts 1 per point: it comes out as a copy.
// ------------------------------------------------------------------------------------
// the segment that owns element i (0 <= i < off[S]): the last s with off[s] <= i, which steps over empty segments
__device__ __forceinline__ int segment_of(const int64_t *__restrict__ off, const int S, const int64_t i) {
    int lo = 0, hi = S;                             // first s with off[s + 1] > i (off[S] > i)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= i) lo = mid + 1; else hi = mid;
    }
    return lo < S ? lo : S - 1;
}

// dt of a segment to fill, 0 for one to copy (which[s] == 0: dt[s] is not read)
__device__ __forceinline__ double segment_cadence(const uint8_t *__restrict__ which, const double *__restrict__ dt,
                                                  const int s) {
    if (which && !which[s]) return 0.0;
    const double d = dt[s];
    return (d > 0.0 && d < __builtin_inf()) ? d : 0.0;
}

// k_interp_count over the concatenation: plan[i] = exclusive scan of the counts WITHIN the workgroup
__global__ void __launch_bounds__(256)
k_interp_count_seg(const int S, const int64_t total, const int64_t *__restrict__ off, const double *__restrict__ t,
                   const int64_t *__restrict__ cad, const double *__restrict__ dt, const uint8_t *__restrict__ which,
                   int64_t *__restrict__ plan, int64_t *__restrict__ block_sums) {
    __shared__ int64_t part[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_WG + (int64_t)threadIdx.x * 8;
    int64_t loc[8], run = 0;
    if (base < total) {
        int s = segment_of(off, S, base);
        int64_t b = off[s], e = off[s + 1];
        double d = segment_cadence(which, dt, s);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t i = base + k;
            int64_t cnt = 0;
            if (i < total) {
                if (i >= e) {                       // the thread's 8 neighbours cross into a later segment
                    while (i >= e && s + 1 < S) { ++s; e = off[s + 1]; }
                    b = off[s];
                    d = segment_cadence(which, dt, s);
                }
                cnt = (d > 0.0) ? interp_count(e - b, t + b, cad ? cad + b : nullptr, t[b], d, i - b) : 1;
            }
            loc[k] = run;
            run += cnt;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) loc[k] = 0;
    }
    const int64_t before = interp_scan_wg(part, run);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (base + k < total) plan[base + k] = before + loc[k];
    if (threadIdx.x == 255) block_sums[blockIdx.x] = part[255];
}

// new_off[s] = plan[off[s]] (s = 0 .. S); info[s] = 1 where a segment to fill has no usable dt
__global__ void __launch_bounds__(256)
k_interp_seg_offsets(const int S, const int64_t *__restrict__ off, const double *__restrict__ dt,
                     const uint8_t *__restrict__ which, const int64_t *__restrict__ plan,
                     int64_t *__restrict__ new_off, int32_t *__restrict__ info) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s > S) return;
    new_off[s] = plan[off[s]];
    if (s < S) {
        const bool fill = (!which || which[s]) && off[s + 1] > off[s];
        info[s] = (fill && !(segment_cadence(which, dt, s) > 0.0)) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256)
k_interp_points_seg(const int S, const int64_t total, const int64_t *__restrict__ off, const double *__restrict__ t,
                    const double *__restrict__ f, const int64_t *__restrict__ cad, const double *__restrict__ dt,
                    const uint8_t *__restrict__ which, const int64_t *__restrict__ plan,
                    double *__restrict__ t_out, double *__restrict__ f_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int s = segment_of(off, S, i);
    const int64_t b = off[s], n = off[s + 1] - b, o = plan[b];
    const double d = segment_cadence(which, dt, s);
    if (!(d > 0.0)) {
        t_out[o + (i - b)] = t[i];
        f_out[o + (i - b)] = f[i];
        return;
    }
    interp_point(n, t + b, f + b, cad ? cad + b : nullptr, t[b], d, plan + b, o, i - b, t_out + o, f_out + o);
}

__global__ void __launch_bounds__(256)
k_interp_missing_seg(const int S, const int64_t total, const int64_t *__restrict__ off, const double *__restrict__ t,
                     const double *__restrict__ f, const int64_t *__restrict__ cad, const double *__restrict__ dt,
                     const uint8_t *__restrict__ which, const int64_t *__restrict__ plan,
                     double *__restrict__ t_out, double *__restrict__ f_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t gap = plan[i + 1] - plan[i] - 1;
    if (gap <= 0) return;                           // also every point of a copied segment
    const int s = segment_of(off, S, i);
    const int64_t b = off[s], n = off[s + 1] - b, o = plan[b];
    interp_missing(n, t + b, f + b, cad ? cad + b : nullptr, t[b], segment_cadence(which, dt, s),
                   plan[i] - o - (i - b), gap, i - b, t_out + o, f_out + o);
}

int check_segments(const char *who, int S, int64_t total) {
    if (S < 1) return gf_internal_error(-1, "%s: no segments (S=%d)", who, S);
    if (total < 0) return gf_internal_error(-1, "%s: negative length (total=%lld)", who, (long long)total);
    return 0;
}

}  // namespace

extern "C" {

int64_t gf_interp_work(int64_t N) {
    return (N < 1) ? 0 : (N + SCAN_PER_WG - 1) / SCAN_PER_WG;
}

int gf_interp_plan(int64_t N, const double *t, const int64_t *cadences, double dt,
                   int64_t *offsets, int64_t *work, void *stream) {
    if (N < 1) return gf_internal_error(-1, "gf_interp_plan: empty series (N=%lld)", (long long)N);
    if (!t || !offsets || !work) return gf_internal_error(-1, "gf_interp_plan: null pointer");
    if (!(dt > 0.0)) return gf_internal_error(-1, "gf_interp_plan: the cadence must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = gf_interp_work(N);
    double t0;
    if (hipMemcpyAsync(&t0, t, sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return gf_internal_error(-1, "gf_interp_plan: cannot read the first time");
    hipLaunchKernelGGL(k_interp_count, dim3((unsigned)nb), dim3(256), 0, st, N, t, cadences, t0, dt, offsets, work);
    hipLaunchKernelGGL(k_interp_scan_top, dim3(1), dim3(256), 0, st, nb, N, work, offsets);
    hipLaunchKernelGGL(k_interp_offsets, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, work, offsets);
    return check_launch("gf_interp_plan");
}

int gf_interp_fill(int64_t N, const double *t, const double *f, const int64_t *cadences, double dt,
                   const int64_t *offsets, double *t_out, double *f_out, void *stream) {
    if (N < 1) return gf_internal_error(-1, "gf_interp_fill: empty series (N=%lld)", (long long)N);
    if (!t || !f || !offsets || !t_out || !f_out) return gf_internal_error(-1, "gf_interp_fill: null pointer");
    hipStream_t st = (hipStream_t)stream;
    double t0;
    if (hipMemcpyAsync(&t0, t, sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return gf_internal_error(-1, "gf_interp_fill: cannot read the first time");
    hipLaunchKernelGGL(k_interp_points, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, t, f, cadences,
                       t0, dt, offsets, t_out, f_out);
    hipLaunchKernelGGL(k_interp_missing, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, t, f, cadences,
                       t0, dt, offsets, t_out, f_out);
    return check_launch("gf_interp_fill");
}

int64_t gf_interp_seg_work(int64_t total) {
    if (total < 0) return gf_internal_error(-1, "gf_interp_seg_work: negative length (total=%lld)", (long long)total);
    return gf_interp_work(total);
}

int gf_interp_plan_seg(int S, int64_t total, const int64_t *off, const double *t, const int64_t *cadences,
                       const double *dt, const uint8_t *which, int64_t *plan, int64_t *new_off, int32_t *info,
                       int64_t *work, void *stream) {
    if (int st = check_segments("gf_interp_plan_seg", S, total)) return st;
    if (!off || !t || !dt || !plan || !new_off || !info || !work)
        return gf_internal_error(-1, "gf_interp_plan_seg: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = gf_interp_seg_work(total);
    if (nb > 0)
        hipLaunchKernelGGL(k_interp_count_seg, dim3((unsigned)nb), dim3(256), 0, st, S, total, off, t, cadences, dt,
                           which, plan, work);
    hipLaunchKernelGGL(k_interp_scan_top, dim3(1), dim3(256), 0, st, nb, total, work, plan);
    if (total > 0)
        hipLaunchKernelGGL(k_interp_offsets, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, work,
                           plan);
    hipLaunchKernelGGL(k_interp_seg_offsets, dim3((unsigned)(S / 256 + 1)), dim3(256), 0, st, S, off, dt, which, plan,
                       new_off, info);
    return check_launch("gf_interp_plan_seg");
}

int gf_interp_fill_seg(int S, int64_t total, const int64_t *off, const double *t, const double *f,
                       const int64_t *cadences, const double *dt, const uint8_t *which, const int64_t *plan,
                       double *t_out, double *f_out, void *stream) {
    if (int st = check_segments("gf_interp_fill_seg", S, total)) return st;
    if (!off || !t || !f || !dt || !plan || !t_out || !f_out)
        return gf_internal_error(-1, "gf_interp_fill_seg: null pointer");
    if (total == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(k_interp_points_seg, grid, dim3(256), 0, st, S, total, off, t, f, cadences, dt, which, plan,
                       t_out, f_out);
    hipLaunchKernelGGL(k_interp_missing_seg, grid, dim3(256), 0, st, S, total, off, t, f, cadences, dt, which, plan,
                       t_out, f_out);
    return check_launch("gf_interp_fill_seg");
}

int gf_psd_power(int R, int64_t M, int64_t first, double norm, const double *spec,
                 double *power, void *stream) {
    if (R < 1 || M < 1 || first < 0 || first >= M) return gf_internal_error(-1, "gf_psd_power: bad shape (M=%lld, first=%lld)", (long long)M, (long long)first);
    if (!spec || !power) return gf_internal_error(-1, "gf_psd_power: null pointer");
    if (R > 65535) return gf_internal_error(-1, "gf_psd_power: more than 65535 series");
    const int64_t Mout = M - first;
    int64_t blocks = (Mout + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_psd_power, dim3((unsigned)blocks, R), dim3(256), 0, (hipStream_t)stream, M, Mout,
                       first, norm, (const double2 *)spec, power);
    return check_launch("gf_psd_power");
}

int gf_psd_bin(int R, int64_t M, int nb, const double *x, const double *power,
               const int64_t *start, double constant, double *stat, double *err, void *stream) {
    if (R < 1 || M < 1 || nb < 1) return gf_internal_error(-1, "gf_psd_bin: bad shape (M=%lld, bins=%d)", (long long)M, nb);
    if (!x || !power || !start || !stat || !err) return gf_internal_error(-1, "gf_psd_bin: null pointer");
    if (R > 65535) return gf_internal_error(-1, "gf_psd_bin: more than 65535 series");
    hipLaunchKernelGGL(k_psd_bin, dim3(nb, R), dim3(256), 0, (hipStream_t)stream, M, nb, x, power, start,
                       constant, stat, err);
    return check_launch("gf_psd_bin");
}

}  // extern "C"
