// gadfly_linmodel.hip -- [A | y]^T Sigma^-1 [A | y] of B problems from ONE forward sweep
//
// A linear mean under a celerite kernel, y = A beta + eps with eps ~ N(0, Sigma): the generalised least squares fit,
// its covariance, the profile and the marginal likelihood all follow from the (R+1) x (R+1) Gram matrix
//     G = Z^T D^-1 Z,   Z = L^-1 [A | y],   Sigma = L D L^T,
// and sum log D.  No upper solve, no checkpoints, nothing of size N comes back.
//
// k_lin_sweep: one workgroup of two waves per (problem, block of 64 columns of [A | y]).
//   wave 0   runs gf_rows.h's fwd_row, exactly as k_solve's pass 1 (no right-hand side): D and info are
//            gf_solve_batch's.  fwd_row publishes w_{n-1}, p_n, u_n in LDS, double-buffered by row parity, behind its
//            one workgroup barrier per row; D_n goes to one more slot and is read one row later.
//   wave 1   carries one column per lane, lane r its own G_r[WM] in registers:
//                G_j <- p_j (G_j + w_j z_prev)      z = A[n, r] - sum_j u_j G_j
//            2 WM FMAs per row from broadcast LDS reads, no cross-lane operation.  z_n / sqrt(D_n) goes to the
//            workspace row-major, (N, ld): 64 lanes store one contiguous run.  Its barrier orders LDS only, so the
//            rows of A loaded four ahead stay in flight.
// k_lin_gram: G_ij = sum_n zs_ni zs_nj, one thread per entry of an 8 x 8 tile of the upper triangle, the rows n = s mod 4
//   summed in order by wave s and the four partial sums added as (0 + 1) + (2 + 3): one fixed order per entry, whatever
//   the batch, the groups and the other columns.  fma(a, b, c) == fma(b, a, c), and both halves are written from one
//   value: G equals its transpose bit for bit.  No atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"
#include "gf_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int LIN_MAX_R = 255;          // columns of A: [A | y] fills at most four blocks of 64
constexpr int LIN_AHEAD = 4;            // rows of A a lane holds ahead of the sweep
constexpr int LIN_TILE = 8;             // edge of a tile of Gram entries
constexpr int LIN_SLICES = 4;           // waves of k_lin_gram: rows n = s mod 4

// leading dimension of the stored zs rows: the R + 1 columns rounded up to whole tiles (the pad columns hold zeros)
__host__ __device__ inline int lin_ld(int R) { return (R + 1 + LIN_TILE - 1) / LIN_TILE * LIN_TILE; }

template <int WM>
__global__ __launch_bounds__(2 * ROW_LANES) void k_lin_sweep(
    int64_t N, int R, int ld, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add,
    const double *__restrict__ t, int64_t t_bs, const double *__restrict__ dg, int64_t d_bs,
    const double *__restrict__ y, int64_t y_bs, const int64_t *__restrict__ nobs,
    const double *__restrict__ A, int64_t lda, int64_t a_bs, double *__restrict__ work, int64_t work_bs,
    double *__restrict__ logdet, int32_t *__restrict__ info) {
    __shared__ double sh[2][3 * ROW_LANES];
    __shared__ double dsh[2];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x & (ROW_LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int64_t Nb = clamp_count(nobs, b, N);

    if (wave == 0) {
        // ---- the factor: k_solve's pass 1 without a right-hand side
        const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
        t += (int64_t)b * t_bs;
        if (dg) dg += (int64_t)b * d_bs;
        const double dadd = diag_add[b];
        double S[WM];
#pragma unroll
        for (int k = 0; k < WM; ++k) S[k] = 0.0;
        double w = 0.0, D = 0.0, u, p;
        double ld_sum = 0.0;
        int64_t bad = 0;
        #pragma unroll 1
        for (int64_t n = 0; n < Nb; ++n) {
            const double tn = t[n], tp = n ? t[n - 1] : tn;
            const double An = (dg ? dg[n] : 0.0) + dadd;
            double G0 = 0.0, z0 = 0.0;
            fwd_row<WM>(S, G0, w, D, z0, q, tp, tn, An, 0.0, sh[n & 1], lane, u, p);
            if (lane == 0) dsh[n & 1] = D;
            if (!(D > 0.0)) { bad = n + 1; break; }
            ld_sum += log(D);
        }
        __syncthreads();                // wave 1 reads the last row's D (or the failed pivot) behind this one
        if (lane == 0 && blockIdx.y == 0) {
            info[b] = (int32_t)bad;
            logdet[b] = bad ? __builtin_nan("") : ld_sum;
        }
        return;
    }

    // ---- the columns: lane r carries column c of [A | y]
    const int c = (int)blockIdx.y * ROW_LANES + lane;
    const bool stored = c < ld;                             // (c > R: a zero column, so that whole tiles can be read)
    const double *src = nullptr;
    int64_t step = 0;
    if (c < R) { src = A + (int64_t)b * a_bs + c; step = lda; }
    else if (c == R) { src = y + (int64_t)b * y_bs; step = 1; }
    double *zs = work + (int64_t)b * work_bs + c;
    double G[WM];
#pragma unroll
    for (int k = 0; k < WM; ++k) G[k] = 0.0;
    double z = 0.0;
    double nxt[LIN_AHEAD];                                  // rows n .. n + LIN_AHEAD - 1 of the column, loaded ahead
#pragma unroll
    for (int k = 0; k < LIN_AHEAD; ++k) nxt[k] = (src && k < Nb) ? src[(int64_t)k * step] : 0.0;
    #pragma unroll 1
    for (int64_t n = 0;; ++n) {                             // rows 0 .. Nb: the last turn only finishes row Nb - 1
        wg_lds_barrier();
        if (n > 0) {
            const double Dp = read_lane(dsh[(n - 1) & 1], 0);
            if (!(Dp > 0.0)) break;                         // (the factor wave has set info)
            if (stored) zs[(n - 1) * (int64_t)ld] = z / sqrt(Dp);
        }
        if (n >= Nb) break;
        const double an = nxt[0];
#pragma unroll
        for (int k = 0; k + 1 < LIN_AHEAD; ++k) nxt[k] = nxt[k + 1];
        nxt[LIN_AHEAD - 1] = (src && n + LIN_AHEAD < Nb) ? src[(n + LIN_AHEAD) * step] : 0.0;
        const double *s = sh[n & 1];
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < WM; ++j) {
            const double g = s[ROW_LANES + j] * fma(s[j], z, G[j]);
            G[j] = g;
            acc = fma(s[2 * ROW_LANES + j], g, acc);
            ROW_PACE(j);
        }
        z = an - acc;
    }
}

__global__ __launch_bounds__(LIN_SLICES * ROW_LANES) void k_lin_gram(
    int64_t N, int R, int ld, const int64_t *__restrict__ nobs, const double *__restrict__ work, int64_t work_bs,
    const int32_t *__restrict__ info, double *__restrict__ gram) {
    __shared__ double part[LIN_SLICES][ROW_LANES];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x & (ROW_LANES - 1), s = (int)threadIdx.x >> 6;
    const int C = R + 1, T = ld / LIN_TILE;
    int ti = 0, rem = (int)blockIdx.y;                      // tile (ti, tj), ti <= tj, of the upper triangle
    while (rem >= T - ti) { rem -= T - ti; ++ti; }
    const int tj = ti + rem;
    const int i = ti * LIN_TILE + (lane >> 3), j = tj * LIN_TILE + (lane & 7);
    const int64_t Nb = clamp_count(nobs, b, N);
    const bool bad = info[b] != 0;
    double acc = 0.0;
    if (!bad) {
        const double *zi = work + (int64_t)b * work_bs + i, *zj = work + (int64_t)b * work_bs + j;
        #pragma unroll 4
        for (int64_t n = s; n < Nb; n += LIN_SLICES) acc = fma(zi[n * ld], zj[n * ld], acc);
    }
    part[s][lane] = acc;
    __syncthreads();
    if (s == 0 && i <= j && j < C) {
        const double g = bad ? __builtin_nan("") : (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        double *o = gram + (int64_t)b * C * C;
        o[(int64_t)i * C + j] = g;
        o[(int64_t)j * C + i] = g;
    }
}

}  // namespace

extern "C" {

int64_t gf_linear_gram_work(int64_t N, int W, int R) {
    if (!row_shape_ok(N, W) || R < 1 || R > LIN_MAX_R) return 0;
    return N * lin_ld(R);
}

int gf_linear_gram(int B, int64_t N, int R, int Jr, int Jc,
                   const double *ar, const double *cr, const double *ac, const double *bc,
                   const double *cc, const double *dc, const double *diag_add,
                   const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                   const double *y, int64_t y_bs, const int64_t *nobs,
                   const double *A, int64_t lda, int64_t a_bs, double *work, int64_t work_bs,
                   double *gram, double *logdet, int32_t *info, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || R < 1 || R > LIN_MAX_R || Jr < 0 || Jc < 0 || W < 1)
        return gf_internal_error(-1, "gf_linear_gram: bad shape (B=%d, N=%lld, R=%d of 1..%d, Jr=%d, Jc=%d)", B,
                                 (long long)N, R, LIN_MAX_R, Jr, Jc);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_linear_gram: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    const int ld = lin_ld(R);
    if (work_bs < N * ld)
        return gf_internal_error(-1, "gf_linear_gram: work_bs=%lld < gf_linear_gram_work(N, W, R)=%lld",
                                 (long long)work_bs, (long long)(N * ld));
    if (t_bs < 0 || diag_bs < 0 || y_bs < 0 || lda < R || a_bs < 0 || (a_bs != 0 && a_bs < (N - 1) * lda + R))
        return gf_internal_error(-1, "gf_linear_gram: bad stride (t_bs=%lld, diag_bs=%lld, y_bs=%lld, lda=%lld, "
                                 "a_bs=%lld for R=%d, N=%lld)", (long long)t_bs, (long long)diag_bs, (long long)y_bs,
                                 (long long)lda, (long long)a_bs, R, (long long)N);
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !A || !work || !gram ||
        !logdet || !info)
        return gf_internal_error(-1, "gf_linear_gram: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (R + 1 + ROW_LANES - 1) / ROW_LANES, T = ld / LIN_TILE;
    const int WM = row_wm(W);
#define LM_LAUNCH(WMV)                                                                                             \
    hipLaunchKernelGGL((k_lin_sweep<WMV>), dim3((unsigned)B, (unsigned)nblk), dim3(2 * ROW_LANES), 0, st, N, R, ld, \
                       Jr, Jc, ar, cr, ac, bc, cc, dc, diag_add, t, t_bs, diag, diag_bs, y, y_bs, nobs, A, lda,    \
                       a_bs, work, work_bs, logdet, info)
    if (WM == 16) LM_LAUNCH(16);
    else if (WM == 32) LM_LAUNCH(32);
    else LM_LAUNCH(64);
#undef LM_LAUNCH
    const int st1 = gf_internal_check_launch("gf_linear_gram");
    if (st1) return st1;
    hipLaunchKernelGGL(k_lin_gram, dim3((unsigned)B, (unsigned)(T * (T + 1) / 2)), dim3(LIN_SLICES * ROW_LANES), 0, st,
                       N, R, ld, nobs, (const double *)work, work_bs, (const int32_t *)info, gram);
    return gf_internal_check_launch("gf_linear_gram");
}

}  // extern "C"
