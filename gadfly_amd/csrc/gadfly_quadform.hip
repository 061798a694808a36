// gadfly_quadform.hip -- x^T (d Sigma / d theta) x for every celerite coefficient, R vectors per problem
//
// Sigma = K + diag with K_nm = sum_j exp(-c_j tau) (a_j cos d_j tau + b_j sin d_j tau), tau = |t_n - t_m|.  For a vector
// x the derivatives of x^T Sigma x with respect to a, b, c, d of every term are sums over the pairs n > m that factor
// through the generator rows (cos / sin of theta_n = fl(d t_n), gf_rows.h's gen_row: the matrix gf_loglike_grad
// differentiates), so they are diagonal linear recurrences along the rows, per state column (lane) and vector:
//     F_n = p_n (F_{n-1} + v_{n-1} x_{n-1})        v = cos theta (cosine column), sin theta (sine column), 1 (real term)
//     T_n = p_n T_{n-1} + dt_n F_n                 p_n = exp(-c dt_n)
//     P1 += x_n v_n F_n    X1 += x_n v'_n F_n    P2 += x_n v_n T_n    X2 += x_n v'_n T_n     (v' = the partner's phase)
// and, with the cosine and the sine column's sums,  C1 = P1c + P1s, S1 = X1c - X1s, C2 = P2c + P2s, S2 = X2c - X2s:
//     d/da = 2 C1    d/db = 2 S1    d/dc = -2 (a C2 + b S2)    d/dd = 2 (b C2 - a S2)        (real: 2 P1, -2 a P2)
// Lag zero belongs to diag_add alone: g_diag = sum_r w_r |x_r|^2.  No factor, no adjoint sweep.
//
// k_quadform: one wave per (problem, block of QF_RB vectors), lane j owning column j as in k_solve.  The row's phases
//   and decay are made once per block; t_n and x_n are wave-uniform reads, one row ahead of the arithmetic.  Every
//   lane keeps F + v x, T and the four sums of its QF_RB vectors in registers, summed in row order; at the end the
//   block's weighted sums, vectors in order, go to the workspace.  No cross-lane operation, no LDS.
// k_quadform_sum: one wave per problem adds the blocks in order and forms the outputs.
// One summation order per output, no atomics: a problem's bits do not depend on the batch around it, and vectors of
// zeros (or of weight zero) behind its own add exact zeros.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int QF_RB = 8;                // vectors a wave carries
constexpr int QF_MAX_R = 256;          // gf_linear_gram's 255 columns and one more
constexpr int QF_SLOTS = 5;             // per block and lane: P1, X1, P2, X2, sum w x^2

__host__ __device__ inline int qf_blocks(int R) { return (R + QF_RB - 1) / QF_RB; }
inline int64_t qf_work(int R) { return (int64_t)qf_blocks(R) * QF_SLOTS * ROW_LANES; }

// gen_row's phases of a column: (its own, its partner's); (1, 0) for a real term
__device__ __forceinline__ void qf_phases(const Col &q, double tn, double &v, double &vp) {
    if (q.kind == 2) {
        double s, co;
        sincos(q.d * tn, &s, &co);        // theta = fl(d t), as gen_row
        v = q.half ? s : co;
        vp = q.half ? co : s;
    } else {
        v = q.kind == 1 ? 1.0 : 0.0;
        vp = 0.0;
    }
}

__global__ __launch_bounds__(ROW_LANES) void k_quadform(
    int64_t N, int R, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ t, int64_t t_bs, const int64_t *__restrict__ nobs,
    const double *__restrict__ x, int64_t x_bs, int64_t x_rs, const double *__restrict__ w, int64_t w_bs,
    double *__restrict__ work, int64_t work_bs) {
    const int b = (int)blockIdx.x, blk = (int)blockIdx.y, lane = (int)threadIdx.x;
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    const int64_t Nb = clamp_count(nobs, b, N);
    const int r0 = blk * QF_RB;
    const int nr = R - r0 < QF_RB ? R - r0 : QF_RB;        // 1 .. QF_RB vectors of this block
    t += (int64_t)b * t_bs;
    const double *xs = x + (int64_t)b * x_bs + (int64_t)r0 * x_rs;

    double H[QF_RB], T[QF_RB], P1[QF_RB], X1[QF_RB], P2[QF_RB], X2[QF_RB], Q0[QF_RB];
    double xn[QF_RB], xa[QF_RB];                            // row n, and row n + 1 loaded ahead
#pragma unroll
    for (int k = 0; k < QF_RB; ++k) {
        H[k] = T[k] = P1[k] = X1[k] = P2[k] = X2[k] = Q0[k] = 0.0;
        xa[k] = (k < nr && Nb > 0) ? xs[(int64_t)k * x_rs] : 0.0;
    }
    double ta = Nb > 0 ? t[0] : 0.0, tp = ta;
    #pragma unroll 1
    for (int64_t n = 0; n < Nb; ++n) {
        const double tn = ta;
#pragma unroll
        for (int k = 0; k < QF_RB; ++k) xn[k] = xa[k];
        if (n + 1 < Nb) {
            ta = t[n + 1];
#pragma unroll
            for (int k = 0; k < QF_RB; ++k)
                if (k < nr) xa[k] = xs[(int64_t)k * x_rs + n + 1];
        }
        double v, vp;
        qf_phases(q, tn, v, vp);
        const double dt = tn - tp;
        const double p = exp(q.c * (tp - tn));
        tp = tn;
#pragma unroll
        for (int k = 0; k < QF_RB; ++k) {
            const double xk = xn[k];
            const double F = p * H[k];
            const double Tk = fma(dt, F, p * T[k]);
            const double xv = xk * v, xp = xk * vp;
            P1[k] = fma(xv, F, P1[k]);
            X1[k] = fma(xp, F, X1[k]);
            P2[k] = fma(xv, Tk, P2[k]);
            X2[k] = fma(xp, Tk, X2[k]);
            Q0[k] = fma(xk, xk, Q0[k]);
            H[k] = fma(v, xk, F);
            T[k] = Tk;
        }
    }
    // the block's weighted sums, its vectors in order
    const double *wb = w ? w + (int64_t)b * w_bs + r0 : nullptr;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s0 = 0.0;
#pragma unroll
    for (int k = 0; k < QF_RB; ++k) {
        if (k < nr) {
            const double wk = wb ? wb[k] : 1.0;
            s1 = fma(wk, P1[k], s1);
            s2 = fma(wk, X1[k], s2);
            s3 = fma(wk, P2[k], s3);
            s4 = fma(wk, X2[k], s4);
            s0 = fma(wk, Q0[k], s0);
        }
    }
    double *o = work + (int64_t)b * work_bs + (int64_t)blk * QF_SLOTS * ROW_LANES + lane;
    o[0 * ROW_LANES] = s1;
    o[1 * ROW_LANES] = s2;
    o[2 * ROW_LANES] = s3;
    o[3 * ROW_LANES] = s4;
    o[4 * ROW_LANES] = s0;
}

__global__ __launch_bounds__(ROW_LANES) void k_quadform_sum(
    int R, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ work, int64_t work_bs,
    double *__restrict__ g_real, double *__restrict__ g_comp, double *__restrict__ g_diag) {
    const int B = (int)gridDim.x, b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int lr = Jr > 0 ? Jr : 1, lc = Jc > 0 ? Jc : 1;
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    const bool sine = q.kind == 2 && q.half == 1;
    if (q.kind == 0 || sine) {
        if (lane != ROW_LANES - 1) return;                  // (W <= 63: the last lane owns no column; it sums g_diag)
    }
    const int nblk = qf_blocks(R);
    const double *s = work + (int64_t)b * work_bs + lane;
    if (q.kind == 0) {
        double d0 = 0.0;
        for (int k = 0; k < nblk; ++k) d0 += s[((int64_t)k * QF_SLOTS + 4) * ROW_LANES];
        g_diag[b] = d0;
        return;
    }
    // a cosine column adds its sine column's sums (the next lane's), block by block in order
    double p1 = 0.0, x1 = 0.0, p2 = 0.0, x2 = 0.0, p1s = 0.0, x1s = 0.0, p2s = 0.0, x2s = 0.0;
    for (int k = 0; k < nblk; ++k) {
        const double *e = s + (int64_t)k * QF_SLOTS * ROW_LANES;
        p1 += e[0];
        x1 += e[ROW_LANES];
        p2 += e[2 * ROW_LANES];
        x2 += e[3 * ROW_LANES];
        if (q.kind == 2) {
            p1s += e[1];
            x1s += e[ROW_LANES + 1];
            p2s += e[2 * ROW_LANES + 1];
            x2s += e[3 * ROW_LANES + 1];
        }
    }
    if (q.kind == 1) {
        g_real[(int64_t)b * lr + lane] = 2.0 * p1;
        g_real[(int64_t)B * lr + (int64_t)b * lr + lane] = -2.0 * (q.a * p2);
    } else {
        const double C1 = p1 + p1s, S1 = x1 - x1s, C2 = p2 + p2s, S2 = x2 - x2s;
        const int64_t o = (int64_t)b * lc + ((lane - Jr) >> 1);
        g_comp[o] = 2.0 * C1;
        g_comp[(int64_t)B * lc + o] = 2.0 * S1;
        g_comp[(int64_t)2 * B * lc + o] = -2.0 * fma(q.a, C2, q.b * S2);
        g_comp[(int64_t)3 * B * lc + o] = 2.0 * fma(q.b, C2, -(q.a * S2));
    }
}

}  // namespace

extern "C" {

int gf_quadform_grad_block(void) { return QF_RB; }

int64_t gf_quadform_grad_work(int W, int R) {
    if (W < 1 || W > ROW_MAX_W || R < 1 || R > QF_MAX_R) return 0;
    return qf_work(R);
}

int gf_quadform_grad(int B, int64_t N, int R, int Jr, int Jc,
                     const double *ar, const double *cr, const double *ac, const double *bc,
                     const double *cc, const double *dc,
                     const double *t, int64_t t_bs, const int64_t *nobs,
                     const double *x, int64_t x_bs, int64_t x_rs, const double *w, int64_t w_bs,
                     double *work, int64_t work_bs,
                     double *g_real, double *g_comp, double *g_diag, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || R < 1 || R > QF_MAX_R || Jr < 0 || Jc < 0 || W < 1)
        return gf_internal_error(-1, "gf_quadform_grad: bad shape (B=%d, N=%lld, R=%d of 1..%d, Jr=%d, Jc=%d)", B,
                                 (long long)N, R, QF_MAX_R, Jr, Jc);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_quadform_grad: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    if (work_bs < qf_work(R))
        return gf_internal_error(-1, "gf_quadform_grad: work_bs=%lld < gf_quadform_grad_work(W, R)=%lld",
                                 (long long)work_bs, (long long)qf_work(R));
    if (t_bs < 0 || x_rs < N || x_bs < 0 || (x_bs != 0 && x_bs < (int64_t)(R - 1) * x_rs + N) || w_bs < 0 ||
        (w && w_bs != 0 && w_bs < R))
        return gf_internal_error(-1, "gf_quadform_grad: bad stride (t_bs=%lld, x_bs=%lld, x_rs=%lld, w_bs=%lld for "
                                 "R=%d, N=%lld)", (long long)t_bs, (long long)x_bs, (long long)x_rs, (long long)w_bs,
                                 R, (long long)N);
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !t || !x || !work || !g_real || !g_comp ||
        !g_diag)
        return gf_internal_error(-1, "gf_quadform_grad: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_quadform, dim3((unsigned)B, (unsigned)qf_blocks(R)), dim3(ROW_LANES), 0, st, N, R, Jr, Jc,
                       ar, cr, ac, bc, cc, dc, t, t_bs, nobs, x, x_bs, x_rs, w, w_bs, work, work_bs);
    const int st1 = gf_internal_check_launch("gf_quadform_grad");
    if (st1) return st1;
    hipLaunchKernelGGL(k_quadform_sum, dim3((unsigned)B), dim3(ROW_LANES), 0, st, R, Jr, Jc, ar, cr, ac, bc, cc, dc,
                       (const double *)work, work_bs, g_real, g_comp, g_diag);
    return gf_internal_check_launch("gf_quadform_grad");
}

}  // extern "C"
