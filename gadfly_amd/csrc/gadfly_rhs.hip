// gadfly_rhs.hip -- R right-hand sides per problem through ONE pass over the rows
//
// gf_solve_batch and gf_predict_batch_at take one right-hand side per problem and rebuild every generator row and the
// whole W x W state update for it.  The factor does not depend on the right-hand side: here a wave carries RB of them
// at once.  Per row the generator row, the decays, the S update, the pivot D and W are made once (gf_rows.h's fwd_row,
// for the block's first right-hand side); every further right-hand side adds only its own two lines of the recurrence,
//     G_n = P_n (G_{n-1} + W_{n-1} z_{n-1})      z_n = y_n - U_n^T G_n          (lower solve)
//     H_n = P_{n+1} (H_{n+1} + U_{n+1} alpha_{n+1})      alpha_n = z_n / D_n - W_n^T H_n      (upper solve)
// written with fwd_row's and k_solve's own operations and wsum's association: column r of every output has the bits
// gf_solve_batch gives for that column alone, for every R, every seg and every batch around the problem.
// The blocks of RB right-hand sides are the grid's second dimension: ceil(R / RB) waves per problem, each with its own
// workspace slice, run side by side (a batch of a few hundred problems leaves most SIMDs of the device idle).  The
// recompute of pass 2 needs (W, U, P) only: it runs fwd_row with no right-hand side at all.  No atomics.
//
// k_predict_at_rhs is k_predict_at (gadfly_predict.hip) with the generator rows, sincos and exp of every observed row
// and every query made once and the two sums carried for RB columns of alpha.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"
#include "gf_rows.h"

#pragma clang fp contract(off)

namespace {

// right-hand sides a wave carries, per instance (chosen from the resource report: no scratch)
__host__ __device__ constexpr int rhs_rb(int WM) { return WM == 16 ? 8 : WM == 32 ? 8 : 4; }
constexpr int PRED_RB = 8;

// gf_solve_batch's segment rule (the same checkpoints and segments)
inline int64_t rhs_pick_seg(int64_t N, int W, int64_t seg) {
    if (seg == 0) return gf_solve_batch_seg(N, W);
    return seg > N ? N : seg;
}

// one block of right-hand sides: checkpoints, one segment's staged rows, D of every row, z (then alpha) per column
inline int64_t rhs_work_block(int64_t N, int WM, int64_t K) {
    const int64_t nseg = (N + K - 1) / K;
    return nseg * solve_ck(WM) + K * solve_rs() + (1 + rhs_rb(WM)) * solve_n64(N);
}

inline int rhs_blocks(int R, int RB) { return (R + RB - 1) / RB; }

template <int WM, int RB>
__global__ __launch_bounds__(ROW_LANES) void k_solve_rhs(
    int64_t N, int R, int64_t K, int64_t nseg, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add,
    const double *__restrict__ t, int64_t t_bs, const double *__restrict__ dg, int64_t d_bs,
    const double *__restrict__ y, int64_t y_bs, int64_t y_rs, double *__restrict__ work, int64_t work_bs,
    int64_t blk_work, double *alpha, double *mu, int64_t o_bs, int64_t o_rs, double *__restrict__ ll,
    int32_t *__restrict__ info) {
    __shared__ double sh[2][3 * ROW_LANES];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int r0 = (int)blockIdx.y * RB;
    const int nr = (R - r0 < RB) ? R - r0 : RB;            // live columns of this block (>= 1)
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    t += (int64_t)b * t_bs;
    if (dg) dg += (int64_t)b * d_bs;
    // column j of the block; a dead one (j >= nr) reads the block's last live column and stores nothing
    const double *yj[RB];
    double *aj[RB], *mj[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int r = r0 + (j < nr ? j : nr - 1);
        yj[j] = y + (int64_t)b * y_bs + (int64_t)r * y_rs;
        aj[j] = alpha ? alpha + (int64_t)b * o_bs + (int64_t)r * o_rs : nullptr;
        mj[j] = mu ? mu + (int64_t)b * o_bs + (int64_t)r * o_rs : nullptr;
    }
    double *ck = work + (int64_t)b * work_bs + (int64_t)blockIdx.y * blk_work;
    double *rows = ck + nseg * solve_ck(WM);
    double *Dw = rows + K * solve_rs();
    double *zw = Dw + solve_n64(N);                        // z_n, then alpha_n: column j at zw + j n64
    const int64_t n64 = solve_n64(N);
    const double dadd = diag_add[b];

    // ---- pass 1: log L, D of every row, z of every row and column, the checkpoints
    double S[WM];
#pragma unroll
    for (int k = 0; k < WM; ++k) S[k] = 0.0;
    double G[RB], z[RB], quad[RB], zbuf[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) { G[j] = 0.0; z[j] = 0.0; quad[j] = 0.0; zbuf[j] = 0.0; }
    double w = 0.0, D = 0.0, u, p;
    double logdet = 0.0, dbuf = 1.0;
    int64_t bad = 0, left = 0, seg = 0;
    #pragma unroll 1
    for (int64_t n = 0; n < N; ++n) {
        if (left == 0) {
            ck_store<WM>(ck + seg * solve_ck(WM), lane, S, G[0], w, D, z[0]);
            left = K;
            ++seg;
        }
        --left;
        const double tn = t[n], tp = n ? t[n - 1] : tn;
        const double An = (dg ? dg[n] : 0.0) + dadd;
        const double wold = w;
        fwd_row<WM>(S, G[0], w, D, z[0], q, tp, tn, An, yj[0][n], sh[n & 1], lane, u, p);
#pragma unroll
        for (int j = 1; j < RB; ++j) {
            G[j] = p * fma(wold, z[j], G[j]);
            z[j] = yj[j][n] - wsum(u * G[j]);
        }
        if (!(D > 0.0)) { bad = n + 1; break; }
        logdet += log(D);
        const int slot = (int)(n & 63);
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            quad[j] += z[j] * z[j] / D;
            if (lane == slot) zbuf[j] = z[j];
        }
        if (lane == slot) dbuf = D;
        if (slot == 63 || n == N - 1) {
            const int64_t i = (n - slot) + lane;
            if (i <= n) {
                Dw[i] = dbuf;
#pragma unroll
                for (int j = 0; j < RB; ++j) zw[j * n64 + i] = zbuf[j];
            }
        }
    }
    if (bad) {
        const double nan = __builtin_nan("");
        if (lane == 0) {
            if (blockIdx.y == 0) info[b] = (int32_t)bad;
            for (int j = 0; j < nr; ++j) ll[(int64_t)b * R + r0 + j] = -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            if (j < nr) {
                for (int64_t i = lane; i < N; i += ROW_LANES) {
                    if (alpha) aj[j][i] = nan;
                    if (mu) mj[j][i] = nan;
                }
            }
        }
        return;
    }
    if (lane == 0) {
        if (blockIdx.y == 0) info[b] = 0;
#pragma unroll
        for (int j = 0; j < RB; ++j)
            if (j < nr) ll[(int64_t)b * R + r0 + j] = -0.5 * (logdet + quad[j] + (double)N * log(6.283185307179586));
    }

    // ---- pass 2: segments last first, (W, U, P) of their rows recomputed from the checkpoint, then the upper solves
    double H[RB], anext[RB], abuf[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) { H[j] = 0.0; anext[j] = 0.0; abuf[j] = 0.0; }
    double unext = 0.0, pnext = 0.0;
    #pragma unroll 1
    for (int64_t s = nseg - 1; s >= 0; --s) {
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        const double *c = ck + s * solve_ck(WM);
#pragma unroll
        for (int k = 0; k < WM; ++k) S[k] = c[lane * WM + k];
        w = c[(WM + 1) * ROW_LANES + lane];
        D = c[(WM + 2) * ROW_LANES + lane];
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            const double tn = t[n], tp = n ? t[n - 1] : tn;
            const double An = (dg ? dg[n] : 0.0) + dadd;
            double G0 = 0.0, z0 = 0.0;                     // (the factor's rows do not depend on a right-hand side)
            fwd_row<WM>(S, G0, w, D, z0, q, tp, tn, An, 0.0, sh[n & 1], lane, u, p);
            double *r = rows + (n - n0) * solve_rs();
            r[lane] = w;
            r[ROW_LANES + lane] = u;
            r[2 * ROW_LANES + lane] = p;
        }
        #pragma unroll 1
        for (int64_t n = n1 - 1; n >= n0; --n) {
            const double *r = rows + (n - n0) * solve_rs();
            const double wn = r[lane], un = r[ROW_LANES + lane], pn = r[2 * ROW_LANES + lane];
            const int slot = (int)(n & 63);
            if (slot == 63 || n == N - 1) {
                const int64_t i = (n - slot) + lane;
                dbuf = i <= n ? Dw[i] : 1.0;
#pragma unroll
                for (int j = 0; j < RB; ++j) zbuf[j] = i <= n ? zw[j * n64 + i] : 0.0;
            }
            const double Dn = read_lane(dbuf, slot);
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const double zn = read_lane(zbuf[j], slot);
                H[j] = pnext * fma(unext, anext[j], H[j]);
                const double a = zn / Dn - wsum(wn * H[j]);
                anext[j] = a;
                if (lane == slot) abuf[j] = a;
            }
            unext = un; pnext = pn;
            if (slot == 0) {
                const int64_t i = n + lane;
                if (i < N) {
#pragma unroll
                    for (int j = 0; j < RB; ++j)
                        if (j < nr) stage_alpha(i, abuf[j], zw + j * n64, aj[j], mj[j], dg, yj[j]);
                }
            }
        }
    }
}

// NR arrays x_j[0 .. n) read one element at a time, in steps of DIR = +1 or -1, by the whole wave: lane l holds
// x_j[64 blk + l], the block after it in the direction of travel is already loaded
template <int DIR, int NR>
struct RunR {
    const double *x[NR];
    int64_t n, blk;
    double cur[NR], nxt[NR];

    __device__ __forceinline__ double block(int j, int64_t b, int lane) const {
        const int64_t i = b * ROW_LANES + lane;
        return (b >= 0 && i < n) ? x[j][i] : 0.0;
    }
    // (n >= 1, 0 <= first < n; x[] set by the caller)
    __device__ __forceinline__ void open(int64_t n_, int64_t first, int lane) {
        n = n_; blk = first >> 6;
#pragma unroll
        for (int j = 0; j < NR; ++j) { cur[j] = block(j, blk, lane); nxt[j] = block(j, blk + DIR, lane); }
    }
    // 0 <= i < n, and i is the index of the previous call or one step of DIR beyond it
    __device__ __forceinline__ void step(int64_t i, int lane) {
        if ((i >> 6) != blk) {
            blk += DIR;
#pragma unroll
            for (int j = 0; j < NR; ++j) { cur[j] = nxt[j]; nxt[j] = block(j, blk + DIR, lane); }
        }
    }
    __device__ __forceinline__ double get(int j, int64_t i) const { return read_lane(cur[j], (int)(i & 63)); }
};

template <int RB>
__global__ __launch_bounds__(ROW_LANES) void k_predict_at_rhs(
    int64_t N, int64_t M, int R, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ t, int64_t t_bs, const int64_t *__restrict__ nobs,
    const double *__restrict__ ts, int64_t ts_bs, const int64_t *__restrict__ nq,
    const double *__restrict__ alpha, int64_t alpha_bs, int64_t alpha_rs, double *mu, int64_t mu_bs, int64_t mu_rs) {
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int r0 = (int)blockIdx.y * RB;
    const int nr = (R - r0 < RB) ? R - r0 : RB;
    const int64_t No = clamp_count(nobs, b, N), Mq = clamp_count(nq, b, M);
    if (Mq == 0) return;
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    t += (int64_t)b * t_bs;
    ts += (int64_t)b * ts_bs;
    const double *aj[RB];
    double *mj[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int r = r0 + (j < nr ? j : nr - 1);          // (a dead column reads the last live one, stores nothing)
        aj[j] = alpha + (int64_t)b * alpha_bs + (int64_t)r * alpha_rs;
        mj[j] = mu + (int64_t)b * mu_bs + (int64_t)r * mu_rs;
    }
    double buf[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) buf[j] = 0.0;

    // ---- forward: the observed rows at or before each query
    {
        RunR<1, 1> T, Q;
        RunR<1, RB> A;
        Q.x[0] = ts; T.x[0] = t;
#pragma unroll
        for (int j = 0; j < RB; ++j) A.x[j] = aj[j];
        Q.open(Mq, 0, lane);
        if (No) { T.open(No, 0, lane); A.open(No, 0, lane); }
        double F[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) F[j] = 0.0;
        double last = 0.0;
        int64_t n = 0;
        double tn = No ? T.get(0, 0) : 0.0;
        #pragma unroll 1
        for (int64_t m = 0; m < Mq; ++m) {
            Q.step(m, lane);
            const double tm = Q.get(0, m);
            #pragma unroll 1
            while (n < No && tn <= tm) {
                A.step(n, lane);
                double u, v;
                gen_row(q, tn, u, v);
                const double p = exp(q.c * ((n ? last : tn) - tn));
#pragma unroll
                for (int j = 0; j < RB; ++j) F[j] = fma(v, A.get(j, n), p * F[j]);
                last = tn;
                if (++n < No) { T.step(n, lane); tn = T.get(0, n); }
            }
            const int slot = (int)(m & 63);
            if (n) {                                  // (no observed row yet: nothing below this query)
                double u, v;
                gen_row(q, tm, u, v);
                const double ue = u * exp(q.c * (last - tm));
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const double lo = wsum(ue * F[j]);
                    if (lane == slot) buf[j] = lo;
                }
            } else {
#pragma unroll
                for (int j = 0; j < RB; ++j)
                    if (lane == slot) buf[j] = 0.0;
            }
            if (slot == 63 || m == Mq - 1) {
                const int64_t i = (m - slot) + lane;
                if (i <= m) {
#pragma unroll
                    for (int j = 0; j < RB; ++j)
                        if (j < nr) mj[j][i] = buf[j];
                }
            }
        }
    }

    // ---- backward: the observed rows beyond each query, added to what the forward pass left
    {
        RunR<-1, 1> T, Q;
        RunR<-1, RB> A;
        Q.x[0] = ts; T.x[0] = t;
#pragma unroll
        for (int j = 0; j < RB; ++j) A.x[j] = aj[j];
        Q.open(Mq, Mq - 1, lane);
        if (No) { T.open(No, No - 1, lane); A.open(No, No - 1, lane); }
        double H[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) H[j] = 0.0;
        double last = 0.0;
        int64_t n = No - 1;
        double tn = No ? T.get(0, n) : 0.0;
        #pragma unroll 1
        for (int64_t m = Mq - 1; m >= 0; --m) {
            Q.step(m, lane);
            const double tm = Q.get(0, m);
            #pragma unroll 1
            while (n >= 0 && tn > tm) {
                A.step(n, lane);
                double u, v;
                gen_row(q, tn, u, v);
                const double p = exp(q.c * (tn - (n == No - 1 ? tn : last)));
#pragma unroll
                for (int j = 0; j < RB; ++j) H[j] = fma(u, A.get(j, n), p * H[j]);
                last = tn;
                if (--n >= 0) { T.step(n, lane); tn = T.get(0, n); }
            }
            const int slot = (int)(m & 63);
            if (slot == 63 || m == Mq - 1) {
                const int64_t i = (m - slot) + lane;
#pragma unroll
                for (int j = 0; j < RB; ++j) buf[j] = (i <= m && j < nr) ? mj[j][i] : 0.0;
            }
            if (n < No - 1) {
                double u, v;
                gen_row(q, tm, u, v);
                const double ve = v * exp(q.c * (tm - last));
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const double up = wsum(ve * H[j]);
                    if (lane == slot) buf[j] = buf[j] + up;
                }
            } else {
#pragma unroll
                for (int j = 0; j < RB; ++j)
                    if (lane == slot) buf[j] = buf[j] + 0.0;
            }
            if (slot == 0) {
                const int64_t i = m + lane;
                if (i < Mq) {
#pragma unroll
                    for (int j = 0; j < RB; ++j)
                        if (j < nr) mj[j][i] = buf[j];
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int gf_solve_batch_rhs_block(int W) {
    if (W < 1 || W > ROW_MAX_W) return 0;
    return rhs_rb(row_wm(W));
}

int gf_predict_batch_at_rhs_block(void) { return PRED_RB; }

int64_t gf_solve_batch_rhs_work(int64_t N, int W, int R, int64_t seg) {
    if (!row_shape_ok(N, W) || R < 1 || seg < 0) return 0;
    const int WM = row_wm(W);
    return rhs_blocks(R, rhs_rb(WM)) * rhs_work_block(N, WM, rhs_pick_seg(N, W, seg));
}

int gf_solve_batch_rhs(int B, int64_t N, int R, int Jr, int Jc,
                       const double *ar, const double *cr, const double *ac, const double *bc,
                       const double *cc, const double *dc, const double *diag_add,
                       const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                       const double *y, int64_t y_bs, int64_t y_rs, int64_t seg, double *work, int64_t work_bs,
                       double *alpha, double *mu, int64_t out_bs, int64_t out_rs, double *ll, int32_t *info,
                       void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || R < 1 || Jr < 0 || Jc < 0 || W < 1 || seg < 0)
        return gf_internal_error(-1, "gf_solve_batch_rhs: bad shape (B=%d, N=%lld, R=%d, Jr=%d, Jc=%d, seg=%lld)",
                                 B, (long long)N, R, Jr, Jc, (long long)seg);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_solve_batch_rhs: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    const int WM = row_wm(W), RB = rhs_rb(WM), nblk = rhs_blocks(R, RB);
    if (nblk > 65535)
        return gf_internal_error(-1, "gf_solve_batch_rhs: R=%d right-hand sides exceed %d blocks of %d", R, 65535, RB);
    const int64_t K = rhs_pick_seg(N, W, seg), nseg = (N + K - 1) / K;
    const int64_t blk_work = rhs_work_block(N, WM, K);
    if (work_bs < nblk * blk_work)
        return gf_internal_error(-1, "gf_solve_batch_rhs: work_bs=%lld < gf_solve_batch_rhs_work(N, W, R, seg)=%lld",
                                 (long long)work_bs, (long long)(nblk * blk_work));
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !work || !ll || !info)
        return gf_internal_error(-1, "gf_solve_batch_rhs: null pointer");
    if (t_bs < 0 || y_bs < 0 || y_rs < 0 || (R > 1 && y_rs < N) ||
        ((alpha || mu) && ((R > 1 && out_rs < N) || (B > 1 && out_bs < (int64_t)R * N))))
        return gf_internal_error(-1, "gf_solve_batch_rhs: bad stride (t_bs=%lld, y_bs=%lld, y_rs=%lld, out_bs=%lld, "
                                 "out_rs=%lld for R=%d, N=%lld)", (long long)t_bs, (long long)y_bs, (long long)y_rs,
                                 (long long)out_bs, (long long)out_rs, R, (long long)N);
    hipStream_t st = (hipStream_t)stream;
#define RS_LAUNCH(WMV)                                                                                             \
    hipLaunchKernelGGL((k_solve_rhs<WMV, rhs_rb(WMV)>), dim3((unsigned)B, (unsigned)nblk), dim3(ROW_LANES), 0, st, \
                       N, R, K, nseg, Jr, Jc, ar, cr, ac, bc, cc, dc, diag_add, t, t_bs, diag, diag_bs, y, y_bs,  \
                       y_rs, work, work_bs, blk_work, alpha, mu, out_bs, out_rs, ll, info)
    if (WM == 16) RS_LAUNCH(16);
    else if (WM == 32) RS_LAUNCH(32);
    else RS_LAUNCH(64);
#undef RS_LAUNCH
    return gf_internal_check_launch("gf_solve_batch_rhs");
}

int gf_predict_batch_at_rhs(int B, int64_t N, int64_t M, int R, int Jr, int Jc,
                            const double *ar, const double *cr, const double *ac,
                            const double *bc, const double *cc, const double *dc,
                            const double *t, int64_t t_bs, const int64_t *nobs,
                            const double *ts, int64_t ts_bs, const int64_t *nq,
                            const double *alpha, int64_t alpha_bs, int64_t alpha_rs,
                            double *mu, int64_t mu_bs, int64_t mu_rs, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || M < 1 || R < 1 || Jr < 0 || Jc < 0 || W < 1)
        return gf_internal_error(-1, "gf_predict_batch_at_rhs: bad shape (B=%d, N=%lld, M=%lld, R=%d, Jr=%d, Jc=%d)",
                                 B, (long long)N, (long long)M, R, Jr, Jc);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_predict_batch_at_rhs: width W=%d exceeds the one-wave limit %d", W,
                                 ROW_MAX_W);
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !t || !ts || !alpha || !mu)
        return gf_internal_error(-1, "gf_predict_batch_at_rhs: null pointer");
    const int nblk = rhs_blocks(R, PRED_RB);
    if (nblk > 65535)
        return gf_internal_error(-1, "gf_predict_batch_at_rhs: R=%d right-hand sides exceed %d blocks of %d", R, 65535,
                                 PRED_RB);
    if (t_bs < 0 || ts_bs < 0 || (R > 1 && (alpha_rs < N || mu_rs < M)) ||
        (B > 1 && (alpha_bs < (int64_t)R * N || mu_bs < (int64_t)R * M)))
        return gf_internal_error(-1, "gf_predict_batch_at_rhs: bad stride (t_bs=%lld, ts_bs=%lld, alpha_bs=%lld, "
                                 "alpha_rs=%lld, mu_bs=%lld, mu_rs=%lld for R=%d, N=%lld, M=%lld)", (long long)t_bs,
                                 (long long)ts_bs, (long long)alpha_bs, (long long)alpha_rs, (long long)mu_bs,
                                 (long long)mu_rs, R, (long long)N, (long long)M);
    hipLaunchKernelGGL((k_predict_at_rhs<PRED_RB>), dim3((unsigned)B, (unsigned)nblk), dim3(ROW_LANES), 0,
                       (hipStream_t)stream, N, M, R, Jr, Jc, ar, cr, ac, bc, cc, dc, t, t_bs, nobs, ts, ts_bs, nq,
                       alpha, alpha_bs, alpha_rs, mu, mu_bs, mu_rs);
    return gf_internal_check_launch("gf_predict_batch_at_rhs");
}

}  // extern "C"
