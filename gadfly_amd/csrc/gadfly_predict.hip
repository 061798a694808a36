// gadfly_predict.hip -- conditional means of B problems at new times t* in one call
//
// celerite2's counterpart: general_matmul_lower + general_matmul_upper between two sorted axes, what
// GaussianProcess.predict(y, t=t*) runs after apply_inverse (ConditionalDistribution.mean).  With alpha = K^-1 (y - mean)
// already on the device (gf_solve_batch),
//     mu*_m = sum_{t_n <= t*_m} (U*_m o e^{-c (t*_m - t_n)}) . V_n alpha_n
//           + sum_{t_n >  t*_m} (V*_m o e^{-c (t_n - t*_m)}) . U_n alpha_n
// for the coefficients of the full kernel or of one of its parts.  One wave per problem, lane j owning column j, the
// two sorted axes merged under wave-uniform control flow (every stamp is read through readlane, so every branch is a
// scalar one):
//   forward    F <- e^{c (last - t_n)} o F + V_n alpha_n for the observed rows up to and including t*_m, then
//              lo_m = U*_m^T (e^{c (last - t*_m)} o F);
//   backward   H <- e^{c (t_n - last)} o H + U_n alpha_n for the observed rows beyond t*_m, then
//              mu*_m = lo_m + V*_m^T (e^{c (t*_m - last)} o H).
// The state steps from observed stamp to observed stamp only and a query reads it without touching it: a query's value
// does not depend on which other queries the call holds.  Generator rows are exact on every row, observed or queried
// (theta = fl(d t), as celerite2), made in registers by gadfly_solve.hip's gen_row (gf_rows.h): nothing of size N W or
// M W exists.
// Stamps, alpha and results live in lane i mod 64 and move 64 at a time: every load and store of the wave is one
// contiguous 512-byte run, the next run of each input is in flight while the current one is consumed, and a lane reads
// back only the results it wrote itself.  No workspace, no LDS, no atomics: results are bit-identical from run to run
// and whatever the batch around a problem.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"
#include "gf_rows.h"

#pragma clang fp contract(off)

namespace {

// x[0 .. n) read one element at a time, in steps of DIR = +1 or -1, by the whole wave: lane l holds x[64 blk + l], the
// block after it in the direction of travel is already loaded
template <int DIR>
struct Run {
    const double *x;
    int64_t n, blk;
    double cur, nxt;

    __device__ __forceinline__ double block(int64_t b, int lane) const {
        const int64_t i = b * ROW_LANES + lane;
        return (b >= 0 && i < n) ? x[i] : 0.0;
    }
    // (n >= 1, 0 <= first < n)
    __device__ __forceinline__ void open(const double *x_, int64_t n_, int64_t first, int lane) {
        x = x_; n = n_; blk = first >> 6;
        cur = block(blk, lane);
        nxt = block(blk + DIR, lane);
    }
    // 0 <= i < n, and i is the index of the previous call or one step of DIR beyond it
    __device__ __forceinline__ double get(int64_t i, int lane) {
        if ((i >> 6) != blk) {
            blk += DIR;
            cur = nxt;
            nxt = block(blk + DIR, lane);
        }
        return read_lane(cur, (int)(i & 63));
    }
};

__global__ __launch_bounds__(ROW_LANES) void k_predict_at(
    int64_t N, int64_t M, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ t, int64_t t_bs, const int64_t *__restrict__ nobs,
    const double *__restrict__ ts, int64_t ts_bs, const int64_t *__restrict__ nq,
    const double *__restrict__ alpha, int64_t alpha_bs, double *mu, int64_t mu_bs) {
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int64_t No = clamp_count(nobs, b, N), Mq = clamp_count(nq, b, M);
    if (Mq == 0) return;
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    t += (int64_t)b * t_bs;
    ts += (int64_t)b * ts_bs;
    alpha += (int64_t)b * alpha_bs;
    mu += (int64_t)b * mu_bs;
    double buf = 0.0;

    // ---- forward: the observed rows at or before each query
    {
        Run<1> T, A, Q;
        Q.open(ts, Mq, 0, lane);
        if (No) { T.open(t, No, 0, lane); A.open(alpha, No, 0, lane); }
        double F = 0.0, last = 0.0;
        int64_t n = 0;
        double tn = No ? T.get(0, lane) : 0.0;
        #pragma unroll 1
        for (int64_t m = 0; m < Mq; ++m) {
            const double tm = Q.get(m, lane);
            #pragma unroll 1
            while (n < No && tn <= tm) {
                const double an = A.get(n, lane);
                double u, v;
                gen_row(q, tn, u, v);
                const double p = exp(q.c * ((n ? last : tn) - tn));
                F = fma(v, an, p * F);
                last = tn;
                if (++n < No) tn = T.get(n, lane);
            }
            double lo = 0.0;
            if (n) {                                  // (no observed row yet: nothing below this query)
                double u, v;
                gen_row(q, tm, u, v);
                lo = wsum((u * exp(q.c * (last - tm))) * F);
            }
            const int slot = (int)(m & 63);
            if (lane == slot) buf = lo;
            if (slot == 63 || m == Mq - 1) {
                const int64_t i = (m - slot) + lane;
                if (i <= m) mu[i] = buf;
            }
        }
    }

    // ---- backward: the observed rows beyond each query, added to what the forward pass left
    {
        Run<-1> T, A, Q;
        Q.open(ts, Mq, Mq - 1, lane);
        if (No) { T.open(t, No, No - 1, lane); A.open(alpha, No, No - 1, lane); }
        double H = 0.0, last = 0.0;
        int64_t n = No - 1;
        double tn = No ? T.get(n, lane) : 0.0;
        #pragma unroll 1
        for (int64_t m = Mq - 1; m >= 0; --m) {
            const double tm = Q.get(m, lane);
            #pragma unroll 1
            while (n >= 0 && tn > tm) {
                const double an = A.get(n, lane);
                double u, v;
                gen_row(q, tn, u, v);
                const double p = exp(q.c * (tn - (n == No - 1 ? tn : last)));
                H = fma(u, an, p * H);
                last = tn;
                if (--n >= 0) tn = T.get(n, lane);
            }
            double up = 0.0;
            if (n < No - 1) {
                double u, v;
                gen_row(q, tm, u, v);
                up = wsum((v * exp(q.c * (tm - last))) * H);
            }
            const int slot = (int)(m & 63);
            if (slot == 63 || m == Mq - 1) {
                const int64_t i = (m - slot) + lane;
                buf = i <= m ? mu[i] : 0.0;
            }
            if (lane == slot) buf = buf + up;
            if (slot == 0) {
                const int64_t i = m + lane;
                if (i < Mq) mu[i] = buf;
            }
        }
    }
}

}  // namespace

extern "C" {

int gf_predict_batch_at(int B, int64_t N, int64_t M, int Jr, int Jc,
                        const double *ar, const double *cr, const double *ac,
                        const double *bc, const double *cc, const double *dc,
                        const double *t, int64_t t_bs, const int64_t *nobs,
                        const double *ts, int64_t ts_bs, const int64_t *nq,
                        const double *alpha, int64_t alpha_bs,
                        double *mu, int64_t mu_bs, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || M < 1 || Jr < 0 || Jc < 0 || W < 1)
        return gf_internal_error(-1, "gf_predict_batch_at: bad shape (B=%d, N=%lld, M=%lld, Jr=%d, Jc=%d)", B,
                                 (long long)N, (long long)M, Jr, Jc);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_predict_batch_at: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !t || !ts || !alpha || !mu)
        return gf_internal_error(-1, "gf_predict_batch_at: null pointer");
    if (t_bs < 0 || ts_bs < 0 || (B > 1 && (alpha_bs < N || mu_bs < M)))
        return gf_internal_error(-1, "gf_predict_batch_at: bad stride (t_bs=%lld, ts_bs=%lld, alpha_bs=%lld < N=%lld "
                                 "or mu_bs=%lld < M=%lld)", (long long)t_bs, (long long)ts_bs, (long long)alpha_bs,
                                 (long long)N, (long long)mu_bs, (long long)M);
    hipLaunchKernelGGL(k_predict_at, dim3((unsigned)B), dim3(ROW_LANES), 0, (hipStream_t)stream, N, M, Jr, Jc, ar, cr,
                       ac, bc, cc, dc, t, t_bs, nobs, ts, ts_bs, nq, alpha, alpha_bs, mu, mu_bs);
    return gf_internal_check_launch("gf_predict_batch_at");
}

}  // extern "C"
