// gadfly_var.hip -- conditional variances of B problems in one call
//
// celerite2's counterpart: the second half of GaussianProcess.predict(y, t, return_var=True)
// (ConditionalDistribution.variance: one right-hand side per query through the stored factor).  Here every variance of
// a problem comes from one more backward recurrence over the rows gf_solve_batch stages anyway, no stored factor.
// With Sigma = K + diag = L D L^T and the forward rows S_n, D_n, W_n, U_n, P_n of gadfly_solve.hip,
//     h_n = (Sigma^-1)_nn = 1 / D_n + W_n^T Z_n W_n,       Z_n = P_{n+1} Y_{n+1} P_{n+1}    (0 at the last row)
//     q = Z_n W_n,  r = h_n U_n / 2 - q,                   Y_n = Z_n + U_n r^T + r U_n^T     (symmetric rank two)
//     var_n = diag_n - diag_n^2 h_n                        (K(0) - K_n Sigma^-1 K_n^T, exactly 0 where diag_n = 0)
// and at a new time t* owned by row n (t_n <= t* < t_{n+1}; the tie rule of gf_general_matmul's lower part), with
// p* = e^{-c (t* - t_n)} and the generator row (U*, V*) at t*,
//     f* = (p* p*^T o (S_n + D_n W_n W_n^T)) U*,   d* = K(0) - U*^T f*,   R* = V* - f*      (forward, at the owner)
//     x = e^{-c (t_{n+1} - t*)} o R*,              var* = d* - x^T Y_{n+1} x            (backward, once Y is Y_{n+1})
// (before the first row f* = 0, after the last one var* = d*; K(0) is the diag_add argument, sum a + the exposure
// shift, what gf_solve_batch puts on the diagonal).
// One wave per problem, lane j owning column j of S and row j of Y, gf_solve_batch's structure:
//   pass 1   gadfly_solve.hip's pass 1; after each row the sorted queries the row owns are staged, R* per lane in the
//            workspace and d* in var_at itself (the queries before t_0 first);
//   pass 2   per segment, last first: Y is parked in its workspace slot, the rows are recomputed from the checkpoint
//            staging (W_n, U_n, P_n), Y comes back into the registers that held S, and the backward loop carries the
//            vector H (alpha, mu) and the matrix Y: two LDS broadcast loops per row (q = Z W, then the rank-two
//            update) with one wave sum between them; the queries between row n - 1 and row n follow row n's update.
// S and Y are one register array: never live in the same loop.  fwd_row, Col, load_col, gen_row, wsum and the
// checkpoint layout are the ones gadfly_solve.hip runs (gf_rows.h): alpha, mu, log L and info have gf_solve_batch's bits.
// The recompute replays pass 1's arithmetic (explicitly fused operations, contraction off), Y travels through the
// workspace unrounded: every output is bit-identical whatever the segment length and the batch.  No atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"
#include "gf_rows.h"

#pragma clang fp contract(off)

namespace {

inline int64_t solve_pick_seg(int64_t N, int W, int64_t seg) {
    if (seg == 0) return gf_solve_batch_seg(N, W);            // (one segment rule for both kernels)
    return seg > N ? N : seg;
}

// gf_solve_batch's workspace (checkpoints, one segment's staged rows, z / alpha and D of every row), the slot Y is
// parked in while a segment is recomputed (a lane's row contiguous), R* of every query
inline int64_t var_work(int64_t N, int WM, int64_t K, int64_t M) {
    const int64_t nseg = (N + K - 1) / K;
    return nseg * solve_ck(WM) + K * solve_rs() + 2 * solve_n64(N) + (int64_t)WM * ROW_LANES + M * ROW_LANES;
}

// the virtual row at t* >= t_n behind row n, whose (S, w, D) come in and stay: its pivot d* (the filter variance at
// t*) and R* = V* - f* (its W times its pivot).  rows == false: no row before t*, f* = 0.
template <int WM>
__device__ __forceinline__ void query_row(const double (&S)[WM], double w, double D, const Col &q, bool rows,
                                          double tn, double tq, double k0, double *sh, int lane, double &R,
                                          double &d) {
    double u, v, f = 0.0;
    gen_row(q, tq, u, v);
    if (rows) {                                  // (wave-uniform)
        const double p = exp(q.c * (tn - tq));
        const double wi = D * w;
        sh[lane] = w;
        sh[ROW_LANES + lane] = p;
        sh[2 * ROW_LANES + lane] = u;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WM; ++k) {
            f = fma((p * sh[ROW_LANES + k]) * fma(wi, sh[k], S[k]), sh[2 * ROW_LANES + k], f);
            ROW_PACE(k);
        }
    }
    d = k0 - wsum(u * f);
    R = v - f;
}

template <int WM, bool QUERY>
__global__ __launch_bounds__(ROW_LANES) void k_var(
    int64_t N, int64_t M, int64_t K, int64_t nseg, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add,
    const double *__restrict__ t, int64_t t_bs, const double *__restrict__ dg, int64_t d_bs,
    const double *__restrict__ y, int64_t y_bs,
    const double *__restrict__ ts, int64_t ts_bs, const int64_t *__restrict__ nobs, const int64_t *__restrict__ nq,
    double *__restrict__ work, int64_t work_bs,
    double *alpha, double *mu, double *hdiag, double *var, double *var_at,
    double *__restrict__ ll, int32_t *__restrict__ info) {
    __shared__ double sh[2][3 * ROW_LANES];       // fwd_row's and the backward row's broadcasts (W, P, U), by row parity
    // pass 1: a query's broadcasts (W, p*, U*), by query parity; pass 2: [n & 1][0 .. 64) r of row n and
    // [m & 1][64 .. 128) x of query m
    __shared__ double sx[2][3 * ROW_LANES];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    t += (int64_t)b * t_bs;
    y += (int64_t)b * y_bs;
    if (dg) dg += (int64_t)b * d_bs;
    if (alpha) alpha += (int64_t)b * N;
    if (mu) mu += (int64_t)b * N;
    if (hdiag) hdiag += (int64_t)b * N;
    if (var) var += (int64_t)b * N;
    double *ck = work + (int64_t)b * work_bs;
    double *rows = ck + nseg * solve_ck(WM);
    double *zw = rows + K * solve_rs();            // z_n, then alpha_n
    double *Dw = zw + solve_n64(N);
    double *Yw = Dw + solve_n64(N);                // Y while a segment is recomputed
    double *Rw = Yw + (int64_t)WM * ROW_LANES;      // R* of every query
    const double dadd = diag_add[b];
    // (M = 0 without QUERY, a fact the compiler is not told: the backward loop keeps its query loop in both
    // instances, where it runs no iteration.  Without that inner loop the register allocator does not split the live
    // ranges around the two broadcast loops, and k_var<64, false> spills a dozen addresses to scratch.)
    const int64_t No = QUERY ? clamp_count(nobs, b, N) : N, Mq = clamp_count(nq, b, M);
    if (QUERY) {
        ts += (int64_t)b * ts_bs;
        var_at += (int64_t)b * M;
    }

    // ---- pass 1: log L, z and D of every row, the checkpoints; (R*, d*) of every query at its owner
    double S[WM];
#pragma unroll
    for (int k = 0; k < WM; ++k) S[k] = 0.0;
    double G = 0.0, w = 0.0, D = 0.0, z = 0.0, u, p;
    double logdet = 0.0, quad = 0.0, zbuf = 0.0, dbuf = 1.0;
    int64_t bad = 0, left = 0, seg = 0, m = 0;
    if (QUERY) {
        #pragma unroll 1
        while (m < Mq && (No == 0 || ts[m] < t[0])) {          // owned by no row: the prior
            double R, d;
            query_row<WM>(S, w, D, q, false, 0.0, ts[m], dadd, sx[m & 1], lane, R, d);
            Rw[m * ROW_LANES + lane] = R;
            if (lane == (int)(m & 63)) var_at[m] = d;
            ++m;
        }
    }
    #pragma unroll 1
    for (int64_t n = 0; n < N; ++n) {
        if (left == 0) {
            ck_store<WM>(ck + seg * solve_ck(WM), lane, S, G, w, D, z);
            left = K;
            ++seg;
        }
        --left;
        const double tn = t[n], tp = n ? t[n - 1] : tn;
        const double An = (dg ? dg[n] : 0.0) + dadd;
        fwd_row<WM>(S, G, w, D, z, q, tp, tn, An, y[n], sh[n & 1], lane, u, p);
        if (!(D > 0.0)) { bad = n + 1; break; }
        logdet += log(D);
        quad += z * z / D;
        const int slot = (int)(n & 63);
        if (lane == slot) { zbuf = z; dbuf = D; }
        if (slot == 63 || n == N - 1) {
            const int64_t i = (n - slot) + lane;
            if (i <= n) { zw[i] = zbuf; Dw[i] = dbuf; }
        }
        if (QUERY) {
            #pragma unroll 1
            while (m < Mq && n < No && (n + 1 >= No || ts[m] < t[n + 1])) {      // t_n <= t* < t_{n+1}
                double R, d;
                query_row<WM>(S, w, D, q, true, tn, ts[m], dadd, sx[m & 1], lane, R, d);
                Rw[m * ROW_LANES + lane] = R;
                if (lane == (int)(m & 63)) var_at[m] = d;
                ++m;
            }
        }
    }
    if (bad) {
        const double nan = __builtin_nan("");
        if (lane == 0) { ll[b] = -INFINITY; info[b] = (int32_t)bad; }
        for (int64_t i = lane; i < N; i += ROW_LANES) {
            if (alpha) alpha[i] = nan;
            if (mu) mu[i] = nan;
            if (hdiag) hdiag[i] = nan;
            if (var) var[i] = nan;
        }
        if (QUERY)
            for (int64_t i = lane; i < Mq; i += ROW_LANES) var_at[i] = nan;
        return;
    }
    if (lane == 0) {
        ll[b] = -0.5 * (logdet + quad + (double)N * log(6.283185307179586));
        info[b] = 0;
    }

    // ---- pass 2: segments last first, each recomputed from its checkpoint, then the upper solve and the Y
    // recurrence over its rows
    double (&Y)[WM] = S;                         // one register array: S while a segment is recomputed, Y after it
#pragma unroll
    for (int k = 0; k < WM; ++k) Y[k] = 0.0;
    double H = 0.0, unext = 0.0, pnext = 0.0, anext = 0.0;       // (U, P, alpha of row n + 1: nothing beyond the end)
    double abuf = 0.0, hbuf = 0.0;
    int64_t mq = Mq - 1;
    if (QUERY) {
        #pragma unroll 1
        while (mq >= 0 && (No == 0 || ts[mq] >= t[No - 1])) --mq;      // owned by the last row: var* = d*
    }
    #pragma unroll 1
    for (int64_t s = nseg - 1; s >= 0; --s) {
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        const double *c = ck + s * solve_ck(WM);
#pragma unroll
        for (int k = 0; k < WM; ++k) Yw[lane * WM + k] = Y[k];
        __builtin_amdgcn_sched_barrier(0);       // (Y is out before S comes in: the two never share the registers)
#pragma unroll
        for (int k = 0; k < WM; ++k) S[k] = c[lane * WM + k];
        G = c[(WM + 0) * ROW_LANES + lane];
        w = c[(WM + 1) * ROW_LANES + lane];
        D = c[(WM + 2) * ROW_LANES + lane];
        z = c[(WM + 3) * ROW_LANES + lane];
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            const double tn = t[n], tp = n ? t[n - 1] : tn;
            const double An = (dg ? dg[n] : 0.0) + dadd;
            fwd_row<WM>(S, G, w, D, z, q, tp, tn, An, y[n], sh[n & 1], lane, u, p);
            double *r = rows + (n - n0) * solve_rs();
            r[lane] = w;
            r[ROW_LANES + lane] = u;
            r[2 * ROW_LANES + lane] = p;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < WM; ++k) Y[k] = Yw[lane * WM + k];
        __syncthreads();                 // (the recompute's last broadcasts are read before the next are written)
        #pragma unroll 1
        for (int64_t n = n1 - 1; n >= n0; --n) {
            const double *r = rows + (n - n0) * solve_rs();
            const double wn = r[lane], un = r[ROW_LANES + lane], pn = r[2 * ROW_LANES + lane];
            const int slot = (int)(n & 63);
            if (slot == 63 || n == N - 1) {
                const int64_t i = (n - slot) + lane;
                zbuf = i <= n ? zw[i] : 0.0;
                dbuf = i <= n ? Dw[i] : 1.0;
            }
            const double zn = read_lane(zbuf, slot), Dn = read_lane(dbuf, slot);
            H = pnext * fma(unext, anext, H);
            const double a = zn / Dn - wsum(wn * H);
            // Z = P_{n+1} Y P_{n+1} in place, q = Z W_n
            double *bw = sh[n & 1], *br = sx[n & 1];
            bw[lane] = wn;
            bw[ROW_LANES + lane] = pnext;
            bw[2 * ROW_LANES + lane] = un;
            __syncthreads();
            double qv = 0.0;
#pragma unroll
            for (int k = 0; k < WM; ++k) {
                const double zk = (pnext * bw[ROW_LANES + k]) * Y[k];
                Y[k] = zk;
                qv = fma(zk, bw[k], qv);
                ROW_PACE(k);
            }
            const double h = 1.0 / Dn + wsum(wn * qv);
            const double rv = fma(0.5 * h, un, -qv);
            br[lane] = rv;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < WM; ++k) {
                Y[k] = fma(un, br[k], fma(rv, bw[2 * ROW_LANES + k], Y[k]));
                ROW_PACE(k);
            }
            unext = un; pnext = pn; anext = a;
            if (lane == slot) { abuf = a; hbuf = h; }
            {
                // Y is Y_n: the queries between row n - 1 and row n (before row 0: all that are left)
                const double tn = t[n];
                #pragma unroll 1
                while (mq >= 0 && (n == 0 || ts[mq] >= t[n - 1])) {
                    double *bx = sx[mq & 1] + ROW_LANES;
                    const double x = exp(q.c * (ts[mq] - tn)) * Rw[mq * ROW_LANES + lane];
                    bx[lane] = x;
                    __syncthreads();
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < WM; ++k) {
                        acc = fma(Y[k], bx[k], acc);
                        ROW_PACE(k);
                    }
                    const double quadq = wsum(x * acc);
                    if (lane == (int)(mq & 63)) var_at[mq] = var_at[mq] - quadq;     // (d*: this lane's own write)
                    --mq;
                }
            }
            if (slot == 0) {
                const int64_t i = n + lane;
                if (i < N) {
                    stage_alpha(i, abuf, zw, alpha, mu, dg, y);
                    if (hdiag) hdiag[i] = hbuf;
                    if (var) {
                        const double di = dg ? dg[i] : 0.0;
                        var[i] = di * fma(-di, hbuf, 1.0);        // diag - diag^2 h, no overflow on a missing-data row
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int64_t gf_var_batch_work(int64_t N, int W, int64_t M, int64_t seg) {
    if (!row_shape_ok(N, W) || M < 0 || seg < 0) return 0;
    const int WM = row_wm(W);
    return var_work(N, WM, solve_pick_seg(N, W, seg), M);
}

int gf_var_batch(int B, int64_t N, int Jr, int Jc,
                 const double *ar, const double *cr, const double *ac, const double *bc,
                 const double *cc, const double *dc, const double *diag_add,
                 const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                 const double *y, int64_t y_bs,
                 const double *ts, int64_t ts_bs, int64_t M, const int64_t *nobs, const int64_t *nq,
                 int64_t seg, double *work, int64_t work_bs,
                 double *alpha, double *mu, double *hdiag, double *var, double *var_at,
                 double *ll, int32_t *info, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || M < 0 || Jr < 0 || Jc < 0 || W < 1 || seg < 0)
        return gf_internal_error(-1, "gf_var_batch: bad shape (B=%d, N=%lld, M=%lld, Jr=%d, Jc=%d, seg=%lld)", B,
                                 (long long)N, (long long)M, Jr, Jc, (long long)seg);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_var_batch: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    if ((M > 0) != (var_at != nullptr) || (M > 0 && !ts))
        return gf_internal_error(-1, "gf_var_batch: ts and var_at go with M=%lld > 0 queries", (long long)M);
    if (t_bs < 0 || diag_bs < 0 || y_bs < 0 || ts_bs < 0)
        return gf_internal_error(-1, "gf_var_batch: negative stride");
    const int WM = row_wm(W);
    const int64_t K = solve_pick_seg(N, W, seg), nseg = (N + K - 1) / K;
    if (work_bs < var_work(N, WM, K, M))
        return gf_internal_error(-1, "gf_var_batch: work_bs=%lld < gf_var_batch_work(N, W, M, seg)=%lld",
                                 (long long)work_bs, (long long)var_work(N, WM, K, M));
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !work || !ll || !info)
        return gf_internal_error(-1, "gf_var_batch: null pointer");
    hipStream_t st = (hipStream_t)stream;
#define VR_LAUNCH(WMV, QV)                                                                                         \
    hipLaunchKernelGGL((k_var<WMV, QV>), dim3((unsigned)B), dim3(ROW_LANES), 0, st, N, M, K, nseg, Jr, Jc, ar, cr,  \
                       ac, bc, cc, dc, diag_add, t, t_bs, diag, diag_bs, y, y_bs, ts, ts_bs, nobs, nq, work,       \
                       work_bs, alpha, mu, hdiag, var, var_at, ll, info)
    if (M > 0) {
        if (WM == 16) VR_LAUNCH(16, true);
        else if (WM == 32) VR_LAUNCH(32, true);
        else VR_LAUNCH(64, true);
    } else {
        if (WM == 16) VR_LAUNCH(16, false);
        else if (WM == 32) VR_LAUNCH(32, false);
        else VR_LAUNCH(64, false);
    }
#undef VR_LAUNCH
    return gf_internal_check_launch("gf_var_batch");
}

}  // extern "C"
