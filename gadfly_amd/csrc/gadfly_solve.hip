// gadfly_solve.hip -- alpha = K^-1 y and the conditional means of B problems in one call
//
// celerite2's counterpart: driver.factor + solve_lower + solve_upper (GaussianProcess.apply_inverse) and, for the
// share of the data one part of the kernel explains, general_matmul_lower + general_matmul_upper at t* = t
// (GaussianProcess.predict(y, kernel=component)).  The forward recurrence is gadfly_grad.hip's (the plain, unscaled
// one of oracle/celerite_ref.c with exact generator rows, theta_n = fl(d t_n)):
//     S_n = P_n (S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T) P_n     f_n = S_n U_n     D_n = A_n - U_n^T f_n
//     W_n = (V_n - f_n) / D_n      G_n = P_n (G_{n-1} + W_{n-1} z_{n-1})      z_n = y_n - U_n^T G_n
// The upper solve runs the other way and needs W_n, which needs S_n: checkpointed recompute, one wave per problem,
// lane j owning column j.
//   pass 1   forward: log L, z_n and D_n of every row, the state (S, G, W, D, z) entering every K-th row;
//   pass 2   per segment of K rows, last first: recompute the rows from the checkpoint staging (W_n, U_n, P_n), three
//            values per lane and row, then
//                H_n = P_{n+1} (H_{n+1} + U_{n+1} alpha_{n+1})      alpha_n = z_n / D_n - W_n^T H_n
//            and mu_n = y_n - diag_n alpha_n; with a component (U', V', P'): H'_n likewise, up'_n = V'_n^T H'_n;
//   pass 3   (component only) forward over the finished alpha: F'_n = P'_n F'_{n-1} + V'_n alpha_n,
//            mu'_n = U'_n^T F'_n + up'_n.
// Per-row scalars (z, D, alpha, mu, mu') live in lane n mod 64 between rows and move 64 rows at a time: every load
// and store of the wave is one contiguous 512-byte run, and a lane reads back only what it wrote itself.
// The recompute replays pass 1's arithmetic (one set of explicitly fused operations, contraction off), so every
// output is bit-identical whatever the segment length and whatever the batch around a problem.  No atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"
#include "gf_rows.h"

#pragma clang fp contract(off)

namespace {

// rows per segment that balance nseg checkpoints against K staged rows: the smallest K with 3 K^2 >= N (WM + 4)
inline int64_t solve_seg(int64_t N, int WM) {
    const unsigned __int128 want = (unsigned __int128)N * (unsigned)(WM + 4);
    int64_t K = (int64_t)sqrt((double)N * (double)(WM + 4) / 3.0);
    if (K < 1) K = 1;
    while ((unsigned __int128)K * K * 3 < want) ++K;
    while (K > 1 && (unsigned __int128)(K - 1) * (K - 1) * 3 >= want) --K;
    return K > N ? N : K;
}

inline int64_t solve_pick_seg(int64_t N, int WM, int64_t seg) {
    if (seg == 0) return solve_seg(N, WM);
    return seg > N ? N : seg;
}

// checkpoints, one segment's staged rows, z (alpha after pass 2) and D of every row
inline int64_t solve_work(int64_t N, int WM, int64_t K) {
    const int64_t nseg = (N + K - 1) / K;
    return nseg * solve_ck(WM) + K * solve_rs() + 2 * solve_n64(N);
}

template <int WM, bool COMP>
__global__ __launch_bounds__(ROW_LANES) void k_solve(
    int64_t N, int64_t K, int64_t nseg, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add, int Jr2, int Jc2,
    const double *__restrict__ ar2, const double *__restrict__ cr2, const double *__restrict__ ac2,
    const double *__restrict__ bc2, const double *__restrict__ cc2, const double *__restrict__ dc2,
    const double *__restrict__ t, int64_t t_bs, const double *__restrict__ dg, int64_t d_bs,
    const double *__restrict__ y, int64_t y_bs, double *__restrict__ work, int64_t work_bs,
    double *alpha, double *mu, double *mu_comp, double *__restrict__ ll, int32_t *__restrict__ info) {
    __shared__ double sh[2][3 * ROW_LANES];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const Col q = load_col(b, lane, Jr, Jc, ar, cr, ac, bc, cc, dc);
    t += (int64_t)b * t_bs;
    y += (int64_t)b * y_bs;
    if (dg) dg += (int64_t)b * d_bs;
    if (alpha) alpha += (int64_t)b * N;
    if (mu) mu += (int64_t)b * N;
    if (COMP) mu_comp += (int64_t)b * N;
    double *ck = work + (int64_t)b * work_bs;
    double *rows = ck + nseg * solve_ck(WM);
    double *zw = rows + K * solve_rs();            // z_n, then alpha_n
    double *Dw = zw + solve_n64(N);
    const double dadd = diag_add[b];

    // ---- pass 1: log L, z and D of every row, the checkpoints
    double S[WM];
#pragma unroll
    for (int k = 0; k < WM; ++k) S[k] = 0.0;
    double G = 0.0, w = 0.0, D = 0.0, z = 0.0, u, p;
    double logdet = 0.0, quad = 0.0, zbuf = 0.0, dbuf = 1.0;
    int64_t bad = 0, left = 0, seg = 0;
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
    }
    if (bad) {
        const double nan = __builtin_nan("");
        if (lane == 0) { ll[b] = -INFINITY; info[b] = (int32_t)bad; }
        for (int64_t i = lane; i < N; i += ROW_LANES) {
            if (alpha) alpha[i] = nan;
            if (mu) mu[i] = nan;
            if (COMP) mu_comp[i] = nan;
        }
        return;
    }
    if (lane == 0) {
        ll[b] = -0.5 * (logdet + quad + (double)N * log(6.283185307179586));
        info[b] = 0;
    }

    // ---- pass 2: segments last first, each recomputed from its checkpoint, then the upper solve over its rows
    Col q2{0.0, 0.0, 0.0, 0.0, 0, 0};
    if (COMP) q2 = load_col(b, lane, Jr2, Jc2, ar2, cr2, ac2, bc2, cc2, dc2);
    double H = 0.0, unext = 0.0, pnext = 0.0, anext = 0.0;       // (U, P, alpha of row n + 1: nothing beyond the end)
    double H2 = 0.0, u2next = 0.0, tnext = t[N - 1];
    double abuf = 0.0, ubuf = 0.0;
    #pragma unroll 1
    for (int64_t s = nseg - 1; s >= 0; --s) {
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        const double *c = ck + s * solve_ck(WM);
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
            if (COMP) {
                const double tn = t[n];
                const double p2 = exp(q2.c * (tn - tnext));
                H2 = p2 * fma(u2next, anext, H2);
                double u2, v2;
                gen_row(q2, tn, u2, v2);
                const double up = wsum(v2 * H2);
                u2next = u2;
                tnext = tn;
                if (lane == slot) ubuf = up;
            }
            unext = un; pnext = pn; anext = a;
            if (lane == slot) abuf = a;
            if (slot == 0) {
                const int64_t i = n + lane;
                if (i < N) {
                    stage_alpha(i, abuf, zw, alpha, mu, dg, y);
                    if (COMP) mu_comp[i] = ubuf;
                }
            }
        }
    }

    // ---- pass 3: the component's lower part over the finished alpha
    if (COMP) {
        double F = 0.0, tprev = t[0];
        #pragma unroll 1
        for (int64_t n = 0; n < N; ++n) {
            const int slot = (int)(n & 63);
            if (slot == 0) {
                const int64_t i = n + lane;
                abuf = i < N ? zw[i] : 0.0;
                ubuf = i < N ? mu_comp[i] : 0.0;
            }
            const double tn = t[n];
            const double p2 = exp(q2.c * (tprev - tn));
            double u2, v2;
            gen_row(q2, tn, u2, v2);
            F = fma(v2, read_lane(abuf, slot), p2 * F);
            const double lo = wsum(u2 * F);
            if (lane == slot) ubuf = lo + ubuf;
            if (slot == 63 || n == N - 1) {
                const int64_t i = (n - slot) + lane;
                if (i <= n) mu_comp[i] = ubuf;
            }
            tprev = tn;
        }
    }
}

}  // namespace

extern "C" {

int64_t gf_solve_batch_seg(int64_t N, int W) {
    if (!row_shape_ok(N, W)) return 0;
    return solve_seg(N, row_wm(W));
}

int64_t gf_solve_batch_work(int64_t N, int W, int64_t seg) {
    if (!row_shape_ok(N, W) || seg < 0) return 0;
    const int WM = row_wm(W);
    return solve_work(N, WM, solve_pick_seg(N, WM, seg));
}

int gf_solve_batch(int B, int64_t N, int Jr, int Jc,
                   const double *ar, const double *cr, const double *ac, const double *bc,
                   const double *cc, const double *dc, const double *diag_add,
                   int Jr2, int Jc2,
                   const double *ar2, const double *cr2, const double *ac2, const double *bc2,
                   const double *cc2, const double *dc2,
                   const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                   const double *y, int64_t y_bs, int64_t seg, double *work, int64_t work_bs,
                   double *alpha, double *mu, double *mu_comp, double *ll, int32_t *info, void *stream) {
    const int W = Jr + 2 * Jc, W2 = Jr2 + 2 * Jc2;
    if (B < 1 || N < 1 || Jr < 0 || Jc < 0 || W < 1 || Jr2 < 0 || Jc2 < 0 || seg < 0)
        return gf_internal_error(-1, "gf_solve_batch: bad shape (B=%d, N=%lld, Jr=%d, Jc=%d, Jr'=%d, Jc'=%d, seg=%lld)",
                                 B, (long long)N, Jr, Jc, Jr2, Jc2, (long long)seg);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_solve_batch: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    if (W2 > ROW_MAX_W)
        return gf_internal_error(-3, "gf_solve_batch: component width W'=%d exceeds the one-wave limit %d", W2,
                                 ROW_MAX_W);
    const bool comp = mu_comp != nullptr;
    if (comp != (W2 > 0))
        return gf_internal_error(-1, "gf_solve_batch: mu_comp and a component (W'=%d) go together", W2);
    const int WM = row_wm(W);
    const int64_t K = solve_pick_seg(N, WM, seg), nseg = (N + K - 1) / K;
    if (work_bs < solve_work(N, WM, K))
        return gf_internal_error(-1, "gf_solve_batch: work_bs=%lld < gf_solve_batch_work(N, W, seg)=%lld",
                                 (long long)work_bs, (long long)solve_work(N, WM, K));
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || (Jr2 && (!ar2 || !cr2)) ||
        (Jc2 && (!ac2 || !bc2 || !cc2 || !dc2)) || !diag_add || !t || !y || !work || !ll || !info)
        return gf_internal_error(-1, "gf_solve_batch: null pointer");
    hipStream_t st = (hipStream_t)stream;
#define SV_LAUNCH(WMV, CV)                                                                                        \
    hipLaunchKernelGGL((k_solve<WMV, CV>), dim3((unsigned)B), dim3(ROW_LANES), 0, st, N, K, nseg, Jr, Jc, ar, cr,  \
                       ac, bc, cc, dc, diag_add, Jr2, Jc2, ar2, cr2, ac2, bc2, cc2, dc2, t, t_bs, diag, diag_bs, \
                       y, y_bs, work, work_bs, alpha, mu, mu_comp, ll, info)
    if (comp) {
        if (WM == 16) SV_LAUNCH(16, true);
        else if (WM == 32) SV_LAUNCH(32, true);
        else SV_LAUNCH(64, true);
    } else {
        if (WM == 16) SV_LAUNCH(16, false);
        else if (WM == 32) SV_LAUNCH(32, false);
        else SV_LAUNCH(64, false);
    }
#undef SV_LAUNCH
    return gf_internal_check_launch("gf_solve_batch");
}

}  // extern "C"
