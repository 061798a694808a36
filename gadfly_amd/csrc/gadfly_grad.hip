// gadfly_grad.hip -- reverse-mode gradient of the celerite log-likelihood of B problems
//
// celerite2's counterpart: driver.factor_rev + driver.solve_lower_rev and the norm's adjoint (the ops its JAX and
// PyMC interfaces differentiate through).  The forward recurrence is the plain, unscaled one of
// oracle/celerite_ref.c (ref_get_matrices, ref_factor, ref_solve_lower) with exact generator rows at every row
// (theta_n = fl(d t_n), the rounded product celerite2 takes cos / sin of):
//     M_n = S_{n-1} + D_{n-1} W_{n-1} W_{n-1}^T      S_n = P_n M_n P_n        (P_n = diag exp(-c dt_n))
//     f_n = S_n U_n     D_n = A_n - U_n^T f_n      W_n = (V_n - f_n) / D_n
//     G_n = P_n (G_{n-1} + W_{n-1} z_{n-1})          z_n = y_n - U_n^T G_n
//     log L = -1/2 sum z_n^2 / D_n - 1/2 sum log D_n - N/2 log 2 pi
// The reverse step carries the adjoints of M (W x W, kept symmetric) and of G_{n-1} + W_{n-1} z_{n-1} (W)
// backwards; it needs S_n itself at every row (the mat-vec S_n fbar feeding Ubar, and sum_k Sbar[j,k] S[j,k]
// feeding cbar), which cannot be had by running the recurrence backwards (P^-1 explodes for fast terms).
// Checkpointed recompute, one wave per problem, lane j owning row j of S (registers) and of Sbar (LDS):
//   pass 1    the forward sweep: log L, and the state entering every K-th row (S, G, W, D, z) to the workspace;
//   reverse   per segment of K rows, last first: recompute the rows forward from the segment's checkpoint,
//             staging each row's S and vectors in the workspace, then run the reverse step over them.
// K = ceil(sqrt(N)) balances the checkpoints against the segment's rows.  No atomics: every sum has one fixed
// association (butterfly reductions across the wave, per-lane accumulation in row order), and a problem's
// arithmetic depends on its own data and N alone, so results are bit-identical whatever the batch around it.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_rows.h"

namespace {

// rows per segment: the smallest K with K^2 >= N
inline int64_t grad_seg(int64_t N) {
    int64_t K = (int64_t)sqrt((double)N);
    while (K * K < N) ++K;
    while (K > 1 && (K - 1) * (K - 1) >= N) --K;
    return K < 1 ? 1 : K;
}

// doubles per checkpoint (S rows, G, W, D, z; a lane's row of S contiguous) and per staged row (S, G, W, f, U, V, p,
// D, z; S column-major, element (j, k) at k * 64 + j, so that every load and store of the wave is one contiguous
// 512-byte run), the vectors one element per lane
__host__ __device__ inline int64_t grad_ck(int WM) { return (int64_t)(WM + 4) * ROW_LANES; }
__host__ __device__ inline int64_t grad_rs(int WM) { return (int64_t)(WM + 8) * ROW_LANES; }

inline int64_t grad_work(int64_t N, int W) {
    const int WM = row_wm(W);
    const int64_t K = grad_seg(N), nseg = (N + K - 1) / K;
    return nseg * grad_ck(WM) + K * grad_rs(WM);
}

// every 8 columns of the forward row and of the reverse step's contraction with Sbar: keeps the scheduler from
// hoisting all of a row's LDS reads (three W-vectors of broadcasts, or Sbar) ahead of their FMAs.  Only LDS reads sit
// in those loops; the reverse step's staged S is loaded whole before them (one memory wait per row).
#define GR_PACE(k) do { if (((k) & 7) == 7) __builtin_amdgcn_sched_barrier(0); } while (0)

// gf_rows.h's gen_row and fwd_row with plain products and sums (this unit contracts them; no explicit fma) and with
// f and v as further outputs: separate on purpose, sharing them would change this kernel's bits
__device__ __forceinline__ void grad_gen_row(const Col &q, double tn, double &u, double &v) {
    if (q.kind == 2) {
        double s, co;
        sincos(q.d * tn, &s, &co);        // theta = fl(d t), as celerite2
        if (q.half == 0) { u = q.a * co + q.b * s; v = co; }
        else             { u = q.a * s - q.b * co; v = s; }
    } else if (q.kind == 1) {
        u = q.a; v = 1.0;
    } else {
        u = 0.0; v = 0.0;
    }
}

// one forward row: (S, G, w, D, z) of row n-1 in, of row n out; f, u, v, p of row n out
template <int WM>
__device__ __forceinline__ void grad_fwd_row(double (&S)[WM], double &G, double &w, double &D, double &z,
                                             const Col &q, double tprev, double tn, double An, double yn,
                                             double *sh, int lane, double &f, double &u, double &v, double &p) {
    grad_gen_row(q, tn, u, v);
    p = exp(q.c * (tprev - tn));
    const double wi = D * w;
    sh[lane] = w;
    sh[ROW_LANES + lane] = p;
    sh[2 * ROW_LANES + lane] = u;
    __syncthreads();
    f = 0.0;
#pragma unroll
    for (int k = 0; k < WM; ++k) {
        const double s = (p * sh[ROW_LANES + k]) * (S[k] + wi * sh[k]);
        S[k] = s;
        f += s * sh[2 * ROW_LANES + k];
        GR_PACE(k);
    }
    G = p * (G + w * z);
    const double uf = wsum(u * f), ug = wsum(u * G);
    D = An - uf;
    z = yn - ug;
    w = (v - f) / D;
}

template <int WM>
__global__ __launch_bounds__(ROW_LANES) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_grad(
    int64_t N, int64_t K, int64_t nseg, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add, const double *__restrict__ t, int64_t t_bs,
    const double *__restrict__ dg, int64_t d_bs, const double *__restrict__ y, int64_t y_bs,
    double *__restrict__ work, int64_t work_bs, double *__restrict__ ll, double *__restrict__ g_real,
    double *__restrict__ g_comp, double *__restrict__ g_diag, double *__restrict__ g_mean,
    int32_t *__restrict__ info) {
    __shared__ double sh[2][4 * ROW_LANES];
    __shared__ double Sb[WM * ROW_LANES];           // Sbar, element (j, k) at k * 64 + j: lane j's row, conflict-free
    const int B = (int)gridDim.x, b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int lr = Jr > 0 ? Jr : 1, lc = Jc > 0 ? Jc : 1, W = Jr + 2 * Jc;
    Col q{0.0, 0.0, 0.0, 0.0, 0, 0};
    int term = -1;
    if (lane < Jr) {
        term = lane;
        q.kind = 1; q.a = ar[(int64_t)b * lr + lane]; q.c = cr[(int64_t)b * lr + lane];
    } else if (lane < W) {
        term = (lane - Jr) >> 1;
        const int64_t o = (int64_t)b * lc + term;
        q.kind = 2; q.half = (lane - Jr) & 1;
        q.a = ac[o]; q.b = bc[o]; q.c = cc[o]; q.d = dc[o];
    }
    const int partner = q.kind == 2 ? (q.half ? lane - 1 : lane + 1) : lane;
    t += (int64_t)b * t_bs;
    y += (int64_t)b * y_bs;
    if (dg) dg += (int64_t)b * d_bs;
    double *ck = work + (int64_t)b * work_bs;
    double *rows = ck + nseg * grad_ck(WM);
    const double dadd = diag_add[b];
    const double t0 = t[0];

    // ---- pass 1: log L and the checkpoints
    double S[WM];
#pragma unroll
    for (int k = 0; k < WM; ++k) S[k] = 0.0;
    double G = 0.0, w = 0.0, D = 0.0, z = 0.0, f, u, v, p;
    double logdet = 0.0, quad = 0.0;
    int64_t bad = 0;
    #pragma unroll 1
    for (int64_t n = 0; n < N; ++n) {
        if (n % K == 0) {
            double *c = ck + (n / K) * grad_ck(WM);
#pragma unroll
            for (int k = 0; k < WM; ++k) c[lane * WM + k] = S[k];
            c[(WM + 0) * ROW_LANES + lane] = G;
            c[(WM + 1) * ROW_LANES + lane] = w;
            c[(WM + 2) * ROW_LANES + lane] = D;
            c[(WM + 3) * ROW_LANES + lane] = z;
        }
        const double tn = t[n], tp = n ? t[n - 1] : tn;
        const double An = (dg ? dg[n] : 0.0) + dadd;
        grad_fwd_row<WM>(S, G, w, D, z, q, tp, tn, An, y[n], sh[n & 1], lane, f, u, v, p);
        if (!(D > 0.0)) { bad = n + 1; break; }
        logdet += log(D);
        quad += z * z / D;
    }
    if (bad) {
        const double nan = __builtin_nan("");
        if (lane == 0) { ll[b] = -INFINITY; info[b] = (int32_t)bad; g_diag[b] = nan; g_mean[b] = nan; }
        if (q.kind == 1) {
            g_real[(int64_t)b * lr + term] = nan;
            g_real[(int64_t)B * lr + (int64_t)b * lr + term] = nan;
        } else if (q.kind == 2 && q.half == 0) {
            for (int r = 0; r < 4; ++r) g_comp[(int64_t)r * B * lc + (int64_t)b * lc + term] = nan;
        }
        return;
    }

    // ---- reverse: segments last first, each recomputed from its checkpoint and staged row by row
#pragma unroll
    for (int k = 0; k < WM; ++k) Sb[k * ROW_LANES + lane] = 0.0;
    double Hb = 0.0;                                   // adjoint of G_{n} + W_{n} z_{n}, i.e. of P^-1 G_{n+1}
    double ga = 0.0, gb = 0.0, gc = 0.0, gtht = 0.0, gA = 0.0, gy = 0.0;
    #pragma unroll 1
    for (int64_t s = nseg - 1; s >= 0; --s) {
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        const double *c = ck + s * grad_ck(WM);
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
            grad_fwd_row<WM>(S, G, w, D, z, q, tp, tn, An, y[n], sh[n & 1], lane, f, u, v, p);
            double *r = rows + (n - n0) * grad_rs(WM);
#pragma unroll
            for (int k = 0; k < WM; ++k) r[k * ROW_LANES + lane] = S[k];
            r[(WM + 0) * ROW_LANES + lane] = G;
            r[(WM + 1) * ROW_LANES + lane] = w;
            r[(WM + 2) * ROW_LANES + lane] = f;
            r[(WM + 3) * ROW_LANES + lane] = u;
            r[(WM + 4) * ROW_LANES + lane] = v;
            r[(WM + 5) * ROW_LANES + lane] = p;
            r[(WM + 6) * ROW_LANES + lane] = D;
            r[(WM + 7) * ROW_LANES + lane] = z;
        }
        #pragma unroll 1
        for (int64_t n = n1 - 1; n >= n0; --n) {
            const double *r = rows + (n - n0) * grad_rs(WM);
            // the row's scalars and vectors first, then its S whole, before anything waits on it (the load counter
            // retires in order: waiting for the vectors does not wait for S).  S's HBM latency then runs under the
            // first half of the step -- the LDS contraction with Sbar and three reductions -- one wait per row.
            const double tn = t[n], tq = t[n ? n - 1 : 0];
            const double Gn = r[(WM + 0) * ROW_LANES + lane], wn = r[(WM + 1) * ROW_LANES + lane];
            const double fn = r[(WM + 2) * ROW_LANES + lane], un = r[(WM + 3) * ROW_LANES + lane];
            const double vn = r[(WM + 4) * ROW_LANES + lane], pn = r[(WM + 5) * ROW_LANES + lane];
            const double Dn = r[(WM + 6) * ROW_LANES + lane], zn = r[(WM + 7) * ROW_LANES + lane];
            __builtin_amdgcn_sched_barrier(0);
            double sn[WM];
#pragma unroll
            for (int k = 0; k < WM; ++k) sn[k] = r[k * ROW_LANES + lane];
            __builtin_amdgcn_sched_barrier(0);
            const double dtn = tq - tn;                    // 0 at row 0
            double *x = sh[n & 1];
            x[lane] = wn;
            x[ROW_LANES + lane] = pn;
            x[2 * ROW_LANES + lane] = un;
            __syncthreads();
            // M_{n+1} = S_n + D_n W_n W_n^T and H_{n+1} = G_n + W_n z_n
            double qv = 0.0;
#pragma unroll
            for (int k = 0; k < WM; ++k) {
                qv += Sb[k * ROW_LANES + lane] * x[k];
                GR_PACE(k);
            }
            double Db = wsum(wn * qv);
            double zb = wsum(wn * Hb);
            double Wb = 2.0 * Dn * qv + Hb * zn;
            double Gb = Hb;
            // log L
            const double iD = 1.0 / Dn, zd = zn * iD;
            zb -= zd;
            Db += 0.5 * zd * zd - 0.5 * iD;
            // z_n = y_n - U_n^T G_n
            double Ub = -zb * Gn;
            Gb -= zb * un;
            // W_n = (V_n - f_n) / D_n
            const double Vb = Wb * iD;
            double fb = -Vb;
            Db -= wsum(Wb * wn) * iD;
            // D_n = A_n - U_n^T f_n
            Ub -= Db * fn;
            fb -= Db * un;
            x[3 * ROW_LANES + lane] = fb;
            __syncthreads();
            // f_n = S_n U_n: Ubar += S_n fbar, Sbar += sym(fbar U^T); then P's adjoint and Mbar_n = P Sbar P
            double sf = 0.0, ss = 0.0;
#pragma unroll
            for (int k = 0; k < WM; ++k) {
                const double snk = sn[k];
                sf += snk * x[3 * ROW_LANES + k];
                const double sb = Sb[k * ROW_LANES + lane] + 0.5 * (fb * x[2 * ROW_LANES + k] + un * x[3 * ROW_LANES + k]);
                ss += sb * snk;
                Sb[k * ROW_LANES + lane] = sb * (pn * x[ROW_LANES + k]);
            }
            Ub += sf;
            gc += dtn * (2.0 * ss + Gb * Gn);          // p_j Pbar_j dp/dc / p = dt (t_{n-1} - t_n)
            Hb = pn * Gb;
            gA += Db;
            gy += zb;
            // coefficient adjoints of this row's U, V
            const double pUb = __shfl(Ub, partner, ROW_LANES), pU = __shfl(un, partner, ROW_LANES);
            const double pV = __shfl(vn, partner, ROW_LANES), pVb = __shfl(Vb, partner, ROW_LANES);
            if (q.kind == 1) {
                ga += Ub;
            } else if (q.kind == 2 && q.half == 0) {
                const double co = vn, si = pV;
                ga += Ub * co + pUb * si;
                gb += Ub * si - pUb * co;
                // d theta_n / d d = t_n, summed as (t_n - t_0): rotating every phase of a term by one angle leaves K
                // unchanged, so sum_n thbar_n = 0 analytically.  In float64 that sum is rounding residue, and adding
                // t_0 times it back put up to 1.6e-6 of error into this adjoint on a JD-based axis (t_0 = 2e5)
                const double th = -Ub * pU + pUb * un - Vb * si + pVb * co;
                gtht += (tn - t0) * th;
            }
        }
    }
    const double gcp = __shfl(gc, partner, ROW_LANES);
    if (q.kind == 1) {
        g_real[(int64_t)b * lr + term] = ga;
        g_real[(int64_t)B * lr + (int64_t)b * lr + term] = gc;
    } else if (q.kind == 2 && q.half == 0) {
        const int64_t o = (int64_t)b * lc + term;
        g_comp[o] = ga;
        g_comp[(int64_t)B * lc + o] = gb;
        g_comp[(int64_t)2 * B * lc + o] = gc + gcp;
        g_comp[(int64_t)3 * B * lc + o] = gtht;
    }
    if (lane == 0) {
        ll[b] = -0.5 * (logdet + quad + (double)N * log(6.283185307179586));
        info[b] = 0;
        g_diag[b] = gA;
        g_mean[b] = -gy;
    }
}

}  // namespace

extern "C" {

int64_t gf_grad_work(int64_t N, int W) {
    if (N < 1 || W < 1 || W > ROW_MAX_W) return 0;
    return grad_work(N, W);
}

int gf_loglike_grad(int B, int64_t N, int Jr, int Jc,
                    const double *ar, const double *cr, const double *ac, const double *bc,
                    const double *cc, const double *dc, const double *diag_add,
                    const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                    const double *y, int64_t y_bs, double *work, int64_t work_bs,
                    double *ll, double *g_real, double *g_comp, double *g_diag, double *g_mean,
                    int32_t *info, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || Jr < 0 || Jc < 0 || W < 1)
        return gf_internal_error(-1, "gf_loglike_grad: bad shape (B=%d, N=%lld, Jr=%d, Jc=%d)", B, (long long)N,
                                 Jr, Jc);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_loglike_grad: width W=%d exceeds the one-wave limit %d", W, ROW_MAX_W);
    if (work_bs < grad_work(N, W))
        return gf_internal_error(-1, "gf_loglike_grad: work_bs=%lld < gf_grad_work(N, W)=%lld", (long long)work_bs,
                                 (long long)grad_work(N, W));
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !work || !ll ||
        !g_real || !g_comp || !g_diag || !g_mean || !info)
        return gf_internal_error(-1, "gf_loglike_grad: null pointer");
    const int64_t K = grad_seg(N), nseg = (N + K - 1) / K;
    hipStream_t st = (hipStream_t)stream;
    const int WM = row_wm(W);
#define GR_LAUNCH(WMV)                                                                                          \
    hipLaunchKernelGGL(k_grad<WMV>, dim3((unsigned)B), dim3(ROW_LANES), 0, st, N, K, nseg, Jr, Jc, ar, cr, ac, bc, \
                       cc, dc, diag_add, t, t_bs, diag, diag_bs, y, y_bs, work, work_bs, ll, g_real, g_comp,     \
                       g_diag, g_mean, info)
    if (WM == 16) GR_LAUNCH(16);
    else if (WM == 32) GR_LAUNCH(32);
    else GR_LAUNCH(64);
#undef GR_LAUNCH
    return gf_internal_check_launch("gf_loglike_grad");
}

}  // extern "C"
