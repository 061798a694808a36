// gadfly_gradtp.hip -- the gradient of gadfly_grad.hip for ONE long series (or a few), cut into chunks that are
// swept concurrently, one wave per (problem, chunk)
//
// Same recurrence, same reverse step and same conventions as k_grad (gadfly_grad.hip): the plain, unscaled
// celerite recurrence with exact generator rows, lane j owning row j of S and of Sbar.  The state that enters a
// chunk's first row n0 is (X, Y) = (M_n0, H_n0) = (S + D W W^T, G + W z) of row n0 - 1, in that row's coordinates:
// the chunk's first row applies P with dt = t[n0 - 1] - t[n0] like any other row.
//   A  nominal pass    every chunk from (0, 0): end state (Xbar, Ybar), closed-loop transition Phi = prod A_n,
//                      A_n = (I - W_n U_n^T) diag(p_n), and the Gram sums G = sum h h^T / D, m = sum h z / D with
//                      h_n = Phi_{->n}^T (p_n o U_n): the chunk map of oracle/lft.py in plain coordinates;
//                      gf_chunk_combine_tree (gf_chunk_combine below 8 chunks) turns the maps into the TRUE start
//                      state of every chunk
//   B  forward pass    every chunk from its true start: sum log D, sum z^2 / D, checkpoints every K rows, true Phi
//   C  reverse passes  across a chunk the adjoint recurrence is affine with the linear part Phi:
//                        Hbar_in = Phi^T Hbar_out + srcH              (independent of Mbar)
//                        Mbar_in = Phi^T Mbar_out Phi + srcM(Hbar_out)
//                      sweep 1 (terminal 0, 0) gives srcH, a scan over the chunks the true Hbar at every boundary;
//                      sweep 2 (terminal 0, Hbar) gives srcM, a second scan the true Mbar; sweep 3 runs from the
//                      true terminals and alone accumulates the coefficient adjoints, per chunk; a last kernel adds
//                      the chunks' partial sums in chunk order.
// No atomics; every sum has one fixed association, and a problem's bits depend on its own data, N and chunk_len
// alone.  The workspace is laid out array by array over the problems of the call ([B * nch] slots each), which is
// what the combines read; the 64 x 64 slots hold element (i, j) at j * 64 + i, zero beyond the width.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_rows.h"

namespace {

constexpr int64_t TP_SLOT = ROW_LANES * ROW_LANES;      // a 64 x 64 state slot
constexpr int64_t TP_PART = 8 * ROW_LANES;              // a chunk's partial sums: a, b, c, theta per lane; sum A, sum y;
                                                        // row 6: log det, quad, failing row (pass B); row 7: (pass A)

// rows per segment of a chunk of L rows: the smallest K with K^2 >= L
inline int64_t tp_seg(int64_t L) {
    int64_t K = (int64_t)sqrt((double)L);
    while (K * K < L) ++K;
    while (K > 1 && (K - 1) * (K - 1) >= L) --K;
    return K < 1 ? 1 : K;
}

// doubles per checkpoint and per staged row: the layouts of gadfly_grad.hip
__host__ __device__ inline int64_t tp_ck(int WM) { return (int64_t)(WM + 4) * ROW_LANES; }
__host__ __device__ inline int64_t tp_rs(int WM) { return (int64_t)(WM + 8) * ROW_LANES; }

inline int64_t tp_clamp_len(int64_t N, int64_t L) { return L > N ? N : L; }

// from this many chunks on the start states come from the log-depth combine (gf_chunk_combine_tree: 2 (log2 P - 1)
// levels of 64 us) instead of the sequential one (51 us a chunk); below, the sequential one is the shorter
constexpr int64_t TP_TREE_MIN = 8;

// the power of two P with P / 2 < nch <= P
inline int64_t tp_pow2(int64_t nch) {
    int64_t P = 2;
    while (P < nch) P *= 2;
    return P;
}

// doubles per problem the tree combine needs beyond the maps: its output states and the slots of its padding
inline int64_t tp_tree_work(int64_t nch) {
    if (nch < TP_TREE_MIN) return 0;
    return nch * (TP_SLOT + ROW_LANES) + (tp_pow2(nch) - nch) * (4 * TP_SLOT + 3 * ROW_LANES) + 8;
}

inline int64_t tp_work(int64_t N, int W, int64_t L) {
    const int WM = row_wm(W);
    L = tp_clamp_len(N, L);
    const int64_t nch = (N + L - 1) / L, K = tp_seg(L), nseg = (L + K - 1) / K;
    return nch * (3 * TP_SLOT + 3 * ROW_LANES + TP_PART + nseg * tp_ck(WM) + K * tp_rs(WM)) + ROW_LANES +
           tp_tree_work(nch);
}

struct TpArgs {
    int B, Jr, Jc;
    int64_t N, L, nch, K, nseg;
    const double *ar, *cr, *ac, *bc, *cc, *dc, *diag_add;
    const double *t, *dg, *y;
    int64_t t_bs, d_bs, y_bs;
    double *Phi, *Gm, *X;       // [B * nch][4096]: transition; Gram sum, then srcM / Mbar_out; nominal end, then start
    double *mv, *Yv, *Hv;       // [B * nch][64]:   m; nominal end, then start; srcH, then Hbar_out
    double *part;               // [B * nch][TP_PART]
    double *hdr;                // [B][64]: element 0 = the problem's failing row (0: none)
    double *ck, *rows;          // [B * nch][nseg][tp_ck], [B * nch][K][tp_rs]
};

#define TP_PACE(k) do { if (((k) & 7) == 7) __builtin_amdgcn_sched_barrier(0); } while (0)

__device__ __forceinline__ void tp_gen_row(const Col &q, double tn, double &u, double &v) {
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

// one forward row: (S, G, w, D, z) of row n-1 in, of row n out; f, u, v, p of row n out.  sh keeps w_{n-1}, p, u.
template <int WM>
__device__ __forceinline__ void tp_fwd_row(double (&S)[WM], double &G, double &w, double &D, double &z,
                                           const Col &q, double tprev, double tn, double An, double yn,
                                           double *sh, int lane, double &f, double &u, double &v, double &p) {
    tp_gen_row(q, tn, u, v);
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
        TP_PACE(k);
    }
    G = p * (G + w * z);
    const double uf = wsum(u * f), ug = wsum(u * G);
    D = An - uf;
    z = yn - ug;
    w = (v - f) / D;
}

// what every sweep kernel derives from its block index
struct TpChunk {
    int b, lane;
    int64_t slot, n0, n1;
};
__device__ __forceinline__ TpChunk tp_chunk(const TpArgs &a) {
    TpChunk c;
    c.lane = (int)threadIdx.x;
    c.slot = (int64_t)blockIdx.x;
    c.b = (int)(c.slot / a.nch);
    const int64_t ch = c.slot - (int64_t)c.b * a.nch;
    c.n0 = ch * a.L;
    c.n1 = c.n0 + a.L < a.N ? c.n0 + a.L : a.N;
    return c;
}

// ---- passes A (NOM) and B: the forward sweep of one chunk with its closed-loop transition
template <int WM, bool NOM>
__global__ __launch_bounds__(ROW_LANES) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_tp_fwd(const TpArgs a) {
    __shared__ double sh[2][4 * ROW_LANES];
    __shared__ double hs[2][ROW_LANES];
    const TpChunk c = tp_chunk(a);
    const int b = c.b, lane = c.lane, W = a.Jr + 2 * a.Jc;
    const Col q = load_col(b, lane, a.Jr, a.Jc, a.ar, a.cr, a.ac, a.bc, a.cc, a.dc);
    const double *t = a.t + (int64_t)b * a.t_bs, *y = a.y + (int64_t)b * a.y_bs;
    const double *dg = a.dg ? a.dg + (int64_t)b * a.d_bs : nullptr;
    const double dadd = a.diag_add[b];
    double *Xs = a.X + c.slot * TP_SLOT, *Ps = a.Phi + c.slot * TP_SLOT, *Gs = a.Gm + c.slot * TP_SLOT;
    double *pt = a.part + c.slot * TP_PART;

    double S[WM], T[WM], Gr[NOM ? WM : 1];
    double G = 0.0, w = 0.0, D = 0.0, z = 0.0, f, u, v, p;
    const bool zero = NOM || c.n0 == 0;
#pragma unroll
    for (int k = 0; k < WM; ++k) {
        // (the combines write the leading rows and columns of a start state only: nothing beyond the width is read)
        S[k] = (zero || k >= W || lane >= W) ? 0.0 : Xs[k * ROW_LANES + lane];
        T[k] = (k == lane && lane < W) ? 1.0 : 0.0;
    }
    if (NOM) {
#pragma unroll
        for (int k = 0; k < WM; ++k) Gr[k] = 0.0;
    }
    if (!zero && lane < W) G = a.Yv[c.slot * ROW_LANES + lane];
    double logdet = 0.0, quad = 0.0, mm = 0.0;
    int64_t bad = 0;
    #pragma unroll 1
    for (int64_t n = c.n0; n < c.n1; ++n) {
        if (!NOM && (n - c.n0) % a.K == 0) {
            double *k0 = a.ck + (c.slot * a.nseg + (n - c.n0) / a.K) * tp_ck(WM);
            ck_store<WM>(k0, lane, S, G, w, D, z);
        }
        const double tn = t[n], tp = n ? t[n - 1] : tn;
        const double An = (dg ? dg[n] : 0.0) + dadd;
        double *x = sh[n & 1];
        tp_fwd_row<WM>(S, G, w, D, z, q, tp, tn, An, y[n], x, lane, f, u, v, p);
        if (!(D > 0.0)) { bad = n + 1; break; }
        logdet += log(D);
        quad += z * z / D;
        // Phi <- (I - w u^T) diag(p) Phi, lane j on column j; h_j = sum_i u_i p_i Phi[i][j] falls out of it
        x[3 * ROW_LANES + lane] = w;
        __syncthreads();
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            T[i] *= x[ROW_LANES + i];
            s += x[2 * ROW_LANES + i] * T[i];
            TP_PACE(i);
        }
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            T[i] -= x[3 * ROW_LANES + i] * s;
            TP_PACE(i);
        }
        if (NOM) {
            const double hd = s / D;
            mm += hd * z;
            double *hv = hs[n & 1];
            hv[lane] = s;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < WM; ++k) {
                Gr[k] += hd * hv[k];
                TP_PACE(k);
            }
        }
    }
    if (NOM) {
        // the chunk map; a chunk that failed from the zero state hands the combine an inert map and flags the problem
        double *x = sh[0];
        __syncthreads();
        x[lane] = w;
        __syncthreads();
        const double wi = D * w;
#pragma unroll
        for (int k = 0; k < WM; ++k) {
            Xs[k * ROW_LANES + lane] = bad ? 0.0 : S[k] + wi * x[k];
            Gs[k * ROW_LANES + lane] = bad ? 0.0 : Gr[k];
            Ps[lane * ROW_LANES + k] = bad ? 0.0 : T[k];
        }
        for (int k = WM; k < ROW_LANES; ++k) {
            Xs[k * ROW_LANES + lane] = 0.0;
            Gs[k * ROW_LANES + lane] = 0.0;
            Ps[lane * ROW_LANES + k] = 0.0;
        }
        a.Yv[c.slot * ROW_LANES + lane] = bad ? 0.0 : G + w * z;
        a.mv[c.slot * ROW_LANES + lane] = bad ? 0.0 : mm;
        pt[7 * ROW_LANES + lane] = (double)bad;
    } else {
#pragma unroll
        for (int k = 0; k < WM; ++k) Ps[lane * ROW_LANES + k] = T[k];
        for (int k = WM; k < ROW_LANES; ++k) Ps[lane * ROW_LANES + k] = 0.0;
        pt[6 * ROW_LANES + lane] = lane == 0 ? logdet : lane == 1 ? quad : (double)bad;
    }
}

__device__ __forceinline__ int64_t wmin(int64_t x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const int64_t o = __shfl_xor(x, m, ROW_LANES);
        x = o < x ? o : x;
    }
    return x;
}

// the problem's failing row: that of the first chunk, in series order, whose true pass met a non-positive pivot
// (the sequential recurrence's own first failure whenever the nominal pass was clean); else a nominal pass' one
__global__ __launch_bounds__(ROW_LANES) void k_tp_flag(const TpArgs a, int nominal) {
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const double *pt = a.part + (int64_t)b * a.nch * TP_PART;
    int64_t first = a.nch, firstn = a.nch;
    for (int64_t ch = lane; ch < a.nch; ch += ROW_LANES) {
        if (pt[ch * TP_PART + 6 * ROW_LANES + 2] != 0.0 && ch < first) first = ch;
        if (nominal && pt[ch * TP_PART + 7 * ROW_LANES] != 0.0 && ch < firstn) firstn = ch;
    }
    first = wmin(first);
    firstn = wmin(firstn);
    double r = 0.0;
    if (first < a.nch) r = pt[first * TP_PART + 6 * ROW_LANES + 2];
    else if (firstn < a.nch) r = pt[firstn * TP_PART + 7 * ROW_LANES];
    a.hdr[(int64_t)b * ROW_LANES + lane] = r;
}

// ---- pass C: the reverse sweep of one chunk.  MODE 0: terminal (0, 0), stores Hbar_in (= srcH); MODE 1: terminal
// (0, Hbar_out), stores Mbar_in (= srcM); MODE 2: terminal (Mbar_out, Hbar_out), stores the chunk's partial sums.
// The body is k_grad's reverse (gadfly_grad.hip), segment by segment from pass B's checkpoints.
template <int WM, int MODE>
__global__ __launch_bounds__(ROW_LANES) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_tp_rev(const TpArgs a) {
    __shared__ double sh[2][4 * ROW_LANES];
    __shared__ double Sb[WM * ROW_LANES];           // Sbar, element (j, k) at k * 64 + j
    const TpChunk c = tp_chunk(a);
    const int b = c.b, lane = c.lane;
    if (a.hdr[(int64_t)b * ROW_LANES] != 0.0) return;
    const Col q = load_col(b, lane, a.Jr, a.Jc, a.ar, a.cr, a.ac, a.bc, a.cc, a.dc);
    const int partner = q.kind == 2 ? (q.half ? lane - 1 : lane + 1) : lane;
    const double *t = a.t + (int64_t)b * a.t_bs, *y = a.y + (int64_t)b * a.y_bs;
    const double *dg = a.dg ? a.dg + (int64_t)b * a.d_bs : nullptr;
    const double dadd = a.diag_add[b];
    const double t0 = t[0];
    const double *ck = a.ck + c.slot * a.nseg * tp_ck(WM);
    double *rows = a.rows + c.slot * a.K * tp_rs(WM);
    double *Ms = a.Gm + c.slot * TP_SLOT;

#pragma unroll
    for (int k = 0; k < WM; ++k) Sb[k * ROW_LANES + lane] = MODE == 2 ? Ms[k * ROW_LANES + lane] : 0.0;
    double Hb = MODE >= 1 ? a.Hv[c.slot * ROW_LANES + lane] : 0.0;
    double ga = 0.0, gb = 0.0, gc = 0.0, gtht = 0.0, gA = 0.0, gy = 0.0;
    double S[WM];
    double G, w, D, z, f, u, v, p;
    const int64_t K = a.K, nsegc = (c.n1 - c.n0 + K - 1) / K;
    #pragma unroll 1
    for (int64_t s = nsegc - 1; s >= 0; --s) {
        const int64_t n0 = c.n0 + s * K, n1 = (n0 + K < c.n1) ? n0 + K : c.n1;
        const double *k0 = ck + s * tp_ck(WM);
#pragma unroll
        for (int k = 0; k < WM; ++k) S[k] = k0[lane * WM + k];
        G = k0[(WM + 0) * ROW_LANES + lane];
        w = k0[(WM + 1) * ROW_LANES + lane];
        D = k0[(WM + 2) * ROW_LANES + lane];
        z = k0[(WM + 3) * ROW_LANES + lane];
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            const double tn = t[n], tp = n ? t[n - 1] : tn;
            const double An = (dg ? dg[n] : 0.0) + dadd;
            tp_fwd_row<WM>(S, G, w, D, z, q, tp, tn, An, y[n], sh[n & 1], lane, f, u, v, p);
            double *r = rows + (n - n0) * tp_rs(WM);
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
            const double *r = rows + (n - n0) * tp_rs(WM);
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
            const double dtn = tq - tn;                    // 0 at row 0 of the series only
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
                TP_PACE(k);
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
            Hb = pn * Gb;
            if (MODE == 2) {
                Ub += sf;
                gc += dtn * (2.0 * ss + Gb * Gn);
                gA += Db;
                gy += zb;
                const double pUb = __shfl(Ub, partner, ROW_LANES), pU = __shfl(un, partner, ROW_LANES);
                const double pV = __shfl(vn, partner, ROW_LANES), pVb = __shfl(Vb, partner, ROW_LANES);
                if (q.kind == 1) {
                    ga += Ub;
                } else if (q.kind == 2 && q.half == 0) {
                    const double co = vn, si = pV;
                    ga += Ub * co + pUb * si;
                    gb += Ub * si - pUb * co;
                    // weighted by (t_n - t_0) with t_0 the first stamp of the SERIES, as k_grad
                    const double th = -Ub * pU + pUb * un - Vb * si + pVb * co;
                    gtht += (tn - t0) * th;
                }
            }
        }
    }
    if (MODE == 0) {
        a.Hv[c.slot * ROW_LANES + lane] = Hb;
    } else if (MODE == 1) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WM; ++k) Ms[k * ROW_LANES + lane] = Sb[k * ROW_LANES + lane];
        for (int k = WM; k < ROW_LANES; ++k) Ms[k * ROW_LANES + lane] = 0.0;
    } else {
        double *pt = a.part + c.slot * TP_PART;
        pt[0 * ROW_LANES + lane] = ga;
        pt[1 * ROW_LANES + lane] = gb;
        pt[2 * ROW_LANES + lane] = gc;
        pt[3 * ROW_LANES + lane] = gtht;
        pt[4 * ROW_LANES + lane] = gA;
        pt[5 * ROW_LANES + lane] = gy;
    }
}

// ---- the Hbar scan, last chunk first, one wave per problem: slot c <- Hbar_out(c); Hbar_in = Phi^T Hbar_out + srcH.
// Lane j reads column j of Phi (64 contiguous doubles), the next chunk's while this one's is being used.
__global__ __launch_bounds__(ROW_LANES) void k_tp_hscan(const TpArgs a) {
    __shared__ double hv[2][ROW_LANES];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (a.hdr[(int64_t)b * ROW_LANES] != 0.0) return;
    const int64_t s0 = (int64_t)b * a.nch;
    double Hb = 0.0;
    double nx[ROW_LANES], cur[ROW_LANES];
    if (a.nch > 1) {
        const double *col = a.Phi + (s0 + a.nch - 1) * TP_SLOT + lane * ROW_LANES;
#pragma unroll
        for (int i = 0; i < ROW_LANES; ++i) nx[i] = col[i];
    }
    #pragma unroll 1
    for (int64_t ch = a.nch - 1; ch >= 0; --ch) {
        double *hs = a.Hv + (s0 + ch) * ROW_LANES;
        const double src = hs[lane];
        hs[lane] = Hb;
        if (ch == 0) break;
#pragma unroll
        for (int i = 0; i < ROW_LANES; ++i) cur[i] = nx[i];
        if (ch > 1) {
            const double *col = a.Phi + (s0 + ch - 1) * TP_SLOT + lane * ROW_LANES;
#pragma unroll
            for (int i = 0; i < ROW_LANES; ++i) nx[i] = col[i];
        }
        double *x = hv[ch & 1];
        x[lane] = Hb;
        __syncthreads();
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < ROW_LANES; ++i) acc += cur[i] * x[i];
        Hb = acc + src;
    }
}

// ---- the Mbar scan, last chunk first, one workgroup per problem with Mbar in LDS: slot c <- Mbar_out(c);
// Mbar_in = Phi^T Mbar_out Phi + srcM.  Two 64^3 products on 4 x 4 register blocks; Phi's slot ([column][row]) sits in
// LDS with every column rotated by its own index, so that the strided reads of both products meet no bank twice.
__global__ __launch_bounds__(256) void k_tp_mscan(const TpArgs a) {
    __shared__ double Ms[TP_SLOT], Qs[TP_SLOT];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (a.hdr[(int64_t)b * ROW_LANES] != 0.0) return;
    const int64_t s0 = (int64_t)b * a.nch;
    for (int e = tid; e < TP_SLOT; e += 256) Ms[e] = 0.0;
    __syncthreads();
    #pragma unroll 1
    for (int64_t ch = a.nch - 1; ch >= 0; --ch) {
        double *ms = a.Gm + (s0 + ch) * TP_SLOT;
        const double *ph = a.Phi + (s0 + ch) * TP_SLOT;
        double src[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) src[q] = ms[tid + 256 * q];
#pragma unroll
        for (int q = 0; q < 16; ++q) ms[tid + 256 * q] = Ms[tid + 256 * q];
        if (ch == 0) break;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q, j = e >> 6, i = e & 63;
            Qs[j * 64 + ((i + j) & 63)] = ph[e];            // Phi[i][j]
        }
        __syncthreads();
        double acc[4][4];
        // T = Mbar Phi (Mbar symmetric: its column r read as row r)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        #pragma unroll 4
        for (int k = 0; k < 64; ++k) {
            double av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = Ms[k * 64 + 4 * ty + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int cc = tx + 16 * j; bv[j] = Qs[cc * 64 + ((k + cc) & 63)]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) Ms[(4 * ty + i) * 64 + tx + 16 * j] = acc[i][j];
        __syncthreads();
        // Phi^T T
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        #pragma unroll 4
        for (int k = 0; k < 64; ++k) {
            double av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int r = 4 * ty + i; av[i] = Qs[r * 64 + ((k + r) & 63)]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Ms[k * 64 + tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * ty + i, cc = tx + 16 * j;
                Qs[r * 64 + ((cc + r) & 63)] = acc[i][j];
            }
        __syncthreads();
        // symmetrise, add the chunk's source
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q, j = e >> 6, i = e & 63;
            Ms[e] = 0.5 * (Qs[j * 64 + ((i + j) & 63)] + Qs[i * 64 + ((j + i) & 63)]) + src[q];
        }
        __syncthreads();
    }
}

// ---- the chunks' partial sums in chunk order, and the outputs in gf_loglike_grad's layout
__global__ __launch_bounds__(ROW_LANES) void k_tp_reduce(const TpArgs a, double *__restrict__ ll,
                                                         double *__restrict__ g_real, double *__restrict__ g_comp,
                                                         double *__restrict__ g_diag, double *__restrict__ g_mean,
                                                         int32_t *__restrict__ info) {
    const int B = a.B, b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int lr = a.Jr > 0 ? a.Jr : 1, lc = a.Jc > 0 ? a.Jc : 1;
    const Col q = load_col(b, lane, a.Jr, a.Jc, a.ar, a.cr, a.ac, a.bc, a.cc, a.dc);
    const int term = q.kind == 1 ? lane : (lane - a.Jr) >> 1;
    const int partner = q.kind == 2 ? (q.half ? lane - 1 : lane + 1) : lane;
    const double bad = a.hdr[(int64_t)b * ROW_LANES];
    if (bad != 0.0) {
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
    double ga = 0.0, gb = 0.0, gc = 0.0, gtht = 0.0, gA = 0.0, gy = 0.0, logdet = 0.0, quad = 0.0;
    #pragma unroll 1
    for (int64_t ch = 0; ch < a.nch; ++ch) {
        const double *pt = a.part + ((int64_t)b * a.nch + ch) * TP_PART;
        ga += pt[0 * ROW_LANES + lane];
        gb += pt[1 * ROW_LANES + lane];
        gc += pt[2 * ROW_LANES + lane];
        gtht += pt[3 * ROW_LANES + lane];
        gA += pt[4 * ROW_LANES + lane];
        gy += pt[5 * ROW_LANES + lane];
        logdet += pt[6 * ROW_LANES + 0];
        quad += pt[6 * ROW_LANES + 1];
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
        ll[b] = -0.5 * (logdet + quad + (double)a.N * log(6.283185307179586));
        info[b] = 0;
        g_diag[b] = gA;
        g_mean[b] = -gy;
    }
}

template <int WM>
void tp_launch_sweeps(const TpArgs &a, int stage, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)a.B * a.nch)), block(ROW_LANES);
    switch (stage) {
    case 0: hipLaunchKernelGGL((k_tp_fwd<WM, true>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_tp_fwd<WM, false>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_tp_rev<WM, 0>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_tp_rev<WM, 1>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_tp_rev<WM, 2>), grid, block, 0, st, a); break;
    }
}

void tp_sweeps(const TpArgs &a, int WM, int stage, hipStream_t st) {
    if (WM == 16) tp_launch_sweeps<16>(a, stage, st);
    else if (WM == 32) tp_launch_sweeps<32>(a, stage, st);
    else tp_launch_sweeps<64>(a, stage, st);
}

}  // namespace

extern "C" {

int64_t gf_grad_chunk_len(int B, int64_t N, int W) {
    if (B < 1 || N < 1 || W < 1 || W > ROW_MAX_W) return 0;
    // The sweeps' time grows with the rows of a chunk (0.030 ms a row at W = 60 while every wave has a SIMD of its
    // own, B * nch <= 1024), the scans' with the chunks of a series (0.015 ms a chunk; the tree combine's hardly at
    // all): the sum is smallest at chunk_len^2 = N / 2 (measured on shape (c)).  Lo: the smallest
    // length with 2 Lo^2 >= N, 64 rows at least.
    int64_t Lo = (int64_t)sqrt(0.5 * (double)N);
    while (2 * Lo * Lo < N) ++Lo;
    while (Lo > 1 && 2 * (Lo - 1) * (Lo - 1) >= N) --Lo;
    if (Lo < 64) Lo = 64;
    int64_t nch = 1024 / B;
    if (nch < 1) nch = 1;
    const int64_t most = (N + Lo - 1) / Lo;
    if (nch > most) nch = most;
    return (N + nch - 1) / nch;
}

int64_t gf_grad_chunked_work(int64_t N, int W, int64_t chunk_len) {
    if (N < 1 || W < 1 || W > ROW_MAX_W || chunk_len < 1) return 0;
    return tp_work(N, W, chunk_len);
}

int gf_loglike_grad_chunked(int B, int64_t N, int64_t chunk_len, int Jr, int Jc,
                            const double *ar, const double *cr, const double *ac, const double *bc,
                            const double *cc, const double *dc, const double *diag_add,
                            const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                            const double *y, int64_t y_bs, double *work, int64_t work_bs,
                            double *ll, double *g_real, double *g_comp, double *g_diag, double *g_mean,
                            int32_t *info, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1 || chunk_len < 1 || Jr < 0 || Jc < 0 || W < 1)
        return gf_internal_error(-1, "gf_loglike_grad_chunked: bad shape (B=%d, N=%lld, chunk_len=%lld, Jr=%d, Jc=%d)",
                                 B, (long long)N, (long long)chunk_len, Jr, Jc);
    if (W > ROW_MAX_W)
        return gf_internal_error(-3, "gf_loglike_grad_chunked: width W=%d exceeds the one-wave limit %d", W,
                                 ROW_MAX_W);
    const int64_t L = tp_clamp_len(N, chunk_len), nch = (N + L - 1) / L;
    if ((int64_t)B * nch > 0x7fffffffLL)
        return gf_internal_error(-1, "gf_loglike_grad_chunked: too many chunks (B=%d, %lld each)", B, (long long)nch);
    const int64_t per = tp_work(N, W, L);
    if (work_bs < per)
        return gf_internal_error(-1, "gf_loglike_grad_chunked: work_bs=%lld < gf_grad_chunked_work(N, W, chunk_len)=%lld",
                                 (long long)work_bs, (long long)per);
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !work || !ll ||
        !g_real || !g_comp || !g_diag || !g_mean || !info)
        return gf_internal_error(-1, "gf_loglike_grad_chunked: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int WM = row_wm(W);
    TpArgs a;
    a.B = B; a.Jr = Jr; a.Jc = Jc; a.N = N; a.L = L; a.nch = nch;
    a.K = tp_seg(L); a.nseg = (L + a.K - 1) / a.K;
    a.ar = ar; a.cr = cr; a.ac = ac; a.bc = bc; a.cc = cc; a.dc = dc; a.diag_add = diag_add;
    a.t = t; a.dg = diag; a.y = y; a.t_bs = t_bs; a.d_bs = diag_bs; a.y_bs = y_bs;
    const int64_t slots = (int64_t)B * nch;
    double *p = work;
    a.Phi = p; p += slots * TP_SLOT;
    a.Gm = p; p += slots * TP_SLOT;
    a.X = p; p += slots * TP_SLOT;
    a.mv = p; p += slots * ROW_LANES;
    a.Yv = p; p += slots * ROW_LANES;
    a.Hv = p; p += slots * ROW_LANES;
    a.part = p; p += slots * TP_PART;
    a.hdr = p; p += (int64_t)B * ROW_LANES;
    a.ck = p; p += slots * a.nseg * tp_ck(WM);
    a.rows = p; p += slots * a.K * tp_rs(WM);
    int rc;
    if (nch > 1) {
        tp_sweeps(a, WM, 0, st);
        if ((rc = gf_internal_check_launch("gf_loglike_grad_chunked (nominal pass)"))) return rc;
        if (nch >= TP_TREE_MIN) {
            // the log-depth combine leaves the start states in arrays of their own: pass B reads them there
            double *Xst = p, *Yst = Xst + slots * TP_SLOT, *tw = Yst + slots * ROW_LANES;
            const int P = (int)tp_pow2(nch);
            if (gf_chunk_combine_tree_work(B, P, (int)nch) > (int64_t)B * (tp_tree_work(nch) - nch * (TP_SLOT + ROW_LANES)))
                return gf_internal_error(-1, "gf_loglike_grad_chunked: internal workspace error");
            if ((rc = gf_chunk_combine_tree(B, P, (int)nch, W, a.Phi, a.Gm, a.mv, a.X, a.Yv, Xst, Yst, tw, stream)))
                return rc;
            a.X = Xst;
            a.Yv = Yst;
        } else if ((rc = gf_chunk_combine(B, (int)nch, W, a.Phi, a.Gm, a.mv, a.X, a.Yv, stream))) {
            return rc;
        }
    }
    tp_sweeps(a, WM, 1, st);
    hipLaunchKernelGGL(k_tp_flag, dim3((unsigned)B), dim3(ROW_LANES), 0, st, a, nch > 1 ? 1 : 0);
    tp_sweeps(a, WM, 2, st);
    hipLaunchKernelGGL(k_tp_hscan, dim3((unsigned)B), dim3(ROW_LANES), 0, st, a);
    tp_sweeps(a, WM, 3, st);
    hipLaunchKernelGGL(k_tp_mscan, dim3((unsigned)B), dim3(256), 0, st, a);
    tp_sweeps(a, WM, 4, st);
    hipLaunchKernelGGL(k_tp_reduce, dim3((unsigned)B), dim3(ROW_LANES), 0, st, a, ll, g_real, g_comp, g_diag, g_mean,
                       info);
    return gf_internal_check_launch("gf_loglike_grad_chunked");
}

}  // extern "C"
