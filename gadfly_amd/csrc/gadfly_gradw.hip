// gadfly_gradw.hip -- reverse-mode gradient of the celerite log-likelihood for wide kernels
//
// The mathematics of gadfly_grad.hip (k_grad is the specification: the plain unscaled recurrence with exact generator
// rows, a checkpointed reverse pass, real and complex terms in the original layout), with one problem's W x W state
// held by a WORKGROUP of several waves instead of one wave, so that W reaches gadfly's 86-term default (W = 172).
//
// Geometry of an instance <RT, NS, CW, CL>: RT row threads (a multiple of 64) times NS column slabs of CW columns.
// Thread (r, cs) = (tid % RT, tid / RT) owns columns cs CW .. cs CW + CW - 1 of row r of the resident matrix -- the
// first CW - CL in registers, the last CL in LDS: S in pass 1 and in a segment's recompute, Mbar in the reverse step
// (whose S_n streams in from the staged row).  Only one matrix is resident: Mbar is parked in the workspace while a
// segment is recomputed.  A wave holds 64 consecutive rows of ONE slab, so every vector element it reads from LDS is
// a broadcast, and every load and store of the staged matrix (element (r, k) at k RT + r) is one contiguous 512-byte
// run.
//   * mat-vecs (S u, Mbar w, S fbar): per-slab partials through LDS, added in slab order 0 .. NS - 1;
//   * the row's dots: a fixed tree over a wave's 64 rows, then the per-wave partials of slab 0 added in row-block
//     order;
//   * the per-row scalars and vectors (G, w, D, z, Hbar, ...) are held redundantly by the NS threads of a row -- they
//     come out of the same LDS values by the same operations, so they agree to the bit;
//   * the generator rows (sincos, exp) of a segment are laid out ahead of its row loop by all threads, and log D is
//     summed after it: the row loops hold none of their constants;
//   * the coefficient adjoints are per-THREAD sums in row order (a thread adds what its own slab contributes: its
//     partial of S fbar and of sum Sbar S; slab 0 also the row's vector terms), combined across slabs and across
//     the two columns of a complex term once, at the end, in a fixed order.
// Contraction is off in this unit and every fused operation is written out: pass 1 and the recompute run the same
// row function inlined twice, and a segment's recompute must reproduce pass 1's state to the bit for the outputs to
// be independent of the segment length.  No atomics; a problem's bits depend on its own data, N and W alone.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <atomic>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_rows.h"
#include "gf_wave.h"

#pragma clang fp contract(off)

namespace {

constexpr int GW_MAX_W = 192;
#ifndef GW_CL192
#define GW_CL192 32
#endif

// the instance of a width: row threads RT, slabs NS, columns per slab CW (NS CW = RT >= W), of which the last CL
// are held in LDS and the others in registers
struct GwGeo { int rt, ns, cw, cl; };
__host__ __device__ inline GwGeo gw_geo(int W) {
    return W <= 64 ? GwGeo{64, 2, 32, 0} : W <= 128 ? GwGeo{128, 2, 64, 0} : GwGeo{192, 2, 96, GW_CL192};
}

// rows per segment by default: the smallest K with K^2 >= N
inline int64_t gw_seg(int64_t N) {
    int64_t K = (int64_t)sqrt((double)N);
    while (K * K < N) ++K;
    while (K > 1 && (K - 1) * (K - 1) >= N) --K;
    return K < 1 ? 1 : K;
}

// doubles per checkpoint (S, then G, w, D, z) and per staged row (S, then G, w, f, u, v, p, D, z): S element (r, k) at
// k RT + r, the vectors one element per row thread (D and z repeated along it).  The workspace of a problem: the
// checkpoints, one segment of staged rows, and one matrix where Mbar is parked during a recompute.
__host__ __device__ constexpr int64_t gw_ck(int RT, int NC) { return (int64_t)(NC + 4) * RT; }
__host__ __device__ constexpr int64_t gw_rs(int RT, int NC) { return (int64_t)(NC + 8) * RT; }

inline int64_t gw_work(int64_t N, int W, int64_t seg) {
    const GwGeo g = gw_geo(W);
    const int64_t nseg = (N + seg - 1) / seg;
    return nseg * gw_ck(g.rt, g.ns * g.cw) + seg * gw_rs(g.rt, g.ns * g.cw) + (int64_t)g.ns * g.cw * g.rt;
}

inline int64_t gw_clamp_seg(int64_t N, int64_t seg) { return seg <= 0 ? gw_seg(N) : seg > N ? N : seg; }

// (the workspace is global memory: said outright, the accesses are global_ rather than flat_ instructions with a
// scalar base and the lane's 32-bit offset)
typedef __attribute__((address_space(1))) char gw_gchar;
typedef __attribute__((address_space(1))) double gw_gdouble;
__device__ __forceinline__ double gw_ld(const double *base, unsigned boff) {
    return *(const gw_gdouble *)((const gw_gchar *)base + boff);
}
__device__ __forceinline__ void gw_st(double *base, unsigned boff, double x) {
    *(gw_gdouble *)((gw_gchar *)base + boff) = x;
}
#define GW_LANE_OFFSETS unsigned bo = bo0, ro = ro0; asm volatile("" : "+v"(bo), "+v"(ro))
// a uniform base pointer made opaque where it is used: its per-column addresses (base + k RT, one scalar pair each)
// are then formed at the access, not hoisted out of the row and segment loops where 2 NC scalar registers hold them
template <class T>
__device__ __forceinline__ T *gw_here(T *ptr) {
    const uint64_t a = (uint64_t)ptr;
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (T *)(((uint64_t)hi << 32) | lo);
}

// Every GW_G columns of a row's loops: no load (LDS broadcast, staged S) moves across, and the loop's running sums
// pass through, so that a loop holds the operands of a few columns at a time instead of all of them.  (A scheduling
// barrier does not do it: it binds the machine scheduler, and by then instruction selection has put a block's loads
// in program order at its top and the arithmetic, which nothing orders, next to its users at the bottom.)
constexpr int GW_G = 4;
#define GW_FENCE asm volatile("" ::: "memory")
#define GW_FENCE1(a) asm volatile("" : "+v"(a) :: "memory")
#define GW_FENCE2(a, b) asm volatile("" : "+v"(a), "+v"(b) :: "memory")

// element k of the thread's run of the resident matrix: the first CW - CL in registers, the others in LDS at
// [k - CR][tid] (conflict-free)
// (two bases, xl and xh = xl + (CL / 2) NT, so that every LDS offset fits the instruction's 16 bits)
#define GW_XL(j) ((j) < CL / 2 ? xl[(j) * NT] : xh[((j) - CL / 2) * NT])
#define GW_X(k) ((k) < CR ? X[(k) < CR ? (k) : 0] : GW_XL((k) - CR))
#define GW_SETX(k, val) do { if ((k) < CR) X[(k) < CR ? (k) : 0] = (val); else GW_XL((k) - CR) = (val); } while (0)

// LDS of one row step (two of them, by the row's parity): the vectors w, p, u, v, fbar (RT each), the slab partials
// (NS RT) and the dots' per-wave partials (3 per row block); behind them the matrix's LDS columns
template <int RT, int NS> constexpr int gw_lds() { return (5 + NS) * RT + 16; }
inline size_t gw_lds_bytes(const GwGeo &g) {
    return sizeof(double) * (2 * ((size_t)(5 + g.ns) * g.rt + 16) + (size_t)g.cl * g.rt * g.ns);
}

__device__ __forceinline__ void gw_gen_row(const Col &q, double tn, double &u, double &v) {
    if (q.kind == 2) {
        double s, co;
        sincos(q.d * tn, &s, &co);        // theta = fl(d t), as celerite2
        if (q.half == 0) { u = fma(q.a, co, q.b * s); v = co; }
        else             { u = fma(q.a, s, -(q.b * co)); v = s; }
    } else if (q.kind == 1) {
        u = q.a; v = 1.0;
    } else {
        u = 0.0; v = 0.0;
    }
}

// the generator rows of a segment, ahead of its row loop: u, v, p of the rows n0 .. n1 - 1 into their slots of the
// staged rows.  Thread (r, cs) takes row r of every NS-th stamp; nothing of the matrix is live here, and the row loops
// hold none of sincos' and exp's constants.
template <int RT, int NS, int NC>
__device__ __forceinline__ void gw_gen_seg(int b, int r, int Jr, int Jc, const double *ar, const double *cr,
                                           const double *ac, const double *bc, const double *cc, const double *dc,
                                           const double *t, int64_t n0, int64_t n1, double *rows, unsigned ro, int cs) {
    asm volatile("" : "+s"(b));                        // the coefficients are read here, not held through the row loops
    const Col q = load_col(b, r, Jr, Jc, ar, cr, ac, bc, cc, dc);
    #pragma unroll 1
    for (int64_t n = n0 + cs; n < n1; n += NS) {
        const double tn = t[n], tp = n ? t[n - 1] : tn;
        double u, v;
        gw_gen_row(q, tn, u, v);
        const double p = exp(q.c * (tp - tn));
        double *rw = rows + (n - n0) * gw_rs(RT, NC);
        gw_st(rw + (NC + 3) * RT, ro, u);
        gw_st(rw + (NC + 4) * RT, ro, v);
        gw_st(rw + (NC + 5) * RT, ro, p);
    }
}

// one forward row: (S, G, w, D, z) of row n-1 and u, v, p of row n in, (S, G, w, D, z) and f of row n out.  Two
// workgroup barriers with one row block, three with more.
template <int RT, int NS, int CW, int CL>
__device__ __forceinline__ void gw_fwd_row(double (&X)[CW - CL], double *xl, double *xh, double &G, double &w, double &D, double &z, double u,
                                           double v, double p, double An, double yn, double *sh, int r, int cs,
                                           double &f) {
    constexpr int NRB = RT / 64, CR = CW - CL, NT = RT * NS;
    double *part = sh + 5 * RT, *dots = sh + (5 + NS) * RT;
    if (cs == 0) {
        sh[r] = w;
        sh[RT + r] = p;
        sh[2 * RT + r] = u;
    }
    wg_lds_barrier();
    const double wi = D * w;
    const double *xw = sh + cs * CW, *xp = sh + RT + cs * CW, *xu = sh + 2 * RT + cs * CW;
    double fp = 0.0;
#pragma unroll
    for (int k = 0; k < CW; ++k) {
        const double s = (p * xp[k]) * fma(wi, xw[k], GW_X(k));
        GW_SETX(k, s);
        fp = fma(s, xu[k], fp);
        if (k % GW_G == GW_G - 1) GW_FENCE1(fp);
    }
    part[cs * RT + r] = fp;
    wg_lds_barrier();
    f = part[r];
#pragma unroll
    for (int c = 1; c < NS; ++c) f += part[c * RT + r];
    G = p * fma(w, z, G);
    double uf = wave_sum(u * f), ug = wave_sum(u * G);
    if (NRB > 1) {
        if (cs == 0 && (r & 63) == 0) { dots[3 * (r >> 6)] = uf; dots[3 * (r >> 6) + 1] = ug; }
        wg_lds_barrier();
        uf = dots[0]; ug = dots[1];
#pragma unroll
        for (int i = 1; i < NRB; ++i) { uf += dots[3 * i]; ug += dots[3 * i + 1]; }
    }
    D = An - uf;
    z = yn - ug;
    w = (v - f) / D;
}

template <int RT, int NS, int CW, int CL>
__global__ __launch_bounds__(RT * NS) void k_gradw(
    int64_t N, int64_t K, int64_t nseg, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add, const double *__restrict__ t, int64_t t_bs,
    const double *__restrict__ dg, int64_t d_bs, const double *__restrict__ y, int64_t y_bs,
    double *work, int64_t work_bs, double *__restrict__ ll, double *__restrict__ g_real,
    double *__restrict__ g_comp, double *__restrict__ g_diag, double *__restrict__ g_mean,
    int32_t *__restrict__ info) {
    constexpr int NT = RT * NS, NC = NS * CW, NRB = RT / 64, LDS = gw_lds<RT, NS>(), CR = CW - CL;
    static_assert(NC <= RT && RT % 64 == 0 && NT <= 1024, "gw geometry");
    static_assert(2 * LDS >= 4 * NT, "the final combine reuses the row steps' LDS");
    static_assert(CR >= GW_G && CW % GW_G == 0, "gw geometry");
    extern __shared__ double shm[];                   // 2 LDS doubles of row steps, then the matrix's LDS columns
    const int B = (int)gridDim.x, b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int r = tid % RT, cs = tid / RT;
    const int lr = Jr > 0 ? Jr : 1, lc = Jc > 0 ? Jc : 1, W = Jr + 2 * Jc;
    struct { int kind, half; } q{0, 0};              // (the coefficients themselves: gw_gen_seg)
    int term = -1;
    if (r < Jr) {
        term = r;
        q.kind = 1;
    } else if (r < W) {
        term = (r - Jr) >> 1;
        q.kind = 2; q.half = (r - Jr) & 1;
    }
    const int partner = q.kind == 2 ? (q.half ? r - 1 : r + 1) : r;
    t += (int64_t)b * t_bs;
    y += (int64_t)b * y_bs;
    if (dg) dg += (int64_t)b * d_bs;
    constexpr int64_t CK = gw_ck(RT, NC), RS = gw_rs(RT, NC);
    double *ck = work + (int64_t)b * work_bs;
    double *rows = ck + nseg * CK;
    double *mbs = rows + K * RS;                       // Mbar, parked while a segment is recomputed
    const double dadd = diag_add[b];
    const double t0 = t[0];
    const int k0 = cs * CW;
    // S element (r, k0 + k) at (k RT) + k0 RT + r, a vector's element at r: a uniform base and one 32-bit byte offset
    // per lane (GW_LANE_OFFSETS keeps them from being folded into per-column addresses hoisted out of the row loops)
    const unsigned bo0 = 8u * (unsigned)(k0 * RT + r), ro0 = 8u * (unsigned)r;

    // ---- pass 1: log L and the checkpoints, segment by segment.  The state goes to the segment's checkpoint, the
    // segment's generator rows are laid out (the matrix is not live meanwhile), the state comes back.
    double X[CR];
    double *xl = shm + 2 * LDS + tid, *xh = xl + (CL / 2) * NT;
    asm volatile("" : "+v"(xh));
#pragma unroll
    for (int k = 0; k < CW; ++k) GW_SETX(k, 0.0);
    double G = 0.0, w = 0.0, D = 0.0, z = 0.0, f;
    double logdet = 0.0, quad = 0.0;
    int64_t bad = 0;
    #pragma unroll 1
    for (int64_t s = 0; s < nseg && !bad; ++s) {
        GW_LANE_OFFSETS;
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        double *c = gw_here(ck + s * CK);
#pragma unroll
        for (int k = 0; k < CW; ++k) gw_st(c + k * RT, bo, GW_X(k));
        if (cs == 0) {
            gw_st(c + (NC + 0) * RT, ro, G);
            gw_st(c + (NC + 1) * RT, ro, w);
            gw_st(c + (NC + 2) * RT, ro, D);
            gw_st(c + (NC + 3) * RT, ro, z);
        }
        gw_gen_seg<RT, NS, NC>(b, r, Jr, Jc, ar, cr, ac, bc, cc, dc, t, n0, n1, rows, ro, cs);
        __syncthreads();              // the generator rows were written by all slabs
        c = gw_here(c);
#pragma unroll
        for (int k = 0; k < CW; ++k) GW_SETX(k, gw_ld(c + k * RT, bo));
        double nu = gw_ld(rows + (NC + 3) * RT, ro), nv = gw_ld(rows + (NC + 4) * RT, ro);
        double np = gw_ld(rows + (NC + 5) * RT, ro);
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            GW_LANE_OFFSETS;
            const double u = nu, v = nv, p = np;
            if (n + 1 < n1) {                          // the next row's generator values, one row ahead
                const double *rn = gw_here(rows + (n + 1 - n0) * RS);
                nu = gw_ld(rn + (NC + 3) * RT, ro); nv = gw_ld(rn + (NC + 4) * RT, ro);
                np = gw_ld(rn + (NC + 5) * RT, ro);
            }
            const double An = (dg ? dg[n] : 0.0) + dadd;
            gw_fwd_row<RT, NS, CW, CL>(X, xl, xh, G, w, D, z, u, v, p, An, y[n], shm + (n & 1) * LDS, r, cs, f);
            if (!(D > 0.0)) { bad = n + 1; break; }
            quad += z * z / D;
            if (cs == 0) gw_st(gw_here(rows + (n - n0) * RS) + (NC + 6) * RT, ro, D);
        }
        if (bad) break;
        // sum log D over the segment's rows, in row order, outside the row loop (which then holds none of log's
        // constants): every thread adds the same values in the same order
        __syncthreads();
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) logdet += log(gw_ld(gw_here(rows + (n - n0) * RS) + (NC + 6) * RT, ro));
    }
    if (bad) {                                         // (D is the same in every thread: all of them leave)
        const double nan = __builtin_nan("");
        if (tid == 0) { ll[b] = -INFINITY; info[b] = (int32_t)bad; g_diag[b] = nan; g_mean[b] = nan; }
        if (cs == 0) {
            if (q.kind == 1) {
                g_real[(int64_t)b * lr + term] = nan;
                g_real[(int64_t)B * lr + (int64_t)b * lr + term] = nan;
            } else if (q.kind == 2 && q.half == 0) {
                for (int i = 0; i < 4; ++i) g_comp[(int64_t)i * B * lc + (int64_t)b * lc + term] = nan;
            }
        }
        return;
    }

    // ---- reverse: segments last first, each recomputed from its checkpoint and staged row by row.  S and Mbar take
    // turns in the SAME registers and LDS columns: Mbar waits in the workspace while a segment's rows are recomputed.
    {
        GW_LANE_OFFSETS;
#pragma unroll
        for (int k = 0; k < CW; ++k) gw_st(gw_here(mbs) + k * RT, bo, 0.0);
    }
    double Hb = 0.0;                                   // adjoint of G_n + W_n z_n
    double ga = 0.0, gb = 0.0, gc = 0.0, gtht = 0.0, gA = 0.0, gy = 0.0;
    #pragma unroll 1
    for (int64_t s = nseg - 1; s >= 0; --s) {
        GW_LANE_OFFSETS;
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        const double *c = ck + s * CK;
        __syncthreads();              // the last segment's staged rows have been read; LDS changes hands
        gw_gen_seg<RT, NS, NC>(b, r, Jr, Jc, ar, cr, ac, bc, cc, dc, t, n0, n1, rows, ro, cs);
        __syncthreads();              // generator rows: written by all slabs; the checkpoint's vectors: by slab 0
        c = gw_here(c);
#pragma unroll
        for (int k = 0; k < CW; ++k) GW_SETX(k, gw_ld(c + k * RT, bo));
        G = gw_ld(c + (NC + 0) * RT, ro);
        w = gw_ld(c + (NC + 1) * RT, ro);
        D = gw_ld(c + (NC + 2) * RT, ro);
        z = gw_ld(c + (NC + 3) * RT, ro);
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            GW_LANE_OFFSETS;
            double *rw = gw_here(rows + (n - n0) * RS);
            const double u = gw_ld(rw + (NC + 3) * RT, ro), v = gw_ld(rw + (NC + 4) * RT, ro);
            const double p = gw_ld(rw + (NC + 5) * RT, ro);
            const double An = (dg ? dg[n] : 0.0) + dadd;
            gw_fwd_row<RT, NS, CW, CL>(X, xl, xh, G, w, D, z, u, v, p, An, y[n], shm + (n & 1) * LDS, r, cs, f);
#pragma unroll
            for (int k = 0; k < CW; ++k) gw_st(rw + k * RT, bo, GW_X(k));
            if (cs == 0) {
                gw_st(rw + (NC + 0) * RT, ro, G);
                gw_st(rw + (NC + 1) * RT, ro, w);
                gw_st(rw + (NC + 2) * RT, ro, f);
                gw_st(rw + (NC + 6) * RT, ro, D);
                gw_st(rw + (NC + 7) * RT, ro, z);
            }
        }
        __syncthreads();              // the staged vectors were written by slab 0
#pragma unroll
        for (int k = 0; k < CW; ++k) GW_SETX(k, gw_ld(gw_here(mbs) + k * RT, bo));
        #pragma unroll 1
        for (int64_t n = n1 - 1; n >= n0; --n) {
            GW_LANE_OFFSETS;
            const double *rw = gw_here(rows + (n - n0) * RS);
            const double tn = t[n], tq = t[n ? n - 1 : 0];
            const double Gn = gw_ld(rw + (NC + 0) * RT, ro), wn = gw_ld(rw + (NC + 1) * RT, ro);
            const double fn = gw_ld(rw + (NC + 2) * RT, ro), un = gw_ld(rw + (NC + 3) * RT, ro);
            const double vn = gw_ld(rw + (NC + 4) * RT, ro), pn = gw_ld(rw + (NC + 5) * RT, ro);
            const double Dn = gw_ld(rw + (NC + 6) * RT, ro), zn = gw_ld(rw + (NC + 7) * RT, ro);
            const double dtn = tq - tn;                    // 0 at row 0
            double sn[2][GW_G];                            // S_n streams in GW_G columns at a time, one group ahead
#pragma unroll
            for (int j = 0; j < GW_G; ++j) sn[0][j] = gw_ld(rw + j * RT, bo);
            double *x = shm + (n & 1) * LDS;
            double *part = x + 5 * RT, *dots = x + (5 + NS) * RT;
            if (cs == 0) {
                x[r] = wn;
                x[RT + r] = pn;
                x[2 * RT + r] = un;
                x[3 * RT + r] = vn;
            }
            wg_lds_barrier();
            // M_{n+1} = S_n + D_n W_n W_n^T and H_{n+1} = G_n + W_n z_n
            const double *xw = x + k0, *xp = x + RT + k0, *xu = x + 2 * RT + k0, *xf = x + 4 * RT + k0;
            double qp = 0.0;
#pragma unroll
            for (int k = 0; k < CW; ++k) {
                qp = fma(GW_X(k), xw[k], qp);
                if (k % GW_G == GW_G - 1) GW_FENCE1(qp);
            }
            part[cs * RT + r] = qp;
            wg_lds_barrier();
            double qv = part[r];
#pragma unroll
            for (int i = 1; i < NS; ++i) qv += part[i * RT + r];
            const double Wb = fma(2.0 * Dn, qv, Hb * zn);
            double Db = wave_sum(wn * qv), zb = wave_sum(wn * Hb), ww = wave_sum(Wb * wn);
            if (NRB > 1) {
                if (cs == 0 && (r & 63) == 0) {
                    dots[3 * (r >> 6)] = Db; dots[3 * (r >> 6) + 1] = zb; dots[3 * (r >> 6) + 2] = ww;
                }
                wg_lds_barrier();
                Db = dots[0]; zb = dots[1]; ww = dots[2];
#pragma unroll
                for (int i = 1; i < NRB; ++i) { Db += dots[3 * i]; zb += dots[3 * i + 1]; ww += dots[3 * i + 2]; }
            }
            // log L
            const double iD = 1.0 / Dn, zd = zn * iD;
            zb -= zd;
            Db += 0.5 * zd * zd - 0.5 * iD;
            // z_n = y_n - U_n^T G_n
            double Ub = -zb * Gn;
            const double Gb = fma(-zb, un, Hb);
            // W_n = (V_n - f_n) / D_n
            const double Vb = Wb * iD;
            double fb = -Vb;
            Db -= ww * iD;
            // D_n = A_n - U_n^T f_n
            Ub = fma(-Db, fn, Ub);
            fb = fma(-Db, un, fb);
            if (cs == 0) x[4 * RT + r] = fb;
            wg_lds_barrier();
            // f_n = S_n U_n: Ubar += S_n fbar, Sbar += sym(fbar U^T); then P's adjoint and Mbar_n = P Sbar P.
            // This thread's slab of both sums; S_n streams in from the staged row.
            double sf = 0.0, ss = 0.0;
#pragma unroll
            for (int g = 0; g < CW / GW_G; ++g) {
                if (g + 1 < CW / GW_G) {               // the next columns of S_n, while these are worked on
#pragma unroll
                    for (int j = 0; j < GW_G; ++j) sn[(g + 1) & 1][j] = gw_ld(rw + ((g + 1) * GW_G + j) * RT, bo);
                }
                GW_FENCE;
#pragma unroll
                for (int j = 0; j < GW_G; ++j) {
                    const int k = g * GW_G + j;
                    const double snk = sn[g & 1][j];
                    sf = fma(snk, xf[k], sf);
                    const double sb = fma(0.5, fma(fb, xu[k], un * xf[k]), GW_X(k));
                    ss = fma(sb, snk, ss);
                    GW_SETX(k, sb * (pn * xp[k]));
                    if (k < CR) asm volatile("" : "+v"(X[k < CR ? k : 0]));        // (not put off to the row's end)
                }
                GW_FENCE2(sf, ss);
            }
            // the thread's share of the row's adjoints: its slab's partial sums, and in slab 0 the vector terms
            const double Up = cs == 0 ? Ub + sf : sf;
            const double Vp = cs == 0 ? Vb : 0.0;
            gc = fma(dtn, cs == 0 ? fma(2.0, ss, Gb * Gn) : 2.0 * ss, gc);
            Hb = pn * Gb;
            gA += Db;
            gy += zb;
            if (q.kind == 1) {
                ga += Up;
            } else if (q.kind == 2) {
                // d theta_n / d d = t_n, summed as (t_n - t_0) (see k_grad).  A complex term's two columns each add
                // their own half of k_grad's sums: column j (cosine) what holds Ubar_j and Vbar_j, column j + 1 the rest
                const double vo = x[3 * RT + partner], uo = x[2 * RT + partner];
                if (q.half == 0) {
                    ga = fma(Up, vn, ga);
                    gb = fma(Up, vo, gb);
                    gtht = fma(tn - t0, -fma(Up, uo, Vp * vo), gtht);
                } else {
                    ga = fma(Up, vn, ga);
                    gb = fma(-Up, vo, gb);
                    gtht = fma(tn - t0, fma(Up, uo, Vp * vo), gtht);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CW; ++k) gw_st(gw_here(mbs) + k * RT, bo, GW_X(k));
    }

    // ---- combine: slabs in order, then the two columns of a complex term
    __syncthreads();
    shm[0 * NT + tid] = ga;
    shm[1 * NT + tid] = gb;
    shm[2 * NT + tid] = gc;
    shm[3 * NT + tid] = gtht;
    __syncthreads();
    if (cs == 0 && (q.kind == 1 || (q.kind == 2 && q.half == 0))) {
        double tot[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double a = shm[i * NT + r];
#pragma unroll
            for (int c2 = 1; c2 < NS; ++c2) a += shm[i * NT + c2 * RT + r];
            if (q.kind == 2) {
                double o = shm[i * NT + partner];
#pragma unroll
                for (int c2 = 1; c2 < NS; ++c2) o += shm[i * NT + c2 * RT + partner];
                a += o;
            }
            tot[i] = a;
        }
        if (q.kind == 1) {
            g_real[(int64_t)b * lr + term] = tot[0];
            g_real[(int64_t)B * lr + (int64_t)b * lr + term] = tot[2];
        } else {
            const int64_t o = (int64_t)b * lc + term;
            g_comp[o] = tot[0];
            g_comp[(int64_t)B * lc + o] = tot[1];
            g_comp[(int64_t)2 * B * lc + o] = tot[2];
            g_comp[(int64_t)3 * B * lc + o] = tot[3];
        }
    }
    if (tid == 0) {
        ll[b] = -0.5 * (logdet + quad + (double)N * log(6.283185307179586));
        info[b] = 0;
        g_diag[b] = gA;
        g_mean[b] = -gy;
    }
}

// opt the widest instance in to its dynamic LDS on the current device, once per device
bool gw_lds_opt_in(const void *fn, size_t bytes) {
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (done[dev].load(std::memory_order_acquire)) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    done[dev].store(true, std::memory_order_release);
    return true;
}

}  // namespace

extern "C" {

int gf_grad_wide_max_width(void) { return GW_MAX_W; }

int64_t gf_grad_wide_seg(int64_t N, int W) {
    if (N < 1 || W < 1 || W > GW_MAX_W) return 0;
    return gw_seg(N);
}

int64_t gf_grad_wide_work(int64_t N, int W, int64_t seg) {
    if (N < 1 || W < 1 || W > GW_MAX_W || seg < 0) return 0;
    return gw_work(N, W, gw_clamp_seg(N, seg));
}

int gf_loglike_grad_wide(int B, int64_t N, int64_t seg, int Jr, int Jc,
                         const double *ar, const double *cr, const double *ac, const double *bc,
                         const double *cc, const double *dc, const double *diag_add,
                         const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                         const double *y, int64_t y_bs, double *work, int64_t work_bs,
                         double *ll, double *g_real, double *g_comp, double *g_diag, double *g_mean,
                         int32_t *info, void *stream) {
    const int64_t W64 = (int64_t)Jr + 2 * (int64_t)Jc;
    if (B < 1 || N < 1 || seg < 0 || Jr < 0 || Jc < 0 || W64 < 1)
        return gf_internal_error(-1, "gf_loglike_grad_wide: bad shape (B=%d, N=%lld, seg=%lld, Jr=%d, Jc=%d)", B,
                                 (long long)N, (long long)seg, Jr, Jc);
    if (W64 > GW_MAX_W)
        return gf_internal_error(-3, "gf_loglike_grad_wide: width W=%lld exceeds the workgroup limit %d",
                                 (long long)W64, GW_MAX_W);
    const int W = (int)W64;
    const int64_t K = gw_clamp_seg(N, seg), nseg = (N + K - 1) / K;
    if (work_bs < gw_work(N, W, K))
        return gf_internal_error(-1, "gf_loglike_grad_wide: work_bs=%lld < gf_grad_wide_work(N, W, seg)=%lld",
                                 (long long)work_bs, (long long)gw_work(N, W, K));
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !work || !ll ||
        !g_real || !g_comp || !g_diag || !g_mean || !info)
        return gf_internal_error(-1, "gf_loglike_grad_wide: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const GwGeo g = gw_geo(W);
    const size_t lds = gw_lds_bytes(g);
    if (lds > 64 * 1024) {
        const void *fn[1] = {(const void *)k_gradw<192, 2, 96, GW_CL192>};     // (the one instance beyond 64 KB)
        if (!gw_lds_opt_in(fn[0], lds))
            return gf_internal_error(-1, "gf_loglike_grad_wide: cannot opt in to %lld bytes of LDS", (long long)lds);
    }
#define GW_LAUNCH(RT, NS, CW, CL)                                                                               \
    hipLaunchKernelGGL((k_gradw<RT, NS, CW, CL>), dim3((unsigned)B), dim3((RT) * (NS)), lds, st, N, K, nseg, Jr, \
                       Jc, ar, cr, ac, bc, cc, dc, diag_add, t, t_bs, diag, diag_bs, y, y_bs, work, work_bs, ll, \
                       g_real, g_comp, g_diag, g_mean, info)
    if (g.rt == 64) GW_LAUNCH(64, 2, 32, 0);
    else if (g.rt == 128) GW_LAUNCH(128, 2, 64, 0);
    else GW_LAUNCH(192, 2, 96, GW_CL192);
#undef GW_LAUNCH
    return gf_internal_check_launch("gf_loglike_grad_wide");
}

}  // extern "C"
