// gadfly_solvew.hip -- alpha = K^-1 y and the conditional means of B problems for wide kernels
//
// The mathematics of gadfly_solve.hip (k_solve without a component is the specification: the plain unscaled
// recurrence with exact generator rows, a checkpointed forward sweep and the upper solve backwards over segments
// recomputed from the checkpoints), with one problem's W x W state held by a WORKGROUP of several waves, in the
// layout of gadfly_gradw.hip's pass 1, so that W reaches gadfly's 86-term default (W = 172).
//
// Geometry of an instance <RT, NS, CW, CL>: RT row threads (a multiple of 64) times NS column slabs of CW columns.
// Thread (r, cs) = (tid % RT, tid / RT) owns columns cs CW .. cs CW + CW - 1 of row r of S -- the first CW - CL in
// registers, the last CL in LDS.  A wave holds 64 consecutive rows of ONE slab, so every vector element it reads from
// LDS is a broadcast, and every load and store of a checkpoint (element (r, k) at k RT + r) is one contiguous
// 512-byte run.
//   * S u: per-slab partials through LDS, added in slab order 0 .. NS - 1;
//   * the row's dots: a fixed tree over a wave's 64 rows, then the per-wave partials of slab 0 added in row-block
//     order;
//   * the per-row scalars and vectors (G, w, D, z) are held redundantly by the NS threads of a row -- they come out of
//     the same LDS values by the same operations, so they agree to the bit;
//   * the generator rows (sincos, exp) of a segment are laid out ahead of its row loop by all threads, and log D is
//     summed after it: the row loops hold none of their constants;
//   * the backward rows carry W-vectors only: slab 0's threads hold H, one column each; alpha_n is a wave tree plus
//     the row blocks' partials through a double-buffered LDS slot -- one LDS barrier per backward row, none where slab
//     0 is a single wave;
//   * z, D, alpha and mu move 64 rows at a time through the lanes of a wave (contiguous 512-byte runs); alpha
//     overwrites z in the workspace as a block of 64 rows finishes.
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

constexpr int SW_MAX_W = 192;
#ifndef SW_CL192
#define SW_CL192 32
#endif

// the instance of a width: row threads RT, slabs NS, columns per slab CW (NS CW = RT >= W), of which the last CL
// are held in LDS and the others in registers
struct SwGeo { int rt, ns, cw, cl; };
__host__ __device__ inline SwGeo sw_geo(int W) {
    return W <= 64 ? SwGeo{64, 2, 32, 0} : W <= 128 ? SwGeo{128, 2, 64, 0} : SwGeo{192, 2, 96, SW_CL192};
}

// doubles per checkpoint (S, then G, w, D, z: S element (r, k) at k RT + r, the vectors one element per row thread, D
// and z repeated along it) and per staged row (u, then v -- W_n once the recompute has passed the row --, then p)
__host__ __device__ constexpr int64_t sw_ck(int RT, int NC) { return (int64_t)(NC + 4) * RT; }
__host__ __device__ constexpr int64_t sw_rs(int RT) { return (int64_t)3 * RT; }

// rows per segment that balance nseg checkpoints against K staged rows: the smallest K with 3 K^2 >= N (NC + 4)
inline int64_t sw_seg(int64_t N, int NC) {
    const unsigned __int128 want = (unsigned __int128)N * (unsigned)(NC + 4);
    int64_t K = (int64_t)sqrt((double)N * (double)(NC + 4) / 3.0);
    if (K < 1) K = 1;
    while ((unsigned __int128)K * K * 3 < want) ++K;
    while (K > 1 && (unsigned __int128)(K - 1) * (K - 1) * 3 >= want) --K;
    return K > N ? N : K;
}

inline int64_t sw_pick_seg(int64_t N, int W, int64_t seg) {
    const SwGeo g = sw_geo(W);
    if (seg == 0) return sw_seg(N, g.ns * g.cw);
    return seg > N ? N : seg;
}

// checkpoints, one segment's staged rows, z (alpha after pass 2) and D of every row
inline int64_t sw_work(int64_t N, int W, int64_t K) {
    const SwGeo g = sw_geo(W);
    const int64_t nseg = (N + K - 1) / K;
    return nseg * sw_ck(g.rt, g.ns * g.cw) + K * sw_rs(g.rt) + 2 * solve_n64(N);
}

// (the workspace is global memory: said outright, the accesses are global_ rather than flat_ instructions with a
// scalar base and the lane's 32-bit offset)
typedef __attribute__((address_space(1))) char sw_gchar;
typedef __attribute__((address_space(1))) double sw_gdouble;
__device__ __forceinline__ double sw_ld(const double *base, unsigned boff) {
    return *(const sw_gdouble *)((const sw_gchar *)base + boff);
}
__device__ __forceinline__ void sw_st(double *base, unsigned boff, double x) {
    *(sw_gdouble *)((sw_gchar *)base + boff) = x;
}
#define SW_LANE_OFFSETS unsigned bo = bo0, ro = ro0; asm volatile("" : "+v"(bo), "+v"(ro))
// a uniform base pointer made opaque where it is used: its per-column addresses (base + k RT, one scalar pair each)
// are then formed at the access, not hoisted out of the row and segment loops where 2 NC scalar registers hold them
template <class T>
__device__ __forceinline__ T *sw_here(T *ptr) {
    const uint64_t a = (uint64_t)ptr;
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (T *)(((uint64_t)hi << 32) | lo);
}

// Every SW_G columns of the row's loop: no LDS broadcast moves across, and the running sum passes through, so that
// the loop holds the operands of a few columns at a time instead of all of them
constexpr int SW_G = 4;
#define SW_FENCE1(a) asm volatile("" : "+v"(a) :: "memory")

// element k of the thread's run of S: the first CW - CL in registers, the others in LDS at [k - CR][tid]
// (conflict-free; two bases, xl and xh = xl + (CL / 2) NT, so that every LDS offset fits the instruction's 16 bits)
#define SW_XL(j) ((j) < CL / 2 ? xl[(j) * NT] : xh[((j) - CL / 2) * NT])
#define SW_X(k) ((k) < CR ? X[(k) < CR ? (k) : 0] : SW_XL((k) - CR))
#define SW_SETX(k, val) do { if ((k) < CR) X[(k) < CR ? (k) : 0] = (val); else SW_XL((k) - CR) = (val); } while (0)

// LDS of one row step (two of them, by the row's parity): the vectors w, p, u (RT each), the slab partials (NS RT)
// and the per-wave partials (3 per row block: the forward row's two dots, the backward row's one); behind them the
// matrix's LDS columns
template <int RT, int NS> constexpr int sw_lds() { return (3 + NS) * RT + 16; }
inline size_t sw_lds_bytes(const SwGeo &g) {
    return sizeof(double) * (2 * ((size_t)(3 + g.ns) * g.rt + 16) + (size_t)g.cl * g.rt * g.ns);
}

__device__ __forceinline__ void sw_gen_row(const Col &q, double tn, double &u, double &v) {
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

// the generator rows of a segment, ahead of its row loop: u, v, p of the rows n0 .. n1 - 1 into the staged rows.
// Thread (r, cs) takes row r of every NS-th stamp; nothing of the matrix is live here, and the row loops hold none of
// sincos' and exp's constants.
template <int RT, int NS>
__device__ __forceinline__ void sw_gen_seg(int b, int r, int Jr, int Jc, const double *ar, const double *cr,
                                           const double *ac, const double *bc, const double *cc, const double *dc,
                                           const double *t, int64_t n0, int64_t n1, double *rows, unsigned ro, int cs) {
    asm volatile("" : "+s"(b));                        // the coefficients are read here, not held through the row loops
    const Col q = load_col(b, r, Jr, Jc, ar, cr, ac, bc, cc, dc);
    #pragma unroll 1
    for (int64_t n = n0 + cs; n < n1; n += NS) {
        const double tn = t[n], tp = n ? t[n - 1] : tn;
        double u, v;
        sw_gen_row(q, tn, u, v);
        const double p = exp(q.c * (tp - tn));
        double *rw = rows + (n - n0) * sw_rs(RT);
        sw_st(rw, ro, u);
        sw_st(rw + RT, ro, v);
        sw_st(rw + 2 * RT, ro, p);
    }
}

// one forward row: (S, G, w, D, z) of row n-1 and u, v, p of row n in, (S, G, w, D, z) of row n out.  Two workgroup
// barriers with one row block, three with more.  (gadfly_gradw.hip's forward row, operation for operation.)
template <int RT, int NS, int CW, int CL>
__device__ __forceinline__ void sw_fwd_row(double (&X)[CW - CL], double *xl, double *xh, double &G, double &w,
                                           double &D, double &z, double u, double v, double p, double An, double yn,
                                           double *sh, int r, int cs) {
    constexpr int NRB = RT / 64, CR = CW - CL, NT = RT * NS;
    double *part = sh + 3 * RT, *dots = sh + (3 + NS) * RT;
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
        const double s = (p * xp[k]) * fma(wi, xw[k], SW_X(k));
        SW_SETX(k, s);
        fp = fma(s, xu[k], fp);
        if (k % SW_G == SW_G - 1) SW_FENCE1(fp);
    }
    part[cs * RT + r] = fp;
    wg_lds_barrier();
    double f = part[r];
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
__global__ __launch_bounds__(RT * NS) void k_solvew(
    int64_t N, int64_t K, int64_t nseg, int Jr, int Jc,
    const double *__restrict__ ar, const double *__restrict__ cr, const double *__restrict__ ac,
    const double *__restrict__ bc, const double *__restrict__ cc, const double *__restrict__ dc,
    const double *__restrict__ diag_add, const double *__restrict__ t, int64_t t_bs,
    const double *__restrict__ dg, int64_t d_bs, const double *__restrict__ y, int64_t y_bs,
    double *work, int64_t work_bs, double *alpha, double *mu, double *__restrict__ ll,
    int32_t *__restrict__ info) {
    constexpr int NT = RT * NS, NC = NS * CW, NRB = RT / 64, LDS = sw_lds<RT, NS>(), CR = CW - CL;
    static_assert(NC <= RT && RT % 64 == 0 && NT <= 1024, "sw geometry");
    static_assert(CR >= SW_G && CW % SW_G == 0 && 3 * NRB <= 16, "sw geometry");
    extern __shared__ double shm[];                   // 2 LDS doubles of row steps, then the matrix's LDS columns
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int r = tid % RT, cs = tid / RT, lane = tid & 63;
    t += (int64_t)b * t_bs;
    y += (int64_t)b * y_bs;
    if (dg) dg += (int64_t)b * d_bs;
    if (alpha) alpha += (int64_t)b * N;
    if (mu) mu += (int64_t)b * N;
    constexpr int64_t CK = sw_ck(RT, NC), RS = sw_rs(RT);
    double *ck = work + (int64_t)b * work_bs;
    double *rows = ck + nseg * CK;
    double *zw = rows + K * RS;                        // z_n, then alpha_n
    double *Dw = zw + solve_n64(N);
    const double dadd = diag_add[b];
    const int k0 = cs * CW;
    // S element (r, k0 + k) at (k RT) + k0 RT + r, a vector's element at r: a uniform base and one 32-bit byte offset
    // per lane (SW_LANE_OFFSETS keeps them from being folded into per-column addresses hoisted out of the row loops)
    const unsigned bo0 = 8u * (unsigned)(k0 * RT + r), ro0 = 8u * (unsigned)r;

    // ---- pass 1: log L, z and D of every row and the checkpoints, segment by segment.  The state goes to the
    // segment's checkpoint, the segment's generator rows are laid out (the matrix is not live meanwhile), the state
    // comes back.
    double X[CR];
    double *xl = shm + 2 * LDS + tid, *xh = xl + (CL / 2) * NT;
    asm volatile("" : "+v"(xh));
#pragma unroll
    for (int k = 0; k < CW; ++k) SW_SETX(k, 0.0);
    double G = 0.0, w = 0.0, D = 0.0, z = 0.0;
    double logdet = 0.0, quad = 0.0, zbuf = 0.0, dbuf = 1.0;
    int64_t bad = 0;
    #pragma unroll 1
    for (int64_t s = 0; s < nseg && !bad; ++s) {
        SW_LANE_OFFSETS;
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        double *c = sw_here(ck + s * CK);
#pragma unroll
        for (int k = 0; k < CW; ++k) sw_st(c + k * RT, bo, SW_X(k));
        if (cs == 0) {
            sw_st(c + (NC + 0) * RT, ro, G);
            sw_st(c + (NC + 1) * RT, ro, w);
            sw_st(c + (NC + 2) * RT, ro, D);
            sw_st(c + (NC + 3) * RT, ro, z);
        }
        sw_gen_seg<RT, NS>(b, r, Jr, Jc, ar, cr, ac, bc, cc, dc, t, n0, n1, rows, ro, cs);
        __syncthreads();              // the generator rows were written by all slabs
        c = sw_here(c);
#pragma unroll
        for (int k = 0; k < CW; ++k) SW_SETX(k, sw_ld(c + k * RT, bo));
        double nv = sw_ld(rows + RT, ro), nu = sw_ld(rows, ro), np = sw_ld(rows + 2 * RT, ro);
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            SW_LANE_OFFSETS;
            const double u = nu, v = nv, p = np;
            if (n + 1 < n1) {                          // the next row's generator values, one row ahead
                const double *rn = sw_here(rows + (n + 1 - n0) * RS);
                nv = sw_ld(rn + RT, ro); nu = sw_ld(rn, ro); np = sw_ld(rn + 2 * RT, ro);
            }
            const double An = (dg ? dg[n] : 0.0) + dadd;
            sw_fwd_row<RT, NS, CW, CL>(X, xl, xh, G, w, D, z, u, v, p, An, y[n], shm + (n & 1) * LDS, r, cs);
            if (!(D > 0.0)) { bad = n + 1; break; }
            quad += z * z / D;
            if (tid < 64) {                            // z and D of 64 rows in the lanes of wave 0, stored as one run
                const int slot = (int)(n & 63);        // (and at a segment's end, for its sum of log D)
                if (lane == slot) { zbuf = z; dbuf = D; }
                if (slot == 63 || n == n1 - 1) {
                    const int64_t i = (n - slot) + lane;
                    if (i <= n) { zw[i] = zbuf; Dw[i] = dbuf; }
                }
            }
        }
        if (bad) break;
        // sum log D over the segment's rows, in row order, outside the row loop (which then holds none of log's
        // constants): every thread adds the same values in the same order
        __syncthreads();
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) logdet += log(sw_ld(sw_here(Dw + n), 0u));
    }
    if (bad) {                                         // (D is the same in every thread: all of them leave)
        const double nan = __builtin_nan("");
        if (tid == 0) { ll[b] = -INFINITY; info[b] = (int32_t)bad; }
        for (int64_t i = tid; i < N; i += NT) {
            if (alpha) alpha[i] = nan;
            if (mu) mu[i] = nan;
        }
        return;
    }
    if (tid == 0) {
        ll[b] = -0.5 * (logdet + quad + (double)N * log(6.283185307179586));
        info[b] = 0;
    }

    // ---- pass 2: segments last first, each recomputed from its checkpoint staging (W_n, U_n, P_n), then the upper
    // solve over its rows in slab 0: thread r holds column r of H
    double H = 0.0, unext = 0.0, pnext = 0.0, anext = 0.0;       // (U, P, alpha of row n + 1: nothing beyond the end)
    double abuf = 0.0;
    #pragma unroll 1
    for (int64_t s = nseg - 1; s >= 0; --s) {
        SW_LANE_OFFSETS;
        const int64_t n0 = s * K, n1 = (n0 + K < N) ? n0 + K : N;
        const double *c = ck + s * CK;
        __syncthreads();              // the last segment's staged rows have been read (pass 1's: z, D are written)
        sw_gen_seg<RT, NS>(b, r, Jr, Jc, ar, cr, ac, bc, cc, dc, t, n0, n1, rows, ro, cs);
        __syncthreads();              // generator rows: written by all slabs; the checkpoint's vectors: by slab 0
        c = sw_here(c);
#pragma unroll
        for (int k = 0; k < CW; ++k) SW_SETX(k, sw_ld(c + k * RT, bo));
        G = sw_ld(c + (NC + 0) * RT, ro);
        w = sw_ld(c + (NC + 1) * RT, ro);
        D = sw_ld(c + (NC + 2) * RT, ro);
        z = sw_ld(c + (NC + 3) * RT, ro);
        #pragma unroll 1
        for (int64_t n = n0; n < n1; ++n) {
            SW_LANE_OFFSETS;
            double *rw = sw_here(rows + (n - n0) * RS);
            // (v first: the other slabs' threads of row r hold it until the row's end, where slab 0 overwrites it with
            // W_n; u and p, which every thread needs ahead of the row's second barrier, come in behind it)
            const double v = sw_ld(rw + RT, ro), u = sw_ld(rw, ro), p = sw_ld(rw + 2 * RT, ro);
            const double An = (dg ? dg[n] : 0.0) + dadd;
            sw_fwd_row<RT, NS, CW, CL>(X, xl, xh, G, w, D, z, u, v, p, An, y[n], shm + (n & 1) * LDS, r, cs);
            if (cs == 0) sw_st(rw + RT, ro, w);        // (in the backward rows thread r reads back what it wrote itself)
        }
        __syncthreads();              // LDS changes hands
        #pragma unroll 1
        for (int64_t n = n1 - 1; n >= n0; --n) {
            SW_LANE_OFFSETS;
            const int slot = (int)(n & 63);
            double part = 0.0, zn = 0.0, Dn = 1.0, un = 0.0, pn = 0.0;
            if (cs == 0) {
                const double *rw = sw_here(rows + (n - n0) * RS);
                un = sw_ld(rw, ro);
                const double wn = sw_ld(rw + RT, ro);
                pn = sw_ld(rw + 2 * RT, ro);
                if (slot == 63 || n == N - 1) {        // every wave of slab 0 holds its own copy of the 64 rows' z, D
                    const int64_t i = (n - slot) + lane;
                    zbuf = i <= n ? zw[i] : 0.0;
                    dbuf = i <= n ? Dw[i] : 1.0;
                }
                zn = read_lane(zbuf, slot);
                Dn = read_lane(dbuf, slot);
                H = pnext * fma(unext, anext, H);
                part = wave_sum(wn * H);
            }
            if (NRB > 1) {
                double *dots = shm + (n & 1) * LDS + (3 + NS) * RT;
                if (cs == 0 && lane == 0) dots[3 * (r >> 6) + 2] = part;
                wg_lds_barrier();
                if (cs == 0) {
                    part = dots[2];
#pragma unroll
                    for (int i = 1; i < NRB; ++i) part += dots[3 * i + 2];
                }
            }
            if (cs == 0) {
                const double a = zn / Dn - part;
                unext = un; pnext = pn; anext = a;
                if (tid < 64) {
                    if (lane == slot) abuf = a;
                    if (slot == 0) {
                        const int64_t i = n + lane;
                        if (i < N) stage_alpha(i, abuf, zw, alpha, mu, dg, y);
                    }
                }
            }
        }
    }
}

// opt the widest instance in to its dynamic LDS on the current device, once per device
bool sw_lds_opt_in(const void *fn, size_t bytes) {
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

int gf_solve_wide_max_width(void) { return SW_MAX_W; }

int64_t gf_solve_wide_seg(int64_t N, int W) {
    if (N < 1 || W < 1 || W > SW_MAX_W) return 0;
    return sw_pick_seg(N, W, 0);
}

int64_t gf_solve_wide_work(int64_t N, int W, int64_t seg) {
    if (N < 1 || W < 1 || W > SW_MAX_W || seg < 0) return 0;
    return sw_work(N, W, sw_pick_seg(N, W, seg));
}

int gf_solve_batch_wide(int B, int64_t N, int Jr, int Jc,
                        const double *ar, const double *cr, const double *ac, const double *bc,
                        const double *cc, const double *dc, const double *diag_add,
                        const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                        const double *y, int64_t y_bs, int64_t seg, double *work, int64_t work_bs,
                        double *alpha, double *mu, double *ll, int32_t *info, void *stream) {
    const int64_t W64 = (int64_t)Jr + 2 * (int64_t)Jc;
    if (B < 1 || N < 1 || seg < 0 || Jr < 0 || Jc < 0 || W64 < 1)
        return gf_internal_error(-1, "gf_solve_batch_wide: bad shape (B=%d, N=%lld, Jr=%d, Jc=%d, seg=%lld)", B,
                                 (long long)N, Jr, Jc, (long long)seg);
    if ((t_bs != 0 && t_bs < N) || (diag && diag_bs != 0 && diag_bs < N) || (y_bs != 0 && y_bs < N))
        return gf_internal_error(-1, "gf_solve_batch_wide: bad batch stride (t_bs=%lld, diag_bs=%lld, y_bs=%lld: 0 "
                                 "or at least N=%lld)", (long long)t_bs, (long long)diag_bs, (long long)y_bs,
                                 (long long)N);
    if (W64 > SW_MAX_W)
        return gf_internal_error(-3, "gf_solve_batch_wide: width W=%lld exceeds the workgroup limit %d",
                                 (long long)W64, SW_MAX_W);
    const int W = (int)W64;
    const int64_t K = sw_pick_seg(N, W, seg), nseg = (N + K - 1) / K;
    if (work_bs < sw_work(N, W, K))
        return gf_internal_error(-1, "gf_solve_batch_wide: work_bs=%lld < gf_solve_wide_work(N, W, seg)=%lld",
                                 (long long)work_bs, (long long)sw_work(N, W, K));
    if ((Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)) || !diag_add || !t || !y || !work || !ll || !info)
        return gf_internal_error(-1, "gf_solve_batch_wide: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const SwGeo g = sw_geo(W);
    const size_t lds = sw_lds_bytes(g);
    if (lds > 64 * 1024) {
        const void *fn[1] = {(const void *)k_solvew<192, 2, 96, SW_CL192>};    // (the one instance beyond 64 KB)
        if (!sw_lds_opt_in(fn[0], lds))
            return gf_internal_error(-1, "gf_solve_batch_wide: cannot opt in to %lld bytes of LDS", (long long)lds);
    }
#define SW_LAUNCH(RT, NS, CW, CL)                                                                                \
    hipLaunchKernelGGL((k_solvew<RT, NS, CW, CL>), dim3((unsigned)B), dim3((RT) * (NS)), lds, st, N, K, nseg, Jr, \
                       Jc, ar, cr, ac, bc, cc, dc, diag_add, t, t_bs, diag, diag_bs, y, y_bs, work, work_bs,     \
                       alpha, mu, ll, info)
    if (g.rt == 64) SW_LAUNCH(64, 2, 32, 0);
    else if (g.rt == 128) SW_LAUNCH(128, 2, 64, 0);
    else SW_LAUNCH(192, 2, 96, SW_CL192);
#undef SW_LAUNCH
    return gf_internal_check_launch("gf_solve_batch_wide");
}

}  // extern "C"
