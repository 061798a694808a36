// gadfly_stored.hip -- the sweeps on MATERIALISED rows: the generator rows are built into memory, the factorisation
// reads them and stores its rows, and the solves, products and conditional means sweep the stored factor.
//
// What is replaced: the celerite2 C++ driver routines behind gadfly's GaussianProcess
// (the reference's gadfly/gp.py:202,:232, :327, :350, :370, :391).
// The arithmetic follows SURVEY.md Appendix A.4-A.8.
//   k_build, k_factor          A.4 generator rows U, V (+ a, + propagator rows P); A.5 LDL^T recurrence, state S (W x W)
//                              in VGPRs, rows split over NW waves, optional fused forward solve (A.6)
//   k_build2, k_factor2        the same in block-scaled coordinates (no per-row decay), one wave, W <= 64
//   k_factor2w                 the block-scaled recurrence beyond one wave (64 < W <= 256)
//   k_scaled_propagator        propagator rows of a factor stored in block-scaled form, for the general-width sweeps
//   k_solve_vec, k_solve_rhs   A.6/A.7 sweeps on stored rows: one right-hand side lane-resident, or one lane each
//   k_gmm*, k_add2, k_cross    A.8 conditional mean at new times; cross-covariance block
// and the queries that describe these kernels' shapes: gf_leading_dim (the rows' leading dimension), gf_state_size /
// gf_state_cols (k_factor's and k_factor2w's state), gf_scaled_supported / gf_scaled_wide_supported (the widths of
// k_factor2 / k_factor2w), gf_scaled_span (k_build2's reset rule).
// Elsewhere: the fused sweeps, which never store a row (gadfly_hip.hip), and the chunk-parallel linear sweeps on the
// stored scaled factor (gadfly_linear.hip).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"

// sincos / exp with <= 1 ulp error for the argument ranges of k_build2 (validated against
// long-double libm by oracle/fastmath_check.c); ~4x fewer instructions than the general OCML
// routines, which carry Payne-Hanek reduction for arbitrary arguments.
#define FM_INLINE __device__ __forceinline__
#include "fastmath.h"
#include "gf_wave.h"
#include "gf_sweep.h"

namespace {

// ------------------------------------------------------------------------------------
// K0: generator rows + propagator rows
// ------------------------------------------------------------------------------------
struct BuildArgs {
    int64_t N, n_first;             // rows built: global n_first .. n_first + N - 1
    int Jr, Jc, ld, units;          // units per row = Jr + Jc + (ld - W)
    const double *ar, *cr, *ac, *bc, *cc, *dc, *diag_add;
    const double *t; int64_t t_bs;
    const double *diag; int64_t diag_bs;
    double *a, *U, *V, *P;
};

__global__ void __launch_bounds__(256) k_build(const BuildArgs A) {
    const int b = blockIdx.y;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = id / A.units;
    if (n >= A.N) return;
    const int q = (int)(id - n * A.units);
    const int W = A.Jr + 2 * A.Jc;
    const double *t = A.t + (size_t)b * A.t_bs;
    const int64_t ng = A.n_first + n;                // global row (t, diag are global arrays)
    const double tn = t[ng];
    const double dt = (ng > 0) ? (t[ng - 1] - tn) : 0.0;
    const size_t row = ((size_t)b * A.N + n) * A.ld;
    if (q == 0 && A.a) {
        const double dg = A.diag ? A.diag[(size_t)b * A.diag_bs + ng] : 0.0;
        A.a[(size_t)b * A.N + n] = dg + A.diag_add[b];
    }
    if (q < A.Jr) {                                  // real term: one column
        const double ar = A.ar[(size_t)b * A.Jr + q], cr = A.cr[(size_t)b * A.Jr + q];
        A.U[row + q] = ar;
        A.V[row + q] = 1.0;
        if (A.P) A.P[row + q] = (ng > 0) ? exp(cr * dt) : 1.0;
    } else if (q < A.Jr + A.Jc) {                    // complex term: two columns
        const int k = q - A.Jr;
        const size_t ck = (size_t)b * A.Jc + k;
        const double ac = A.ac[ck], bc = A.bc[ck], cc = A.cc[ck], dc = A.dc[ck];
        const double arg = dc * tn;                  // ONE rounded multiply (parity hazard i)
        double si, co;
        sincos(arg, &si, &co);
        const int j = A.Jr + 2 * k;
        A.U[row + j]     = ac * co + bc * si;
        A.U[row + j + 1] = ac * si - bc * co;
        A.V[row + j]     = co;
        A.V[row + j + 1] = si;
        if (A.P) {
            const double p = (ng > 0) ? exp(cc * dt) : 1.0;
            A.P[row + j] = p;
            A.P[row + j + 1] = p;
        }
    } else {                                         // pad column
        const int j = W + (q - A.Jr - A.Jc);
        A.U[row + j] = 0.0;
        A.V[row + j] = 0.0;
        if (A.P) A.P[row + j] = 1.0;
    }
}

// ------------------------------------------------------------------------------------
// K1: factor (+ fused forward solve).  One workgroup of NW waves per (problem, chunk).
//   thread (wave w, lane l) holds S[i][j] for rows i = w*RB + r (r < RB) and
//   columns j = c*64 + l (c < CT).  Per row n:
//     S   <- P_n (S + d_{n-1} w_{n-1} w_{n-1}^T) P_n      (fused with the mat-vec below)
//     tmp  = u_n^T S      (partial over this wave's rows; reduced across waves through LDS)
//     d_n  = a_n - tmp . u_n        (DPP tree)
//     w_n  = (v_n - tmp) / d_n
//   Row-indexed operands (u_i, p_i, w_i) are wave-uniform: each wave stages the lane-form
//   vectors in its private LDS slice and reads them back as broadcasts.
// ------------------------------------------------------------------------------------
struct FactorArgs {
    int64_t N, chunk_len, n_first;  // n_first: global index of row 0 (tile streaming), for info
    int W, ld;
    const double *a, *U, *V, *P;
    const double *y; int64_t y_bs;
    double *d, *Wm, *z;
    const double *S_in, *F_in;      // per (problem, chunk) state, or NULL = zero
    double *S_out, *F_out;          // or NULL
    int32_t *info;
};

template <int RB, int CT, int NW>
__global__ void __launch_bounds__(64 * NW) k_factor(const FactorArgs A) {
    constexpr int WPC = CT * 64;
    constexpr int RT = RB * NW;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.y, ch = blockIdx.x;
    const int nch = gridDim.x;
    const int64_t n0 = (int64_t)ch * A.chunk_len;
    const int64_t n1 = (n0 + A.chunk_len < A.N) ? (n0 + A.chunk_len) : A.N;
    const int ld = A.ld;
    const size_t pb = (size_t)b * A.N;
    const double *__restrict__ Ug = A.U + pb * ld;
    const double *__restrict__ Vg = A.V + pb * ld;
    const double *__restrict__ Pg = A.P + pb * ld;
    const double *__restrict__ ag = A.a + pb;
    const double *__restrict__ yg = A.y ? (A.y + (size_t)b * A.y_bs) : nullptr;

    __shared__ double s_part[2][NW][WPC];
    __shared__ double s_vec[NW][3][WPC];
    double *sv_u = s_vec[wave][0], *sv_p = s_vec[wave][1], *sv_w = s_vec[wave][2];

    double S[RB][CT];
    double Fv[CT], wv[CT];
    bool colok[CT];
    int colc[CT];                       // pad lanes read a clamped (valid) column and are masked at use
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        colok[c] = (c * 64 + lane) < ld;
        colc[c] = colok[c] ? (c * 64 + lane) : (ld - 1);
        wv[c] = 0.0;
        Fv[c] = 0.0;
    }
    const size_t sidx = (size_t)b * nch + ch;
    if (A.info[sidx] != 0) return;      // an earlier tile of this problem already failed
    if (A.S_in) {
        const double *Si = A.S_in + sidx * RT * WPC;
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int c = 0; c < CT; ++c) S[r][c] = Si[(size_t)(wave * RB + r) * WPC + c * 64 + lane];
        if (A.F_in) {
#pragma unroll
            for (int c = 0; c < CT; ++c) Fv[c] = A.F_in[sidx * WPC + c * 64 + lane];
        }
    } else {
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int c = 0; c < CT; ++c) S[r][c] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) sv_w[c * 64 + lane] = 0.0;

    double dprev = 0.0, zprev = 0.0;
    int32_t fail = 0;

    // software prefetch of row n0: plain unconditional loads that nothing touches before the row
    // is processed (a `colok ? load : 0` here makes the wave wait for HBM right where it issued the load)
    double un[CT], vn[CT], pn[CT], an, yn;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const size_t o = (size_t)n0 * ld + colc[c];
        un[c] = Ug[o];
        vn[c] = Vg[o];
        pn[c] = Pg[o];
    }
    // the per-row scalars travel in the vector-load queue too (opaque zero lane offset): a scalar load
    // would be waited for at the next LDS access, which shares its counter
    const int vz = __builtin_amdgcn_mbcnt_lo(0u, 0u);
    const double *__restrict__ ys = yg ? yg : ag;          // always a valid address; dropped below
    an = ag[n0 + vz];
    yn = ys[n0 + vz];

    for (int64_t n = n0; n < n1; ++n) {
        double u[CT], v[CT], p[CT];
        const double a_n = an, y_n = yg ? yn : 0.0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            u[c] = colok[c] ? un[c] : 0.0; v[c] = colok[c] ? vn[c] : 0.0; p[c] = colok[c] ? pn[c] : 1.0;
            sv_u[c * 64 + lane] = u[c];
            sv_p[c * 64 + lane] = p[c];
        }
        // prefetch the next row (clamped: the last iteration re-reads its own row)
        const int64_t nn = (n + 1 < n1) ? (n + 1) : n;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const size_t o = (size_t)nn * ld + colc[c];
            un[c] = Ug[o];
            vn[c] = Vg[o];
            pn[c] = Pg[o];
        }
        an = ag[nn + vz];
        yn = ys[nn + vz];

        wave_lds_fence();

        // fused: pending rank-1 update + decay, then the mat-vec partial for this wave's rows
        double acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0.0;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = wave * RB + r;
            const double ui = sv_u[i], pi = sv_p[i];
            const double wid = sv_w[i] * dprev;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const double s = (S[r][c] + wid * wv[c]) * (pi * p[c]);
                S[r][c] = s;
                acc[c] = fma(ui, s, acc[c]);
            }
        }
        double tmp[CT];
        if constexpr (NW > 1) {
            const int buf = (int)(n & 1);
#pragma unroll
            for (int c = 0; c < CT; ++c) s_part[buf][wave][c * 64 + lane] = acc[c];
            wg_lds_barrier();           // (not __syncthreads: the next row's prefetch stays in flight)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                double s = s_part[buf][0][c * 64 + lane];
#pragma unroll
                for (int w2 = 1; w2 < NW; ++w2) s += s_part[buf][w2][c * 64 + lane];
                tmp[c] = s;
            }
        } else {
#pragma unroll
            for (int c = 0; c < CT; ++c) tmp[c] = acc[c];
        }
        // F_n = P_n (F_{n-1} + w_{n-1} z_{n-1});  two dot products in one DPP tree
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            Fv[c] = p[c] * fma(wv[c], zprev, Fv[c]);
            s1 = fma(u[c], tmp[c], s1);
            s2 = fma(u[c], Fv[c], s2);
        }
        wave_sum2(s1, s2);
        const double dn = a_n - s1;
        const double zn = y_n - s2;
        if (!(dn > 0.0)) {              // uniform across the whole workgroup
            const int64_t ng = A.n_first + n + 1;
            fail = (int32_t)(ng > 0x7fffffff ? 0x7fffffff : ng);
            break;
        }
        const double inv_dn = fast_rcp(dn);     // one reciprocal (<= 1 ulp) instead of CT IEEE divisions
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            wv[c] = (v[c] - tmp[c]) * inv_dn;
            sv_w[c * 64 + lane] = wv[c];
        }
        if (wave == 0) {
            if (A.Wm) {
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    if (colok[c]) A.Wm[(pb + n) * ld + c * 64 + lane] = wv[c];
            }
            if (lane == 0) {
                A.d[pb + n] = dn;
                if (A.z) A.z[pb + n] = zn;
            }
        }
        dprev = dn;
        zprev = zn;
    }

    if (fail && wave == 0 && lane == 0) A.info[sidx] = fail;
    if (fail) return;

    if (A.S_out) {                      // state handed to the next chunk: pending update, no decay
        wave_lds_fence();
        double *So = A.S_out + sidx * RT * WPC;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = wave * RB + r;
            const double wid = sv_w[i] * dprev;
#pragma unroll
            for (int c = 0; c < CT; ++c) So[(size_t)i * WPC + c * 64 + lane] = fma(wid, wv[c], S[r][c]);
        }
        if (A.F_out && wave == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) A.F_out[sidx * WPC + c * 64 + lane] = fma(wv[c], zprev, Fv[c]);
        }
    }
}

// ------------------------------------------------------------------------------------
// v2 log-likelihood path (W <= 64): block-scaled coordinates, one wave per problem.
//
// Within a block of rows [r, r') (r = "reset row") the state is kept in coordinates scaled by
// rho_n = exp(-c (t_n - t_r)):   S_n = rho_n T_n rho_n,  u~_n = u_n o rho_n,  v~_n = v_n / rho_n,
// w~_n = w_n / rho_n.  In these coordinates the celerite recurrence has NO per-row decay:
//     T   <- T + d_{n-1} w~_{n-1} w~_{n-1}^T
//     tmp  = T u~_n ;  d_n = a_n - u~_n . tmp ;  w~_n = (v~_n - tmp) / d_n
//     F~  <- F~ + w~_{n-1} z_{n-1} ;  z_n = y_n - u~_n . F~
// i.e. 2 FMAs per element of T per row instead of an update, two decays and a mat-vec.  At a
// reset row the accumulated decay E = exp(-c (t_r' - t_r)) is applied once (T <- E T E).  This is
// the un-preconditioned celerite (2017) recurrence made safe by bounding the block span:
// reset(n) = (n % 8 == 0) or cmax (t_n - t_{n-1}) > 4  =>  |log rho| <= 28 inside a block.
// k_build2 writes u~, v~ (and E at reset rows); k_factor2 reads the row operands u~_i as
// wave-uniform scalar loads (SGPR operands of v_fma_f64), so only w~ needs an LDS broadcast.
// ------------------------------------------------------------------------------------
struct Build2Args {
    int64_t N, n_first;
    int Jr, Jc, ld, units, block;   // block: power of two, rows between forced resets
    double gap;                     // cmax * dt above which a row is a reset of its own
    const double *ar, *cr, *ac, *bc, *cc, *dc, *diag_add, *cmax;
    const double *t; int64_t t_bs;
    const double *diag; int64_t diag_bs;
    double *a, *Ut, *Vt, *de;       // de[n] = t_ref(n) - t_ref(n-1) at reset rows, -1 elsewhere
};

__device__ __forceinline__ bool sc_is_reset(const double *t, int64_t g, double cmax, int block,
                                            double gap) {
    return (g & (block - 1)) == 0 || cmax * (t[g] - t[g - 1]) > gap;
}

// latest reset row <= g (bounded walk: g - g % block is always a reset)
__device__ __forceinline__ int64_t sc_ref(const double *t, int64_t g, double cmax, int block,
                                          double gap) {
    while (!sc_is_reset(t, g, cmax, block, gap)) --g;
    return g;
}

constexpr int B2_ROWS = 32;         // rows per workgroup of k_build2

__global__ void __launch_bounds__(256) k_build2(const Build2Args A) {
    const int b = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * B2_ROWS;          // first tile-local row of the block
    const int nrows = (int)((A.N - n0 < B2_ROWS) ? (A.N - n0) : B2_ROWS);
    const int W = A.Jr + 2 * A.Jc;
    const double *t = A.t + (size_t)b * A.t_bs;
    const double cmax = A.cmax[b];

    // phase 1: one thread per row -- reset rule, distance to the block reference, block decay
    __shared__ double s_t[B2_ROWS], s_ds[B2_ROWS];
    if ((int)threadIdx.x < nrows) {
        const int r = threadIdx.x;
        const int64_t g = A.n_first + n0 + r;
        const double tn = t[g];
        const bool reset = sc_is_reset(t, g, cmax, A.block, A.gap);
        const int64_t ref = reset ? g : sc_ref(t, g, cmax, A.block, A.gap);
        const double de = reset ? ((g > 0) ? (tn - t[sc_ref(t, g - 1, cmax, A.block, A.gap)]) : 0.0)
                                : -1.0;
        s_t[r] = tn;
        s_ds[r] = tn - t[ref];                                   // >= 0, 0 at a reset row
        const size_t o = (size_t)b * A.N + n0 + r;
        const double dg = A.diag ? A.diag[(size_t)b * A.diag_bs + g] : 0.0;
        A.a[o] = dg + A.diag_add[b];
        A.de[o] = de;
    }
    __syncthreads();

    // phase 2: one thread per (row, term); the first (ld - W) units of a row also zero a pad column
    const unsigned units = (unsigned)(A.Jr + A.Jc);
    const unsigned total = (unsigned)nrows * units;
    const int npad = A.ld - W;
    for (unsigned idx = threadIdx.x; idx < total; idx += 256) {
        const unsigned r = idx / units;
        const int q = (int)(idx - r * units);
        const double tn = s_t[r], ds = s_ds[r];
        const size_t row = ((size_t)b * A.N + n0 + r) * A.ld;
        if (q < A.Jr) {
            const double ar = A.ar[(size_t)b * A.Jr + q], cr = A.cr[(size_t)b * A.Jr + q];
            const double rho = fm_exp(-cr * ds);
            A.Ut[row + q] = ar * rho;
            A.Vt[row + q] = 1.0 / rho;
        } else {
            const int k = q - A.Jr;
            const size_t ck = (size_t)b * A.Jc + k;
            const double ac = A.ac[ck], bc = A.bc[ck], cc = A.cc[ck], dc = A.dc[ck];
            const double arg = dc * tn;              // ONE rounded multiply (parity hazard i)
            double si, co;
            if (fabs(arg) < FM_SINCOS_RANGE) fm_sincos(arg, &si, &co);
            else sincos(arg, &si, &co);                        // e.g. JD-based time axes
            const double rho = fm_exp(-cc * ds), irho = 1.0 / rho;
            const int j = A.Jr + 2 * k;
            double2 u2, v2;
            u2.x = (ac * co + bc * si) * rho;
            u2.y = (ac * si - bc * co) * rho;
            v2.x = co * irho;
            v2.y = si * irho;
            if ((j & 1) == 0) {                      // 16-byte aligned pair
                *reinterpret_cast<double2 *>(A.Ut + row + j) = u2;
                *reinterpret_cast<double2 *>(A.Vt + row + j) = v2;
            } else {
                A.Ut[row + j] = u2.x; A.Ut[row + j + 1] = u2.y;
                A.Vt[row + j] = v2.x; A.Vt[row + j + 1] = v2.y;
            }
        }
        if (q < npad) {
            A.Ut[row + W + q] = 0.0;
            A.Vt[row + W + q] = 0.0;
        }
    }
    // more pad columns than units (tiny kernels only)
    if (npad > (int)units) {
        for (unsigned idx = threadIdx.x; idx < (unsigned)nrows * (unsigned)npad; idx += 256) {
            const unsigned r = idx / (unsigned)npad;
            const int q = (int)(idx - r * (unsigned)npad);
            const size_t row = ((size_t)b * A.N + n0 + r) * A.ld;
            A.Ut[row + W + q] = 0.0;
            A.Vt[row + W + q] = 0.0;
        }
    }
}

// Per row n (scaled coordinates; r = v~ - tmp, so w~ = r/d and d w~ = r):
//     sweep :  T_i += r_{n-1,i} * q_{n-1}  (q = r/d, lane-form) ;  tmp = sum_i u~_{n,i} T_i
//     r_n = v~_n - tmp ;  stage r_n and u~_{n+1} in LDS, start reading the next row's operands
//     d_n = a_n - u~_n . tmp ;  z_n = y_n - u~_n . F~ ;  q_n = r_n / d_n
// The division and the DPP reduction sit between two sweeps; staging r (not w~) lets the LDS
// traffic of the next sweep start before they finish.
// Forward solve for free (W < 64): lane 63 is a pad column of T; loading it with F~ (as
// T[i][63] = F~_i) and giving it the multiplier q_63 = z/d makes the sweep's rank-1 update
// perform F~ += r z/d and its mat-vec return u~ . F~ in lane 63's partial sum, so the
// solve needs neither its own recurrence nor a second DPP reduction.
template <int ROWS>
__global__ void __launch_bounds__(64, 2)     // 2 waves/SIMD: one wave alone gets half the VALU issue rate
k_factor2(const int64_t N, const int64_t n_first, const int ld, const int W,
          const double *__restrict__ c_,
          const double *__restrict__ a_, const double *__restrict__ Ut_,
          const double *__restrict__ Vt_, const double *__restrict__ de_,
          const double *__restrict__ y_, const int64_t y_bs,
          double *__restrict__ d_, double *__restrict__ z_,
          double *__restrict__ S_state, double *__restrict__ F_state,
          int32_t *__restrict__ info) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    if (info[b] != 0) return;
    const size_t pb = (size_t)b * N;
    const double *__restrict__ ag = a_ + pb;
    const double *__restrict__ Ug = Ut_ + pb * ld;
    const double *__restrict__ Vg = Vt_ + pb * ld;
    const double *__restrict__ eg = de_ + pb;
    const double *__restrict__ yg = y_ + (size_t)b * y_bs;
    double *__restrict__ dg = d_ + pb;
    double *__restrict__ zg = z_ + pb;
    // state layout [lane][64 rows]: one base address per lane, immediate offsets per row
    double *__restrict__ Sg = S_state + (size_t)b * (64 * 64) + (size_t)lane * 64;
    double *__restrict__ Fg = F_state + (size_t)b * 64;

    __shared__ double s_w[64];      // r_{n-1}  (pending rank-1 update, row form)
    __shared__ double s_u[64];      // u~_n
    __shared__ double s_e[64];      // block decay E at reset rows
    const bool colok = lane < ld;
    const double cj = (lane < W) ? c_[(size_t)b * W + lane] : 0.0;

    // PADF: the forward solve rides in pad lane 63 (needs W < 64, i.e. ld <= 64 and lane 63 unused)
    const bool PADF = (ROWS < 64) || (W < 64);   // compile-time true except for ROWS == 64
    const bool fl = PADF && lane == 63;
    double T[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) T[i] = Sg[i];
    double Fv = Fg[lane];                       // only used when !PADF
    if (PADF) {
        // F~ (row form in F_state) becomes lane 63's column of T
#pragma unroll
        for (int i = 0; i < ROWS; ++i) T[i] = fl ? Fg[i] : T[i];
    }
    double rprev = 0.0, q = 0.0, zq = 0.0;      // pending: T += r r^T/d, F~ += r z/d
    int32_t fail = 0;

    // Everything a row needs is prefetched two rows ahead, unconditionally (the caller pads
    // every buffer, y included, by two rows/elements): a clamped index makes hipcc give up its
    // scalarisation of uniform loads, and an un-prefetched scalar costs a full memory round
    // trip per row.  Pad lanes (>= ld) re-read column ld-1 and are masked in registers.
    const int lanec = colok ? lane : (ld - 1);
    double ut_n = Ug[lanec], ut_n2 = Ug[ld + lanec];
    double vt_n = Vg[lanec], vt_n2 = Vg[ld + lanec];
    double a_nx = ag[0], y_nx = yg[0], e_nx = eg[0];
    double a_nx2 = ag[1], y_nx2 = yg[1], e_nx2 = eg[1];

    double ab[SW_AHEAD + 1][SW_BR], wb[SW_AHEAD + 1][SW_BR];
    s_w[lane] = 0.0;
    s_u[lane] = colok ? ut_n : 0.0;
    wave_lds_fence();
    sweep_preload<ROWS>(ab, wb, s_u, s_w);

    for (int64_t n = 0; n < N; ++n) {
        const double ut = colok ? ut_n : 0.0, vt = colok ? vt_n : 0.0;
        const double a_n = a_nx, y_n = y_nx, e_n = e_nx;
        ut_n = ut_n2; vt_n = vt_n2; a_nx = a_nx2; y_nx = y_nx2; e_nx = e_nx2;
        ut_n2 = Ug[(size_t)(n + 2) * ld + lanec];
        vt_n2 = Vg[(size_t)(n + 2) * ld + lanec];
        a_nx2 = ag[n + 2];
        y_nx2 = yg[n + 2];
        e_nx2 = eg[n + 2];
        if (e_n >= 0.0) {                   // wave-uniform: reset row
            // fold the pending update, then decay by E = exp(-c * de) (de = t_ref - t_ref_prev)
            const double el = colok ? exp(-cj * e_n) : 1.0;
            s_e[lane] = el;
            wave_lds_fence();
            sweep_preload<ROWS>(ab, wb, s_e, s_w);      // ring reused, re-fetched below
            (void)sweep_run<ROWS, true>(T, ab, wb, s_e, s_w, q, el);
            sweep_preload<ROWS>(ab, wb, s_u, s_w);
            Fv = el * fma(rprev, zq, Fv);
            q = 0.0;
            zq = 0.0;
        }
        const double tmp = sweep_run<ROWS, false>(T, ab, wb, s_u, s_w, q, 0.0);
        const double r = fl ? 0.0 : (vt - tmp); // pad lanes: 0 - 0; lane 63 carries u~ . F~
        Fv = fma(rprev, zq, Fv);
        // stage the next row's operands and start fetching them under the reduction
        wave_lds_fence();
        s_w[lane] = r;
        s_u[lane] = colok ? ut_n : 0.0;
        wave_lds_fence();
        sweep_preload<ROWS>(ab, wb, s_u, s_w);
        double s1 = ut * tmp, s2;
        if (PADF) {                             // wave-uniform
            s1 = wave_sum(s1);                  // ut = 0 in lane 63
            s2 = read_lane(tmp, 63);
        } else {
            s2 = ut * Fv;
            wave_sum2(s1, s2);
        }
        const double dn = a_n - s1;
        const double zn = y_n - s2;
        if (!(dn > 0.0)) {
            const int64_t gg = n_first + n + 1;
            fail = (int32_t)(gg > 0x7fffffff ? 0x7fffffff : gg);
            break;
        }
        const double inv = 1.0 / dn;
        zq = zn * inv;
        q = fl ? zq : r * inv;
        rprev = r;
        if (lane == 0) { dg[n] = dn; zg[n] = zn; }
    }
    if (fail) {
        if (lane == 0) info[b] = fail;
        return;
    }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const double v = fma(s_w[i], q, T[i]);
        if (fl) Fg[i] = v; else Sg[i] = v;
    }
    if (!PADF) Fg[lane] = fma(rprev, zq, Fv);
}

// ------------------------------------------------------------------------------------
// K2/K3/K4 with ONE right-hand side: F lane-resident (column j = c*64 + lane), one wave
// per problem, one DPP tree per row.
// ------------------------------------------------------------------------------------
struct SolveArgs {
    int64_t N;
    int W, ld, R, mode;
    const double *U, *Wm, *P, *scale, *Y;
    double *Z;
    // chunk mode of k_solve_vec (gf_solve_chunk): the grid is (problem, chunk); chunk c sweeps its rows
    // from the state in F_state slot (problem * nch + c) -- [ld] doubles, pending push folded, the decay
    // of the boundary left to the receiving chunk -- and leaves its end state there; store = 0: no Z
    int64_t chunk_len;
    int nch, store;
    double *F_state;
};

// MODE and SCALED are compile-time (the three sweeps x with / without the per-row scale): no
// branches on the chain.  CT = 3 covers the full solar kernel (W = 172, ld = 176).
template <int CT, int MODE, bool SCALED>
__global__ void __launch_bounds__(64) k_solve_vec(const SolveArgs A) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x / A.nch, ch = blockIdx.x - b * A.nch;     // (problem, chunk); nch = 1: whole series
    const int64_t N = A.N;
    const int ld = A.ld;
    const size_t pb = (size_t)b * N;
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int64_t L = (N - c0 < A.chunk_len) ? (N - c0) : A.chunk_len;         // rows of this chunk
    constexpr bool up = (MODE == GF_SOLVE_UPPER);
    constexpr bool mm = (MODE == GF_MATMUL_LOWER);
    // "push" rows multiply the carried value into F; "pull" rows are dotted with F
    const double *__restrict__ push = (up ? A.U : A.Wm) + pb * ld;
    const double *__restrict__ pull = (up ? A.Wm : A.U) + pb * ld;
    const double *__restrict__ Pg = A.P + pb * ld;
    const double *Y = A.Y + pb;         // (Z may alias Y: rows are read ahead of, never behind, the writes)
    const double *__restrict__ sc = SCALED ? A.scale + pb : nullptr;
    double *Z = A.Z + pb;
    // The sweep is one dependent chain per row (two FMAs, a 64-lane reduction: a few hundred cycles),
    // so a row's operands -- three generator rows, y, the scale -- must already be in registers when
    // the chain reaches it.  They are fetched DEPTH rows ahead into a register ring, by plain
    // unconditional vector loads that nothing touches until the row is processed: pad lanes read a
    // clamped column and are switched off by a 0/1 factor on P, the per-row scalars go through the
    // same (in-order) vector-load queue via an opaque zero lane offset instead of scalar loads the
    // wave would have to wait for on the spot.  Without the ring every row waited for its own HBM
    // round trip: 1.6 us per row.
    constexpr int DEPTH = 8;
    const int vz = __builtin_amdgcn_mbcnt_lo(0u, 0u);      // 0 in every lane, not known to be uniform
    int col[CT];
    double okf[CT], F[CT];
    double *__restrict__ Fs = A.F_state ? A.F_state + (size_t)blockIdx.x * ld : nullptr;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int j = c * 64 + lane;
        col[c] = j < ld ? j : ld - 1;
        okf[c] = j < ld ? 1.0 : 0.0;
        F[c] = Fs ? Fs[col[c]] * okf[c] : 0.0;
    }
    auto row_of = [&](const int64_t s) { return up ? (c0 + L - 1 - s) : (c0 + s); };
    auto scaled = [&](const double yv, const double sv) {
        if constexpr (SCALED) return mm ? yv * sqrt(sv) : yv / sv;
        else return yv;
    };

    // the first row of the sweep carries nothing itself (carry = 0): the state handed over already holds
    // the pending push of the row before it (F = 0 at the very start).  The decay of a chunk boundary is
    // applied by the chunk that OWNS the boundary row -- its first row: ascending sweeps apply it on entry
    // (the first processed row), the descending sweep on exit, so that the homogeneous part of a chunk is
    // exactly its closed-loop transition Phi_c (Phi_c^T going down), as in k_lin1.
    double carry = 0.0;
    double rp[DEPTH][CT], ra[DEPTH][CT], rb[DEPTH][CT], ry[DEPTH], rs[DEPTH];
    auto clampN = [&](const int64_t n) { return n < 0 ? (int64_t)0 : (n > N - 1 ? N - 1 : n); };
    auto fetch = [&](const int slot, int64_t s) {
        s = s < L ? s : L - 1;                      // past the end: re-read the last row, never used
        const int64_t n = row_of(s);
        const int64_t prev = clampN(up ? (n + 1) : (n - 1));    // (rows outside the series: multiplied by 0)
        const int64_t prow = clampN(up ? (n + 1) : n);
        ry[slot] = Y[n + vz];
        rs[slot] = SCALED ? sc[n + vz] : 1.0;
        const bool entry = up && Fs != nullptr && s == 0;      // descending chunk entry: no decay here
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            rp[slot][c] = entry ? 1.0 : Pg[(size_t)prow * ld + col[c]];
            ra[slot][c] = push[(size_t)prev * ld + col[c]];
            rb[slot][c] = pull[(size_t)n * ld + col[c]];
        }
    };
    auto process = [&](const int64_t s, const double (&p)[CT], const double (&a)[CT],
                       const double (&q)[CT], const double yv, const double sv) {
        const int64_t n = row_of(s);
        const double yn = scaled(yv, sv);
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            F[c] = (p[c] * okf[c]) * fma(a[c], carry, F[c]);
            dot = fma(q[c], F[c], dot);
        }
        dot = wave_sum(dot);
        const double zn = mm ? (yn + dot) : (yn - dot);
        if (A.store && lane == 0) Z[n] = zn;
        carry = mm ? yn : zn;
    };
    int64_t s0 = 0;
    if (L >= DEPTH) {
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) fetch(k, k);
        for (; s0 + DEPTH <= L; s0 += DEPTH) {
#pragma unroll
            for (int k = 0; k < DEPTH; ++k) {
                process(s0 + k, rp[k], ra[k], rb[k], ry[k], rs[k]);
                fetch(k, s0 + k + DEPTH);
            }
        }
    }
    for (; s0 < L; ++s0) {                          // fewer than DEPTH rows left
        fetch(0, s0);
        process(s0, rp[0], ra[0], rb[0], ry[0], rs[0]);
    }
    if (Fs) {                                       // end state: pending push folded, no decay
        const int64_t last = row_of(L - 1);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const double a = push[(size_t)last * ld + col[c]];
            double v = fma(a, carry, F[c]);
            if (up) v *= Pg[(size_t)last * ld + col[c]];       // cross the chunk's first-row boundary
            if (c * 64 + lane < ld) Fs[c * 64 + lane] = v;
        }
    }
}

// ------------------------------------------------------------------------------------
// K2/K3/K4 with R right-hand sides: lane r of a wave owns column r of Y/Z and the W-vector
// F[:, r] in VGPRs; the generator rows are wave-uniform operands (prefetched by vector loads,
// broadcast through LDS).  Widths above 64 split j over NWV waves (one LDS exchange/row).
// ------------------------------------------------------------------------------------
template <int JB, int NWV>
__global__ void __launch_bounds__(64 * NWV) k_solve_rhs(const SolveArgs A) {
    static_assert(JB % 2 == 0 && JB <= 64, "column slice: even, at most one wave wide");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // (problem, chunk): nch = 1 is the whole series; chunk mode (F_state != nullptr) as in k_solve_vec --
    // start state in, end state out (pending push folded; ascending sweeps apply a boundary's decay on
    // entry, the descending one on exit), Z only when A.store
    const int b = blockIdx.y / A.nch, ch = blockIdx.y - b * A.nch;
    const int r = blockIdx.x * 64 + lane;
    const int R = A.R;
    const bool rok = r < R;
    const int rc = rok ? r : (R - 1);   // idle lanes re-read the last right-hand side, never store
    const int64_t N = A.N;
    const int ld = A.ld;
    const size_t pb = (size_t)b * N;
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int64_t L = (N - c0 < A.chunk_len) ? (N - c0) : A.chunk_len;
    const bool up = (A.mode == GF_SOLVE_UPPER);
    const bool mm = (A.mode == GF_MATMUL_LOWER);
    const double *__restrict__ push = (up ? A.U : A.Wm) + pb * ld;
    const double *__restrict__ pull = (up ? A.Wm : A.U) + pb * ld;
    const double *__restrict__ Pg = A.P + pb * ld;
    const double *Y = A.Y + pb * R;     // (Z may alias Y: rows are read ahead of, never behind, the writes)
    const double *__restrict__ sc = A.scale ? A.scale + pb : nullptr;
    double *Z = A.Z + pb * R;
    double *__restrict__ Fs = A.F_state ? A.F_state + (size_t)blockIdx.y * ld * R : nullptr;     // [ld][R]
    const int j0 = wave * JB;
    int jn = ld - j0;                    // valid columns in this wave's slice
    if (jn > JB) jn = JB;
    if (jn < 0) jn = 0;
    // The generator rows of this wave's slice are wave-uniform operands of the per-lane recurrences.
    // Lane l fetches column j0 + l of the three rows DEPTH rows ahead (plain vector loads into a
    // register ring), the row being processed is staged in LDS and read back as broadcasts.  (As
    // scalar loads issued when the row needed them, they cost a memory round trip per row: 5.6 us
    // per row at W = 172.)
    constexpr int DEPTH = 8;
    const bool lok = lane < jn;
    const int jl = j0 + (lok ? lane : (jn > 0 ? jn - 1 : 0));
    const int jc = jl < ld ? jl : ld - 1;
    const int vz = __builtin_amdgcn_mbcnt_lo(0u, 0u);

    __shared__ __attribute__((aligned(16))) double s_row[NWV][3][64];
    __shared__ double s_dot[2][NWV][64];
    double *sp = s_row[wave][0], *sa = s_row[wave][1], *sb = s_row[wave][2];

    double F[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) F[j] = (Fs && j < jn) ? Fs[(size_t)(j0 + j) * R + rc] : 0.0;
    auto row_of = [&](const int64_t s) { return up ? (c0 + L - 1 - s) : (c0 + s); };
    auto scaled = [&](const double yv, const double sv) {
        return sc ? (mm ? yv * sqrt(sv) : yv / sv) : yv;
    };
    // the first row of the sweep carries nothing itself: the state handed over already holds the pending
    // push of the row before it (zero at the very start)
    double carry = 0.0;
    double rp[DEPTH], ra[DEPTH], rb[DEPTH], ry[DEPTH], rs[DEPTH];
    auto clampN = [&](const int64_t n) { return n < 0 ? (int64_t)0 : (n > N - 1 ? N - 1 : n); };
    auto fetch = [&](const int slot, int64_t s) {
        s = s < L ? s : L - 1;                      // past the end: re-read the last row, never used
        const int64_t n = row_of(s);
        const int64_t prev = clampN(up ? (n + 1) : (n - 1));    // (rows outside the series: multiplied by 0)
        const int64_t prow = clampN(up ? (n + 1) : n);
        ry[slot] = Y[(size_t)n * R + rc];
        rs[slot] = sc ? sc[n + vz] : 1.0;
        const bool entry = up && Fs != nullptr && s == 0;      // descending chunk entry: no decay here
        rp[slot] = entry ? 1.0 : Pg[(size_t)prow * ld + jc];
        ra[slot] = push[(size_t)prev * ld + jc];
        rb[slot] = pull[(size_t)n * ld + jc];
    };
    auto process = [&](const int64_t s, const double pv, const double av, const double bv,
                       const double yv, const double sv) {
        const int64_t n = row_of(s);
        const double yn = scaled(yv, sv);
        wave_lds_fence();                           // the previous row's broadcasts are done
        sp[lane] = lok ? pv : 0.0;                  // columns past the slice: all zero, F stays 0
        sa[lane] = lok ? av : 0.0;
        sb[lane] = lok ? bv : 0.0;
        wave_lds_fence();
        double dot = 0.0;
#pragma unroll
        for (int j = 0; j < JB; j += 2) {
            const double2 p2 = *(const double2 *)(sp + j), a2 = *(const double2 *)(sa + j);
            const double2 b2 = *(const double2 *)(sb + j);
            F[j] = p2.x * fma(a2.x, carry, F[j]);
            F[j + 1] = p2.y * fma(a2.y, carry, F[j + 1]);
            dot = fma(b2.x, F[j], dot);
            dot = fma(b2.y, F[j + 1], dot);
        }
        if constexpr (NWV > 1) {
            const int buf = (int)(s & 1);
            s_dot[buf][wave][lane] = dot;
            wg_lds_barrier();
            dot = s_dot[buf][0][lane];
#pragma unroll
            for (int w2 = 1; w2 < NWV; ++w2) dot += s_dot[buf][w2][lane];
        }
        const double zn = mm ? (yn + dot) : (yn - dot);
        if (A.store && rok && wave == 0) Z[(size_t)n * R + r] = zn;
        carry = mm ? yn : zn;
    };
    int64_t s0 = 0;
    if (L >= DEPTH) {
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) fetch(k, k);
        for (; s0 + DEPTH <= L; s0 += DEPTH) {
#pragma unroll
            for (int k = 0; k < DEPTH; ++k) {
                process(s0 + k, rp[k], ra[k], rb[k], ry[k], rs[k]);
                fetch(k, s0 + k + DEPTH);
            }
        }
    }
    for (; s0 < L; ++s0) {                          // fewer than DEPTH rows left
        fetch(0, s0);
        process(s0, rp[0], ra[0], rb[0], ry[0], rs[0]);
    }
    if (Fs) {                                       // end state: pending push folded, no decay
        const int64_t last = row_of(L - 1);
        wave_lds_fence();
        sa[lane] = lok ? push[(size_t)last * ld + jc] : 0.0;
        sp[lane] = (lok && up) ? Pg[(size_t)last * ld + jc] : 1.0;     // cross the chunk's first-row boundary
        wave_lds_fence();
        if (rok) {
#pragma unroll
            for (int j = 0; j < JB; ++j)
                if (j < jn) Fs[(size_t)(j0 + j) * R + r] = sp[j] * fma(sa[j], carry, F[j]);
        }
    }
}

// ------------------------------------------------------------------------------------
// K5: conditional mean at new times.  One wave per (problem, direction);
// F lane-resident; consecutive observed rows advance with the stored propagator rows P2,
// only the hop from the last observed row to the query time needs an exp.
//   dir 0 (lower): ascending;  dir 1 (upper): descending.  Partial results go to work[dir].
// ------------------------------------------------------------------------------------
struct GmmArgs {
    int64_t M, N;
    int W, ld;
    const double *c;
    const double *t1; int64_t t1_bs;
    const double *U1, *V1;
    const double *t2; int64_t t2_bs;
    const double *U2, *V2, *P2, *alpha;
    const int64_t *qidx;            // [B][M]: number of observed rows with t2 <= t1[m]
    double *work;
};

// Rows are streamed in unrolled blocks of GB (all loads of a block are issued before its
// FMAs: one dependent FMA per row instead of one memory round trip per row); a query is
// emitted when the sweep passes its row:  lower: after row qidx-1;  upper: after row qidx.
template <int CT>
__global__ void __launch_bounds__(64) k_gmm(const GmmArgs A) {
    constexpr int GB = 8;
    const int lane = threadIdx.x, b = blockIdx.x, dir = blockIdx.y;
    const int64_t M = A.M, N = A.N;
    const int ld = A.ld;
    const double *t1 = A.t1 + (size_t)b * A.t1_bs;
    const double *t2 = A.t2 + (size_t)b * A.t2_bs;
    const double *__restrict__ Q1 = (dir == 0 ? A.U1 : A.V1) + (size_t)b * M * ld;   // query-side rows
    const double *__restrict__ G2 = (dir == 0 ? A.V2 : A.U2) + (size_t)b * N * ld;   // data-side rows
    const double *__restrict__ P2 = A.P2 + (size_t)b * N * ld;
    const double *__restrict__ al = A.alpha + (size_t)b * N;
    const int64_t *__restrict__ qi = A.qidx + (size_t)b * M;
    double *out = A.work + ((size_t)b * 2 + dir) * M;
    bool colok[CT];
    int col[CT];
    double F[CT], cj[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int j = c * 64 + lane;
        colok[c] = j < A.W;
        col[c] = colok[c] ? j : 0;      // pad lanes re-read column 0 and are masked in registers
        F[c] = 0.0;
        cj[c] = colok[c] ? A.c[(size_t)b * A.W + j] : 0.0;
    }
    auto emit = [&](int64_t m, double tdata) {
        const double dt = (dir == 0) ? (tdata - t1[m]) : (t1[m] - tdata);   // <= 0
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (colok[c]) acc = fma(Q1[(size_t)m * ld + col[c]] * exp(cj[c] * dt), F[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) out[m] = acc;
    };
    if (dir == 0) {
        int64_t m = 0;
        while (m < M && qi[m] == 0) { if (lane == 0) out[m] = 0.0; ++m; }
        int64_t next = (m < M) ? qi[m] : (N + 1);          // emit after row next-1
        int64_t n = 0;
        for (; n + GB <= N; n += GB) {
            double pr[GB][CT], gr[GB][CT], an[GB];
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                an[k] = al[n + k];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const size_t o = (size_t)(n + k) * ld + col[c];
                    pr[k][c] = P2[o];                       // exp(c (t2[n-1] - t2[n])); row 0: 1
                    gr[k][c] = G2[o];
                }
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
#pragma unroll
                for (int c = 0; c < CT; ++c) F[c] = colok[c] ? fma(pr[k][c], F[c], gr[k][c] * an[k]) : 0.0;
                while (next == n + k + 1) {                 // wave-uniform, rare
                    emit(m, t2[n + k]);
                    ++m;
                    next = (m < M) ? qi[m] : (N + 1);
                }
            }
        }
        for (; n < N; ++n) {
            const double a1 = al[n];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const size_t o = (size_t)n * ld + col[c];
                F[c] = colok[c] ? fma(P2[o], F[c], G2[o] * a1) : 0.0;
            }
            while (next == n + 1) {
                emit(m, t2[n]);
                ++m;
                next = (m < M) ? qi[m] : (N + 1);
            }
        }
    } else {
        int64_t m = M - 1;
        while (m >= 0 && qi[m] == N) { if (lane == 0) out[m] = 0.0; --m; }
        int64_t next = (m >= 0) ? qi[m] : -1;               // emit after row next (descending)
        int64_t n = N - 1;
        for (; n - GB + 1 >= 0; n -= GB) {
            double pr[GB][CT], gr[GB][CT], an[GB];
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                const int64_t r = n - k;
                an[k] = al[r];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const size_t o = (size_t)r * ld + col[c];
                    // exp(c (t2[r] - t2[r+1])) is propagator row r+1 (the last row decays nothing)
                    pr[k][c] = (r + 1 < N) ? P2[o + ld] : 1.0;
                    gr[k][c] = G2[o];
                }
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
#pragma unroll
                for (int c = 0; c < CT; ++c) F[c] = colok[c] ? fma(pr[k][c], F[c], gr[k][c] * an[k]) : 0.0;
                while (next == n - k) {
                    emit(m, t2[n - k]);
                    --m;
                    next = (m >= 0) ? qi[m] : -1;
                }
            }
        }
        for (; n >= 0; --n) {
            const double a1 = al[n];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const size_t o = (size_t)n * ld + col[c];
                const double pj = (n + 1 < N) ? P2[o + ld] : 1.0;
                F[c] = colok[c] ? fma(pj, F[c], G2[o] * a1) : 0.0;
            }
            while (next == n) {
                emit(m, t2[n]);
                --m;
                next = (m >= 0) ? qi[m] : -1;
            }
        }
    }
}

// ---- chunk-parallel form (long series): the recurrence F <- p o F + g alpha is linear with a
// DIAGONAL transition, so chunks of rows are swept concurrently:
//   k_gmm_chunk<CT, 0>  local pass from F = 0: end state F_loc and the chunk's decay D = prod p
//   k_gmm_scan          F_start of every chunk (sequential over chunks, 64-wide FMAs)
//   k_gmm_chunk<CT, 1>  chunks that contain queries are swept again from F_start and emit
// Row ranges: dir 0 sweeps rows a..b ascending with p_n = P2[n]; dir 1 sweeps b..a descending
// with p_n = P2[n+1] (1 for the last row of the series).  A query is emitted after row
// qidx-1 (dir 0) / row qidx (dir 1), as in k_gmm.
struct GmmChunk {
    int64_t chunk_len;
    int nch;
    double *Floc, *Dloc, *Fstart;   // [B][2][nch][CT*64]
};

__device__ __forceinline__ int64_t gmm_lower_bound(const int64_t *q, int64_t M, int64_t v) {
    int64_t lo = 0, hi = M;         // first m with q[m] >= v
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (q[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

template <int CT, int PHASE>
__global__ void __launch_bounds__(64) k_gmm_chunk(const GmmArgs A, const GmmChunk C) {
    const int lane = threadIdx.x, b = blockIdx.x, dir = blockIdx.y, ch = blockIdx.z;
    const int64_t M = A.M, N = A.N;
    const int ld = A.ld;
    const int64_t a = (int64_t)ch * C.chunk_len;
    const int64_t e = (a + C.chunk_len < N) ? (a + C.chunk_len) : N;      // rows [a, e)
    const double *t1 = A.t1 + (size_t)b * A.t1_bs;
    const double *t2 = A.t2 + (size_t)b * A.t2_bs;
    const double *__restrict__ Q1 = (dir == 0 ? A.U1 : A.V1) + (size_t)b * M * ld;
    const double *__restrict__ G2 = (dir == 0 ? A.V2 : A.U2) + (size_t)b * N * ld;
    const double *__restrict__ P2 = A.P2 + (size_t)b * N * ld;
    const double *__restrict__ al = A.alpha + (size_t)b * N;
    const int64_t *__restrict__ qi = A.qidx + (size_t)b * M;
    double *out = A.work + ((size_t)b * 2 + dir) * M;
    const size_t slot = (((size_t)b * 2 + dir) * C.nch + ch) * (CT * 64);
    bool colok[CT];
    int col[CT];
    double F[CT], D[CT], cj[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int j = c * 64 + lane;
        colok[c] = j < A.W;
        col[c] = colok[c] ? j : 0;
        F[c] = (PHASE == 1) ? C.Fstart[slot + c * 64 + lane] : 0.0;
        D[c] = 1.0;
        cj[c] = colok[c] ? A.c[(size_t)b * A.W + j] : 0.0;
    }
    // queries of this chunk: [m_lo, m_hi)
    int64_t m_lo = 0, m_hi = 0;
    if (PHASE == 1) {
        if (dir == 0) { m_lo = gmm_lower_bound(qi, M, a + 1); m_hi = gmm_lower_bound(qi, M, e + 1); }
        else          { m_lo = gmm_lower_bound(qi, M, a);     m_hi = gmm_lower_bound(qi, M, e); }
        // queries before the first / after the last observed row get no contribution
        if (dir == 0 && ch == 0) for (int64_t m = lane; m < m_lo; m += 64) out[m] = 0.0;
        if (dir == 1 && ch == C.nch - 1) for (int64_t m = m_hi + lane; m < M; m += 64) out[m] = 0.0;
        if (m_lo == m_hi) return;
    }
    auto emit = [&](int64_t m, double tdata) {
        const double dt = (dir == 0) ? (tdata - t1[m]) : (t1[m] - tdata);   // <= 0
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (colok[c]) acc = fma(Q1[(size_t)m * ld + col[c]] * exp(cj[c] * dt), F[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) out[m] = acc;
    };
    constexpr int GB = 8;
    if (dir == 0) {
        int64_t m = m_lo;
        int64_t next = (PHASE == 1) ? qi[m] : (N + 2);                      // emit after row next-1
        const int64_t last = (PHASE == 1) ? qi[m_hi - 1] : e;               // rows [a, last)
        for (int64_t n = a; n < last; n += GB) {
            double pr[GB][CT], gr[GB][CT], an[GB];
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                const int64_t r = (n + k < last) ? (n + k) : (last - 1);
                an[k] = al[r];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const size_t o = (size_t)r * ld + col[c];
                    pr[k][c] = P2[o];
                    gr[k][c] = G2[o];
                }
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                if (n + k < last) {                                          // wave-uniform
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        F[c] = colok[c] ? fma(pr[k][c], F[c], gr[k][c] * an[k]) : 0.0;
                        if (PHASE == 0) D[c] *= pr[k][c];
                    }
                    if (PHASE == 1) {
                        while (m < m_hi && next == n + k + 1) {
                            emit(m, t2[n + k]);
                            ++m;
                            next = (m < m_hi) ? qi[m] : (N + 2);
                        }
                    }
                }
            }
        }
    } else {
        int64_t m = m_hi - 1;
        int64_t next = (PHASE == 1) ? qi[m] : -2;                           // emit after row next
        const int64_t first = (PHASE == 1) ? qi[m_lo] : a;                  // rows (e-1) .. first
        for (int64_t n = e - 1; n >= first; n -= GB) {
            double pr[GB][CT], gr[GB][CT], an[GB];
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                const int64_t r = (n - k >= first) ? (n - k) : first;
                an[k] = al[r];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const size_t o = (size_t)r * ld + col[c];
                    pr[k][c] = (r + 1 < N) ? P2[o + ld] : 1.0;
                    gr[k][c] = G2[o];
                }
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                if (n - k >= first) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        F[c] = colok[c] ? fma(pr[k][c], F[c], gr[k][c] * an[k]) : 0.0;
                        if (PHASE == 0) D[c] *= pr[k][c];
                    }
                    if (PHASE == 1) {
                        while (m >= m_lo && next == n - k) {
                            emit(m, t2[n - k]);
                            --m;
                            next = (m >= m_lo) ? qi[m] : -2;
                        }
                    }
                }
            }
        }
    }
    if (PHASE == 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            C.Floc[slot + c * 64 + lane] = F[c];
            C.Dloc[slot + c * 64 + lane] = colok[c] ? D[c] : 0.0;
        }
    }
}

// F_start of every chunk.  dir 0: F_start[0] = 0, F_start[c+1] = D_c F_start[c] + F_loc[c];
// dir 1 runs from the last chunk down.
__global__ void __launch_bounds__(256) k_gmm_scan(const int CTW, const GmmChunk C) {
    const int b = blockIdx.x, dir = blockIdx.y;
    const size_t base = ((size_t)b * 2 + dir) * C.nch * CTW;
    // sixteen chunks' (D, F_loc) are fetched before their sixteen dependent FMAs: one memory round trip per
    // chunk made the scan 0.28 ms for the 1024 chunks of a 1e6-row series (a tenth of predict at new times)
    constexpr int GB = 16;
    for (int j = threadIdx.x; j < CTW; j += 256) {
        double F = 0.0;
        for (int s0 = 0; s0 < C.nch; s0 += GB) {
            double d[GB], f[GB];
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                int sidx = s0 + k;
                sidx = (sidx < C.nch) ? sidx : C.nch - 1;
                const int c = (dir == 0) ? sidx : C.nch - 1 - sidx;
                const size_t o = base + (size_t)c * CTW + j;
                d[k] = C.Dloc[o];
                f[k] = C.Floc[o];
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                const int sidx = s0 + k;
                if (sidx < C.nch) {
                    const int c = (dir == 0) ? sidx : C.nch - 1 - sidx;
                    C.Fstart[base + (size_t)c * CTW + j] = F;
                    F = fma(d[k], F, f[k]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// k_cross: cross-covariance block K(t_n, t*_r) of the celerite kernel, written in the
// [B][N][R] layout the multi-RHS sweeps take (conditional variance / covariance:
// celerite2's ConditionalDistribution builds the same dense block on the host).
//   K = sum_r a_r e^{-c_r tau} + sum_c (a_c cos d_c tau + b_c sin d_c tau) e^{-c_c tau},
//   tau = |t_n - t*_r|.
// A term is Re[(a - i b) w(tau)] with w(tau) = e^{(-c + i d) tau}, and w(tau_b + delta) = w(tau_b) w(delta): one
// workgroup takes 256 rows, whose times span [tmin, tmax].  A query at or beyond tmax has tau = (t* - tmax) +
// (tmax - t_n), one at or before tmin tau = (tmin - t*) + (t_n - tmin) -- both parts non-negative, both factors
// decaying.  So per workgroup and term: (a - i b) w(t* - tmax) or w(tmin - t*) for every query (a table in LDS), and
// per row w(tmax - t_n), w(t_n - tmin); an entry is then TWO FMAs per term instead of a sine, a cosine and an
// exponential (1.9e9 of each per 64 queries at N = 1e6, J = 30: 5.3 ms, half of predict(return_var=True)).  Queries
// inside the workgroup's span are evaluated entry by entry, as before (one workgroup per query).  Lane = row, RT
// accumulators per lane; the row's RT entries leave as one contiguous run.
// The exposure-integrated kernel differs from its coefficient form for tau < delta; the caller
// patches those (at most a few per query) entries.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void cross_w(const double cc, const double dd, const double x, double &re, double &im) {
    const double e = fm_exp(-cc * x);               // x >= 0
    if (dd == 0.0) { re = e; im = 0.0; return; }    // (real term)
    double si, cs;
    const double ph = dd * x;
    if (fabs(ph) < FM_SINCOS_RANGE) fm_sincos(ph, &si, &cs); else sincos(ph, &si, &cs);
    re = e * cs;
    im = e * si;
}

template <int RT>
__global__ void __launch_bounds__(256)
k_cross(const int64_t N, const int R, const int Jr, const int Jc,
        const double *__restrict__ ar_, const double *__restrict__ cr_,
        const double *__restrict__ ac_, const double *__restrict__ bc_,
        const double *__restrict__ cc_, const double *__restrict__ dc_,
        const double *__restrict__ t_, const int64_t t_bs,
        const double *__restrict__ ts_, const int64_t ts_bs, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int J = Jr + Jc, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *co = lds;                               // [J][4]: a, b, c, d (real terms: b = d = 0)
    double2 *AE = reinterpret_cast<double2 *>(co + 4 * J);      // [RT][J]: (a - i b) w(tau_b), zero for queries inside
    double *tq = reinterpret_cast<double *>(AE + (size_t)RT * J);  // [RT]
    __shared__ double s_mm[2][4];
    __shared__ unsigned long long s_side[3];        // bit r: query at / beyond tmax, at / before tmin, inside
    for (int i = tid; i < J; i += 256) {
        double *q = co + 4 * i;
        if (i < Jr) { q[0] = ar_[(size_t)b * Jr + i]; q[1] = 0.0; q[2] = cr_[(size_t)b * Jr + i]; q[3] = 0.0; }
        else {
            const size_t o = (size_t)b * Jc + (i - Jr);
            q[0] = ac_[o]; q[1] = bc_[o]; q[2] = cc_[o]; q[3] = dc_[o];
        }
    }
    const int64_t n = (int64_t)blockIdx.x * 256 + tid;
    const bool row = n < N;
    const double tn = t_[(size_t)b * t_bs + (row ? n : N - 1)];
    {
        const double hi = wave_max(tn), lo = -wave_max(-tn);
        if (lane == 0) { s_mm[0][wave] = hi; s_mm[1][wave] = lo; }
    }
    __syncthreads();
    const double tmax = fmax(fmax(s_mm[0][0], s_mm[0][1]), fmax(s_mm[0][2], s_mm[0][3]));
    const double tmin = fmin(fmin(s_mm[1][0], s_mm[1][1]), fmin(s_mm[1][2], s_mm[1][3]));
    const double dL = tmax - tn, dR = tn - tmin;   // >= 0
    double *og = out + ((size_t)b * N + (row ? n : 0)) * R;
    for (int r0 = 0; r0 < R; r0 += RT) {
        const int rt = (R - r0 < RT) ? R - r0 : RT;
        __syncthreads();
        if (tid < 64) {
            const double q = (tid < rt) ? ts_[(size_t)b * ts_bs + r0 + tid] : 0.0;
            if (tid < RT) tq[tid] = q;
            const bool L = tid < rt && q >= tmax, Rr = tid < rt && !L && q <= tmin, in = tid < rt && !L && !Rr;
            const unsigned long long mL = __ballot(L), mR = __ballot(Rr), mI = __ballot(in);
            if (tid == 0) { s_side[0] = mL; s_side[1] = mR; s_side[2] = mI; }
        }
        __syncthreads();
        const unsigned long long mL = s_side[0], mR = s_side[1], mI = s_side[2];
        for (int e = tid; e < rt * J; e += 256) {
            const int r = e / J, i = e - r * J;
            const double *q = co + 4 * i;
            double re = 0.0, im = 0.0;
            if (!((mI >> r) & 1ull)) {
                const double taub = ((mL >> r) & 1ull) ? tq[r] - tmax : tmin - tq[r];
                double wr, wi;
                cross_w(q[2], q[3], taub, wr, wi);
                re = fma(q[0], wr, q[1] * wi);      // (a - i b)(wr + i wi)
                im = fma(q[0], wi, -q[1] * wr);
            }
            AE[(size_t)r * J + i] = double2{re, im};
        }
        __syncthreads();
        double acc[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r] = 0.0;
        // (the masks as scalars: the tests below become scalar branches, not exec-mask switches)
        const unsigned mLlo = __builtin_amdgcn_readfirstlane((unsigned)mL), mLhi = __builtin_amdgcn_readfirstlane((unsigned)(mL >> 32));
        const unsigned mRlo = __builtin_amdgcn_readfirstlane((unsigned)mR), mRhi = __builtin_amdgcn_readfirstlane((unsigned)(mR >> 32));
        for (int i = 0; i < J; ++i) {
            const double *q = co + 4 * i;
            double lr = 0.0, li = 0.0, rr = 0.0, ri = 0.0;
            if (mL) cross_w(q[2], q[3], dL, lr, li);            // (workgroup-uniform)
            if (mR) cross_w(q[2], q[3], dR, rr, ri);
            const double2 *ae = AE + i;
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const bool isL = ((r < 32 ? mLlo : mLhi) >> (r & 31)) & 1u, isR = ((r < 32 ? mRlo : mRhi) >> (r & 31)) & 1u;
                if (isL) { const double2 v = ae[(size_t)r * J]; acc[r] = fma(v.x, lr, fma(-v.y, li, acc[r])); }
                else if (isR) { const double2 v = ae[(size_t)r * J]; acc[r] = fma(v.x, rr, fma(-v.y, ri, acc[r])); }
            }
        }
        if (mI) {                                   // queries inside this workgroup's span: entry by entry
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                if ((mI >> r) & 1ull) {
                    const double tau = fabs(tn - tq[r]);
                    double k = 0.0;
                    for (int i = 0; i < J; ++i) {
                        const double *q = co + 4 * i;
                        double wr, wi;
                        cross_w(q[2], q[3], tau, wr, wi);
                        k = fma(q[0], wr, fma(q[1], wi, k));
                    }
                    acc[r] = k;
                }
            }
        }
        if (row) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (r < rt) og[r0 + r] = acc[r];
        }
    }
}

// mu[b][m] = work[b][0][m] + work[b][1][m]
__global__ void k_add2(int64_t M, const double *work, double *mu) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t b = blockIdx.y;
    if (m < M) mu[b * M + m] = work[(b * 2) * M + m] + work[(b * 2 + 1) * M + m];
}

// ------------------------------------------------------------------------------------
// k_factor2w: the block-scaled recurrence of k_factor2 for widths beyond one wave (64 < W <= 256),
// in k_factor's multi-wave mapping.  Scaled coordinates turn the per-row decay
// S <- P (S + ...) P (two multiplies per element and row) into a rescaling at reset rows only:
// per element and row one FMA for the pending rank-1 update and one for the mat-vec, instead of
// the four operations of k_factor.  Inputs are gf_build_scaled's rows (U~, V~, a, de); the state
// handed from tile to tile is k_factor's layout [RT rows][CT * 64 columns] with the pending
// update folded in, F~ in column form.  Log-likelihood path only (no factor rows are stored).
// ------------------------------------------------------------------------------------
struct Factor2wArgs {
    int64_t N, n_first;
    int W, ld;
    const double *c, *a, *Ut, *Vt, *de, *y;
    int64_t y_bs;
    double *d, *z, *S_state, *F_state;
    int32_t *info;
};

template <int RB, int CT, int NW>
__global__ void __launch_bounds__(64 * NW, 2) k_factor2w(const Factor2wArgs A) {     // 2 waves per SIMD
    static_assert(RB % 4 == 0, "rows per wave must be a multiple of 4");
    constexpr int WPC = CT * 64;
    constexpr int RT = RB * NW;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x;
    if (A.info[b] != 0) return;         // an earlier tile of this problem already failed
    const int ld = A.ld;
    const size_t pb = (size_t)b * A.N;
    const double *__restrict__ ag = A.a + pb;
    const double *__restrict__ Ug = A.Ut + pb * ld;
    const double *__restrict__ Vg = A.Vt + pb * ld;
    const double *__restrict__ eg = A.de + pb;
    const double *__restrict__ yg = A.y + (size_t)b * A.y_bs;
    double *__restrict__ Sg = A.S_state + (size_t)b * RT * WPC;
    double *__restrict__ Fg = A.F_state + (size_t)b * WPC;

    __shared__ double s_part[2][NW][WPC];
    __shared__ double s_vec[NW][3][WPC];
    double *sv_u = s_vec[wave][0], *sv_w = s_vec[wave][1], *sv_e = s_vec[wave][2];

    double S[RB][CT], Fv[CT], q[CT];         // pending update: S += w q^T, F~ += q z (q = r / d)
    bool colok[CT];
    int colc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int j = c * 64 + lane;
        colok[c] = j < ld;
        colc[c] = colok[c] ? j : (ld - 1);
        Fv[c] = Fg[j];
        q[c] = 0.0;
        sv_w[j] = 0.0;
#pragma unroll
        for (int r = 0; r < RB; ++r) S[r][c] = Sg[(size_t)(wave * RB + r) * WPC + j];
    }
    double zp = 0.0;                    // z of the pending row
    int32_t fail = 0;

    // row operands one row ahead: plain unconditional loads (clamped pad columns, masked at use; the
    // per-row scalars through the vector-load queue): the caller pads every buffer by two rows
    const int vz = __builtin_amdgcn_mbcnt_lo(0u, 0u);
    double un[CT], vn[CT], an, yn, en;
#pragma unroll
    for (int c = 0; c < CT; ++c) { un[c] = Ug[colc[c]]; vn[c] = Vg[colc[c]]; }
    an = ag[vz]; yn = yg[vz]; en = eg[vz];

    for (int64_t n = 0; n < A.N; ++n) {
        double u[CT], v[CT];
        const double a_n = an, y_n = yn;
        const double e_n = read_lane(en, 0);    // wave-uniform: say so
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            u[c] = colok[c] ? un[c] : 0.0;
            v[c] = colok[c] ? vn[c] : 0.0;
            sv_u[c * 64 + lane] = u[c];
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const size_t o = (size_t)(n + 1) * ld + colc[c];
            un[c] = Ug[o];
            vn[c] = Vg[o];
        }
        an = ag[n + 1 + vz]; yn = yg[n + 1 + vz]; en = eg[n + 1 + vz];

        if (e_n >= 0.0) {               // reset row: fold the pending update, decay by exp(-c de)
            double el[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int j = c * 64 + lane;     // (decay rates are read here: resets are rare, registers are not)
                el[c] = (j < A.W) ? exp(-A.c[(size_t)b * A.W + j] * e_n) : 1.0;
                sv_e[c * 64 + lane] = el[c];
            }
            wave_lds_fence();
#pragma unroll
            for (int r0 = 0; r0 < RB; r0 += 4) {    // batches of 4 rows, fenced: hipcc otherwise hoists
                double wi[4], ei[4];                // every LDS read of the loop (and spills)
#pragma unroll
                for (int k = 0; k < 4; ++k) { wi[k] = sv_w[wave * RB + r0 + k]; ei[k] = sv_e[wave * RB + r0 + k]; }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        S[r0 + k][c] = fma(wi[k], q[c], S[r0 + k][c]) * (ei[k] * el[c]);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int c = 0; c < CT; ++c) { Fv[c] = el[c] * fma(q[c], zp, Fv[c]); q[c] = 0.0; }
            zp = 0.0;
        }
        wave_lds_fence();

        double acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0.0;
#pragma unroll
        for (int r0 = 0; r0 < RB; r0 += 4) {
            double wi[4], ui[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { wi[k] = sv_w[wave * RB + r0 + k]; ui[k] = sv_u[wave * RB + r0 + k]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    S[r0 + k][c] = fma(wi[k], q[c], S[r0 + k][c]);
                    acc[c] = fma(ui[k], S[r0 + k][c], acc[c]);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        double tmp[CT];
        if constexpr (NW > 1) {
            const int buf = (int)(n & 1);
#pragma unroll
            for (int c = 0; c < CT; ++c) s_part[buf][wave][c * 64 + lane] = acc[c];
            wg_lds_barrier();
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                double t2 = s_part[buf][0][c * 64 + lane];
#pragma unroll
                for (int w2 = 1; w2 < NW; ++w2) t2 += s_part[buf][w2][c * 64 + lane];
                tmp[c] = t2;
            }
        } else {
#pragma unroll
            for (int c = 0; c < CT; ++c) tmp[c] = acc[c];
        }
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            Fv[c] = fma(q[c], zp, Fv[c]);
            s1 = fma(u[c], tmp[c], s1);
            s2 = fma(u[c], Fv[c], s2);
        }
        wave_sum2(s1, s2);
        const double dn = a_n - s1;
        const double zn = y_n - s2;
        if (!(dn > 0.0)) {              // uniform across the whole workgroup
            const int64_t ng = A.n_first + n + 1;
            fail = (int32_t)(ng > 0x7fffffff ? 0x7fffffff : ng);
            break;
        }
        const double inv = fast_rcp(dn);
        zp = zn;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const double r = v[c] - tmp[c];     // pad lanes: 0 - 0
            q[c] = r * inv;
            sv_w[c * 64 + lane] = r;
        }
        if (wave == 0 && lane == 0) { A.d[pb + n] = dn; A.z[pb + n] = zn; }
    }
    if (fail) {
        if (wave == 0 && lane == 0) A.info[b] = fail;
        return;
    }
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int i = wave * RB + r;
        const double wi = sv_w[i];
#pragma unroll
        for (int c = 0; c < CT; ++c) Sg[(size_t)i * WPC + c * 64 + lane] = fma(wi, q[c], S[r][c]);
    }
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) Fg[c * 64 + lane] = fma(q[c], zp, Fv[c]);
    }
}

// ------------------------------------------------------------------------------------
// dispatch helpers
// ------------------------------------------------------------------------------------
template <int RB, int CT, int NW>
int launch_factor(const FactorArgs &A, int B, int nch, hipStream_t st) {
    hipLaunchKernelGGL((k_factor<RB, CT, NW>), dim3(nch, B), dim3(64 * NW), 0, st, A);
    return check_launch("gf_factor");
}

int dispatch_factor(const FactorArgs &A, int B, int nch, hipStream_t st) {
    const int W = A.W;
    if (W <= 16)  return launch_factor<4, 1, 4>(A, B, nch, st);
    if (W <= 32)  return launch_factor<8, 1, 4>(A, B, nch, st);
    if (W <= 48)  return launch_factor<12, 1, 4>(A, B, nch, st);
    if (W <= 64)  return launch_factor<16, 1, 4>(A, B, nch, st);
    if (W <= 96)  return launch_factor<24, 2, 4>(A, B, nch, st);
    if (W <= 128) return launch_factor<32, 2, 4>(A, B, nch, st);
    if (W <= 192) return launch_factor<24, 3, 8>(A, B, nch, st);
    return launch_factor<32, 4, 8>(A, B, nch, st);
}

template <int RB, int CT, int NW>
int launch_factor2w(const Factor2wArgs &A, int B, hipStream_t st) {
    hipLaunchKernelGGL((k_factor2w<RB, CT, NW>), dim3(B), dim3(64 * NW), 0, st, A);
    return check_launch("gf_factor_scaled");
}

int dispatch_factor2w(const Factor2wArgs &A, int B, hipStream_t st) {      // same shapes as dispatch_factor
    const int W = A.W;
    if (W <= 96)  return launch_factor2w<24, 2, 4>(A, B, st);
    if (W <= 128) return launch_factor2w<32, 2, 4>(A, B, st);
    if (W <= 192) return launch_factor2w<24, 3, 8>(A, B, st);
    return launch_factor2w<32, 4, 8>(A, B, st);
}

// Propagator rows of a factor stored in block-scaled form (rows u~, w~ = r/d and the reset spans de of
// gf_chunk_sweep): in scaled coordinates the row-to-row propagator is 1, and exp(-c de) at a reset row.
// With these rows the general-width sweeps (gf_solve) run on the scaled factor unchanged.
__global__ void __launch_bounds__(256)
k_scaled_propagator(const int64_t N, const int W, const int ld, const double *__restrict__ c_,
                    const double *__restrict__ de_, double *__restrict__ P_out) {
    const int b = blockIdx.y;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = id / ld;
    if (n >= N) return;
    const int j = (int)(id - n * ld);
    const double de = de_[(size_t)b * N + n];
    const double cj = (j < W) ? c_[(size_t)b * W + j] : 0.0;
    P_out[((size_t)b * N + n) * ld + j] = (de > 0.0) ? exp(-cj * de) : 1.0;
}

}  // namespace

// ======================================================================================
// C-ABI
// ======================================================================================
extern "C" {

int gf_leading_dim(int W) {
    if (W < 1 || W > GF_MAX_WIDTH) return -1;
    return (W + 15) / 16 * 16;
}

int gf_build_matrices(int B, int64_t N, int64_t n_first, int Jr, int Jc, int ld,
                      const double *ar, const double *cr, const double *ac,
                      const double *bc, const double *cc, const double *dc,
                      const double *diag_add,
                      const double *t, int64_t t_bs,
                      const double *diag, int64_t diag_bs,
                      double *a, double *U, double *V, double *P, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_build_matrices: empty problem (B=%d, N=%lld)", B, (long long)N);
    if (check_width_ld("gf_build_matrices", W, ld)) return -1;
    if (!t || !U || !V || (a && !diag_add)) return gf_internal_error(-1, "gf_build_matrices: null pointer");
    BuildArgs A;
    if (n_first < 0) return gf_internal_error(-1, "gf_build_matrices: negative n_first");
    A.N = N; A.n_first = n_first; A.Jr = Jr; A.Jc = Jc; A.ld = ld; A.units = Jr + Jc + (ld - W);
    A.ar = ar; A.cr = cr; A.ac = ac; A.bc = bc; A.cc = cc; A.dc = dc; A.diag_add = diag_add;
    A.t = t; A.t_bs = t_bs; A.diag = diag; A.diag_bs = diag_bs;
    A.a = a; A.U = U; A.V = V; A.P = P;
    const int64_t total = N * A.units;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return gf_internal_error(-1, "gf_build_matrices: problem too large");
    hipLaunchKernelGGL(k_build, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, A);
    return check_launch("gf_build_matrices");
}

int64_t gf_state_size(int W) {
    if (W < 1 || W > GF_MAX_WIDTH) return -1;
    if (W <= 16)  return 16 * 64;
    if (W <= 32)  return 32 * 64;
    if (W <= 48)  return 48 * 64;
    if (W <= 64)  return 64 * 64;
    if (W <= 96)  return 96 * 128;
    if (W <= 128) return 128 * 128;
    if (W <= 192) return 192 * 192;
    return 256 * 256;
}

int gf_state_cols(int W) {
    if (W < 1 || W > GF_MAX_WIDTH) return -1;
    return (W + 63) / 64 * 64;
}

int gf_factor(int B, int64_t N, int64_t n_first, int W, int ld,
              const double *a, const double *U, const double *V, const double *P,
              const double *y, int64_t y_bs,
              double *d, double *Wm, double *z,
              double *S_state, double *F_state, int32_t *info, void *stream) {
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_factor: empty problem (B=%d, N=%lld)", B, (long long)N);
    if (check_width_ld("gf_factor", W, ld)) return -1;
    if (!a || !U || !V || !P || !d || !info) return gf_internal_error(-1, "gf_factor: null pointer");
    if (z && !y) return gf_internal_error(-1, "gf_factor: z requested without y");
    FactorArgs A;
    if (F_state && !S_state) return gf_internal_error(-1, "gf_factor: F_state without S_state");
    A.N = N; A.chunk_len = N; A.n_first = n_first; A.W = W; A.ld = ld;
    A.a = a; A.U = U; A.V = V; A.P = P; A.y = y; A.y_bs = y_bs;
    A.d = d; A.Wm = Wm; A.z = z;
    A.S_in = S_state; A.F_in = F_state; A.S_out = S_state; A.F_out = F_state;
    A.info = info;
    return dispatch_factor(A, B, 1, (hipStream_t)stream);
}

int gf_scaled_supported(int W) { return (W >= 1 && W <= 64) ? 1 : 0; }

double gf_scaled_span(int long_span) { return long_span ? SC_SPAN_LONG : SC_SPAN; }

// widths the block-scaled build + multi-wave sweep (k_build2 + k_factor2w) take beyond one wave
int gf_scaled_wide_supported(int W) { return (W > 64 && W <= 192) ? 1 : 0; }   // (beyond: register spills, gf_factor is faster)

int gf_build_scaled(int B, int64_t N, int64_t n_first, int Jr, int Jc, int ld,
                    const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc,
                    const double *diag_add, const double *cmax, int block,
                    const double *t, int64_t t_bs,
                    const double *diag, int64_t diag_bs,
                    double *a, double *Ut, double *Vt, double *de, void *stream) {
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_build_scaled: empty problem (B=%d, N=%lld)", B, (long long)N);
    if (!gf_scaled_supported(W) && !gf_scaled_wide_supported(W)) return gf_internal_error(-1, "gf_build_scaled: width %d unsupported", W);
    if (check_ld("gf_build_scaled", W, ld) || check_block("gf_build_scaled", block)
        || check_n_first("gf_build_scaled", n_first, block)) return -1;
    if (!t || !a || !Ut || !Vt || !de || !diag_add || !cmax) return gf_internal_error(-1, "gf_build_scaled: null pointer");
    Build2Args A;
    A.N = N; A.n_first = n_first; A.Jr = Jr; A.Jc = Jc; A.ld = ld; A.units = Jr + Jc + (ld - W);
    A.block = block; A.gap = sweep_gap(block, GF_SWEEP_AUTO);
    A.ar = ar; A.cr = cr; A.ac = ac; A.bc = bc; A.cc = cc; A.dc = dc; A.diag_add = diag_add; A.cmax = cmax;
    A.t = t; A.t_bs = t_bs; A.diag = diag; A.diag_bs = diag_bs;
    A.a = a; A.Ut = Ut; A.Vt = Vt; A.de = de;
    const int64_t blocks = (N + B2_ROWS - 1) / B2_ROWS;
    if (blocks > 0x7fffffffLL) return gf_internal_error(-1, "gf_build_scaled: problem too large");
    hipLaunchKernelGGL(k_build2, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, A);
    return check_launch("gf_build_scaled");
}

int gf_factor_scaled(int B, int64_t N, int64_t n_first, int W, int ld, const double *c,
                     const double *a, const double *Ut, const double *Vt, const double *de,
                     const double *y, int64_t y_bs,
                     double *d, double *z, double *S_state, double *F_state,
                     int32_t *info, void *stream) {
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_factor_scaled: empty problem (B=%d, N=%lld)", B, (long long)N);
    if (!gf_scaled_supported(W) && !gf_scaled_wide_supported(W)) return gf_internal_error(-1, "gf_factor_scaled: width %d unsupported", W);
    if (check_ld("gf_factor_scaled", W, ld)) return -1;
    if (!c || !a || !Ut || !Vt || !de || !y || !d || !z || !S_state || !F_state || !info)
        return gf_internal_error(-1, "gf_factor_scaled: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (W > 64) {                       // state: gf_state_size(W) / gf_state_cols(W) doubles per problem
        Factor2wArgs A;
        A.N = N; A.n_first = n_first; A.W = W; A.ld = ld;
        A.c = c; A.a = a; A.Ut = Ut; A.Vt = Vt; A.de = de; A.y = y; A.y_bs = y_bs;
        A.d = d; A.z = z; A.S_state = S_state; A.F_state = F_state; A.info = info;
        return dispatch_factor2w(A, B, st);
    }
    if (!dispatch_rows((W + 3) / 4 * 4, [&](auto r) {
            hipLaunchKernelGGL((k_factor2<decltype(r)::value>), dim3(B), dim3(64), 0, st, N, n_first, ld, W, c, a, Ut, Vt,
                               de, y, y_bs, d, z, S_state, F_state, info);
        }))
        return gf_internal_error(-1, "gf_factor_scaled: internal dispatch error");
    return check_launch("gf_factor_scaled");
}

int gf_scaled_propagator(int B, int64_t N, int W, int ld, const double *c, const double *de,
                         double *P_out, void *stream) {
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_scaled_propagator: empty problem (N=%lld)", (long long)N);
    if (W < 1 || ld < W) return gf_internal_error(-1, "gf_scaled_propagator: bad width / ld (W=%d, ld=%d)", W, ld);
    if (!c || !de || !P_out) return gf_internal_error(-1, "gf_scaled_propagator: null pointer");
    const int64_t blocks = (N * ld + 255) / 256;
    if (blocks > 0x7fffffffLL) return gf_internal_error(-1, "gf_scaled_propagator: problem too large");
    hipLaunchKernelGGL(k_scaled_propagator, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream,
                       N, W, ld, c, de, P_out);
    return check_launch("gf_scaled_propagator");
}

// one-right-hand-side sweeps: `grid` single-wave workgroups (problems x chunks)
static void launch_solve_vec(const SolveArgs &A, int grid, hipStream_t st) {
    const int mode = A.mode;
#define GF_SV(CT, M, S) hipLaunchKernelGGL((k_solve_vec<CT, M, S>), dim3(grid), dim3(64), 0, st, A)
#define GF_SV_MODE(CT) do { const bool sd = A.scale != nullptr; \
        if (mode == GF_SOLVE_LOWER) { if (sd) GF_SV(CT, GF_SOLVE_LOWER, true); else GF_SV(CT, GF_SOLVE_LOWER, false); } \
        else if (mode == GF_SOLVE_UPPER) { if (sd) GF_SV(CT, GF_SOLVE_UPPER, true); else GF_SV(CT, GF_SOLVE_UPPER, false); } \
        else { if (sd) GF_SV(CT, GF_MATMUL_LOWER, true); else GF_SV(CT, GF_MATMUL_LOWER, false); } } while (0)
    if (A.ld <= 64)       GF_SV_MODE(1);
    else if (A.ld <= 128) GF_SV_MODE(2);
    else if (A.ld <= 192) GF_SV_MODE(3);
    else                  GF_SV_MODE(4);
#undef GF_SV_MODE
#undef GF_SV
}

// several right-hand sides: one workgroup per (tile of 64 right-hand sides, problem x chunk)
static void launch_solve_rhs(const SolveArgs &A, int slots, hipStream_t st) {
    const int ld = A.ld;
    const dim3 grid((A.R + 63) / 64, slots);
    if (ld <= 16)       hipLaunchKernelGGL((k_solve_rhs<16, 1>), grid, dim3(64), 0, st, A);
    else if (ld <= 32)  hipLaunchKernelGGL((k_solve_rhs<32, 1>), grid, dim3(64), 0, st, A);
    else if (ld <= 48)  hipLaunchKernelGGL((k_solve_rhs<48, 1>), grid, dim3(64), 0, st, A);
    else if (ld <= 64)  hipLaunchKernelGGL((k_solve_rhs<64, 1>), grid, dim3(64), 0, st, A);
    else if (ld <= 96)  hipLaunchKernelGGL((k_solve_rhs<48, 2>), grid, dim3(128), 0, st, A);
    else if (ld <= 128) hipLaunchKernelGGL((k_solve_rhs<64, 2>), grid, dim3(128), 0, st, A);
    else if (ld <= 192) hipLaunchKernelGGL((k_solve_rhs<48, 4>), grid, dim3(256), 0, st, A);
    else                hipLaunchKernelGGL((k_solve_rhs<64, 4>), grid, dim3(256), 0, st, A);
}

// Chunk-parallel form of the one-right-hand-side sweeps of gf_solve (any width; what the wide stored
// factor uses): local pass (F_state zeroed by the caller, store = 0) -> combine of the chunk states on the
// caller's side (GF_MATMUL_LOWER: diagonal decays, gf_chunk_diag_scan; the solves: the chunks' closed-loop
// transitions) -> final pass from the true start states (store = 1).  F_state: [B * nch][ld].
int gf_solve_chunk(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int ld,
                   const double *U, const double *Wm, const double *P, const double *scale,
                   const double *Y, double *Z, double *F_state, int store, void *stream) {
    if (mode < 0 || mode > 2) return gf_internal_error(-1, "gf_solve_chunk: bad mode %d", mode);
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_solve_chunk: empty problem (N=%lld)", (long long)N);
    if (check_width_ld("gf_solve_chunk", W, ld)) return -1;
    if (check_chunking("gf_solve_chunk", N, chunk_len, nch, 1)) return -1;
    if (!U || !Wm || !P || !Y || !Z || !F_state) return gf_internal_error(-1, "gf_solve_chunk: null pointer");
    if ((int64_t)B * nch > 0x7fffffffLL) return gf_internal_error(-1, "gf_solve_chunk: problem too large");
    SolveArgs A;
    A.N = N; A.W = W; A.ld = ld; A.R = 1; A.mode = mode;
    A.U = U; A.Wm = Wm; A.P = P; A.scale = scale; A.Y = Y; A.Z = Z;
    A.chunk_len = chunk_len; A.nch = nch; A.store = store; A.F_state = F_state;
    launch_solve_vec(A, B * nch, (hipStream_t)stream);
    return check_launch("gf_solve_chunk");
}

// gf_solve_chunk with R right-hand sides (k_solve_rhs in chunk mode): Y, Z [B][N][R]; F_state
// [B * nch][ld][R].  The combine between the two passes is the caller's (W x W chunk transitions applied to
// W x R states: batched GEMMs).
int gf_solve_chunk_rhs(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int ld, int R,
                       const double *U, const double *Wm, const double *P, const double *scale,
                       const double *Y, double *Z, double *F_state, int store, void *stream) {
    if (mode < 0 || mode > 2) return gf_internal_error(-1, "gf_solve_chunk_rhs: bad mode %d", mode);
    if (B < 1 || N < 1 || R < 1) return gf_internal_error(-1, "gf_solve_chunk_rhs: empty problem (N=%lld, R=%d)", (long long)N, R);
    if (check_width_ld("gf_solve_chunk_rhs", W, ld)) return -1;
    if (check_chunking("gf_solve_chunk_rhs", N, chunk_len, nch, 1)) return -1;
    if (!U || !Wm || !P || !Y || !Z || !F_state) return gf_internal_error(-1, "gf_solve_chunk_rhs: null pointer");
    if ((int64_t)B * nch > 65535) return gf_internal_error(-1, "gf_solve_chunk_rhs: too many chunks (B * nch = %lld > 65535)", (long long)B * nch);
    SolveArgs A;
    A.N = N; A.W = W; A.ld = ld; A.R = R; A.mode = mode;
    A.U = U; A.Wm = Wm; A.P = P; A.scale = scale; A.Y = Y; A.Z = Z;
    A.chunk_len = chunk_len; A.nch = nch; A.store = store; A.F_state = F_state;
    launch_solve_rhs(A, B * nch, (hipStream_t)stream);
    return check_launch("gf_solve_chunk_rhs");
}

int gf_solve(int mode, int B, int64_t N, int W, int ld, int R,
             const double *U, const double *Wm, const double *P, const double *scale,
             const double *Y, double *Z, void *stream) {
    if (mode < 0 || mode > 2) return gf_internal_error(-1, "gf_solve: bad mode %d", mode);
    if (B < 1 || N < 1 || R < 1) return gf_internal_error(-1, "gf_solve: empty problem (N=%lld, R=%d)", (long long)N, R);
    if (check_width_ld("gf_solve", W, ld)) return -1;
    if (!U || !Wm || !P || !Y || !Z) return gf_internal_error(-1, "gf_solve: null pointer");
    if (mode == GF_MATMUL_LOWER && Y == Z) return gf_internal_error(-1, "gf_solve: GF_MATMUL_LOWER cannot run in place");
    SolveArgs A;
    A.N = N; A.W = W; A.ld = ld; A.R = R; A.mode = mode;
    A.U = U; A.Wm = Wm; A.P = P; A.scale = scale; A.Y = Y; A.Z = Z;
    A.chunk_len = N; A.nch = 1; A.store = 1; A.F_state = nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (R == 1) {
        launch_solve_vec(A, B, st);
    } else {
        launch_solve_rhs(A, B, st);
    }
    return check_launch("gf_solve");
}

// K(t_n, t*_r) for n < N, r < R into out [B][N][R] (row-major; R <= 4096 query times per call).
int gf_cross_covariance(int B, int64_t N, int R, int Jr, int Jc,
                        const double *ar, const double *cr, const double *ac,
                        const double *bc, const double *cc, const double *dc,
                        const double *t, int64_t t_bs, const double *ts, int64_t ts_bs,
                        double *out, void *stream) {
    if (B < 1 || N < 1 || R < 1 || R > 4096) return gf_internal_error(-1, "gf_cross_covariance: bad shape (N=%lld, R=%d)", (long long)N, R);
    if (Jr < 0 || Jc < 0 || Jr + Jc < 1 || Jr + 2 * Jc > GF_MAX_WIDTH) return gf_internal_error(-1, "gf_cross_covariance: bad term counts");
    if (!t || !ts || !out || (Jr && (!ar || !cr)) || (Jc && (!ac || !bc || !cc || !dc)))
        return gf_internal_error(-1, "gf_cross_covariance: null pointer");
    // queries per pass (accumulators per lane) so that the table of (term, query) factors fits 48 KB of LDS up to
    // J = 92 and, with the kernel's 88 static bytes, the 64 KB a launch may ask for without the large-LDS attribute
    // beyond: 8 (36 J + 16) bytes at RT = 16 pass it from J = 227 on (real-term kernels up to J = 256 are within
    // GF_MAX_WIDTH), so those take RT = 8 (8 (20 J + 8) bytes: 41 KB at J = 256)
    const int J = Jr + Jc;
    const int RT = (J <= 44) ? 64 : (J <= 92) ? 32 : (J <= 226) ? 16 : 8;
    const size_t lds = sizeof(double) * ((size_t)4 * J + (size_t)2 * RT * J + RT);
    const int64_t blocks = (N + 255) / 256;
    if (blocks > 0x7fffffffLL) return gf_internal_error(-1, "gf_cross_covariance: problem too large");
    const dim3 grid((unsigned)blocks, B);
    hipStream_t st = (hipStream_t)stream;
#define GF_CX(RTv) hipLaunchKernelGGL((k_cross<RTv>), grid, dim3(256), lds, st, N, R, Jr, Jc, ar, cr, ac, bc, cc, dc, t, t_bs, ts, ts_bs, out)
    if (RT == 64) GF_CX(64); else if (RT == 32) GF_CX(32); else if (RT == 16) GF_CX(16); else GF_CX(8);
#undef GF_CX
    return check_launch("gf_cross_covariance");
}

// chunking of the conditional-mean sweeps: ~2048 waves over (problem, direction, chunk), chunks of
// at least 256 rows; one chunk = the sequential k_gmm
static void gmm_chunking(int B, int64_t N, int *nch, int64_t *chunk_len) {
    int64_t n = N / 256;
    const int64_t cap = (1024 / B) > 1 ? (1024 / B) : 1;
    if (n > cap) n = cap;
    if (n < 1) n = 1;
    int64_t len = (N + n - 1) / n;
    *nch = (int)((N + len - 1) / len);
    *chunk_len = len;
}

// doubles of `work` that gf_general_matmul needs
int64_t gf_general_matmul_work(int B, int64_t M, int64_t N, int W) {
    int nch;
    int64_t chunk_len;
    if (B < 1 || N < 1 || M < 1 || W < 1) return 0;
    gmm_chunking(B, N, &nch, &chunk_len);
    const int CT = (W <= 64) ? 1 : (W <= 128) ? 2 : 4;
    return (int64_t)B * 2 * M + (nch > 1 ? 3 * (int64_t)B * 2 * nch * CT * 64 : 0);
}

int gf_general_matmul(int B, int64_t M, int64_t N, int W, int ld,
                      const double *c,
                      const double *t1, int64_t t1_bs, const double *U1, const double *V1,
                      const double *t2, int64_t t2_bs, const double *U2, const double *V2,
                      const double *P2, const double *alpha, const int64_t *qidx,
                      double *work, double *mu, void *stream) {
    if (B < 1 || N < 1 || M < 1) return gf_internal_error(-1, "gf_general_matmul: empty problem (M=%lld, N=%lld)", (long long)M, (long long)N);
    if (check_width_ld("gf_general_matmul", W, ld)) return -1;
    if (!c || !t1 || !U1 || !V1 || !t2 || !U2 || !V2 || !P2 || !alpha || !qidx || !work || !mu)
        return gf_internal_error(-1, "gf_general_matmul: null pointer");
    GmmArgs A;
    A.M = M; A.N = N; A.W = W; A.ld = ld; A.c = c;
    A.t1 = t1; A.t1_bs = t1_bs; A.U1 = U1; A.V1 = V1;
    A.t2 = t2; A.t2_bs = t2_bs; A.U2 = U2; A.V2 = V2; A.P2 = P2; A.alpha = alpha;
    A.qidx = qidx; A.work = work;
    hipStream_t st = (hipStream_t)stream;
    const int CT = (W <= 64) ? 1 : (W <= 128) ? 2 : 4;
    int nch;
    int64_t chunk_len;
    gmm_chunking(B, N, &nch, &chunk_len);
    dispatch_among<1, 2, 4>(CT, [&](auto ct) {
        constexpr int CTv = decltype(ct)::value;
        if (nch == 1) {
            hipLaunchKernelGGL(k_gmm<CTv>, dim3(B, 2), dim3(64), 0, st, A);
            return;
        }
        GmmChunk C;                     // long series: chunk-parallel (decayed prefix sums)
        C.chunk_len = chunk_len; C.nch = nch;
        const size_t per = (size_t)B * 2 * nch * CT * 64;
        C.Floc = work + (size_t)B * 2 * M;
        C.Dloc = C.Floc + per;
        C.Fstart = C.Dloc + per;
        const dim3 grid(B, 2, nch);
        hipLaunchKernelGGL((k_gmm_chunk<CTv, 0>), grid, dim3(64), 0, st, A, C);
        hipLaunchKernelGGL(k_gmm_scan, dim3(B, 2), dim3(256), 0, st, CT * 64, C);
        hipLaunchKernelGGL((k_gmm_chunk<CTv, 1>), grid, dim3(64), 0, st, A, C);
    });
    hipLaunchKernelGGL(k_add2, dim3((unsigned)((M + 255) / 256), B), dim3(256), 0, st, M, work, mu);
    return check_launch("gf_general_matmul");
}

}  // extern "C"
