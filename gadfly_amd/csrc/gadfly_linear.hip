// gadfly_linear.hip -- the stored scaled factor's chunk-parallel linear sweeps and the combines of their chunk states
//
// What is replaced: celerite2's sequential solve_lower / solve_upper / matmul_lower behind gadfly's GaussianProcess
// (apply_inverse, dot_tril and the conditional means of the reference's gadfly/gp.py),
// on the rows u~, w~ that gf_chunk_sweep stored: a local pass per chunk from a zero state, a combine that turns the
// chunks' end states into their true start states, and a final pass from those.
//   k_lin1                     one right-hand side: the state lane-resident, one DPP tree per row
//   k_linR, k_linR7            R right-hand sides, one per lane: every state row in the lane (no entry point launches
//                              it: what k_linR7's comment measures against), and k_factor7's 2 x 32 lane tiling
//   k_mmR_mfma                 GF_MATMUL_LOWER with R >= 16 (no feedback): blocks of 16 rows as matrix products
//   k_lincombine               the combine per right-hand side: plain scan, or the two-level scan over segments
//   k_lincombine_R             the segment scans for 64 right-hand sides at a time on the matrix pipe
//   k_lincombine_mm, k_chunk_decay   the combine of GF_MATMUL_LOWER: diagonal chunk transitions (also gf_chunk_diag_scan)
// Elsewhere: the segments' composed transitions and the transposes the backward solve takes (k_segment_transition,
// k_transpose64, gf_chunk_segment_transitions: gadfly_hip.hip, which says why), the sweeps that store the factor
// (gadfly_hip.hip) and the sweeps on unscaled stored rows (gadfly_stored.hip).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"

#define FM_INLINE __device__ __forceinline__
#include "fastmath.h"           // fm_exp: the decay of a reset row
#include "gf_wave.h"
#include "gf_sweep.h"

namespace {

// ------------------------------------------------------------------------------------
// Triangular sweeps on the STORED scaled factor (u~, w~ = r/d rows, d, reset spans de), chunked:
// every (problem, chunk) starts from the state in F_state and leaves its end state there.
// In scaled coordinates the recurrences have no per-row decay (A.6/A.7 with P folded into the
// block scaling); at a reset row the state is multiplied by E = exp(-c de) once:
//   lower  : F <- [E](F + w~_{n-1} z_{n-1}) ;  z_n = y_n - u~_n . F           (ascending)
//   upper  : G <- [E_{n+1}](G + u~_{n+1} z_{n+1}) ;  z_n = y_n - w~_n . G     (descending; the
//            decay of reset row n+1 is crossed when stepping from n+1 down to n)
//   matmul : F <- [E](F + w~_{n-1} y_{n-1}) ;  z_n = y_n + u~_n . F           (ascending)
// with optional input scaling y <- y / d (upper: apply_inverse) or y <- y sqrt(d) (matmul:
// dot_tril).  R = 1: the state is lane-resident, one DPP tree per row.
// ------------------------------------------------------------------------------------
struct LinArgs {
    int64_t N, chunk_len;
    int nch, W, mode, scale, store;     // store: write z (final pass) or only the end state
    const double *c;                    // [B][W]
    const double *Ut, *Wt, *d, *de, *Y; // rows [B][N][64] / [B][N]; Y [B][N][R]
    double *Z;
    double *F_state;                    // [B*nch][64 * R]  (R = 1: [64])
    int R;
};

// Rows in flight per lane.  The sweep itself is a DPP reduction and two FMAs per row (~400 cycles): what it waits
// for is memory.  u~ / w~ of a row are one double per lane each: a register ring LIN1_RING rows deep, every slot
// refilled with the row LIN1_RING ahead as soon as its row is used (static indices: the row loop is unrolled over the
// ring).  The per-row scalars y, de, d are wave-uniform: fetched 64 rows at a time, lane j its row, one block ahead,
// parked in LDS and read back as broadcasts a row before their use.  (Two batches of eight rows with five registers
// per row and lane -- 241 VGPRs -- left every eighth row waiting on HBM: 0.18 of a pass' 0.45 ms at N = 1e6.)
constexpr int LIN1_RING = 24;
__global__ void __launch_bounds__(64) k_lin1(const LinArgs A) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int pr = b / A.nch, ch = b - pr * A.nch;
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int64_t rows = (A.N - c0 < A.chunk_len) ? (A.N - c0) : A.chunk_len;
    const size_t pb = (size_t)pr * A.N + c0;
    const double *__restrict__ Ug = A.Ut + pb * 64 + lane;
    const double *__restrict__ Wg = A.Wt + pb * 64 + lane;
    const double *__restrict__ dg = A.d + pb;
    const double *__restrict__ eg = A.de + pb;
    const double *__restrict__ Yg = A.Y + pb;
    double *__restrict__ Zg = A.Z + pb;
    double *__restrict__ Fg = A.F_state + (size_t)b * 64;
    const double cj = (lane < A.W) ? A.c[(size_t)pr * A.W + lane] : 0.0;
    const bool up = A.mode == GF_SOLVE_UPPER, mm = A.mode == GF_MATMUL_LOWER;
    double F = A.store ? Fg[lane] : 0.0;            // (the local pass starts from zero)
    constexpr int D = LIN1_RING;
    // step s of the sweep works on row n(s): ascending, or descending for the upper solve (clamped: reads past
    // the chunk's last step fetch its last row again and are never used)
    auto row_of = [&](int64_t s) { s = (s > rows - 1) ? rows - 1 : s; return up ? (rows - 1 - s) : s; };
    __shared__ double sc[2][3][64];                 // y, de, d of 64 steps, two blocks
    double ys, es, dv;                              // the block after those: this lane's step
    auto load_sc = [&](const int64_t blk) {
        const int64_t n = row_of(64 * blk + lane);
        ys = Yg[n]; es = eg[n]; dv = A.scale ? dg[n] : 1.0;
    };
    auto put_sc = [&](const int buf) { sc[buf][0][lane] = ys; sc[buf][1][lane] = es; sc[buf][2][lane] = dv; };
    load_sc(0);
    double qu[D], qw[D];
#pragma unroll
    for (int j = 0; j < D; ++j) { const int64_t n = row_of(j); qu[j] = Ug[(size_t)n * 64]; qw[j] = Wg[(size_t)n * 64]; }
    put_sc(0);
    load_sc(1);
    wave_lds_fence();
    double y_n = sc[0][0][0], e_n = sc[0][1][0], d_n = sc[0][2][0];       // step 0's scalars
    double carry = 0.0, prev = 0.0, de_up = -1.0;   // pending F += prev * carry (w~_{n-1} z_{n-1}, or u~_{n+1} z_{n+1})
    for (int64_t s0 = 0; s0 < rows; s0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int64_t s = s0 + j;
            if (s < rows) {                         // (wave-uniform)
                const int64_t n = up ? (rows - 1 - s) : s;
                const double u = qu[j], w = qw[j];
                double yn = y_n;
                const double de = e_n, dd = d_n;
                // the next step's scalars (a block boundary first hands the parked block over)
                const int li = (int)(s & 63);
                if (li == 63) { put_sc((int)(((s >> 6) + 1) & 1)); load_sc((s >> 6) + 2); wave_lds_fence(); }
                {
                    const int64_t s1 = s + 1;
                    const int b1 = (int)((s1 >> 6) & 1), l1 = (int)(s1 & 63);
                    y_n = sc[b1][0][l1]; e_n = sc[b1][1][l1]; d_n = sc[b1][2][l1];
                }
                if (!up) {
                    if (A.scale) yn = mm ? yn * sqrt(dd) : yn / dd;
                    F = fma(prev, carry, F);
                    if (de >= 0.0) F *= fm_exp(-cj * de);
                    const double dot = wave_sum(u * F);
                    const double zn = mm ? (yn + dot) : (yn - dot);
                    if (A.store && lane == 0) Zg[n] = zn;
                    carry = mm ? yn : zn;
                    prev = w;
                } else {
                    // the state handed DOWN to this chunk already carries the decay of the boundary it crossed
                    if (A.scale) yn = yn / dd;
                    F = fma(prev, carry, F);
                    if (de_up >= 0.0) F *= fm_exp(-cj * de_up);
                    const double dot = wave_sum(w * F);
                    const double zn = yn - dot;
                    if (A.store && lane == 0) Zg[n] = zn;
                    carry = zn;
                    prev = u;
                    de_up = de;
                }
            }
            {   // the slot's next tenant: the row LIN1_RING steps ahead
                const int64_t n2 = row_of(s + D);
                qu[j] = Ug[(size_t)n2 * 64];
                qw[j] = Wg[(size_t)n2 * 64];
            }
        }
    }
    F = fma(prev, carry, F);                        // pending folded (lower: decay left to the next chunk)
    if (up && de_up >= 0.0) F *= fm_exp(-cj * de_up);       // upper: cross the chunk's first-row boundary
    Fg[lane] = F;
}

// R right-hand sides: lane r owns column r of Y/Z and F[:, r] (ROWS doubles in VGPRs); the
// generator rows are staged per row in LDS and read back as wave-uniform operands.
template <int ROWS>
__global__ void __launch_bounds__(64) k_linR(const LinArgs A) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;                       // (problem, chunk)
    const int rt = blockIdx.y;                      // RHS tile of 64 columns
    const int pr = b / A.nch, ch = b - pr * A.nch;
    const int R = A.R;
    const int r = rt * 64 + lane;
    const bool rok = r < R;
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int64_t rows = (A.N - c0 < A.chunk_len) ? (A.N - c0) : A.chunk_len;
    const size_t pb = (size_t)pr * A.N + c0;
    const double *__restrict__ Ug = A.Ut + pb * 64 + lane;
    const double *__restrict__ Wg = A.Wt + pb * 64 + lane;
    const double *__restrict__ dg = A.d + pb;
    const double *__restrict__ eg = A.de + pb;
    const double *__restrict__ Yg = A.Y + pb * R;
    double *__restrict__ Zg = A.Z + pb * R;
    double *__restrict__ Fg = A.F_state + (size_t)b * 64 * R;      // [i][R]
    const double cj = (lane < A.W) ? A.c[(size_t)pr * A.W + lane] : 0.0;
    const bool up = A.mode == GF_SOLVE_UPPER, mm = A.mode == GF_MATMUL_LOWER;
    __shared__ double s_a[64], s_b[64], s_e[64];
    double F[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) F[i] = (rok && A.store) ? Fg[(size_t)i * R + r] : 0.0;
    double carry = 0.0;
    s_a[lane] = 0.0;                                // pending push row (w~_{n-1} or u~_{n+1})
    double de_cross = -1.0;
    // everything a row needs from memory is fetched three rows ahead (the loads used to sit at
    // their point of use: one full memory round trip per row, 5 us)
    struct RowIn { double y, pull, push, e, d; };
    auto fetch = [&](int64_t s) {
        if (s > rows - 1) s = rows - 1;
        const int64_t n = up ? (rows - 1 - s) : s;
        RowIn q;
        q.y = rok ? Yg[(size_t)n * R + r] : 0.0;
        q.pull = up ? Wg[(size_t)n * 64] : Ug[(size_t)n * 64];
        q.push = up ? Ug[(size_t)n * 64] : Wg[(size_t)n * 64];
        q.e = eg[n];
        q.d = A.scale ? dg[n] : 1.0;
        return q;
    };
    RowIn p0 = fetch(0), p1 = fetch(1), p2 = fetch(2);
    for (int64_t s = 0; s < rows; ++s) {
        const int64_t n = up ? (rows - 1 - s) : s;
        const RowIn cur = p0;
        p0 = p1; p1 = p2; p2 = fetch(s + 3);
        double yn = cur.y;
        if (A.scale) yn = mm ? yn * sqrt(cur.d) : yn / cur.d;
        const double de = up ? de_cross : cur.e;    // decay to apply before this row's dot
        wave_lds_fence();
        s_b[lane] = cur.pull;
        const bool dec = de >= 0.0;
        if (dec) s_e[lane] = fm_exp(-cj * de);
        wave_lds_fence();
        double dot = 0.0, dot2 = 0.0;
        if (dec) {
#pragma unroll
            for (int i = 0; i < ROWS; i += 2) {
                F[i] = fma(s_a[i], carry, F[i]) * s_e[i];
                dot = fma(s_b[i], F[i], dot);
                F[i + 1] = fma(s_a[i + 1], carry, F[i + 1]) * s_e[i + 1];
                dot2 = fma(s_b[i + 1], F[i + 1], dot2);
            }
        } else {
#pragma unroll
            for (int i = 0; i < ROWS; i += 2) {
                F[i] = fma(s_a[i], carry, F[i]);
                dot = fma(s_b[i], F[i], dot);
                F[i + 1] = fma(s_a[i + 1], carry, F[i + 1]);
                dot2 = fma(s_b[i + 1], F[i + 1], dot2);
            }
        }
        dot += dot2;
        const double zn = mm ? (yn + dot) : (yn - dot);
        if (A.store && rok) Zg[(size_t)n * R + r] = zn;
        carry = mm ? yn : zn;
        wave_lds_fence();
        s_a[lane] = cur.push;
        if (up) de_cross = cur.e;
    }
    wave_lds_fence();
    const bool dec = up && de_cross >= 0.0;
    if (dec) s_e[lane] = fm_exp(-cj * de_cross);
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        double v = fma(s_a[i], carry, F[i]);
        if (dec) v *= s_e[i];
        if (rok) Fg[(size_t)i * R + r] = v;
    }
}

// k_linR in k_factor7's lane tiling.  k_linR gives every lane ONE right-hand side and all ROWS state
// rows, so each FMA takes a wave-uniform row operand through an LDS broadcast read: 2 ROWS reads per row,
// and with eight waves per CU the LDS array -- not the 2 ROWS FMAs -- set the pace (4 % of the HBM roofline
// on cfg5).  The per-row update is exactly k_factor7's sweep (T += a q^T ; dot += b^T T with T = the
// state, columns = right-hand sides, q = the carries), so it takes the same tiling: lane (g, c) holds the
// right-hand sides 2c, 2c + 1 of half the state rows (pairs 4k + 2g, 4k + 2g + 1), one ds_read_b128
// feeds 8 FMAs (ROWS / 2 reads per row instead of 2 ROWS), and the lane's OWN right-hand side 2c + g
// (its y, z and carry) is connected to its two state columns by the same two v_permlane32_swap pairs.
// NODOT: the local pass of GF_MATMUL_LOWER (dot_tril) -- its carries are the inputs themselves, so the
// pass only accumulates the state: half the FMAs, no reduction.
template <int ROWS, bool NODOT>
__global__ void __launch_bounds__(64, 2) k_linR7(const LinArgs A) {
    const int lane = threadIdx.x;
    const int g = lane >> 5, c = lane & 31;
    const int b = blockIdx.x;                       // (problem, chunk)
    const int rt = blockIdx.y;                      // RHS tile of 64 columns
    const int pr = b / A.nch, ch = b - pr * A.nch;
    const int R = A.R;
    const int r = rt * 64 + 2 * c + g;              // this lane's own right-hand side
    const bool rok = r < R;
    const int r0 = rt * 64 + 2 * c;                 // its two state columns: r0, r0 + 1
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int64_t rows = (A.N - c0 < A.chunk_len) ? (A.N - c0) : A.chunk_len;
    const size_t pb = (size_t)pr * A.N + c0;
    const double *__restrict__ Ug = A.Ut + pb * 64 + lane;
    const double *__restrict__ Wg = A.Wt + pb * 64 + lane;
    const double *__restrict__ dg = A.d + pb;
    const double *__restrict__ eg = A.de + pb;
    const double *__restrict__ Yg = A.Y + pb * R;
    double *__restrict__ Zg = A.Z + pb * R;
    double *__restrict__ Fg = A.F_state + (size_t)b * 64 * R;      // [i][R]
    const double cj = (lane < A.W) ? A.c[(size_t)pr * A.W + lane] : 0.0;
    const bool up = A.mode == GF_SOLVE_UPPER, mm = A.mode == GF_MATMUL_LOWER;
    __shared__ __attribute__((aligned(16))) double s_a[64], s_b[64], s_e[64];
    const double2 *pa = (const double2 *)s_a + g, *pb2 = (const double2 *)s_b + g;
    const double2 *pe = (const double2 *)s_e + g;
    double T[ROWS / 2][2];
#pragma unroll
    for (int m2 = 0; m2 < ROWS / 2; ++m2) {
        const int i = 4 * (m2 >> 1) + 2 * g + (m2 & 1);
        T[m2][0] = (r0 < R && A.store) ? Fg[(size_t)i * R + r0] : 0.0;
        T[m2][1] = (r0 + 1 < R && A.store) ? Fg[(size_t)i * R + r0 + 1] : 0.0;
    }
    double q0 = 0.0, q1 = 0.0, carry = 0.0;
    s_a[lane] = 0.0;                                // pending push row (w~_{n-1} or u~_{n+1})
    double de_cross = -1.0;
    struct RowIn { double y, pull, push, e, d; };
    auto fetch = [&](int64_t s) {
        if (s > rows - 1) s = rows - 1;
        const int64_t n = up ? (rows - 1 - s) : s;
        RowIn q;
        q.y = rok ? Yg[(size_t)n * R + r] : 0.0;
        q.pull = up ? Wg[(size_t)n * 64] : Ug[(size_t)n * 64];
        q.push = up ? Ug[(size_t)n * 64] : Wg[(size_t)n * 64];
        q.e = eg[n];
        q.d = A.scale ? dg[n] : 1.0;
        return q;
    };
    RowIn p0 = fetch(0), p1 = fetch(1), p2 = fetch(2);
    double2 ub[S7_AHEAD + 1], wb[S7_AHEAD + 1];
    for (int64_t s = 0; s < rows; ++s) {
        const int64_t n = up ? (rows - 1 - s) : s;
        const RowIn cur = p0;
        p0 = p1; p1 = p2; p2 = fetch(s + 3);
        double yn = cur.y;
        if (A.scale) yn = mm ? yn * sqrt(cur.d) : yn / cur.d;
        const double de = up ? de_cross : cur.e;    // decay to apply before this row's dot
        wave_lds_fence();
        s_b[lane] = cur.pull;
        const bool dec = de >= 0.0;
        if (dec) s_e[lane] = fm_exp(-cj * de);
        wave_lds_fence();
        if (dec) {                                  // fold the pending push, decay the state rows
            double d0, d1;
            sweep7_preload<ROWS>(ub, wb, pe, pa);
            sweep7_run<ROWS, true>(T, ub, wb, pe, pa, q0, q1, 1.0, 1.0, d0, d1);
            q0 = 0.0;
            q1 = 0.0;
        }
        if constexpr (NODOT) {
#pragma unroll
            for (int k = 0; k < ROWS / 4; ++k) {
                const double2 w = pa[2 * k];
                T[2 * k][0] = fma(w.x, q0, T[2 * k][0]);
                T[2 * k][1] = fma(w.x, q1, T[2 * k][1]);
                T[2 * k + 1][0] = fma(w.y, q0, T[2 * k + 1][0]);
                T[2 * k + 1][1] = fma(w.y, q1, T[2 * k + 1][1]);
            }
            carry = yn;
        } else {
            double acc0, acc1;
            __builtin_amdgcn_s_setprio(0);
            sweep7_preload<ROWS>(ub, wb, pb2, pa);
            sweep7_run<ROWS, false>(T, ub, wb, pb2, pa, q0, q1, 0.0, 0.0, acc0, acc1);
            __builtin_amdgcn_s_setprio(GF_CHAIN_PRIO);
            const double dot = own_column_sum(acc0, acc1);
            const double zn = mm ? (yn + dot) : (yn - dot);
            if (A.store && rok) Zg[(size_t)n * R + r] = zn;
            carry = mm ? yn : zn;
        }
        both_halves(carry, q0, q1);                 // the carries of this lane's two state columns
        wave_lds_fence();
        s_a[lane] = cur.push;
        if (up) de_cross = cur.e;
    }
    wave_lds_fence();
    const bool dec = up && de_cross >= 0.0;
    if (dec) s_e[lane] = fm_exp(-cj * de_cross);
    wave_lds_fence();
#pragma unroll
    for (int m2 = 0; m2 < ROWS / 2; ++m2) {
        const int i = 4 * (m2 >> 1) + 2 * g + (m2 & 1);
        double v0 = fma(s_a[i], q0, T[m2][0]), v1 = fma(s_a[i], q1, T[m2][1]);
        if (dec) { v0 *= s_e[i]; v1 *= s_e[i]; }
        if (r0 < R) Fg[(size_t)i * R + r0] = v0;
        if (r0 + 1 < R) Fg[(size_t)i * R + r0 + 1] = v1;
    }
}

// GF_MATMUL_LOWER (dot_tril, GP.sample) with many right-hand sides on the matrix pipe.  The sweep has no
// feedback in this mode (the carries are the inputs), so 16 rows at a time are plain products:
//     Z_b = Y_b + U_b F + strict_lower(U_b W_b^T) Y_b ,     F <- F + W_b^T Y_b
// (U_b, W_b: the block's 16 rows of u~, w~; F: W x R state; decay E o F first when the block starts on a
// reset row; a reset inside a block cuts it there, rows past the cut are masked).  k_linR7 does the same
// arithmetic row by row and runs at the pace of its LDS broadcasts (30 ds_read_b128 per row and wave: 14.9 %
// of the HBM roofline on cfg5).  Here one wave owns 64 right-hand sides of one chunk; everything is
// v_mfma_f64_16x16x4 (lane (i, k) = (lane & 15, lane >> 4) supplies A[i][4 s + k], B[4 s + k][i] of slice s
// and receives D[k + 4 r][i], r = 0..3), laid out so that no result ever changes lanes:
//   * the accumulators of  F += W_b^T Y_b  (tile mt, register r = state 16 mt + k + 4 r) ARE the B
//     operands of  U_b F  (slice s = 4 mt + r <-> state 4 s + k);
//   * the C layout of  G^T = W_b U_b^T  is the A layout of  strict_lower(G) Y_b  (entry (i, k + 4 r));
//   * the B operand rows of Y_b (4 s + k) are the C rows of Z_b (k + 4 r): one load serves both.
// 16 + 36 T MFMAs per block and wave (T = 4 tiles of 16 right-hand sides: the rows are read once), 16 T for
// the local pass; one wave per SIMD (the state alone is 128 accumulator registers).
// The block's u~ / w~ rows (2 x 8 KB, contiguous in memory) come in as flat 16-byte loads issued one block
// ahead, go through an LDS tile (row stride 66: the A-operand reads are conflict-free) and are read slice by
// slice at their point of use.  Taking the operands from global in their MFMA layout instead cost more than
// the MFMAs: a lane-per-row pattern is 64 separate sectors per load instruction (the texture addresser
// serialises them), and a masked load in a branch of its own gets its own s_waitcnt (30 round trips per block).
template <int MT, bool NODOT, int NWV>
__global__ void __launch_bounds__(64 * NWV, (NWV == 1 && !NODOT) ? 1 : 2) k_mmR_mfma(const LinArgs A) {
    constexpr int KS = 4 * MT, T = 2, LDT = 66, NQ = 8 / NWV;
    const int lane = threadIdx.x & 63, i = lane & 15, k = lane >> 4;
    const int wv = (NWV > 1) ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
    const int b = blockIdx.x, rt = blockIdx.y;
    const int pr = b / A.nch, ch = b - pr * A.nch;
    const int R = A.R;
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int rows = (int)((A.N - c0 < A.chunk_len) ? (A.N - c0) : A.chunk_len);
    const size_t pb = (size_t)pr * A.N + c0;
    const double *__restrict__ Ug = A.Ut + pb * 64;
    const double *__restrict__ Wg = A.Wt + pb * 64;
    const double *__restrict__ dg = A.d + pb;
    const double *__restrict__ eg = A.de + pb;
    const double *__restrict__ Yg = A.Y + pb * R;
    double *__restrict__ Zg = A.Z + pb * R;
    double *__restrict__ Fg = A.F_state + (size_t)b * 64 * R;      // [state][R]
    __shared__ double s_e[NWV][64];                 // decays of the states at a reset row
    const double c_lane = (lane < A.W) ? A.c[(size_t)pr * A.W + lane] : 0.0;
    // the block's rows, two buffers: a wave that runs ahead stashes block n + 1 while its partner still
    // reads block n (one barrier per block)
    __shared__ __attribute__((aligned(16))) double s_u[NODOT ? 2 : 2 * 16 * LDT], s_w[2 * 16 * LDT];
    int rhs[T], rhc[T];                             // (rhc: clamped, loads are unconditional; masks come after)
    bool rok[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        rhs[t] = (rt * NWV + wv) * 16 * T + 16 * t + i; rok[t] = rhs[t] < R; rhc[t] = rok[t] ? rhs[t] : R - 1;
    }
    d4 F[T][MT];                                    // F[t][mt][r] = state 16 mt + k + 4 r, rhs[t]
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)     // (the local pass starts from zero)
                F[t][mt][r] = NODOT ? 0.0 : Fg[(size_t)(16 * mt + k + 4 * r) * R + rhc[t]];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) F[t][mt][r] = rok[t] ? F[t][mt][r] : 0.0;
    // one block of inputs, as loaded (rows clamped to the chunk; no branch around any load); the waves of
    // the workgroup share the copy of the u~ / w~ rows (row 2 NWV q + 2 wv + (lane >> 5) of the tile)
    double pux[NODOT ? 1 : NQ], puy[NODOT ? 1 : NQ], pwx[NQ], pwy[NQ];
    double e_raw, d_raw, yraw[T][4];
#define GF_MM_FETCH(N0)                                                                             \
    do {                                                                                            \
        const int f_n0 = (N0);                                                                      \
        const int f_lim = (rows - f_n0 < 16) ? rows - f_n0 : 16;                                    \
        e_raw = eg[f_n0 + ((lane < f_lim) ? lane : f_lim - 1)];                                     \
        d_raw = dg[f_n0 + (((lane & 15) < f_lim) ? (lane & 15) : f_lim - 1)];                       \
        _Pragma("unroll")                                                                           \
        for (int s4 = 0; s4 < 4; ++s4) {                                                            \
            const int f_row = 4 * s4 + k;                                                           \
            const size_t f_n = (size_t)(f_n0 + ((f_row < f_lim) ? f_row : f_lim - 1));              \
            _Pragma("unroll")                                                                       \
            for (int t = 0; t < T; ++t) yraw[t][s4] = Yg[f_n * R + rhc[t]];                         \
        }                                                                                           \
        _Pragma("unroll")                                                                           \
        for (int q = 0; q < NQ; ++q) {  /* flat copy: 16-byte pieces of the 16 x 64 tile */         \
            const int f_row = 2 * NWV * q + 2 * wv + (lane >> 5);                                   \
            const size_t f_off = (size_t)(f_n0 + ((f_row < f_lim) ? f_row : f_lim - 1)) * 64 + 2 * (lane & 31); \
            const double2 f_w = *reinterpret_cast<const double2 *>(Wg + f_off);                     \
            pwx[q] = f_w.x; pwy[q] = f_w.y;                                                         \
            if constexpr (!NODOT) {                                                                 \
                const double2 f_u = *reinterpret_cast<const double2 *>(Ug + f_off);                 \
                pux[q] = f_u.x; puy[q] = f_u.y;                                                     \
            }                                                                                       \
        }                                                                                           \
    } while (0)
    GF_MM_FETCH(0);
    int buf = 0;
    for (int n0 = 0; n0 < rows; buf ^= 1) {
        const int lim = (rows - n0 < 16) ? rows - n0 : 16;
        const double *su = s_u + (NODOT ? 0 : buf * 16 * LDT), *sw = s_w + buf * 16 * LDT;
        if (NWV == 1) wave_lds_fence();             // (the block before the previous one has been read)
        // the block: rows n0 .. n0 + cnt - 1, cut at the first reset row after n0
        const double e_l = (lane < lim) ? e_raw : -1.0;
        const unsigned long long inner = __ballot(e_l >= 0.0 && lane >= 1);
        const int cnt = inner ? (int)__ffsll((long long)inner) - 1 : lim;
        const double de0 = read_lane(e_l, 0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {              // (rows past the cut enter the tile as zeros: no operand masks)
            const int row = 2 * NWV * q + 2 * wv + (lane >> 5);
            const int at = buf * 16 * LDT + row * LDT + 2 * (lane & 31);
            const bool in = row < cnt;
            *reinterpret_cast<double2 *>(&s_w[at]) = double2{in ? pwx[q] : 0.0, in ? pwy[q] : 0.0};
            if constexpr (!NODOT) *reinterpret_cast<double2 *>(&s_u[at]) = double2{in ? pux[q] : 0.0, in ? puy[q] : 0.0};
        }
        double yv[T][4];                            // rows n0 + 4 s + k (B operand of slice s; C rows of Z_b)
        bool okK[4];
        const double sq = A.scale ? sqrt(d_raw) : 1.0;      // lane l: sqrt(d) of row n0 + (l & 15)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            okK[s4] = 4 * s4 + k < cnt;
            const double sc = A.scale ? __shfl(sq, 4 * s4 + k) : 1.0;
#pragma unroll
            for (int t = 0; t < T; ++t) yv[t][s4] = (okK[s4] && rok[t]) ? yraw[t][s4] * sc : 0.0;
        }
        if (NWV == 1) wave_lds_fence(); else wg_lds_barrier();
        // the next block's loads fly under this block's MFMAs (past the chunk's end: the last row again,
        // never used -- an unconditional fetch keeps the staging registers out of scratch)
        GF_MM_FETCH((n0 + cnt < rows) ? n0 + cnt : rows - 1);
        if (de0 >= 0.0) {
            // reset row: F <- E o F before the block's products.  Lane l forms the decay of state l, the
            // lanes pick theirs (state 16 mt + k + 4 r) up from LDS: one exponential and 8 T multiplies per
            // lane.  (As diag(E) F on the matrix pipe -- the form this kernel had while F lived in accumulator
            // registers -- the decay cost 16 T MFMAs per reset: half the local pass when every 16-row block
            // starts on one, as with the solar-like kernels at one-minute cadence.)
            s_e[wv][lane] = fm_exp(-c_lane * de0);
            wave_lds_fence();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double e = s_e[wv][16 * mt + k + 4 * r];
#pragma unroll
                    for (int t = 0; t < T; ++t) F[t][mt][r] *= e;
                }
        }
        if constexpr (!NODOT) {
            d4 G = {0.0, 0.0, 0.0, 0.0};            // G^T = W_b U_b^T: lane (i, k) gets u~_i . w~_{k + 4 r}
            d4 Z[T];
#pragma unroll
            for (int t = 0; t < T; ++t) Z[t] = d4{yv[t][0], yv[t][1], yv[t][2], yv[t][3]};
#pragma unroll
            for (int s = 0; s < KS; ++s) {          // u~, w~[n0 + i][4 s + k]
                const double ua = su[i * LDT + 4 * s + k], wa = sw[i * LDT + 4 * s + k];
                G = GF_MFMA64(wa, ua, G);
#pragma unroll
                for (int t = 0; t < T; ++t) Z[t] = GF_MFMA64(ua, F[t][s >> 2][s & 3], Z[t]);
                if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // (operand reads stay near their use)
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) if (k + 4 * r >= i) G[r] = 0.0;        // strictly lower
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) Z[t] = GF_MFMA64(G[s4], yv[t][s4], Z[t]);
                if (A.store && rok[t]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k + 4 * r < cnt) Zg[(size_t)(n0 + k + 4 * r) * R + rhs[t]] = Z[t][r];
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {        // w~[n0 + 4 s + k][16 mt + i]
                const double wt = sw[(4 * s4 + k) * LDT + 16 * mt + i];
#pragma unroll
                for (int t = 0; t < T; ++t) F[t][mt] = GF_MFMA64(wt, yv[t][s4], F[t][mt]);
            }
        n0 += cnt;
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (rok[t]) Fg[(size_t)(16 * mt + k + 4 * r) * R + rhs[t]] = F[t][mt][r];
}
#undef GF_MM_FETCH

constexpr int LC_TRANSPOSED = 0x100;     // (flag on the combine kernels' mode: transitions handed over transposed)

// Linear combine of the chunk states of a sweep: on entry F_state slot c holds chunk c's end
// state from a zero start (local pass); on exit it holds the TRUE start state of chunk c.
//   lower  : F_{c+1} = Fbar_c + Phi_c F_c            (ascending; Phi = true closed-loop transition)
//   upper  : G_{c-1} = Gbar_c + Phi_c^T G_c          (descending)
//   matmul : F_{c+1} = Fbar_c + D_c o F_c            (D = product of the chunk's reset decays)
// One workgroup of 64 x RT threads per (problem, RHS tile); Phi is stored [j][i].
//
// Two-level form (PHASE 1 / 2; PHASE 0 is the plain scan over all chunks): the chunks are cut into
// segments of seg_len whose composed transitions Psi_s = Phi_{e-1} ... Phi_b are part of the factor
// (k_segment_transition, once per factor; the backward solve uses Psi_s^T).  PHASE 1 scans every
// segment concurrently from a zero start and leaves its end state in Vseg; a PHASE 0 scan of
// (Psi, Vseg) turns those into the segments' true start states; PHASE 2 rescans every segment from
// there and writes the chunks' start states.  Sequential depth 2 seg_len + nch / seg_len chunks
// instead of nch.
template <int PHASE>
__global__ void __launch_bounds__(256)
k_lincombine(const int nch, const int seg_len, const int mode_, const int R,
             const double *__restrict__ Phi_, const double *__restrict__ Dch_,
             double *__restrict__ F_state, double *__restrict__ Vseg) {
    // mode_ | LC_TRANSPOSED: Phi_ holds the TRANSPOSED transitions (backward solve): its loads then run along the
    // lanes like the forward solve's (a row of Phi^T per lane is one 128-byte run per lane and load: 0.12 against
    // 0.07 ms for the scan of 1954 chunks)
    const int mode = mode_ & ~LC_TRANSPOSED;
    const bool pre_t = (mode_ & LC_TRANSPOSED) != 0;
    // One workgroup of four waves per (problem, right-hand side): the scan is sequential over the
    // chunks only.  Lane i owns state row i; wave w multiplies columns 16w..16w+15 of the chunk's
    // 64 x 64 transition (rows of Phi^T for the backward solve), which it holds in registers and
    // fetches THREE chunks ahead (a ring of four 16-double buffers: the 32 KB per chunk come from
    // L2 with ~2 us latency, which a single buffer exposed on every step: 2.3 us per chunk, now
    // ~0.4); the four partial sums meet in LDS, one barrier per chunk.
    const int r = blockIdx.y, i = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool up = mode == GF_SOLVE_UPPER, mm = mode == GF_MATMUL_LOWER;
    const int nseg = PHASE ? (nch + seg_len - 1) / seg_len : 1;
    const int pr = blockIdx.x / nseg, sg = blockIdx.x - pr * nseg;
    const int c_lo = PHASE ? sg * seg_len : 0;
    const int c_hi = PHASE ? ((c_lo + seg_len < nch) ? c_lo + seg_len : nch) : nch;
    const int len = c_hi - c_lo;
    __shared__ __attribute__((aligned(16))) double s_cur[64];
    __shared__ double s_part[2][4][64];
    double P[4][16];
    auto chunk_of = [&](int s) { return up ? (c_hi - 1 - s) : (c_lo + s); };
    auto load_phi = [&](double (&buf)[16], int s) {
        if (s >= len) return;
        const double *Pg = Phi_ + ((size_t)pr * nch + chunk_of(s)) * 4096;
        if (!up || pre_t) {
#pragma unroll
            for (int j = 0; j < 16; ++j) buf[j] = Pg[(size_t)(16 * w + j) * 64 + i];    // Phi(i, j) (or Phi^T's)
        } else {
            const double2 *row = reinterpret_cast<const double2 *>(Pg + (size_t)i * 64 + 16 * w);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double2 v = row[j]; buf[2 * j] = v.x; buf[2 * j + 1] = v.y; }  // Phi(j, i)
        }
    };
    double cur = 0.0;                               // state row i (carried by wave 0)
    double *Vg = PHASE ? Vseg + ((size_t)pr * nseg + sg) * 64 * R + (size_t)i * R + r : nullptr;
    if (PHASE == 2 && w == 0) cur = *Vg;
    if (PHASE == 0 && mm) {                         // diagonal transitions: one wave does it all
        if (w != 0) return;
        constexpr int GB = 16;                      // (loads of sixteen chunks ahead of their dependent FMAs)
        for (int s0 = 0; s0 < nch; s0 += GB) {
            double loc[GB], dd[GB];
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                const int s = (s0 + k < nch) ? s0 + k : nch - 1;
                const size_t slot = (size_t)pr * nch + s;
                loc[k] = F_state[slot * 64 * R + (size_t)i * R + r];
                dd[k] = Dch_[slot * 64 + i];
            }
#pragma unroll
            for (int k = 0; k < GB; ++k) {
                if (s0 + k < nch) {
                    const size_t slot = (size_t)pr * nch + s0 + k;
                    F_state[slot * 64 * R + (size_t)i * R + r] = cur;
                    cur = fma(dd[k], cur, loc[k]);
                }
            }
        }
        return;
    }
    load_phi(P[0], 0); load_phi(P[1], 1); load_phi(P[2], 2);
    if (threadIdx.x < 64) s_cur[i] = cur;
    __syncthreads();
    auto step = [&](double (&buf)[16], double (&next)[16], int s) {
        const size_t slot = (size_t)pr * nch + chunk_of(s);
        double *Fg = F_state + slot * 64 * R + (size_t)i * R + r;
        double loc = 0.0;
        if (w == 0) { loc = *Fg; if (PHASE != 1) *Fg = cur; }   // local end state in, true start state out
        load_phi(next, s + 3);
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
            a0 = fma(buf[j], s_cur[16 * w + j], a0);
            a1 = fma(buf[j + 1], s_cur[16 * w + j + 1], a1);
        }
        s_part[s & 1][w][i] = a0 + a1;
        __syncthreads();
        if (w == 0) {                               // wave 0 carries the state
            const double *sp = &s_part[s & 1][0][0];
            cur = loc + ((sp[i] + sp[64 + i]) + (sp[128 + i] + sp[192 + i]));
            s_cur[i] = cur;
        }
        __syncthreads();
    };
    int s = 0;
    for (; s + 4 <= len; s += 4) {
        step(P[0], P[3], s);
        step(P[1], P[0], s + 1);
        step(P[2], P[1], s + 2);
        step(P[3], P[2], s + 3);
    }
    if (s < len) step(P[0], P[3], s);
    if (s + 1 < len) step(P[1], P[0], s + 1);
    if (s + 2 < len) step(P[2], P[1], s + 2);
    if (PHASE == 1 && w == 0) *Vg = cur;            // the segment's end state from a zero start
}

// The segment scans (PHASE 1 / 2 of k_lincombine) for MANY right-hand sides: 64 at a time, the chunk step
// S <- Fbar_c + Phi_c S (Phi_c^T for the backward solve) as one 64 x 64 x 64 product on the matrix pipe.  One
// workgroup per (problem, segment, 64 right-hand sides): the state S [j][r] sits in LDS as the B operand, Phi_c is
// the A operand straight from global -- lane (i, k) of wave w supplies Phi(16 w + i, 4 ks + k) -- fetched one chunk
// ahead together with the chunk's local end state (in accumulator layout: the MFMAs start from it).  One workgroup
// per right-hand side re-read every Phi_c 64 times and took 0.38 ms per phase for 64 right-hand sides at 1954
// chunks (a quarter of predict(return_var=True)); this one streams them once.
template <int PHASE>
__global__ void __launch_bounds__(256)
k_lincombine_R(const int nch, const int seg_len, const int mode_, const int R,
               const double *__restrict__ Phi_, double *__restrict__ F_state, double *__restrict__ Vseg) {
    const int mode = mode_ & ~LC_TRANSPOSED;
    const bool pre_t = (mode_ & LC_TRANSPOSED) != 0;         // (Phi_ holds the transposed transitions)
    constexpr int LDB = 80;                         // (rows k, k + 1 of the B operand 32 banks apart)
    __shared__ __attribute__((aligned(16))) double Sb[64 * LDB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, k = lane >> 4;
    const bool up = mode == GF_SOLVE_UPPER;
    const int nseg = (nch + seg_len - 1) / seg_len;
    const int pr = blockIdx.x / nseg, sg = blockIdx.x - pr * nseg;
    const int r0 = 64 * blockIdx.y;
    const int c_lo = sg * seg_len, c_hi = (c_lo + seg_len < nch) ? c_lo + seg_len : nch, len = c_hi - c_lo;
    auto chunk_of = [&](int sidx) { return up ? (c_hi - 1 - sidx) : (c_lo + sidx); };
    // a 64 x 64 block of a state array [64][R] in accumulator layout: x[q][rr] = (row 16 w + k + 4 rr, column r0 + 16 q + i)
    auto ld_state = [&](const double *base, d4 (&x)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int col = r0 + 16 * q + i;
                x[q][rr] = (col < R) ? base[(size_t)(16 * w + k + 4 * rr) * R + col] : 0.0;
            }
    };
    auto st_state = [&](double *base, const d4 (&x)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int col = r0 + 16 * q + i;
                if (col < R) base[(size_t)(16 * w + k + 4 * rr) * R + col] = x[q][rr];
            }
    };
    auto ld_A = [&](double (&a)[16], const int sidx) {
        if (sidx >= len) return;
        const double *Pg = Phi_ + ((size_t)pr * nch + chunk_of(sidx)) * 4096;      // Phi(i, j) at [j][i]
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
            a[ks] = (up && !pre_t) ? Pg[(size_t)(16 * w + i) * 64 + 4 * ks + k] : Pg[(size_t)(4 * ks + k) * 64 + 16 * w + i];
    };
    auto slot_of = [&](int sidx) { return F_state + ((size_t)pr * nch + chunk_of(sidx)) * 64 * R; };
    d4 cur[4];
    double *Vg = Vseg + ((size_t)pr * nseg + sg) * 64 * R;
    if (PHASE == 2) ld_state(Vg, cur);
    else {
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = d4{0.0, 0.0, 0.0, 0.0};
    }
    auto put = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) Sb[(16 * w + k + 4 * rr) * LDB + 16 * q + i] = cur[q][rr];
    };
    put();
    double a0[16], a1[16];
    d4 l0[4], l1[4];
    ld_A(a0, 0);
    ld_state(slot_of(0), l0);
    __syncthreads();
    auto step = [&](double (&a)[16], d4 (&loc)[4], double (&an)[16], d4 (&locn)[4], const int sidx) {
        ld_A(an, sidx + 1);
        if (sidx + 1 < len) ld_state(slot_of(sidx + 1), locn);
        if (PHASE == 2) st_state(slot_of(sidx), cur);           // local end state in (above), true start state out
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = loc[q];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const double av = a[ks];
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = GF_MFMA64(av, Sb[(4 * ks + k) * LDB + 16 * q + i], cur[q]);
        }
        __syncthreads();                            // every wave has read the old state
        put();
        __syncthreads();
    };
    int sidx = 0;
    for (; sidx + 2 <= len; sidx += 2) {
        step(a0, l0, a1, l1, sidx);
        step(a1, l1, a0, l0, sidx + 1);
    }
    if (sidx < len) step(a0, l0, a1, l1, sidx);
    if (PHASE == 1) st_state(Vg, cur);              // the segment's end state from a zero start
}

// Combine of GF_MATMUL_LOWER (dot_tril): the chunk transitions are DIAGONAL (D_c), so the start states are
// a plain scan  F_{c+1} = loc_c + D_c o F_c  of 64 x R independent scalar sequences.  One workgroup of 16
// waves per (problem, state row, 16 right-hand sides): a wave's four 16-lane groups take one segment of the
// chunks each (64 segments per workgroup), lane & 15 = right-hand side (the states are stored [row][R]: 128-byte
// pieces of a row; with lane = state row every lane touched its own cache line).  The segments are scanned
// concurrently (zero start; eight chunks of loads in flight per lane: the loop is otherwise one dependent memory
// round trip per chunk), the 64 segment summaries are chained in LDS, and every group rescans its segment from
// its true start state, writing the start state of every chunk.  (With lane = right-hand side over all 64 and
// 16 segments there were 64 workgroups per problem: a quarter of the chip, 45 us at cfg5's size.)
constexpr int LCM_WAVES = 16, LCM_BATCH = 8, LCM_SEGS = 4 * LCM_WAVES;
__global__ void __launch_bounds__(64 * LCM_WAVES)
k_lincombine_mm(const int nch, const int R, const int rows, const double *__restrict__ Dch_,
                double *__restrict__ F_state) {
    const int pr = blockIdx.x, i = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rr = lane & 15, sg = 4 * w + (lane >> 4);        // right-hand side within the 16, segment
    const int rq = 16 * blockIdx.z + rr;
    const int r = (rq < R) ? rq : (R - 1);          // idle lanes shadow the last right-hand side (no stores)
    const bool rok = rq < R;
    const int seg = (nch + LCM_SEGS - 1) / LCM_SEGS;
    const int s0 = (sg * seg < nch) ? sg * seg : nch, s1 = (s0 + seg < nch) ? (s0 + seg) : nch;
    __shared__ double s_end[LCM_SEGS][16], s_dec[LCM_SEGS][16];
    auto F_at = [&](int s) { return F_state + ((size_t)pr * nch + s) * rows * R + (size_t)i * R + r; };
    auto D_at = [&](int s) { return Dch_[((size_t)pr * nch + s) * rows + i]; };
    // phase 1: segment end state from a zero start, and the segment's total decay
    double cur = 0.0, dec = 1.0;
    for (int s = s0; s < s1; s += LCM_BATCH) {
        double loc[LCM_BATCH], dd[LCM_BATCH];
#pragma unroll
        for (int j = 0; j < LCM_BATCH; ++j) {
            const bool ok = s + j < s1;
            loc[j] = ok ? *F_at(s + j) : 0.0;
            dd[j] = ok ? D_at(s + j) : 1.0;
        }
#pragma unroll
        for (int j = 0; j < LCM_BATCH; ++j) { cur = fma(dd[j], cur, loc[j]); dec *= dd[j]; }
    }
    s_end[sg][rr] = cur;
    s_dec[sg][rr] = dec;
    __syncthreads();
    // phase 2: this segment's true start state (chain of the summaries before it)
    double start = 0.0;
    for (int g2 = 0; g2 < sg; ++g2) start = fma(s_dec[g2][rr], start, s_end[g2][rr]);
    // phase 3: rescan, leaving the true start state of every chunk in its slot
    cur = start;
    for (int s = s0; s < s1; s += LCM_BATCH) {
        double loc[LCM_BATCH], dd[LCM_BATCH];
#pragma unroll
        for (int j = 0; j < LCM_BATCH; ++j) {
            const bool ok = s + j < s1;
            loc[j] = ok ? *F_at(s + j) : 0.0;
            dd[j] = ok ? D_at(s + j) : 1.0;
        }
#pragma unroll
        for (int j = 0; j < LCM_BATCH; ++j) {
            if (rok && s + j < s1) *F_at(s + j) = cur;
            cur = fma(dd[j], cur, loc[j]);
        }
    }
}

// D_c[j] = exp(-c_j * (sum of the reset spans inside chunk c))   (diagonal chunk transition of
// matmul_lower; the first row of every chunk is a reset row)
__global__ void __launch_bounds__(64)
k_chunk_decay(const int64_t N, const int64_t chunk_len, const int nch, const int W,
              const double *__restrict__ c_, const double *__restrict__ de_, double *__restrict__ D_out) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int pr = b / nch, ch = b - pr * nch;
    const int64_t c0 = (int64_t)ch * chunk_len;
    const int64_t rows = (N - c0 < chunk_len) ? (N - c0) : chunk_len;
    const double *eg = de_ + (size_t)pr * N + c0;
    double acc = 0.0;
    for (int64_t n = lane; n < rows; n += 64) { const double v = eg[n]; if (v > 0.0) acc += v; }
    acc = wave_sum(acc);
    const double cj = (lane < W) ? c_[(size_t)pr * W + lane] : 0.0;
    D_out[(size_t)b * 64 + lane] = fm_exp(-cj * acc);
}

}  // namespace

// ======================================================================================
// C-ABI
// ======================================================================================
extern "C" {

int gf_chunk_linear(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int R,
                    int scale, int store, const double *c,
                    const double *Ut, const double *Wt, const double *d, const double *de,
                    const double *Y, double *Z, double *F_state, void *stream) {
    if (mode < 0 || mode > 2) return gf_internal_error(-1, "gf_chunk_linear: bad mode %d", mode);
    if (B < 1 || N < 1 || R < 1) return gf_internal_error(-1, "gf_chunk_linear: empty problem (N=%lld, R=%d)", (long long)N, R);
    if (W < 1 || W > 63) return gf_internal_error(-1, "gf_chunk_linear: width %d unsupported (1..63)", W);
    if (check_chunking("gf_chunk_linear", N, chunk_len, nch, 1)) return -1;
    if (!c || !Ut || !Wt || !d || !de || !Y || !Z || !F_state) return gf_internal_error(-1, "gf_chunk_linear: null pointer");
    LinArgs A;
    A.N = N; A.chunk_len = chunk_len; A.nch = nch; A.W = W; A.mode = mode; A.scale = scale; A.store = store;
    A.c = c; A.Ut = Ut; A.Wt = Wt; A.d = d; A.de = de; A.Y = Y; A.Z = Z; A.F_state = F_state; A.R = R;
    hipStream_t st = (hipStream_t)stream;
    bool ok = true;
    if (R == 1) {
        hipLaunchKernelGGL(k_lin1, dim3(B * nch), dim3(64), 0, st, A);
    } else if (mode == GF_MATMUL_LOWER && R >= 16) {
        // no feedback in this mode: blocks of 16 rows as matrix products (k_mmR_mfma)
        // two waves per workgroup share the block's rows (32 right-hand sides each); one when R <= 32
        const int nwv = (R > 32) ? 2 : 1;
        const dim3 grid(B * nch, (R + 32 * nwv - 1) / (32 * nwv));
        ok = dispatch_among<1, 2, 3, 4>((W + 15) / 16, [&](auto mt) {
            constexpr int MT = decltype(mt)::value;
            if (nwv == 2) hipLaunchKernelGGL((store ? k_mmR_mfma<MT, false, 2> : k_mmR_mfma<MT, true, 2>), grid, dim3(128), 0, st, A);
            else          hipLaunchKernelGGL((store ? k_mmR_mfma<MT, false, 1> : k_mmR_mfma<MT, true, 1>), grid, dim3(64), 0, st, A);
        });
    } else {
        ok = dispatch_rows((W + 3) / 4 * 4, [&](auto r) {
            constexpr int Rw = decltype(r)::value;
            hipLaunchKernelGGL((mode == GF_MATMUL_LOWER && !store ? k_linR7<Rw, true> : k_linR7<Rw, false>),
                               dim3(B * nch, (R + 63) / 64), dim3(64), 0, st, A);
        });
    }
    if (!ok) return gf_internal_error(-1, "gf_chunk_linear: internal dispatch error");
    return check_launch("gf_chunk_linear");
}

int gf_chunk_linear_combine(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int R,
                            const double *c, const double *de, const double *Phi,
                            double *D_work, double *F_state, void *stream) {
    if (mode < 0 || mode > 2) return gf_internal_error(-1, "gf_chunk_linear_combine: bad mode %d", mode);
    if (B < 1 || nch < 1 || R < 1) return gf_internal_error(-1, "gf_chunk_linear_combine: empty problem");
    if (!F_state || (mode == GF_MATMUL_LOWER ? (!D_work || !c || !de) : !Phi))
        return gf_internal_error(-1, "gf_chunk_linear_combine: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (mode == GF_MATMUL_LOWER) {
        hipLaunchKernelGGL(k_chunk_decay, dim3(B * nch), dim3(64), 0, st, N, chunk_len, nch, W, c, de, D_work);
        hipLaunchKernelGGL(k_lincombine_mm, dim3(B, 64, (R + 15) / 16), dim3(64 * LCM_WAVES), 0, st, nch, R, 64, D_work, F_state);
        return check_launch("gf_chunk_linear_combine");
    }
    hipLaunchKernelGGL(k_lincombine<0>, dim3(B, R), dim3(256), 0, st, nch, nch, mode, R, Phi, D_work, F_state,
                       (double *)nullptr);
    return check_launch("gf_chunk_linear_combine");
}

int gf_chunk_linear_combine_seg(int mode, int B, int nch, int seg_len, int R, const double *Phi,
                                const double *Psi, const double *PhiT, const double *PsiT,
                                double *F_state, double *V_work, void *stream) {
    if (mode != GF_SOLVE_LOWER && mode != GF_SOLVE_UPPER)
        return gf_internal_error(-1, "gf_chunk_linear_combine_seg: bad mode %d (the solves only)", mode);
    if ((PhiT != nullptr) != (PsiT != nullptr)) return gf_internal_error(-1, "gf_chunk_linear_combine_seg: PhiT and PsiT go together");
    if (mode == GF_SOLVE_UPPER && PhiT) { Phi = PhiT; Psi = PsiT; mode |= LC_TRANSPOSED; }
    if (B < 1 || nch < 1 || R < 1 || seg_len < 1) return gf_internal_error(-1, "gf_chunk_linear_combine_seg: empty problem");
    if (!Phi || !Psi || !F_state || !V_work) return gf_internal_error(-1, "gf_chunk_linear_combine_seg: null pointer");
    const int nseg = (nch + seg_len - 1) / seg_len;
    hipStream_t st = (hipStream_t)stream;
    // the segment scans: per right-hand side, or 64 right-hand sides at a time on the matrix pipe
    const bool many = R >= 16;
    const dim3 gridR(B * nseg, (R + 63) / 64);
    if (many) hipLaunchKernelGGL(k_lincombine_R<1>, gridR, dim3(256), 0, st, nch, seg_len, mode, R, Phi, F_state, V_work);
    else hipLaunchKernelGGL(k_lincombine<1>, dim3(B * nseg, R), dim3(256), 0, st, nch, seg_len, mode, R, Phi,
                            (const double *)nullptr, F_state, V_work);
    hipLaunchKernelGGL(k_lincombine<0>, dim3(B, R), dim3(256), 0, st, nseg, nseg, mode, R, Psi,
                       (const double *)nullptr, V_work, (double *)nullptr);
    if (many) hipLaunchKernelGGL(k_lincombine_R<2>, gridR, dim3(256), 0, st, nch, seg_len, mode, R, Phi, F_state, V_work);
    else hipLaunchKernelGGL(k_lincombine<2>, dim3(B * nseg, R), dim3(256), 0, st, nch, seg_len, mode, R, Phi,
                            (const double *)nullptr, F_state, V_work);
    return check_launch("gf_chunk_linear_combine_seg");
}

// Scan of chunk states with DIAGONAL transitions: F_state slot c [rows][R] <- true start state of chunk c
// from the local end states, F_{c+1} = loc_c + D_c o F_c (D [B * nch][rows]); gf_chunk_linear_combine's
// GF_MATMUL_LOWER branch for any number of state rows.
int gf_chunk_diag_scan(int B, int nch, int rows, int R, const double *D, double *F_state, void *stream) {
    if (B < 1 || nch < 1 || rows < 1 || R < 1 || R > 64)
        return gf_internal_error(-1, "gf_chunk_diag_scan: bad shape (rows=%d, R=%d)", rows, R);
    if (!D || !F_state) return gf_internal_error(-1, "gf_chunk_diag_scan: null pointer");
    hipLaunchKernelGGL(k_lincombine_mm, dim3(B, rows, (R + 15) / 16), dim3(64 * LCM_WAVES), 0, (hipStream_t)stream,
                       nch, R, rows, D, F_state);
    return check_launch("gf_chunk_diag_scan");
}

}  // extern "C"
