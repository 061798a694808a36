// Device helpers that the block-scaled sweeps of different kernel families share (all __forceinline__: a unit that
// includes this gets its own inlined copies), and the one constant pair those sweeps and the host share.
//   SC_SPAN, SC_SPAN_LONG, sweep_gap   the reset rule's span (k_build2, the fused sweeps, gf_scaled_span)
//   sweep_preload / sweep_run          one column per lane: k_factor2 (stored rows), k_factor3, k_phi (fused)
//   own_column_sum / both_halves,
//   sweep7_preload / sweep7_run        2 x 32 lane tiling: k_factor7, k_phi7 (fused), k_linR7 (the stored scaled factor)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gadfly_hip.h"

namespace {

// reset(n) = (n % block == 0) or cmax (t_n - t_{n-1}) > gap, with (block - 1) * gap = SC_SPAN: |log rho| <= SC_SPAN.
// The streamed log-likelihood (gf_loglike_fused with GF_SWEEP_LONG_SPAN, one-wave sweeps only) may take
// SC_SPAN_LONG: T~ then stays within e^+-2 SC_SPAN_LONG = e^+-256 of S, u~ / v~ / w~ / F~ within e^+-128 of the
// unscaled rows, far inside FP64's e^+-708 for amplitudes and pivots within 1e+-100 (the host falls
// back to SC_SPAN outside that range).  Every other route -- the time-parallel sweeps, the stored factor, the wide
// kernels -- keeps SC_SPAN: their transition and solve kernels rebuild the reset rows from it.
constexpr double SC_SPAN = 28.0;
constexpr double SC_SPAN_LONG = 128.0;
// the reset gap of a sweep with this scaling block (`variant`: its GF_SWEEP_LONG_SPAN bit)
double sweep_gap(int block, int variant) {
    return (block > 1) ? ((variant & GF_SWEEP_LONG_SPAN) ? SC_SPAN_LONG : SC_SPAN) / (double)(block - 1) : 0.0;
}

// Sweeps over the ROWS register-resident rows of T with wave-uniform row operands read from
// LDS (xa[i], xw[i]), software-pipelined: batches of 4 rows (2 + 2 ds_read_b128), SW_AHEAD
// batches in flight ahead of the FMAs, so the LDS latency is paid once per sweep and not once
// per read (hipcc otherwise parks every read right in front of its use).
constexpr int SW_BR = 4, SW_AHEAD = 1;
#ifndef GF_CHAIN_PRIO
#define GF_CHAIN_PRIO 1
#endif

// issue the reads of the first SW_AHEAD batches (done early, under the reduction of the
// previous row: the operands do not depend on it)
template <int ROWS>
__device__ __forceinline__ void sweep_preload(double (&ab)[SW_AHEAD + 1][SW_BR],
                                              double (&wb)[SW_AHEAD + 1][SW_BR],
                                              const double *xa, const double *xw) {
    constexpr int NB = ROWS / SW_BR;
#pragma unroll
    for (int k = 0; k < SW_AHEAD && k < NB; ++k) {
#pragma unroll
        for (int r = 0; r < SW_BR; ++r) { ab[k][r] = xa[k * SW_BR + r]; wb[k][r] = xw[k * SW_BR + r]; }
    }
}

//   RESET = false:  T_i += xw_i * q ;  acc += xa_i * T_i            (update + mat-vec)
//   RESET = true :  T_i  = (T_i + xw_i * q) * (xa_i * el)          (fold pending, decay)
template <int ROWS, bool RESET>
__device__ __forceinline__ double sweep_run(double (&T)[ROWS], double (&ab)[SW_AHEAD + 1][SW_BR],
                                            double (&wb)[SW_AHEAD + 1][SW_BR], const double *xa,
                                            const double *xw, const double q, const double el) {
    constexpr int BR = SW_BR, NB = ROWS / BR, AHEAD = SW_AHEAD;
    static_assert(ROWS % BR == 0, "ROWS must be a multiple of 4");
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        if (k + AHEAD < NB) {
#pragma unroll
            for (int r = 0; r < BR; ++r) {
                ab[(k + AHEAD) % (AHEAD + 1)][r] = xa[(k + AHEAD) * BR + r];
                wb[(k + AHEAD) % (AHEAD + 1)][r] = xw[(k + AHEAD) * BR + r];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const int c = k % (AHEAD + 1);
        if constexpr (RESET) {
#pragma unroll
            for (int r = 0; r < BR; ++r)
                T[k * BR + r] = fma(wb[c][r], q, T[k * BR + r]) * (ab[c][r] * el);
        } else {
            T[k * BR + 0] = fma(wb[c][0], q, T[k * BR + 0]);
            T[k * BR + 1] = fma(wb[c][1], q, T[k * BR + 1]);
            T[k * BR + 2] = fma(wb[c][2], q, T[k * BR + 2]);
            T[k * BR + 3] = fma(wb[c][3], q, T[k * BR + 3]);
            acc0 = fma(ab[c][0], T[k * BR + 0], acc0);
            acc1 = fma(ab[c][1], T[k * BR + 1], acc1);
            acc2 = fma(ab[c][2], T[k * BR + 2], acc2);
            acc3 = fma(ab[c][3], T[k * BR + 3], acc3);
            // pin the partial sums to this batch: LLVM otherwise sinks all the mat-vec FMAs
            // to the end of the sweep and keeps every row operand alive (register blow-up)
            asm volatile("" : "+v"(acc0), "+v"(acc1), "+v"(acc2), "+v"(acc3));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return (acc0 + acc2) + (acc1 + acc3);
}

// The row vectors (u~, v~, r, q) live one column per lane as in k_factor3 -- lane (g, c) owns column
// 2c + g -- while the state is tiled two columns x half the rows per lane.  Two exchanges between
// the half-waves connect the two layouts, each a pair of v_permlane32_swap (which swaps the upper
// half of its first operand with the lower half of its second):
//   own_column_sum(a, b): a, b = this half-wave's partial sums of columns 2c, 2c + 1; returns the
//     full sum of the lane's OWN column (lower half: a_L + a_U, upper half: b_L + b_U);
//   both_halves(x, lo, up): lo = x of lane c, up = x of lane c + 32, in both lanes.
__device__ __forceinline__ double own_column_sum(const double a, const double b) {
    const auto l = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
    return __hiloint2double(h[0], l[0]) + __hiloint2double(h[1], l[1]);
}
__device__ __forceinline__ void both_halves(const double x, double &lo, double &up) {
    const auto l = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(x), false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(x), false, false);
    lo = __hiloint2double(h[0], l[0]);
    up = __hiloint2double(h[1], l[1]);
}

constexpr int S7_AHEAD = 1;         // batches (one row pair = 8 FMAs + 2 reads) of LDS look-ahead

template <int ROWS>
__device__ __forceinline__ void sweep7_preload(double2 (&ub)[S7_AHEAD + 1], double2 (&wb)[S7_AHEAD + 1],
                                               const double2 *pu, const double2 *pw) {
#pragma unroll
    for (int k = 0; k < S7_AHEAD && k < ROWS / 4; ++k) { ub[k] = pu[2 * k]; wb[k] = pw[2 * k]; }
}

// T[2k + s][e] is row 4k + 2g + s, column 2c + e.  pu / pw point at this half-wave's first row pair.
//   RESET = false:  T += w q^T ;  acc += u^T T         (update + mat-vec, acc[e][s])
//   RESET = true :  T  = (T + w q^T) * (e_row el_col)  (fold pending, decay; pu = the row decays)
template <int ROWS, bool RESET>
__device__ __forceinline__ void sweep7_run(double (&T)[ROWS / 2][2], double2 (&ub)[S7_AHEAD + 1],
                                           double2 (&wb)[S7_AHEAD + 1], const double2 *pu,
                                           const double2 *pw, const double q0, const double q1,
                                           const double el0, const double el1, double &o0, double &o1) {
    constexpr int NK = ROWS / 4, AHEAD = S7_AHEAD;
    static_assert(ROWS % 4 == 0, "ROWS must be a multiple of 4");
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (k + AHEAD < NK) {
            ub[(k + AHEAD) % (AHEAD + 1)] = pu[2 * (k + AHEAD)];
            wb[(k + AHEAD) % (AHEAD + 1)] = pw[2 * (k + AHEAD)];
        }
        __builtin_amdgcn_sched_barrier(0);
        const double2 u = ub[k % (AHEAD + 1)], w = wb[k % (AHEAD + 1)];
        if constexpr (RESET) {
            T[2 * k][0] = fma(w.x, q0, T[2 * k][0]) * (u.x * el0);
            T[2 * k][1] = fma(w.x, q1, T[2 * k][1]) * (u.x * el1);
            T[2 * k + 1][0] = fma(w.y, q0, T[2 * k + 1][0]) * (u.y * el0);
            T[2 * k + 1][1] = fma(w.y, q1, T[2 * k + 1][1]) * (u.y * el1);
        } else {
            T[2 * k][0] = fma(w.x, q0, T[2 * k][0]);
            T[2 * k][1] = fma(w.x, q1, T[2 * k][1]);
            T[2 * k + 1][0] = fma(w.y, q0, T[2 * k + 1][0]);
            T[2 * k + 1][1] = fma(w.y, q1, T[2 * k + 1][1]);
            a00 = fma(u.x, T[2 * k][0], a00);
            a01 = fma(u.x, T[2 * k][1], a01);
            a10 = fma(u.y, T[2 * k + 1][0], a10);
            a11 = fma(u.y, T[2 * k + 1][1], a11);
            asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    o0 = a00 + a10;
    o1 = a01 + a11;
}

}  // namespace
