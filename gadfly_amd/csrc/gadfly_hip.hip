// gadfly_hip.hip -- the sweep unit: the hand-written fused sweeps for gfx950 (MI355X, CDNA4) with their part of the
// C-ABI of include/gadfly_hip.h, and the library's error state.  float64 throughout; wave = 64 lanes.
//
// What is replaced: the celerite2 C++ driver routines behind gadfly's GaussianProcess
// (the reference's gadfly/gp.py:202,:232, :327, :350, :370, :391).
// The arithmetic follows SURVEY.md Appendix A.4-A.8.
//
// Kernel inventory
//   k_factor3, k_factor7       the FUSED sweep (build + factor + forward solve, rows never written; RowGen): one column
//                              per lane, and the 2 x 32 lane tiling; SAMPLE instances draw
//   k_steady_*                 the rows around the steady switch: tail, finish, chunked finish, rank-one rows
//   k_phi7, k_phi, k_phiw      closed-loop transition sweeps of the time-parallel evaluation
//   k_factorw                  the fused sweep for wide kernels (several waves)
//   k_combine, k_tree_*        the chunk maps' combine, sequential and as a tree scan (cb_*: 64 x 64 LDS block algebra)
//   k_segment_transition, k_transpose64   the composed transitions of the linear sweeps' segments (kept here: see there)
//   k_reduce1, k_reduce2, k_finish   sum log d, sum z^2/d (deterministic fixed-shape tree), the log-likelihood
// Elsewhere: the sweeps on materialised rows (gadfly_stored.hip), the stored scaled factor's chunk-parallel linear
// sweeps (gadfly_linear.hip), the batched dense solve of the wide chunk maps (gadfly_dense.hip), the wave-level
// primitives (gf_wave.h), the sweeps' shared row helpers and SC_SPAN (gf_sweep.h), the entry points' argument checks
// and instance dispatch (gf_internal.h), and the power-spectrum and gap-filling kernels (gadfly_series.hip).
// gf_internal_error / gf_internal_check_launch / gf_internal_lds_opt_in are defined here for every unit of the library.
//
// No CUDA compatibility layer, no Triton, no CPU fallback.

#include <hip/hip_runtime.h>
#include <atomic>
#include <utility>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"

// sincos / exp with <= 1 ulp error for the argument ranges of the row generators (validated against
// long-double libm by oracle/fastmath_check.c); ~4x fewer instructions than the general OCML
// routines, which carry Payne-Hanek reduction for arbitrary arguments.
#define FM_INLINE __device__ __forceinline__
#include "fastmath.h"
#include "gf_wave.h"
#include "gf_sweep.h"

// fm_exp with its coefficients formed where they are used.  Written as literals, hipcc hoists the fourteen FP64
// coefficients out of any loop that contains a call -- also when the call sits on a reset row, one row in 16 to
// 64 -- and holds them in 28 VGPRs for the whole sweep (k_phi7<60> then spills).  Each coefficient's two words
// XOR an opaque zero taken once per call, so it is not loop-invariant; same bits, same result.  For the sweeps
// whose only transcendental is this one (the transition sweeps); the factor sweeps are faster with the hoisted
// literals (measured: DESIGN.md 2.1e).
template <unsigned long long BITS>
__device__ __forceinline__ double fm_local_constant(const int z) {
    return __hiloint2double((int)(unsigned)(BITS >> 32) ^ z, (int)(unsigned)(BITS & 0xffffffffull) ^ z);
}
#define GF_K(x) fm_local_constant<__builtin_bit_cast(unsigned long long, (double)(x))>(fm_z)
__device__ __forceinline__ double fm_exp_local(const double x) {
    int fm_z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(fm_z));
    if (x < -745.0) return 0.0;
    const double k = rint(x * GF_K(1.44269504088896338700e+00));
    const double r = fma(-k, GF_K(1.90821492927058770002e-10), fma(-k, GF_K(6.93147180369123816490e-01), x));
    double p = GF_K(1.0 / 6227020800.0);
    p = fma(p, r, GF_K(1.0 / 479001600.0));
    p = fma(p, r, GF_K(1.0 / 39916800.0));
    p = fma(p, r, GF_K(1.0 / 3628800.0));
    p = fma(p, r, GF_K(1.0 / 362880.0));
    p = fma(p, r, GF_K(1.0 / 40320.0));
    p = fma(p, r, GF_K(1.0 / 5040.0));
    p = fma(p, r, GF_K(1.0 / 720.0));
    p = fma(p, r, GF_K(1.0 / 120.0));
    p = fma(p, r, GF_K(1.0 / 24.0));
    p = fma(p, r, GF_K(1.0 / 6.0));
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)k);
}
#undef GF_K

namespace {

thread_local char g_err[512] = "";

}  // namespace

// what every translation unit of the library reports through, this one included (gf_internal.h)
int gf_internal_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int gf_internal_check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return -2;
    }
    return 0;
}

namespace {

// ------------------------------------------------------------------------------------
// k_factor3: the fully fused log-likelihood sweep (W < 64).  Same recurrence as k_factor2, but
// the generator rows are never materialised: every row's u~, v~ are produced in registers
// from t_n (theta = d t_n as one rounded multiply, fm_sincos, running products for rho), so an
// evaluation reads only t, y, diag (24 B/row) and writes d, z (16 B/row).  Each lane computes
// sin AND cos of its own phase (lanes 2k, 2k+1 share theta_k), which removes any cross-lane
// exchange:  u~ = (uA * own + uB * other) * rho,  v~ = own / rho  with
//   even column: own = cos, uA = a, uB = +b ;  odd column: own = sin, uA = a, uB = -b ;
//   real column: d = 0 (cos = 1), uA = a_r, uB = 0.
// Between reset rows (anchors: exact fm_sincos, rho = 1) the rho-scaled phasor advances by a cached
// one-cadence rotation with a second-order correction for cadence jitter (RowGen::next).
// Valid while |d t| < 1e12 (fm_sincos's range, FM_SINCOS_RANGE): the caller checks and otherwise
// uses the k_build2 + k_factor2 pair.
//
// Chunk mode (time-parallel evaluation of one series, see k_phi / k_combine): the grid is
// (problem, chunk); block b handles rows [c L, (c+1) L) of problem b / nch with its own state
// slot b, so the same kernel serves the nominal pass (zero start state, r~ rows stored for
// k_phi) and the final pass (true start states from k_combine).
// ------------------------------------------------------------------------------------
struct RowGen {
    // per-lane column constants: u~ = (k1 cu + k2 su), v~ = own / rho^2 with (cu, su) =
    // rho (cos, sin)(d t); lanes 2k, 2k+1 carry the same (cu, su)
    double cj, dj, k1, k2;
    // own-component selectors of v~ as exact 0/1 factors (pad lanes: both 0): two FMAs-worth of
    // VALU work instead of two 64-bit selects, and no lane masks held in SGPRs
    double sel_c, sel_s;
    // wave-uniform thresholds of the row tests, divided out once: a row is a reset of its own when
    // dt > gthr (= gap / cmax), its spacing counts as the cached one when |ddt| < jthr (= 2e-6 / wmax)
    double gthr, jthr, jthr1;       // jthr1 = 1.4e-9 / wmax: below it the step's correction is first order
    int block, sub_mask;            // scaling block length; sub-anchor period - 1
    // far from t = 0 the rotation steps follow celerite2's ROUNDED phases theta_n = fl(d t_n) (see step())
    bool qmode;
    // running state: rho-scaled phasor, 1 / rho^2, cached one-cadence multipliers
    double cu, su, irho2, Er, Ei, G2, dt_ref, dt_last, tref, t_m1;

    __device__ __forceinline__ void init(int lane, int b, int Jr, int Jc, int block_sub, double gap_,
                                         const double *ar_, const double *cr_, const double *ac_,
                                         const double *bc_, const double *cc_, const double *dc_,
                                         const double *cmax_, const double *tg, int64_t n_first) {
        const int W = Jr + 2 * Jc;
        const bool colok = lane < W;
        bool is_sin = false;
        cj = 0.0; dj = 0.0; k1 = 0.0; k2 = 0.0;
        if (lane < Jr) {
            cj = cr_[(size_t)b * Jr + lane];
            k1 = ar_[(size_t)b * Jr + lane];
        } else if (colok) {
            const int k = (lane - Jr) >> 1;
            const size_t ck = (size_t)b * Jc + k;
            is_sin = ((lane - Jr) & 1) != 0;
            cj = cc_[ck];
            dj = dc_[ck];
            // cos column: a cos + b sin ;  sin column: a sin - b cos
            k1 = is_sin ? -bc_[ck] : ac_[ck];
            k2 = is_sin ? ac_[ck] : bc_[ck];
        }
        sel_c = (colok && !is_sin) ? 1.0 : 0.0;
        sel_s = (colok && is_sin) ? 1.0 : 0.0;
        const double cmax = cmax_[b];
        const double wmax = read_lane(wave_max(fmax(cj, fabs(dj))), 0);
        gthr = read_lane(gap_ / cmax, 0);                       // uniform: live in SGPRs
        jthr = read_lane(2e-6 / wmax, 0);
        // phases beyond 4e6 rad at the first row (a time axis that does not start near zero: 5e9 rad on a JD-based
        // one): their rounding, half an ulp of theta, is no longer negligible against the accuracy target
        qmode = __builtin_amdgcn_readfirstlane((int)(wmax * fabs(tg[0]) > 4.0e6)) != 0;
        jthr1 = qmode ? 0.0 : read_lane(1.4e-9 / wmax, 0);      // (the first-order step assumes |x| < 1.4e-9)
        block = block_sub & 0xff;           // (block <= 64) | (sub-anchor period << 8)
        sub_mask = ((block_sub >> 8) & 0xff) - 1;  // (bit 30: zero start, see the sweeps)
        cu = 1.0; su = 0.0; irho2 = 1.0; Er = 1.0; Ei = 0.0; G2 = 1.0; dt_ref = -1.0; dt_last = -2.0;
        // reference time of the block that precedes the first row (for its decay); tg points
        // at the first row, earlier rows are at negative indices
        tref = tg[0];
        if (n_first > 0) {
            int64_t g = -1;
            while (!(((n_first + g) & (block - 1)) == 0 || (tg[g] - tg[g - 1]) > gthr)) --g;
            tref = tg[g];
        }
        t_m1 = (n_first > 0) ? tg[-1] : tg[0];
    }

    // generate global row g at time tn: u~, v~, reset flag and (for reset rows) the decay span.
    // Reset rows (every `block` <= 64 rows, and after gaps) are anchors: rho = 1 and the phase is
    // theta = d t_n as ONE rounded multiply through fm_sincos.  Between anchors the phasor
    // advances by the cached one-cadence multiplier exp((-c + i d) dt_ref), corrected to second
    // order for the deviation of this row's spacing from dt_ref (rounding-level jitter of a
    // regular cadence: |(c, d) ddt| < 2e-6 => truncation < 2e-18 per row); any other spacing
    // recomputes the phasor exactly (and re-caches the multiplier once the new spacing repeats).
    // Per-row rounding accumulates over at most period - 1 rows (sub-anchors).
    // The pieces of next(): kind of the row at time tn (0 = plain rotation step, 1 = the cached
    // multipliers must be refreshed first, 2 = reset row / anchor); wave-uniform.
    __device__ __forceinline__ int peek(const double tn, const int64_t g, double &dt, double &ddt) const {
        dt = tn - t_m1;
        ddt = dt - dt_ref;
        if (((g & (block - 1)) == 0) || (dt > gthr)) return 2;
        if ((g & sub_mask) == 0) return 3;                      // exact phasor again, same scaling
        return (fabs(ddt) < jthr) ? 0 : 1;
    }
    // Sub-anchor: every `period` rows (gf_set_generator_period: 1, 2, 4, ... 64) the phasor is
    // recomputed exactly (theta = d t_n as one rounded multiply, rho = exp(-c (t_n - t_ref))), so
    // the rotation's rounding -- coherent within a segment, the cached multiplier carries one
    // fixed 0.5-ulp error -- accumulates over at most period - 1 steps.  Measured against the
    // 80-bit recurrence (tests/test_gpu_random.py seeds, condition 4e5): period 1 = exact
    // generation every row 2e-10 (the float64 class), 4: 2e-9, 16: 1e-8, 64: several 1e-8.
    __device__ __forceinline__ void subanchor(const double tn) {
        t_m1 = tn;
        double si, co;
        fm_sincos(dj * tn, &si, &co);
        const double rho = fm_exp(-cj * (tn - tref));
        cu = rho * co;
        su = rho * si;
        irho2 = fast_rcp(rho * rho);
    }
    __device__ __forceinline__ void anchor(const double tn, const int64_t g, double &de) {
        de = (g > 0) ? (tn - tref) : 0.0;
        tref = tn;
        t_m1 = tn;
        fm_sincos(dj * tn, &su, &cu);               // real columns: d = 0 -> (1, 0)
        irho2 = 1.0;
    }
    __device__ __forceinline__ void refresh(const double dt) {
        double si, co;
        fm_sincos(dj * dt, &si, &co);
        const double pr = fm_exp(-cj * dt);
        Er = pr * co;
        Ei = pr * si;
        G2 = fast_rcp(pr * pr);
        dt_ref = read_lane(dt, 0);                  // uniform: keep it in SGPRs
    }
    __device__ __forceinline__ void step(const double tn, const double ddt) {
        const double tp = t_m1;
        t_m1 = tn;
        const double xr = -cj * ddt;
        double xi;
        if (qmode) {
            // celerite2 takes cos / sin of theta_n = fl(d t_n): at 5e9 rad that is the true phase +- 5e-7 rad,
            // row by row.  The step must land on THAT phase: the phasor stands at theta_{n-1}, the cached
            // multiplier turns it by fl(d dt_ref) (what refresh() took the sincos of), so the correction is the
            // difference of the two ROUNDED products -- exact (neighbouring values) -- minus that angle.  (The
            // decay needs nothing of the kind: celerite2's exp(-c (t_n - t_{n-1})) sees the time difference too.)
#pragma clang fp contract(off)
            const double th_n = dj * tn, th_p = dj * tp;        // two rounded products, as celerite2 forms them
            xi = (th_n - th_p) - dj * dt_ref;
        } else {
            xi = dj * ddt;
        }
        double Mr, Mi, g2;
        if (fabs(ddt) < jthr1) {
            // |x| < 1.4e-9 (the rounding jitter of a regular cadence): exp(x) = 1 + x to 1e-18
            Mr = fma(-Ei, xi, fma(Er, xr, Er));                     // E (1 + x)
            Mi = fma(Ei, xr, fma(Er, xi, Ei));
            g2 = fma(G2 * -2.0, xr, G2);                            // G2 (1 - 2 xr)
        } else {
            const double qr = 1.0 + fma(0.5, fma(xr, xr, -xi * xi), xr);    // exp(xr + i xi), 2nd order
            const double qi = fma(xr, xi, xi);
            Mr = fma(Er, qr, -Ei * qi);
            Mi = fma(Er, qi, Ei * qr);
            const double x2 = -2.0 * xr;
            g2 = G2 * (1.0 + fma(0.5 * x2, x2, x2));
        }
        const double c2 = fma(cu, Mr, -su * Mi);
        su = fma(cu, Mi, su * Mr);
        cu = c2;
        irho2 *= g2;
    }
    __device__ __forceinline__ void emit(double &ut, double &vt) const {
        ut = fma(k1, cu, k2 * su);                  // pad lanes: k1 = k2 = 0
        vt = fma(sel_s, su, sel_c * cu) * irho2;
    }
    __device__ __forceinline__ void next(const double tn, const int64_t g, double &ut, double &vt,
                                         bool &rst, double &de) {
        advance(tn, g, rst, de);
        emit(ut, vt);
    }
    __device__ __forceinline__ void advance(const double tn, const int64_t g, bool &rst, double &de) {
        // two wave-uniform tests on the common path (reset? plain step?); the rare cases are told
        // apart inside the rare branch
        const double dt = tn - t_m1;
        double ddt = dt - dt_ref;
        rst = ((g & (block - 1)) == 0) || (dt > gthr);
        de = -1.0;
        if (__builtin_expect(rst, 0)) {
            anchor(tn, g, de);
        } else if (__builtin_expect(((g & sub_mask) != 0) && (fabs(ddt) < jthr), 1)) {
            step(tn, ddt);
        } else {
            // sub-anchor row, or a spacing that differs from the cached one: exact phasor (an
            // irregular cadence thus never accumulates rotation steps: same cost as refreshing
            // the multiplier, exact accuracy); the cached multipliers move to a new spacing
            // only once it repeats (a lasting change of cadence, not a single odd row)
            subanchor(tn);
            if (!(fabs(ddt) < jthr)) {
                if (fabs(dt - dt_last) < jthr) refresh(dt);
                dt_last = read_lane(dt, 0);
            }
        }
    }

    // Park / restore the ten per-lane doubles in LDS (buf[10][64]): a kernel that needs its
    // registers while no row is being generated spills them here instead of to scratch.
    __device__ __forceinline__ void park(double *buf, int lane) const {
        buf[0 * 64 + lane] = cj; buf[1 * 64 + lane] = dj; buf[2 * 64 + lane] = k1; buf[3 * 64 + lane] = k2;
        buf[4 * 64 + lane] = cu; buf[5 * 64 + lane] = su; buf[6 * 64 + lane] = irho2;
        buf[7 * 64 + lane] = Er; buf[8 * 64 + lane] = Ei; buf[9 * 64 + lane] = G2;
    }
    __device__ __forceinline__ void park_state(double *buf, int lane) const {       // what next() changes
        buf[4 * 64 + lane] = cu; buf[5 * 64 + lane] = su; buf[6 * 64 + lane] = irho2;
        buf[7 * 64 + lane] = Er; buf[8 * 64 + lane] = Ei; buf[9 * 64 + lane] = G2;
    }
    __device__ __forceinline__ void unpark(const double *buf, int lane) {
        cj = buf[0 * 64 + lane]; dj = buf[1 * 64 + lane]; k1 = buf[2 * 64 + lane]; k2 = buf[3 * 64 + lane];
        cu = buf[4 * 64 + lane]; su = buf[5 * 64 + lane]; irho2 = buf[6 * 64 + lane];
        Er = buf[7 * 64 + lane]; Ei = buf[8 * 64 + lane]; G2 = buf[9 * 64 + lane];
    }
};

// SAMPLE = true: the sampling sweep (gf_sample_fused).  y_ holds the standard normals eps and the pad column
// carries the DRAW instead of the solve:  x_n = sqrt(d_n) eps_n,  F~ += r x_n / d_n,  out_n = x_n + u~ . F~
// (y = L D^1/2 eps, celerite2's matmul_lower with V := W after factor) -- the solve's recurrence with the sign
// flipped and the input carried instead of the output.  z_ is then the draw, indexed by the GLOBAL row with
// y's batch stride.  Reset rows, decays, block scaling and the row generator are the log-likelihood's.
template <int ROWS, bool SAMPLE = false>
__global__ void __launch_bounds__(64, 2)
k_factor3(const int64_t N, const int64_t n_first, const int64_t chunk_len, const int nch,
          const int ch0, const int nsel, const int Jr, const int Jc, const int block_sub, const double gap,
          const double *__restrict__ ar_, const double *__restrict__ cr_,
          const double *__restrict__ ac_, const double *__restrict__ bc_,
          const double *__restrict__ cc_, const double *__restrict__ dc_,
          const double *__restrict__ diag_add_, const double *__restrict__ cmax_,
          const double *__restrict__ t_, const int64_t t_bs,
          const double *__restrict__ diag_, const int64_t diag_bs,
          const double *__restrict__ y_, const int64_t y_bs,
          double *__restrict__ d_, double *__restrict__ z_, double *__restrict__ r_out,
          double *__restrict__ Ut_out, double *__restrict__ Wt_out, double *__restrict__ de_out,
          double *__restrict__ S_state, double *__restrict__ F_state,
          int32_t *__restrict__ info) {
    const int lane = threadIdx.x;
    const int sel = blockIdx.x;                     // chunks ch0 .. ch0 + nsel - 1 of every problem
    const int pr = sel / nsel, ch = ch0 + (sel - pr * nsel);
    const int b = pr * nch + ch;                    // state slot = problem * nch + chunk
    if (info[b] != 0) return;
    const int64_t c0 = (int64_t)ch * chunk_len;     // first row of the chunk within this call
    const int64_t rows = (N - c0 < chunk_len) ? (N - c0) : chunk_len;
    const int64_t g0 = n_first + c0;                // global index of the chunk's first row
    const size_t pb = (size_t)pr * N + c0;
    const double *__restrict__ tg = t_ + (size_t)pr * t_bs + g0;
    const double *__restrict__ yg = y_ + (size_t)pr * y_bs + g0;
    // per-row diagonal: always read (through an address that is valid either way, so the loads stay
    // unconditional scalar loads) and dropped by a scalar select when there is none
    const bool has_g = diag_ != nullptr;
    const double *__restrict__ gg = has_g ? diag_ + (size_t)pr * diag_bs + g0 : yg;
    double *__restrict__ dg = d_ + pb;
    double *__restrict__ zg = SAMPLE ? z_ + (size_t)pr * y_bs + g0 : z_ + pb;
    // chunk-mode row stores: loop-invariant per-lane pointers, indexed with opaque_uniform(row)
    double *__restrict__ rg = r_out ? r_out + pb * 64 + lane : nullptr;
    double *__restrict__ ug = Ut_out ? Ut_out + pb * 64 + lane : nullptr;   // stored factor:
    double *__restrict__ wg = Wt_out ? Wt_out + pb * 64 + lane : nullptr;   // u~, w~ = r/d rows
    double *__restrict__ eg = de_out ? de_out + pb : nullptr;               // reset spans (-1: none)
    double *__restrict__ Sg = S_state + (size_t)b * (64 * 64) + (size_t)lane * 64;
    double *__restrict__ Fg = F_state + (size_t)b * 64;
    const double diag_add = diag_add_[pr];

    RowGen G;
    G.init(lane, pr, Jr, Jc, block_sub, gap, ar_, cr_, ac_, bc_, cc_, dc_, cmax_, tg, g0);
    const double cj = G.cj;

    __shared__ double s_w[64];      // r_{n-1}  (pending rank-1 update, row form)
    __shared__ double s_u[64];      // u~_n
    __shared__ double s_e[64];      // block decay E at reset rows
    const bool fl = lane == 63;     // pad lane carrying the forward solve (W < 64)
    // exact 0/1 factors for "every lane but 63" / "lane 63 only": one multiply (FMA) where a
    // 64-bit select costs two instructions on the row's serial chain
    const double not63 = fl ? 0.0 : 1.0, is63 = fl ? 1.0 : 0.0;

    double T[ROWS];
    const bool zero_start = (block_sub >> 30) & 1;  // nominal pass: the state slots are outputs only
#pragma unroll
    for (int i = 0; i < ROWS; ++i) T[i] = zero_start ? 0.0 : (fl ? Fg[i] : Sg[i]);
    double q = 0.0;
    int32_t fail = 0;

    // rows are generated one row ahead of their sweep; t is prefetched two further rows ahead, y and
    // diag one (the caller pads t, y, diag by three elements; a row takes far longer than a scalar load)
    double t_n1 = tg[1], t_n2 = tg[2];
    double y_n = yg[0], y_n1 = yg[1];
    double g_n = gg[0], g_n1 = gg[1];
    double ut, vt, de;
    bool rst;
    G.next(tg[0], g0, ut, vt, rst, de);

    double ab[SW_AHEAD + 1][SW_BR], wb[SW_AHEAD + 1][SW_BR];
    s_w[lane] = 0.0;
    s_u[lane] = ut;
    wave_lds_fence();
    sweep_preload<ROWS>(ab, wb, s_u, s_w);

    for (int64_t n = 0; n < rows; ++n) {
        const double a_n = (has_g ? g_n : 0.0) + diag_add, yy = y_n;
        const double ut_c = ut, vt_c = vt;
        if (eg && lane == 0) eg[n] = rst ? de : -1.0;
        if (rst) {                          // wave-uniform: fold the pending update, then decay
            const double el = fm_exp(-cj * de);     // pad lanes: cj = 0 -> 1
            s_e[lane] = el;
            wave_lds_fence();
            // the operand ring is reused (its preloaded rows are simply fetched again below):
            // keeping a second ring alive across this branch costs 48 VGPRs on every row
            sweep_preload<ROWS>(ab, wb, s_e, s_w);
            (void)sweep_run<ROWS, true>(T, ab, wb, s_e, s_w, q, el);
            sweep_preload<ROWS>(ab, wb, s_u, s_w);
            q = 0.0;
        }
        __builtin_amdgcn_s_setprio(0);
        const double tmp = sweep_run<ROWS, false>(T, ab, wb, s_u, s_w, q, 0.0);
        // the serial part of the row (reduction, reciprocal, next row's operands) wins the issue
        // arbitration against the partner wave's FMA stream: its instructions are dependent and
        // each lost slot lengthens the chain, the partner's are not
        __builtin_amdgcn_s_setprio(GF_CHAIN_PRIO);
        const double r = (vt_c - tmp) * not63;
        // next row's operands: generated here, where the operand ring is dead (register budget)
        G.next(t_n1, g0 + n + 1, ut, vt, rst, de);
        t_n1 = t_n2; y_n = y_n1; g_n = g_n1;
        t_n2 = tg[n + 3];
        y_n1 = yg[n + 2];
        g_n1 = gg[n + 2];
        wave_lds_fence();
        s_w[lane] = r;
        s_u[lane] = ut;
        wave_lds_fence();
        sweep_preload<ROWS>(ab, wb, s_u, s_w);
        const double s1 = wave_sum(ut_c * tmp);     // u~ = 0 in lane 63
        const double s2 = read_lane(tmp, 63);       // u~ . F~
        const double dn = a_n - s1;
        const double zn = SAMPLE ? __dsqrt_rn(dn) * yy : yy - s2;      // (the draw: x_n rides where z_n does)
        if (!(dn > 0.0)) {
            const int64_t gf = g0 + n + 1;
            fail = (int32_t)(gf > 0x7fffffff ? 0x7fffffff : gf);
            break;
        }
        const double inv = fast_rcp(dn);
        q = fma(zn, is63, r) * inv;                 // lane 63: z / d (r is 0 there)
        const size_t ro = opaque_uniform((size_t)n * 64);
        if (lane < ROWS || wg) {                    // (nominal passes store the first ROWS columns only: k_factor7)
            if (rg) rg[ro] = r;                     // r~ rows for k_phi (chunk mode)
            if (ug) ug[ro] = ut_c;
            if (wg) wg[ro] = fl ? 0.0 : q;
        }
        if (lane == 0) { dg[n] = dn; zg[n] = SAMPLE ? zn + s2 : zn; }
    }
    if (fail) {
        if (lane == 0) info[b] = fail;
        if (zero_start) {                           // an output-only slot is never left stale: the combines read
            for (int i = 0; i < 64; ++i) { if (fl) Fg[i] = 0.0; else Sg[i] = 0.0; }   // its padding as zeros
            if (fl) for (int i = 0; i < 64; ++i) Sg[i] = 0.0;
        }
        return;
    }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const double v = fma(s_w[i], q, T[i]);
        if (fl) Fg[i] = v; else Sg[i] = v;
    }
    if (zero_start) {                               // the slot is an output only: its padding rows too,
        for (int i = ROWS; i < 64; ++i) { if (fl) Fg[i] = 0.0; else Sg[i] = 0.0; }
        if (fl) for (int i = 0; i < 64; ++i) Sg[i] = 0.0;          // and S's own column 63 (lane 63 carries F~)
    }
}

// ------------------------------------------------------------------------------------
// k_factor7: the fused sweep with a 2 x 32 lane tiling (half the LDS operand traffic).
//
// k_factor3 gives every lane one column of T and all ROWS rows, so each FMA needs a wave-uniform row
// operand that reaches the lanes as an LDS broadcast: 1 KiB through the LDS array for 16 useful
// bytes, 60 ds_read_b128 per row.  With two waves on each of the four SIMDs that is 81 % of the
// CU's LDS-array cycles (SQ_LDS_IDX_ACTIVE) -- the resource the kernel actually saturates, ahead of
// vector issue (69 %).  Here lane = (g, c) = (lane >> 5, lane & 31) holds the TWO columns 2c, 2c+1
// (the cos and sin columns of complex term c: one phasor per lane instead of the same phasor in two
// lanes) of HALF the rows (pairs of rows 4k + 2g, 4k + 2g + 1): a ds_read_b128 then delivers a
// different operand pair to each half-wave and feeds 8 FMAs, 30 reads per row instead of 60.  The
// row vectors stay one column per lane (lane (g, c) owns column 2c + g, the generator is
// k_factor3's); two v_permlane32_swap exchanges per row connect the layouts (7 vector
// instructions: the mat-vec's partial sums, then the multipliers q).  Same arguments,
// state layout in memory and results as k_factor3; needs Jr = 0 (every gadfly kernel with
// Q > 1/2) and Jc <= 31 (block 31 carries the pad column 62 and the forward solve in column 63).
// ------------------------------------------------------------------------------------
// One LDS-DMA instruction (global_load_lds_dwordx4): lane l copies 16 bytes from ITS OWN global address to
// LDS byte `lds_byte` + 16 l -- no VGPR destination, so a deep prefetch costs LDS instead of registers.
// hipcc does not count it: completion is waited for with vm_wait (vector-memory operations retire in
// issue order).  `after` is a value that must exist before the copy may issue (keeps the copy behind
// the reads of the ring slot it overwrites).
__device__ __forceinline__ void glds16(const void *gsrc, const unsigned lds_byte, const int after) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_byte), "v"(after) : "memory");
}
template <int CNT>
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" : : "n"(CNT) : "memory"); }

// ROWSTORE = false: no row is stored (r_out, Ut_out, Wt_out, de_out all null: the streamed log-likelihood
// and the plain final pass) -- their tests, pointer arithmetic and exec-mask switches leave the row loop
// SAMPLE = true: the sampling sweep, column 63 carries the draw (see k_factor3)
//
// STEADY = true (gf_loglike_steady; ROWSTORE = SAMPLE = false): on a regular cadence with a constant diagonal the
// recurrence is a time-invariant Riccati iteration, which converges geometrically to a fixed point in the frame
// that rotates with the terms' phasors: the pivot d and the derotated gains G_k = (w_2k + i w_2k+1) e^{-i d_k t}
// (w = r / d) become constants, and the W x W state carries nothing new.  At the rows = 0 mod ST_GRID = 64 (block
// resets whatever the scaling block, a power of two <= 64: rho = 1, exact phasor) from global row arm_from on, the
// wave compares d and its lanes' gain components with the values of ST_LAG such anchors before -- 1024 ROWS, so
// that the rule means the same at every block -- (a ring in the per-problem steady buffer); once both have moved
// by less than ST_THR -- the gains relative to the largest gain -- at ST_COUNT consecutive anchors it freezes them,
// leaves the derotated forward-solve state s_k = e^{-i d_k t} (F_2k + i F_2k+1) (this row's update folded), the gains,
// the pivot and the cadence (over the last 1024 rows) in the buffer and ends.  The rows after belong to the block
// filter below: k_steady_tail, which gf_loglike_steady launches behind this kernel on every tile, or k_steady_finish,
// once per evaluation behind the last tile of gf_steady_sweep; on later tiles this kernel returns at once for such
// a problem.  A row the tail cannot take -- a gap reset, a spacing off the frozen cadence -- raises the
// buffer's violation flag: the caller repeats the evaluation without the mode.
constexpr int ST_SW = 0;            // first tail row (global) ; 0 = full mode
constexpr int ST_D = 1;             // frozen pivot
constexpr int ST_VIOL = 2;          // != 0: the tail met a row it cannot take
constexpr int ST_CNT = 3;           // consecutive converged anchors so far
constexpr int ST_FILL = 4;          // anchors in the ring
constexpr int ST_HOK = 5;           // != 0: the tail's impulse response is in ST_H
constexpr int ST_DT = 6;            // frozen cadence: (t_sw - t_{sw - 1024}) / 1024
constexpr int ST_GR = 8, ST_GI = 40;        // [32] frozen derotated gain G_k by term
constexpr int ST_SR = 72, ST_SI = 104;      // [32] the tail's state s_k by term, as of the last row done
constexpr int ST_RING = 136;        // [ST_LAG][64] gain component per lane (lane 63: the pivot)
constexpr int ST_H = ST_RING;       // [64] the tail's impulse response (the ring is dead after the switch)
constexpr int ST_DLAG = 1024;       // rows behind the switch row that the cadence is taken over
constexpr int ST_GRID = 64;         // rows between the anchors the rule looks at
constexpr int ST_LAG = 16, ST_COUNT = 4;
constexpr double ST_THR = 1e-10;
constexpr int ST_SIZE = ST_RING + ST_LAG * 64;

// The log-likelihood reductions' shape (k_reduce1 / k_reduce2, below): G groups of RED_BLOCK rows per problem.
constexpr int RED_NACC = 3;         // the reductions' accumulators per problem: sum log d, sum z^2/d, min d
constexpr int RED_BLOCK = 256;
constexpr int RED_MAXG = 512;

__host__ __device__ inline int red_groups(int64_t N) {
    int64_t g = (N + 4095) / 4096;
    if (g < 1) g = 1;
    if (g > RED_MAXG) g = RED_MAXG;
    return (int)g;
}

// Rows of a tile (first global row n_first) that the steady mode's sweep instance stored for problem b: those in
// front of the problem's switch row, all N of a problem that has not switched (the bounded reductions).
__device__ inline int64_t steady_rows_stored(const double *steady, int b, int64_t N, int64_t n_first) {
    const double swd = steady[(size_t)b * ST_SIZE + ST_SW];
    if (!(swd > 0.0)) return N;
    const int64_t r = (int64_t)swd - n_first;
    return r < 0 ? 0 : (r < N ? r : N);
}

// One row's terms of the sums: the same expressions wherever a tile is summed (k_reduce1 and steady_tile_sums must
// give the same bits, so neither may be contracted differently from the other).
__device__ __forceinline__ void red_row(const double dn, double &s1, double &mn) {
    s1 += log(dn);
    mn = fmin(mn, dn);
}
__device__ __forceinline__ void red_row_z(const double dn, const double zn, double &s2) { s2 += zn * zn / dn; }

// gf_reduce_tile_steady's additions for ONE problem by ONE wave (the steady sweep's own wave behind its rows:
// gf_steady_sweep_reduced): rows [0, lim) of the tile's d and z.  The same operations in the same order as
// k_reduce1<true> + k_reduce2<true>, so the same bits: per group g of RED_BLOCK rows the block's four waves one after
// the other (lane l of wave w takes rows g RED_BLOCK + 64 w + l + k G RED_BLOCK), thread 0's sum over the four from
// 0.0 / inf, then k_reduce2's lane g & 63 over its groups in order, the tree over the lanes and lane 0's addition to
// acc.  (Exact zeros from the lanes and waves without a row change no bit, there as here.)
__device__ __forceinline__ void steady_tile_sums(const double *dp, const double *zp, const int64_t N, const int64_t lim,
                                                 double *acc, const int init, const int lane) {
    if (lim == 0 && !init) return;
    const int G = red_groups(N);
    const int64_t gl = (lim + RED_BLOCK - 1) / RED_BLOCK;
    const int Gn = gl < G ? (int)gl : G;
    double a1 = 0.0, a2 = 0.0, am = INFINITY;
#pragma unroll 1
    for (int g = 0; g < Gn; ++g) {
        double t1 = 0.0, t2 = 0.0, t3 = INFINITY;
#pragma unroll 1
        for (int w = 0; w < RED_BLOCK / 64; ++w) {
            double s1 = 0.0, s2 = 0.0, mn = INFINITY;
#pragma unroll 1
            for (int64_t n = (int64_t)g * RED_BLOCK + 64 * w + lane; n < lim; n += (int64_t)G * RED_BLOCK) {
                const double dn = dp[n];
                red_row(dn, s1, mn);
                red_row_z(dn, zp[n], s2);
            }
            wave_sum2(s1, s2);
            mn = -wave_max(-mn);
            t1 += s1;
            t2 += s2;
            t3 = fmin(t3, mn);
        }
        if (lane == (g & 63)) {
            a1 += t1;
            a2 += t2;
            am = fmin(am, t3);
        }
    }
    wave_sum2(a1, a2);
    am = -wave_max(-am);
    if (lane == 0) {
        if (!init) { a1 += acc[0]; a2 += acc[1]; am = fmin(am, acc[2]); }
        acc[0] = a1; acc[1] = a2; acc[2] = am;
    }
}

template <int ROWS, bool ROWSTORE, bool SAMPLE = false, bool STEADY = false>
__global__ void __launch_bounds__(64, 2)
k_factor7(const int64_t N, const int64_t n_first, const int64_t chunk_len, const int nch,
          const int ch0, const int nsel, const int Jr, const int Jc, const int block_sub, const double gap,
          const double *__restrict__ ar_, const double *__restrict__ cr_,
          const double *__restrict__ ac_, const double *__restrict__ bc_,
          const double *__restrict__ cc_, const double *__restrict__ dc_,
          const double *__restrict__ diag_add_, const double *__restrict__ cmax_,
          const double *__restrict__ t_, const int64_t t_bs,
          const double *__restrict__ diag_, const int64_t diag_bs,
          const double *__restrict__ y_, const int64_t y_bs,
          double *__restrict__ d_, double *__restrict__ z_, double *__restrict__ r_out,
          double *__restrict__ Ut_out, double *__restrict__ Wt_out, double *__restrict__ de_out,
          double *__restrict__ S_state, double *__restrict__ F_state,
          int32_t *__restrict__ info, double *__restrict__ steady_, const int64_t arm_from,
          double *acc_, const int acc_init) {
    static_assert(!STEADY || (!ROWSTORE && !SAMPLE), "steady mode: the streamed log-likelihood only");
    const int lane = threadIdx.x;
    const int g = lane >> 5, c = lane & 31;         // row group, column block (columns 2c, 2c + 1)
    const int sel = blockIdx.x;                     // chunks ch0 .. ch0 + nsel - 1 of every problem
    const int pr = sel / nsel, ch = ch0 + (sel - pr * nsel);
    const int b = pr * nch + ch;                    // state slot = problem * nch + chunk
    // steady mode with acc_ (gf_steady_sweep_reduced; wave-uniform): the wave adds this tile's stored rows to acc[pr]
    // itself, at whichever exit it leaves by, as gf_reduce_tile_steady would behind it -- tile_lim rows, what
    // steady_rows_stored gives once the kernel has ended (label tile_sums, at the kernel's end; acc_ null: every
    // exit is the plain return it was, and the other instances hold nothing of this)
    int64_t tile_lim = 0;
#define STEADY_EXIT(lim) do { if constexpr (STEADY) { if (acc_) { tile_lim = (lim); goto tile_sums; } } return; } while (0)
  {
    if (info[b] != 0) STEADY_EXIT(steady_rows_stored(steady_, pr, N, n_first));    // (stale rows, as the reduction takes them)
    // steady mode: this problem's buffer; a problem that has switched is k_steady_tail's from its switch row on
    double *__restrict__ hdr = STEADY ? steady_ + (size_t)pr * ST_SIZE : nullptr;
    if constexpr (STEADY) { if (hdr[ST_SW] > 0.0) STEADY_EXIT(steady_rows_stored(steady_, pr, N, n_first)); }
    const int64_t c0 = (int64_t)ch * chunk_len;
    const int64_t rows = (N - c0 < chunk_len) ? (N - c0) : chunk_len;
    const int64_t g0 = n_first + c0;
    const size_t pb = (size_t)pr * N + c0;
    const double *__restrict__ tg = t_ + (size_t)pr * t_bs + g0;
    const double *__restrict__ yg = y_ + (size_t)pr * y_bs + g0;
    const bool has_g = diag_ != nullptr;
    const double *__restrict__ gg = has_g ? diag_ + (size_t)pr * diag_bs + g0 : yg;
    double *__restrict__ dg = d_ + pb;
    double *__restrict__ zg = SAMPLE ? z_ + (size_t)pr * y_bs + g0 : z_ + pb;
    const int own = 2 * c + g;                      // the column whose row-vector entries this lane carries
    // chunk-mode row stores: loop-invariant per-lane pointers, indexed with opaque_uniform(row)
    double *__restrict__ rg = (ROWSTORE && r_out) ? r_out + pb * 64 + own : nullptr;
    double *__restrict__ ug = (ROWSTORE && Ut_out) ? Ut_out + pb * 64 + own : nullptr;
    double *__restrict__ wg = (ROWSTORE && Wt_out) ? Wt_out + pb * 64 + own : nullptr;
    // a nominal pass (no w~ rows: nothing but the transition sweep reads what it stores) writes the first ROWS
    // columns of its 64-double rows only -- cfg3 (W = 40) moved 34 GB per evaluation, a third of it padding; the
    // stored factor's rows keep their zero padding (the solves read whole rows)
    const bool st_ok = own < ROWS || Wt_out != nullptr;
    double *__restrict__ eg = (ROWSTORE && de_out) ? de_out + pb : nullptr;
    double *__restrict__ Sg = S_state + (size_t)b * (64 * 64);     // [column][row]
    double *__restrict__ Fg = F_state + (size_t)b * 64;
    const double diag_add = diag_add_[pr];

    RowGen G;                                       // this lane generates its own column, as in k_factor3
    G.init(own, pr, Jr, Jc, block_sub, gap, ar_, cr_, ac_, bc_, cc_, dc_, cmax_, tg, g0);
    const double cj = G.cj;

    __shared__ __attribute__((aligned(16))) double s_w[64];     // r_{n-1}  (pending update, row form)
    __shared__ __attribute__((aligned(16))) double s_u[64];     // u~_n
    __shared__ __attribute__((aligned(16))) double s_e[64];     // block decay at reset rows
    const double2 *pw = (const double2 *)s_w + g, *pu = (const double2 *)s_u + g;
    const double2 *pe = (const double2 *)s_e + g;
    const bool f31 = c == 31;                       // block 31: pad column 62, forward solve in 63
    const bool fl = lane == 63;                     // own column 63: the forward solve
    const double not63 = fl ? 0.0 : 1.0, is31 = f31 ? 1.0 : 0.0;

    // this lane's two columns in memory, from its first row on (column 63 lives in F_state)
    double *__restrict__ col0 = Sg + (size_t)(2 * c) * 64 + 2 * g;
    double *__restrict__ col1 = (f31 ? Fg : Sg + (size_t)(2 * c + 1) * 64) + 2 * g;
    double T[ROWS / 2][2];
    const bool zero_start = (block_sub >> 30) & 1;  // nominal pass: the state slots are outputs only
    constexpr double thr = ST_THR;
    int cnt = 0, fill = 0;                          // steady mode: the rule's counters
    if constexpr (STEADY) {
        cnt = __builtin_amdgcn_readfirstlane((int)hdr[ST_CNT]);
        fill = __builtin_amdgcn_readfirstlane((int)hdr[ST_FILL]);
    }
#pragma unroll
    for (int m = 0; m < ROWS / 2; ++m) {
        T[m][0] = zero_start ? 0.0 : col0[4 * (m >> 1) + (m & 1)];
        T[m][1] = zero_start ? 0.0 : col1[4 * (m >> 1) + (m & 1)];
    }
    double q0 = 0.0, q1 = 0.0;
    int32_t fail = 0;

    double t_n1 = tg[1], t_n2 = tg[2];
    double y_n = yg[0], y_n1 = yg[1];
    double g_n = gg[0], g_n1 = gg[1];
    double ut, vt, de;
    bool rst;
    G.next(tg[0], g0, ut, vt, rst, de);

    double2 ub[S7_AHEAD + 1], wb[S7_AHEAD + 1];
    s_w[own] = 0.0;
    s_u[own] = ut;
    wave_lds_fence();
    sweep7_preload<ROWS>(ub, wb, pu, pw);

    int64_t n = 0;
    for (; n < rows; ++n) {
        const double a_n = (has_g ? g_n : 0.0) + diag_add, yy = y_n;
        const double ut_c = ut, vt_c = vt;
        const bool rst_c = rst;
        if constexpr (ROWSTORE) { if (eg && lane == 0) eg[n] = rst ? de : -1.0; }
        if (rst) {                          // wave-uniform: fold the pending update, then decay
            const double el = fm_exp(-cj * de);     // pad columns: cj = 0 -> 1
            s_e[own] = el;
            wave_lds_fence();
            double d0, d1, el0, el1;
            both_halves(el, el0, el1);              // decays of this lane's two state columns
            sweep7_preload<ROWS>(ub, wb, pe, pw);
            sweep7_run<ROWS, true>(T, ub, wb, pe, pw, q0, q1, el0, el1, d0, d1);
            sweep7_preload<ROWS>(ub, wb, pu, pw);
            q0 = 0.0;
            q1 = 0.0;
        }
        __builtin_amdgcn_s_setprio(0);
        double acc0, acc1;
        sweep7_run<ROWS, false>(T, ub, wb, pu, pw, q0, q1, 0.0, 0.0, acc0, acc1);
        __builtin_amdgcn_s_setprio(GF_CHAIN_PRIO);
        const double tmp = own_column_sum(acc0, acc1);
        const double r = (vt_c - tmp) * not63;
        double r0, r1;
        both_halves(r, r0, r1);                     // r of this lane's two state columns: off the d-chain
        G.next(t_n1, g0 + n + 1, ut, vt, rst, de);
        t_n1 = t_n2; y_n = y_n1; g_n = g_n1;
        t_n2 = tg[n + 3];
        y_n1 = yg[n + 2];
        g_n1 = gg[n + 2];
        wave_lds_fence();
        s_w[own] = r;
        s_u[own] = ut;
        wave_lds_fence();
        sweep7_preload<ROWS>(ub, wb, pu, pw);
        const double s1 = wave_sum(ut_c * tmp);     // u~ = 0 in the pad / forward-solve columns
        const double s2 = read_lane(tmp, 63);       // u~ . F~ (column 63)
        const double dn = a_n - s1;
        const double zn = SAMPLE ? __dsqrt_rn(dn) * yy : yy - s2;      // (the draw: x_n rides where z_n does)
        if (!(dn > 0.0)) {
            const int64_t gf = g0 + n + 1;
            fail = (int32_t)(gf > 0x7fffffff ? 0x7fffffff : gf);
            break;
        }
        const double inv = fast_rcp(dn);
        q0 = r0 * inv;                              // multipliers of this lane's two state columns;
        q1 = fma(zn, is31, r1) * inv;               // column 63: z / d (r is 0 there)
        if constexpr (ROWSTORE) {
            const size_t ro = opaque_uniform((size_t)n * 64);
            if (st_ok) {
                if (rg) rg[ro] = r;                 // r~ rows for k_phi (chunk mode)
                if (ug) ug[ro] = ut_c;
                if (wg) wg[ro] = r * inv;
            }
        }
        if (lane == 0) { dg[n] = dn; zg[n] = SAMPLE ? zn + s2 : zn; }
        if constexpr (STEADY) {
            // anchor of the 64-row grid (a block reset at every block: rho = 1, exact phasor): the rotated-frame
            // invariants of this row against those of ST_LAG such anchors (1024 rows) before
            const int64_t gn = g0 + n;
            if (rst_c && gn >= arm_from && (gn & (ST_GRID - 1)) == 0) {
                double cs, sn;
                both_halves(vt_c, cs, sn);          // v~ at an anchor: (cos, sin) of this lane's term
                const double Gr = fma(r0, cs, r1 * sn) * inv, Gi = fma(r1, cs, -r0 * sn) * inv;
                const double x = fl ? dn : (g ? Gi : Gr);       // (lane 63's own gain component is a pad: zero)
                double *__restrict__ slot = hdr + ST_RING + (size_t)((gn / ST_GRID) & (ST_LAG - 1)) * 64 + lane;
                const double xo = *slot;
                *slot = x;
                const double dx = fl ? 0.0 : fabs(x - xo);
                const double mdx = wave_max(dx), mx = wave_max(fl ? 0.0 : fabs(x));
                const double dold = read_lane(xo, 63);
                const bool ok = fill >= ST_LAG && mdx <= thr * mx && fabs(dn - dold) <= thr * dn && !G.qmode;
                cnt = ok ? cnt + 1 : 0;
                fill = fill < ST_LAG ? fill + 1 : fill;
                if (lane == 0) { hdr[ST_CNT] = (double)cnt; hdr[ST_FILL] = (double)fill; }
                if (cnt >= ST_COUNT && G.dt_ref > 0.0) {       // (a cached cadence: not on a tile's first row)
                    // the switch: freeze pivot and gains and hand the rest of the series to k_steady_tail.  The
                    // forward-solve column (this row's update folded; rho = 1 at an anchor) goes from the tiled layout
                    // (block 31, rows split over the half-waves) through LDS to the lanes of its terms, which turn it
                    // back by the anchor's phase: s = e^{-i d t} (F_2c + i F_2c+1)
                    wave_lds_fence();
                    if (f31) {
#pragma unroll
                        for (int m = 0; m < ROWS / 2; ++m) {
                            const int i = 2 * g + 4 * (m >> 1) + (m & 1);
                            s_e[i] = fma(s_w[i], q1, T[m][1]);
                        }
                    }
                    wave_lds_fence();
                    const double F0 = (2 * c + 1 < ROWS) ? s_e[2 * c] : 0.0, F1 = (2 * c + 1 < ROWS) ? s_e[2 * c + 1] : 0.0;
                    if (g == 0) {                   // (pad terms: cs = sn = 0, so their gain and state are zero)
                        hdr[ST_GR + c] = Gr;
                        hdr[ST_GI + c] = Gi;
                        hdr[ST_SR + c] = fma(cs, F0, sn * F1);
                        hdr[ST_SI + c] = fma(cs, F1, -sn * F0);
                    }
                    if (lane == 0) {
                        hdr[ST_SW] = (double)(gn + 1);
                        hdr[ST_D] = dn;
                        hdr[ST_DT] = (tg[n] - tg[n - ST_DLAG]) * (1.0 / ST_DLAG);
                    }
                    STEADY_EXIT(n + 1);             // (row n + 1 is the tail's first; rows 0 .. n were stored)
                }
            }
        }
    }
    if (fail) {
        if (lane == 0) info[b] = fail;
        if (zero_start) {                           // an output-only slot is never left stale: the combines read
            for (int m = 0; m < 32; ++m) {          // its padding as zeros (a failed chunk's state means nothing)
                col0[4 * (m >> 1) + (m & 1)] = 0.0;
                col1[4 * (m >> 1) + (m & 1)] = 0.0;
            }
            if (f31)
                for (int m = 0; m < 32; ++m) Sg[63 * 64 + 2 * g + 4 * (m >> 1) + (m & 1)] = 0.0;
        }
        STEADY_EXIT(N);                             // (not switched: the reduction takes the tile's N rows, stale ones too)
    }
    wave_lds_fence();
#pragma unroll
    for (int m = 0; m < ROWS / 2; ++m) {
        const double w = s_w[2 * g + 4 * (m >> 1) + (m & 1)];
        col0[4 * (m >> 1) + (m & 1)] = fma(w, q0, T[m][0]);
        col1[4 * (m >> 1) + (m & 1)] = fma(w, q1, T[m][1]);
    }
    if (zero_start) {                               // the slot is an output only: its padding rows too
        for (int m = ROWS / 2; m < 32; ++m) {
            col0[4 * (m >> 1) + (m & 1)] = 0.0;
            col1[4 * (m >> 1) + (m & 1)] = 0.0;
        }
        if (f31)                                    // S's own column 63 (these lanes' second column is F~)
            for (int m = 0; m < 32; ++m) Sg[63 * 64 + 2 * g + 4 * (m >> 1) + (m & 1)] = 0.0;
    }
    STEADY_EXIT(N);                                 // the end of the tile, not switched: all its rows
  }
#undef STEADY_EXIT
tile_sums:
    if constexpr (STEADY) {
        // lane 0 stored this tile's d and z (and the other lanes read them back now): its stores are ordered before
        // the loads at workgroup scope -- the block is this one wave -- and the sums run at the tail waves' priority
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        steady_tile_sums(d_ + (size_t)pr * N, z_ + (size_t)pr * N, N, tile_lim, acc_ + (size_t)pr * RED_NACC, acc_init, lane);
    }
}

// ------------------------------------------------------------------------------------
// k_steady_tail: the rows behind the switch of the steady mode, as a time-invariant filter in blocks of 64 rows.
//
// With pivot, gains and cadence frozen, a row is  x = lambda o s ;  z_n = y_n - sum_k Re(alpha_k x_k) ;
// s = x + G z_n  with, per complex term k, alpha = a + i b, lambda = exp(-(c + i d) Delta), G the derotated gain and
// s the derotated forward-solve state (this row's update folded): no row generator, no block scaling, no resets,
// and no reduction on the row's chain.  A block of 64 rows from incoming s:
//   p_i  = y_i - sum_k Re(alpha_k lambda_k^(i+1) s_k)       lane = row; s by LDS broadcast, coefficients in registers
//   z    = H p,  H lower-triangular Toeplitz of the impulse response h(0 .. 63)     (h(63) ~ 5e-3 on the flagship
//          kernel: H is not truncated); lane i reads p[i - m] from an LDS image of p with 64 zeros in front
//   s   <- lambda^2 s + lambda G z_j + G z_j+1              lane = term, two rows per step, z by LDS broadcast
//          (k_steady_finish: on both half-waves, rows 32 .. 63 from a zero state, joined by lambda^32 -- FOLD below)
// k_steady_finish folds the first two lines (FOLD below): with p = y + C s,  z = H y + Q s,  Q = H C.  Q takes C's
// registers (one row per lane; the set-up applies H to each of C's columns: a column lies one row per lane and moves
// up one lane per tap, DPP wave_shr:1, h by broadcast), u = H y depends on the data alone and is formed for 16 blocks
// at once on the matrix pipe in front of them (the group phase, below), and the chain from a block's state to the
// next is  s -> LDS -> z = u + Q s -> LDS -> state update -> join: H's 64 reads and its 32-deep FMA chains are off it.
// h is the row form's answer to a unit impulse, computed at the problem's first tail entry of an evaluation and kept
// in the steady buffer; the p coefficients are recomputed at every launch (per lane one fm_sincos + fm_exp per term,
// through an LDS staging area of 8 terms so that the loop over the terms is not unrolled around them).
// One wave per problem, grid B; rows [max(switch row + 1, tile start), tile end) of a problem that has switched.
// t and y arrive by one coalesced load per block, issued a block ahead (k_steady_finish: t so, y in the group phase's
// operand layout for 16 blocks at once); d (= d_inf) and z leave by one coalesced
// store per block (k_steady_tail; k_steady_finish, the streamed log-likelihood's instance, stores no row: below).
// A partial last block runs the same code: H is lower triangular, so the rows beyond the tile (y clamped to the
// last row) touch no row before them; the s loop is bounded and the stores are masked.  (k_steady_finish: behind its
// group's full blocks, with its own column of the group's U.)
// Every spacing t_r - t_{r-1} of a tail row r is tested as RowGen tests it (a gap: > gthr; off the frozen cadence:
// >= jthr): a hit raises ST_VIOL and the rows of that evaluation mean nothing (finite).  The finishing launches skip
// the test, its loads of t and the flag where the caller has proved it for every tail row (PROVEN,
// GF_SWEEP_AXIS_PROVEN: the engine's axis scan): the other bits of the launch do not depend on it.
// ------------------------------------------------------------------------------------
constexpr int STT_STAGE = 8;        // terms per staging pass of the p coefficients
constexpr int FG = 6;               // terms per group of s broadcasts in the folded block's z phase
// lane i <- lane i - 1, lane 0 <- 0 (DPP wave_shr:1, one move per half of the double)
__device__ __forceinline__ double wave_shr1(const double v) { return dpp_get<0x138, 0xf>(v); }
// closes a stage of a hand-staged basic block: the LDS reads behind it are issued behind it (the fence orders them
// where the block is laid out, the scheduling barrier where it is scheduled); no instruction of its own
__device__ __forceinline__ void stage_end() {
    wave_lds_fence();
    __builtin_amdgcn_sched_barrier(0);
}

// a complex number in double-double, (rh + rl) + i (ih + il), and the product of two of them: the set-up's powers of
// lambda (steady_tail_rows, FOUR).  Products split exactly by FMA, sums by Knuth's two-sum; no fast-math here
struct cdd { double rh, rl, ih, il; };
__device__ __forceinline__ void dd_sum(const double a, const double b, double &s, double &e) {
#pragma clang fp contract(off)
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// hi + lo of p1 + sg p2 + tail, with p1, p2 given as exact products (p, e)
__device__ __forceinline__ void dd_pair(const double a1, const double b1, const double a2, const double b2, const double sg,
                                        const double tail, double &hi, double &lo) {
#pragma clang fp contract(off)
    const double p1 = a1 * b1, e1 = fma(a1, b1, -p1);
    const double p2 = sg * (a2 * b2), e2 = sg * fma(a2, b2, -(a2 * b2));
    double s, es;
    dd_sum(p1, p2, s, es);
    const double l = es + ((e1 + e2) + tail);
    dd_sum(s, l, hi, lo);
}
__device__ __forceinline__ cdd cdd_mul(const cdd a, const cdd b) {
    cdd c;
    dd_pair(a.rh, b.rh, a.ih, b.ih, -1.0, fma(a.rh, b.rl, a.rl * b.rh) - fma(a.ih, b.il, a.il * b.ih), c.rh, c.rl);
    dd_pair(a.rh, b.ih, a.ih, b.rh, 1.0, fma(a.rh, b.il, a.rl * b.ih) + fma(a.ih, b.rl, a.il * b.rh), c.ih, c.il);
    return c;
}

// STORE = true: the rows leave as d and z (k_steady_tail, tile by tile); STORE = false: no row is stored, every lane
// keeps the running sum of z^2 of its row slot over all blocks, and the wave adds the problem's tail to acc
// (k_steady_finish: rows [switch row, N) of the whole series in one launch).
//
// CHUNK != 0 (STORE = false only): one wave of the chunked finishing launch (k_steady_chunk, below).  Behind the
// switch a block is linear and time-invariant in the state -- z = u + Q s, s' = M s + K u --, so a chunk of n blocks
// from s_in ends in M^n s_in + (its end state from zero), and the chunks of one tail run side by side:
//   CHUNK = 1 (pass A): wave (problem, c) runs the rows [sw + c chunk_rows, sw + (c + 1) chunk_rows) -- chunk 0 from the
//     header's state, keeping its sum of z^2; the others from zero, for their end state alone; the last one (c > 0)
//     not at all -- and writes the end state to its workspace slot;
//   CHUNK = 3 (one wave per problem of three chunks or more, no spacing test): M, the full block's own code on the
//     2 Jc unit states with u = 0, column by column into the workspace's P;
//   CHUNK = 2 (pass B, behind k_steady_chunk_power, which leaves P = M^n there): wave c >= 1 forms its true s_in,
//     s_in[1] = s_out[0], s_in[c + 1] = s_out0[c] + P s_in[c], runs its rows from it and writes its sum of z^2 to its
//     slot; the last chunk writes the header's state.
// No two waves write different values to one word: acc is k_steady_chunk_sum's, the header's state the last chunk's,
// ST_VIOL takes the same value from any wave, and h is computed by every wave for itself (ST_H, ST_HOK read only).
// chunk_rows is a multiple of 16 blocks, so every chunk starts on the problem's own grid of groups: u keeps the bits
// of the one-wave launch.
constexpr int CH_P = 64 * 64;       // workspace of a problem: P[64][64] over (s_r[0..31], s_i[0..31]), then the slots
constexpr int CH_SLOT = 72;         // a chunk's slot: [0, 64) its end state, [64] its sum of z^2

template <int ROWS, bool STORE, int CHUNK = 0, bool PROVEN = false>
__device__ __forceinline__ void
steady_tail_rows(const int64_t N, const int64_t n_first, const int Jc, const double gap,
                 const double *__restrict__ ac_, const double *__restrict__ bc_,
                 const double *__restrict__ cc_, const double *__restrict__ dc_, const double *__restrict__ cmax_,
                 const double *__restrict__ t_, const int64_t t_bs, const double *__restrict__ y_, const int64_t y_bs,
                 double *__restrict__ d_, double *__restrict__ z_, const int32_t *__restrict__ info,
                 double *__restrict__ steady_, double *__restrict__ acc_,
                 const int64_t sw_lo, const int64_t sw_hi,
                 const int64_t chunk_rows = 0, double *__restrict__ ws_ = nullptr, const int64_t ws_ld = 0) {
    static_assert(CHUNK == 0 || !STORE, "the chunked launch stores no row");
    static_assert(!PROVEN || (!STORE && CHUNK != 3), "GF_SWEEP_AXIS_PROVEN is the finishing launches' (M's waves test nothing)");
    constexpr int JT = ROWS / 2;                    // term slots (Jc <= JT <= 32; slots from Jc on are zero)
    // the finishing instance's form of a block: the state update on both half-waves (lane 32 h + k: term k, rows 32 h ..
    // 32 h + 31 of a block), and H off the chain from one block's state to the next, z = H (y + C s) = H y + Q s with
    // Q = H C (both below); k_steady_tail keeps the update on the lower half-wave and the three phases in series
    constexpr bool FOLD = !STORE;
    // the folded block's state update takes four rows per step; ROWS = 64 has no registers for its constants (256
    // VGPRs and a spill) and keeps the two-row step
    constexpr bool FOUR = FOLD && ROWS < 64;
    const int lane = threadIdx.x, pr = blockIdx.x;
    const int half = lane >> 5, tk = FOLD ? (lane & 31) : lane;    // tk: the term whose constants this lane holds
    if (info[pr] != 0) return;
    double *__restrict__ hdr = steady_ + (size_t)pr * ST_SIZE;
    const double swd = hdr[ST_SW];
    if (!(swd > 0.0)) return;
    const int64_t sw = (int64_t)swd;                // first tail row (global, >= 1)
    if constexpr (!STORE) { if (sw < sw_lo || sw >= sw_hi) return; }    // another launch's problem: nothing touched
    const int64_t nb = sw > n_first ? sw - n_first : 0;     // first tail row of this tile (local)
    if (nb >= N) return;
    // the rows [r_lo, r_hi) of this wave: the whole tail, or one chunk of it
    int64_t r_lo_ = nb, r_hi_ = N;
    int ch = 0, nch = 1;
    double *__restrict__ wsp = nullptr;
    if constexpr (CHUNK != 0) {
        ch = blockIdx.y;
        nch = (int)((N - nb + chunk_rows - 1) / chunk_rows);
        wsp = ws_ + (size_t)pr * ws_ld;
        if constexpr (CHUNK == 3) {
            if (nch < 3) return;                    // no chunk takes a correction by P
            r_hi_ = nb + 128 * (int64_t)Jc;         // 2 Jc blocks; no row of the series is read for them
        } else {
            if (ch >= nch) return;
            if (CHUNK == 1 && ch > 0 && ch == nch - 1) return;
            if (CHUNK == 2 && ch == 0) return;
            r_lo_ = nb + ch * chunk_rows;
            r_hi_ = (N - r_lo_ > chunk_rows) ? r_lo_ + chunk_rows : N;
        }
    }
    const int64_t r_lo = r_lo_, r_hi = r_hi_;
    const double *__restrict__ tg = t_ + (size_t)pr * t_bs + n_first;
    const double *__restrict__ yg = y_ + (size_t)pr * y_bs + n_first;
    double *__restrict__ dg = STORE ? d_ + (size_t)pr * N : nullptr;
    double *__restrict__ zg = STORE ? z_ + (size_t)pr * N : nullptr;
    const double dinf = hdr[ST_D], delta = hdr[ST_DT];
    double zsq = 0.0;                               // STORE = false: sum of z^2 over this lane's rows

    __shared__ __attribute__((aligned(16))) double s_s[64];         // (s_r, s_i) of term k at [2k], [2k + 1]
    __shared__ __attribute__((aligned(16))) double s_p[128];        // 64 zeros, then p of the block
    // impulse response; FOLD: behind 16 zeros, h at a negative index for the group phase's tiles on H's diagonal
    __shared__ __attribute__((aligned(16))) double s_h[FOLD ? 16 + 64 : 64];
    double *const hh = s_h + (FOLD ? 16 : 0);       // h(0)
    __shared__ __attribute__((aligned(16))) double s_z[64];         // z of the block
    __shared__ double s_c[STT_STAGE][2][64];                        // staging of the p coefficients
    // 64 rows of H against an image: lane i adds h(m) v[i - m], m in [0, 64), even m to a0 and odd m to a1
    auto taps = [&](const double *pp, double &a0, double &a1) {
#pragma unroll
        for (int m = 0; m < 64; m += 2) {
            const double2 hv = ((const double2 *)hh)[m >> 1];
            a0 = fma(hv.x, pp[-m], a0);
            a1 = fma(hv.y, pp[-m - 1], a1);
        }
    };
    // the same on a vector that lies one row per lane, without an image: lane i adds h(m) v[i - m] with v moved up one
    // lane per tap (a DPP wave shift; zeros come in at lane 0).  Two vectors against one read of h, in a loop that stays
    // rolled: the set-up's form, which runs with Q in the registers
    auto shifted_taps = [&](double va, double vb, double &ra, double &rb) {
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
#pragma unroll 1
        for (int m = 0; m < 64; m += 2) {
            const double2 hv = ((const double2 *)hh)[m >> 1];
            a0 = fma(hv.x, va, a0);
            b0 = fma(hv.x, vb, b0);
            va = wave_shr1(va);
            vb = wave_shr1(vb);
            a1 = fma(hv.y, va, a1);
            b1 = fma(hv.y, vb, b1);
            va = wave_shr1(va);
            vb = wave_shr1(vb);
        }
        ra = a0 + a1;
        rb = b0 + b1;
    };

    // lane = term: this term's constants and state
    const bool term = tk < Jc;
    const size_t ck = (size_t)pr * Jc + (term ? tk : 0);
    const double ck_c = term ? cc_[ck] : 0.0, ck_d = term ? dc_[ck] : 0.0;
    const double ck_a = term ? ac_[ck] : 0.0, ck_b = term ? bc_[ck] : 0.0;
    const double wmax = wave_max(fmax(ck_c, fabs(ck_d)));
    const double gthr = gap / cmax_[pr], jthr = 2e-6 / wmax;        // RowGen::init's thresholds
    double lr, li;                                                  // lambda = exp(-c Delta) (cos - i sin)(d Delta)
    {
        double sn, cs;
        fm_sincos(ck_d * delta, &sn, &cs);
        const double e = fm_exp(-ck_c * delta);
        lr = e * cs;
        li = -e * sn;
    }
    const bool gain = FOLD || lane < 32;
    const double Gr = gain ? hdr[ST_GR + (lane & 31)] : 0.0, Gi = gain ? hdr[ST_GI + (lane & 31)] : 0.0;
    double sr = (lane < 32) ? hdr[ST_SR + (lane & 31)] : 0.0, si = (lane < 32) ? hdr[ST_SI + (lane & 31)] : 0.0;
    if constexpr (CHUNK == 1) {
        if (ch > 0) { sr = 0.0; si = 0.0; }
    }
    if constexpr (CHUNK == 2) {
        // this chunk's true incoming state from the end states of pass A, lane = element of (s_r[0..31], s_i[0..31]):
        // v = s_out[0];  v <- s_out0[c'] + P v  for c' = 1 .. ch - 1, v by LDS broadcast, P's row from memory
        const double *__restrict__ slot = wsp + CH_P;
        const double *__restrict__ prow = wsp + 64 * lane;
        double v = slot[lane];
        for (int cp = 1; cp < ch; ++cp) {
            wave_lds_fence();
            s_z[lane] = v;
            wave_lds_fence();
            double a0 = slot[cp * CH_SLOT + lane], a1 = 0.0;
#pragma unroll 4
            for (int k = 0; k < 64; k += 2) {
                const double2 vv = ((const double2 *)s_z)[k >> 1];
                a0 = fma(prow[k], vv.x, a0);
                a1 = fma(prow[k + 1], vv.y, a1);
            }
            v = a0 + a1;
        }
        wave_lds_fence();
        s_z[lane] = v;
        wave_lds_fence();
        sr = (lane < 32) ? s_z[lane] : 0.0;
        si = (lane < 32) ? s_z[lane + 32] : 0.0;
        wave_lds_fence();
    }
    const double l2r = fma(lr, lr, -li * li), l2i = 2.0 * lr * li;  // lambda^2
    const double lgr = fma(lr, Gr, -li * Gi), lgi = fma(lr, Gi, li * Gr);   // lambda G
    double l32r = l2r, l32i = l2i;                                  // FOLD: lambda^32 joins the two half-blocks
    if constexpr (FOLD) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xr = fma(l32r, l32r, -l32i * l32i);
            l32i = 2.0 * l32r * l32i;
            l32r = xr;
        }
    }

    // impulse response: the row form on y = (1, 0, 0, ...) from s = 0, once per evaluation
    if (hdr[ST_HOK] != 0.0) {
        hh[lane] = hdr[ST_H + lane];
    } else {
        double hr = Gr, hi = Gi, hv = (lane == 0) ? 1.0 : 0.0;      // h(0) = 1, s = G
        const double ha = (lane < 32) ? ck_a : 0.0, hb = (lane < 32) ? ck_b : 0.0;  // (each term once in the sum)
        for (int m = 1; m < 64; ++m) {
            const double xr = fma(lr, hr, -li * hi), xi = fma(lr, hi, li * hr);
            const double hm = -wave_sum(fma(ha, xr, -hb * xi));
            hr = fma(Gr, hm, xr);
            hi = fma(Gi, hm, xi);
            hv = (lane == m) ? hm : hv;
        }
        hh[lane] = hv;
        if constexpr (CHUNK == 0) {                 // (a chunk's wave keeps h to itself: its neighbours may be reading)
            hdr[ST_H + lane] = hv;
            if (lane == 0) hdr[ST_HOK] = 1.0;
        }
    }
    if constexpr (!FOLD) s_p[lane] = 0.0;
    else if (lane < 16) s_h[lane] = 0.0;

    // lane = row of a block: -alpha_k lambda_k^(i+1) = (pr_k, pi_k) with Re(.) taken against (s_r, s_i):
    // p = y + sum_k pr_k s_r,k + pi_k s_i,k.  FOLD: H applied to each of these 2 JT columns where they are
    // computed (shifted_taps): pcr, pci hold the rows of Q, z = H y + sum_k pr_k s_r,k + pi_k s_i,k
    double pcr[JT], pci[JT];
    const double di = delta * (double)(lane + 1);
#pragma unroll
    for (int k0 = 0; k0 < JT; k0 += STT_STAGE) {
        wave_lds_fence();
#pragma unroll 1
        for (int kk = 0; kk < STT_STAGE; ++kk) {
            const int k = k0 + kk;
            double vr = 0.0, vi = 0.0;
            if (k < Jc) {                           // wave-uniform
                const size_t uk = (size_t)pr * Jc + k;
                const double a = ac_[uk], b = bc_[uk];
                double sn, cs;
                fm_sincos(dc_[uk] * di, &sn, &cs);
                const double e = fm_exp(-cc_[uk] * di);
                vr = -e * fma(a, cs, b * sn);       // Re(alpha lambda^(i+1)), Im = e (b cs - a sn)
                vi = e * fma(b, cs, -a * sn);
                if constexpr (FOLD) shifted_taps(vr, vi, vr, vi);
            }
            s_c[kk][0][lane] = vr;
            s_c[kk][1][lane] = vi;
        }
        wave_lds_fence();
#pragma unroll
        for (int kk = 0; kk < STT_STAGE; ++kk) {
            if (k0 + kk < JT) { pcr[k0 + kk] = s_c[kk][0][lane]; pci[k0 + kk] = s_c[kk][1][lane]; }
        }
    }

    const int64_t last = N - 1;
    auto row_of = [&](const int64_t cb) { const int64_t i = cb + lane; return i < last ? i : last; };
    bool viol = false;
    double t_nx = 0.0, tp_nx = 0.0;
    if constexpr (!PROVEN) { t_nx = tg[row_of(r_lo)]; tp_nx = tg[row_of(r_lo) - 1]; }
    // the pieces every form of a block shares: term k of p (or of Q s) against the broadcast (s_r, s_i), even terms to
    // x0 and odd ones to x1; the state over two rows z_j, z_j+1, and over one
    auto add_term = [&](const int k, const double2 sv, double &x0, double &x1) {
        if (k & 1) x1 = fma(pci[k], sv.y, fma(pcr[k], sv.x, x1));
        else x0 = fma(pci[k], sv.y, fma(pcr[k], sv.x, x0));
    };
    auto two_rows = [&](const double2 zz) {
        const double wr = fma(lgr, zz.x, Gr * zz.y), wi = fma(lgi, zz.x, Gi * zz.y);
        const double nr = fma(l2r, sr, fma(-l2i, si, wr));
        si = fma(l2r, si, fma(l2i, sr, wi));
        sr = nr;
    };
    auto one_row = [&](const double zj) {
        const double nr = fma(lr, sr, fma(-li, si, Gr * zj));
        si = fma(lr, si, fma(li, sr, Gi * zj));
        sr = nr;
    };
    if constexpr (!FOLD) {
    double y_nx = yg[row_of(nb)];
    for (int64_t cb = nb; cb < N; cb += 64) {
        const double yv = y_nx, tv = t_nx, tp = tp_nx;              // rows cb + lane (clamped to the tile's last)
        {
            const int64_t i = row_of(cb + 64);
            y_nx = yg[i]; t_nx = tg[i]; tp_nx = tg[i - 1];
        }
        const int lim = (int)(N - cb < 64 ? N - cb : 64);
        const double dt = tv - tp;
        viol |= (lane < lim) && ((dt > gthr) || !(fabs(dt - delta) < jthr));
        wave_lds_fence();
        if (lane < 32) { s_s[2 * lane] = sr; s_s[2 * lane + 1] = si; }
        wave_lds_fence();
        double p0 = yv, p1 = 0.0;
#pragma unroll
        for (int k = 0; k < JT; ++k) add_term(k, ((const double2 *)s_s)[k], p0, p1);
        s_p[64 + lane] = p0 + p1;
        wave_lds_fence();
        double z0 = 0.0, z1 = 0.0;
        taps(s_p + 64 + lane, z0, z1);
        const double zv = z0 + z1;
        s_z[lane] = zv;
        wave_lds_fence();
        if (lane < lim) { dg[cb + lane] = dinf; zg[cb + lane] = zv; }
        // the state update, two rows per step
        int j = 0;
#pragma unroll 4
        for (; j + 1 < lim; j += 2) two_rows(((const double2 *)s_z)[j >> 1]);
        if (j < lim) one_row(s_z[j]);
    }
    } else {
    // The folded block.  u = H y of a block depends on the data alone, and on its own block's alone (H is the Toeplitz
    // triangle inside a block): the group phase forms it for 16 consecutive blocks at once, on the matrix pipe, as
    // U = H [y_k .. y_k+15], a (64 x 64) (64 x 16) product in 16 x 16 tiles of H against 4-row slices of Y
    // (v_mfma_f64_16x16x4_f64).  H is lower block-triangular: 10 tiles x 4 slices = 40 MFMAs into one accumulator per
    // 16 rows of U.  No lane shifts and no broadcasts of h:
    //   B (4 x 16, slice q of Y's tile Jt): lane l holds y[g0 + 64 (l & 15) + 16 Jt + 4 q + (l >> 4)] straight from
    //     memory, its index clamped to the series' last row as row_of clamps (rows < N only); 16 loads per group;
    //   A (16 x 4, slice q of H's tile type d = I - Jt): lane l holds h(16 d + (l & 15) - 4 q - (l >> 4)), zero at a
    //     negative index: one read of s_h with its 16 zeros in front, 19 consecutive doubles per read;
    //   D: lane l holds U[16 I + (l >> 4) + 4 r][block l & 15] in element r; it goes to s_u[block][row] with a row
    //     stride of 64 + 1 doubles: a 64-bit LDS store is served in groups of 16 consecutive lanes over 32 banks, and
    //     the 16 blocks of a group then fall on its 16 double-wide banks (no conflict; a pad of 2 measured 2-way).
    // A block then takes its u, lane = row, by one read.  A partial group runs the same phase: its surplus columns hold
    // clamped rows, columns do not mix, and nothing reads them.  The chain of a block stays
    // s -> LDS -> z = u + Q s -> LDS -> state update -> join.
    constexpr int SU = 64 + 1;
    __shared__ __attribute__((aligned(16))) double s_u[16 * SU];
    const int mc = lane & 15, mk = lane >> 4;
    auto group_phase = [&](const int64_t g0) {
        double ha[4][4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int q = 0; q < 4; ++q) ha[d][q] = hh[16 * d + mc - 4 * q - mk];
        d4 U[4];
#pragma unroll
        for (int I = 0; I < 4; ++I) U[I] = d4{0.0, 0.0, 0.0, 0.0};
        const int64_t r0 = g0 + 64 * mc + mk;
#pragma unroll
        for (int Jt = 0; Jt < 4; ++Jt) {
            double yb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t i = r0 + 16 * Jt + 4 * q;
                yb[q] = yg[i < last ? i : last];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int I = Jt; I < 4; ++I) U[I] = GF_MFMA64(ha[I - Jt][q], yb[q], U[I]);
        }
        wave_lds_fence();                           // behind the last block's read of its u
#pragma unroll
        for (int I = 0; I < 4; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_u[mc * SU + 16 * I + mk + 4 * r] = U[I][r];
        wave_lds_fence();
    };
    // the state update: the lower half-wave takes the block's rows 0 .. 31 from the incoming state, the upper one the
    // rows 32 .. 63 from a zero state -- half the chain --, and s <- lambda^(rows of the upper half) s_low + s_high
    // joins them (the update is linear in the state); the upper half starts the next block from zero again.  A
    // partial block (the series' last) splits the same way with the rows it has.
    const double *zb = s_z + 32 * half;
    auto join = [&](const double jr, const double ji) {
        double slr, sur, sli, sui;
        both_halves(sr, slr, sur);
        both_halves(si, sli, sui);
        sr = half ? 0.0 : fma(jr, slr, fma(-ji, sli, sur));
        si = half ? 0.0 : fma(jr, sli, fma(ji, slr, sui));
    };
    // The four-row step's constants, lambda^4 and lambda^k G, k = 1 .. 3, and the join's lambda^32.  A constant that is
    // off by a rounding is off the same way in every step of a tail, and lambda^32 by squarings in double gathers 30 of
    // them: the powers are formed in double-double, once per launch, and each constant is rounded once
    double l4r = 0.0, l4i = 0.0, g1r = 0.0, g1i = 0.0, g2r = 0.0, g2i = 0.0, g3r = 0.0, g3i = 0.0;
    if constexpr (FOUR) {
        const cdd l1{lr, 0.0, li, 0.0}, gd{Gr, 0.0, Gi, 0.0};
        const cdd l2 = cdd_mul(l1, l1), l3 = cdd_mul(l2, l1), l4 = cdd_mul(l2, l2);
        cdd lp = l4;
#pragma unroll
        for (int q = 0; q < 3; ++q) lp = cdd_mul(lp, lp);
        const cdd g1 = cdd_mul(l1, gd), g2 = cdd_mul(l2, gd), g3 = cdd_mul(l3, gd);
        l4r = l4.rh; l4i = l4.ih;
        l32r = lp.rh; l32i = lp.ih;
        g1r = g1.rh; g1i = g1.ih; g2r = g2.rh; g2i = g2.ih; g3r = g3.rh; g3i = g3.ih;
    }
    // FOLD, the full block's forms.  The terms k (even) and k + 1 of Q s with the two accumulators in turn, so that no
    // FMA waits on the one issued in front of it; each accumulator takes its terms in add_term's order: the same bits
    auto add_pair = [&](const int k, const double2 sa, const double2 sb, double &x0, double &x1) {
        x0 = fma(pcr[k], sa.x, x0);
        x1 = fma(pcr[k + 1], sb.x, x1);
        x0 = fma(pci[k], sa.y, x0);
        x1 = fma(pci[k + 1], sb.y, x1);
    };
    // the state over four rows z_j .. z_j+3:  s <- lambda^4 s + w,  w = lambda^3 G z_j + lambda^2 G z_j+1 +
    // lambda G z_j+2 + G z_j+3.  w does not depend on the state: eight instructions off the chain from block to block,
    // which keeps the two dependent FMAs per component on lambda^4 -- half of what two two-row steps have
    auto four_w = [&](const double2 za, const double2 zc, double &wr, double &wi) {
        wr = fma(g3r, za.x, fma(g2r, za.y, fma(g1r, zc.x, Gr * zc.y)));
        wi = fma(g3i, za.x, fma(g2i, za.y, fma(g1i, zc.x, Gi * zc.y)));
    };
    auto four_s = [&](const double wr, const double wi) {
        const double nr = fma(l4r, sr, fma(-l4i, si, wr));
        si = fma(l4r, si, fma(l4i, sr, wi));
        sr = nr;
    };
    int64_t cb = r_lo;
    // A group: its phase, then its blocks.  The full blocks: one basic block each, in stages.  A stage ends in a
    // scheduling barrier, so that its LDS reads are issued a stage before the FMAs that take them and no further ahead
    // (the registers hold Q): the s broadcasts in groups of FG terms, z of the state update eight rows ahead.
    if constexpr (CHUNK == 3) {                     // M is the block's map at u = 0; the unused columns of P are zero
        for (int i = lane; i < 16 * SU; i += 64) s_u[i] = 0.0;
        for (int i = lane; i < 64 * (32 - Jc); i += 64) {
            const int r = i / (32 - Jc), k = Jc + i % (32 - Jc);
            wsp[64 * r + k] = 0.0;
            wsp[64 * r + 32 + k] = 0.0;
        }
        wave_lds_fence();
    }
    while (cb < r_hi) {
    if constexpr (CHUNK != 3) group_phase(cb);
    const double *ub = s_u + lane;                  // this lane's row of the block's u
    // the group's full blocks, counted in 32 bits (cb moves behind them)
    const int nfull = (r_hi - cb >= 16 * 64) ? 16 : (int)((r_hi - cb) >> 6);
    for (int c = 0; c < nfull; ++c, ub += SU) {
        if constexpr (CHUNK == 3) {                 // block j of this wave: unit state j (s_r of term j, then s_i)
            const int j = (int)((cb - r_lo) >> 6) + c;
            sr = (j < Jc && lane == j) ? 1.0 : 0.0;
            si = (j >= Jc && lane == j - Jc) ? 1.0 : 0.0;
        } else if constexpr (!PROVEN) {
        const double tv = t_nx, tp = tp_nx;         // t of the rows cb + 64 c + lane
        {
            const int64_t i = row_of(cb + 64 * (int64_t)(c + 1));
            t_nx = tg[i]; tp_nx = tg[i - 1];
        }
        const double dt = tv - tp;
        viol |= (dt > gthr) || !(fabs(dt - delta) < jthr);
        }
        wave_lds_fence();
        if (lane < 32) { s_s[2 * lane] = sr; s_s[2 * lane + 1] = si; }
        wave_lds_fence();
        constexpr int NG = (JT + FG - 1) / FG;
        double z0 = *ub, z1 = 0.0;
        double2 sv[2][FG], zz[16];
        auto s_ld = [&](const int g) {
#pragma unroll
            for (int i = 0; i < FG; ++i)
                if (g * FG + i < JT) sv[g & 1][i] = ((const double2 *)s_s)[g * FG + i];
        };
        s_ld(0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) s_ld(g + 1);
            stage_end();
#pragma unroll
            for (int i = 0; i < FG; i += 2) {       // (FG and JT are even: a pair lies in one group)
                const int k = g * FG + i;
                if (k < JT) add_pair(k, sv[g & 1][i], sv[g & 1][i + 1], z0, z1);
            }
        }
        const double zv = z0 + z1;
        s_z[lane] = zv;
        wave_lds_fence();
        zsq = fma(zv, zv, zsq);
#pragma unroll
        for (int i = 0; i < 8; ++i) zz[i] = ((const double2 *)zb)[i];
        if constexpr (FOUR) {
            // eight trips of four rows; w of a trip is formed in the stage of the trip in front of it, beside that
            // trip's two FMAs on the state, and z is read two trips ahead of its w
            double wr, wi;
            stage_end();
            four_w(zz[0], zz[1], wr, wi);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (t == 1 || t == 3) {
#pragma unroll
                    for (int i = 6 + 2 * t; i < 10 + 2 * t; ++i) zz[i] = ((const double2 *)zb)[i];
                }
                stage_end();
                double nwr = 0.0, nwi = 0.0;
                if (t < 7) four_w(zz[2 * t + 2], zz[2 * t + 3], nwr, nwi);
                four_s(wr, wi);
                wr = nwr;
                wi = nwi;
            }
        } else {
#pragma unroll
        for (int j2 = 0; j2 < 16; ++j2) {
            if (j2 >= 4 && j2 < 12 && (j2 & 3) == 0) {
#pragma unroll
                for (int i = j2 + 4; i < j2 + 8; ++i) zz[i] = ((const double2 *)zb)[i];
            }
            stage_end();
            two_rows(zz[j2]);
        }
        }
        join(l32r, l32i);
        if constexpr (CHUNK == 3) {
            if (lane < 32) {                        // column j of M
                const int j = (int)((cb - r_lo) >> 6) + c, col = j < Jc ? j : 32 + j - Jc;
                wsp[64 * lane + col] = sr;
                wsp[64 * (32 + lane) + col] = si;
            }
        }
    }
    cb += 64 * (int64_t)nfull;
    if (nfull < 16 && cb < r_hi) {                  // a partial last block (of the series, or of M's 2 Jc): lim rows
        const int lim = (int)(r_hi - cb);
        if constexpr (!PROVEN) {                    // (PROVEN: the caller's proof covers these rows too; t is not read)
            const double dt = t_nx - tp_nx;
            viol |= (lane < lim) && ((dt > gthr) || !(fabs(dt - delta) < jthr));
        }
        wave_lds_fence();
        if (lane < 32) { s_s[2 * lane] = sr; s_s[2 * lane + 1] = si; }
        wave_lds_fence();
        double z0 = *ub, z1 = 0.0;
#pragma unroll
        for (int k = 0; k < JT; ++k) {
            add_term(k, ((const double2 *)s_s)[k], z0, z1);
            if (k % FG == FG - 1) stage_end();
        }
        const double zv = z0 + z1;
        s_z[lane] = zv;
        wave_lds_fence();
        zsq = (lane < lim) ? fma(zv, zv, zsq) : zsq;
        const int mine = half ? (lim > 32 ? lim - 32 : 0) : (lim < 32 ? lim : 32);
        int j = 0;
        if constexpr (FOUR) {                       // four-row trips while they fit, then row by row
#pragma unroll 1
            for (; j + 3 < mine; j += 4) {
                double wr, wi;
                four_w(((const double2 *)zb)[j >> 1], ((const double2 *)zb)[(j >> 1) + 1], wr, wi);
                four_s(wr, wi);
            }
#pragma unroll 1
            for (; j < mine; ++j) one_row(zb[j]);
        } else {
#pragma unroll 1
        for (; j + 1 < mine; j += 2) two_rows(((const double2 *)zb)[j >> 1]);
        if (j < mine) one_row(zb[j]);
        }
        double jr = 1.0, ji = 0.0;                  // lambda^(lim - 32)
        for (int q = 32; q < lim; ++q) {
            const double xr = fma(jr, lr, -ji * li);
            ji = fma(jr, li, ji * lr);
            jr = xr;
        }
        join(jr, ji);
        cb = r_hi;
    }
    }
    }
    if constexpr (CHUNK != 0) {
        if constexpr (CHUNK == 3) return;           // (its rows were no rows of the series)
        if constexpr (!PROVEN) { if (__ballot(viol) != 0ull && lane == 0) hdr[ST_VIOL] = 1.0; }
        double *__restrict__ slot = wsp + CH_P + ch * CH_SLOT;
        if (ch == nch - 1) {
            if (lane < 32) { hdr[ST_SR + lane] = sr; hdr[ST_SI + lane] = si; }
        } else if (CHUNK == 1 && lane < 32) {
            slot[lane] = sr;
            slot[32 + lane] = si;
        }
        if (CHUNK == 2 || ch == 0) {
            const double q = wave_sum(zsq);         // fixed order; k_steady_chunk_sum adds the chunks' in chunk order
            if (lane == 0) slot[64] = q;
        }
        return;
    }
    if (lane < 32) { hdr[ST_SR + lane] = sr; hdr[ST_SI + lane] = si; }
    if constexpr (!PROVEN) { if (__ballot(viol) != 0ull && lane == 0) hdr[ST_VIOL] = 1.0; }
    if constexpr (!STORE) {
        // d = d_inf on every tail row: sum log d = rows * log d_inf, sum z^2 / d = (sum z^2) / d_inf
        const double q = wave_sum(zsq);             // fixed order: the same bits for the same launch shape
        if (lane == 0) {
            double *__restrict__ a = acc_ + (size_t)pr * RED_NACC;
            a[0] += (double)(N - nb) * log(dinf);
            a[1] += q / dinf;
            a[2] = fmin(a[2], dinf);
        }
    }
}

template <int ROWS>
__global__ void __launch_bounds__(64, 2)
k_steady_tail(const int64_t N, const int64_t n_first, const int Jc, const double gap,
              const double *__restrict__ ac_, const double *__restrict__ bc_,
              const double *__restrict__ cc_, const double *__restrict__ dc_, const double *__restrict__ cmax_,
              const double *__restrict__ t_, const int64_t t_bs, const double *__restrict__ y_, const int64_t y_bs,
              double *__restrict__ d_, double *__restrict__ z_, const int32_t *__restrict__ info,
              double *__restrict__ steady_) {
    steady_tail_rows<ROWS, true>(N, n_first, Jc, gap, ac_, bc_, cc_, dc_, cmax_, t_, t_bs, y_, y_bs, d_, z_, info,
                                 steady_, nullptr, 0, 0);
}

// The finishing instance: the rows [switch row, N) of the WHOLE series (N rows from global row 0) of every switched
// problem in one launch behind the last tile's reduction -- one set-up per evaluation, blocks from the switch row on
// across the tiles' boundaries, no row stored; acc[b] = {sum log d, sum z^2 / d, min d} takes the tail's share.
// A launch takes the problems whose switch row lies in [sw_lo, sw_hi) and returns at once for every other one, before
// it reads or writes anything else of theirs: launches over disjoint windows that cover [1, N] finish every switched
// problem exactly once, with no flag in the buffer.  Such a launch may run BESIDE later tiles of the same evaluation
// (gf_steady_sweep + gf_reduce_tile_steady on another stream), without atomics, once the reduction of the tile that
// holds the window's last switch row is behind it (an event):
//   - it reads and writes only its own problems' header and acc[b] (and reads their t, y, coefficients and info);
//   - the sweep wave of a switched problem returns at its test of hdr[ST_SW], which nothing writes after the switch;
//   - k_reduce1<true> / k_reduce2<true> of a later tile find steady_rows_stored == 0 for such a problem and return
//     without touching `work` or acc[b] (init is set on the series' first tile only, which cannot lie behind a
//     switch): the last write of acc[b] on the sweep's stream is the reduction of the tile that holds the switch;
//   - where the sweep adds its own tile (gf_steady_sweep_reduced: no reduction behind it) that last write is the sweep
//     of the tile that holds the switch, and the event stands behind that sweep: on a later tile the wave of a switched
//     problem finds steady_rows_stored == 0 at its exit and leaves acc[b] alone, as k_reduce2<true> does;
//   - the problems that have not switched are not this launch's: it leaves at the window test above.
// PROVEN (GF_SWEEP_AXIS_PROVEN): the caller has proved both spacing tests for every tail row; t is not read, nothing
// is tested and ST_VIOL is not written.
template <int ROWS, bool PROVEN>
__global__ void __launch_bounds__(64, 2)
k_steady_finish(const int64_t N, const int Jc, const double gap,
                const double *__restrict__ ac_, const double *__restrict__ bc_,
                const double *__restrict__ cc_, const double *__restrict__ dc_, const double *__restrict__ cmax_,
                const double *__restrict__ t_, const int64_t t_bs, const double *__restrict__ y_, const int64_t y_bs,
                const int32_t *__restrict__ info, double *__restrict__ steady_, double *__restrict__ acc_,
                const int64_t sw_lo, const int64_t sw_hi) {
    steady_tail_rows<ROWS, false, 0, PROVEN>(N, 0, Jc, gap, ac_, bc_, cc_, dc_, cmax_, t_, t_bs, y_, y_bs, nullptr, nullptr,
                                             info, steady_, acc_, sw_lo, sw_hi);
}

// The chunked finishing launch: the tail of a problem of the window in chunks of chunk_rows rows, one wave per chunk,
// grid B x (the largest chunk count of a series of N rows; B x 1 for PASS = 3, the waves of M).  PASS = 3 and 1, then
// k_steady_chunk_power, then PASS = 2, then k_steady_chunk_sum, on one stream (steady_tail_rows has the scheme).
template <int ROWS, int PASS, bool PROVEN = false>
__global__ void __launch_bounds__(64, 2)
k_steady_chunk(const int64_t N, const int Jc, const double gap,
               const double *__restrict__ ac_, const double *__restrict__ bc_,
               const double *__restrict__ cc_, const double *__restrict__ dc_, const double *__restrict__ cmax_,
               const double *__restrict__ t_, const int64_t t_bs, const double *__restrict__ y_, const int64_t y_bs,
               const int32_t *__restrict__ info, double *__restrict__ steady_,
               const int64_t sw_lo, const int64_t sw_hi, const int64_t chunk_rows, double *__restrict__ ws_,
               const int64_t ws_ld) {
    steady_tail_rows<ROWS, false, PASS, PROVEN>(N, 0, Jc, gap, ac_, bc_, cc_, dc_, cmax_, t_, t_bs, y_, y_bs, nullptr,
                                                nullptr, info, steady_, nullptr, sw_lo, sw_hi, chunk_rows, ws_, ws_ld);
}

// the window's problems with at least `least` chunks: first tail row, 0 for every other problem
__device__ __forceinline__ int64_t steady_chunk_problem(const int pr, const int64_t N, const int32_t *__restrict__ info,
                                                        const double *__restrict__ steady_, const int64_t sw_lo,
                                                        const int64_t sw_hi, const int64_t chunk_rows, const int least) {
    if (info[pr] != 0) return 0;
    const double swd = steady_[(size_t)pr * ST_SIZE + ST_SW];
    if (!(swd > 0.0)) return 0;
    const int64_t sw = (int64_t)swd;
    if (sw < sw_lo || sw >= sw_hi || sw >= N) return 0;
    return (N - sw + chunk_rows - 1) / chunk_rows >= least ? sw : 0;
}

// P = M^(2^squarings) in place, one workgroup of 256 per problem: thread (i, q) holds P[i][16 q .. 16 q + 15], the
// matrix lies in LDS between two squarings.  About 11 squarings of 64 x 64 per problem: the rate does not matter.
__global__ void __launch_bounds__(256)
k_steady_chunk_power(const int64_t N, const int32_t *__restrict__ info, const double *__restrict__ steady_,
                     const int64_t sw_lo, const int64_t sw_hi, const int64_t chunk_rows, const int squarings,
                     double *__restrict__ ws_, const int64_t ws_ld) {
    const int pr = blockIdx.x;
    if (steady_chunk_problem(pr, N, info, steady_, sw_lo, sw_hi, chunk_rows, 3) == 0) return;   // (block-uniform)
    __shared__ double s_m[64][64 + 1];
    double *__restrict__ P = ws_ + (size_t)pr * ws_ld;
    const int i = threadIdx.x >> 2, c0 = 16 * (threadIdx.x & 3);
    double a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = P[64 * i + c0 + j];
    for (int q = 0; q < squarings; ++q) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) s_m[i][c0 + j] = a[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = 0.0;
#pragma unroll 4
        for (int k = 0; k < 64; ++k) {
            const double m = s_m[i][k];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = fma(m, s_m[k][c0 + j], a[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) P[64 * i + c0 + j] = a[j];
}

// the chunks' sums into acc, one thread per problem, in chunk order: the additions of the one-wave launch
__global__ void __launch_bounds__(64)
k_steady_chunk_sum(const int B, const int64_t N, const int32_t *__restrict__ info, const double *__restrict__ steady_,
                   const int64_t sw_lo, const int64_t sw_hi, const int64_t chunk_rows,
                   const double *__restrict__ ws_, const int64_t ws_ld, double *__restrict__ acc_) {
    const int pr = blockIdx.x * 64 + threadIdx.x;
    if (pr >= B) return;
    const int64_t sw = steady_chunk_problem(pr, N, info, steady_, sw_lo, sw_hi, chunk_rows, 1);
    if (sw == 0) return;
    const int nch = (int)((N - sw + chunk_rows - 1) / chunk_rows);
    const double *__restrict__ slot = ws_ + (size_t)pr * ws_ld + CH_P;
    double q = 0.0;
    for (int c = 0; c < nch; ++c) q += slot[c * CH_SLOT + 64];
    const double dinf = steady_[(size_t)pr * ST_SIZE + ST_D];
    double *__restrict__ a = acc_ + (size_t)pr * RED_NACC;
    a[0] += (double)(N - sw) * log(dinf);
    a[1] += q / dinf;
    a[2] = fmin(a[2], dinf);
}

// ------------------------------------------------------------------------------------
// k_steady_rank1: the rows IN FRONT of the steady switch in O(W) per row (gf_steady_sweep_rank1).
//
// On an axis that is regular from row 0 with a constant diagonal the recurrence, in the frame that rotates with the
// terms' phasors, is a time-invariant Riccati iteration from S_0 = 0, and S_n+1 - S_n keeps rank one (Chandrasekhar /
// Morf-Sidhu-Kailath): pivot, gain and forward solve need vectors of one entry per complex term, never the W x W
// state.  With <p, q> = sum_k Re(conj(p_k) q_k), u0 = a - i b, lambda = exp(-(c + i d) Delta), a0 = the matrix' diagonal:
//   start  r = 1, d = a0, Y = lambda r, sigma = 1 / d, f = 0;
//   row n  k = r / d ;  z_n = y_n - <u0, f> ;  f <- lambda (f + k z_n)
//          beta = <u0, Y> ;  r <- r - sigma beta Y ;  d' = d - sigma beta^2 ;  Y <- lambda (Y - beta k)
//          sigma <- sigma d / d' ;  d <- d'
// k is the derotated gain G of the switch rule and of the tail directly, f + k z the tail's state s.  No time stamp
// enters: no row generator, no block scaling (|lambda| < 1), no resets.  Delta is the cadence of the WHOLE axis (dt[b],
// from the caller): an error of the cadence is a phase error n w dDelta at row n.
// One complex term per lane, complex values in register pairs, on BOTH half-waves: lane (h, c) holds r, Y and k of
// term c, and X = f on the lower half-wave, X = Y on the upper one.  Both updates are X <- lambda (X + k m) with
// m = z_n below and m = -beta above, and both dot products are <u0, X>: one tree over the half-waves (five DPP steps)
// gives <u0, f> in lane 31 and beta in lane 63.  1 / d' is formed beside the tree of the next row: the chain from row
// to row is X -> tree -> X.
// The contract towards everything downstream is k_factor7<.., STEADY>'s: rows in front of the switch row in d and z,
// the rule on the same anchors with the same ring (real parts in the lower half-wave's slots, imaginary parts in the
// upper one's, the pivot in lane 63's: Jc <= 31, so term 31 is a pad), the same header at the switch, info, acc.
// Between tiles the state lies in the problem's S_state slot (R1_* below), which this route does not otherwise use.
// ------------------------------------------------------------------------------------
constexpr int R1_RR = 0, R1_RI = 64, R1_YR = 128, R1_YI = 192, R1_XR = 256, R1_XI = 320;   // [64] per lane
constexpr int R1_D = 384, R1_SG = 385;                                                    // d, sigma

// sums over the lower and over the upper half-wave, broadcast
__device__ __forceinline__ void half_wave_sums(double v, double &lo, double &up) {
    v += dpp_get<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v += dpp_get<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v += dpp_get<0x141, 0xf>(v);   // row_half_mirror
    v += dpp_get<0x140, 0xf>(v);   // row_mirror       -> every lane holds its 16-lane row sum
    v += dpp_get<0x142, 0xf>(v);   // row_bcast15: rows 1, 3 += total of rows 0, 2
    lo = read_lane(v, 31);
    up = read_lane(v, 63);
}

// v in the lanes of the mask, keep in the others: the mask is wave-uniform and stays in a scalar register pair (as a
// comparison of the lane number it would be a vector compare per use)
__device__ __forceinline__ double lane_select(const unsigned long long lanes, const double v, const double keep) {
    int lo = __double2loint(keep), hi = __double2hiint(keep);
    asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(lo) : "v"(__double2loint(v)), "s"(lanes));
    asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(hi) : "v"(__double2hiint(v)), "s"(lanes));
    return __hiloint2double(hi, lo);
}

constexpr int R1_UNROLL = 8;                        // plain rows per trip of the unrolled body

__global__ void __launch_bounds__(64, 2)
k_steady_rank1(const int64_t N, const int64_t n_first, const int Jc, const double gap,
               const double *__restrict__ ac_, const double *__restrict__ bc_,
               const double *__restrict__ cc_, const double *__restrict__ dc_,
               const double *__restrict__ diag_add_, const double *__restrict__ cmax_,
               const double *__restrict__ t_, const int64_t t_bs,
               const double *__restrict__ diag_, const int64_t diag_bs,
               const double *__restrict__ y_, const int64_t y_bs,
               double *__restrict__ d_, double *__restrict__ z_, double *__restrict__ S_state,
               int32_t *__restrict__ info, double *__restrict__ steady_, const int64_t arm_from,
               const double *__restrict__ dt_, double *acc_, const int acc_init) {
    const int lane = threadIdx.x, pr = blockIdx.x;
    const int h = lane >> 5, c = lane & 31;         // half-wave (0: X = f, 1: X = Y), term
    int64_t tile_lim = 0;                           // (acc_: as k_factor7's steady instance leaves, label tile_sums)
#define R1_EXIT(lim) do { if (acc_) { tile_lim = (lim); goto tile_sums; } return; } while (0)
  {
    if (info[pr] != 0) R1_EXIT(steady_rows_stored(steady_, pr, N, n_first));
    double *__restrict__ hdr = steady_ + (size_t)pr * ST_SIZE;
    if (hdr[ST_SW] > 0.0) R1_EXIT(steady_rows_stored(steady_, pr, N, n_first));
    const double *__restrict__ tg = t_ + (size_t)pr * t_bs + n_first;
    const double *__restrict__ yg = y_ + (size_t)pr * y_bs + n_first;
    double *__restrict__ dg = d_ + (size_t)pr * N;
    double *__restrict__ zg = z_ + (size_t)pr * N;
    double *__restrict__ Sg = S_state + (size_t)pr * (64 * 64);
    const bool term = c < Jc, fl = lane == 63;
    const size_t ck = (size_t)pr * Jc + (term ? c : 0);
    const double ck_c = term ? cc_[ck] : 0.0, ck_d = term ? dc_[ck] : 0.0;
    const double ck_a = term ? ac_[ck] : 0.0, ck_b = term ? bc_[ck] : 0.0;
    const double wmax = wave_max(fmax(ck_c, fabs(ck_d)));
    const double gthr = gap / cmax_[pr], jthr = 2e-6 / wmax;        // the tail's thresholds (RowGen::init's)
    const double delta = dt_[pr];
    double lr, li;                                  // lambda, as the tail's set-up forms it
    {
        double sn, cs;
        fm_sincos(ck_d * delta, &sn, &cs);
        const double e = fm_exp(-ck_c * delta);
        lr = e * cs;
        li = -e * sn;
    }
    double rr, ri, Yr, Yi, Xr, Xi, d, sg;
    if (n_first == 0) {                             // from the coefficients (pad terms: r = Y = 0 for good)
        d = (diag_ ? diag_[(size_t)pr * diag_bs] : 0.0) + diag_add_[pr];     // a0 (diag_add holds the sum of the a_k)
        sg = fast_rcp(d);
        rr = term ? 1.0 : 0.0;
        ri = 0.0;
        Yr = term ? lr : 0.0;
        Yi = term ? li : 0.0;
        Xr = h ? Yr : 0.0;
        Xi = h ? Yi : 0.0;
    } else {
        rr = Sg[R1_RR + lane]; ri = Sg[R1_RI + lane];
        Yr = Sg[R1_YR + lane]; Yi = Sg[R1_YI + lane];
        Xr = Sg[R1_XR + lane]; Xi = Sg[R1_XI + lane];
        d = Sg[R1_D]; sg = Sg[R1_SG];
    }
    constexpr double thr = ST_THR;
    int cnt = __builtin_amdgcn_readfirstlane((int)hdr[ST_CNT]);
    int fill = __builtin_amdgcn_readfirstlane((int)hdr[ST_FILL]);
    int32_t fail = 0;
    double inv = fast_rcp(d);
    double kr = rr * inv, ki = ri * inv;
    const int64_t last = N - 1;
    // The rows in blocks of 64 (local: a tile may start anywhere): t, its predecessor and y of the rows nb + lane come
    // by one lane-parallel load each, a block ahead; the row takes its y by readlane, and the block's 64 spacings are
    // tested at once, as the tail tests them (global row 0 has none).  Nothing a row waits for is loaded in the row.
    auto row_of = [&](const int64_t cb) { const int64_t i = cb + lane; return i < last ? i : last; };
    double t_nx, tp_nx, y_nx;
    {
        const int64_t i = row_of(0);
        t_nx = tg[i];
        tp_nx = (n_first + i > 0) ? tg[i - 1] : t_nx - delta;
        y_nx = yg[i];
    }
    // A block's d and z are staged in two registers, row j's in lane j, and leave by one lane-parallel store each where
    // the block ends: at its last row, at the switch row, in front of the first row whose pivot is not positive.  The
    // pivots are tested there and at the anchor, on the staged lanes at once: the recursion may run up to 63 rows past
    // a failed pivot (nothing traps, nothing of those rows is stored), but no anchor is taken behind one.
    double sd = 0.0, sz = 0.0, sr, si, beta, yv_blk = 0.0;
    auto row_front = [&](const int j) __attribute__((always_inline)) {             // pivot and residual of block row j, and s = X + k m
        const double yy = read_lane(yv_blk, j);
        double sf;
        half_wave_sums(fma(ck_a, Xr, -(ck_b * Xi)), sf, beta);          // Re((a + i b) X): <u0, f> below, <u0, Y> above
        const double zn = yy - sf;
        const unsigned long long row_lane = 1ull << j;
        sd = lane_select(row_lane, d, sd);
        sz = lane_select(row_lane, zn, sz);
        const double m = h ? -beta : zn;
        sr = fma(kr, m, Xr), si = fma(ki, m, Xi);   // below: s = f + k z, the tail's state
    };
    auto row_back = [&]() __attribute__((always_inline)) {
        Xr = fma(lr, sr, -(li * si));
        Xi = fma(lr, si, li * sr);
        const double sb = sg * beta;
        rr = fma(-sb, Yr, rr);
        ri = fma(-sb, Yi, ri);
        const double dn = fma(-sb, beta, d);
        const double wr = fma(-beta, kr, Yr), wi = fma(-beta, ki, Yi);          // (k: the old gain)
        Yr = fma(lr, wr, -(li * wi));
        Yi = fma(lr, wi, li * wr);
        inv = fast_rcp(dn);
        sg = sg * d * inv;
        d = dn;
        kr = rr * inv;
        ki = ri * inv;
    };
    auto plain_rows = [&](int j, const int j1) __attribute__((always_inline)) {    // rows without an anchor: no test, no store, no exit
        for (; j + R1_UNROLL <= j1; j += R1_UNROLL) {
#pragma unroll
            for (int u = 0; u < R1_UNROLL; ++u) {
                row_front(j + u);
                row_back();
            }
        }
#pragma unroll 1
        for (; j < j1; ++j) {
            row_front(j);
            row_back();
        }
    };
    // the first of the staged rows [0, rows) whose pivot is not positive, -1: none
    auto first_failed = [&](const int rows) __attribute__((always_inline)) {
        const unsigned long long staged = rows < 64 ? (1ull << rows) - 1 : ~0ull;
        const unsigned long long bad = __ballot(!(sd > 0.0)) & staged;
        return bad ? (int)__ffsll((long long)bad) - 1 : -1;
    };
    auto flush = [&](const int64_t nb, const int rows) __attribute__((always_inline)) {
        if (lane < rows) { dg[nb + lane] = sd; zg[nb + lane] = sz; }
    };
    const int g0lo = (int)(n_first & (ST_GRID - 1));
    const int ja = (ST_GRID - g0lo) & (ST_GRID - 1);        // the anchor's row in every block of this tile
    __builtin_amdgcn_s_setprio(GF_CHAIN_PRIO);
    for (int64_t nb = 0; nb < N; nb += 64) {
        const int lim = (int)(N - nb < 64 ? N - nb : 64);
        yv_blk = y_nx;
        // the block's y has arrived HERE: left to the rows, its first use puts a vector-memory wait into every row,
        // and that counter holds the blocks' stores of d and z too
        asm volatile("" : "+v"(yv_blk));
        {
            const double dt = t_nx - tp_nx;
            const bool bad = (dt > gthr) || !(fabs(dt - delta) < jthr);
            if (__any(bad) && lane == 0) hdr[ST_VIOL] = 1.0;
            const int64_t i = row_of(nb + 64);
            t_nx = tg[i];
            tp_nx = (n_first + i > 0) ? tg[i - 1] : t_nx - delta;
            y_nx = yg[i];
        }
        int jf;                                     // the block's first failed row
        if (ja < lim) {
            plain_rows(0, ja);
            row_front(ja);
            jf = first_failed(ja + 1);              // (in front of the ring, ST_CNT, ST_FILL and the header)
            if (jf < 0) {
                const int64_t n = nb + ja, gn = n_first + n;
                if (gn >= arm_from) {
                    // an anchor of the rule: k_factor7's test on the same ring
                    const double x = fl ? d : (h ? ki : kr);
                    double *__restrict__ slot = hdr + ST_RING + (size_t)((gn / ST_GRID) & (ST_LAG - 1)) * 64 + lane;
                    const double xo = *slot;
                    *slot = x;
                    const double dx = fl ? 0.0 : fabs(x - xo);
                    const double mdx = wave_max(dx), mx = wave_max(fl ? 0.0 : fabs(x));
                    const double dold = read_lane(xo, 63);
                    const bool ok = fill >= ST_LAG && mdx <= thr * mx && fabs(d - dold) <= thr * d;
                    cnt = ok ? cnt + 1 : 0;
                    fill = fill < ST_LAG ? fill + 1 : fill;
                    if (lane == 0) { hdr[ST_CNT] = (double)cnt; hdr[ST_FILL] = (double)fill; }
                    if (cnt >= ST_COUNT && gn >= ST_DLAG) { // the switch: what k_steady_finish and k_steady_tail start from
                        if (h == 0) {
                            hdr[ST_GR + c] = kr;
                            hdr[ST_GI + c] = ki;
                            hdr[ST_SR + c] = sr;
                            hdr[ST_SI + c] = si;
                        }
                        if (lane == 0) {
                            hdr[ST_SW] = (double)(gn + 1);
                            hdr[ST_D] = d;
                            hdr[ST_DT] = (tg[n] - tg[n - ST_DLAG]) * (1.0 / ST_DLAG);     // (gn >= 1024)
                        }
                        flush(nb, ja + 1);
                        R1_EXIT(n + 1);             // (row n + 1 is the tail's first; rows 0 .. n were stored)
                    }
                }
                row_back();
                plain_rows(ja + 1, lim);
                jf = first_failed(lim);
            }
        } else {                                    // the tile's last block ends in front of its anchor
            plain_rows(0, lim);
            jf = first_failed(lim);
        }
        if (jf >= 0) {                              // the failed row and the rows behind it are not stored
            flush(nb, jf);
            const int64_t gf = n_first + nb + jf + 1;
            fail = (int32_t)(gf > 0x7fffffff ? 0x7fffffff : gf);
            break;
        }
        flush(nb, lim);
    }
    if (fail) {
        if (lane == 0) info[pr] = fail;
        R1_EXIT(N);                                 // (not switched: the reduction takes the tile's N rows, stale ones too)
    }
    Sg[R1_RR + lane] = rr; Sg[R1_RI + lane] = ri;
    Sg[R1_YR + lane] = Yr; Sg[R1_YI + lane] = Yi;
    Sg[R1_XR + lane] = Xr; Sg[R1_XI + lane] = Xi;
    if (lane == 0) { Sg[R1_D] = d; Sg[R1_SG] = sg; }
    R1_EXIT(N);                                     // the end of the tile, not switched: all its rows
  }
#undef R1_EXIT
tile_sums:
    // as k_factor7's steady instance: the blocks' stores of d and z ordered before the wave's loads of them
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    steady_tile_sums(d_ + (size_t)pr * N, z_ + (size_t)pr * N, N, tile_lim, acc_ + (size_t)pr * RED_NACC, acc_init, lane);
}

// ------------------------------------------------------------------------------------
// Closed-loop transition sweeps of the time-parallel evaluation, W <= 63 (k_phi7: k_factor7's lane tiling,
// complex terms only; k_phi: one column per lane, any terms), DESIGN.md 4.3:
//     Phi <- (I - w~ u~^T) Phi  (E Phi at reset rows),  h_n = Phi^T u~_n,
//     G = sum_n h_n h_n^T / dbar_n,   m = sum_n h_n zbar_n / dbar_n
// on the rows the nominal pass stored (u~, r-bar, dbar, zbar, reset spans): no row generator here, and the
// Gram sums are accumulated in the same kernel -- the rows h never leave the chip.
//   * rows arrive through an LDS ring filled by LDS-DMA five rows ahead of their use (PhiRing); a register
//     queue two rows deep left every row waiting on HBM once the row arrays outgrew the caches (cfg3: 8.5 GB);
//   * sixteen rows of h are collected in an LDS tile and folded into the G accumulators as a rank-16
//     update on v_mfma_f64_16x16x4 (PhiGram: NT (NT + 1) / 2 symmetric tiles of 16 x 16, NT = ceil(W / 16)).
// ------------------------------------------------------------------------------------
struct PhiRing {
    static constexpr int PD = 8;                    // slots; rows are fetched PD - 1 ahead, used PD - 3 later
    static constexpr int USL = 72, RSL = 64;        // doubles per slot: u~ row + 3 scalar pairs / r-bar row
    static constexpr int OD = 64, OE = 66, OZ = 68; // dbar / reset span / zbar pair of the row in its u~ slot
    double u[PD][USL];
    double r[PD + 1][RSL];                          // slot PD: zeros ("no pending update" of the first row)
};

// per-lane copy cursors: lanes 0 .. 31 the row's doubles 2 lane, 2 lane + 1; lanes 32 / 33 / 34 of the u~
// copy the aligned pairs that hold dbar[row] / de[row] / zbar[row]; the other lanes stay out (EXEC)
struct PhiCursor {
    uintptr_t cu, cr, mask;
    unsigned long long ustep;
    bool in_u, in_r;
    unsigned lds_u, lds_r;
    // `rows`: the sweep's state rows (ROWS >= W): the copies fetch the row's first `rows` doubles only -- with the
    // nominal pass storing no more than that (see its row stores) the padding of the 64-double rows never travels
    template <int rows = 64>
    __device__ __forceinline__ void init(PhiRing &R, const int lane, const size_t pb, const double *ut_,
                                         const double *rbar_, const double *dbar_, const double *de_,
                                         const double *zbar_) {
        cu = reinterpret_cast<uintptr_t>(ut_ + pb * 64 + 2 * (lane & 31));
        cr = reinterpret_cast<uintptr_t>(rbar_ + pb * 64 + 2 * (lane & 31));
        mask = ~(uintptr_t)0;
        ustep = 64 * 8;
        if (lane >= 32) {
            const double *sp = (lane == 32) ? dbar_ : (lane == 33) ? de_ : zbar_;
            cu = reinterpret_cast<uintptr_t>(sp + pb);
            mask = ~(uintptr_t)15;
            ustep = 8;
        }
        in_u = lane < (rows + 1) / 2 || (lane >= 32 && lane < 35);
        in_r = lane < (rows + 1) / 2;
        lds_u = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(&R.u[0][0]));
        lds_r = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(&R.r[0][0]));
    }
    // row m (the cursors stand at it) -> slot m mod PD; two vector-memory operations
    __device__ __forceinline__ void issue(const int64_t m, const int after) {
        const unsigned sl = (unsigned)(m & (PhiRing::PD - 1));
        if (in_u) glds16(reinterpret_cast<const void *>(cu & mask), lds_u + sl * (PhiRing::USL * 8), after);
        if (in_r) glds16(reinterpret_cast<const void *>(cr), lds_r + sl * (PhiRing::RSL * 8), after);
        cu += ustep;
        cr += 64 * 8;
    }
};

template <int NT>
struct PhiGram {
    static constexpr int LD = 80;                   // tile row stride: rows k, k + 1 land 32 banks apart
    static constexpr int NACC = NT * (NT + 1) / 2;
    double hs[16][LD];                              // h of sixteen rows
    double sv[16];                                  // 1 / dbar of those rows (0: row not there)
};

// fold the tile into the accumulators: acc(it, jt) += sum_k (h_k[16 it + i] / d_k) h_k[16 jt + j]
template <int NT>
__device__ __forceinline__ void phi_gram_flush(PhiGram<NT> &Gm, d4 (&acc)[PhiGram<NT>::NACC], const int lane) {
    const int li = lane & 15, lk = lane >> 4;
    wave_lds_fence();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const int k = 4 * ks + lk;
        const double sc = Gm.sv[k];
        double hv[NT];
#pragma unroll
        for (int it = 0; it < NT; ++it) hv[it] = Gm.hs[k][16 * it + li];
        int t = 0;
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
            for (int jt = it; jt < NT; ++jt, ++t) acc[t] = GF_MFMA64(hv[it] * sc, hv[jt], acc[t]);
    }
    wave_lds_fence();
    if (lane < 16) Gm.sv[lane] = 0.0;               // (a partial last block folds zeros for the missing rows)
}

// G ([column][row], 64 x 64, zero outside the tiles) and m of one chunk
template <int NT>
__device__ __forceinline__ void phi_gram_store(const d4 (&acc)[PhiGram<NT>::NACC], const double macc,
                                               double *__restrict__ Gg, double *__restrict__ mg, const int lane,
                                               const int own) {
    const int li = lane & 15, lk = lane >> 4;
    for (int e = lane; e < 4096; e += 64) {
        const int col = e >> 6, row = e & 63;
        if (col >= 16 * NT || row >= 16 * NT) Gg[e] = 0.0;
    }
    int t = 0;
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int jt = it; jt < NT; ++jt, ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * it + lk + 4 * r, col = 16 * jt + li;
                const double v = acc[t][r];
                if (jt > it || col >= row) {        // upper triangle, mirrored: exactly symmetric
                    Gg[(size_t)col * 64 + row] = v;
                    Gg[(size_t)row * 64 + col] = v;
                }
            }
    mg[own] = macc;
}

template <int ROWS>
__global__ void __launch_bounds__(64, 2)
k_phi7(const int64_t N, const int64_t chunk_len, const int nch, const int ch0, const int nsel, const int W,
       const double *__restrict__ c_, const double *__restrict__ de_, const double *__restrict__ dbar_,
       const double *__restrict__ zbar_, const double *__restrict__ rbar_, const double *__restrict__ ut_,
       double *__restrict__ Phi_out, double *__restrict__ G_out, double *__restrict__ m_out) {
    constexpr int NT = (ROWS + 15) / 16, PD = PhiRing::PD;
    const int lane = threadIdx.x;
    const int g = lane >> 5, c = lane & 31, own = 2 * c + g;    // k_factor7's tiling: state columns 2c, 2c + 1
    const int sel = blockIdx.x;                                 // of half the rows; row vectors: column `own`
    const int pr = sel / nsel, ch = ch0 + (sel - pr * nsel);    // chunks ch0 .. ch0 + nsel - 1 of every problem
    const int b = pr * nch + ch;                                // state slot
    const int64_t c0 = (int64_t)ch * chunk_len;
    const int64_t rows = (N - c0 < chunk_len) ? (N - c0) : chunk_len;
    const size_t pb = (size_t)pr * N + c0;
    double *__restrict__ col0 = Phi_out + (size_t)b * (64 * 64) + (size_t)(2 * c) * 64 + 2 * g;
    double *__restrict__ col1 = col0 + 64;
    const double cj = (own < W) ? c_[(size_t)pr * W + own] : 0.0;

    __shared__ __attribute__((aligned(16))) PhiRing R;
    __shared__ __attribute__((aligned(16))) PhiGram<NT> Gm;
    __shared__ __attribute__((aligned(16))) double s_e[64];
    const double2 *pe = (const double2 *)s_e + g;
    double T[ROWS / 2][2];
#pragma unroll
    for (int m = 0; m < ROWS / 2; ++m) {                        // Phi = I
        const int row = 4 * (m >> 1) + 2 * g + (m & 1);
        T[m][0] = (row == 2 * c) ? 1.0 : 0.0;
        T[m][1] = (row == 2 * c + 1) ? 1.0 : 0.0;
    }
    double q0 = 0.0, q1 = 0.0, macc = 0.0;
    d4 acc[PhiGram<NT>::NACC];
#pragma unroll
    for (int t = 0; t < PhiGram<NT>::NACC; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    R.r[PD][lane] = 0.0;
    for (int e = lane; e < 16 * PhiGram<NT>::LD; e += 64) (&Gm.hs[0][0])[e] = 0.0;
    if (lane < 16) Gm.sv[lane] = 0.0;
    PhiCursor C;
    C.template init<ROWS>(R, lane, pb, ut_, rbar_, dbar_, de_, zbar_);
#pragma unroll
    for (int m = 0; m < PD - 1; ++m) C.issue(m, 0);
    vm_wait<2 * (PD - 2)>();                        // row 0 has landed
    wave_lds_fence();
    double2 ub[S7_AHEAD + 1], wb[S7_AHEAD + 1];
    const double2 *pu = (const double2 *)&R.u[0][0] + g;
    const double2 *pw = (const double2 *)&R.r[PD][0] + g;
    sweep7_preload<ROWS>(ub, wb, pu, pw);

    for (int64_t n = 0; n < rows; ++n) {
        // rows up to n + 1 have landed: behind row n + 1's copies are those of the PD - 3 rows after it
        vm_wait<2 * (PD - 3)>();
        const int sl = (int)(n & (PD - 1)), par = (int)((pb + n) & 1);
        const double dcur = R.u[sl][PhiRing::OD + par], zcur = R.u[sl][PhiRing::OZ + par];
        const double dev = R.u[sl][PhiRing::OE + par];
        const double de = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(dev)),
                                           __builtin_amdgcn_readfirstlane(__double2loint(dev)));
        if (de >= 0.0) {                    // reset row: Phi <- E (Phi + pending): row scaling only
            s_e[own] = fm_exp_local(-cj * de);
            wave_lds_fence();
            double d0, d1;
            sweep7_preload<ROWS>(ub, wb, pe, pw);
            sweep7_run<ROWS, true>(T, ub, wb, pe, pw, q0, q1, 1.0, 1.0, d0, d1);
            sweep7_preload<ROWS>(ub, wb, pu, pw);
            q0 = 0.0;
            q1 = 0.0;
        }
        double acc0, acc1;
        sweep7_run<ROWS, false>(T, ub, wb, pu, pw, q0, q1, 0.0, 0.0, acc0, acc1);
        const double h = own_column_sum(acc0, acc1);
        const double rinv = (dcur > 0.0) ? fast_rcp(dcur) : 0.0;
        Gm.hs[n & 15][own] = h;
        if (lane == 0) Gm.sv[n & 15] = rinv;
        macc = fma(h, zcur * rinv, macc);
        // next row's operands: u~ of row n + 1 (landed), the pending r-bar of row n in its ring slot
        pu = (const double2 *)&R.u[(int)((n + 1) & (PD - 1))][0] + g;
        pw = (const double2 *)&R.r[sl][0] + g;
        sweep7_preload<ROWS>(ub, wb, pu, pw);
        both_halves(-h * rinv, q0, q1);     // pending: Phi_i -= (r_i / d) h_j
        // row n + PD - 1 into the slot of row n - 1, whose rows this iteration's sweeps were the last to read
        C.issue(n + PD - 1, __double2loint(h));
        if ((n & 15) == 15) phi_gram_flush<NT>(Gm, acc, lane);
    }
    vm_wait<0>();                           // no copy may outlive the wave's LDS allocation
    if (rows & 15) phi_gram_flush<NT>(Gm, acc, lane);
    wave_lds_fence();
    const double *s_w = &R.r[(int)((rows - 1) & (PD - 1))][0];
#pragma unroll
    for (int m = 0; m < ROWS / 2; ++m) {
        const int ro = 4 * (m >> 1) + (m & 1);
        const double w = s_w[2 * g + ro];
        col0[ro] = fma(w, q0, T[m][0]);
        col1[ro] = fma(w, q1, T[m][1]);
    }
#pragma unroll
    for (int k2 = ROWS / 4; k2 < 16; ++k2) {                    // rows past ROWS: zero
        col0[4 * k2] = 0.0; col0[4 * k2 + 1] = 0.0;
        col1[4 * k2] = 0.0; col1[4 * k2 + 1] = 0.0;
    }
    phi_gram_store<NT>(acc, macc, G_out + (size_t)b * (64 * 64), m_out + (size_t)b * 64, lane, own);
}

// ------------------------------------------------------------------------------------
// k_factorw: the fused sweep (build + factor + forward solve, nothing materialised) for WIDE kernels,
// 64 <= W <= 176, complex terms only (Jr = 0): cfg4's W = 80, the 86-term solar kernel's W = 172.
//
// One workgroup of NW sweep waves + ONE generator wave per (problem, chunk).
// Sweep waves: the state columns are split over the waves and, inside a wave, tiled as in k_factor7 but
// four ways: lane = (g, c) = (lane >> 4, lane & 15) of wave w holds the column pair cb = 16 w + c
// (columns 2cb, 2cb + 1: the cos and sin columns of complex term cb) of the row pairs 8k + 2g,
// 8k + 2g + 1: a ds_read_b128 delivers a different operand pair to each 16-lane row group of the wave and
// feeds 8 FMAs.  EVERY wave holds all rows of its 32 columns, so the mat-vec needs no cross-wave
// reduction: the four row groups of a wave are folded with one v_permlane32_swap pair (reduce-scatter:
// lower half <- column 2cb, upper half <- column 2cb + 1) and one v_permlane16_swap pair -- 6 vector
// instructions.  Lane (g, c) then owns column own = 2cb + (lane >> 5) of the row vectors.
// Generator wave: lane l carries the phasors of complex terms l and l + 64 (k_factor3's RowGen) and
// writes row n + 1's u~, v~ (and, for a reset row, its span and the column decays) to LDS while the sweep
// waves work on row n.  A sweep wave therefore holds nothing but its state, the operand ring and a few
// scalars -- which is what lets W = 176 (T = 176 VGPRs per lane) fit the register file: with the
// generator inside the sweep waves (as in k_factor7) the state of W > 112 spilled.
// What crosses waves, through LDS and ONE workgroup barrier per row: the new r (every wave's next sweep
// needs all of it as row operands), the next row's u~ / v~, and the per-wave partial of u~ . tmp (the
// pivot) -- double-buffered by row parity.  The forward solve rides in the last padded column
// (FCOL = 32 NW - 1) exactly as in k_factor3 / k_factor7.
// Replaces k_build2 + k_factor2w (materialised u~, v~ rows: 2 x 8 ld bytes per row and evaluation
// through HBM, and a sweep that waited on them) on the log-likelihood path.
// ------------------------------------------------------------------------------------
struct FactorWArgs {            // the scalars; the arrays are separate __restrict__ kernel parameters
    int64_t N, n_first, chunk_len, t_bs, diag_bs, y_bs;
    int nch, ch0, nsel, Jc, block_sub;
    double gap;
};

struct FactorWPtrs {
    const double *ac, *bc, *cc, *dc, *diag_add, *cmax, *t, *diag, *y;
    double *d, *z, *r_out, *Ut_out, *Wt_out, *de_out, *S_state;
    int32_t *info;
};

// folds the four 16-lane row groups of a wave: a, b = this lane's partial sums of columns 2cb, 2cb + 1;
// returns the full sum of the lane's OWN column (lanes 0..31: column 2cb, lanes 32..63: 2cb + 1)
__device__ __forceinline__ double own_column_sum4(const double a, const double b) {
    const double h = own_column_sum(a, b);          // lanes l, l ^ 32 folded (reduce-scatter over the halves)
    const auto l = __builtin_amdgcn_permlane16_swap(__double2loint(h), __double2loint(h), false, false);
    const auto u = __builtin_amdgcn_permlane16_swap(__double2hiint(h), __double2hiint(h), false, false);
    return __hiloint2double(u[0], l[0]) + __hiloint2double(u[1], l[1]);         // l, l ^ 16
}

#ifndef GF_WIDE_AHEAD
#define GF_WIDE_AHEAD 1
#endif
// T[2k + s][e] is row 2G k + 2g + s, column 2cb + e (G = row groups per wave: 4 in k_factorw, 8 in
// k_phiw).  pu / pw point at this row group's first row pair.
//   RESET = false:  T += w q^T ;  acc += u^T T         (update + mat-vec)
//   RESET = true :  T  = (T + w q^T) * (e_row el_col)  (fold pending, decay; pu = the row decays)
template <int TR, bool RESET, int G = 4>
__device__ __forceinline__ void sweepw_run(double (&T)[TR][2], const double2 *pu, const double2 *pw,
                                           const double q0, const double q1, const double el0,
                                           const double el1, double &o0, double &o1) {
    constexpr int NK = TR / 2;
    // operand ring: AH row pairs of LDS look-ahead (one batch = 8 FMAs = ~35 cycles of issue covers
    // nothing of the LDS latency when the partner wave is not issuing; the state of a wide kernel leaves
    // room for a deeper ring only while TR is small)
    constexpr int AH = (GF_WIDE_AHEAD < NK) ? GF_WIDE_AHEAD : NK;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    double2 ub[AH + 1], wb[AH + 1];
#pragma unroll
    for (int k = 0; k < AH; ++k) { ub[k] = pu[G * k]; wb[k] = pw[G * k]; }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (k + AH < NK) { ub[(k + AH) % (AH + 1)] = pu[G * (k + AH)]; wb[(k + AH) % (AH + 1)] = pw[G * (k + AH)]; }
        __builtin_amdgcn_sched_barrier(0);
        const double2 u = ub[k % (AH + 1)], w = wb[k % (AH + 1)];
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

// LDS of one k_factorw workgroup.  The generator runs TWO rows ahead of the sweep (three buffers for
// what it writes), so that everything a sweep wave needs of row n + 1 except the new r is readable before
// row n's barrier; r and the pivot partials alternate between two buffers.
template <int NW>
struct WideShared {
    static constexpr int CP = 32 * NW;
    double w[2][CP];            // r_{n-1}: pending rank-1 update (row form)
    double u[3][CP];            // u~_n
    double v[3][CP];            // v~_n
    double e[3][CP];            // column decays of a reset row
    double f[3][4];             // per row: reset span de (>= 0, or -1 for a plain row), diagonal a_n, y_n
    double p[2][NW][2];         // per-wave partials: u~^T T u~ share, u~ . F~
};

// the update + mat-vec sweep with the w operands (the new r: the only operands behind the row's barrier)
// already in registers -- fetched right after the barrier, in the shadow of the pivot -- and the u~
// operands (readable long before) through a two-deep LDS ring: the FMAs never wait on the critical path
template <int TR>
__device__ __forceinline__ void sweepw_regs(double (&T)[TR][2], const double2 *pu,
                                            const double2 (&wb)[TR / 2], const double q0, const double q1,
                                            double &o0, double &o1) {
    constexpr int NK = TR / 2, AH = (NK > 2) ? 2 : NK;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    double2 ub[AH + 1];
#pragma unroll
    for (int k = 0; k < AH; ++k) ub[k] = pu[4 * k];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (k + AH < NK) ub[(k + AH) % (AH + 1)] = pu[4 * (k + AH)];
        __builtin_amdgcn_sched_barrier(0);
        const double2 u = ub[k % (AH + 1)], w = wb[k];
        T[2 * k][0] = fma(w.x, q0, T[2 * k][0]);
        T[2 * k][1] = fma(w.x, q1, T[2 * k][1]);
        T[2 * k + 1][0] = fma(w.y, q0, T[2 * k + 1][0]);
        T[2 * k + 1][1] = fma(w.y, q1, T[2 * k + 1][1]);
        a00 = fma(u.x, T[2 * k][0], a00);
        a01 = fma(u.x, T[2 * k][1], a01);
        a10 = fma(u.y, T[2 * k + 1][0], a10);
        a11 = fma(u.y, T[2 * k + 1][1], a11);
        asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11));
        __builtin_amdgcn_sched_barrier(0);
    }
    o0 = a00 + a10;
    o1 = a01 + a11;
}

// rows between looks at the failure flag (a non-positive pivot is recorded without a branch; the rows
// swept after it, at most this many, are thrown away)
constexpr int WIDE_FAIL_CHECK = 64;

// (The arrays are passed as separate __restrict__ parameters, not inside FactorWArgs: only then can
// hipcc prove the wave-uniform t loads unclobbered and issue them as scalar loads.)
// SAMPLE = true: the sampling sweep, column FCOL carries the draw (see k_factor3); y_ = eps, z_ = the draw by
// global row (y's batch stride).  The sweep waves hold nothing more than in the log-likelihood: sqrt(d_n) is
// formed where z_n was.
template <int TR, int NW, bool SAMPLE = false>
__global__ void __launch_bounds__(64 * (NW + 1), 2)
k_factorw(const FactorWArgs A,
          const double *__restrict__ ac_, const double *__restrict__ bc_,
          const double *__restrict__ cc_, const double *__restrict__ dc_,
          const double *__restrict__ diag_add_, const double *__restrict__ cmax_,
          const double *__restrict__ t_, const double *__restrict__ diag_,
          const double *__restrict__ y_,
          double *__restrict__ d_, double *__restrict__ z_, double *__restrict__ r_out,
          double *__restrict__ Ut_out, double *__restrict__ Wt_out, double *__restrict__ de_out,
          double *__restrict__ S_state, int32_t *__restrict__ info) {
    static_assert(TR % 2 == 0, "rows per lane come in pairs");
    constexpr int RP = 4 * TR;                      // rows, padded (rows >= W: u~ = r = 0, T stays 0)
    constexpr int CP = 32 * NW;                     // columns, padded; the last one carries the forward solve
    static_assert(RP <= CP, "row operands are read from the column-indexed LDS vectors");
    constexpr int FCOL = CP - 1;                    // forward-solve column: last sweep wave, lanes 47 and 63
    constexpr int NK = TR / 2;
    constexpr bool PRE = TR <= 20;                  // the w operands of a whole row fit in registers (W <= 80)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sel = blockIdx.x;                     // chunks ch0 .. ch0 + nsel - 1 of every problem
    const int pr = sel / A.nsel, ch = A.ch0 + (sel - pr * A.nsel);
    const int b = pr * A.nch + ch;                  // state slot = problem * nch + chunk
    if (info[b] != 0) return;                       // (uniform over the workgroup)
    const int64_t c0 = (int64_t)ch * A.chunk_len;
    const int64_t rows = (A.N - c0 < A.chunk_len) ? (A.N - c0) : A.chunk_len;
    const int64_t g0 = A.n_first + c0;
    const size_t pb = (size_t)pr * A.N + c0;
    const double *__restrict__ tg = t_ + (size_t)pr * A.t_bs + g0;

    __shared__ __attribute__((aligned(16))) WideShared<NW> sh;

    if (wave == NW) {
        // ------- generator wave: rows u~, v~, reset spans and decays two rows ahead; the pivots -------
        const double *__restrict__ yg = y_ + (size_t)pr * A.y_bs + g0;
        const bool has_g = diag_ != nullptr;
        const double *__restrict__ gg = has_g ? diag_ + (size_t)pr * A.diag_bs + g0 : yg;
        const double diag_add = diag_add_[pr];
        double *__restrict__ dg = d_ + pb;
        double *__restrict__ zg = SAMPLE ? z_ + (size_t)pr * A.y_bs + g0 : z_ + pb;
        constexpr int NP = (CP / 2 + 63) / 64;      // phasors per lane (1 up to W + 1 <= 128 columns, else 2)
        RowGen gen[NP];
        bool live[NP];
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            const int ph = lane + 64 * h;           // complex term (column pair) of this slot
            live[h] = ph < CP / 2;
            gen[h].init(2 * ph, pr, 0, A.Jc, A.block_sub, A.gap, nullptr, nullptr, ac_, bc_, cc_, dc_,
                        cmax_, tg, g0);
        }
        double *__restrict__ ug = Ut_out ? Ut_out + pb * CP : nullptr;
        double *__restrict__ eg = de_out ? de_out + pb : nullptr;
        auto emit = [&](const double tn, const int64_t gi, const int buf, double *urow, const double an,
                        const double yn) {
            bool rst = false;
            double de = -1.0;
#pragma unroll
            for (int h = 0; h < NP; ++h) {
                gen[h].advance(tn, gi, rst, de);            // rst, de: the same for every phasor
                const double uc = fma(gen[h].k1, gen[h].cu, gen[h].k2 * gen[h].su);        // a cos + b sin
                const double us = fma(gen[h].k1, gen[h].su, -gen[h].k2 * gen[h].cu);       // a sin - b cos
                const double vc = gen[h].sel_c * gen[h].cu * gen[h].irho2;                 // pad pairs: 0
                const double vs = gen[h].sel_c * gen[h].su * gen[h].irho2;
                if (live[h]) {
                    const int j = 2 * (lane + 64 * h);
                    *reinterpret_cast<double2 *>(&sh.u[buf][j]) = double2{uc, us};
                    *reinterpret_cast<double2 *>(&sh.v[buf][j]) = double2{vc, vs};
                    if (rst) {
                        const double el = fm_exp(-gen[h].cj * de);      // pad pairs: cj = 0 -> 1
                        *reinterpret_cast<double2 *>(&sh.e[buf][j]) = double2{el, el};
                    }
                    if (urow) *reinterpret_cast<double2 *>(urow + j) = double2{uc, us};
                }
            }
            const double span = rst ? de : -1.0;
            // the row's scalars for the sweep waves (every lane writes the same values: no branch)
            *reinterpret_cast<double2 *>(&sh.f[buf][0]) = double2{span, an};
            sh.f[buf][2] = yn;
            return span;
        };
        // y, diag in the vector-load queue (opaque zero lane offset), three rows ahead: as scalar loads
        // they share the LDS counter, and every LDS wait of the row would wait for them as well
        const int vz = __builtin_amdgcn_mbcnt_lo(0u, 0u);
        auto diag_of = [&](const double gv) { return (has_g ? gv : 0.0) + diag_add; };
        // (t, y, diag) of rows n + 2 and n + 3; rows n, n + 1 keep (a, y) for the pivots
        double t_2 = tg[2 + vz], t_3 = tg[3 + vz], y_2 = yg[2 + vz], y_3 = yg[3 + vz];
        double g_2 = gg[2 + vz], g_3 = gg[3 + vz];
        double a_0 = diag_of(gg[vz]), a_1 = diag_of(gg[1 + vz]), y_0 = yg[vz], y_1 = yg[1 + vz];
        double de_0 = emit(tg[vz], g0, 0, ug, a_0, y_0);
        double de_1 = emit(tg[1 + vz], g0 + 1, 1, (ug && rows > 1) ? ug + CP : nullptr, a_1, y_1);
        wg_lds_barrier();
        int b2 = 2;                                 // buffer of row n + 2
        int32_t fail = 0;
        double dacc = 0.0, zacc = 0.0;
        for (int64_t n = 0; n < rows; ++n) {
            const int nxt = (int)(n & 1) ^ 1;
            const double a_n = a_0, yy = y_0;
            if (eg && lane == 0) eg[n] = de_0;
            const double a_2 = diag_of(g_2);
            de_0 = de_1;
            de_1 = emit(t_2, g0 + n + 2, b2, (ug && n + 2 < rows) ? ug + (size_t)(n + 2) * CP : nullptr, a_2, y_2);
            b2 = (b2 == 2) ? 0 : b2 + 1;
            a_0 = a_1; y_0 = y_1; a_1 = a_2; y_1 = y_2;
            t_2 = t_3; y_2 = y_3; g_2 = g_3;
            // (row n + 4 is used only while n + 4 <= rows + 1: the index stops at the third element past the last
            // row, the padding that the entry points ask for)
            const int64_t n4 = (n + 4 < rows + 2) ? n + 4 : rows + 2;
            t_3 = tg[n4 + vz];
            y_3 = yg[n4 + vz];
            g_3 = gg[n4 + vz];
            wg_lds_barrier();
            double s1 = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) s1 += sh.p[nxt][w2][0];
            const double dn = a_n - s1;
            const double zn = SAMPLE ? fma(__dsqrt_rn(dn), yy, sh.p[nxt][NW - 1][1])   // the draw x_n + u~ . F~
                                     : yy - sh.p[nxt][NW - 1][1];
            // d, z leave in coalesced blocks of 64 rows (lane j keeps row 64 m + j): a store per row would
            // sit in the same in-order queue as the y / diag prefetches and make their waits wait for HBM
            // write acknowledgements
            dacc = (lane == (int)(n & 63)) ? dn : dacc;
            zacc = (lane == (int)(n & 63)) ? zn : zacc;
            if ((n & 63) == 63) { dg[n - 63 + lane] = dacc; zg[n - 63 + lane] = zacc; }
            if (!(dn > 0.0) && fail == 0) {
                const int64_t gf = g0 + n + 1;
                fail = (int32_t)(gf > 0x7fffffff ? 0x7fffffff : gf);
            }
            if ((n & (WIDE_FAIL_CHECK - 1)) == WIDE_FAIL_CHECK - 1 && fail) break;
        }
        if (fail) {
            if (lane == 0) info[b] = fail;
        } else if (rows & 63) {                     // the last, partial block of d, z
            const int64_t base = rows - (rows & 63);
            if (lane < (int)(rows & 63)) { dg[base + lane] = dacc; zg[base + lane] = zacc; }
        }
        return;
    }

    // ---------------- sweep waves ------------------------------------------------------------------
    const int g = lane >> 4, c = lane & 15;
    const int cb = wave * 16 + c;                   // column pair (complex term) of this lane
    const int own = 2 * cb + (lane >> 5);           // the column whose row-vector entries this lane carries
    double *__restrict__ rg = r_out ? r_out + pb * CP + own : nullptr;
    double *__restrict__ wg = Wt_out ? Wt_out + pb * CP + own : nullptr;
    double *__restrict__ Sg = S_state + (size_t)b * ((size_t)CP * RP);      // [column][row]
    const double notF = (own == FCOL) ? 0.0 : 1.0;
    const double isF1 = (2 * cb + 1 == FCOL) ? 1.0 : 0.0;   // this lane's second state column is F~
    double *__restrict__ col0 = Sg + (size_t)(2 * cb) * RP + 2 * g;
    double *__restrict__ col1 = col0 + RP;
    double T[TR][2];
    const bool zero_start = (A.block_sub >> 30) & 1;        // nominal pass: the state slots are outputs only
#pragma unroll
    for (int m = 0; m < TR; ++m) {
        T[m][0] = zero_start ? 0.0 : col0[8 * (m >> 1) + (m & 1)];
        T[m][1] = zero_start ? 0.0 : col1[8 * (m >> 1) + (m & 1)];
    }
    double q0 = 0.0, q1 = 0.0;
    sh.w[0][own] = 0.0;
    wg_lds_barrier();
    // row 0's operands, own-column entries and reset span
    double2 wb[PRE ? NK : 1];
    if constexpr (PRE) {
#pragma unroll
        for (int k = 0; k < NK; ++k) wb[k] = double2{0.0, 0.0};
    }
    double vt_c = sh.v[0][own];
    double2 u01 = *reinterpret_cast<const double2 *>(&sh.u[0][2 * cb]);     // u~ of the two state columns
    double2 fa = *reinterpret_cast<const double2 *>(&sh.f[0][0]);           // (reset span, a_n)
    double yy = sh.f[0][2];
    double de = read_lane(fa.x, 0);
    int b0 = 0, b1 = 1;                             // buffers of rows n and n + 1
    int32_t fail = 0;

    // Two loops: the outer one runs once per scaling block (its first row is a reset row: fold the pending
    // update, decay), the inner one over the block's rows has NO conditional update of T -- with the reset
    // inside the row loop the register allocator kept T in two register sets and copied all of it twice
    // per row (84 v_mov_b64 next to 80 FMAs).
    int64_t n = 0;
    bool stop = false;
    while (n < rows && !stop) {
    if (de >= 0.0) {                        // workgroup-uniform reset row
        const double2 *pw = (const double2 *)sh.w[n & 1] + g;
        double d0, d1, el0, el1;
        both_halves(sh.e[b0][own], el0, el1);               // decays of this lane's two state columns
        if constexpr (PRE) {                                // (the pending multipliers are in registers)
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const double2 e = ((const double2 *)sh.e[b0] + g)[4 * k], w = wb[k];
                T[2 * k][0] = fma(w.x, q0, T[2 * k][0]) * (e.x * el0);
                T[2 * k][1] = fma(w.x, q1, T[2 * k][1]) * (e.x * el1);
                T[2 * k + 1][0] = fma(w.y, q0, T[2 * k + 1][0]) * (e.y * el0);
                T[2 * k + 1][1] = fma(w.y, q1, T[2 * k + 1][1]) * (e.y * el1);
            }
            (void)pw; (void)d0; (void)d1;
        } else {
            sweepw_run<TR, true>(T, (const double2 *)sh.e[b0] + g, pw, q0, q1, el0, el1, d0, d1);
        }
        q0 = 0.0;
        q1 = 0.0;
    }
    do {
        const int cur = (int)(n & 1), nxt = cur ^ 1;
        const double2 *pw = (const double2 *)sh.w[cur] + g, *pu = (const double2 *)sh.u[b0] + g;
        __builtin_amdgcn_s_setprio(0);
        double acc0, acc1;
        if constexpr (PRE) sweepw_regs<TR>(T, pu, wb, q0, q1, acc0, acc1);
        else sweepw_run<TR, false>(T, pu, pw, q0, q1, 0.0, 0.0, acc0, acc1);
        // the serial part of the row wins the issue arbitration against the other workgroup's sweep
        __builtin_amdgcn_s_setprio(GF_CHAIN_PRIO);
        // what the generator wrote of row n + 1 (two rows ahead) is fetched here, in the shadow of the
        // reductions: this lane's own-column entries, the reset span, the diagonal and y
        const double vt_n = sh.v[b1][own];
        const double2 u01_n = *reinterpret_cast<const double2 *>(&sh.u[b1][2 * cb]);
        const double2 fa_n = *reinterpret_cast<const double2 *>(&sh.f[b1][0]);
        const double yy_n = sh.f[b1][2];
        // this lane's share of the quadratic form u~^T T u~ (its rows x its two columns): the pivot's
        // reduction runs next to -- not after -- the column sums
        const double p1 = wave_sum(fma(acc0, u01.x, acc1 * u01.y));
        const double tmp = own_column_sum4(acc0, acc1);
        const double r = (vt_c - tmp) * notF;
        double r0, r1;
        both_halves(r, r0, r1);                     // r of this lane's two state columns
        sh.w[nxt][own] = r;
        const double p2 = read_lane(tmp, 47);       // column FCOL of the last sweep wave: u~ . F~
        *reinterpret_cast<double2 *>(sh.p[nxt][wave]) = double2{p1, p2};    // (uniform, every lane: no branch)
        wg_lds_barrier();
        double s1 = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) s1 += sh.p[nxt][w2][0];
        const double s2 = sh.p[nxt][NW - 1][1];
        if constexpr (PRE) {                        // next row's w operands: the only reads behind the barrier
#pragma unroll
            for (int k = 0; k < NK; ++k) wb[k] = ((const double2 *)sh.w[nxt] + g)[4 * k];
        }
        const double dn = fa.y - s1;                // every wave forms the pivot itself
        const double zn = SAMPLE ? __dsqrt_rn(dn) * yy : yy - s2;      // (the draw: x_n rides where z_n does)
        vt_c = vt_n; u01 = u01_n; fa = fa_n; yy = yy_n;
        de = read_lane(fa.x, 0);
        b0 = b1; b1 = (b1 == 2) ? 0 : b1 + 1;
        if (!(dn > 0.0)) fail = 1;                  // (the generator wave records the row)
        const double inv = fast_rcp(dn);
        q0 = r0 * inv;                              // multipliers of this lane's two state columns;
        q1 = fma(zn, isF1, r1) * inv;               // column FCOL: z / d (r is 0 there)
        const size_t ro = opaque_uniform((size_t)n * CP);
        if (rg) rg[ro] = r;                         // r~ rows (chunk mode)
        if (wg) wg[ro] = r * inv;
        stop = (n & (WIDE_FAIL_CHECK - 1)) == WIDE_FAIL_CHECK - 1 && fail;
        ++n;
    } while (n < rows && !(de >= 0.0) && !stop);
    }
    __builtin_amdgcn_s_setprio(0);
    if (fail) return;                               // (the generator wave records the row)
    const int fin = (int)(rows & 1);                // buffer written by the last row
#pragma unroll
    for (int m = 0; m < TR; ++m) {
        const int ro = 8 * (m >> 1) + (m & 1);
        const double w = sh.w[fin][2 * g + ro];
        col0[ro] = fma(w, q0, T[m][0]);
        col1[ro] = fma(w, q1, T[m][1]);
    }
}

// ------------------------------------------------------------------------------------
// k_phiw: the closed-loop transition sweep of the exact time-parallel evaluation (k_phi / k_phi7) for WIDE
// kernels:  Phi <- (I - w~ u~^T) Phi  (rows scaled by E at reset rows),  h_n = Phi^T u~_n, on the rows the
// nominal pass stored (u~ rows, r~ rows, pivots, reset spans).  Its columns are INDEPENDENT -- the
// multipliers -h_j / d of a column come from that column's own mat-vec -- so every wave sweeps its 16
// columns of Phi with no barrier and no generator: one single-wave workgroup per (problem, chunk, 16
// columns), lane (g, c) = (lane >> 3, lane & 7) holds the column pair 8 w + c of the row pairs
// 16k + 2g, 16k + 2g + 1 (8 row groups: 22 rows per lane at W = 172, so two waves per SIMD fit), row
// operands staged per wave in LDS from plain coalesced row loads two rows ahead.  The Gram sums
// G = sum h h^T / d and the W x W combines of the chunk maps are plain dense GEMMs / solves and run
// as library calls (rocBLAS / hipSOLVER through torch) on these outputs.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double own_column_sum8(const double a, const double b) {
    const double h = own_column_sum(a, b);          // lanes l, l ^ 32 (reduce-scatter over the halves)
    const auto l = __builtin_amdgcn_permlane16_swap(__double2loint(h), __double2loint(h), false, false);
    const auto u = __builtin_amdgcn_permlane16_swap(__double2hiint(h), __double2hiint(h), false, false);
    double s = __hiloint2double(u[0], l[0]) + __hiloint2double(u[1], l[1]);     // l, l ^ 16
    s += dpp_get<0x128, 0xf>(s);                                                  // row_ror:8: l, l ^ 8
    return s;
}

// D ring slots (a power of two) of NI kilobytes per row vector; rows arrive D - 2 rows ahead of their use
// (the u~ row, the pivot and the reset span of a row travel in ONE slot: lanes 63 / 62 of the last piece
// fetch the 16-byte pairs that hold dbar[row] / de[row]).  The register queue this replaces was two rows
// deep: with row arrays beyond the caches (a shard of cfg4: 3 x 9.8 GB) a row cost 0.9 us, all of it
// memory latency at eight waves per CU.
template <int TR, int D, int NI>
__global__ void __launch_bounds__(64, (TR <= 12 && NI == 1) ? 4 : 2)
k_phiw(const int64_t N, const int64_t chunk_len, const int nch, const int ch0, const int nsel, const int W,
       const int CP,
       const double *__restrict__ c_, const double *__restrict__ de_, const double *__restrict__ dbar_,
       const double *__restrict__ rbar_, const double *__restrict__ ut_,
       double *__restrict__ h_out, double *__restrict__ Phi_out) {
    static_assert((D & (D - 1)) == 0 && D >= 4, "ring slots: a power of two");
    constexpr int RP = 8 * TR;                      // state rows, padded
    constexpr int LV = 192;                         // LDS row vectors (CP, RP <= 192)
    constexpr int NL = 3;                           // row entries per lane (lane, lane + 64, lane + 128)
    constexpr int SL = 128 * NI;                    // doubles per ring slot (CP <= SL - 4)
    constexpr int SD = SL - 2, SE = SL - 4;         // the row's pivot pair / reset-span pair
    const int lane = threadIdx.x;
    // waves (16-column groups) per chunk: groups made of pad columns only are not swept (the combine reads
    // 16 ceil(W / 16) columns of h and W columns of Phi; what lies beyond is left unwritten)
    const int nwv = (W + 15) / 16;
    const int sel = blockIdx.x / nwv, wave = blockIdx.x - sel * nwv;
    const int pr = sel / nsel, ch = ch0 + (sel - pr * nsel);       // chunks ch0 .. ch0 + nsel - 1 of every problem
    const int slot = pr * nch + ch;
    const int g = lane >> 3, c = lane & 7;
    const int cb = wave * 8 + c;                    // column pair of this lane
    const int own = 2 * cb + (lane >> 5);           // its own column (h, multipliers)
    const int64_t c0 = (int64_t)ch * chunk_len;
    const int64_t rows = (N - c0 < chunk_len) ? (N - c0) : chunk_len;
    const size_t pb = (size_t)pr * N + c0;
    double *__restrict__ hg = h_out + pb * CP + own;
    __shared__ __attribute__((aligned(16))) double ring_u[D][SL], ring_r[D + 1][SL], s_e[LV];
    const unsigned lds_u = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(&ring_u[0][0]));
    const unsigned lds_r = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<uintptr_t>(&ring_r[0][0]));
    const double2 *pe = (const double2 *)s_e + g;
    double ci[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int i = lane + 64 * k;
        ci[k] = (i < W) ? c_[(size_t)pr * W + i] : 0.0;
        s_e[i] = 1.0;                               // (LV = 192 = 3 * 64: every entry initialised)
    }
    for (int e = lane; e < SL; e += 64) ring_r[D][e] = 0.0;        // "no pending update" for the first row
    // Per-lane source of piece j of a row's u~ slot / r~ slot: address = cursor & mask, the cursor advancing by
    // `step` bytes per row.  Data lanes: the row's doubles 128 j + 2 lane (lanes past the row re-read its
    // start).  Lanes 63 / 62 of the last piece: the aligned 16-byte pair that holds dbar[row] / de[row] (step
    // 8, mask clears bit 3).  Rows are fetched D - 1 ahead, unconditionally: the caller's arrays are readable
    // 8 rows past the end.
    uintptr_t cu[NI], cr[NI], mu[NI];
    unsigned long long su_step[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int e = 128 * j + 2 * lane;
        const int ec = (e < CP) ? e : 0;
        cu[j] = reinterpret_cast<uintptr_t>(ut_ + pb * CP + ec);
        cr[j] = reinterpret_cast<uintptr_t>(rbar_ + pb * CP + ec);
        mu[j] = ~(uintptr_t)0;
        su_step[j] = (unsigned long long)CP * 8;
        if (j == NI - 1 && lane >= 62) {
            cu[j] = reinterpret_cast<uintptr_t>((lane == 63 ? dbar_ : de_) + pb);
            mu[j] = ~(uintptr_t)15;
            su_step[j] = 8;
        }
    }
    const unsigned long long r_step = (unsigned long long)CP * 8;
    auto issue = [&](const int64_t m, const int after) {      // row m (the cursors stand at it) -> slot m mod D
        const unsigned so = (unsigned)(m & (D - 1)) * (SL * 8);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            glds16(reinterpret_cast<const void *>(cu[j] & mu[j]), lds_u + so + 1024 * j, after);
            glds16(reinterpret_cast<const void *>(cr[j]), lds_r + so + 1024 * j, after);
            cu[j] += su_step[j];
            cr[j] += r_step;
        }
    };
#pragma unroll
    for (int m = 0; m < D - 1; ++m) issue(m, 0);
    double T[TR][2];
#pragma unroll
    for (int m2 = 0; m2 < TR; ++m2) {               // Phi = I
        const int row = 16 * (m2 >> 1) + 2 * g + (m2 & 1);
        T[m2][0] = (row == 2 * cb) ? 1.0 : 0.0;
        T[m2][1] = (row == 2 * cb + 1) ? 1.0 : 0.0;
    }
    double q0 = 0.0, q1 = 0.0;
    wave_lds_fence();
    for (int64_t n = 0; n < rows; ++n) {
        // row n has landed: the operations issued after its copies are the (D - 2) rows behind it and, once
        // the loop is in its steady state, one h store per iteration
        if (n < D - 2) vm_wait<(D - 2) * 2 * NI>();
        else vm_wait<(D - 2) * (2 * NI + 1)>();
        const int sl = (int)(n & (D - 1)), par = (int)((pb + n) & 1);
        const double dcur = ring_u[sl][SD + par];
        const double de = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(ring_u[sl][SE + par])),
                                           __builtin_amdgcn_readfirstlane(__double2loint(ring_u[sl][SE + par])));
        const double2 *pu = (const double2 *)&ring_u[sl][0] + g;
        const double2 *pw = (const double2 *)&ring_r[(n == 0) ? D : (int)((n - 1) & (D - 1))][0] + g;
        if (de >= 0.0) {                    // reset row: Phi <- E (Phi + pending): row scaling only
#pragma unroll
            for (int k = 0; k < NL; ++k) s_e[lane + 64 * k] = fm_exp_local(-ci[k] * de);
            wave_lds_fence();
            double d0, d1;
            sweepw_run<TR, true, 8>(T, pe, pw, q0, q1, 1.0, 1.0, d0, d1);
            q0 = 0.0;
            q1 = 0.0;
        }
        double acc0, acc1;
        sweepw_run<TR, false, 8>(T, pu, pw, q0, q1, 0.0, 0.0, acc0, acc1);
        const double h = own_column_sum8(acc0, acc1);
        hg[(size_t)n * CP] = h;             // (the four owner lanes of a column write the same value)
        both_halves(-h * fast_rcp(dcur), q0, q1);      // pending: Phi_i -= (r_i / d) h_j, row n's r from its ring slot
        // row n + D - 1 into the slot of row n - 1, whose r~ this iteration's sweeps were the last to read
        issue(n + D - 1, __double2loint(h));
    }
    vm_wait<0>();                           // no copy may outlive the wave's LDS allocation
    const double *s_w = &ring_r[(int)((rows - 1) & (D - 1))][0];
    double *__restrict__ col0 = Phi_out + (size_t)slot * ((size_t)CP * RP) + (size_t)(2 * cb) * RP + 2 * g;
    double *__restrict__ col1 = col0 + RP;
#pragma unroll
    for (int m2 = 0; m2 < TR; ++m2) {
        const int ro = 16 * (m2 >> 1) + (m2 & 1);
        const double w = s_w[2 * g + ro];
        col0[ro] = fma(w, q0, T[m2][0]);
        col1[ro] = fma(w, q1, T[m2][1]);
    }
}

// (the archived sweep variants k_factor4/5/6 of rounds 1-3 live outside the package: tools/archive/sweeps_456.inc)

// ------------------------------------------------------------------------------------
// Exact time-parallel evaluation of ONE series (Lainiotis-type partitioning; the numpy
// derivation and its verification against the sequential recurrence are in DESIGN.md 4.3).
// The series is cut into nch chunks.  With X = S (+ pending update) handed from chunk to chunk:
//   nominal pass  (k_factor3, zero start)      : Xbar_end, Ybar_end, dbar, zbar, rbar per chunk
//   k_phi         : closed-loop transition      Phi <- (I - w~ u~^T) Phi,  h_n = Phi^T u~_n
//   k_gram        : G = sum h h^T / dbar ,  m = sum h zbar / dbar
//   k_combine     : X+ = Xbar_end + Phi K Phi^T ,  K = (I - X G)^-1 X          (sequential in c)
//                   Y+ = Ybar_end + Phi (I - X G)^-1 (Y - X m)
//   final pass    (k_factor3 from the true X, Y): d, z  -- identical to the sequential run
// k_phi is the same register-resident sweep as the factor: Phi_i += (r~_{n-1,i}) * (-h_{n-1}/d),
// h_n = sum_i u~_{n,i} Phi_i, with no reduction and no division on its chain.
// ------------------------------------------------------------------------------------
template <int ROWS>
__global__ void __launch_bounds__(64, 2)
k_phi(const int64_t N, const int64_t chunk_len, const int nch, const int ch0, const int nsel, const int W,
      const double *__restrict__ c_, const double *__restrict__ de_, const double *__restrict__ dbar_,
      const double *__restrict__ zbar_, const double *__restrict__ rbar_, const double *__restrict__ ut_,
      double *__restrict__ Phi_out, double *__restrict__ G_out, double *__restrict__ m_out) {
    constexpr int NT = (ROWS + 15) / 16, PD = PhiRing::PD;
    const int lane = threadIdx.x;
    const int sel = blockIdx.x;
    const int pr = sel / nsel, ch = ch0 + (sel - pr * nsel);
    const int b = pr * nch + ch;
    const int64_t c0 = (int64_t)ch * chunk_len;
    const int64_t rows = (N - c0 < chunk_len) ? (N - c0) : chunk_len;
    const size_t pb = (size_t)pr * N + c0;
    double *__restrict__ Pg = Phi_out + (size_t)b * (64 * 64) + (size_t)lane * 64;
    const double cj = (lane < W) ? c_[(size_t)pr * W + lane] : 0.0;

    __shared__ __attribute__((aligned(16))) PhiRing R;
    __shared__ __attribute__((aligned(16))) PhiGram<NT> Gm;
    __shared__ __attribute__((aligned(16))) double s_e[64];
    double T[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) T[i] = (i == lane) ? 1.0 : 0.0;      // Phi = I
    double q = 0.0, macc = 0.0;
    d4 acc[PhiGram<NT>::NACC];
#pragma unroll
    for (int t = 0; t < PhiGram<NT>::NACC; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    R.r[PD][lane] = 0.0;
    for (int e = lane; e < 16 * PhiGram<NT>::LD; e += 64) (&Gm.hs[0][0])[e] = 0.0;
    if (lane < 16) Gm.sv[lane] = 0.0;
    PhiCursor C;
    C.template init<ROWS>(R, lane, pb, ut_, rbar_, dbar_, de_, zbar_);
#pragma unroll
    for (int m = 0; m < PD - 1; ++m) C.issue(m, 0);
    vm_wait<2 * (PD - 2)>();
    wave_lds_fence();
    double ab[SW_AHEAD + 1][SW_BR], wb[SW_AHEAD + 1][SW_BR];
    const double *su = &R.u[0][0], *sw = &R.r[PD][0];
    sweep_preload<ROWS>(ab, wb, su, sw);

    for (int64_t n = 0; n < rows; ++n) {
        vm_wait<2 * (PD - 3)>();
        const int sl = (int)(n & (PD - 1)), par = (int)((pb + n) & 1);
        const double dcur = R.u[sl][PhiRing::OD + par], zcur = R.u[sl][PhiRing::OZ + par];
        const double dev = R.u[sl][PhiRing::OE + par];
        const double de = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(dev)),
                                           __builtin_amdgcn_readfirstlane(__double2loint(dev)));
        if (de >= 0.0) {                    // Phi <- E (Phi + pending): row scaling only
            s_e[lane] = fm_exp_local(-cj * de);
            wave_lds_fence();
            sweep_preload<ROWS>(ab, wb, s_e, sw);
            (void)sweep_run<ROWS, true>(T, ab, wb, s_e, sw, q, 1.0);
            sweep_preload<ROWS>(ab, wb, su, sw);
            q = 0.0;
        }
        const double h = sweep_run<ROWS, false>(T, ab, wb, su, sw, q, 0.0);
        const double rinv = (dcur > 0.0) ? fast_rcp(dcur) : 0.0;
        Gm.hs[n & 15][lane] = h;
        if (lane == 0) Gm.sv[n & 15] = rinv;
        macc = fma(h, zcur * rinv, macc);
        su = &R.u[(int)((n + 1) & (PD - 1))][0];
        sw = &R.r[sl][0];
        sweep_preload<ROWS>(ab, wb, su, sw);
        q = -h * rinv;                      // pending: Phi_i -= (r_i / d) h_j
        C.issue(n + PD - 1, __double2loint(h));
        if ((n & 15) == 15) phi_gram_flush<NT>(Gm, acc, lane);
    }
    vm_wait<0>();
    if (rows & 15) phi_gram_flush<NT>(Gm, acc, lane);
    wave_lds_fence();
    const double *s_w = &R.r[(int)((rows - 1) & (PD - 1))][0];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) Pg[i] = fma(s_w[i], q, T[i]);
#pragma unroll
    for (int i = ROWS; i < 64; ++i) Pg[i] = 0.0;
    phi_gram_store<NT>(acc, macc, G_out + (size_t)b * (64 * 64), m_out + (size_t)b * 64, lane, lane);
}

// ---- dense helpers for the chunk combines (one workgroup of 256 threads) ---------------------
// LDS matrices are NS x NS, row-major with the odd leading dimension NS + 1 (conflict-free rows); global
// matrices are 64 x 64 slots stored [j][i] (column-major = the lane-major layout of the sweep states), zero
// beyond the width.  NS = 64, 48 for the widths <= 48, 32 for those <= 32: 135 / 77 / 36 KB of LDS per workgroup,
// one / two / four workgroups per CU -- the levels of the tree scan with more pairs than CUs run in half / a
// quarter of the rounds.
template <int NS> struct CbDims {
    static constexpr int LD = NS + 1;           // a matrix' row stride
    static constexpr int LA = 2 * NS + 2;       // the augmented system's: [A | RHS | one vector]
    static constexpr int VC = 2 * NS;           // the vector's column
    static constexpr int NC = NS / 2 + 1;       // Gauss-Jordan: registers per lane (columns c = 4 lc + wave <= VC)
    static constexpr int R0 = NS / 4;           // ... the first one of the right-hand sides
};

template <int NS = 64>
__device__ __forceinline__ void cb_load(double *dst, const double *__restrict__ src, int tid,
                                        int ld = CbDims<NS>::LD) {
    if (NS < 64 && (tid & 63) >= NS) return;            // (element e = [j][i]: row i = e & 63, column j = e >> 6)
#pragma unroll
    for (int q = 0; q < NS / 4; ++q) { const int e = tid + 256 * q, j = e >> 6, i = e & 63; dst[i * ld + j] = src[e]; }
}

// 64 x 64 x 64 products on v_mfma_f64_16x16x4 (256 threads = 4 waves; wave w owns rows 16w..16w+15
// of the result as four accumulator tiles): acc[q][r] = element (cb_row(ty, r), cb_col(tx, q)) of
// A' B' with A'(row, k) = a_of(row, k), B'(k, col) = b_of(k, col) read from LDS -- two LDS reads per
// 1024 FMAs instead of one per two with 4x4 register blocks (which ran LDS-bound).
__device__ __forceinline__ int cb_row(int ty, int r) { return 16 * (ty >> 2) + (ty & 3) + 4 * r; }
__device__ __forceinline__ int cb_col(int tx, int q) { return 16 * q + tx; }

// nt (wave-uniform, 1 .. 4): only the leading 16 nt rows / columns of the operands are non-zero (states of
// width W <= 16 nt, zero-padded to 64): the other tiles of the result are zeros and are not computed.
template <class FA, class FB>
__device__ __forceinline__ void cb_mm(double (&acc)[4][4], FA a_of, FB b_of, int tx, int ty, const int nt = 4) {
    const int i = tx, k = ty & 3, w = ty >> 2;          // lane = (i, k) of wave w
    d4 C[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) C[q] = d4{0.0, 0.0, 0.0, 0.0};
    if (nt == 4) {
        // the full width as straight-line code: with a loop the accumulators travel between the vector and the
        // accumulation registers on every trip (64 moves per 16 MFMAs)
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const double av = a_of(16 * w + i, 4 * ks + k);
#pragma unroll
            for (int q = 0; q < 4; ++q) C[q] = GF_MFMA64(av, b_of(4 * ks + k, 16 * q + i), C[q]);
        }
    } else if (nt == 3) {                               // (widths 33 .. 48: cfg3's W = 40)
        if (w < 3) {
#pragma unroll
            for (int ks = 0; ks < 12; ++ks) {
                const double av = a_of(16 * w + i, 4 * ks + k);
#pragma unroll
                for (int q = 0; q < 3; ++q) C[q] = GF_MFMA64(av, b_of(4 * ks + k, 16 * q + i), C[q]);
            }
        }
    } else if (w < nt) {
#pragma unroll 4
        for (int ks = 0; ks < 4 * nt; ++ks) {
            const double av = a_of(16 * w + i, 4 * ks + k);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nt) C[q] = GF_MFMA64(av, b_of(4 * ks + k, 16 * q + i), C[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[q][r] = C[q][r];
}

// acc = A' B' with A' = A or A^T (TA), B' = B or B^T (TB), row-major LDS matrices
template <bool TA, bool TB>
__device__ __forceinline__ void cb_matmul(double (&acc)[4][4], const double *A, int lda,
                                          const double *B, int ldb, int tx, int ty, const int nt = 4) {
    cb_mm(acc,
          [&](int row, int k) { return TA ? A[k * lda + row] : A[row * lda + k]; },
          [&](int k, int col) { return TB ? B[col * ldb + k] : B[k * ldb + col]; }, tx, ty, nt);
}

template <int NS = 64>
__device__ __forceinline__ void cb_store_lds(double *dst, int ld, const double (&acc)[4][4], int tx, int ty) {
    if (NS < 64 && 16 * (ty >> 2) >= NS) return;        // (wave ty >> 2 holds the rows 16 (ty >> 2) ...)
#pragma unroll
    for (int q = 0; q < NS / 16; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[cb_row(ty, r) * ld + cb_col(tx, q)] = acc[q][r];
}

// Gauss-Jordan with IMPLICIT partial pivoting on the 64 x 129 augmented system Au = [A | RHS],
// held in registers with lanes = rows: wave w (of 4) owns the columns c = w (mod 4), 33 registers
// per lane.  Step k: the wave that owns column k searches the pivot among the unused rows, forms the
// row multipliers f_i = a_ik / a_pk (lane form, f_p = 0) and publishes them with the pivot's lane
// index through LDS; after ONE barrier every wave eliminates its columns, fetching the pivot row's
// entries with readlane (an SGPR operand of the FMA: no LDS traffic in the update).  Rows are never
// swapped or normalised, eliminated columns are not revisited (updating them is harmless and keeps
// the loops compile-time).  The multiplier buffer alternates between two halves so that the next
// owner may write while slower waves still read.
// The search runs one step AHEAD: behind the barrier of step k the owner of column k + 1 updates that
// column first, searches and publishes step k + 1, and only then eliminates the rest of its columns --
// while the other three waves are still eliminating for step k.  And its dependent chain is short: the
// magnitudes compare as 32-bit keys (the high word of |a|: exponent + 20 mantissa bits -- a pivot within
// 1e-6 of the largest is as good), a DPP max per step inside the rows of 16 lanes and scalar maxima
// across them; every lane has the reciprocal of its own entry ready before the pivot is known.  (A step
// took 1290 cycles with the search of a 64-bit maximum, its reciprocal and the whole update in sequence;
// tools/_dbg_tree.py.)
// scratch >= 140 doubles.  On exit Au[:, 64:129] = A^-1 RHS.
// n (uniform, <= 64): the system is the identity beyond its leading n x n block with zero right-hand sides there
// (zero-padded states): the steps k >= n are skipped and those rows of the solution are zeros.
template <int NS = 64>
__device__ __forceinline__ void cb_gauss_jordan(double *Au, double *scratch, int tid, const int n = NS) {
    constexpr int LA = CbDims<NS>::LA, NC = CbDims<NS>::NC, VC = CbDims<NS>::VC, R0 = CbDims<NS>::R0;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *fbuf = scratch;                                     // [2][64] multipliers
    double *pinvbuf = scratch + 128;                            // [2]
    int *pvbuf = reinterpret_cast<int *>(scratch + 130);        // [2]
    const bool dead = NS < 64 && lane >= NS;                    // (no such row)
    double R[NC];
#pragma unroll
    for (int lc = 0; lc < NC; ++lc) {
        const int c = 4 * lc + w;
        R[lc] = (c <= VC && !dead) ? Au[lane * LA + c] : 0.0;
    }
    bool used = dead;                       // row `lane` already served as a pivot (or does not exist)
    int myk = 0;                            // ... of which variable
    double mypinv = 0.0;                    // ... with which 1 / pivot
    if (w == 0 && n > 0) gj_search(R[0], used, lane, fbuf, pvbuf, pinvbuf);
    static_for([&](auto kc) {
        constexpr int k = decltype(kc)::value, lk = k >> 2, buf = k & 1;
        constexpr int k1 = k + 1, w1 = k1 & 3, lk1 = k1 >> 2, buf1 = k1 & 1;
        if (k >= n) return;
        __syncthreads();
        const double f = fbuf[buf * 64 + lane];
        const int pv = __builtin_amdgcn_readfirstlane(pvbuf[buf]);
        if (lane == pv) { used = true; myk = k; mypinv = pinvbuf[buf]; }
        if (k1 < NS && k1 < n && w == w1) {                     // (wave-uniform) the next column's owner
            R[lk1] = fma(-f, read_lane(R[lk1], pv), R[lk1]);
            gj_search(R[lk1], used, lane, fbuf + buf1 * 64, pvbuf + buf1, pinvbuf + buf1);
            gj_update<lk, NC, lk1>(R, f, pv);
        } else {
            gj_update<lk, NC, -1>(R, f, pv);
        }
    }, std::make_integer_sequence<int, NS>{});
    // row `lane` solved variable myk:  x(myk, :) = (right part of the row) / pivot
    const bool piv = used && !dead;
#pragma unroll
    for (int lc = R0; lc < NC; ++lc) {
        const int c = 4 * lc + w;
        if (c <= VC && !dead) Au[(piv ? myk : lane) * LA + c] = piv ? R[lc] * mypinv : 0.0;   // (rows >= n: never pivots)
    }
    __syncthreads();
}

// One application of a chunk map to a state, in LDS:  on entry Xs = X, Ys = Y (LDS); Phi, G, m,
// Xbar, Ybar of the map are read from global.  On exit Xs = X+, Ys = Y+.
//   A = I - X G ;  [K | v] = A^-1 [X | Y - X m] ;  X+ = Xbar + Phi K Phi^T ;  Y+ = Ybar + Phi v
template <int NS = 64>
__device__ __forceinline__ void cb_apply(double *Xs, double *Au, double *Bs, double *Ys, double *vs,
                                         const double *__restrict__ Pg, const double *__restrict__ Gg,
                                         const double *__restrict__ mg, const double *__restrict__ Xbar,
                                         const double *__restrict__ Ybar, const double (&xreg)[16],
                                         const double yreg, int tid, const int n = NS) {
    const int nt = (n + 15) >> 4;             // (maps of width n <= NS, zero-padded: cb_mm / cb_gauss_jordan)
    // Xbar/Ybar: global pointers, or nullptr to take them from registers (xreg[q] = element
    // e = tid + 256 q of the [j][i] layout, yreg = element tid)
    constexpr int LD = CbDims<NS>::LD, LA = CbDims<NS>::LA, VC = CbDims<NS>::VC;
    const int tx = tid & 15, ty = tid >> 4;
    cb_load<NS>(Bs, Gg, tid);
    if (tid < 64) vs[tid] = mg[tid];
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, Xs, LD, Bs, LD, tx, ty, nt);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int i = cb_row(ty, cc), j = cb_col(tx, a);
                if (NS == 64 || (i < NS && j < NS)) {
                    Au[i * LA + j] = ((i == j) ? 1.0 : 0.0) - acc[a][cc];
                    Au[i * LA + NS + j] = Xs[i * LD + j];
                }
            }
    }
    if (tid < NS) {                         // rhs = Y - X m
        double sacc = Ys[tid];
        for (int k = 0; k < n; ++k) sacc = fma(-Xs[tid * LD + k], vs[k], sacc);
        Au[tid * LA + VC] = sacc;
    }
    __syncthreads();
    cb_gauss_jordan<NS>(Au, Bs, tid, n);
    // Bs <- Phi ; Xs <- Z = Phi K  (K symmetrised)
    cb_load<NS>(Bs, Pg, tid);
    if (tid < NS) vs[tid] = Au[tid * LA + VC];
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_mm(acc,
              [&](int row, int k) { return Bs[row * LD + k]; },
              [&](int k, int col) { return 0.5 * (Au[k * LA + NS + col] + Au[col * LA + NS + k]); },
              tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(Xs, LD, acc, tx, ty);
    }
    double ynew = 0.0;
    if (tid < NS) {                         // Y+ = Ybar + Phi v
        ynew = Ybar ? Ybar[tid] : yreg;
        for (int k = 0; k < n; ++k) ynew = fma(Bs[tid * LD + k], vs[k], ynew);
    }
    __syncthreads();
    {                                       // X+ = Xbar + Z Phi^T  -> Au left half as staging
        double acc[4][4] = {};
        cb_matmul<false, true>(acc, Xs, LD, Bs, LD, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(Au, LA, acc, tx, ty);
    }
    __syncthreads();
    if (NS == 64 || (tid & 63) < NS) {
#pragma unroll
        for (int q = 0; q < NS / 4; ++q) {          // add Xbar (coalesced) and symmetrise
            const int e = tid + 256 * q, j = e >> 6, i = e & 63;
            Xs[i * LD + j] = (Xbar ? Xbar[e] : xreg[q]) + 0.5 * (Au[i * LA + j] + Au[j * LA + i]);
        }
    }
    if (tid < 64) Ys[tid] = ynew;
    __syncthreads();
}

// Sequential LFT combine over the chunks of each problem (one workgroup per problem).
// S_state/F_state slot c holds (Xbar_end, Ybar_end) of chunk c on entry and the TRUE start
// state of chunk c on exit (slot 0 <- 0).
template <int NS>                       // LDS matrix size: 64 (widths beyond 48: compile-time bounds), 48 or 32
__global__ void __launch_bounds__(256)
k_combine(const int nch, const int n_, const double *__restrict__ Phi_, const double *__restrict__ G_,
          const double *__restrict__ m_, double *__restrict__ S_state,
          double *__restrict__ F_state) {
    constexpr bool FULL = NS == 64;
    constexpr int LD = CbDims<NS>::LD, LA = CbDims<NS>::LA;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *Xs = lds;                       // [NS][LD]
    double *Au = Xs + NS * LD;              // [NS][LA]
    double *Bs = Au + NS * LA;              // [NS][LD]
    double *Ys = Bs + NS * LD;              // [64]
    double *vs = Ys + 64;                   // [64]
    const int pr = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = FULL ? 64 : n_;
    const bool in = NS == 64 || (tid & 63) < NS;    // this thread's elements e = tid + 256 q lie in rows < NS
    for (int e = tid; e < NS * LD; e += 256) Xs[e] = 0.0;
    if (tid < 64) Ys[tid] = 0.0;
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const size_t slot = (size_t)pr * nch + c;
        double *Sg = S_state + slot * 4096;
        double *Fg = F_state + slot * 64;
        // keep this chunk's nominal end state, publish its TRUE start state (beyond NS the slots hold zeros, and keep them)
        double xbar[16], ybar = 0.0;
#pragma unroll
        for (int q = 0; q < NS / 4; ++q) {
            const int e = tid + 256 * q, j = e >> 6, i = e & 63;
            if (in) { xbar[q] = Sg[e]; Sg[e] = Xs[i * LD + j]; }
        }
        if (tid < 64) { ybar = Fg[tid]; Fg[tid] = Ys[tid]; }
        if (c == nch - 1) break;
        if (c == 0) {
            // from the zero state a chunk's map returns its own nominal end state (K = 0, v = 0): no solve
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NS / 4; ++q) {
                const int e = tid + 256 * q, j = e >> 6, i = e & 63;
                if (in) Xs[i * LD + j] = xbar[q];
            }
            if (tid < 64) Ys[tid] = ybar;
            __syncthreads();
            continue;
        }
        cb_apply<NS>(Xs, Au, Bs, Ys, vs, Phi_ + slot * 4096, G_ + slot * 4096, m_ + slot * 64,
                     nullptr, nullptr, xbar, ybar, tid, n);
    }
}

// ---- log-depth tree combine (Blelloch scan over the chunk maps) -----------------------------
// Map of a chunk: M = (Phi, G, Xbar, Ybar, m).  Up-sweep: map[right] <- map[right] o map[left]
//   D = (I - Xbar1 G2)^-1 ;  Phi12 = Phi2 D Phi1 ;  Xbar12 = Xbar2 + Phi2 D Xbar1 Phi2^T
//   G12 = G1 + Phi1^T G2 D Phi1 ;  v = D (Ybar1 - Xbar1 m2) ;  Ybar12 = Ybar2 + Phi2 v
//   m12 = m1 + Phi1^T (m2 - G2 v)                      (1 = left, applied first; 2 = right)
// Down-sweep on states: s[left] <- s[right] ; s[right] <- map[left](s[right]).
// Slots are (problem, index) with P = power-of-two indices per problem; identity maps pad.
struct TreeArgs {
    int P, d, n;                            // level: pairs (idx - d, idx), idx = (k+1) 2d - 1; n = state width
    int nch, pairs;                         // real chunks per problem; pairs launched per problem at this level
    double *Phi, *G, *S, *F, *m;            // maps   [B*nch][...]: the slots idx < nch, where the sweeps put them
    double *Xst, *Yst;                      // states [B*nch][4096] / [64]
    double *oPhi, *oG, *oS, *oF, *om, *oX, *oY;     // the slots nch <= idx < P (composites that reach into the padding
                                                    // and their states): [B*(P - nch)][...] in the caller's work buffer
};
struct TreeSlot { double *Phi, *G, *S, *F, *m, *X, *Y; };
__device__ __forceinline__ TreeSlot tree_slot(const TreeArgs &A, const int pr, const int idx) {
    TreeSlot t;
    if (idx < A.nch) {
        const size_t s = (size_t)pr * A.nch + idx;
        t.Phi = A.Phi + s * 4096; t.G = A.G + s * 4096; t.S = A.S + s * 4096; t.X = A.Xst + s * 4096;
        t.F = A.F + s * 64; t.m = A.m + s * 64; t.Y = A.Yst + s * 64;
    } else {
        const size_t s = (size_t)pr * (A.P - A.nch) + (idx - A.nch);
        t.Phi = A.oPhi + s * 4096; t.G = A.oG + s * 4096; t.S = A.oS + s * 4096; t.X = A.oX + s * 4096;
        t.F = A.oF + s * 64; t.m = A.om + s * 64; t.Y = A.oY + s * 64;
    }
    return t;
}

template <int NS>
__global__ void __launch_bounds__(256) k_tree_compose(const TreeArgs A) {
    constexpr bool FULL = NS == 64;
    constexpr int LD = CbDims<NS>::LD, LA = CbDims<NS>::LA, VC = CbDims<NS>::VC;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *M0 = lds;                       // [NS][LD]
    double *Au = M0 + NS * LD;              // [NS][LA]  = AL | AR | one vector
    double *M1 = Au + NS * LA;              // [NS][LD]
    double *v1 = M1 + NS * LD;              // [64] x 4 small vectors
    const int pairs = A.pairs;              // (the pairs whose left range holds a real chunk: the others are not launched)
    const int pr = blockIdx.x / pairs, k = blockIdx.x - pr * pairs;
    const int ir = (k + 1) * 2 * A.d - 1, il = ir - A.d;
    const TreeSlot SL = tree_slot(A, pr, il), SR = tree_slot(A, pr, ir);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n = FULL ? 64 : A.n, nt = FULL ? 4 : ((n + 15) >> 4);
    if (il + 1 >= A.nch) {
        // the right range [il + 1, ir] is padding (an identity map, nowhere stored): the composite is the left map
        for (int e = tid; e < 4096; e += 256) {
            SR.Phi[e] = SL.Phi[e];
            SR.G[e] = SL.G[e];
            SR.S[e] = SL.S[e];
        }
        if (tid < 64) { SR.F[tid] = SL.F[tid]; SR.m[tid] = SL.m[tid]; }
        return;
    }
    const bool in = NS == 64 || (tid & 63) < NS;    // this thread's slot elements e = tid + 256 q lie in rows < NS
    const bool vin = tid < NS;                      // ... its vector element exists
    double *w = v1, *vv = v1 + 64, *g2v = v1 + 128, *tmpv = v1 + 192;
    // a. M0 = Xbar1, M1 = G2 ;  AL = I - Xbar1 G2 ; AR = I ; the vector column = Ybar1 - Xbar1 m2
    cb_load<NS>(M0, SL.S, tid);
    cb_load<NS>(M1, SR.G, tid);
    if (tid < 64) tmpv[tid] = SR.m[tid];
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, M0, LD, M1, LD, tx, ty, nt);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = cb_row(ty, c), j = cb_col(tx, a);
                if (NS == 64 || (i < NS && j < NS)) {
                    Au[i * LA + j] = ((i == j) ? 1.0 : 0.0) - acc[a][c];
                    Au[i * LA + NS + j] = (i == j) ? 1.0 : 0.0;
                }
            }
    }
    if (vin) {
        double sacc = SL.F[tid];
        for (int kk = 0; kk < n; ++kk) sacc = fma(-M0[tid * LD + kk], tmpv[kk], sacc);
        Au[tid * LA + VC] = sacc;
    }
    __syncthreads();
    cb_gauss_jordan<NS>(Au, v1, tid, n);    // AR = D, the vector column = v   (scratch: w | vv | g2v, not yet in use;
                                            // G2 stays where it is -- with M1 as the scratch it was loaded twice)
    if (tid < 64) vv[tid] = vin ? Au[tid * LA + VC] : 0.0;
    __syncthreads();
    if (tid < 64) {                         // g2v = G2 v ;  m12 pieces need it
        double sacc = 0.0;
        if (vin)
            for (int kk = 0; kk < n; ++kk) sacc = fma(M1[tid * LD + kk], vv[kk], sacc);
        g2v[tid] = sacc;
    }
    // c. AL = D Xbar1
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, Au + NS, LA, M0, LD, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(Au, LA, acc, tx, ty);
    }
    __syncthreads();
    // d. M0 = Phi2 ;  AL <- Phi2 (D Xbar1) ;  Xbar12 = Xbar2 + AL Phi2^T ;  Ybar12 = Ybar2 + Phi2 v
    cb_load<NS>(M0, SR.Phi, tid);
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, M0, LD, Au, LA, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(Au, LA, acc, tx, ty);
    }
    if (tid < 64) {
        double sacc = SR.F[tid];
        if (vin)
            for (int kk = 0; kk < n; ++kk) sacc = fma(M0[tid * LD + kk], vv[kk], sacc);
        w[tid] = sacc;                      // Ybar12 (stored at the end)
    }
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<false, true>(acc, Au, LA, M0, LD, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(Au, LA, acc, tx, ty);
    }
    __syncthreads();
    if (in) {
        double *Sr = SR.S;
#pragma unroll
        for (int q = 0; q < NS / 4; ++q) {
            const int e = tid + 256 * q, j = e >> 6, i = e & 63;
            Sr[e] += 0.5 * (Au[i * LA + j] + Au[j * LA + i]);
        }
    }
    __syncthreads();
    // e. AL = Phi1 ;  AR <- D Phi1 ;  Phi12 = Phi2 (D Phi1)
    cb_load<NS>(Au, SL.Phi, tid, LA);
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, Au + NS, LA, Au, LA, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(Au + NS, LA, acc, tx, ty);
    }
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, M0, LD, Au + NS, LA, tx, ty, nt);
        double *Pr = SR.Phi;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) Pr[(size_t)cb_col(tx, a) * 64 + cb_row(ty, c)] = acc[a][c];
    }
    __syncthreads();
    // f. M1 <- G2 (D Phi1) ;  G12 = G1 + Phi1^T M1 ;  m12 = m1 + Phi1^T (m2 - G2 v)
    {
        double acc[4][4] = {};
        cb_matmul<false, false>(acc, M1, LD, Au + NS, LA, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(M1, LD, acc, tx, ty);
    }
    __syncthreads();
    {
        double acc[4][4] = {};
        cb_matmul<true, false>(acc, Au, LA, M1, LD, tx, ty, nt);
        __syncthreads();
        cb_store_lds<NS>(M0, LD, acc, tx, ty);  // Phi2 no longer needed
    }
    if (tid < 64) {
        double sacc = SL.m[tid];
        if (vin)
            for (int kk = 0; kk < n; ++kk) sacc = fma(Au[kk * LA + tid], tmpv[kk] - g2v[kk], sacc);
        SR.m[tid] = sacc;
        SR.F[tid] = w[tid];
    }
    __syncthreads();
    if (in) {
        double *Gr = SR.G;
        const double *Gl = SL.G;
#pragma unroll
        for (int q = 0; q < NS / 4; ++q) {
            const int e = tid + 256 * q, j = e >> 6, i = e & 63;
            Gr[e] = Gl[e] + 0.5 * (M0[i * LD + j] + M0[j * LD + i]);
        }
    }
}

// The top of the down-sweep: the whole range starts from the zero state, and a map applied to the zero state
// returns its own nominal end state (K = 0, v = 0) -- so  s[left half's last slot] <- 0,
// s[last slot] <- (Xbar, Ybar) of the left half's composite: a copy instead of the root's memset and one
// level of k_tree_apply (a level costs one workgroup's latency whatever it holds: 55 us).
__global__ void __launch_bounds__(256) k_tree_top(const TreeArgs A) {
    const TreeSlot l = tree_slot(A, blockIdx.x, A.P / 2 - 1), r = tree_slot(A, blockIdx.x, A.P - 1);
    for (int e = threadIdx.x; e < 4096; e += 256) { l.X[e] = 0.0; r.X[e] = l.S[e]; }
    if (threadIdx.x < 64) { l.Y[threadIdx.x] = 0.0; r.Y[threadIdx.x] = l.F[threadIdx.x]; }
}

template <int NS>
__global__ void __launch_bounds__(256) k_tree_apply(const TreeArgs A) {
    constexpr bool FULL = NS == 64;
    constexpr int LD = CbDims<NS>::LD, LA = CbDims<NS>::LA;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *Xs = lds;
    double *Au = Xs + NS * LD;
    double *Bs = Au + NS * LA;
    double *Ys = Bs + NS * LD;
    double *vs = Ys + 64;
    const int pairs = A.pairs;
    const int pr = blockIdx.x / pairs, k = blockIdx.x - pr * pairs;
    const int ir = (k + 1) * 2 * A.d - 1, il = ir - A.d;
    const TreeSlot SL = tree_slot(A, pr, il), SR = tree_slot(A, pr, ir);
    const int tid = threadIdx.x;
    double *Xr = SR.X, *Xl = SL.X;
    if (il + 1 >= A.nch) {
        // the right range is padding: nobody reads its states -- the left child inherits the parent's, no solve
        for (int e = tid; e < 4096; e += 256) Xl[e] = Xr[e];
        if (tid < 64) SL.Y[tid] = SR.Y[tid];
        return;
    }
    // s[left] <- s[right] (incoming state) ;  s[right] <- map[left](s[right])
    // (the whole slot is handed to the left child -- its padding too: state slots are not cleared between scans;
    // of the right child's slot the leading NS x NS block is rewritten, the rest holds zeros already)
    const bool in = NS == 64 || (tid & 63) < NS;
    _Pragma("unroll 16")
    for (int e = tid; e < 4096; e += 256) {
        const int j = e >> 6, i = e & 63;
        const double v = Xr[e];
        Xl[e] = v;
        if (NS == 64 || (in && j < NS)) Xs[i * LD + j] = v;
    }
    if (tid < 64) { const double v = SR.Y[tid]; SL.Y[tid] = v; Ys[tid] = v; }
    __syncthreads();
    const double noreg[16] = {};
    cb_apply<NS>(Xs, Au, Bs, Ys, vs, SL.Phi, SL.G, SL.m,
                 SL.S, SL.F, noreg, 0.0, tid, FULL ? 64 : A.n);
    if (in) {
#pragma unroll
        for (int q = 0; q < NS / 4; ++q) { const int e = tid + 256 * q, j = e >> 6, i = e & 63; Xr[e] = Xs[i * LD + j]; }
    }
    if (tid < 64) SR.Y[tid] = Ys[tid];
}

// ------------------------------------------------------------------------------------
// What the two-level combine of the stored scaled factor's linear sweeps (k_lincombine, gadfly_linear.hip) needs once
// per factor: the segments' composed transitions, and the transposes for the backward solve.  These two kernels and
// gf_chunk_segment_transitions stay in this unit although their family has left it: k_segment_transition compiles to
// one instruction more in any other unit, also with the cb_* helpers it calls moved along in a header
// (profiles/r30_isa_compare.txt), and the moves keep every kernel's instructions as they were.
// ------------------------------------------------------------------------------------
// out[m] = in[m]^T for a batch of 64 x 64 matrices (the transitions' transposes for the backward solve: once per factor)
__global__ void __launch_bounds__(256) k_transpose64(const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double tile[64][65];
    const size_t m = blockIdx.x;
    for (int e = threadIdx.x; e < 4096; e += 256) tile[e >> 6][e & 63] = in[m * 4096 + e];
    __syncthreads();
    for (int e = threadIdx.x; e < 4096; e += 256) out[m * 4096 + e] = tile[e & 63][e >> 6];
}

// Composed transition of every segment of seg_len chunks:  Psi_s = Phi_{e-1} ... Phi_{b+1} Phi_b
// (stored [j][i] like Phi).  One workgroup per segment: the running product lives in LDS (B operand
// of the MFMA tiles), the next chunk's Phi is the A operand straight from global (lanes = rows of a
// column: coalesced).
__global__ void __launch_bounds__(256)
k_segment_transition(const int nch, const int seg_len, const double *__restrict__ Phi_,
                     double *__restrict__ Psi_) {
    const int nseg = (nch + seg_len - 1) / seg_len;
    const int pr = blockIdx.x / nseg, sg = blockIdx.x - pr * nseg;
    const int c_lo = sg * seg_len, c_hi = (c_lo + seg_len < nch) ? c_lo + seg_len : nch;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    __shared__ __attribute__((aligned(16))) double Ps[64 * 64];     // row-major
    {
        const double *Pg = Phi_ + ((size_t)pr * nch + c_lo) * 4096;
        for (int e = tid; e < 4096; e += 256) Ps[(e & 63) * 64 + (e >> 6)] = Pg[e];
    }
    __syncthreads();
    for (int c = c_lo + 1; c < c_hi; ++c) {
        const double *Pg = Phi_ + ((size_t)pr * nch + c) * 4096;
        double acc[4][4];
        cb_mm(acc,
              [&](int row, int k) { return Pg[k * 64 + row]; },
              [&](int k, int col) { return Ps[k * 64 + col]; }, tx, ty);
        __syncthreads();
        cb_store_lds(Ps, 64, acc, tx, ty);
        __syncthreads();
    }
    double *Og = Psi_ + ((size_t)pr * nseg + sg) * 4096;
    for (int e = tid; e < 4096; e += 256) Og[e] = Ps[(e & 63) * 64 + (e >> 6)];
}

// ------------------------------------------------------------------------------------
// log-likelihood reductions: fixed-shape two-stage tree (deterministic)
//   stage 1: G blocks per problem -> partial (sum log d, sum z^2/d);  stage 2: one wave
// (RED_BLOCK, red_groups, steady_rows_stored and the rows' terms stand in front of k_factor7, whose steady instance
// can add its own tile: steady_tile_sums)
// ------------------------------------------------------------------------------------
// BOUNDED: the rows [0, steady_rows_stored) only, in the order the plain instance takes them; a group with no such row
// ends at once and leaves its slot of `work` alone (k_reduce2<true> does not read it)
template <bool BOUNDED>
__global__ void __launch_bounds__(RED_BLOCK) k_reduce1(int64_t N, const double *d, const double *z,
                                                       double *work, const double *steady, int64_t n_first) {
    const int b = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    const double *dp = d + (size_t)b * N;
    const double *zp = z ? z + (size_t)b * N : nullptr;
    const int64_t lim = BOUNDED ? steady_rows_stored(steady, b, N, n_first) : N;
    if (BOUNDED && (int64_t)g * RED_BLOCK >= lim) return;
    double s1 = 0.0, s2 = 0.0, mn = INFINITY;
    for (int64_t n = (int64_t)g * RED_BLOCK + threadIdx.x; n < lim; n += (int64_t)G * RED_BLOCK) {
        const double dn = dp[n];
        red_row(dn, s1, mn);
        if (zp) red_row_z(dn, zp[n], s2);
    }
    wave_sum2(s1, s2);
    mn = -wave_max(-mn);
    __shared__ double sh[RED_NACC][RED_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[0][wave] = s1; sh[1][wave] = s2; sh[2][wave] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0, t3 = INFINITY;
        for (int w = 0; w < RED_BLOCK / 64; ++w) { t1 += sh[0][w]; t2 += sh[1][w]; t3 = fmin(t3, sh[2][w]); }
        double *o = work + ((size_t)b * G + g) * RED_NACC;
        o[0] = t1; o[1] = t2; o[2] = t3;
    }
}

// acc[b] = {sum log d, sum z^2/d, min d}; init != 0 overwrites, else accumulates (tile streaming,
// fixed order).  BOUNDED: the groups that k_reduce1<true> filled (a problem that has not switched: all of them, in the
// same order)
template <bool BOUNDED>
__global__ void __launch_bounds__(64) k_reduce2(int G, const double *work, double *acc, int init,
                                                const double *steady, int64_t N, int64_t n_first) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int Gn = G;                                     // groups with rows
    if constexpr (BOUNDED) {
        const int64_t lim = steady_rows_stored(steady, b, N, n_first);
        if (lim == 0 && !init) return;
        const int64_t gl = (lim + RED_BLOCK - 1) / RED_BLOCK;
        Gn = gl < G ? (int)gl : G;
    }
    double s1 = 0.0, s2 = 0.0, mn = INFINITY;
    for (int g = lane; g < Gn; g += 64) {
        const double *w = work + ((size_t)b * G + g) * RED_NACC;
        s1 += w[0];
        s2 += w[1];
        mn = fmin(mn, w[2]);
    }
    wave_sum2(s1, s2);
    mn = -wave_max(-mn);
    if (lane == 0) {
        double *a = acc + (size_t)b * RED_NACC;
        if (!init) { s1 += a[0]; s2 += a[1]; mn = fmin(mn, a[2]); }
        a[0] = s1; a[1] = s2; a[2] = mn;
    }
}

__global__ void k_finish(int B, int64_t N, const double *acc, const int32_t *info,
                         double *out, double *logdet) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool bad = info && info[b] != 0;
    const double s1 = acc[(size_t)b * RED_NACC], s2 = acc[(size_t)b * RED_NACC + 1];
    if (logdet) logdet[b] = bad ? -INFINITY : s1;
    if (out) out[b] = bad ? -INFINITY : (-0.5 * (s1 + (double)N * 1.8378770664093453) - 0.5 * s2);
}

// wide fused sweep: NW = sweep waves for W + 1 columns (32 per wave, one spare column for the forward
// solve), TR = rows per lane = W / 4 rounded up to a multiple of 4; one more wave generates the rows
struct WideShape { int nw, tr; };
inline WideShape wide_shape(int W) {
    WideShape s;
    s.nw = (W + 1 + 31) / 32;
    s.tr = (W + 15) / 16 * 4;
    return s;
}

template <int TR, int NW, bool SAMPLE>
int launch_factorw(const FactorWArgs &A, const FactorWPtrs &P, int grid, hipStream_t st) {
    hipLaunchKernelGGL((k_factorw<TR, NW, SAMPLE>), dim3(grid), dim3(64 * (NW + 1)), 0, st, A, P.ac, P.bc, P.cc, P.dc,
                       P.diag_add, P.cmax, P.t, P.diag, P.y, P.d, P.z, P.r_out, P.Ut_out, P.Wt_out, P.de_out,
                       P.S_state, P.info);
    return 0;
}

int dispatch_factorw(const FactorWArgs &A, const FactorWPtrs &P, int W, int grid, bool sample, hipStream_t st) {
    const WideShape s = wide_shape(W);
#define GF_FW(TRv, NWv) if (s.tr == TRv && s.nw == NWv) return sample ? launch_factorw<TRv, NWv, true>(A, P, grid, st) : launch_factorw<TRv, NWv, false>(A, P, grid, st);
    GF_FW(16, 3) GF_FW(20, 3) GF_FW(24, 3)
    GF_FW(24, 4) GF_FW(28, 4) GF_FW(32, 4)
    GF_FW(32, 5) GF_FW(36, 5) GF_FW(40, 5)
    GF_FW(40, 6) GF_FW(44, 6)
#undef GF_FW
    return -1;
}


}  // namespace

// ======================================================================================
// C-ABI
// ======================================================================================
// (shared with gadfly_dense.hip: `which` = 0, 1 here, 2 and 3 there)
bool gf_internal_lds_opt_in(int which, hipStream_t st, const void *const *funcs, int nfuncs, size_t bytes) {
    static std::atomic<bool> done[4][64];
    if (which < 0 || which >= 4) return false;
    int dev = -1;
    if (st == nullptr || hipStreamGetDevice(st, &dev) != hipSuccess) {
        if (hipGetDevice(&dev) != hipSuccess) return false;
    }
    if (dev < 0 || dev >= 64) return false;
    if (done[which][dev].load(std::memory_order_acquire)) return true;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return false;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return false;
    bool ok = true;
    for (int i = 0; i < nfuncs; ++i)
        ok = ok && hipFuncSetAttribute(funcs[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
    if (cur != dev) (void)hipSetDevice(cur);
    if (ok) done[which][dev].store(true, std::memory_order_release);
    return ok;
}


extern "C" {

int gf_version(void) { return 100; }

const char *gf_last_error(void) { return g_err; }

// Fused sweeps exist for W <= 63 (any mix of terms) and, for kernels of complex terms only, up to
// W = 176 (k_factorw).  gf_fused_state_size: doubles of S_state per (problem, chunk) slot.
int gf_fused_supported(int Jr, int Jc) {
    const int W = Jr + 2 * Jc;
    if (Jr < 0 || Jc < 0 || W < 1) return 0;
    if (W <= 63) return 1;
    return (Jr == 0 && W <= 176) ? 1 : 0;
}

int64_t gf_fused_state_size(int Jr, int Jc) {
    if (!gf_fused_supported(Jr, Jc)) return -1;
    const int W = Jr + 2 * Jc;
    if (W <= 63) return 64 * 64;
    const WideShape ws = wide_shape(W);
    return (int64_t)(32 * ws.nw) * (4 * ws.tr);                                // [columns][rows], padded
}

// which fused sweep runs (argument `variant` of gf_loglike_fused / gf_chunk_sweep / gf_chunk_transition)
//   GF_SWEEP_AUTO   the lane-tiled k_factor7 / k_phi7 for kernels of complex terms only (Jr = 0,
//                   Jc <= 31: every gadfly kernel with Q >= 1/2), k_factor3 / k_phi otherwise
//   GF_SWEEP_COLUMN k_factor3 / k_phi (one column per lane), any term mix
//   GF_SWEEP_TILED  k_factor7 / k_phi7; an error if the term structure does not allow it
static bool sweep_tiled(int variant, int Jr, int Jc) {
    return variant != GF_SWEEP_COLUMN && Jr == 0 && Jc <= 31;
}

static int check_sweep_options(const char *who, int gen_period, int variant, int Jr, int Jc) {
    if (gen_period < 1 || gen_period > 64 || (gen_period & (gen_period - 1)))
        return gf_internal_error(-1, "%s: gen_period=%d must be a power of two in 1..64", who, gen_period);
    if (variant < GF_SWEEP_AUTO || variant > GF_SWEEP_TILED)
        return gf_internal_error(-1, "%s: unknown sweep variant %d", who, variant);
    if (variant == GF_SWEEP_TILED && !(Jr == 0 && Jc <= 31))
        return gf_internal_error(-1, "%s: GF_SWEEP_TILED needs complex terms only (Jr = 0) and Jc <= 31 (Jc=%d)", who, Jc);
    return 0;
}

// One call of a fused sweep.  sweep_call() fills what the seven sweep entry points share, their leading arguments;
// the rest stands for the streamed log-likelihood sweep (one chunk, no rows stored) until an entry point says otherwise.
struct SweepCall {
    const char *who;
    int B, Jr, Jc, block, gen_period, variant;
    int64_t N, n_first;
    const double *ar, *cr, *ac, *bc, *cc, *dc, *diag_add, *cmax;        // kernel coefficients
    const double *t, *diag, *y;                                         // series, with their batch strides
    int64_t t_bs, diag_bs, y_bs;
    double *d, *z, *S_state, *F_state;
    int32_t *info;
    hipStream_t st;
    int64_t chunk_len;                                                  // chunks of a time-parallel pass ...
    int nch = 1, chunk_first = 0, chunk_count = 1;
    double *r_out = nullptr, *Ut_out = nullptr, *Wt_out = nullptr, *de_out = nullptr;      // ... and the rows it stores
    bool sample = false;                // y = eps, z = the draw by global row with y's batch stride
    double *steady = nullptr;           // steady mode: the switch records, armed from row arm_from on
    int64_t arm_from = 0;
    bool tail = true;                   // k_steady_tail behind the sweep, for the tile's rows behind the switch row
    double *acc = nullptr;              // the sweep's own sums (acc_init != 0 overwrites them, 0 accumulates): the
    int acc_init = 0;                   // steady instance without its tail kernel only
};

static SweepCall sweep_call(const char *who, int B, int64_t N, int64_t n_first, int Jr, int Jc, int block, int gen_period,
                            int variant, const double *ar, const double *cr, const double *ac, const double *bc,
                            const double *cc, const double *dc, const double *diag_add, const double *cmax,
                            const double *t, int64_t t_bs, const double *diag, int64_t diag_bs, const double *y,
                            int64_t y_bs, double *d, double *z, double *S_state, double *F_state, int32_t *info,
                            void *stream) {
    SweepCall c;
    c.who = who; c.B = B; c.N = N; c.n_first = n_first; c.Jr = Jr; c.Jc = Jc;
    c.block = block; c.gen_period = gen_period; c.variant = variant;
    c.ar = ar; c.cr = cr; c.ac = ac; c.bc = bc; c.cc = cc; c.dc = dc; c.diag_add = diag_add; c.cmax = cmax;
    c.t = t; c.t_bs = t_bs; c.diag = diag; c.diag_bs = diag_bs; c.y = y; c.y_bs = y_bs;
    c.d = d; c.z = z; c.S_state = S_state; c.F_state = F_state; c.info = info; c.st = (hipStream_t)stream;
    c.chunk_len = N;
    return c;
}

static int launch_sweep(const SweepCall &c) {
    const char *who = c.who;
    const int W = c.Jr + 2 * c.Jc;
    const bool rowstore = c.r_out || c.Ut_out || c.Wt_out || c.de_out;
    if (c.B < 1 || c.N < 1) return gf_internal_error(-1, "%s: empty problem (N=%lld)", who, (long long)c.N);
    // the sampling sweeps: streamed tiles only
    if (c.sample && (c.nch > 1 || rowstore || (c.variant & GF_SWEEP_ZERO_START) || (c.B > 1 && c.y_bs < 1)))
        return gf_internal_error(-1, "%s: one chunk, no row outputs, and a batch stride for eps / out (eps_bs=%lld)", who,
                                 (long long)c.y_bs);
    // (u~ rows / reset spans and the w~ rows are stored independently: a nominal pass needs no w~ rows)
    if ((c.Ut_out != nullptr) != (c.de_out != nullptr) || (c.Wt_out && !c.Ut_out))
        return gf_internal_error(-1, "%s: Ut_out and de_out go together, Wt_out needs them", who);
    if (!gf_fused_supported(c.Jr, c.Jc))
        return gf_internal_error(-1, "%s: width %d unsupported (1..63 any terms; 64..176 complex terms only)", who, W);
    if (check_block(who, c.block) || check_n_first(who, c.n_first, c.block)
        || check_chunking(who, c.N, c.chunk_len, c.nch, c.block)
        || check_chunk_range(who, c.chunk_first, c.chunk_count, c.nch)) return -1;
    if (!c.t || !c.y || !c.d || !c.z || !c.S_state || (!c.F_state && W <= 63) || !c.info || !c.diag_add || !c.cmax)
        return gf_internal_error(-1, "%s: null pointer", who);
    const int zero_start = (c.variant & GF_SWEEP_ZERO_START) ? (1 << 30) : 0;
    const bool long_span = (c.variant & GF_SWEEP_LONG_SPAN) != 0;
    const int variant = c.variant & ~(GF_SWEEP_ZERO_START | GF_SWEEP_LONG_SPAN);
    if (long_span && (W > 63 || c.nch > 1 || rowstore))
        return gf_internal_error(-1, "%s: GF_SWEEP_LONG_SPAN is for the streamed one-wave sweep only (W <= 63, one chunk, no row outputs)", who);
    if (check_sweep_options(who, c.gen_period, W > 63 ? GF_SWEEP_AUTO : variant, c.Jr, c.Jc)) return -1;
    if (c.chunk_count == 0) return 0;
    const bool tiled = sweep_tiled(variant, c.Jr, c.Jc);
    const double gap = sweep_gap(c.block, c.variant);
    const int block_sub = c.block | (c.gen_period << 8) | zero_start;
    if (c.steady && (W > 63 || !tiled || rowstore || c.sample || zero_start || c.nch > 1 || c.arm_from < 0))
        return gf_internal_error(-1, "%s: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=%d)", who, c.Jc);
    if (c.acc && (!c.steady || c.tail))
        return gf_internal_error(-1, "%s: acc goes with the steady sweep alone", who);
    if (W > 63) {                       // wide kernels: one workgroup per (problem, chunk), k_factorw
        FactorWArgs A;
        A.N = c.N; A.n_first = c.n_first; A.chunk_len = c.chunk_len; A.nch = c.nch; A.ch0 = c.chunk_first;
        A.nsel = c.chunk_count; A.Jc = c.Jc; A.block_sub = block_sub; A.gap = gap;
        A.t_bs = c.t_bs; A.diag_bs = c.diag_bs; A.y_bs = c.y_bs;
        FactorWPtrs P;
        P.ac = c.ac; P.bc = c.bc; P.cc = c.cc; P.dc = c.dc; P.diag_add = c.diag_add; P.cmax = c.cmax;
        P.t = c.t; P.diag = c.diag; P.y = c.y;
        P.d = c.d; P.z = c.z; P.r_out = c.r_out; P.Ut_out = c.Ut_out; P.Wt_out = c.Wt_out; P.de_out = c.de_out;
        P.S_state = c.S_state; P.info = c.info;
        if (dispatch_factorw(A, P, W, c.B * c.chunk_count, c.sample, c.st))
            return gf_internal_error(-1, "%s: internal dispatch error (wide)", who);
        return check_launch(who);
    }
    // what every one-wave instance takes; k_factor7 then its four steady-mode arguments
    auto launch = [&](auto kernel, auto... steady_mode) {
        hipLaunchKernelGGL(kernel, dim3(c.B * c.chunk_count), dim3(64), 0, c.st, c.N, c.n_first, c.chunk_len, c.nch,
                           c.chunk_first, c.chunk_count, c.Jr, c.Jc, block_sub, gap, c.ar, c.cr, c.ac, c.bc, c.cc, c.dc,
                           c.diag_add, c.cmax, c.t, c.t_bs, c.diag, c.diag_bs, c.y, c.y_bs, c.d, c.z, c.r_out,
                           c.Ut_out, c.Wt_out, c.de_out, c.S_state, c.F_state, c.info, steady_mode...);
    };
    const int rows = (W + 3) / 4 * 4;
    double *const none = nullptr;
    if (!dispatch_rows(rows, [&](auto r) {
            constexpr int R = decltype(r)::value;
            if (c.steady)      launch(k_factor7<R, false, false, true>, c.steady, c.arm_from, c.acc, c.acc_init);
            else if (!tiled)   c.sample ? launch(k_factor3<R, true>) : launch(k_factor3<R>);
            else if (c.sample) launch(k_factor7<R, false, true>, none, (int64_t)0, none, 0);
            else if (rowstore) launch(k_factor7<R, true>, none, (int64_t)0, none, 0);
            else               launch(k_factor7<R, false>, none, (int64_t)0, none, 0);
        }))
        return gf_internal_error(-1, "%s: internal dispatch error", who);
    if (c.steady && c.tail) {           // the rows of this tile behind each problem's switch row (same stream)
        if (const int e = check_launch(who)) return e;
        dispatch_rows(rows, [&](auto r) {
            hipLaunchKernelGGL((k_steady_tail<decltype(r)::value>), dim3(c.B), dim3(64), 0, c.st, c.N, c.n_first, c.Jc,
                               gap, c.ac, c.bc, c.cc, c.dc, c.cmax, c.t, c.t_bs, c.y, c.y_bs, c.d, c.z, c.info, c.steady);
        });
    }
    return check_launch(who);
}

int gf_loglike_fused(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                     int gen_period, int variant,
                     const double *ar, const double *cr, const double *ac,
                     const double *bc, const double *cc, const double *dc,
                     const double *diag_add, const double *cmax,
                     const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                     const double *y, int64_t y_bs,
                     double *d, double *z, double *S_state, double *F_state,
                     int32_t *info, void *stream) {
    return launch_sweep(sweep_call("gf_loglike_fused", B, N, n_first, Jr, Jc, block, gen_period, variant, ar, cr, ac, bc,
                                   cc, dc, diag_add, cmax, t, t_bs, diag, diag_bs, y, y_bs, d, z, S_state, F_state,
                                   info, stream));
}

int64_t gf_steady_size(void) { return ST_SIZE; }

int gf_loglike_steady(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                      int gen_period, int variant,
                      const double *ar, const double *cr, const double *ac,
                      const double *bc, const double *cc, const double *dc,
                      const double *diag_add, const double *cmax,
                      const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                      const double *y, int64_t y_bs,
                      double *d, double *z, double *S_state, double *F_state,
                      int32_t *info, double *steady, int64_t arm_from, void *stream) {
    if (!steady) return gf_internal_error(-1, "gf_loglike_steady: null pointer");
    SweepCall c = sweep_call("gf_loglike_steady", B, N, n_first, Jr, Jc, block, gen_period, variant, ar, cr, ac, bc, cc, dc,
                             diag_add, cmax, t, t_bs, diag, diag_bs, y, y_bs, d, z, S_state, F_state, info, stream);
    c.steady = steady; c.arm_from = arm_from;
    return launch_sweep(c);
}

int gf_steady_sweep(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                    int gen_period, int variant,
                    const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc,
                    const double *diag_add, const double *cmax,
                    const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                    const double *y, int64_t y_bs,
                    double *d, double *z, double *S_state, double *F_state,
                    int32_t *info, double *steady, int64_t arm_from, void *stream) {
    if (!steady) return gf_internal_error(-1, "gf_steady_sweep: null pointer");
    SweepCall c = sweep_call("gf_steady_sweep", B, N, n_first, Jr, Jc, block, gen_period, variant, ar, cr, ac, bc, cc, dc,
                             diag_add, cmax, t, t_bs, diag, diag_bs, y, y_bs, d, z, S_state, F_state, info, stream);
    c.steady = steady; c.arm_from = arm_from; c.tail = false;
    return launch_sweep(c);
}

int gf_steady_sweep_reduced(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                            int gen_period, int variant,
                            const double *ar, const double *cr, const double *ac,
                            const double *bc, const double *cc, const double *dc,
                            const double *diag_add, const double *cmax,
                            const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                            const double *y, int64_t y_bs,
                            double *d, double *z, double *S_state, double *F_state,
                            int32_t *info, double *steady, int64_t arm_from, double *acc, int init, void *stream) {
    if (!steady || !acc) return gf_internal_error(-1, "gf_steady_sweep_reduced: null pointer");
    SweepCall c = sweep_call("gf_steady_sweep_reduced", B, N, n_first, Jr, Jc, block, gen_period, variant, ar, cr, ac, bc,
                             cc, dc, diag_add, cmax, t, t_bs, diag, diag_bs, y, y_bs, d, z, S_state, F_state, info, stream);
    c.steady = steady; c.arm_from = arm_from; c.tail = false; c.acc = acc; c.acc_init = init ? 1 : 0;
    return launch_sweep(c);
}

int gf_steady_sweep_rank1(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                          int gen_period, int variant,
                          const double *ar, const double *cr, const double *ac,
                          const double *bc, const double *cc, const double *dc,
                          const double *diag_add, const double *cmax,
                          const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                          const double *y, int64_t y_bs,
                          double *d, double *z, double *S_state, double *F_state,
                          int32_t *info, double *steady, int64_t arm_from, double *acc, int init,
                          const double *dt, void *stream) {
    // (the arguments of gf_steady_sweep_reduced: no real terms, no forward-solve slot -- ar, cr, F_state are not read)
    const SweepCall c = sweep_call("gf_steady_sweep_rank1", B, N, n_first, Jr, Jc, block, gen_period, variant, ar, cr, ac,
                                   bc, cc, dc, diag_add, cmax, t, t_bs, diag, diag_bs, y, y_bs, d, z, S_state, F_state,
                                   info, stream);
    const char *who = c.who;
    if (B < 1 || N < 1) return gf_internal_error(-1, "%s: empty problem (N=%lld)", who, (long long)N);
    if (check_block(who, block) || check_n_first(who, n_first, block)) return -1;
    if (!t || !y || !d || !z || !S_state || !info || !diag_add || !cmax || !ac || !bc || !cc || !dc || !steady || !dt)
        return gf_internal_error(-1, "%s: null pointer", who);
    if (check_sweep_options(who, gen_period, variant & ~(GF_SWEEP_ZERO_START | GF_SWEEP_LONG_SPAN), Jr, Jc)) return -1;
    if ((variant & GF_SWEEP_ZERO_START) || !sweep_tiled(variant & ~GF_SWEEP_LONG_SPAN, Jr, Jc) || Jc < 1 || arm_from < 0)
        return gf_internal_error(-1, "%s: steady mode is for the streamed lane-tiled sweep only (Jr = 0, Jc <= 31; Jc=%d)", who, Jc);
    hipLaunchKernelGGL(k_steady_rank1, dim3(c.B), dim3(64), 0, c.st, c.N, c.n_first, c.Jc, sweep_gap(block, variant),
                       c.ac, c.bc, c.cc, c.dc, c.diag_add, c.cmax, c.t, c.t_bs, c.diag, c.diag_bs, c.y, c.y_bs, c.d, c.z,
                       c.S_state, c.info, steady, arm_from, dt, acc, init ? 1 : 0);
    return check_launch(who);
}

// what the finishing launches check first, and their window of switch rows
static int check_finish(const char *who, int B, int64_t N, int Jr, int Jc, int block) {
    if (B < 1 || N < 1) return gf_internal_error(-1, "%s: empty problem (B=%d, N=%lld)", who, B, (long long)N);
    if (Jr != 0 || Jc < 1 || Jc > 31)
        return gf_internal_error(-1, "%s: steady mode is for the lane-tiled sweep only (Jr = 0, Jc <= 31; Jr=%d, Jc=%d)", who, Jr, Jc);
    return check_block(who, block);
}
static int check_window(const char *who, int64_t sw_lo, int64_t sw_hi) {
    if (sw_lo < 0 || sw_hi < sw_lo)
        return gf_internal_error(-1, "%s: the window of switch rows needs 0 <= sw_lo <= sw_hi (sw_lo=%lld, sw_hi=%lld)", who,
                                 (long long)sw_lo, (long long)sw_hi);
    return 0;
}

static int steady_finish_launch(const char *who, int B, int64_t N, int Jr, int Jc, int block, int variant,
                                const double *ac, const double *bc, const double *cc, const double *dc,
                                const double *cmax, const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                                const int32_t *info, double *steady, double *acc, int64_t sw_lo, int64_t sw_hi,
                                void *stream) {
    if (check_finish(who, B, N, Jr, Jc, block)) return -1;
    if (!ac || !bc || !cc || !dc || !cmax || !t || !y || !info || !steady || !acc)
        return gf_internal_error(-1, "%s: null pointer", who);
    if (check_window(who, sw_lo, sw_hi)) return -1;
    if (sw_lo == sw_hi) return 0;       // an empty window: no launch
    const double gap = sweep_gap(block, variant & ~GF_SWEEP_AXIS_PROVEN);   // the sweep's
    const bool proven = (variant & GF_SWEEP_AXIS_PROVEN) != 0;
    if (!dispatch_rows((2 * Jc + 3) / 4 * 4, [&](auto r) {
            constexpr int R = decltype(r)::value;
            hipLaunchKernelGGL((proven ? k_steady_finish<R, true> : k_steady_finish<R, false>), dim3(B), dim3(64), 0,
                               (hipStream_t)stream, N, Jc, gap, ac, bc, cc, dc, cmax, t, t_bs, y, y_bs, info, steady, acc,
                               sw_lo, sw_hi);
        }))
        return gf_internal_error(-1, "%s: internal dispatch error", who);
    return check_launch(who);
}

int gf_steady_finish(int B, int64_t N, int Jr, int Jc, int block, int variant,
                     const double *ac, const double *bc, const double *cc, const double *dc, const double *cmax,
                     const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                     const int32_t *info, double *steady, double *acc, void *stream) {
    return steady_finish_launch("gf_steady_finish", B, N, Jr, Jc, block, variant, ac, bc, cc, dc, cmax, t, t_bs, y, y_bs,
                                info, steady, acc, 0, INT64_MAX, stream);
}

int gf_steady_finish_window(int B, int64_t N, int Jr, int Jc, int block, int variant,
                            const double *ac, const double *bc, const double *cc, const double *dc, const double *cmax,
                            const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                            const int32_t *info, double *steady, double *acc,
                            int64_t sw_lo, int64_t sw_hi, void *stream) {
    return steady_finish_launch("gf_steady_finish_window", B, N, Jr, Jc, block, variant, ac, bc, cc, dc, cmax, t, t_bs,
                                y, y_bs, info, steady, acc, sw_lo, sw_hi, stream);
}

int64_t gf_steady_chunk_size(int64_t N, int chunk_blocks) {
    if (N < 1 || chunk_blocks < 1) return 0;
    const int64_t chunk_rows = 64 * (int64_t)chunk_blocks;
    return CH_P + (N + chunk_rows - 1) / chunk_rows * CH_SLOT;
}

int gf_steady_finish_chunked(int B, int64_t N, int Jr, int Jc, int block, int variant,
                             const double *ac, const double *bc, const double *cc, const double *dc, const double *cmax,
                             const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                             const int32_t *info, double *steady, double *acc,
                             int64_t sw_lo, int64_t sw_hi, int chunk_blocks, double *chunk_ws, void *stream) {
    const char *who = "gf_steady_finish_chunked";
    if (check_finish(who, B, N, Jr, Jc, block)) return -1;
    if (!ac || !bc || !cc || !dc || !cmax || !t || !y || !info || !steady || !acc || !chunk_ws)
        return gf_internal_error(-1, "%s: null pointer", who);
    if (check_window(who, sw_lo, sw_hi)) return -1;
    if (chunk_blocks < 16 || (chunk_blocks & (chunk_blocks - 1)))
        return gf_internal_error(-1, "%s: chunk_blocks=%d must be a power of two >= 16 (chunks start on the groups' grid)", who, chunk_blocks);
    if (sw_lo == sw_hi) return 0;       // an empty window: no launch
    const double gap = sweep_gap(block, variant & ~GF_SWEEP_AXIS_PROVEN);   // the sweep's
    const bool proven = (variant & GF_SWEEP_AXIS_PROVEN) != 0;
    const int64_t chunk_rows = 64 * (int64_t)chunk_blocks, ws_ld = gf_steady_chunk_size(N, chunk_blocks);
    const int64_t nmax64 = (N + chunk_rows - 1) / chunk_rows;
    if (nmax64 > 65535)
        return gf_internal_error(-1, "%s: %lld chunks per problem are more than a launch takes", who, (long long)nmax64);
    const int nmax = (int)nmax64;
    int squarings = 0;
    while ((1 << squarings) < chunk_blocks) ++squarings;
    hipStream_t st = (hipStream_t)stream;
    if (!dispatch_rows((2 * Jc + 3) / 4 * 4, [&](auto r) {
            constexpr int R = decltype(r)::value;
            auto pass = [&](auto kernel, dim3 grid) {
                hipLaunchKernelGGL(kernel, grid, dim3(64), 0, st, N, Jc, gap, ac, bc, cc, dc, cmax, t, t_bs, y, y_bs, info,
                                   steady, sw_lo, sw_hi, chunk_rows, chunk_ws, ws_ld);
            };
            pass(k_steady_chunk<R, 3>, dim3(B));
            pass(proven ? k_steady_chunk<R, 1, true> : k_steady_chunk<R, 1, false>, dim3(B, nmax));
            hipLaunchKernelGGL(k_steady_chunk_power, dim3(B), dim3(256), 0, st, N, info, steady, sw_lo, sw_hi, chunk_rows,
                               squarings, chunk_ws, ws_ld);
            pass(proven ? k_steady_chunk<R, 2, true> : k_steady_chunk<R, 2, false>, dim3(B, nmax));
        }))
        return gf_internal_error(-1, "%s: internal dispatch error", who);
    hipLaunchKernelGGL(k_steady_chunk_sum, dim3((B + 63) / 64), dim3(64), 0, st, B, N, info, steady, sw_lo, sw_hi,
                       chunk_rows, chunk_ws, ws_ld, acc);
    return check_launch(who);
}

int gf_sample_fused(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                    int gen_period, int variant,
                    const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc,
                    const double *diag_add, const double *cmax,
                    const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                    const double *eps, int64_t eps_bs,
                    double *d, double *out, double *S_state, double *F_state,
                    int32_t *info, void *stream) {
    SweepCall c = sweep_call("gf_sample_fused", B, N, n_first, Jr, Jc, block, gen_period, variant, ar, cr, ac, bc, cc, dc,
                             diag_add, cmax, t, t_bs, diag, diag_bs, eps, eps_bs, d, out, S_state, F_state, info, stream);
    c.sample = true;
    return launch_sweep(c);
}

int gf_chunk_sweep(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count,
                   int Jr, int Jc, int block, int gen_period, int variant,
                   const double *ar, const double *cr, const double *ac,
                   const double *bc, const double *cc, const double *dc,
                   const double *diag_add, const double *cmax,
                   const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                   const double *y, int64_t y_bs,
                   double *d, double *z, double *r_out, double *Ut_out, double *Wt_out,
                   double *de_out, double *S_state, double *F_state,
                   int32_t *info, void *stream) {
    SweepCall c = sweep_call("gf_chunk_sweep", B, N, 0, Jr, Jc, block, gen_period, variant, ar, cr, ac, bc, cc, dc,
                             diag_add, cmax, t, t_bs, diag, diag_bs, y, y_bs, d, z, S_state, F_state, info, stream);
    c.chunk_len = chunk_len; c.nch = nch; c.chunk_first = chunk_first; c.chunk_count = chunk_count;
    c.r_out = r_out; c.Ut_out = Ut_out; c.Wt_out = Wt_out; c.de_out = de_out;
    return launch_sweep(c);
}

int gf_chunk_transition(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count,
                        int Jr, int Jc, int variant, const double *c, const double *de, const double *dbar,
                        const double *zbar, const double *rbar, const double *Ut,
                        double *Phi_out, double *G_out, double *m_out, void *stream) {
    const char *who = "gf_chunk_transition";
    const int W = Jr + 2 * Jc;
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_chunk_transition: empty problem (N=%lld)", (long long)N);
    if (W < 1 || W > 63) return gf_internal_error(-1, "gf_chunk_transition: width %d unsupported (1..63)", W);
    if (check_chunking(who, N, chunk_len, nch, 64) || check_chunk_range(who, chunk_first, chunk_count, nch)) return -1;
    if (!c || !de || !dbar || !zbar || !rbar || !Ut || !Phi_out || !G_out || !m_out)
        return gf_internal_error(-1, "gf_chunk_transition: null pointer");
    if (check_sweep_options(who, 1, variant, Jr, Jc)) return -1;
    if (chunk_count == 0) return 0;
    const bool tiled = sweep_tiled(variant, Jr, Jc);
    if (!dispatch_rows((W + 3) / 4 * 4, [&](auto r) {
            constexpr int R = decltype(r)::value;
            hipLaunchKernelGGL((tiled ? k_phi7<R> : k_phi<R>), dim3(B * chunk_count), dim3(64), 0, (hipStream_t)stream, N,
                               chunk_len, nch, chunk_first, chunk_count, W, c, de, dbar, zbar, rbar, Ut, Phi_out, G_out,
                               m_out);
        }))
        return gf_internal_error(-1, "gf_chunk_transition: internal dispatch error");
    return check_launch(who);
}


static int cb_ns(int W) { return W > 48 ? 64 : (W > 32 ? 48 : 32); }
static size_t cb_lds_bytes(int W) {      // 48 x 48 matrices: two workgroups per CU; 32 x 32: four
    const int NS = cb_ns(W);
    return sizeof(double) * ((size_t)NS * (2 * (NS + 1) + 2 * NS + 2) + 256);
}

int gf_chunk_combine(int B, int nch, int W, const double *Phi, const double *G, const double *m,
                     double *S_state, double *F_state, void *stream) {
    if (B < 1 || nch < 1) return gf_internal_error(-1, "gf_chunk_combine: empty problem");
    if (W < 1 || W > 64) return gf_internal_error(-1, "gf_chunk_combine: width %d unsupported (1..64)", W);
    if (!Phi || !G || !m || !S_state || !F_state) return gf_internal_error(-1, "gf_chunk_combine: null pointer");
    const size_t lds = cb_lds_bytes(W);
    const void *fn[3] = {(const void *)k_combine<64>, (const void *)k_combine<48>, (const void *)k_combine<32>};
    hipStream_t st = (hipStream_t)stream;
    // (the > 64 KB dynamic-LDS opt-in is per device, the one the STREAM belongs to: gf_internal_lds_opt_in)
    if (!gf_internal_lds_opt_in(0, st, fn, 3, cb_lds_bytes(64)))
        return gf_internal_error(-1, "gf_chunk_combine: cannot opt in to %lld bytes of LDS", (long long)lds);
    dispatch_among<64, 48, 32>(cb_ns(W), [&](auto ns) {
        hipLaunchKernelGGL(k_combine<decltype(ns)::value>, dim3(B), dim3(256), lds, st, nch, W, Phi, G, m, S_state, F_state);
    });
    return check_launch("gf_chunk_combine");
}

// Tree (log-depth) version of gf_chunk_combine, on the same arrays [B * nch] (Phi, G, m and S/F = the nominal end
// states; Xst/Yst [B * nch] receive the TRUE start states).  The scan works on P slots per problem, P the power of
// two with P / 2 < nch <= P: the slots beyond nch stand for identity maps and are never read (a pair whose right
// range is padding copies its left map, one that is padding altogether is not launched); what the scan writes at
// such an index -- composites that reach into the padding, their states -- lives in `work`
// (gf_chunk_combine_tree_work doubles).  The map arrays are overwritten.
int64_t gf_chunk_combine_tree_work(int B, int P, int nch) {
    if (B < 1 || P < 2 || nch < 1 || nch > P) return -1;
    const int64_t n = (int64_t)B * (P - nch);
    return n * (4 * 4096 + 3 * 64) + 8;
}

int gf_chunk_combine_tree(int B, int P, int nch, int W, double *Phi, double *G, double *m, double *S, double *F,
                          double *Xst, double *Yst, double *work, void *stream) {
    if (B < 1 || P < 2 || (P & (P - 1))) return gf_internal_error(-1, "gf_chunk_combine_tree: P=%d must be a power of two >= 2", P);
    if (nch <= P / 2 || nch > P) return gf_internal_error(-1, "gf_chunk_combine_tree: nch=%d must lie in (P / 2, P]", nch);
    if (W < 1 || W > 64) return gf_internal_error(-1, "gf_chunk_combine_tree: width %d unsupported (1..64)", W);
    if (!Phi || !G || !m || !S || !F || !Xst || !Yst || !work) return gf_internal_error(-1, "gf_chunk_combine_tree: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = cb_lds_bytes(W);
    const void *fn[6] = {(const void *)k_tree_compose<64>, (const void *)k_tree_apply<64>,
                         (const void *)k_tree_compose<48>, (const void *)k_tree_apply<48>,
                         (const void *)k_tree_compose<32>, (const void *)k_tree_apply<32>};
    if (!gf_internal_lds_opt_in(1, st, fn, 6, cb_lds_bytes(64))) return gf_internal_error(-1, "gf_chunk_combine_tree: cannot opt in to %lld bytes of LDS", (long long)lds);
    TreeArgs A;
    A.P = P; A.n = W; A.nch = nch; A.Phi = Phi; A.G = G; A.S = S; A.F = F; A.m = m; A.Xst = Xst; A.Yst = Yst;
    {
        const size_t no = (size_t)B * (P - nch);
        A.oPhi = work; A.oG = A.oPhi + no * 4096; A.oS = A.oG + no * 4096; A.oX = A.oS + no * 4096;
        A.oF = A.oX + no * 4096; A.om = A.oF + no * 64; A.oY = A.om + no * 64;
    }
    const int ns = cb_ns(W);
    // pairs of a level whose left range [2 d k, 2 d k + d - 1] holds a real chunk; the rest is padding: not launched
    auto real_pairs = [&](int d) { return (nch + 2 * d - 1) / (2 * d); };
    // up-sweep.  Its top level would compose the whole range into the last slot -- a map the down-sweep never
    // applies (it uses LEFT children only): left out, one level's latency less
    for (int d = 1; d < P / 2; d *= 2) {
        A.d = d; A.pairs = real_pairs(d);
        dispatch_among<64, 48, 32>(ns, [&](auto s) {
            hipLaunchKernelGGL(k_tree_compose<decltype(s)::value>, dim3(B * A.pairs), dim3(256), lds, st, A);
        });
    }
    A.d = P / 2; A.pairs = 1;
    hipLaunchKernelGGL(k_tree_top, dim3(B), dim3(256), 0, st, A);                    // root state = zero, first level
    for (int d = P / 4; d >= 1; d /= 2) {   // down-sweep
        A.d = d; A.pairs = real_pairs(d);
        dispatch_among<64, 48, 32>(ns, [&](auto s) {
            hipLaunchKernelGGL(k_tree_apply<decltype(s)::value>, dim3(B * A.pairs), dim3(256), lds, st, A);
        });
    }
    return check_launch("gf_chunk_combine_tree");
}

int gf_chunk_transition_wide(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count,
                             int Jc, const double *c, const double *de, const double *dbar, const double *rbar,
                             const double *Ut, double *h_out, double *Phi_out, void *stream) {
    const int W = 2 * Jc;
    if (check_chunk_range("gf_chunk_transition_wide", chunk_first, chunk_count, nch)) return -1;
    if (chunk_count == 0) return 0;
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_chunk_transition_wide: empty problem (N=%lld)", (long long)N);
    if (W <= 63 || !gf_fused_supported(0, Jc)) return gf_internal_error(-1, "gf_chunk_transition_wide: width %d unsupported (64..176)", W);
    if (check_chunking("gf_chunk_transition_wide", N, chunk_len, nch, 64)) return -1;
    if (!c || !de || !dbar || !rbar || !Ut || !h_out || !Phi_out) return gf_internal_error(-1, "gf_chunk_transition_wide: null pointer");
    const WideShape ws = wide_shape(W);
    const int CP = 32 * ws.nw, tr8 = ws.tr / 2;     // rows per lane with 8 row groups
    const int64_t grid = (int64_t)B * chunk_count * ((W + 15) / 16);
    if (grid > 0x7fffffffLL) return gf_internal_error(-1, "gf_chunk_transition_wide: problem too large");
    hipStream_t st = (hipStream_t)stream;
    // one kilobyte per row vector while the row, its pivot pair and its reset-span pair fit (CP <= 124), else two
    const int ni = (CP * 8 + 32 <= 1024) ? 1 : 2;
#define GF_PW(TRv, Dv, NIv) if (tr8 == TRv && ni == NIv) { hipLaunchKernelGGL((k_phiw<TRv, Dv, NIv>), dim3((unsigned)grid), dim3(64), 0, st, N, chunk_len, nch, chunk_first, chunk_count, W, CP, c, de, dbar, rbar, Ut, h_out, Phi_out); return check_launch("gf_chunk_transition_wide"); }
    GF_PW(8, 4, 1) GF_PW(10, 4, 1) GF_PW(12, 4, 1)
    GF_PW(12, 4, 2) GF_PW(14, 4, 2) GF_PW(16, 4, 2) GF_PW(18, 4, 2) GF_PW(20, 4, 2) GF_PW(22, 4, 2)
#undef GF_PW
    return gf_internal_error(-1, "gf_chunk_transition_wide: internal dispatch error");
}

// leading dimension of the rows gf_chunk_sweep stores (Ut_out, Wt_out, r_out): 64 for W <= 63, the padded
// column count of the wide sweep beyond
int gf_fused_row_stride(int Jr, int Jc) {
    if (!gf_fused_supported(Jr, Jc)) return -1;
    const int W = Jr + 2 * Jc;
    return (W <= 63) ? 64 : 32 * wide_shape(W).nw;
}

int gf_chunk_segment_transitions(int B, int nch, int seg_len, const double *Phi, double *Psi_out,
                                 double *PhiT_out, double *PsiT_out, void *stream) {
    if (B < 1 || nch < 1 || seg_len < 1) return gf_internal_error(-1, "gf_chunk_segment_transitions: empty problem");
    if (!Phi || !Psi_out || ((PhiT_out != nullptr) != (PsiT_out != nullptr)))
        return gf_internal_error(-1, "gf_chunk_segment_transitions: null pointer (PhiT_out and PsiT_out go together)");
    const int nseg = (nch + seg_len - 1) / seg_len;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_segment_transition, dim3(B * nseg), dim3(256), 0, st, nch, seg_len, Phi, Psi_out);
    if (PhiT_out) {
        hipLaunchKernelGGL(k_transpose64, dim3(B * nch), dim3(256), 0, st, Phi, PhiT_out);
        hipLaunchKernelGGL(k_transpose64, dim3(B * nseg), dim3(256), 0, st, (const double *)Psi_out, PsiT_out);
    }
    return check_launch("gf_chunk_segment_transitions");
}

int64_t gf_reduce_work(int64_t N) { return RED_NACC * (int64_t)red_groups(N); }

int gf_reduce_tile(int B, int64_t N, const double *d, const double *z,
                   double *work, double *acc, int init, void *stream) {
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_reduce_tile: empty problem (B=%d, N=%lld)", B, (long long)N);
    if (!d || !work || !acc) return gf_internal_error(-1, "gf_reduce_tile: null pointer");
    const int G = red_groups(N);
    hipLaunchKernelGGL(k_reduce1<false>, dim3(G, B), dim3(RED_BLOCK), 0, (hipStream_t)stream, N, d, z, work,
                       (const double *)nullptr, (int64_t)0);
    hipLaunchKernelGGL(k_reduce2<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, G, work, acc, init,
                       (const double *)nullptr, N, (int64_t)0);
    return check_launch("gf_reduce_tile");
}

int gf_reduce_tile_steady(int B, int64_t N, int64_t n_first, const double *d, const double *z,
                          const double *steady, double *work, double *acc, int init, void *stream) {
    if (B < 1 || N < 1 || n_first < 0)
        return gf_internal_error(-1, "gf_reduce_tile_steady: empty problem or negative n_first (N=%lld, n_first=%lld)", (long long)N, (long long)n_first);
    if (!d || !steady || !work || !acc) return gf_internal_error(-1, "gf_reduce_tile_steady: null pointer");
    const int G = red_groups(N);
    hipLaunchKernelGGL(k_reduce1<true>, dim3(G, B), dim3(RED_BLOCK), 0, (hipStream_t)stream, N, d, z, work, steady, n_first);
    hipLaunchKernelGGL(k_reduce2<true>, dim3(B), dim3(64), 0, (hipStream_t)stream, G, work, acc, init, steady, N, n_first);
    return check_launch("gf_reduce_tile_steady");
}

int gf_loglike_finish(int B, int64_t N, const double *acc, const int32_t *info,
                      double *out, double *logdet, void *stream) {
    if (B < 1 || N < 1) return gf_internal_error(-1, "gf_loglike_finish: empty problem (B=%d, N=%lld)", B, (long long)N);
    if (!acc || (!out && !logdet)) return gf_internal_error(-1, "gf_loglike_finish: null pointer");
    hipLaunchKernelGGL(k_finish, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, N, acc, info, out, logdet);
    return check_launch("gf_loglike_finish");
}

}  // extern "C"
