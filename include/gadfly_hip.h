/*
 * gadfly_hip.h -- C-ABI of libgadfly_hip.so, the MI355X (gfx950) replacement for the
 * celerite2 C++ driver calls that gadfly's GP hot path makes.
 *
 * The reference (/root/reference/gadfly/gp.py) reaches native code only through
 * celerite2.GaussianProcess -> pybind11 module `celerite2.driver` (third-party, NOT in
 * /root/reference).  Each entry point below names the driver function
 * it replaces and the gadfly call site that reaches it:
 *
 *   gf_build_matrices   driver.get_celerite_matrices   <- gp.py:202 (compute)
 *   gf_factor           driver.factor                  <- gp.py:202 (compute)
 *   gf_reduce_tile /
 *   gf_loglike_finish   numpy glue in celerite2.core   <- gp.py:350 (_norm - 0.5 sum z^2/d)
 *   gf_solve            driver.solve_lower / solve_upper / matmul_lower
 *                                                      <- gp.py:350, :370, :232, :327, :391
 *   gf_general_matmul   driver.general_matmul_lower + general_matmul_upper
 *                                                      <- gp.py:232 (predict at new times)
 *   gf_loglike_grad     driver.factor_rev + solve_lower_rev + the norm's adjoint
 *                                                      (no gadfly call site: gradients for samplers)
 *   gf_loglike_grad_wide   the same for wide kernels, one workgroup per problem (W up to 192: the 86-term default
 *                                                      kernel of gadfly/core.py, W = 172)
 *   gf_solve_batch      driver.factor + solve_lower + solve_upper + general_matmul_lower / _upper at t* = t
 *                                                      <- gp.py:370, :232 for B kernels at once
 *   gf_solve_batch_wide    the same without a component for wide kernels, one workgroup per problem (W up to 192;
 *                                                      DESIGN.md 3.9.1)
 *   gf_var_batch        the same plus the diagonal of K* - K*^T (K + diag)^-1 K* (celerite2's
 *                       ConditionalDistribution.variance)   <- gp.py:241-306 (predict(..., return_var=True)) for B
 *                                                      kernels at once
 *   gf_solve_batch_rhs / gf_predict_batch_at_rhs
 *                       gf_solve_batch / gf_predict_batch_at for R right-hand sides per problem through one pass over
 *                       the rows: celerite2's apply_inverse of a matrix, the log-likelihoods of R data vectors and the
 *                       operator of exact conditional draws (no celerite2 counterpart beyond the dense
 *                       ConditionalDistribution.sample) for B kernels at once
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP) unless marked "host"; float64 throughout;
 *   - row-major; the N x W generator matrices U, V, W and the propagator P use a leading
 *     dimension `ld` >= W (ld is a multiple of 16, pad columns hold 0 for U/V/W and 1 for P)
 *     so rows start 128-byte aligned; batch stride is N*ld;
 *   - B independent problems per call (light curves or MCMC walkers); per-array
 *     batch strides are in elements, 0 = shared by all problems;
 *   - the caller owns every buffer (torch tensors on the Python side); the library allocates
 *     nothing and keeps no mutable global state: every option is a call argument (the only statics
 *     are the thread-local last-error string and a per-device "large-LDS attribute applied" flag);
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work;
 *   - return value: 0 ok, < 0 bad arguments / launch error (see gf_last_error()).
 *     Numerical failure (non-positive pivot, celerite2's LinAlgError) is reported per problem
 *     in the device array `info` (0 or the 1-based failing row), never by the return value.
 */
#ifndef GADFLY_HIP_H
#define GADFLY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_MAX_WIDTH 256        /* largest supported celerite width W (= 2 J for gadfly) */

/* gf_solve modes */
#define GF_SOLVE_LOWER   0      /* Z = L^-1 Y          driver.solve_lower  */
#define GF_SOLVE_UPPER   1      /* Z = L^-T Y          driver.solve_upper  */
#define GF_MATMUL_LOWER  2      /* Z = L Y             driver.matmul_lower (with V := W) */

/* `variant` of gf_loglike_fused / gf_chunk_sweep / gf_chunk_transition: which fused sweep runs.
 * Both agree to rounding and are parity-tested; callers pass GF_SWEEP_AUTO. */
#define GF_SWEEP_AUTO    0      /* lane-tiled sweep where the term structure allows it, else by column */
#define GF_SWEEP_COLUMN  1      /* k_factor3 / k_phi: one state column per lane, any mix of terms */
#define GF_SWEEP_TILED   2      /* k_factor7 / k_phi7: 2 x 32 lane tiling; needs Jr = 0, Jc <= 31 */
/* OR-ed into gf_chunk_sweep's `variant`: every chunk of the call starts from a ZERO state (a nominal pass);
 * the S_state / F_state slots are then outputs only and need not be initialised. */
#define GF_SWEEP_ZERO_START 0x100
/* OR-ed into gf_loglike_fused's `variant` (W <= 63 only): the block-scaled coordinates may span
 * gf_scaled_span(1) instead of gf_scaled_span(0) in c_max * (t - t_reset) -- fewer reset rows at the same `block`
 * rule, or a longer `block`.  Safe for amplitudes and pivots within 1e+-100. */
#define GF_SWEEP_LONG_SPAN 0x200
/* OR-ed into the `variant` of gf_steady_finish, gf_steady_finish_window and gf_steady_finish_chunked (no other entry
 * point takes it): the CALLER has proved that every spacing t[r] - t[r - 1] of every tail row r (switch row <= r < N)
 * of every problem of the call passes both of the tail's tests -- not a gap (<= gap / cmax[b], gap = gf_scaled_span /
 * (block - 1)) and on the frozen cadence (|spacing - steady[b][6]| < 2e-6 / max(c, |d|)).  The launch then reads no
 * time stamp, tests nothing and never writes steady[b][2]; every other word it writes takes the bits it takes without
 * the flag.  A caller that promises more than its axis keeps gets finite numbers that mean nothing. */
#define GF_SWEEP_AXIS_PROVEN 0x400

int gf_version(void);
const char *gf_last_error(void);

/* leading dimension the library wants for width W (multiple of 16); <0 if W unsupported */
int gf_leading_dim(int W);

/*
 * Matrix build + propagator rows, for the N rows n_first .. n_first+N-1 of a
 * longer series (tile streaming; n_first = 0 and N = series length for a whole series).
 *   coefficients: ar, cr [B][Jr]; ac, bc, cc, dc [B][Jc]   (W = Jr + 2 Jc)
 *   diag_add [B]  : sum(ar) + sum(ac) + TermConvolution diagonal shift, added to diag
 *   t    [B|1][*] : times of the WHOLE series (indexed with the global row), batch stride t_bs
 *   diag [B|1][*] : user diagonal (yerr^2) of the whole series, batch stride diag_bs; NULL = 0
 * outputs (tile-local row index)
 *   a [B][N] (NULL ok);  U, V, P [B][N][ld];  P[n][j] = exp(c_j (t[g-1] - t[g])), g = n_first+n,
 *   P row of global row 0 = 1  (P may be NULL when only U, V are wanted, e.g. at prediction times)
 */
int gf_build_matrices(int B, int64_t N, int64_t n_first, int Jr, int Jc, int ld,
                      const double *ar, const double *cr, const double *ac,
                      const double *bc, const double *cc, const double *dc,
                      const double *diag_add,
                      const double *t, int64_t t_bs,
                      const double *diag, int64_t diag_bs,
                      double *a, double *U, double *V, double *P, void *stream);

/*
 * Semiseparable LDL^T factor of N consecutive rows, optionally fused with the
 * forward solve of one right-hand side (the log-likelihood path).
 *   inputs : a [B][N]; U, V, P [B][N][ld]; y [B|1][N] (pointer to the tile's first row,
 *            batch stride y_bs) or NULL
 *   outputs: d [B][N]; Wm [B][N][ld] or NULL (not stored); z [B][N] (= L^-1 y) or NULL
 *   state  : S_state [B][gf_state_size(W)], F_state [B][gf_state_cols(W)] or NULL.
 *            When given, the recurrence state (S + d w w^T and F + w z of the last row, before
 *            the next propagator is applied) is READ at entry and WRITTEN at exit, so a series
 *            can be streamed tile by tile through fixed-size U/V/P buffers; zero both before
 *            the first tile.  NULL = start from zero, final state not stored.
 *   info [B]: must be zeroed by the caller before the first tile; the kernel only ever writes
 *            a non-zero value (1-based GLOBAL row n_first+n+1 of the first non-positive pivot),
 *            and a problem whose info is already non-zero is skipped.
 */
int64_t gf_state_size(int W);
int gf_state_cols(int W);
int gf_factor(int B, int64_t N, int64_t n_first, int W, int ld,
              const double *a, const double *U, const double *V, const double *P,
              const double *y, int64_t y_bs,
              double *d, double *Wm, double *z,
              double *S_state, double *F_state, int32_t *info, void *stream);

/*
 * Log-likelihood fast path for W <= 64 in block-scaled coordinates (see the derivation above
 * k_build2 in gadfly_stored.hip).  Same role as gf_build_matrices + gf_factor on the
 * log-likelihood path (gp.py:202 + gp.py:350); U~, V~ are u o rho and v / rho with
 * rho = exp(-c (t_n - t_ref)); de[n] = t_ref(n) - t_ref(n-1) >= 0 at reset rows (where the
 * accumulated decay exp(-c de) is applied once) and -1 elsewhere.
 *   cmax [B] : max_j c_j of each problem; block: rows between forced resets, a power of two in
 *   1..64 chosen by the caller so that (block - 1) * cmax * cadence stays well below 28 (a row
 *   whose cmax * dt exceeds 28/(block-1) resets on its own); c [B][W] decay rate per column;
 *   n_first must be a multiple of block.
 *   outputs of gf_build_scaled: a, de [B][N]; Ut, Vt [B][N][ld]
 *   gf_factor_scaled: y (tile pointer), d, z, S_state [B][64*64], F_state [B][64], info as in
 *   gf_factor (state mandatory; zero it and info before the first tile).  Wm is not produced.
 *   Widths 64 < W <= 256 (gf_scaled_wide_supported): the same recurrence on several waves per
 *   problem (k_factor2w: two FMAs per state element and row instead of gf_factor's four operations);
 *   S_state [B][gf_state_size(W)], F_state [B][gf_state_cols(W)] as for gf_factor.
 *   The sweep prefetches rows n+1, n+2 unconditionally: a, de, y, Ut, Vt must each be readable
 *   two rows (elements) past the last row of the last problem.
 */
int gf_scaled_supported(int W);
/* Largest c_max * (t_n - t_reset) inside a scaling block: the block rule of every route is
 * 1.5 * (block - 1) * c_max * cadence <= gf_scaled_span(0); with GF_SWEEP_LONG_SPAN, gf_scaled_span(1). */
double gf_scaled_span(int long_span);
int gf_scaled_wide_supported(int W);
int gf_build_scaled(int B, int64_t N, int64_t n_first, int Jr, int Jc, int ld,
                    const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc,
                    const double *diag_add, const double *cmax, int block,
                    const double *t, int64_t t_bs,
                    const double *diag, int64_t diag_bs,
                    double *a, double *Ut, double *Vt, double *de, void *stream);
int gf_factor_scaled(int B, int64_t N, int64_t n_first, int W, int ld, const double *c,
                     const double *a, const double *Ut, const double *Vt, const double *de,
                     const double *y, int64_t y_bs,
                     double *d, double *z, double *S_state, double *F_state,
                     int32_t *info, void *stream);

/*
 * Fully fused log-likelihood sweep (W <= 63): matrix build + factor + forward solve of N
 * consecutive rows in one kernel, generator rows produced in registers (nothing but t, y, diag
 * is read: 24 B/row).  Replaces gf_build_scaled + gf_factor_scaled on the log-likelihood path
 * (gp.py:202 + gp.py:350) whenever max|d_c| * max|t| < 1e12 (the range of the kernel's
 * FMA-reduced sincos; the caller checks).  Arguments as in gf_build_scaled / gf_factor_scaled;
 * t, diag (NULL = 0), y are the WHOLE series (global row index, batch strides t_bs, diag_bs,
 * y_bs) and must be readable three elements past row n_first + N - 1.
 *
 * gen_period: accuracy / speed of the in-register generator rows (also of gf_chunk_sweep and
 * gf_chunk_transition).  Between exact anchors the rows advance by a cached complex rotation; every
 * `gen_period` rows (a power of two, 1..64) the phasor is recomputed exactly.  Measured at a
 * condition (diagonal / pivot) of 4e5 against an 80-bit recurrence, per 8192-row tile of 2048
 * evaluations: 1 (exact rows) 2e-10 / 12.2 ms, 4: 2e-9 / 10.4 ms, 16: 1e-8 / 10.0 ms, 64: several
 * 1e-8 / 10.0 ms, i.e. error ~ 1.6e-15 * gen_period * condition.  Callers pick it from the condition
 * estimate max(a) / min(d) that gf_reduce_tile returns (1 when in doubt).  Irregular spacings are
 * always generated exactly.  variant: GF_SWEEP_AUTO (see the GF_SWEEP_* constants).
 *
 * Wide kernels: for kernels made of complex terms only (Jr = 0: every SHO term with Q >= 1/2) the
 * same entry points take 64 <= W <= 176 (k_factorw: one workgroup of ceil((W + 1) / 32) + 1 waves per
 * problem; `variant` is ignored).  gf_fused_supported tells; S_state then holds
 * gf_fused_state_size(Jr, Jc) doubles per (problem, chunk) slot instead of 64 * 64 (zeroed by the
 * caller before the first tile; opaque layout) and F_state is not used (may be NULL).
 */
int gf_fused_supported(int Jr, int Jc);
int64_t gf_fused_state_size(int Jr, int Jc);
int gf_loglike_fused(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                     int gen_period, int variant,
                     const double *ar, const double *cr, const double *ac,
                     const double *bc, const double *cc, const double *dc,
                     const double *diag_add, const double *cmax,
                     const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                     const double *y, int64_t y_bs,
                     double *d, double *z, double *S_state, double *F_state,
                     int32_t *info, void *stream);

/*
 * gf_loglike_fused with the STEADY MODE of the lane-tiled sweep (Jr = 0, Jc <= 31; an error otherwise).  On a
 * regular cadence with a constant diagonal the pivot d and the gains w = r / d -- in the frame that rotates with
 * the terms' phasors -- converge geometrically to constants.  From global row arm_from on (the caller's
 * promise: regular cadence, constant diagonal, from there to the end of the series; arm_from >= N: never) the
 * sweep compares both, at the rows = 0 mod 64 (block resets at every block), with their values 16 such rows --
 * 1024 rows -- before; once they have moved by less than 1e-10 (gains: relative to the largest) at 4 consecutive
 * ones it freezes them and ends.  All later rows and tiles of that problem belong to a second kernel, launched
 * on the same stream behind the sweep on every call: with pivot, gains and cadence (taken over the last 1024 rows)
 * frozen, the forward solve is a linear time-invariant filter with Jc complex poles, run in blocks of 64 rows
 * (k_steady_tail in gadfly_hip.hip).  d, z, info, S_state, F_state as for gf_loglike_fused (S_state and F_state
 * are no longer maintained after the switch: the filter's state lives in `steady`).  t must be readable from
 * global row 0 on whatever n_first (the cadence looks 1024 rows behind the switch row).
 *   steady [B][gf_steady_size()] doubles, zeroed by the caller before the FIRST tile of an evaluation and
 *          handed unchanged to the following tiles.  Per problem: [0] first frozen row (global index; 0 = the
 *          mode has not been entered), [1] the frozen pivot, [2] != 0: VIOLATION -- a frozen row met a gap or a
 *          spacing off the frozen cadence, the result is invalid and the evaluation must be repeated with
 *          gf_loglike_fused; the rest is the sweep's own.
 */
int64_t gf_steady_size(void);
int gf_loglike_steady(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                      int gen_period, int variant,
                      const double *ar, const double *cr, const double *ac,
                      const double *bc, const double *cc, const double *dc,
                      const double *diag_add, const double *cmax,
                      const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                      const double *y, int64_t y_bs,
                      double *d, double *z, double *S_state, double *F_state,
                      int32_t *info, double *steady, int64_t arm_from, void *stream);

/*
 * The steady mode without stored tail rows: the route of a streamed log-likelihood.  Per tile
 *   gf_steady_sweep       : gf_loglike_steady's sweep instance alone -- arguments, `steady` and its slots [0], [1],
 *                           [2] as there.  A problem's rows of the tile in front of its switch row are stored in d
 *                           and z; the rows behind it are NOT computed (d, z keep whatever they held);
 *   gf_reduce_tile_steady : gf_reduce_tile over the rows that gf_steady_sweep stored -- per problem the rows of the
 *                           tile (N rows from global row n_first) in front of its switch row, all of them for a
 *                           problem that has not switched (then the same tree in the same order: the same bits as
 *                           gf_reduce_tile).  No other row of d, z is read.  work, acc, init as for gf_reduce_tile;
 *   gf_steady_sweep_reduced : the two in one launch -- gf_steady_sweep, whose wave then adds the rows it stored to
 *                           acc[b] itself: the additions of gf_reduce_tile_steady in its order, so acc, d, z, the state
 *                           and `steady` hold the bits of the two calls (a problem that fails, or had failed, takes
 *                           that reduction's stale rows too; its value is -inf either way).  No work buffer, and no
 *                           workgroup beyond the sweep's own: for tiles in which most problems have no rows left.  A
 *                           problem that had switched before the tile is left alone (init != 0: acc[b] = 0, 0, +inf);
 * and once per evaluation, behind the last tile's reduction on the same stream,
 *   gf_steady_finish      : the rows [switch row, N) of the WHOLE series (N rows; t, y from global row 0) of every
 *                           problem that has switched, in one launch of one wave per problem: the block filter of
 *                           gf_loglike_steady's second kernel with one set-up, blocks of 64 rows from the switch
 *                           row on, no row stored.  With d = steady[b][1] on all of them,
 *                               acc[b][0] += (N - switch row) log d,  acc[b][1] += (sum z^2) / d,
 *                               acc[b][2]  = min(acc[b][2], d)
 *                           (sums in a fixed order: deterministic for given B, N and switch rows).  Every spacing is
 *                           tested as gf_loglike_steady tests it (steady[b][2]), unless `variant` carries
                           GF_SWEEP_AXIS_PROVEN (above: then t is not read).  Problems with info != 0 or
 *                           without a switch are left alone.  block, variant: the sweep's (they set its gap test);
 *                           ac .. dc, cmax, t, y and their batch strides: the sweep's.
 *   gf_steady_finish_window : gf_steady_finish for the problems whose switch row steady[b][0] lies in [sw_lo, sw_hi)
 *                           (0 <= sw_lo <= sw_hi; switch rows are 1 .. N); every other problem is left alone, nothing
 *                           of it read or written beyond info[b] and steady[b][0].  A problem runs the code and takes
 *                           the additions it takes in gf_steady_finish: launches over disjoint windows that cover
 *                           [1, N + 1) give gf_steady_finish's bits, in any order.  An empty window launches nothing.
 *                           A window may run on ANOTHER stream beside later tiles of the same evaluation, once the
 *                           gf_reduce_tile_steady of the tile that holds row sw_hi - 2 has ended (an event): a
 *                           switched problem's header and acc[b] are touched by nothing else after that reduction.
 *                           The caller joins the streams before it reads acc or steady.
 * Then gf_loglike_finish.  The values agree with gf_loglike_steady + gf_reduce_tile to the rounding of the sums.
 */
int gf_steady_sweep(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                    int gen_period, int variant,
                    const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc,
                    const double *diag_add, const double *cmax,
                    const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                    const double *y, int64_t y_bs,
                    double *d, double *z, double *S_state, double *F_state,
                    int32_t *info, double *steady, int64_t arm_from, void *stream);
int gf_reduce_tile_steady(int B, int64_t N, int64_t n_first, const double *d, const double *z,
                          const double *steady, double *work, double *acc, int init, void *stream);
int gf_steady_sweep_reduced(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                            int gen_period, int variant,
                            const double *ar, const double *cr, const double *ac,
                            const double *bc, const double *cc, const double *dc,
                            const double *diag_add, const double *cmax,
                            const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                            const double *y, int64_t y_bs,
                            double *d, double *z, double *S_state, double *F_state,
                            int32_t *info, double *steady, int64_t arm_from, double *acc, int init, void *stream);
/*
 * gf_steady_sweep_rank1 : the rows in front of the switch row in O(W) per row, for an axis that is regular and a
 *     diagonal that is constant FROM ROW 0 of the series (arm_from = 0 promised for every tile; Jr = 0, Jc <= 31).  In
 *     the frame that rotates with the phasors the recurrence is then a time-invariant Riccati iteration from a zero
 *     state whose increments keep rank one: pivot, gain and forward solve from three complex vectors of one entry per
 *     term (r, Y, f) and two scalars, no W x W state.  The arguments of gf_steady_sweep_reduced and
 *         dt[B] : the cadence of each problem's axis over the WHOLE series, (t_last - t_first) / (rows - 1) (a local
 *                 cadence will not do: its error is a phase error that grows with the row).
 *     The contract is gf_steady_sweep's with acc = NULL and gf_steady_sweep_reduced's with acc: one wave per problem,
 *     the rows in front of the switch row stored in d and z, the same switch rule on the same anchors with the same
 *     ring in `steady`, the same slots at the switch (the gf_steady_finish family and gf_loglike_steady's tail read
 *     them), info[b] = first failing row + 1, problems that failed or had switched left alone.  EVERY tile of the
 *     evaluation from global row 0 on goes through this entry point: between tiles the state lies in the problem's
 *     S_state slot (F_state, ar, cr are not read).  Every spacing of a tile's rows is tested as the tail tests it
 *     (steady[b][2]).  The rows agree with gf_steady_sweep's to rounding, not bit for bit.
 */
int gf_steady_sweep_rank1(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                          int gen_period, int variant,
                          const double *ar, const double *cr, const double *ac,
                          const double *bc, const double *cc, const double *dc,
                          const double *diag_add, const double *cmax,
                          const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                          const double *y, int64_t y_bs,
                          double *d, double *z, double *S_state, double *F_state,
                          int32_t *info, double *steady, int64_t arm_from, double *acc, int init,
                          const double *dt, void *stream);
int gf_steady_finish(int B, int64_t N, int Jr, int Jc, int block, int variant,
                     const double *ac, const double *bc, const double *cc, const double *dc, const double *cmax,
                     const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                     const int32_t *info, double *steady, double *acc, void *stream);
int gf_steady_finish_window(int B, int64_t N, int Jr, int Jc, int block, int variant,
                            const double *ac, const double *bc, const double *cc, const double *dc, const double *cmax,
                            const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                            const int32_t *info, double *steady, double *acc,
                            int64_t sw_lo, int64_t sw_hi, void *stream);
/*
 * gf_steady_finish_chunked : gf_steady_finish_window with more than one wave per problem -- for a window that holds
 *     few problems with long tails.  Behind the switch a 64-row block is linear and time-invariant in the state
 *     (z = u + Q s, s' = M s + K u), so the tail runs in chunks of chunk_blocks blocks side by side: pass A (chunk 0
 *     from the true state, the others from zero, and M from the block's own code on unit states), P = M^chunk_blocks
 *     by squarings, pass B (every later chunk again from its true state s_in[c + 1] = s_out0[c] + P s_in[c], summing
 *     z^2), and the chunks' sums added in chunk order: five launches on `stream`, about two chunk lengths instead of
 *     the whole tail.  The window, the problems left alone, what acc and steady take and the spacing tests are
 *     gf_steady_finish_window's; acc[b][0] and acc[b][2] take its bits, acc[b][1] and the state agree with it to
 *     rounding (the same bits for the same N, switch row and chunk_blocks, in whatever order the waves run).
 *     chunk_blocks: a power of two >= 16 (every chunk starts on the problem's grid of 16-block groups).
 *     chunk_ws: B x gf_steady_chunk_size(N, chunk_blocks) doubles, the launch's alone until it has ended.
 */
int64_t gf_steady_chunk_size(int64_t N, int chunk_blocks);
int gf_steady_finish_chunked(int B, int64_t N, int Jr, int Jc, int block, int variant,
                             const double *ac, const double *bc, const double *cc, const double *dc, const double *cmax,
                             const double *t, int64_t t_bs, const double *y, int64_t y_bs,
                             const int32_t *info, double *steady, double *acc,
                             int64_t sw_lo, int64_t sw_hi, int chunk_blocks, double *chunk_ws, void *stream);

/*
 * Fused sampling sweep: B draws y = L D^1/2 eps of B different kernels, K = L D L^T, in the sweep that factors
 * -- no factor is stored (24 B read, 16 B written per row: t, diag, eps; d, out).  Replaces celerite2's
 * driver.matmul_lower with V := W after driver.factor (the reference's GaussianProcess.sample, gp.py:391) for
 * one realisation per kernel.  The pad column that carries gf_loglike_fused's forward solve carries the draw:
 *     x_n = sqrt(d_n) eps_n (correctly rounded sqrt),  F_n = P_n (F_{n-1} + W_{n-1} x_{n-1}),  out_n = x_n + U_n^T F_n.
 * Arguments and conventions are gf_loglike_fused's -- tiles through n_first with S_state / F_state carried
 * between the calls (zeroed by the caller before the first), block, gen_period, variant (GF_SWEEP_LONG_SPAN
 * included), t / diag / eps readable three elements past row n_first + N - 1, info -- with two differences:
 *   eps  (in)  the standard normals, WHOLE series (global row index, batch stride eps_bs), where y stands;
 *   out  (out) the draw, WHOLE series too: row n_first + n of problem b goes to out[b * eps_bs + n_first + n]
 *              (eps's batch stride, which must be >= 1 when B > 1) -- unlike z, which gf_loglike_fused writes
 *              tile-local: the draw is the product, not an intermediate.
 * d (out) is tile-local, (B, N), as in gf_loglike_fused: the caller takes min d from it for the generator-period
 * rule.  A problem whose pivot fails leaves its 1-based global row in info and stops; what its out rows hold
 * from there on is undefined (the caller blanks them).  Takes every term structure gf_fused_supported accepts:
 * W <= 63 with any mix of terms, 64 <= W <= 176 with complex terms only.
 */
int gf_sample_fused(int B, int64_t N, int64_t n_first, int Jr, int Jc, int block,
                    int gen_period, int variant,
                    const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc,
                    const double *diag_add, const double *cmax,
                    const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                    const double *eps, int64_t eps_bs,
                    double *d, double *out, double *S_state, double *F_state,
                    int32_t *info, void *stream);

/*
 * Exact time-parallel evaluation of ONE long series (or a few): the N rows are cut into nch
 * chunks of chunk_len rows (a multiple of `block`; the last chunk may be shorter) that are swept
 * concurrently, then stitched with an exact linear-fractional combine:
 *   1. gf_chunk_sweep      nominal pass: every chunk starts from the zero state -- S_state/F_state
 *                          [B*nch] zeroed by the caller, or variant | GF_SWEEP_ZERO_START (the slots
 *                          are then outputs only); outputs dbar, zbar [B][N], rbar [B][N][64]
 *                          (pass r_out), the rows u~ [B][N][64] and reset spans de [B][N] (pass Ut_out,
 *                          de_out; Wt_out may stay NULL) and the nominal end states in S_state/F_state.
 *   2. gf_chunk_transition closed-loop transition Phi [B*nch][64*64] and the Gram sums G [B*nch][64*64],
 *                          m [B*nch][64] of the chunks chunk_first .. chunk_first + chunk_count - 1 of
 *                          every problem, from those rows (c [B][W]: the columns' decay rates).  The
 *                          start states never depend on the last chunk's map, and on the first chunk's
 *                          only through its end state: callers sweep the chunks 1 .. nch - 2 and hand
 *                          the combine zeros for the first chunk's Phi, G, m.
 *   3. gf_chunk_combine    sequential LFT combine over the chunks (64x64 pivoted solves in LDS):
 *                          S_state/F_state slot c <- TRUE start state of chunk c.
 *      gf_chunk_combine_tree  the same result in 2 (log2(P) - 1) levels (Blelloch scan over the chunk
 *                          maps) on the same arrays [B*nch] (Phi, G, m, S = nominal end X,
 *                          F = nominal end Y); P = the power of two with P / 2 < nch <= P.  The map
 *                          arrays are overwritten; Xst [B*nch][64*64] / Yst [B*nch][64] slot c <- TRUE
 *                          start state of chunk c; work: gf_chunk_combine_tree_work(B, P, nch) doubles
 *                          (the scan's slots beyond nch).
 *   4. gf_chunk_sweep      final pass from those states (r_out = NULL): d, z equal the
 *                          sequential result to rounding; reduce with gf_reduce_tile.  With
 *                          Ut_out, Wt_out [B][N][64] and de_out [B][N] the pass also stores the
 *                          factor in scaled form (rows u~, w~ = r/d and the reset spans) for
 *                          gf_chunk_linear.
 * Same argument conventions (gen_period and variant included: pass the SAME values to all
 * calls of one evaluation) and padding rules as gf_loglike_fused; the row arrays gf_chunk_transition
 * reads (Ut, rbar, dbar, zbar, de) must be readable EIGHT rows past the end (they are fetched ahead by
 * LDS-DMA; what those rows hold never reaches a result, NaN included).  Beyond the width gf_chunk_transition
 * writes: Phi ones on the diagonal W <= j < ROWS = 4 ceil(W / 4) (the sweep carries ROWS state rows from
 * Phi = I and nothing touches the padding ones) and zeros everywhere else; G and m zeros.  The ones are harmless
 * to every consumer: the LFT combines work on the leading W x W only, and in the linear combines they multiply
 * state rows that are zero (tests/test_gpu_chunk_transition.py pins the layout, tests/
 * test_gpu_chunk_linear_combine.py feeds its maps in it).  A row with dbar <= 0 adds nothing to G, m and
 * the pending update.  Width 1..63, phases |d t| < 1e12.  gf_chunk_sweep works on the chunks chunk_first ..
 * chunk_first + chunk_count - 1 of every problem (state slots and rows of the others are left alone): the
 * nominal pass leaves out the last chunk, a final pass that stores no factor the first one (whose nominal
 * pass was exact).  A slot whose info entry is non-zero on entry is skipped as well.
 */
int gf_chunk_sweep(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count,
                   int Jr, int Jc, int block, int gen_period, int variant,
                   const double *ar, const double *cr, const double *ac,
                   const double *bc, const double *cc, const double *dc,
                   const double *diag_add, const double *cmax,
                   const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                   const double *y, int64_t y_bs,
                   double *d, double *z, double *r_out, double *Ut_out, double *Wt_out,
                   double *de_out, double *S_state, double *F_state,
                   int32_t *info, void *stream);
int gf_chunk_transition(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count,
                        int Jr, int Jc, int variant, const double *c, const double *de, const double *dbar,
                        const double *zbar, const double *rbar, const double *Ut,
                        double *Phi_out, double *G_out, double *m_out, void *stream);
/*
 * The stored rows as a factor for gf_solve (any width the fused sweeps take, in particular the wide
 * kernels, which have no chunk-parallel sweeps): gf_fused_row_stride is the leading dimension of
 * Ut_out / Wt_out / r_out (64, or the padded column count of the wide sweep), and
 * gf_scaled_propagator expands the reset spans de [B][N] into the propagator rows P [B][N][ld] of
 * the scaled coordinates (1, or exp(-c de) at a reset row; c [B][W]).  gf_solve(U = Ut, Wm = Wt,
 * P, scale = d) then performs solve_lower / solve_upper / matmul_lower of the TRUE factor
 * (driver.solve_lower etc. <- gp.py:350, :370, :327).
 */
int gf_fused_row_stride(int Jr, int Jc);
int gf_scaled_propagator(int B, int64_t N, int W, int ld, const double *c, const double *de,
                         double *P_out, void *stream);
/*
 * Wide kernels (64 <= W <= 176, complex terms): the closed-loop transition sweep of step 2 on the rows
 * the nominal pass stored -- Ut [B][N][ld] (u~ rows), rbar [B][N][ld], dbar [B][N], de [B][N] (reset
 * spans), ld = gf_fused_row_stride; c [B][W] decay rates; Ut, rbar, dbar and de readable EIGHT rows
 * past the end (the rows are fetched ahead by LDS-DMA, unconditionally).  Outputs the rows h [B][N][ld]
 * and Phi [B*nch][gf_fused_state_size] in the layout of S_state ([column][row], padded; columns from
 * 16 ceil(W / 16) on are left unwritten in both).  The Gram sums
 * G = sum h h^T / dbar, m = sum h zbar / dbar and the combine of the W x W chunk maps follow in
 * gf_wide_combine.  Only the chunks chunk_first .. chunk_first + chunk_count - 1 of every problem are swept.
 */
int gf_chunk_transition_wide(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count, int Jc,
                             const double *c, const double *de, const double *dbar, const double *rbar,
                             const double *Ut, double *h_out, double *Phi_out, void *stream);
/* (W = Jr + 2 Jc, the width of the states, 1 .. 64: the 64 x 64 slots are zero beyond it -- but for the padding
 * ones on Phi's diagonal that gf_chunk_transition leaves, above, which nothing here reads --, and the combines'
 * pivoted solves and matrix products are carried out on the leading W rows and columns only.  The sweeps and
 * gf_chunk_corrections stop at W = 63; the combines themselves take the full slot, W = 64, and are tested there
 * (tests/test_gpu_chunk_combine.py).  Slot 0 of the outputs is zero; the last chunk's Phi, G, m and nominal end
 * state are never read into a result.) */
int gf_chunk_combine(int B, int nch, int W, const double *Phi, const double *G, const double *m,
                     double *S_state, double *F_state, void *stream);
int64_t gf_chunk_combine_tree_work(int B, int P, int nch);
int gf_chunk_combine_tree(int B, int P, int nch, int W, double *Phi, double *G, double *m, double *S, double *F,
                          double *Xst, double *Yst, double *work, void *stream);

/*
 * Triangular sweeps on the stored scaled factor, time-parallel (same modes as gf_solve):
 *   gf_chunk_linear(store=0)   local pass: every chunk from a ZERO state, leaves its end state in its
 *                              F_state slot; nothing else is written (Z is not touched).  The pass
 *                              reads nothing of F_state, but it WRITES only the state rows
 *                              i < ROWS = 4 ceil(W / 4) of every slot (R = 1: all 64 rows;
 *                              GF_MATMUL_LOWER with R >= 16: the rows below 16 ceil(W / 16)), and the
 *                              solves' combines multiply ALL 64 rows of every slot by the rows of Phi
 *                              (zeros there, but 0 x NaN = NaN).  So for GF_SOLVE_LOWER / GF_SOLVE_UPPER
 *                              with R > 1 and W <= 60 the caller ZEROES the rows ROWS .. 63 of every
 *                              slot (elements [i * R + r], i >= ROWS) before the local pass; everything
 *                              else of F_state -- and all of it for R = 1, for W > 60 and for
 *                              GF_MATMUL_LOWER, whose diagonal combine keeps the rows apart -- may hold
 *                              anything, NaN included (tests/test_gpu_chunk_linear_combine.py,
 *                              test_f_state_contract).
 *   gf_chunk_linear_combine    F_state slot c <- true start state of chunk c.  GF_SOLVE_LOWER /
 *                              GF_SOLVE_UPPER need Phi [B*nch][64*64], the chunk transitions of the
 *                              TRUE factor (gf_chunk_transition run on the final pass' d, z, r
 *                              rows; the backward sweep uses its transpose); GF_MATMUL_LOWER
 *                              needs c, de and D_work [B*nch][64] instead.
 *   gf_chunk_linear(store=1)   final pass: Z rows (every chunk's END state replaces its start state in
 *                              F_state).
 * Y, Z are [B][N][R] (Z may alias Y); F_state is [B*nch][64*R]; scale != 0 divides the input
 * rows by d (solves) or multiplies them by sqrt(d) (GF_MATMUL_LOWER), as in gf_solve.  chunk_len is any
 * length >= 1 with (nch - 1) chunk_len < N <= nch chunk_len; W = 1 .. 63; R >= 1 with no upper limit (the
 * right-hand sides are swept in tiles of 64, or of 32 / 64 on the matrix pipe: GF_MATMUL_LOWER with R >= 16;
 * engine.ScaledFactor sends at most 64 at a time, tests/test_gpu_chunk_linear.py runs 65).  The combines take
 * any R as well; gf_chunk_diag_scan stops at 64.
 */
int gf_chunk_linear(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int R,
                    int scale, int store, const double *c,
                    const double *Ut, const double *Wt, const double *d, const double *de,
                    const double *Y, double *Z, double *F_state, void *stream);
int gf_chunk_linear_combine(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int R,
                            const double *c, const double *de, const double *Phi,
                            double *D_work, double *F_state, void *stream);
/*
 * Two-level form of the solves' combine (long single series: the plain combine is one 64 x 64
 * mat-vec per chunk in sequence).  gf_chunk_segment_transitions composes, once per factor, the
 * transitions of every segment of seg_len chunks: Psi_out [B*nseg][64*64], nseg = ceil(nch / seg_len).
 * gf_chunk_linear_combine_seg then does what gf_chunk_linear_combine does with a sequential depth of
 * 2 seg_len + nseg chunks; V_work is [B*nseg][64*R] scratch.  PhiT_out / PsiT_out (both or neither; may be
 * NULL): the transposes of every Phi and Psi, for the backward solve -- handed to gf_chunk_linear_combine_seg as
 * PhiT / PsiT its loads run along the lanes as the forward solve's do (NULL there: the transposes are read out of
 * Phi / Psi, one 128-byte run per lane).
 */
int gf_chunk_segment_transitions(int B, int nch, int seg_len, const double *Phi, double *Psi_out,
                                 double *PhiT_out, double *PsiT_out, void *stream);
int gf_chunk_linear_combine_seg(int mode, int B, int nch, int seg_len, int R, const double *Phi,
                                const double *Psi, const double *PhiT, const double *PsiT,
                                double *F_state, double *V_work, void *stream);

/*
 * Batched dense solve A X = B (Gauss-Jordan with partial pivoting, one launch): A [batch][n][n] row-major
 * (read only), B [batch][n][nrhs] row-major, overwritten with X; n <= 192.  What the time-parallel combine
 * of a wide kernel uses for its W x W chunk maps instead of a blocked LAPACK LU (hundreds of launches per
 * call at this size).  A singular A gives garbage in X, never an error: the maps of chunks after a failed
 * pivot are singular by construction and are not used.  celerite2 has no counterpart (its factorisation
 * is sequential: celerite2.driver.factor, /root/reference/gadfly/gp.py:202).
 */
int gf_dense_solve(int batch, int n, int nrhs, const double *A, double *B, void *stream);
/* The same solve, with logdet_out [batch] <- log det A where det A > 0 (sum of log |pivot|; the sign from the
 * pivots' signs and the parity of the row permutation), NaN where det A <= 0 or A is singular / not finite. */
int gf_dense_solve_logdet(int batch, int n, int nrhs, const double *A, double *B, double *logdet_out,
                          void *stream);

/*
 * The dense combine of the time-parallel factorisation of a WIDE kernel (64 <= W <= 176), all of it in
 * this library (gadfly_dense.hip: batched FP64-MFMA GEMM tiles, mat-vecs and copies as "job" launches,
 * gf_dense_solve once per tree level).  celerite2 has no counterpart: its `factor` is sequential
 * (celerite2.driver.factor <- /root/reference/gadfly/gp.py:202, the reference's default kernel
 * /root/reference/gadfly/core.py:430-461 has W = 172).
 *
 * gf_wide_combine: one call between the nominal pass and the final pass of gf_chunk_sweep.
 *   in : h, dbar, zbar   rows of the nominal pass / gf_chunk_transition_wide ([B*N (+2)][ld], [B*N], [B*N];
 *                        ld = gf_fused_row_stride(0, Jc));
 *        Phi_state       [B*nch][gf_fused_state_size] closed-loop transitions (gf_chunk_transition_wide);
 *        S_state         [B*nch][gf_fused_state_size] END states of the nominal pass (zero start);
 *   out: S_state         the TRUE start state of every chunk (what the final pass starts from).
 *   The start states do not depend on the LAST chunk's map at all, and on the FIRST chunk's only through
 *   its end state: h, dbar, zbar and Phi_state are read for the chunks 1 .. nch - 2 only, S_state of the last
 *   chunk is not read -- the caller may skip the last chunk in the nominal pass and both end chunks in
 *   gf_chunk_transition_wide (chunk_first = 1, chunk_count = nch - 2).
 *   Steps: pack the states into dense W' x W' maps (W' = gf_dense_width(W), zero pads; identity maps pad
 *   nch to a power of two P) -> Gram sums G_c = sum h h^T / dbar, m_c = sum h zbar / dbar -> exclusive scan
 *   over the chunk maps (Blelloch, 2 log2 P - 2 levels of 3 job launches + 1 solve) -> unpack.
 *   work: gf_wide_combine_work(B, nch, Jc) doubles.  nch >= 2; B * P / 2 <= 65535.
 * gf_wide_gram, gf_lft_tree_scan: the two middle steps on dense arrays (maps [B*P][W'][W'] / [B*P][W'],
 *   row-major, W' a multiple of 16 <= 192, pads zero; symmetric G, Xbar): the scan returns the start
 *   states X_start [B*P][W'][W'], Y_start [B*P][W']; work: gf_lft_tree_work(B, P, W') doubles.
 * gf_bgemm: C_b = D_b + op(A_b) op(B_b) for b < batch (D may be NULL), row-major, any M, N, K and leading
 *   dimensions (even leading dimensions and 16-byte aligned bases take the vector-load path); strides in
 *   elements.  Used for the composed segment transitions and multi-right-hand-side chunk chains of the
 *   solves on a wide stored factor, and the conditional covariance.
 */
int gf_dense_width(int W);
int64_t gf_wide_combine_work(int B, int nch, int Jc);
int gf_wide_combine(int B, int64_t N, int64_t chunk_len, int nch, int Jc,
                    const double *h, const double *dbar, const double *zbar,
                    const double *Phi_state, double *S_state, double *acc, double *work, void *stream);
/*
 * Log-likelihood of a chunked series WITHOUT a final pass ("two sweeps").  With (X, Y) the true start state of
 * a chunk and (G, m) its Gram sums from the nominal pass,
 *     sum log d_n     = sum log dbar_n        + log det(I - X G)
 *     sum z_n^2 / d_n = sum zbar_n^2 / dbar_n + e^T G v - 2 m^T e - m^T X m,  e = Y - X m,  v = (I - X G)^-1 e,
 * so the caller reduces the NOMINAL rows (gf_reduce_tile on dbar, zbar of all chunks) and adds these
 * corrections: acc [B][3] (gf_reduce_tile's accumulators) += the sums over the chunks chunk_first ..
 * chunk_first + chunk_count - 1.  The nominal pass and the Gram sums must then cover the LAST chunk too
 * (gf_wide_combine with acc != NULL takes the Gram sums of chunks 1 .. nch - 1; pass NULL for the start
 * states alone).  A non-positive pivot ANYWHERE in the chunk makes the correction NaN -- the sign of EVERY pivot is
 * checked, not the parity det(I - X G) gives: with X = R R^T (Cholesky with diagonal pivoting to the numerical
 * rank) the chunk's pivots are all positive exactly when M = I - R^T G R is positive definite, decided by a
 * Cholesky attempt on M -- and the caller repeats such an evaluation with a final pass, which also names the failing
 * row (celerite2's LinAlgError semantics, reference gp.py:188-192).
 * gf_chunk_corrections: the W <= 63 route (state slots [B*nch][64*64] / [B*nch][64] after gf_chunk_combine[_tree];
 * W = the celerite width); one kernel per map: that check, then log det and v from an LU of I - X G with partial
 * pivoting (the values must not come from M: rounding residue of either sign in X's null directions cancels in
 * det(I - X G) and does not in a Cholesky factor);
 * work: gf_chunk_corrections_work(B, nch) doubles; B * nch <= 65535.
 */
int64_t gf_chunk_corrections_work(int B, int nch);
int gf_chunk_corrections(int B, int nch, int W, int chunk_first, int chunk_count, const double *S_state,
                         const double *F_state, const double *G, const double *m, double *acc, double *work,
                         void *stream);
int gf_wide_gram(int B, int64_t N, int64_t chunk_len, int nch, int chunk_first, int chunk_count, int P, int Jc,
                 const double *h, const double *dbar, const double *zbar,
                 double *G_out, double *m_out, void *stream);
int64_t gf_lft_tree_work(int B, int P, int WP);
int gf_lft_tree_scan(int B, int P, int WP, const double *Phi, const double *G, const double *Xbar,
                     const double *Ybar, const double *m, double *X_start, double *Y_start,
                     double *work, void *stream);
int gf_bgemm(int batch, int trans_a, int trans_b, int M, int N, int K,
             const double *A, int lda, int64_t stride_a, const double *B, int ldb, int64_t stride_b,
             const double *D, int ldd, int64_t stride_d, double *C, int ldc, int64_t stride_c,
             void *stream);

/*
 * Log-likelihood reductions (fixed-shape tree, deterministic):
 *   gf_reduce_tile   : acc[b] = {sum log d, sum z^2/d, min d} (THREE doubles per problem) over N
 *                      rows; init != 0 overwrites acc, init == 0 accumulates (tiles in order).
 *                      z == NULL: second sum is 0.  work: B * gf_reduce_work(N) doubles.
 *                      min d gives the condition estimate max(a) / min(d) that selects the
 *                      generator period (gen_period of gf_loglike_fused).
 *   gf_loglike_finish: out[b] = -0.5 (acc0 + Ntot log 2pi) - 0.5 acc1; logdet[b] = acc0
 *                      (either may be NULL); info[b] != 0 -> -inf for both.
 */
int64_t gf_reduce_work(int64_t N);
int gf_reduce_tile(int B, int64_t N, const double *d, const double *z,
                   double *work, double *acc, int init, void *stream);
int gf_loglike_finish(int B, int64_t N, const double *acc, const int32_t *info,
                      double *out, double *logdet, void *stream);

/*
 * Triangular sweeps with R right-hand sides, Y and Z are [B][N][R] row-major (Z may alias Y
 * for the two solves, not for GF_MATMUL_LOWER):
 *   GF_SOLVE_LOWER : F <- P_n (F + W_{n-1} Z_{n-1}),  Z_n = Y_n - U_n F          (n ascending)
 *   GF_SOLVE_UPPER : F <- P_{n+1} (F + U_{n+1} Z_{n+1}), Z_n = Y_n - W_n F       (n descending)
 *   GF_MATMUL_LOWER: F <- P_n (F + W_{n-1} Y_{n-1}),  Z_n = Y_n + U_n F          (n ascending)
 * `scale` [B][N] or NULL: if given, the input row is first multiplied by
 *   1/scale[n] (solve modes: fuses apply_inverse's division by d) or sqrt(scale[n])
 *   (GF_MATMUL_LOWER: dot_tril's sqrt(d) factor).
 */
int gf_solve(int mode, int B, int64_t N, int W, int ld, int R,
             const double *U, const double *Wm, const double *P, const double *scale,
             const double *Y, double *Z, void *stream);

/*
 * Chunk-parallel form of gf_solve for ONE right-hand side (any width; the wide stored factor's sweeps):
 *   gf_solve_chunk(store=0)  local pass: chunk c of nch sweeps its rows from F_state slot
 *                            (b * nch + c) [ld] (zeroed by the caller) and leaves its end state
 *                            there (pending push folded, the boundary's decay left to the receiver);
 *   combine                  on the caller's side: GF_MATMUL_LOWER has diagonal transitions
 *                            D_c = product of the chunk's propagator rows -> gf_chunk_diag_scan; the
 *                            solves chain F_{c+1} = loc_c + Phi_c F_c (G_{c-1} = loc_c + Phi_c^T G_c)
 *                            with the chunk transitions of the TRUE factor (gf_chunk_transition[_wide]);
 *   gf_solve_chunk(store=1)  final pass from the true start states: Z rows.
 * Y, Z [B][N] (Z may alias Y for the solves); scale as in gf_solve.
 */
int gf_solve_chunk(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int ld,
                   const double *U, const double *Wm, const double *P, const double *scale,
                   const double *Y, double *Z, double *F_state, int store, void *stream);
/* The same with R right-hand sides (Y, Z [B][N][R]; F_state [B * nch][ld][R]; B * nch <= 65535): the
 * conditional variance / covariance on a wide stored factor (celerite2: solve_lower / solve_upper with a
 * matrix right-hand side, /root/reference/gadfly/gp.py:295-304 through ConditionalDistribution). */
int gf_solve_chunk_rhs(int mode, int B, int64_t N, int64_t chunk_len, int nch, int W, int ld, int R,
                       const double *U, const double *Wm, const double *P, const double *scale,
                       const double *Y, double *Z, double *F_state, int store, void *stream);
int gf_chunk_diag_scan(int B, int nch, int rows, int R, const double *D, double *F_state, void *stream);

/*
 * Cross-covariance block for the conditional variance / covariance (celerite2's
 * ConditionalDistribution.variance builds it densely on the host; gp.py:295-304 is gadfly's use):
 *   out[b][n][r] = k(|t[n] - ts[r]|) from the celerite coefficients, layout [B][N][R] = the
 * right-hand-side layout of gf_solve / gf_chunk_linear, so K^-1 K(t, t*) follows without a copy.
 * t [B|1][N] (stride t_bs), ts [B|1][R] (stride ts_bs), R <= 4096.  For an exposure-integrated kernel
 * the coefficient form holds for lags >= delta only: the caller patches the few closer entries.
 */
int gf_cross_covariance(int B, int64_t N, int R, int Jr, int Jc,
                        const double *ar, const double *cr, const double *ac,
                        const double *bc, const double *cc, const double *dc,
                        const double *t, int64_t t_bs, const double *ts, int64_t ts_bs,
                        double *out, void *stream);

/*
 * Power spectral density of R evenly sampled series from their one-sided FFT (hipFFT's rfft,
 * interleaved complex [R][M], M = N/2 + 1): replaces the numpy expression of
 * PowerSpectrum._fft (gadfly/psd.py:566-587),
 *   power[r][k] = (re^2 + im^2)(spec[r][first + k]) * norm,   norm = d / sqrt(2 pi) / N,
 * power is [R][M - first]; first = 1 drops the zero frequency (include_zero_freq=False, psd.py:559-561).
 */
int gf_psd_power(int R, int64_t M, int64_t first, double norm, const double *spec,
                 double *power, void *stream);

/*
 * Binned power spectrum: replaces the two scipy.stats.binned_statistic passes of
 * bin_power_spectrum (gadfly/psd.py:229-300) with spectral_binning / spectral_binning_err
 * (psd.py:186-227) as statistics.  x [M] is the ascending frequency axis the bins were drawn on
 * (log10 frequency by default), power [R][M]; bin b holds the points start[b] <= i < start[b+1]
 * (start [nb+1], int64, ascending: the host applies binned_statistic's edge rules).  Per bin and
 * series: stat = trapz(power, x) / span, err = std(power) / sqrt(n) * mean(x) / span / constant,
 * span = x_last - x_first; a one-point (or zero-span) bin gives the point itself for both, an
 * empty bin NaN.  stat, err are [R][nb].
 */
int gf_psd_bin(int R, int64_t M, int nb, const double *x, const double *power,
               const int64_t *start, double constant, double *stat, double *err, void *stream);

/*
 * Lomb-Scargle power spectra of R (gapped, unevenly sampled) series: replaces PowerSpectrum._lomb_scargle
 * (gadfly/psd.py:589-601), i.e. astropy's LombScargle(t, y, normalization='psd').power(rfftfreq(n, d)) * norm
 * with its defaults (no dy, fit_mean, center_data, nterms = 1), as the exact direct sum over every (point,
 * frequency) pair -- not the Press-Rybicki approximation astropy's method='auto' picks for a regular grid.
 * Series r holds the points pt_off[r] <= i < pt_off[r+1] of t, y (concatenated, [n_total], n_r >= 2) and its
 * frequencies k df[r], first <= k <= n_r/2 (df = 1/(n_r d_r): rfftfreq's grid; first = 1 drops f = 0);
 * power[out_off[r] + k - first] = P(k df[r]) * norm[r] (out_off[r+1] - out_off[r] = n_r/2 + 1 - first).
 * pt_off, out_off [R+1] int64, df, norm [R] are device arrays; n_max = max n_r; S_max >= gf_ls_segments(n_max)
 * (a series' own segment count depends on n_r alone, so its result does not depend on the batch around it);
 * work: gf_ls_work(n_total, out_total, S_max) doubles, 32-byte aligned.  Degenerate frequencies (f = 0, the
 * Nyquist frequency of an even, evenly sampled series, a constant series) take the rank-one or zero limit
 * (DESIGN.md 3.6): no NaN or Inf reaches power.
 */
int gf_ls_segments(int64_t n);
int64_t gf_ls_work(int64_t n_total, int64_t out_total, int S_max);
int gf_ls_power(int R, int64_t n_max, int64_t n_total, int64_t out_total, int S_max, int first,
                const int64_t *pt_off, const int64_t *out_off, const double *df, const double *norm,
                const double *t, const double *y, double *work, double *power, void *stream);

/*
 * The same Lomb-Scargle power spectra (PowerSpectrum._lomb_scargle, gadfly/psd.py:589-601: what astropy's
 * LombScargle(...).power(rfftfreq(n, d)) computes there, gadfly/psd.py:596-600) through a non-uniform FFT, in
 * O(n log n): the seven sums from two type-1 transforms with real strengths, F_1(k) = sum_j e^{2 pi i k x_j}
 * (k <= 2 [n/2]) and F_y(k) = sum_j y'_j e^{2 pi i k x_j} (k <= [n/2]), x = frac((t - t_0) df).  Points are spread
 * onto a fine grid of n_f = gf_lsfft_grid(n) cells (the next 2-3-5-smooth integer >= 4 (2 [n/2] + 1) + 32) with
 * the kernel exp(beta (sqrt(1 - z^2) - 1)) of width 16 cells, beta = 36.8, the caller transforms the grids (rfft)
 * and gf_lsfft_finish deconvolves and forms the power with gf_ls_power's formula and degenerate limits.  The
 * result agrees with gf_ls_power within its own test bar (rtol 1e-8, atol 1e-10 max).
 * Layout: A time axes (axis a: the points ax_off[a] <= i < ax_off[a+1] of t, its fine grid the cells
 * cell_off[a] <= c < cell_off[a+1] of all grids' cells, df[a] = 1/(n d)); R >= A series (series r: the points
 * pt_off[r] <= i < pt_off[r+1] of y, on axis axis[r] of the same length; axes are numbered by their first series).
 * All offset arrays are int64 device arrays, df, norm double device arrays.  The steps of one call:
 *   gf_lsfft_prepare: key[i] <- cell_off[a] + floor(u_i), u[i] <- frac((t_i - t_0) df[a]) n_f (per axis point),
 *     yc <- (y - y_0) - mean per series (centred on the first value, then the mean, as gf_ls_power does; the mean
 *     from min(64, ceil(n/16384)) partial sums in order, part: gf_lsfft_part(R) doubles of scratch);
 *   the caller sorts key (stable) into skey with the permutation perm (int64);
 *   gf_lsfft_spread: start [cells + 1] (scratch) <- per-cell offsets into the sorted points; then
 *     grid[gy_off[r] + c] <- sum_j y'_j phi, and where g1_off[r] >= 0 grid[g1_off[r] + c] <- sum_j phi (the grid
 *     of ones of an axis is written by one of its series), c < n_f; each cell sums the points of its window in
 *     sorted order (no atomics).  n_axes = ax_off[A], cells = cell_off[A], nf_max the largest n_f;
 *   the caller transforms every grid: spec <- rfft(grid) (n_f/2 + 1 interleaved complex values each);
 *   gf_lsfft_finish: power[out_off[r] + k - first] <- P(k df) norm[r], first <= k <= n_r/2, from the transforms
 *     at sy_off[r] (of y') and s1_off[r] (of ones; offsets in complex values into spec, 16-byte aligned);
 *     quad [128]: 64 Gauss-Legendre nodes on [0, 1], then their weights.
 */
int64_t gf_lsfft_grid(int64_t n);
int64_t gf_lsfft_part(int R);
int gf_lsfft_prepare(int A, int R, int64_t n_max, const int64_t *ax_off, const int64_t *cell_off, const double *df,
                     const int64_t *pt_off, const double *t, const double *y, int64_t *key, double *u, double *yc,
                     double *part, void *stream);
int gf_lsfft_spread(int A, int R, int64_t n_axes, int64_t cells, int64_t nf_max, const int64_t *ax_off,
                    const int64_t *cell_off, const int64_t *pt_off, const int64_t *axis, const int64_t *gy_off,
                    const int64_t *g1_off, const int64_t *skey, const int64_t *perm, const double *u, const double *yc,
                    int64_t *start, double *grid, void *stream);
int gf_lsfft_finish(int R, int64_t n_max, int first, const int64_t *pt_off, const int64_t *out_off, const int64_t *axis,
                    const int64_t *cell_off, const int64_t *sy_off, const int64_t *s1_off, const double *norm,
                    const double *quad, const double *spec, double *power, void *stream);

/*
 * Missing cadences of an evenly sampled light curve filled by linear interpolation: replaces
 * interpolate_missing_data (gadfly/interp.py:6-60; called at psd.py:495, :531 before every FFT).
 * t, f [N] ascending times and fluxes; cadences [N] int64 or NULL (then the cadence index of a
 * point is rint((t - t[0]) / dt), interp.py:41-44); dt = the median spacing per cadence
 * (interp.py:36, :40), computed by the caller.
 *   gf_interp_plan: offsets [N + 1] <- i + (number of cadences missing before point i),
 *     offsets[N] = length of the filled series; work = gf_interp_work(N) int64 words of scratch.
 *   gf_interp_fill: t_out, f_out [offsets[N]] <- the input points and the missing cadences at their
 *     grid times t[0] + index * dt (interp.py:51) with flux np.interp(x, t, f) (interp.py:54: the
 *     chord of the interval that holds x, each operation rounded on its own -- bit-identical to the
 *     numpy result), merged in time order (the reference's argsort, interp.py:57-59; with cadence
 *     numbers given the grid may drift past neighbouring time stamps, so positions are ranks).
 * Both read t[0] back to the host (one 8-byte copy, a stream synchronisation).
 */
int64_t gf_interp_work(int64_t N);
int gf_interp_plan(int64_t N, const double *t, const int64_t *cadences, double dt,
                   int64_t *offsets, int64_t *work, void *stream);
int gf_interp_fill(int64_t N, const double *t, const double *f, const int64_t *cadences, double dt,
                   const int64_t *offsets, double *t_out, double *f_out, void *stream);

/*
 * Conditional mean at M new (sorted) times t1 given alpha = K^-1 (y - mean) at the N
 * observed times t2:
 *   mu[m] = sum_{t2[n] <= t1[m]} (U1[m] o e^{-c (t1[m]-t2[n])}) . V2[n] alpha[n]
 *         + sum_{t2[n] >  t1[m]} (V1[m] o e^{-c (t2[n]-t1[m])}) . U2[n] alpha[n]
 *   c [B][W]; U1, V1 [B][M][ld]; U2, V2, P2 [B][N][ld]; t1 [B|1][M]; t2 [B|1][N]
 *   qidx [B][M] (int64): number of observed rows with t2 <= t1[m] (searchsorted, side "right");
 *   work: gf_general_matmul_work(B, M, N, W) doubles.
 * Long series are swept chunk-parallel (the recurrence is a decayed prefix sum: local pass,
 * scan of the chunk states, second pass over the chunks that contain queries).
 */
int64_t gf_general_matmul_work(int B, int64_t M, int64_t N, int W);
int gf_general_matmul(int B, int64_t M, int64_t N, int W, int ld,
                      const double *c,
                      const double *t1, int64_t t1_bs, const double *U1, const double *V1,
                      const double *t2, int64_t t2_bs, const double *U2, const double *V2,
                      const double *P2, const double *alpha, const int64_t *qidx,
                      double *work, double *mu, void *stream);

/*
 * Log-likelihoods of B problems and their gradients with respect to the celerite coefficients:
 * the reverse-mode ops celerite2 ships for its JAX / PyMC interfaces (driver.factor_rev, driver.solve_lower_rev
 * and the adjoint of -1/2 (z^T D^-1 z + sum log D)), on the plain recurrence of oracle/celerite_ref.c with exact
 * generator rows at every row (theta_n = fl(d t_n)).  One wave per problem; W = Jr + 2 Jc <= 63 (-3 beyond).
 *   coefficients as gf_build_matrices: ar, cr [B][max(Jr,1)]; ac, bc, cc, dc [B][max(Jc,1)]; diag_add [B]
 *     (A_n = diag[n] + diag_add); t, diag, y with batch strides in elements (0 = shared; diag may be NULL)
 *   work: work_bs >= gf_grad_work(N, W) doubles per problem (checkpoints of the forward sweep and one segment's
 *     staged rows); B * work_bs in all
 *   ll [B]      log-likelihood, -inf where a pivot is not positive (info = the 1-based failing row)
 *   g_real [2][B][max(Jr,1)]      d log L / d (ar, cr)
 *   g_comp [4][B][max(Jc,1)]      d log L / d (ac, bc, cc, dc)
 *   g_diag [B]  d log L / d diag_add = sum_n d log L / d A_n   (a constant added to the diagonal)
 *   g_mean [B]  d log L / d mean = sum_n alpha_n               (y holds the data minus a constant mean)
 *   every gradient of a failed problem is NaN.  No atomics: results are bit-identical from run to run and do not
 *   depend on the other problems of the call.
 */
int64_t gf_grad_work(int64_t N, int W);
int gf_loglike_grad(int B, int64_t N, int Jr, int Jc,
                    const double *ar, const double *cr, const double *ac, const double *bc,
                    const double *cc, const double *dc, const double *diag_add,
                    const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                    const double *y, int64_t y_bs, double *work, int64_t work_bs,
                    double *ll, double *g_real, double *g_comp, double *g_diag, double *g_mean,
                    int32_t *info, void *stream);

/*
 * The same log-likelihoods and gradients, time-parallel: every series is cut into chunks of
 * chunk_len rows (the last may be shorter; values above N mean N, one chunk) that are swept concurrently, one wave per
 * (problem, chunk) -- a nominal pass from zero states and gf_chunk_combine[_tree] for the true start state of every chunk, a
 * forward pass from those, and three reverse sweeps stitched by two scans over the chunks (across a chunk the adjoint
 * recurrence is affine, its linear part the chunk's closed-loop transition).  For one long series, or a few; many short
 * ones are gf_loglike_grad's.  W = Jr + 2 Jc <= 63 (-3 beyond).
 *   gf_grad_chunk_len(B, N, W)   the default chunk length (0 for a shape the call would refuse)
 *   coefficients, t, diag, y, their strides and every output as gf_loglike_grad, in the same layout
 *   work: work_bs >= gf_grad_chunked_work(N, W, chunk_len) doubles per problem (chunk maps, start states, the
 *     checkpoints and one segment's staged rows of every chunk, adjoint sources, partial sums); B * work_bs in all.
 *     The arrays lie one after the other over the problems of the call, not problem by problem
 *   a problem with a non-positive pivot in any pass: ll = -inf, every gradient NaN, info > 0 -- the 1-based row of the
 *     sequential recurrence's first failing pivot whenever the nominal pass was clean.  The other problems are unaffected
 * No atomics: results are bit-identical from run to run; a problem's bits depend on its own data, N and chunk_len alone.
 */
int64_t gf_grad_chunk_len(int B, int64_t N, int W);
int64_t gf_grad_chunked_work(int64_t N, int W, int64_t chunk_len);
int gf_loglike_grad_chunked(int B, int64_t N, int64_t chunk_len, int Jr, int Jc,
                            const double *ar, const double *cr, const double *ac, const double *bc,
                            const double *cc, const double *dc, const double *diag_add,
                            const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                            const double *y, int64_t y_bs, double *work, int64_t work_bs,
                            double *ll, double *g_real, double *g_comp, double *g_diag, double *g_mean,
                            int32_t *info, void *stream);

/*
 * Gradients for wide kernels: gf_loglike_grad's mathematics, layouts, outputs and failure
 * convention with one WORKGROUP of several waves per problem, for 1 <= W = Jr + 2 Jc <= gf_grad_wide_max_width()
 * (>= 176: gadfly's 86-term default kernel is W = 172; -3 beyond, the limit in gf_last_error()).  Narrow widths are
 * accepted, so that the route can be set against gf_loglike_grad on one problem (same results to rounding, not to
 * the bit).
 *   gf_grad_wide_seg(N, W)          default rows per segment (0 for a shape the call refuses)
 *   gf_grad_wide_work(N, W, seg)    doubles per problem (0 for a shape the call refuses): the checkpoints, one
 *                                   segment's staged rows and one parked matrix
 *   seg: rows per segment, 0 = gf_grad_wide_seg(N, W) (values above N mean N).  Every output is bit-identical for
 *     every seg: it trades workspace against recomputation only
 *   coefficients, t, diag, y, their strides and every output as gf_loglike_grad; work_bs >= gf_grad_wide_work
 *   a problem with a non-positive pivot: ll = -inf, info = the 1-based failing row, every gradient NaN; the other
 *     problems are unaffected
 * No atomics: results are bit-identical from run to run; a problem's bits depend on its own data, N and W alone.
 */
int gf_grad_wide_max_width(void);
int64_t gf_grad_wide_seg(int64_t N, int W);
int64_t gf_grad_wide_work(int64_t N, int W, int64_t seg);
int gf_loglike_grad_wide(int B, int64_t N, int64_t seg, int Jr, int Jc,
                         const double *ar, const double *cr, const double *ac, const double *bc,
                         const double *cc, const double *dc, const double *diag_add,
                         const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                         const double *y, int64_t y_bs, double *work, int64_t work_bs,
                         double *ll, double *g_real, double *g_comp, double *g_diag, double *g_mean,
                         int32_t *info, void *stream);

/*
 * alpha = K^-1 y and the conditional means of B problems: what celerite2's
 * GaussianProcess.apply_inverse (driver.factor + solve_lower + solve_upper) and predict(y[, kernel=component]) at the
 * observed times (general_matmul_lower + general_matmul_upper at t* = t) give one kernel at a time, on the plain
 * recurrence of oracle/celerite_ref.c with exact generator rows at every row.  One wave per problem; W = Jr + 2 Jc
 * <= 63 and W' = Jr2 + 2 Jc2 <= 63 (-3 beyond).  No stored factor: a forward sweep with checkpoints every `seg` rows,
 * then the upper solve backwards over segments recomputed from them.
 *   coefficients, t, diag, y and their strides as gf_loglike_grad (A_n = diag[n] + diag_add; diag may be NULL)
 *   component (optional): a second coefficient set ar2, cr2 [B][max(Jr2,1)]; ac2 .. dc2 [B][max(Jc2,1)].  Pass
 *     Jr2 = Jc2 = 0 and mu_comp = NULL for none; a component and mu_comp go together (-1 otherwise)
 *   seg: rows per segment, 0 = gf_solve_batch_seg(N, W) (values above N mean N).  Every output is bit-identical for
 *     every seg
 *   work: work_bs >= gf_solve_batch_work(N, W, seg) doubles per problem (checkpoints, one segment's staged rows,
 *     z and D of every row); B * work_bs in all
 *   alpha [B][N]    K^-1 y                                                   (may be NULL)
 *   mu [B][N]       y - diag alpha: the observational diagonal only, not diag_add; diag = NULL gives y   (may be NULL)
 *   mu_comp [B][N]  sum_m k'(t_n - t_m) alpha_m over ALL m, the coincident stamp with the earlier ones; the
 *                   component's own diagonal shift is not added (celerite2's predict(y, kernel=...))
 *   ll [B]          log-likelihood, -inf where a pivot is not positive (info = the 1-based failing row); every row of
 *                   alpha, mu and mu_comp of such a problem is NaN
 * No atomics: results are bit-identical from run to run and do not depend on the other problems of the call.
 */
int64_t gf_solve_batch_seg(int64_t N, int W);
int64_t gf_solve_batch_work(int64_t N, int W, int64_t seg);
int gf_solve_batch(int B, int64_t N, int Jr, int Jc,
                   const double *ar, const double *cr, const double *ac, const double *bc,
                   const double *cc, const double *dc, const double *diag_add,
                   int Jr2, int Jc2,
                   const double *ar2, const double *cr2, const double *ac2, const double *bc2,
                   const double *cc2, const double *dc2,
                   const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                   const double *y, int64_t y_bs, int64_t seg, double *work, int64_t work_bs,
                   double *alpha, double *mu, double *mu_comp, double *ll, int32_t *info, void *stream);

/*
 * alpha = K^-1 y and the conditional means for wide kernels: gf_solve_batch's mathematics, layouts,
 * outputs and failure convention without a component, with one WORKGROUP of several waves per problem, for
 * 1 <= W = Jr + 2 Jc <= gf_solve_wide_max_width() (192: gadfly's 86-term default kernel is W = 172; -3 beyond, the
 * limit in gf_last_error()).  Narrow widths are accepted, so that the route can be set against gf_solve_batch on one
 * problem (same results to rounding, not to the bit).  A component's share comes from gf_predict_batch_at on alpha.
 *   gf_solve_wide_seg(N, W)         default rows per segment (0 for a shape the call refuses)
 *   gf_solve_wide_work(N, W, seg)   doubles per problem (0 for a shape the call refuses): ceil(N / seg) checkpoints
 *                                   of (NC + 4) RT doubles, one segment of staged rows at 3 RT each, z and D of every
 *                                   row; RT = NC = 64, 128, 192 for W <= 64, <= 128, <= 192
 *   coefficients, diag_add, t, diag, y and their strides as gf_solve_batch (0 = shared, otherwise at least N; diag
 *     may be NULL)
 *   seg: rows per segment, 0 = gf_solve_wide_seg(N, W) (values above N mean N).  Every output is bit-identical for
 *     every seg
 *   work: work_bs >= gf_solve_wide_work(N, W, seg) doubles per problem; B * work_bs in all.  What it holds on entry
 *     does not matter
 *   alpha [B][N]    K^-1 y                                                   (may be NULL)
 *   mu [B][N]       y - diag alpha; diag = NULL gives y                      (may be NULL)
 *   ll [B]          log-likelihood, -inf where a pivot is not positive (info = the 1-based failing row); every row of
 *                   alpha and mu of such a problem is NaN, the other problems are unaffected to the bit
 * Returns -1 for bad shapes, strides, null pointers or a short work_bs, all checked before any device call.
 * No atomics: results are bit-identical from run to run and do not depend on the other problems of the call.
 */
int gf_solve_wide_max_width(void);
int64_t gf_solve_wide_seg(int64_t N, int W);
int64_t gf_solve_wide_work(int64_t N, int W, int64_t seg);
int gf_solve_batch_wide(int B, int64_t N, int Jr, int Jc,
                        const double *ar, const double *cr, const double *ac, const double *bc,
                        const double *cc, const double *dc, const double *diag_add,
                        const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                        const double *y, int64_t y_bs, int64_t seg, double *work, int64_t work_bs,
                        double *alpha, double *mu, double *ll, int32_t *info, void *stream);

/*
 * Conditional means of B problems at new times t* (DESIGN.md 3.11): what celerite2's general_matmul_lower +
 * general_matmul_upper between two sorted axes give one kernel at a time (GaussianProcess.predict(y, t=t*) after
 * apply_inverse), for alpha = K^-1 (y - mean) already on the device (gf_solve_batch):
 *     mu[b][m] = sum_{t_n <= t*_m} (U*_m o e^{-c (t*_m - t_n)}) . V_n alpha_n
 *              + sum_{t_n >  t*_m} (V*_m o e^{-c (t_n - t*_m)}) . U_n alpha_n
 * an observed stamp that coincides with a query counting in the first sum.  Exact generator rows on every row, made in
 * registers (no U, V, P arrays, no workspace).  One wave per problem; W = Jr + 2 Jc <= 63 (-3 beyond).
 *   coefficients as gf_solve_batch: ar, cr [B][max(Jr,1)]; ac, bc, cc, dc [B][max(Jc,1)] -- of the full kernel or
 *     of one of its parts (the share of that part at t*)
 *   t [N], ts [M]: observed and query stamps, ascending per problem, batch strides in elements (0 = shared)
 *   nobs, nq [B] (either may be NULL: N, M): the real observed rows and the real queries of problem b, clamped to
 *     0 .. N and 0 .. M; t and alpha from nobs[b] on are never read, mu from nq[b] on is never written
 *   alpha [B][alpha_bs >= N], mu [B][mu_bs >= M] (the strides are not looked at when B = 1)
 * A problem whose alpha is NaN (a failed gf_solve_batch) gets NaN in all its rows.  No atomics: results are
 * bit-identical from run to run, do not depend on the other problems of the call, and a query's value does not
 * depend on the other queries of its problem.
 */
int gf_predict_batch_at(int B, int64_t N, int64_t M, int Jr, int Jc,
                        const double *ar, const double *cr, const double *ac,
                        const double *bc, const double *cc, const double *dc,
                        const double *t, int64_t t_bs, const int64_t *nobs,
                        const double *ts, int64_t ts_bs, const int64_t *nq,
                        const double *alpha, int64_t alpha_bs,
                        double *mu, int64_t mu_bs, void *stream);

/*
 * gf_solve_batch for R right-hand sides per problem: alpha_r = K^-1 y_r, mu_r = y_r - diag alpha_r and
 * the log-likelihood of every y_r, the factor rows, decays, state update and pivot of each row made ONCE for the RB =
 * gf_solve_batch_rhs_block(W) right-hand sides a wave carries.  The ceil(R / RB) blocks of a problem are the grid's
 * second dimension (they run side by side, each on its own slice of the workspace).  No component.
 *   coefficients, t, diag, seg as gf_solve_batch
 *   y [B][R][N]: batch stride y_bs (0 = shared by all problems), right-hand-side stride y_rs >= N
 *   work: work_bs >= gf_solve_batch_rhs_work(N, W, R, seg) doubles per problem
 *   alpha, mu [B][R][N] (either may be NULL): batch stride out_bs >= R N, right-hand-side stride out_rs >= N
 *   ll [B][R] (contiguous), info [B]
 * Column r of alpha, mu and ll has the bits gf_solve_batch gives for y_r alone, for every R, seg and batch; info is
 * gf_solve_batch's.  A problem whose pivot fails gets NaN in every row of every right-hand side, -inf in its row of ll
 * and the 1-based failing row in info; the other problems are unaffected.  No atomics.
 * Returns -1 for bad shapes (R < 1 among them), strides or null pointers, -3 for W > 63.
 */
int gf_solve_batch_rhs_block(int W);
int64_t gf_solve_batch_rhs_work(int64_t N, int W, int R, int64_t seg);
int gf_solve_batch_rhs(int B, int64_t N, int R, int Jr, int Jc,
                       const double *ar, const double *cr, const double *ac, const double *bc,
                       const double *cc, const double *dc, const double *diag_add,
                       const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                       const double *y, int64_t y_bs, int64_t y_rs, int64_t seg, double *work, int64_t work_bs,
                       double *alpha, double *mu, int64_t out_bs, int64_t out_rs, double *ll, int32_t *info,
                       void *stream);

/*
 * gf_predict_batch_at for R columns of alpha per problem: generator rows, sincos and exp made once per
 * observed row and per query, the two sums carried for gf_predict_batch_at_rhs_block() columns at a time (the blocks
 * are the grid's second dimension).  Same tie rule, nobs / nq semantics and NaN propagation.
 *   alpha [B][R][N]: strides alpha_bs >= R N, alpha_rs >= N;  mu [B][R][M]: strides mu_bs >= R M, mu_rs >= M
 * Column r of mu has the bits gf_predict_batch_at gives for alpha_r alone.  No workspace, no LDS, no atomics.
 */
int gf_predict_batch_at_rhs_block(void);
int gf_predict_batch_at_rhs(int B, int64_t N, int64_t M, int R, int Jr, int Jc,
                            const double *ar, const double *cr, const double *ac,
                            const double *bc, const double *cc, const double *dc,
                            const double *t, int64_t t_bs, const int64_t *nobs,
                            const double *ts, int64_t ts_bs, const int64_t *nq,
                            const double *alpha, int64_t alpha_bs, int64_t alpha_rs,
                            double *mu, int64_t mu_bs, int64_t mu_rs, void *stream);

/*
 * Conditional variances of B problems: the second half of celerite2's
 * GaussianProcess.predict(y, t, return_var=True) -- the diagonal of K* - K*^T Sigma^-1 K*, one right-hand side per query
 * through the stored factor there -- for B kernels at once and with no stored factor: gf_solve_batch's two passes with
 * one more, matrix-valued, backward recurrence Y over the rows they stage, O((N + M) W^2) per problem.  One wave per
 * problem; W = Jr + 2 Jc <= 63 (-3 beyond).
 *   coefficients, diag_add, t, diag, y, their strides and seg as gf_solve_batch (A_n = diag[n] + diag_add: diag is
 *     the observational noise, diag_add the kernel's value at lag 0; diag may be NULL), no component
 *   ts [M], ts_bs, nobs, nq [B] as gf_predict_batch_at: ascending query stamps, the real observed rows (the rows from
 *     nobs[b] on are missing-data rows at the end: they own no query) and the real queries of problem b (either count
 *     may be NULL: N, M).  M = 0: no queries, ts and var_at NULL
 *   work: work_bs >= gf_var_batch_work(N, W, M, seg) doubles per problem (gf_solve_batch's workspace, one slot of
 *     64 max(16, 32, 64 >= W) doubles for Y, 64 per query); B * work_bs in all
 *   alpha, mu [B][N]  as gf_solve_batch, with its bits                           (each may be NULL)
 *   hdiag [B][N]      h_n = (Sigma^-1)_nn, Sigma = K + diag: the leave-one-out variance is 1 / h_n and the
 *                     leave-one-out mean y_n - alpha_n / h_n                     (may be NULL)
 *   var [B][N]        diag_n - diag_n^2 h_n = K(0) - K_n Sigma^-1 K_n^T: the conditional variance of the noise-free
 *                     process at t_n, exactly 0 where diag_n = 0 (and with diag = NULL)   (may be NULL)
 *   var_at [B][M]     K(0) - K(t*, t) Sigma^-1 K(t, t*) at the queries, K(0) = diag_add and the kernel in its
 *                     coefficient form at every lag; a query that coincides with an observed stamp belongs to the
 *                     interval after it.  Rows from nq[b] on are never written.  Required iff M > 0 (-1 otherwise)
 *   ll, info [B]      as gf_solve_batch; a problem whose pivot fails gets NaN in every row of every output
 * No atomics: results are bit-identical from run to run, for every seg, and do not depend on the other problems of
 * the call.
 */
int64_t gf_var_batch_work(int64_t N, int W, int64_t M, int64_t seg);
int gf_var_batch(int B, int64_t N, int Jr, int Jc,
                 const double *ar, const double *cr, const double *ac, const double *bc,
                 const double *cc, const double *dc, const double *diag_add,
                 const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                 const double *y, int64_t y_bs,
                 const double *ts, int64_t ts_bs, int64_t M, const int64_t *nobs, const int64_t *nq,
                 int64_t seg, double *work, int64_t work_bs,
                 double *alpha, double *mu, double *hdiag, double *var, double *var_at,
                 double *ll, int32_t *info, void *stream);

/*
 * Spectral log-likelihoods of B sums of J SHO terms against observed power spectra, their gradients and the model
 * spectra: the objective behind gadfly's hyperparameters.json (notebooks/virgo_lc.ipynb: chi-square
 * of TermConvolution.get_psd against the binned spectrum) and the Whittle likelihood of a periodogram.  With
 * omega = 2 pi f (f in uHz), exposure delta[b] >= 0 and white floor floor[b] >= 0 (NULL = 0):
 *     S_b(w) = sinc^2(delta_b w / 2) sum_j sqrt(2/pi) S0_j w0_j^4 / (((w - w0_j)(w + w0_j))^2 + w^2 w0_j^2 / Q_j^2) + c_b
 *     objective 0 (whittle):  ll_b = - sum_k n_k (ln S_b(w_k) + P_k / S_b(w_k))     weight = n_k, NULL = 1
 *     objective 1 (chi2):     ll_b = - 1/2 sum_k ((P_k - S_b(w_k)) / e_k)^2          weight = e_k, required
 * over the USED frequencies: P_k and its weight finite, the weight positive; used[b] counts them.
 *   S0, w0, Q [B][J]; delta [B]; omega [M] shared; power / weight with batch strides in elements (0 = one spectrum
 *     for every problem); J <= 256 (-3 beyond), M >= 1, B <= 65535 per call
 *   work: gf_spectral_work(B, M, J) doubles (0 for a shape outside the limits); a problem's share, and so its result,
 *     depends on M and J alone
 *   ll [B], used [B], info [B]: where S_b(w_k) is not > 0 at a used frequency, ll = -inf, every gradient of the
 *     problem is NaN and info = k + 1 for the first such k (0 otherwise)
 *   gS0, gw0, gQ [B][J], gfloor [B]: d ll_b / d (S0, w0, Q, c); each may be NULL, all NULL = value only (the value
 *     has the same bits either way)
 *   model [B][M] (or NULL): S_b(w_k) at every frequency, used or not
 * gf_spectral_tile(): the frequencies one workgroup takes.  No atomics: results are bit-identical from run to run and
 * do not depend on the other problems of the call.
 */
int gf_spectral_tile(void);
int64_t gf_spectral_work(int B, int64_t M, int J);
int gf_spectral_like(int B, int64_t M, int J, int objective,
                     const double *S0, const double *w0, const double *Q,
                     const double *delta, const double *floor, const double *omega,
                     const double *power, int64_t power_bs, const double *weight, int64_t weight_bs,
                     double *work, double *ll, int64_t *used, int32_t *info,
                     double *gS0, double *gw0, double *gQ, double *gfloor,
                     double *model, void *stream);

/*
 * Fisher information of the spectral objectives: per problem the weighted Gram matrix of the model
 * spectrum's Jacobian over the used frequencies,
 *     F_b = sum_k v_k grad S_b(w_k) grad S_b(w_k)^T,    v_k = n_k / S_b(w_k)^2 (whittle),  v_k = 1 / e_k^2 (chi2)
 * the Gauss-Newton matrix of chi2 and the expected information of Whittle (minus the Hessian where P = S).  The
 * arguments, limits, status codes and the rule for USED frequencies are gf_spectral_like's; P_k enters through that
 * rule alone.
 *   fisher [B][P][P], P = 3 J + 1, in the parameter order S0_0 .. S0_{J-1}, w0_0 .., Q_0 .., floor: exactly symmetric,
 *     diagonal >= 0; unused frequencies add exact zeros (no used frequency: a matrix of zeros)
 *   used [B], info [B]: what gf_spectral_like returns for the same inputs; where S_b(w_k) is not > 0 at a used
 *     frequency the problem's whole matrix is NaN (info = k + 1), the other problems are not touched
 *   work: gf_spectral_fisher_work(B, M, J) doubles (0 for a shape outside the limits); a problem's share, and so its
 *     result, depends on M and J alone
 * gf_spectral_fisher_slab(): the frequencies summed into one partial; the partials are added in slab order.  No
 * atomics: a problem's matrix is bit-identical from run to run and does not depend on the other problems of the call.
 */
int gf_spectral_fisher_slab(void);
int64_t gf_spectral_fisher_work(int B, int64_t M, int J);
int gf_spectral_fisher(int B, int64_t M, int J, int objective,
                       const double *S0, const double *w0, const double *Q,
                       const double *delta, const double *floor, const double *omega,
                       const double *power, int64_t power_bs, const double *weight, int64_t weight_bs,
                       double *work, double *fisher, int64_t *used, int32_t *info, void *stream);

/*
 * Raw observing quarters to detrended series: the steps of the detrend=True branch of
 * PowerSpectrum.from_light_curve (gadfly/psd.py:482-535) that are not the gap fill, on S segments (star x quarter) at
 * once.  Segment s owns the elements off[s] .. off[s + 1] - 1 of the concatenated arrays (off [S + 1] int64,
 * ascending; an empty segment is allowed).  One workgroup per segment, no floating-point atomics, every sum in a
 * fixed order: a segment's result bits depend on its own data alone.  All return -1 for S < 1 or a null pointer.
 *   gf_seg_median: med [S] <- numpy.median of each segment's finite values, to the bit (an even count gives
 *     (a + b) / 2 of the two middle elements; -0 counts as +0; NaN for no element).  keep [off[S]] (uint8) or NULL:
 *     only elements with keep != 0 count.  drop_last = 1 leaves each segment's last slot out (x then holds the
 *     n - 1 differences that the diff entry point below wrote into the segment's n slots), 0 takes all.
 *   gf_sigma_clip: astropy's sigma_clip(cenfunc=median, stdfunc=std) as lightkurve's remove_outliers runs it, all
 *     rounds in one launch.  keep <- rows with finite f (and finite t, unless t is NULL); then per round med and the
 *     population standard deviation sd (two passes, ddof 0) of the kept rows, keep only
 *     med - sigma_lower sd <= f <= med + sigma_upper sd, stop after the round that removed nothing or after
 *     maxiters rounds (maxiters < 0: no cap; 0: only the finite rows are selected, the sigmas are not read).
 *     kept [S] (int64) <- rows kept, rounds [S] (int32) <- rounds run.  -1 unless both sigmas are > 0.
 *   gf_seg_compact: the kept rows of (t, f) in their order, packed: new_off [S + 1] <- offsets of the packed
 *     segments, t_out, f_out [up to off[S]] <- the rows.
 *   gf_seg_diff: d[off[s] + i] <- t[off[s] + i + 1] - t[off[s] + i] for i < n_s - 1 (the last slot is set to 0).
 *   gf_poly_normalise: the least-squares polynomial of degree `order` (0 .. GF_DETREND_MAX_ORDER, else -1) of f over
 *     t per segment, and normed <- f / fit.  Basis: Legendre polynomials of u = (t - mid) / half, mid and half from
 *     the segment's first and last time (u = 0 where they coincide) -- the space numpy.polyfit(t - mean(t), f, order)
 *     fits; Gram matrix and right-hand side in float64, Cholesky on chip.  info [S] (int32) <- 0, or the 1-based
 *     index of the pivot that was not positive (an empty segment: 1); such a segment's normed is NaN, the others are
 *     not touched.
 *   gf_seg_ppm: out <- 1e6 (x / med[s] - 1) (out may be x).
 */
#define GF_DETREND_MAX_ORDER 8
int gf_seg_median(int S, const int64_t *off, const double *x, const uint8_t *keep, int drop_last, double *med,
                  void *stream);
int gf_sigma_clip(int S, const int64_t *off, const double *t, const double *f, double sigma_lower,
                  double sigma_upper, int maxiters, uint8_t *keep, int64_t *kept, int32_t *rounds, void *stream);
int gf_seg_compact(int S, const int64_t *off, const uint8_t *keep, const double *t, const double *f,
                   int64_t *new_off, double *t_out, double *f_out, void *stream);
int gf_seg_diff(int S, const int64_t *off, const double *t, double *d, void *stream);
int gf_poly_normalise(int S, const int64_t *off, const double *t, const double *f, int order, double *normed,
                      int32_t *info, void *stream);
int gf_seg_ppm(int S, const int64_t *off, const double *x, const double *med, double *out, void *stream);

/*
 * The gap fill of S series in one call: interpolate_missing_data (gadfly/interp.py:6-60, what the reference runs
 * before every FFT spectrum, psd.py:495, :531) over the segment layout above.  Segment s owns the elements
 * off[s] .. off[s + 1] - 1 (off [S + 1] int64, ascending, off[S] = total; an empty segment is allowed) of t, f and
 * cadences (int64, or NULL: the cadence index of a point is rint((t - t_0) / dt[s]) with t_0 = t[off[s]], read on
 * the device).  dt [S] float64 ON THE DEVICE; which [S] uint8 or NULL for all: a segment with which[s] == 0 is
 * copied and its dt[s] is not read.  Per point the rules of gf_interp_plan / gf_interp_fill with every index and
 * search local to the segment: a segment's result is, bit for bit, what those give for it alone.  One count per
 * point, one scan over the whole concatenation, one thread per point and per gap -- one long segment stays parallel.
 * Nothing is copied to the host and nothing synchronises.  All return -1 for S < 1, total < 0 or a null pointer.
 *   gf_interp_plan_seg: plan [total + 1] <- exclusive scan over the concatenation of 1 + (cadences missing after
 *     the point) (1 for a segment's last point and for every point of a copied segment), plan[total] = length of the
 *     filled concatenation; new_off [S + 1] <- plan[off[s]], the offsets of the filled segments; info [S] (int32)
 *     <- 0, or 1 where a selected, non-empty segment's dt is not a positive finite number: that segment is copied.
 *     work: gf_interp_seg_work(total) int64 words of scratch.
 *   gf_interp_fill_seg: t_out, f_out [plan[total]] <- each segment's input points and missing cadences, merged in
 *     time order, from new_off[s] on.
 */
int64_t gf_interp_seg_work(int64_t total);
int gf_interp_plan_seg(int S, int64_t total, const int64_t *off, const double *t, const int64_t *cadences,
                       const double *dt, const uint8_t *which, int64_t *plan, int64_t *new_off, int32_t *info,
                       int64_t *work, void *stream);
int gf_interp_fill_seg(int S, int64_t total, const int64_t *off, const double *t, const double *f,
                       const int64_t *cadences, const double *dt, const uint8_t *which, const int64_t *plan,
                       double *t_out, double *f_out, void *stream);

/*
 * Linear mean models under B kernels: y = A beta + eps, eps ~ N(0, Sigma_b), Sigma_b = K_b + diag.
 * With Sigma = L D L^T and Z = L^-1 [A | y], one forward sweep gives everything a generalised least squares fit needs:
 *   gram [B][R + 1][R + 1] = [A | y]^T Sigma^-1 [A | y] = Z^T D^-1 Z (contiguous, equal to its transpose bit for bit),
 *   logdet [B] = sum_n log D_n,  info [B] (int32) = 0, or the 1-based row whose pivot fails.
 * No upper solve, no checkpoints, nothing of size N is returned.
 *   coefficients, diag_add, t, diag, y with their batch strides as gf_solve_batch
 *   nobs [B] int64 or NULL: the sweep of problem b stops after nobs[b] rows (held to 0 .. N); later rows of t, diag,
 *     y and A are never read
 *   A [B][N][R], row-major: row stride lda >= R, batch stride a_bs (0 = one matrix shared by all problems)
 *   work: work_bs >= gf_linear_gram_work(N, W, R) doubles per problem (z_n / sqrt(D_n) of every row and column)
 * One workgroup per problem and block of 64 columns of [A | y]: one wave runs gf_solve_batch's forward row (D and
 * info are gf_solve_batch's), a second one carries a column per lane; a second kernel sums the products over the rows
 * in one fixed order.  A problem's outputs have the same bits whatever the batch around it, and the entries among the
 * first r columns and y have the same bits whatever further columns A holds.  A problem whose pivot fails gets NaN in
 * gram and logdet; the other problems are unaffected.  No atomics.
 * Returns -1 for bad shapes (R < 1 or R > 255 among them), strides or null pointers, -3 for W > 63;
 * gf_linear_gram_work returns 0 for them.
 */
int64_t gf_linear_gram_work(int64_t N, int W, int R);
int gf_linear_gram(int B, int64_t N, int R, int Jr, int Jc,
                   const double *ar, const double *cr, const double *ac, const double *bc,
                   const double *cc, const double *dc, const double *diag_add,
                   const double *t, int64_t t_bs, const double *diag, int64_t diag_bs,
                   const double *y, int64_t y_bs, const int64_t *nobs,
                   const double *A, int64_t lda, int64_t a_bs, double *work, int64_t work_bs,
                   double *gram, double *logdet, int32_t *info, void *stream);

/*
 * Quadratic forms of the kernel's derivatives: for B problems with R vectors x_r of N rows each,
 *     Q' = sum_r w_r x_r^T (d Sigma / d theta) x_r       for every celerite coefficient theta of the problem,
 * in gf_loglike_grad's layout and convention: g_real [2][B][max(Jr, 1)] = d/d(a, c), g_comp [4][B][max(Jc, 1)] =
 * d/d(a, b, c, d), g_diag [B] = sum_r w_r |x_r|^2 (the diagonal reaches Sigma through diag_add alone: lag zero is not
 * part of d/da).  What the gradient of log det (A^T Sigma^-1 A) needs, with x_r the columns of Sigma^-1 A F,
 * F F^T = (A^T Sigma^-1 A)^-1, and w = 1/2.  The sums are diagonal linear recurrences along the rows over the generator
 * rows gf_loglike_grad differentiates (cos / sin of fl(d t_n)): no factor, no diagonal, no adjoint sweep.
 *   coefficients, t, t_bs as gf_solve_batch; nobs [B] int64 or NULL: problem b's rows end at nobs[b] (held to 0 .. N),
 *     later rows of t and x are never read
 *   x [B][R][N]: batch stride x_bs (0 = shared by all problems), vector stride x_rs >= N; 1 <= R <= 256
 *   w: NULL (every weight 1), or [R] with w_bs = 0, or [B][R] with w_bs >= R
 *   work: work_bs >= gf_quadform_grad_work(W, R) doubles per problem
 * One wave per problem and block of gf_quadform_grad_block() vectors, then one wave per problem that adds the blocks
 * in order.  No atomics, one summation order per output: a problem's bits do not depend on the batch around it, and
 * vectors of zeros (or of weight zero) behind its own leave them unchanged.  N = 1 gives exact zeros in g_real and
 * g_comp.  Entries of g_real / g_comp of a kind the problem has no term of are not written.
 * Returns -1 for bad shapes, strides or null pointers, -3 for W > 63; gf_quadform_grad_work returns 0 for them.
 */
int gf_quadform_grad_block(void);
int64_t gf_quadform_grad_work(int W, int R);
int gf_quadform_grad(int B, int64_t N, int R, int Jr, int Jc,
                     const double *ar, const double *cr, const double *ac, const double *bc,
                     const double *cc, const double *dc,
                     const double *t, int64_t t_bs, const int64_t *nobs,
                     const double *x, int64_t x_bs, int64_t x_rs, const double *w, int64_t w_bs,
                     double *work, int64_t work_bs,
                     double *g_real, double *g_comp, double *g_diag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GADFLY_HIP_H */
