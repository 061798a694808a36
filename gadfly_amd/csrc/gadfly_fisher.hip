// gadfly_fisher.hip -- Fisher information of the spectral objectives (Whittle, chi-square) of B sums of SHO terms
// (DESIGN.md 3.14): per problem the weighted Gram matrix of the model spectrum's Jacobian over the used frequencies,
//     F = sum_k v_k grad S(w_k) grad S(w_k)^T,     v_k = n_k / S_k^2 (whittle),  v_k = 1 / e_k^2 (chi2)
// in the parameter order S0_0 .. S0_{J-1}, w0_0 .., Q_0 .., floor (P = 3 J + 1).  With the notation of
// gadfly_spectral.hip (x = (w - w0)(w + w0), D = x^2 + w^2 w0^2 / Q^2, r = 1 / D, a1 = sqrt(2/pi) w0^4, a = a1 S0):
//     dS/dS0 = sinc^2 a1 r
//     dS/dw0 = sinc^2 a ((4 / w0) r + 4 w0 r^2 x - (2 w0 / Q^2) r^2 w^2)
//     dS/dQ  = sinc^2 a (2 w0^2 / Q^3) r^2 w^2
//     dS/dc  = 1
// Four kernels:
//   k_fi_prep    per (b, j) the eight numbers of k_sp_prep (restated; rows of padding terms beyond J are zero)
//   k_fi_weight  (slab, problem): S over all J terms with the arithmetic of k_sp_tile's pass A (the same bits, so the
//                same `info`), then v_k (0 where the frequency is not used) and sinc^2_k into the workspace, and per
//                slab the count of used frequencies and the first failing index
//   k_fi_gram    (slab, block, problem), one wave each: the rank updates on v_mfma_f64_16x16x4.  Terms are cut into
//                tiles of 16; a block is a pair (tp <= tq) of term tiles.  Lane (i, k) = (lane & 15, lane >> 4) has term
//                16 tp + i and term 16 tq + i for the whole slab (their constants stay in registers) and walks the
//                slab four frequencies at a time at frequency 4 s + k: one reciprocal per term gives the lane's entry
//                of three operand tiles (S0, w0, Q).  The A operand of a tile is v_k times the entry, the B operand the
//                entry itself -- the same per-lane values, no LDS staging -- and the block's 3 x 3 tile products
//                (6 for tp = tq: the kinds a <= b) accumulate in registers.  The floor's row (sum v dS, sum v) is kept
//                per lane in the diagonal blocks.  One partial per (b, slab, block)
//   k_fi_status  per problem: used, info and whether the problem failed
//   k_fi_finish  per output entry: the partials of its tile added in slab order.  Entries (R, C) and (C, R) read the
//                same accumulator -- block (tp <= tq), inside tp = tq the kinds (a <= b), inside a diagonal tile the
//                lower triangle -- so the matrix is exactly symmetric; a diagonal entry is a sum of (v d) d >= 0
// No floating-point atomics, no contraction left to the compiler (every fma is written): a problem's matrix has one
// fixed association, whatever the batch around it.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/gadfly_hip.h"
#include "gf_internal.h"
#include "gf_wave.h"

#define FM_INLINE static __device__ __forceinline__
#include "fastmath.h"

#pragma clang fp contract(off)

namespace {

constexpr int FI_K = 4;                      // consecutive frequencies per thread of k_fi_weight
constexpr int FI_THREADS = 256;
constexpr int FI_WAVES = FI_THREADS / 64;
constexpr int FI_SLAB = FI_K * FI_THREADS;   // frequencies summed into one partial (and per workgroup of k_fi_weight)
constexpr int FI_MAX_TERMS = 256;
constexpr int FI_COEF = 8;                   // doubles per (b, j) of the table
constexpr int FI_SCAL = 2;                   // per (b, slab): used, first failing index + 1 (0: none)
constexpr int FI_HEAD = 2;                   // per problem: failed (0 / 1), padding
constexpr int FI_SLOTS = 10;                 // per (b, slab, block): 9 tiles of 256 and the floor's 4 x 64 lane sums
constexpr double SQRT_2_OVER_PI = 0.7978845608028654;

#define FI_MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
typedef double fi_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int64_t fi_slabs(int64_t M) { return (M + FI_SLAB - 1) / FI_SLAB; }
__host__ __device__ inline int fi_term_tiles(int J) { return (J + 15) / 16; }
__host__ __device__ inline int fi_blocks(int J) { return fi_term_tiles(J) * (fi_term_tiles(J) + 1) / 2; }
// workspace of one problem: head, [16 TJ][FI_COEF] table, v [M], sinc^2 [M], [slabs][FI_SCAL], [slabs][blocks][10][256]
__host__ __device__ inline int64_t fi_off_coef() { return FI_HEAD; }
__host__ __device__ inline int64_t fi_off_v(int J) { return fi_off_coef() + (int64_t)FI_COEF * 16 * fi_term_tiles(J); }
__host__ __device__ inline int64_t fi_off_scal(int64_t M, int J) { return fi_off_v(J) + 2 * M; }
__host__ __device__ inline int64_t fi_off_part(int64_t M, int J) { return fi_off_scal(M, J) + fi_slabs(M) * FI_SCAL; }
__host__ __device__ inline int64_t fi_work(int64_t M, int J) {
    return fi_off_part(M, J) + fi_slabs(M) * fi_blocks(J) * (int64_t)(FI_SLOTS * 256);
}

// fixed-shape tree sum over the 64 lanes, broadcast (the tree of gadfly_spectral.hip's sp_wave_sum)
__device__ __forceinline__ double fi_wave_sum(double v) {
    v += dpp_get<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v += dpp_get<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v += dpp_get<0x141, 0xf>(v);   // row_half_mirror
    v += dpp_get<0x140, 0xf>(v);   // row_mirror
    v += dpp_get<0x142, 0xf>(v);   // row_bcast15
    v += dpp_get<0x143, 0xf>(v);   // row_bcast31: lane 63 holds the sum
    return read_lane(v, 63);
}

__global__ __launch_bounds__(256) void k_fi_prep(int B, int J, int64_t per, const double *__restrict__ S0,
                                                 const double *__restrict__ w0, const double *__restrict__ Q,
                                                 double *__restrict__ work) {
    const int JP = 16 * fi_term_tiles(J);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * JP) return;
    const int64_t b = i / JP;
    const int j = (int)(i - b * JP);
    double *c = work + b * per + fi_off_coef() + (int64_t)j * FI_COEF;
    if (j >= J) {                               // a padding term: every entry it supplies is an exact zero
        c[0] = 0.0; c[1] = 1.0; c[2] = 1.0; c[3] = 0.0; c[4] = 0.0; c[5] = 0.0; c[6] = 0.0; c[7] = 0.0;
        return;
    }
    const double s = S0[b * J + j], w = w0[b * J + j], q = Q[b * J + j];
    const double w2 = w * w, a1 = SQRT_2_OVER_PI * (w2 * w2), a = a1 * s, q2 = q * q;
    c[0] = a;
    c[1] = w;
    c[2] = w2 / q2;
    c[3] = a1;
    c[4] = a * (2.0 * w2 / (q2 * q));
    c[5] = a * (4.0 / w);
    c[6] = a * (4.0 * w);
    c[7] = a * (2.0 * w / q2);
}

__global__ __launch_bounds__(FI_THREADS) void k_fi_weight(int64_t M, int J, int objective, int64_t per,
                                                          const double *__restrict__ coef_,
                                                          const double *__restrict__ delta_,
                                                          const double *__restrict__ floor_,
                                                          const double *__restrict__ omega,
                                                          const double *__restrict__ power, int64_t power_bs,
                                                          const double *__restrict__ weight, int64_t weight_bs,
                                                          double *__restrict__ work) {
    __shared__ double red[FI_WAVES][2];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t slab = blockIdx.x;
    const double *__restrict__ coef = coef_ + (int64_t)b * per + fi_off_coef();
    double *__restrict__ vout = work + (int64_t)b * per + fi_off_v(J);
    double *__restrict__ sout = vout + M;
    double *__restrict__ scal = work + (int64_t)b * per + fi_off_scal(M, J) + slab * FI_SCAL;
    const double delta = delta_[b], c = floor_ ? floor_[b] : 0.0;
    const int64_t k0 = slab * FI_SLAB + (int64_t)tid * FI_K;

    double om[FI_K], w2[FI_K], sum[FI_K];
#pragma unroll
    for (int i = 0; i < FI_K; ++i) {
        om[i] = (k0 + i < M) ? omega[k0 + i] : 0.0;
        w2[i] = om[i] * om[i];
        sum[i] = 0.0;
    }
    // the sum of the terms at the thread's frequencies: k_sp_tile's pass A, operation for operation
    for (int j = 0; j < J; ++j) {
        const double a = coef[j * FI_COEF], w0 = coef[j * FI_COEF + 1], q = coef[j * FI_COEF + 2];
#pragma unroll
        for (int i = 0; i < FI_K; ++i) {
            const double x = (om[i] - w0) * (om[i] + w0);
            const double r = fast_rcp(fma(w2[i], q, x * x));
            sum[i] = fma(a, r, sum[i]);
        }
    }
    double used = 0.0, bad = -INFINITY;         // bad: -(first failing index + 1)
#pragma unroll
    for (int i = 0; i < FI_K; ++i) {
        if (k0 + i < M) {
            const double arg = 0.5 * delta * om[i];
            double sn, cs, sinc = 1.0;
            if (arg != 0.0) {
                fm_sincos(arg, &sn, &cs);
                sinc = sn / arg;
            }
            const double sinc2 = sinc * sinc;
            const double S = fma(sinc2, sum[i], c);
            const double P = power[(int64_t)b * power_bs + k0 + i];
            const double wt = weight ? weight[(int64_t)b * weight_bs + k0 + i] : 1.0;
            double v = 0.0;
            if (isfinite(P) && isfinite(wt) && wt > 0.0) {
                used += 1.0;
                if (S > 0.0) {
                    if (objective == 0) {
                        const double rs = 1.0 / S;
                        v = wt * (rs * rs);
                    } else {
                        const double re = 1.0 / wt;
                        v = re * re;
                    }
                } else {
                    bad = fmax(bad, -(double)(k0 + i + 1));
                }
            }
            vout[k0 + i] = v;
            sout[k0 + i] = sinc2;
        }
    }
    used = fi_wave_sum(used);
    bad = wave_max(bad);
    if (lane == 0) {
        red[wave][0] = used;
        red[wave][1] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        double v = red[0][0];
        for (int w = 1; w < FI_WAVES; ++w) v += red[w][0];
        scal[0] = v;
    } else if (tid == 1) {
        double v = red[0][1];
        for (int w = 1; w < FI_WAVES; ++w) v = fmax(v, red[w][1]);
        scal[1] = (v == -INFINITY) ? 0.0 : -v;
    }
}

// what a lane keeps of its term for a slab, and its entries of the S0, w0 and Q operand tiles at one frequency
struct FiTerm {
    double w0, q, a1, c4, c5, c6, c7;
    __device__ __forceinline__ void load(const double *__restrict__ c) {
        w0 = c[1]; q = c[2]; a1 = c[3]; c4 = c[4]; c5 = c[5]; c6 = c[6]; c7 = c[7];
    }
    __device__ __forceinline__ void entries(double om, double w2, double s2, double &dS, double &dw, double &dQ) const {
        const double x = (om - w0) * (om + w0);
        const double r = fast_rcp(fma(w2, q, x * x));
        const double sr = s2 * r;
        const double sr2 = sr * r;
        const double t1 = sr2 * w2, t2 = sr2 * x;
        dS = a1 * sr;
        dQ = c4 * t1;
        dw = fma(c5, sr, fma(c6, t2, -(c7 * t1)));
    }
};

template <bool DIAG>
__device__ __forceinline__ void fi_gram_block(int64_t M, int64_t k0, int lane, const double *__restrict__ cp,
                                              const double *__restrict__ cq, const double *__restrict__ omega,
                                              const double *__restrict__ vin, const double *__restrict__ sin2,
                                              double *__restrict__ part) {
    FiTerm tp, tq;
    tp.load(cp + (lane & 15) * FI_COEF);
    if (!DIAG) tq.load(cq + (lane & 15) * FI_COEF);
    fi_d4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[a][c] = fi_d4{0.0, 0.0, 0.0, 0.0};
    double fl[3] = {0.0, 0.0, 0.0}, fv = 0.0;
    const int64_t kend = (k0 + FI_SLAB < M) ? k0 + FI_SLAB : M;
    // (a step's omega, v and sinc^2 are fetched one step ahead: its loads fly under the previous step's MFMAs)
    int64_t kn = k0 + (lane >> 4);
    double om_n = kn < M ? omega[kn] : 0.0, v_n = kn < M ? vin[kn] : 0.0, s2_n = kn < M ? sin2[kn] : 0.0;
    for (int64_t ks = k0; ks < kend; ks += 4) {
        const double om = om_n, v = v_n, s2 = s2_n;
        kn += 4;
        const bool in = kn < kend;
        om_n = in ? omega[kn] : 0.0;
        v_n = in ? vin[kn] : 0.0;
        s2_n = in ? sin2[kn] : 0.0;
        const double w2 = om * om;
        double p[3], q[3], pa[3];
        tp.entries(om, w2, s2, p[0], p[1], p[2]);
        if (DIAG) {
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
        } else {
            tq.entries(om, w2, s2, q[0], q[1], q[2]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) pa[a] = v * p[a];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = DIAG ? a : 0; c < 3; ++c) acc[a][c] = FI_MFMA64(pa[a], q[c], acc[a][c]);
        if (DIAG) {
#pragma unroll
            for (int a = 0; a < 3; ++a) fl[a] += pa[a];
            fv += v;
        }
    }
    // the accumulators as they lie: element (row, col) of a tile is register row >> 2 of lane col + 16 (row & 3)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = DIAG ? a : 0; c < 3; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) part[(a * 3 + c) * 256 + g * 64 + lane] = acc[a][c][g];
    if (DIAG) {
#pragma unroll
        for (int a = 0; a < 3; ++a) part[9 * 256 + a * 64 + lane] = fl[a];
        part[9 * 256 + 3 * 64 + lane] = fv;
    }
}

__global__ __launch_bounds__(64) void k_fi_gram(int64_t M, int J, int64_t per, const double *__restrict__ omega,
                                                double *__restrict__ work) {
    const int b = blockIdx.z, blk = blockIdx.y, lane = threadIdx.x;
    const int64_t slab = blockIdx.x;
    int tq = 0;
    while ((tq + 1) * (tq + 2) / 2 <= blk) ++tq;
    const int tp = blk - tq * (tq + 1) / 2;         // tp <= tq
    double *__restrict__ wb = work + (int64_t)b * per;
    const double *__restrict__ coef = wb + fi_off_coef();
    const double *__restrict__ vin = wb + fi_off_v(J);
    double *__restrict__ part = wb + fi_off_part(M, J) + (slab * fi_blocks(J) + blk) * (int64_t)(FI_SLOTS * 256);
    const double *cp = coef + (int64_t)tp * 16 * FI_COEF, *cq = coef + (int64_t)tq * 16 * FI_COEF;
    if (tp == tq)
        fi_gram_block<true>(M, slab * FI_SLAB, lane, cp, cq, omega, vin, vin + M, part);
    else
        fi_gram_block<false>(M, slab * FI_SLAB, lane, cp, cq, omega, vin, vin + M, part);
}

__global__ __launch_bounds__(64) void k_fi_status(int B, int64_t M, int J, int64_t per, double *__restrict__ work,
                                                  int64_t *__restrict__ used, int32_t *__restrict__ info) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int64_t slabs = fi_slabs(M);
    const double *__restrict__ scal = work + (int64_t)b * per + fi_off_scal(M, J);
    double first = 0.0, n = 0.0;                    // the first failing index + 1 (the slabs are in frequency order)
    for (int64_t t = 0; t < slabs; ++t) {
        const double v = scal[t * FI_SCAL + 1];
        if (first == 0.0 && v != 0.0) first = v;
        n += scal[t * FI_SCAL];
    }
    const bool fail = first != 0.0;
    used[b] = (int64_t)n;
    info[b] = fail ? (int32_t)(first > 2147483647.0 ? 2147483647.0 : first) : 0;
    work[(int64_t)b * per] = fail ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void k_fi_finish(int64_t M, int J, int64_t per, const double *__restrict__ work,
                                                   double *__restrict__ fisher) {
    const int b = blockIdx.y;
    const int P = 3 * J + 1;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)P * P) return;
    int R = (int)(e / P), C = (int)(e - (int64_t)R * P);
    const double *__restrict__ wb = work + (int64_t)b * per;
    double *out = fisher + (int64_t)b * P * P + e;
    if (wb[0] != 0.0) {
        *out = __builtin_nan("");
        return;
    }
    const int64_t slabs = fi_slabs(M), nblk = fi_blocks(J);
    const int64_t stride = nblk * (int64_t)(FI_SLOTS * 256);
    const double *__restrict__ part = wb + fi_off_part(M, J);
    if (R < C) { const int t = R; R = C; C = t; }   // R >= C: the floor, if any, is R
    double sum = 0.0;
    if (R == P - 1) {
        // the floor's row: the four frequency groups of a lane sum in group order, slab after slab
        int64_t off;
        if (C == P - 1) {
            off = 9 * 256 + 3 * 64;                 // sum v: the first diagonal block's, any one term lane
        } else {
            const int a = C / J, j = C - a * J, t = j >> 4;
            off = ((int64_t)t * (t + 1) / 2 + t) * (FI_SLOTS * 256) + 9 * 256 + a * 64 + (j & 15);
        }
        for (int64_t s = 0; s < slabs; ++s) {
            const double *p = part + s * stride + off;
            sum += ((p[0] + p[16]) + p[32]) + p[48];
        }
        *out = sum;
        return;
    }
    int a = R / J, j = R - a * J, ta = j >> 4, ia = j & 15;
    int c = C / J, l = C - c * J, tc = l >> 4, ic = l & 15;
    // one accumulator for (R, C) and (C, R): block (tp <= tq), inside tp = tq kinds (a <= c), inside a = c the lower
    // triangle
    bool swap = ta > tc || (ta == tc && (a > c || (a == c && ia < ic)));
    if (swap) {
        int t;
        t = a; a = c; c = t;
        t = ta; ta = tc; tc = t;
        t = ia; ia = ic; ic = t;
    }
    const int64_t off = ((int64_t)tc * (tc + 1) / 2 + ta) * (FI_SLOTS * 256) + (a * 3 + c) * 256 + (ia >> 2) * 64 +
                        ic + 16 * (ia & 3);
    for (int64_t s = 0; s < slabs; ++s) sum += part[s * stride + off];
    *out = sum;
}

}  // namespace

extern "C" {

int gf_spectral_fisher_slab(void) { return FI_SLAB; }

int64_t gf_spectral_fisher_work(int B, int64_t M, int J) {
    if (B < 1 || M < 1 || J < 1 || J > FI_MAX_TERMS) return 0;
    return (int64_t)B * fi_work(M, J);
}

int gf_spectral_fisher(int B, int64_t M, int J, int objective, const double *S0, const double *w0, const double *Q,
                       const double *delta, const double *floor, const double *omega, const double *power,
                       int64_t power_bs, const double *weight, int64_t weight_bs, double *work, double *fisher,
                       int64_t *used, int32_t *info, void *stream) {
    if (B < 1 || M < 1 || J < 1)
        return gf_internal_error(-1, "gf_spectral_fisher: bad shape (B=%d, M=%lld, J=%d)", B, (long long)M, J);
    if (J > FI_MAX_TERMS)
        return gf_internal_error(-3, "gf_spectral_fisher: J=%d terms, at most %d", J, FI_MAX_TERMS);
    if (B > 65535) return gf_internal_error(-1, "gf_spectral_fisher: more than 65535 problems in one call (B=%d)", B);
    if (fi_slabs(M) > 2147483647LL)
        return gf_internal_error(-1, "gf_spectral_fisher: M=%lld frequencies are too many slabs", (long long)M);
    if (objective != 0 && objective != 1)
        return gf_internal_error(-1, "gf_spectral_fisher: objective %d (0 whittle, 1 chi2)", objective);
    if (objective == 1 && !weight)
        return gf_internal_error(-1, "gf_spectral_fisher: chi2 needs the errors (weight is NULL)");
    if (power_bs < 0 || weight_bs < 0)
        return gf_internal_error(-1, "gf_spectral_fisher: negative batch stride");
    if (!S0 || !w0 || !Q || !delta || !omega || !power || !work || !fisher || !used || !info)
        return gf_internal_error(-1, "gf_spectral_fisher: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t per = fi_work(M, J);
    const int64_t terms = (int64_t)B * 16 * fi_term_tiles(J);
    const int64_t P = 3 * (int64_t)J + 1;
    hipLaunchKernelGGL(k_fi_prep, dim3((unsigned)((terms + 255) / 256)), dim3(256), 0, st, B, J, per, S0, w0, Q, work);
    hipLaunchKernelGGL(k_fi_weight, dim3((unsigned)fi_slabs(M), (unsigned)B), dim3(FI_THREADS), 0, st, M, J, objective,
                       per, (const double *)work, delta, floor, omega, power, power_bs, weight, weight_bs, work);
    hipLaunchKernelGGL(k_fi_gram, dim3((unsigned)fi_slabs(M), (unsigned)fi_blocks(J), (unsigned)B), dim3(64), 0, st, M,
                       J, per, omega, work);
    hipLaunchKernelGGL(k_fi_status, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, M, J, per, work, used,
                       info);
    hipLaunchKernelGGL(k_fi_finish, dim3((unsigned)((P * P + 255) / 256), (unsigned)B), dim3(256), 0, st, M, J, per,
                       (const double *)work, fisher);
    return gf_internal_check_launch("gf_spectral_fisher");
}

}  // extern "C"
