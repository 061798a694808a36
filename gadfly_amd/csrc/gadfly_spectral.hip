// gadfly_spectral.hip -- spectral log-likelihoods (Whittle, chi-square) of B sums of SHO terms against observed power
// spectra, their analytic gradients and the model spectra
//
// What it evaluates is TermConvolution.get_psd over a TermSum of SHOTerms plus a white floor (gadfly/core.py:33-41,
// celerite2's sinc^2 exposure factor), per problem b with terms j, exposure delta_b and floor c_b:
//     x_j = (w - w0_j)(w + w0_j),  D_j = x_j^2 + w^2 w0_j^2 / Q_j^2,  term_j = sqrt(2/pi) S0_j w0_j^4 / D_j
//     S(w) = sinc^2(delta w / 2) sum_j term_j + c
//     whittle:  l = - sum_k n_k (ln S_k + P_k / S_k)          g_k = dl/dS_k = n_k (P_k / S_k - 1) / S_k
//     chi2:     l = - 1/2 sum_k ((P_k - S_k) / e_k)^2         g_k = (P_k - S_k) / e_k^2
// over the USED frequencies (P_k and n_k / e_k finite, n_k / e_k > 0).  With h_k = g_k sinc^2_k and r = 1 / D_j the
// gradients are three sums per term,
//     p0 = sum_k h r,  p1 = sum_k h r^2 w^2,  p2 = sum_k h r^2 x
//     dl/dS0 = a1 p0                                  a1 = sqrt(2/pi) w0^4,  a = a1 S0
//     dl/dQ  = a (2 w0^2 / Q^3) p1
//     dl/dw0 = a ((4 / w0) p0 + 4 w0 p2 - (2 w0 / Q^2) p1)
// and dl/dc = sum_k g_k.  Four kernels:
//   k_sp_prep    per (b, j) what does not depend on w (a, w0, w0^2/Q^2 and the gradient's factors), IEEE divisions
//   k_sp_tile    (frequency tile, problem): each thread owns SP_K consecutive frequencies.  Pass A loops over the terms
//                (parameters by the uniform j from const __restrict__ arrays: the scalar path) for S, then forms the
//                thread's addends of l, dl/dc, the count of used frequencies and the first failing index; pass B (with
//                gradients only) loops over the terms again, recomputes r and reduces p0, p1, p2 over the workgroup
//                straight away (DPP tree in the wave, LDS across the waves): one partial per (b, tile, j, sum)
//   k_sp_finish  one workgroup per problem adds the tiles' partials in tile order and applies the factors
// Reciprocals: 1 / D_j, the one per (frequency, term) pair, is fast_rcp (hardware estimate + two Newton steps, <= ~1
// ulp; D_j is a positive normal number for any w0 a spectrum in uHz meets); the per-frequency ones (1 / S, 1 / e,
// sin(x) / x) and k_sp_prep's are IEEE divisions.  ln is ocml's, sin is fm_sincos (fastmath.h).
// No floating-point atomics, no contraction left to the compiler (every fma is written): each output of a problem has
// one fixed association, whatever the batch around it, with or without gradients, with or without the model output.

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

constexpr int SP_K = 8;                      // consecutive frequencies per thread (16 measured within 3 % of 8)
constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_TILE = SP_K * SP_THREADS;   // frequencies per workgroup
constexpr int SP_MAX_TERMS = 256;
constexpr int SP_COEF = 8;                   // doubles per (b, j) of k_sp_prep's table
constexpr int SP_SCAL = 4;                   // per (b, tile): l, dl/dc, used, first failing index + 1 (0: none)
constexpr double SQRT_2_OVER_PI = 0.7978845608028654;

__host__ __device__ inline int64_t sp_tiles(int64_t M) { return (M + SP_TILE - 1) / SP_TILE; }
// workspace of one problem: [J][SP_COEF] table, [tiles][SP_SCAL] scalars, [tiles][3][J] gradient sums
__host__ __device__ inline int64_t sp_work(int64_t M, int J) {
    return (int64_t)SP_COEF * J + sp_tiles(M) * (SP_SCAL + 3 * (int64_t)J);
}

// fixed-shape tree sum over the 64 lanes, broadcast (the tree of gf_wave.h's wave_sum)
__device__ __forceinline__ double sp_wave_sum(double v) {
    v += dpp_get<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v += dpp_get<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v += dpp_get<0x141, 0xf>(v);   // row_half_mirror
    v += dpp_get<0x140, 0xf>(v);   // row_mirror
    v += dpp_get<0x142, 0xf>(v);   // row_bcast15
    v += dpp_get<0x143, 0xf>(v);   // row_bcast31: lane 63 holds the sum
    return read_lane(v, 63);
}

__global__ __launch_bounds__(256) void k_sp_prep(int B, int J, int64_t per, const double *__restrict__ S0,
                                                 const double *__restrict__ w0, const double *__restrict__ Q,
                                                 double *__restrict__ work) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * J) return;
    const int64_t b = i / J;
    const int j = (int)(i - b * J);
    const double s = S0[i], w = w0[i], q = Q[i];
    const double w2 = w * w, a1 = SQRT_2_OVER_PI * (w2 * w2), a = a1 * s, q2 = q * q;
    double *c = work + b * per + (int64_t)j * SP_COEF;
    c[0] = a;
    c[1] = w;
    c[2] = w2 / q2;
    c[3] = a1;
    c[4] = a * (2.0 * w2 / (q2 * q));
    c[5] = a * (4.0 / w);
    c[6] = a * (4.0 * w);
    c[7] = a * (2.0 * w / q2);
}

template <bool GRAD>
__global__ __launch_bounds__(SP_THREADS) void k_sp_tile(int64_t M, int J, int objective, int64_t per,
                                                        const double *__restrict__ coef_,
                                                        const double *__restrict__ delta_,
                                                        const double *__restrict__ floor_,
                                                        const double *__restrict__ omega,
                                                        const double *__restrict__ power, int64_t power_bs,
                                                        const double *__restrict__ weight, int64_t weight_bs,
                                                        double *__restrict__ part_, double *__restrict__ model) {
    __shared__ double red[2][SP_WAVES][4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x, tiles = sp_tiles(M);
    const double *__restrict__ coef = coef_ + (int64_t)b * per;
    double *__restrict__ scal = part_ + (int64_t)b * per + (int64_t)SP_COEF * J + tile * SP_SCAL;
    const double delta = delta_[b], c = floor_ ? floor_[b] : 0.0;
    const int64_t k0 = tile * SP_TILE + (int64_t)tid * SP_K;

    double om[SP_K], w2[SP_K], sum[SP_K];
#pragma unroll
    for (int i = 0; i < SP_K; ++i) {
        om[i] = (k0 + i < M) ? omega[k0 + i] : 0.0;
        w2[i] = om[i] * om[i];
        sum[i] = 0.0;
    }
    // pass A: the sum of the terms at the thread's frequencies
    for (int j = 0; j < J; ++j) {
        const double a = coef[j * SP_COEF], w0 = coef[j * SP_COEF + 1], q = coef[j * SP_COEF + 2];
#pragma unroll
        for (int i = 0; i < SP_K; ++i) {
            const double x = (om[i] - w0) * (om[i] + w0);
            const double r = fast_rcp(fma(w2[i], q, x * x));
            sum[i] = fma(a, r, sum[i]);
        }
    }
    double h[SP_K];
    double ll = 0.0, gc = 0.0, used = 0.0, bad = -INFINITY;     // bad: -(first failing index + 1)
#pragma unroll
    for (int i = 0; i < SP_K; ++i) {
        h[i] = 0.0;
        if (k0 + i < M) {
            const double arg = 0.5 * delta * om[i];
            double sn, cs, sinc = 1.0;
            if (arg != 0.0) {
                fm_sincos(arg, &sn, &cs);
                sinc = sn / arg;
            }
            const double sinc2 = sinc * sinc;
            const double S = fma(sinc2, sum[i], c);
            if (model) model[(int64_t)b * M + k0 + i] = S;
            const double P = power[(int64_t)b * power_bs + k0 + i];
            const double wt = weight ? weight[(int64_t)b * weight_bs + k0 + i] : 1.0;
            if (isfinite(P) && isfinite(wt) && wt > 0.0) {
                used += 1.0;
                if (S > 0.0) {
                    double g;
                    if (objective == 0) {
                        const double rs = 1.0 / S, ps = P * rs;
                        ll -= wt * (log(S) + ps);
                        g = wt * ((ps - 1.0) * rs);
                    } else {
                        const double re = 1.0 / wt, z = (P - S) * re;
                        ll -= 0.5 * (z * z);
                        g = z * re;
                    }
                    gc += g;
                    h[i] = g * sinc2;
                } else {
                    bad = fmax(bad, -(double)(k0 + i + 1));
                }
            }
        }
    }
    ll = sp_wave_sum(ll);
    gc = sp_wave_sum(gc);
    used = sp_wave_sum(used);
    bad = wave_max(bad);
    if (lane == 0) {
        red[0][wave][0] = ll;
        red[0][wave][1] = gc;
        red[0][wave][2] = used;
        red[0][wave][3] = bad;
    }
    __syncthreads();
    if (tid < 3) {
        double v = red[0][0][tid];
        for (int w = 1; w < SP_WAVES; ++w) v += red[0][w][tid];
        scal[tid] = v;
    } else if (tid == 3) {
        double v = red[0][0][3];
        for (int w = 1; w < SP_WAVES; ++w) v = fmax(v, red[0][w][3]);
        scal[3] = (v == -INFINITY) ? 0.0 : -v;
    }
    if (!GRAD) return;
    // pass B: per term the three sums over the tile's frequencies (the first use of red[1] follows the barrier above,
    // and a buffer is written again only after the barrier that follows its readers' loads in program order)
    double *__restrict__ gp = part_ + (int64_t)b * per + (int64_t)SP_COEF * J + tiles * SP_SCAL + tile * 3 * (int64_t)J;
    for (int j = 0; j < J; ++j) {
        const double w0 = coef[j * SP_COEF + 1], q = coef[j * SP_COEF + 2];
        double p0 = 0.0, p1 = 0.0, p2 = 0.0;
#pragma unroll
        for (int i = 0; i < SP_K; ++i) {
            const double x = (om[i] - w0) * (om[i] + w0);
            const double r = fast_rcp(fma(w2[i], q, x * x));
            const double hr = h[i] * r;
            p0 += hr;
            const double hr2 = hr * r;
            p1 = fma(hr2, w2[i], p1);
            p2 = fma(hr2, x, p2);
        }
        p0 = sp_wave_sum(p0);
        p1 = sp_wave_sum(p1);
        p2 = sp_wave_sum(p2);
        const int buf = (j + 1) & 1;
        if (lane == 0) {
            red[buf][wave][0] = p0;
            red[buf][wave][1] = p1;
            red[buf][wave][2] = p2;
        }
        __syncthreads();
        if (tid < 3) {
            double v = red[buf][0][tid];
            for (int w = 1; w < SP_WAVES; ++w) v += red[buf][w][tid];
            gp[(int64_t)tid * J + j] = v;
        }
    }
}

__global__ __launch_bounds__(64) void k_sp_finish(int64_t M, int J, int64_t per, int grad,
                                                  const double *__restrict__ work, double *__restrict__ ll,
                                                  int64_t *__restrict__ used, int32_t *__restrict__ info,
                                                  double *__restrict__ gS0, double *__restrict__ gw0,
                                                  double *__restrict__ gQ, double *__restrict__ gfloor) {
    const int b = blockIdx.x;
    const int64_t tiles = sp_tiles(M);
    const double *__restrict__ coef = work + (int64_t)b * per;
    const double *__restrict__ scal = coef + (int64_t)SP_COEF * J;
    const double *__restrict__ gp = scal + tiles * SP_SCAL;
    double first = 0.0;                         // the first failing index + 1 (the tiles are in frequency order)
    for (int64_t t = 0; t < tiles; ++t) {
        const double v = scal[t * SP_SCAL + 3];
        if (first == 0.0 && v != 0.0) first = v;
    }
    const bool fail = first != 0.0;
    const double nan = __builtin_nan("");
    if (threadIdx.x == 0) {
        double l = 0.0, g = 0.0, n = 0.0;
        for (int64_t t = 0; t < tiles; ++t) {
            l += scal[t * SP_SCAL];
            g += scal[t * SP_SCAL + 1];
            n += scal[t * SP_SCAL + 2];
        }
        ll[b] = fail ? -INFINITY : l;
        used[b] = (int64_t)n;
        info[b] = fail ? (int32_t)(first > 2147483647.0 ? 2147483647.0 : first) : 0;
        if (gfloor) gfloor[b] = fail ? nan : g;
    }
    if (!grad) return;
    for (int j = threadIdx.x; j < J; j += 64) {
        double p0 = 0.0, p1 = 0.0, p2 = 0.0;
        for (int64_t t = 0; t < tiles; ++t) {
            const double *p = gp + t * 3 * (int64_t)J + j;
            p0 += p[0];
            p1 += p[J];
            p2 += p[2 * (int64_t)J];
        }
        const double *cf = coef + (int64_t)j * SP_COEF;
        const int64_t o = (int64_t)b * J + j;
        if (gS0) gS0[o] = fail ? nan : cf[3] * p0;
        if (gQ) gQ[o] = fail ? nan : cf[4] * p1;
        if (gw0) gw0[o] = fail ? nan : fma(cf[5], p0, fma(cf[6], p2, -(cf[7] * p1)));
    }
}

}  // namespace

extern "C" {

int gf_spectral_tile(void) { return SP_TILE; }

int64_t gf_spectral_work(int B, int64_t M, int J) {
    if (B < 1 || M < 1 || J < 1 || J > SP_MAX_TERMS) return 0;
    return (int64_t)B * sp_work(M, J);
}

int gf_spectral_like(int B, int64_t M, int J, int objective, const double *S0, const double *w0, const double *Q,
                     const double *delta, const double *floor, const double *omega, const double *power,
                     int64_t power_bs, const double *weight, int64_t weight_bs, double *work, double *ll,
                     int64_t *used, int32_t *info, double *gS0, double *gw0, double *gQ, double *gfloor,
                     double *model, void *stream) {
    if (B < 1 || M < 1 || J < 1)
        return gf_internal_error(-1, "gf_spectral_like: bad shape (B=%d, M=%lld, J=%d)", B, (long long)M, J);
    if (J > SP_MAX_TERMS)
        return gf_internal_error(-3, "gf_spectral_like: J=%d terms, at most %d", J, SP_MAX_TERMS);
    if (B > 65535) return gf_internal_error(-1, "gf_spectral_like: more than 65535 problems in one call (B=%d)", B);
    if (sp_tiles(M) > 2147483647LL)
        return gf_internal_error(-1, "gf_spectral_like: M=%lld frequencies are too many tiles", (long long)M);
    if (objective != 0 && objective != 1)
        return gf_internal_error(-1, "gf_spectral_like: objective %d (0 whittle, 1 chi2)", objective);
    if (objective == 1 && !weight)
        return gf_internal_error(-1, "gf_spectral_like: chi2 needs the errors (weight is NULL)");
    if (power_bs < 0 || weight_bs < 0)
        return gf_internal_error(-1, "gf_spectral_like: negative batch stride");
    if (!S0 || !w0 || !Q || !delta || !omega || !power || !work || !ll || !used || !info)
        return gf_internal_error(-1, "gf_spectral_like: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int grad = (gS0 || gw0 || gQ || gfloor) ? 1 : 0;
    const int64_t per = sp_work(M, J);
    const int64_t terms = (int64_t)B * J;
    hipLaunchKernelGGL(k_sp_prep, dim3((unsigned)((terms + 255) / 256)), dim3(256), 0, st, B, J, per, S0, w0, Q, work);
    const dim3 grid((unsigned)sp_tiles(M), (unsigned)B);
    if (grad)
        hipLaunchKernelGGL(k_sp_tile<true>, grid, dim3(SP_THREADS), 0, st, M, J, objective, per, (const double *)work,
                           delta, floor, omega, power, power_bs, weight, weight_bs, work, model);
    else
        hipLaunchKernelGGL(k_sp_tile<false>, grid, dim3(SP_THREADS), 0, st, M, J, objective, per, (const double *)work,
                           delta, floor, omega, power, power_bs, weight, weight_bs, work, model);
    hipLaunchKernelGGL(k_sp_finish, dim3((unsigned)B), dim3(64), 0, st, M, J, per, grad, (const double *)work, ll,
                       used, info, gS0, gw0, gQ, gfloor);
    return gf_internal_check_launch("gf_spectral_like");
}

}  // extern "C"
