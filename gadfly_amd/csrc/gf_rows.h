// The plain celerite recurrence, one wave per problem, lane j owning column j (W <= 63): what gadfly_solve.hip,
// gadfly_var.hip and gadfly_predict.hip share, and the geometry gadfly_grad.hip shares with them.
// Internal linkage: every translation unit gets its own inlined copies.  Nothing here is set at file scope, so a unit
// that includes this header keeps the contraction it had, wherever the include stands.  gen_row, fwd_row and
// stage_alpha switch contraction off in their own bodies (their operations are fused explicitly, and gf_var_batch's
// alpha, mu, log L and info have gf_solve_batch's bits because both run this one copy).  wsum does not: it holds no
// product, and a product handed to it fuses with its first addition only where the caller's own setting lets that
// product contract (gadfly_grad.hip's does, the other units' never).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace {

constexpr int ROW_LANES = 64;
constexpr int ROW_MAX_W = 63;

__host__ __device__ inline int row_wm(int W) { return W <= 16 ? 16 : W <= 32 ? 32 : 64; }

inline bool row_shape_ok(int64_t N, int W) { return N >= 1 && W >= 1 && W <= ROW_MAX_W; }

// doubles per checkpoint (S rows, G, W, D, z; a lane's row of S contiguous) and per staged row (W, U, P)
__host__ __device__ inline int64_t solve_ck(int WM) { return (int64_t)(WM + 4) * ROW_LANES; }
__host__ __device__ inline int64_t solve_rs() { return (int64_t)3 * ROW_LANES; }
__host__ __device__ inline int64_t solve_n64(int64_t N) { return (N + 63) / 64 * 64; }

// every 8 columns of a row's broadcast loop: keeps the scheduler from hoisting all of its LDS reads ahead of their FMAs
#define ROW_PACE(k) do { if (((k) & 7) == 7) __builtin_amdgcn_sched_barrier(0); } while (0)

__device__ __forceinline__ double wsum(double x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m, ROW_LANES);
    return x;        // (a + b == b + a: every lane ends with the same bits)
}

// one state column of the celerite form: a real term (U = a, V = 1) or one half of a complex term
struct Col {
    double a, b, c, d;
    int kind;        // 0 inactive lane, 1 real, 2 complex
    int half;        // complex: 0 = cosine column, 1 = sine column
};

__device__ __forceinline__ Col load_col(int b, int lane, int Jr, int Jc, const double *ar, const double *cr,
                                        const double *ac, const double *bc, const double *cc, const double *dc) {
    const int lr = Jr > 0 ? Jr : 1, lc = Jc > 0 ? Jc : 1;
    Col q{0.0, 0.0, 0.0, 0.0, 0, 0};
    if (lane < Jr) {
        q.kind = 1; q.a = ar[(int64_t)b * lr + lane]; q.c = cr[(int64_t)b * lr + lane];
    } else if (lane < Jr + 2 * Jc) {
        const int64_t o = (int64_t)b * lc + ((lane - Jr) >> 1);
        q.kind = 2; q.half = (lane - Jr) & 1;
        q.a = ac[o]; q.b = bc[o]; q.c = cc[o]; q.d = dc[o];
    }
    return q;
}

// a per-problem count (rows observed, queries asked) held to [0, full]; no array: full
__device__ __forceinline__ int64_t clamp_count(const int64_t *cnt, int b, int64_t full) {
    if (!cnt) return full;
    const int64_t v = cnt[b];
    return v < 0 ? 0 : v > full ? full : v;
}

__device__ __forceinline__ void gen_row(const Col &q, double tn, double &u, double &v) {
#pragma clang fp contract(off)
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

// one forward row: (S, G, w, D, z) of row n-1 in, of row n out; u, p of row n out
template <int WM>
__device__ __forceinline__ void fwd_row(double (&S)[WM], double &G, double &w, double &D, double &z,
                                        const Col &q, double tprev, double tn, double An, double yn,
                                        double *sh, int lane, double &u, double &p) {
#pragma clang fp contract(off)
    double v;
    gen_row(q, tn, u, v);
    p = exp(q.c * (tprev - tn));
    const double wi = D * w;
    sh[lane] = w;
    sh[ROW_LANES + lane] = p;
    sh[2 * ROW_LANES + lane] = u;
    __syncthreads();
    double f = 0.0;
#pragma unroll
    for (int k = 0; k < WM; ++k) {
        const double s = (p * sh[ROW_LANES + k]) * fma(wi, sh[k], S[k]);
        S[k] = s;
        f = fma(s, sh[2 * ROW_LANES + k], f);
        ROW_PACE(k);
    }
    G = p * fma(w, z, G);
    const double uf = wsum(u * f), ug = wsum(u * G);
    D = An - uf;
    z = yn - ug;
    w = (v - f) / D;
}

// ---- what k_solve and k_var share of the checkpoint protocol.  (The checkpoint load, the 64-row staging of z and D
// and the recompute loop read the same in both kernels but stay inline there: as functions they left the compiler
// other address arithmetic and branches, in kernels that sit at the edge of their register budget.)

// the state entering a segment's first row, to the segment's checkpoint c
template <int WM>
__device__ __forceinline__ void ck_store(double *c, int lane, const double (&S)[WM], double G, double w, double D,
                                         double z) {
#pragma unroll
    for (int k = 0; k < WM; ++k) c[lane * WM + k] = S[k];
    c[(WM + 0) * ROW_LANES + lane] = G;
    c[(WM + 1) * ROW_LANES + lane] = w;
    c[(WM + 2) * ROW_LANES + lane] = D;
    c[(WM + 3) * ROW_LANES + lane] = z;
}

// pass 2, at the first row of a 64-row run: alpha of row i over its z, and the outputs that follow from it alone
__device__ __forceinline__ void stage_alpha(int64_t i, double a, double *zw, double *alpha, double *mu,
                                            const double *dg, const double *y) {
#pragma clang fp contract(off)
    zw[i] = a;
    if (alpha) alpha[i] = a;
    if (mu) mu[i] = dg ? y[i] - dg[i] * a : y[i];
}

}  // namespace
