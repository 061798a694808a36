// Wave-level primitives (64 lanes, DPP / readlane: no LDS traffic) shared by the library's translation units.
// Internal linkage: every translation unit gets its own inlined copies.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include <type_traits>

namespace {

// one v_mfma_f64_16x16x4 and its accumulator: four doubles per lane (the steady tail, the chunk combines' block
// algebra, the linear sweeps, the dense scan)
#define GF_MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
typedef double d4 __attribute__((ext_vector_type(4)));

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_get(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, true);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double read_lane(double v, int l) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// max over the 64 lanes (same DPP tree), broadcast
__device__ __forceinline__ double wave_max(double v) {
    v = fmax(v, dpp_get<0xB1, 0xf>(v));
    v = fmax(v, dpp_get<0x4E, 0xf>(v));
    v = fmax(v, dpp_get<0x141, 0xf>(v));
    v = fmax(v, dpp_get<0x140, 0xf>(v));
    double r1 = read_lane(v, 15), r2 = read_lane(v, 31), r3 = read_lane(v, 47), r4 = read_lane(v, 63);
    return fmax(fmax(r1, r2), fmax(r3, r4));
}

// 1/x for normal positive x: hardware estimate + two Newton steps (error <= ~1 ulp); the
// IEEE division sequence costs ~14 VALU instructions on a path every row waits for.
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// max of a 32-bit key over the 64 lanes, broadcast (DPP inside the rows of 16 lanes, scalar across them)
__device__ __forceinline__ int wave_max_key(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true));     // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true));     // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true));    // row_half_mirror
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true));    // row_mirror
    const int r1 = __builtin_amdgcn_readlane(v, 15), r2 = __builtin_amdgcn_readlane(v, 31),
              r3 = __builtin_amdgcn_readlane(v, 47), r4 = __builtin_amdgcn_readlane(v, 63);
    return max(max(r1, r2), max(r3, r4));
}

// Gauss(-Jordan) elimination with lanes = rows (gadfly_hip.hip, cb_gauss_jordan): the owner's part of one step: pivot row among the lanes with !used for the column entries cval;
// multipliers into fb[lane], pivot lane and 1 / pivot into pvb / pinvb
__device__ __forceinline__ void gj_search(const double cval, const bool used, const int lane, double *fb, int *pvb,
                                          double *pinvb) {
    const double rc = fast_rcp(cval);                               // (of the lane's own entry: off the chain)
    const int key = used ? -1 : (__double2hiint(cval) & 0x7fffffff);
    const int vm = wave_max_key(key);
    const unsigned long long hit = __ballot(key == vm);
    const int pv = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)hit) - 1);
    const double pinv = read_lane(rc, pv);
    fb[lane] = (lane == pv) ? 0.0 : cval * pinv;
    if (lane == 0) { *pvb = pv; *pinvb = pinv; }
}

// compile-time loop: f(std::integral_constant<int, K>) for K = 0, 1, ... (register arrays stay in registers)
template <class F, int... K>
__device__ __forceinline__ void static_for(F &&f, std::integer_sequence<int, K...>) {
    (f(std::integral_constant<int, K>{}), ...);
}

// R[lc] -= f * (R[lc] of lane pv) for the columns lc = L0 .. NC - 1 except SKIP.  The pivot row's entries come by
// readlane into SGPR pairs, GJ_BATCH columns at a time and then their FMAs: one column at a time the compiler reuses
// a single SGPR pair, and every FMA waits for its own two readlanes (~30 cycles per column).
constexpr int GJ_BATCH = 8;
template <int L0, int NC, int SKIP, int N>
__device__ __forceinline__ void gj_update(double (&R)[N], const double f, const int pv) {
    static_for([&](auto bc) {
        constexpr int l0 = L0 + GJ_BATCH * decltype(bc)::value;
        auto live = [](int lc) { return lc < NC && lc != SKIP; };
        double pr[GJ_BATCH];
#pragma unroll
        for (int j = 0; j < GJ_BATCH; ++j)
            if (live(l0 + j)) pr[j] = read_lane(R[l0 + j], pv);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < GJ_BATCH; ++j)
            if (live(l0 + j)) R[l0 + j] = fma(-f, pr[j], R[l0 + j]);
        __builtin_amdgcn_sched_barrier(0);
    }, std::make_integer_sequence<int, (NC - L0 + GJ_BATCH - 1) / GJ_BATCH>{});
}


// ------------------------------------------------------------------------------------
// wave-level primitives (64 lanes, DPP; no LDS traffic)
// ------------------------------------------------------------------------------------
// A wave-uniform index made opaque to the optimiser (it stays in SGPRs, at no cost): `p[opaque(i)]`
// with a loop-invariant per-lane pointer p is then addressed as p + i inside the branch that uses
// it, instead of becoming one more per-lane 64-bit pointer that loop strength reduction advances
// with a vector add on EVERY iteration, taken or not.
__device__ __forceinline__ size_t opaque_uniform(size_t i) {
    asm volatile("" : "+s"(i));
    return i;
}

// Fixed-shape tree sum over the 64 lanes, result broadcast to every lane (deterministic).
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_get<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v += dpp_get<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v += dpp_get<0x141, 0xf>(v);   // row_half_mirror
    v += dpp_get<0x140, 0xf>(v);   // row_mirror       -> every lane holds its 16-lane row sum
    // the two broadcasts only matter for row 3 (rows 1, 3 and rows 2, 3 are what LLVM's own
    // reductions enable with row_mask 0xa / 0xc); with all rows enabled and bound_ctrl every lane is
    // written, so no zero-initialised destination (2 v_mov + s_nop per stage) is needed.  The other
    // rows end up with sums nobody reads.
    v += dpp_get<0x142, 0xf>(v);   // row_bcast15: rows 1, 3 += total of rows 0, 2
    v += dpp_get<0x143, 0xf>(v);   // row_bcast31: row 3 += total of rows 0 + 1 -> lane 63 holds the sum
    return read_lane(v, 63);
}

// Two independent sums interleaved (same latency chain as one).
__device__ __forceinline__ void wave_sum2(double &a, double &b) {
    a += dpp_get<0xB1, 0xf>(a);   b += dpp_get<0xB1, 0xf>(b);
    a += dpp_get<0x4E, 0xf>(a);   b += dpp_get<0x4E, 0xf>(b);
    a += dpp_get<0x141, 0xf>(a);  b += dpp_get<0x141, 0xf>(b);
    a += dpp_get<0x140, 0xf>(a);  b += dpp_get<0x140, 0xf>(b);
    a += dpp_get<0x142, 0xf>(a);  b += dpp_get<0x142, 0xf>(b);
    a += dpp_get<0x143, 0xf>(a);  b += dpp_get<0x143, 0xf>(b);
    a = read_lane(a, 63);
    b = read_lane(b, 63);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory
// queue (s_waitcnt vmcnt(0) before s_barrier), which turns a software prefetch issued before the
// barrier into a wait for HBM at the barrier; kernels whose waves exchange data through LDS alone use
// this instead and keep their global loads in flight.
__device__ __forceinline__ void wg_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Order LDS traffic of ONE wave: lane-form writes before uniform (broadcast) reads.
__device__ __forceinline__ void wave_lds_fence() {
    // LDS operations of one wave execute in issue order, so wavefront scope (a pure
    // compiler fence, no s_waitcnt) is enough and leaves global prefetches in flight.
    // The fences name the LDS address space only, so global loads stay provably unclobbered
    // (which is what lets hipcc turn wave-uniform row loads into s_load).
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

}  // namespace
