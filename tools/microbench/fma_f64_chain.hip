// Cycles per v_fma_f64 on one wave, as a chain of dependent FMAs and as 2, 4 and 8 chains side by side (development):
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/fma_f64_chain tools/microbench/fma_f64_chain.hip && /tmp/fma_f64_chain
// One chain gives the dependent latency, eight the issue rate; the finishing block's state update is the first kind.
#include <hip/hip_runtime.h>
#include <stdio.h>
template <int CH>
__global__ void k(double *out, long long *cyc, double a) {
    double x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = out[threadIdx.x] + c;
    const long long t0 = clock64();
    for (int it = 0; it < 256; ++it) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int c = 0; c < CH; ++c) x[c] = fma(a, x[c], 1.0);
        __builtin_amdgcn_sched_barrier(0);
    }
    const long long t1 = clock64();
    double s = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) s += x[c];
    out[threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[0] = t1 - t0;
}
template <int CH>
void run(double *out, long long *cyc) {
    long long h = 0;
    for (int r = 0; r < 2; ++r) hipLaunchKernelGGL(k<CH>, dim3(1), dim3(64), 0, 0, out, cyc, 0.5);
    (void)hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost);
    printf("%d chain(s): %6.2f cycles per fma, %6.2f per step of a chain\n", CH, h / (256.0 * 16 * CH), h / (256.0 * 16));
}
int main() {
    double *out; long long *cyc;
    (void)hipMalloc(&out, 64 * 8); (void)hipMemset(out, 0, 64 * 8);
    (void)hipMalloc(&cyc, 8);
    run<1>(out, cyc); run<2>(out, cyc); run<4>(out, cyc); run<8>(out, cyc);
    return 0;
}
