// Exhaustive check that the column kernels' LeakyReLU keeps its bits: for every one of the 2^32 float bit patterns x,
// maximum(x, 0.01 x) (IEEE-754-2019 maximum: one v_maximum3_f32 on gfx950, what lrelu_max of surs_query.hip compiles to) against
// fmaxf(x, 0.01 x) (maxnum behind a canonicalising v_max_f32, the earlier form).  Prints the number of differing results, split
// into signalling-NaN inputs (which an MFMA never produces) and all others, and the first differing input.
//     hipcc -O3 --offload-arch=gfx950 -ffp-contract=off tools/micro/lrelu_bits.hip -o tools/micro/lrelu_bits && tools/micro/lrelu_bits
#include <hip/hip_runtime.h>
#include <cstdio>
__device__ __forceinline__ float opaque_f(float v) {
    asm volatile("" : "+v"(v));   // hides where x comes from, as an MFMA result is hidden from the compiler
    return v;
}
__global__ void k(unsigned long long *out) {   // out: [0] differing non-sNaN inputs, [1] differing sNaN inputs, [2] first differing input + 1
    const unsigned long long n = 1ull << 32, stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, bad_snan = 0, first = ~0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned xb = (unsigned)i;
        const float x = opaque_f(__uint_as_float(xb));
        const float y = 0.01f * x;
        const unsigned a = __float_as_uint(__builtin_elementwise_maximum(x, y)), b = __float_as_uint(fmaxf(x, y));
        if (a != b) {
            const bool snan = (xb & 0x7f800000u) == 0x7f800000u && (xb & 0x007fffffu) != 0 && !(xb & 0x00400000u);
            if (snan) ++bad_snan; else ++bad;
            if (i < first) first = i;
        }
    }
    if (bad) atomicAdd(&out[0], bad);
    if (bad_snan) atomicAdd(&out[1], bad_snan);
    if (first != ~0ull) atomicMin(&out[2], first + 1);
}
int main() {
    unsigned long long *d, h[3] = {0, 0, ~0ull};
    if (hipMalloc(&d, sizeof h) != hipSuccess || hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return 2;
    k<<<4096, 256>>>(d);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("maximum(x, 0.01 x) vs fmaxf(x, 0.01 x) over 2^32 inputs: %llu differ (not sNaN), %llu differ (sNaN inputs)", h[0], h[1]);
    if (h[2] != ~0ull) printf(", first 0x%08llx", h[2] - 1);
    printf("\n");
    return h[0] ? 1 : 0;
}
