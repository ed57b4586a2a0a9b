// The optimiser step (include/surs.h, "optimiser step"): every parameter tensor of a device table updated in place in ONE launch, by
// the per-element arithmetic of surs_optim_update.h.
//   surs_optim_step       the kernel entry
//   surs_optim_step_host  the same header looped on the host (what the kernel is held against bit for bit)
//   surs_optim_check      the table's check, on a host copy
// A workgroup visit is a chunk of OU_CHUNK = 4096 consecutive elements of one item; the grid is fixed (OP_GRID workgroups striding over
// the chunks of all items, as surs_conv_repack's over its tiles): the table and its chunk total are on the device and the entry takes
// (items, n, hyper-parameters, stream) only.  Memory bound: ADAM reads p, g, m, v and writes p, m, v - 28 bytes per element -, so the
// work is the access pattern: 16-byte loads and stores where every pointer of the item is 16-byte aligned at the chunk (chunks start at
// multiples of 4096 elements, so that is the alignment of the tensors themselves), scalar ones otherwise and for the n % 4 tail.  No LDS,
// no atomics; the kind and the number of state tensors are template parameters, so a kind's kernel holds no other kind's code.
// Built with the library's -ffp-contract=off: no product and sum of the header may become an fma the host does not form.
#include <cstdint>

#include "surs_common.h"
#include "surs_optim_update.h"

namespace surs {

constexpr int OP_THREADS = 256, OP_GRID = 2048;

// The item's pointers come out of the table, so the compiler cannot know their address space and would emit flat accesses: they are
// device (global) pointers by the table's contract, and typed so.
typedef __attribute__((address_space(1))) float gfloat;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gf32x4;

template <int KIND, int NS>
__device__ inline void op_one(gfloat *p, const gfloat *g, gfloat *s0, gfloat *s1, gfloat *s2, int i, const SursOptimHyper &h) {
    float P = p[i], A = 0.0f, B = 0.0f, Cc = 0.0f;
    if (NS > 0) A = s0[i];
    if (NS > 1) B = s1[i];
    if (NS > 2) Cc = s2[i];
    ou_update<KIND>(P, g[i], A, B, Cc, h);
    p[i] = P;
    if (NS > 0) s0[i] = A;
    if (NS > 1) s1[i] = B;
    if (NS > 2) s2[i] = Cc;
}

template <int KIND, int NS>
__global__ __launch_bounds__(OP_THREADS) void optim_kernel(const SursOptimItem *__restrict__ items, int n, SursOptimHyper h) {
    const int total = items[n - 1].chunk_end;
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        // the item of chunk t: the first whose chunk_end is beyond t (uniform over the workgroup; empty items are never found)
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].chunk_end > t) hi = mid;
            else lo = mid + 1;
        }
        const SursOptimItem it = items[lo];
        if (!it.p || !it.g || (NS > 0 && !it.s0) || (NS > 1 && !it.s1) || (NS > 2 && !it.s2)) continue;   // (surs_optim_check refuses these)
        const long long e0 = (long long)(t - (it.chunk_end - ou_chunks(it.n))) * OU_CHUNK;
        if (e0 < 0 || e0 >= it.n) continue;                                                               // (a chunk_end that is no prefix sum)
        const int cnt = it.n - e0 < OU_CHUNK ? (int)(it.n - e0) : OU_CHUNK;
        gfloat *p = (gfloat *)(it.p + e0), *s0 = NS > 0 ? (gfloat *)(it.s0 + e0) : nullptr, *s1 = NS > 1 ? (gfloat *)(it.s1 + e0) : nullptr,
               *s2 = NS > 2 ? (gfloat *)(it.s2 + e0) : nullptr;
        const gfloat *g = (const gfloat *)(it.g + e0);
        const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)s2;
        if ((bits & 15) == 0) {
            const int n4 = cnt >> 2;
            for (int i = threadIdx.x; i < n4; i += OP_THREADS) {
                f32x4 P = ((const gf32x4 *)p)[i], A = {}, B = {}, Cc = {};
                const f32x4 G = ((const gf32x4 *)g)[i];
                if (NS > 0) A = ((const gf32x4 *)s0)[i];
                if (NS > 1) B = ((const gf32x4 *)s1)[i];
                if (NS > 2) Cc = ((const gf32x4 *)s2)[i];
                for (int e = 0; e < 4; ++e) {
                    float pe = P[e], a = A[e], b = B[e], c = Cc[e];
                    ou_update<KIND>(pe, G[e], a, b, c, h);
                    P[e] = pe, A[e] = a, B[e] = b, Cc[e] = c;
                }
                ((gf32x4 *)p)[i] = P;
                if (NS > 0) ((gf32x4 *)s0)[i] = A;
                if (NS > 1) ((gf32x4 *)s1)[i] = B;
                if (NS > 2) ((gf32x4 *)s2)[i] = Cc;
            }
            const int i = (n4 << 2) + (int)threadIdx.x;
            if (i < cnt) op_one<KIND, NS>(p, g, s0, s1, s2, i, h);
        } else {
            for (int i = threadIdx.x; i < cnt; i += OP_THREADS) op_one<KIND, NS>(p, g, s0, s1, s2, i, h);
        }
    }
}

template <int KIND>
inline void host_item(const SursOptimItem &it, const SursOptimHyper &h) {
    float unused = 0.0f;
    for (long long i = 0; i < it.n; ++i)
        ou_update<KIND>(it.p[i], it.g[i], it.s0 ? it.s0[i] : unused, it.s1 ? it.s1[i] : unused, it.s2 ? it.s2[i] : unused, h);
}

}  // namespace surs

using namespace surs;

extern "C" int surs_optim_chunks(long long n) { return ou_chunks(n); }

extern "C" int surs_optim_check(const SursOptimItem *items, int n_items, const SursOptimHyper *h) {
    SURS_REQUIRE(h, "surs_optim: null hyper-parameters");
    const int ns = ou_states(h->kind, h->momentum);
    SURS_REQUIRE(ns >= 0, "surs_optim: kind %d is none of SURS_OPTIM_SGD, _ADAM, _AMSGRAD, _RMSPROP", h->kind);
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_optim: a null table of %d items", n_items);
    long long end = 0;
    for (int i = 0; i < n_items; ++i) {
        const SursOptimItem &it = items[i];
        SURS_REQUIRE(it.n >= 0, "surs_optim: item %d has n = %lld", i, it.n);
        SURS_REQUIRE(it.n <= (long long)OU_CHUNK * 0x7fffffff, "surs_optim: item %d has n = %lld", i, it.n);
        end += ou_chunks(it.n);
        SURS_REQUIRE(end <= 0x7fffffff && it.chunk_end == (int)end, "surs_optim: item %d has chunk_end %d, the prefix sum is %lld", i,
                     it.chunk_end, end);
        if (it.n == 0) continue;
        SURS_REQUIRE(it.p && it.g, "surs_optim: item %d has a null %s", i, it.p ? "gradient" : "value");
        SURS_REQUIRE((ns < 1 || it.s0) && (ns < 2 || it.s1) && (ns < 3 || it.s2), "surs_optim: item %d misses a state tensor (kind %d needs %d)",
                     i, h->kind, ns);
    }
    return SURS_OK;
}

extern "C" int surs_optim_step(const SursOptimItem *items, int n_items, const SursOptimHyper *h, void *stream) {
    SURS_REQUIRE(h, "surs_optim_step: null hyper-parameters");
    const int ns = ou_states(h->kind, h->momentum);
    SURS_REQUIRE(ns >= 0, "surs_optim_step: kind %d is none of SURS_OPTIM_SGD, _ADAM, _AMSGRAD, _RMSPROP", h->kind);
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_optim_step: a null table of %d items", n_items);
    if (n_items == 0) return SURS_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid(OP_GRID), block(OP_THREADS);
    switch (h->kind) {
        case SURS_OPTIM_SGD:
            if (ns) hipLaunchKernelGGL((optim_kernel<SURS_OPTIM_SGD, 1>), grid, block, 0, st, items, n_items, *h);
            else hipLaunchKernelGGL((optim_kernel<SURS_OPTIM_SGD, 0>), grid, block, 0, st, items, n_items, *h);
            break;
        case SURS_OPTIM_ADAM: hipLaunchKernelGGL((optim_kernel<SURS_OPTIM_ADAM, 2>), grid, block, 0, st, items, n_items, *h); break;
        case SURS_OPTIM_AMSGRAD: hipLaunchKernelGGL((optim_kernel<SURS_OPTIM_AMSGRAD, 3>), grid, block, 0, st, items, n_items, *h); break;
        default: hipLaunchKernelGGL((optim_kernel<SURS_OPTIM_RMSPROP, 1>), grid, block, 0, st, items, n_items, *h); break;
    }
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_optim_step_host(const SursOptimItem *items, int n_items, const SursOptimHyper *h) {
    const int rc = surs_optim_check(items, n_items, h);
    if (rc) return rc;
    for (int i = 0; i < n_items; ++i) {
        switch (h->kind) {
            case SURS_OPTIM_SGD: host_item<SURS_OPTIM_SGD>(items[i], *h); break;
            case SURS_OPTIM_ADAM: host_item<SURS_OPTIM_ADAM>(items[i], *h); break;
            case SURS_OPTIM_AMSGRAD: host_item<SURS_OPTIM_AMSGRAD>(items[i], *h); break;
            default: host_item<SURS_OPTIM_RMSPROP>(items[i], *h); break;
        }
    }
    return SURS_OK;
}
