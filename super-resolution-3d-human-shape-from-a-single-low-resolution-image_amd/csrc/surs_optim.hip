// The optimiser step (include/surs.h, "optimiser step"): every parameter tensor of a device table updated in place in ONE launch, by
// the per-element arithmetic of surs_optim_update.h.
//   surs_optim_step       the kernel entry
//   surs_optim_step_host  the same header looped on the host (what the kernel is held against bit for bit)
//   surs_optim_check      the table's check, on a host copy
//   surs_optim_step_ranks the data-parallel step: the gradient of an element is the rank-ordered mean of R gathered slabs, formed in
//                         the same pass (surs_optim_update.h, ou_rank_sum) and never written; _ranks_host is its host twin
//   surs_tensors_pack     one launch that copies a device table of tensors to their destinations (a rank's send slab), on the same
//                         chunking; _check and _host with it
// A workgroup visit is a chunk of OU_CHUNK = 4096 consecutive elements of one item; the grid is fixed (OP_GRID workgroups striding over
// the chunks of all items, as surs_conv_repack's over its tiles): the table and its chunk total are on the device and the entry takes
// (items, n, hyper-parameters, stream) only.  Memory bound: ADAM reads p, g, m, v and writes p, m, v - 28 bytes per element -, so the
// work is the access pattern: 16-byte loads and stores where every pointer of the item is 16-byte aligned at the chunk (chunks start at
// multiples of 4096 elements, so that is the alignment of the tensors themselves), scalar ones otherwise and for the n % 4 tail.  No LDS,
// no atomics; the kind and the number of state tensors are template parameters, so a kind's kernel holds no other kind's code.
// Built with the library's -ffp-contract=off: no product and sum of the header may become an fma the host does not form.
//
// The ranks kernel is the same body with g read R times, rank_stride apart: (R + state) x 4 bytes per element, still memory bound, and
// what matters is how many of a lane's loads are in flight.  A lane issues the loads of up to OU_RANK_UNROLL = 8 ranks (16 bytes each
// on the vector path) before the first add, next to its p and state loads: with R <= 8 - one node - every load of an element is
// independent and issued up front, 8 x 16 B x 256 lanes = 32 KiB of gradient per workgroup visit, which with the two or more
// workgroups a CU holds is beyond the 32-72 KiB per CU that hide an HBM miss on this part; more would only cost registers (8 ranks
// are 32 VGPRs of gradient beside at most 16 of p and state).  Beyond 8 ranks the sum goes on in batches of 8, in the same order.
// The vector path additionally needs rank_stride % 4 == 0, so that every rank's row is as aligned as rank 0's.  num_ranks == 1 with
// scale == 1 launches surs_optim_step's own kernel: the same bits by construction and the same speed.
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

// how the ranks kernel reads a gradient: R rows rank_stride floats apart, summed in rank order and scaled (ou_rank_sum)
struct OpRanks {
    int R;
    long long stride;
    float scale;
};

template <int KIND, int NS, bool RANKS>
__device__ inline void op_one(gfloat *p, const gfloat *g, gfloat *s0, gfloat *s1, gfloat *s2, int i, const SursOptimHyper &h,
                              const OpRanks &rk) {
    float P = p[i], A = 0.0f, B = 0.0f, Cc = 0.0f;
    if (NS > 0) A = s0[i];
    if (NS > 1) B = s1[i];
    if (NS > 2) Cc = s2[i];
    const float G = RANKS ? ou_rank_sum<float>(g + i, rk.stride, rk.R, rk.scale) : g[i];
    ou_update<KIND>(P, G, A, B, Cc, h);
    p[i] = P;
    if (NS > 0) s0[i] = A;
    if (NS > 1) s1[i] = B;
    if (NS > 2) s2[i] = Cc;
}

template <int KIND, int NS, bool RANKS>
__device__ inline void optim_body(const SursOptimItem *__restrict__ items, int n, const SursOptimHyper &h, const OpRanks &rk) {
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
        if ((bits & 15) == 0 && (!RANKS || (rk.stride & 3) == 0)) {
            const int n4 = cnt >> 2;
            for (int i = threadIdx.x; i < n4; i += OP_THREADS) {
                f32x4 P = ((const gf32x4 *)p)[i], A = {}, B = {}, Cc = {};
                const f32x4 G = RANKS ? ou_rank_sum<f32x4>((const gf32x4 *)g + i, rk.stride >> 2, rk.R, rk.scale) : ((const gf32x4 *)g)[i];
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
            if (i < cnt) op_one<KIND, NS, RANKS>(p, g, s0, s1, s2, i, h, rk);
        } else {
            for (int i = threadIdx.x; i < cnt; i += OP_THREADS) op_one<KIND, NS, RANKS>(p, g, s0, s1, s2, i, h, rk);
        }
    }
}

template <int KIND, int NS>
__global__ __launch_bounds__(OP_THREADS) void optim_kernel(const SursOptimItem *__restrict__ items, int n, SursOptimHyper h) {
    optim_body<KIND, NS, false>(items, n, h, OpRanks{1, 0, 1.0f});
}

template <int KIND, int NS>
__global__ __launch_bounds__(OP_THREADS) void optim_ranks_kernel(const SursOptimItem *__restrict__ items, int n, SursOptimHyper h, OpRanks rk) {
    optim_body<KIND, NS, true>(items, n, h, rk);
}

// surs_tensors_pack: the chunk walk of optim_body over a table of (src, dst) pairs
__global__ __launch_bounds__(OP_THREADS) void pack_kernel(const SursPackItem *__restrict__ items, int n) {
    const int total = items[n - 1].chunk_end;
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].chunk_end > t) hi = mid;
            else lo = mid + 1;
        }
        const SursPackItem it = items[lo];
        if (!it.src || !it.dst) continue;                                                                 // (surs_tensors_pack_check refuses these)
        const long long e0 = (long long)(t - (it.chunk_end - ou_chunks(it.n))) * OU_CHUNK;
        if (e0 < 0 || e0 >= it.n) continue;                                                               // (a chunk_end that is no prefix sum)
        const int cnt = it.n - e0 < OU_CHUNK ? (int)(it.n - e0) : OU_CHUNK;
        const gfloat *src = (const gfloat *)(it.src + e0);
        gfloat *dst = (gfloat *)(it.dst + e0);
        if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
            const int n4 = cnt >> 2;
            for (int i = threadIdx.x; i < n4; i += OP_THREADS) ((gf32x4 *)dst)[i] = ((const gf32x4 *)src)[i];
            const int i = (n4 << 2) + (int)threadIdx.x;
            if (i < cnt) dst[i] = src[i];
        } else {
            for (int i = threadIdx.x; i < cnt; i += OP_THREADS) dst[i] = src[i];
        }
    }
}

template <int KIND>
inline void host_item(const SursOptimItem &it, const SursOptimHyper &h) {
    float unused = 0.0f;
    for (long long i = 0; i < it.n; ++i)
        ou_update<KIND>(it.p[i], it.g[i], it.s0 ? it.s0[i] : unused, it.s1 ? it.s1[i] : unused, it.s2 ? it.s2[i] : unused, h);
}

template <int KIND>
inline void host_item_ranks(const SursOptimItem &it, const SursOptimHyper &h, int R, long long stride, float scale) {
    float unused = 0.0f;
    for (long long i = 0; i < it.n; ++i)
        ou_update<KIND>(it.p[i], ou_rank_sum<float>(it.g + i, stride, R, scale), it.s0 ? it.s0[i] : unused, it.s1 ? it.s1[i] : unused,
                        it.s2 ? it.s2[i] : unused, h);
}

inline int ranks_check(const char *who, int num_ranks, long long rank_stride, float scale) {
    SURS_REQUIRE(num_ranks >= 1 && num_ranks <= OU_MAX_RANKS, "%s: %d ranks (1 .. %d)", who, num_ranks, OU_MAX_RANKS);
    SURS_REQUIRE(rank_stride >= 0, "%s: rank_stride %lld", who, rank_stride);
    SURS_REQUIRE(scale == scale, "%s: scale is NaN", who);
    return SURS_OK;
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

extern "C" int surs_optim_step_ranks(const SursOptimItem *items, int n_items, const SursOptimHyper *h, int num_ranks, long long rank_stride,
                                     float scale, void *stream) {
    SURS_REQUIRE(h, "surs_optim_step_ranks: null hyper-parameters");
    const int ns = ou_states(h->kind, h->momentum);
    SURS_REQUIRE(ns >= 0, "surs_optim_step_ranks: kind %d is none of SURS_OPTIM_SGD, _ADAM, _AMSGRAD, _RMSPROP", h->kind);
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_optim_step_ranks: a null table of %d items", n_items);
    const int rc = ranks_check("surs_optim_step_ranks", num_ranks, rank_stride, scale);
    if (rc) return rc;
    if (num_ranks == 1 && scale == 1.0f) return surs_optim_step(items, n_items, h, stream);
    if (n_items == 0) return SURS_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid(OP_GRID), block(OP_THREADS);
    const OpRanks rk{num_ranks, rank_stride, scale};
    switch (h->kind) {
        case SURS_OPTIM_SGD:
            if (ns) hipLaunchKernelGGL((optim_ranks_kernel<SURS_OPTIM_SGD, 1>), grid, block, 0, st, items, n_items, *h, rk);
            else hipLaunchKernelGGL((optim_ranks_kernel<SURS_OPTIM_SGD, 0>), grid, block, 0, st, items, n_items, *h, rk);
            break;
        case SURS_OPTIM_ADAM: hipLaunchKernelGGL((optim_ranks_kernel<SURS_OPTIM_ADAM, 2>), grid, block, 0, st, items, n_items, *h, rk); break;
        case SURS_OPTIM_AMSGRAD: hipLaunchKernelGGL((optim_ranks_kernel<SURS_OPTIM_AMSGRAD, 3>), grid, block, 0, st, items, n_items, *h, rk); break;
        default: hipLaunchKernelGGL((optim_ranks_kernel<SURS_OPTIM_RMSPROP, 1>), grid, block, 0, st, items, n_items, *h, rk); break;
    }
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_optim_step_ranks_host(const SursOptimItem *items, int n_items, const SursOptimHyper *h, int num_ranks,
                                          long long rank_stride, float scale) {
    int rc = surs_optim_check(items, n_items, h);
    if (rc) return rc;
    rc = ranks_check("surs_optim_step_ranks_host", num_ranks, rank_stride, scale);
    if (rc) return rc;
    for (int i = 0; i < n_items; ++i) {
        switch (h->kind) {
            case SURS_OPTIM_SGD: host_item_ranks<SURS_OPTIM_SGD>(items[i], *h, num_ranks, rank_stride, scale); break;
            case SURS_OPTIM_ADAM: host_item_ranks<SURS_OPTIM_ADAM>(items[i], *h, num_ranks, rank_stride, scale); break;
            case SURS_OPTIM_AMSGRAD: host_item_ranks<SURS_OPTIM_AMSGRAD>(items[i], *h, num_ranks, rank_stride, scale); break;
            default: host_item_ranks<SURS_OPTIM_RMSPROP>(items[i], *h, num_ranks, rank_stride, scale); break;
        }
    }
    return SURS_OK;
}

extern "C" int surs_tensors_pack_check(const SursPackItem *items, int n_items) {
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_tensors_pack: a null table of %d items", n_items);
    long long end = 0;
    for (int i = 0; i < n_items; ++i) {
        const SursPackItem &it = items[i];
        SURS_REQUIRE(it.n >= 0 && it.n <= (long long)OU_CHUNK * 0x7fffffff, "surs_tensors_pack: item %d has n = %lld", i, it.n);
        end += ou_chunks(it.n);
        SURS_REQUIRE(end <= 0x7fffffff && it.chunk_end == (int)end, "surs_tensors_pack: item %d has chunk_end %d, the prefix sum is %lld", i,
                     it.chunk_end, end);
        SURS_REQUIRE(it.n == 0 || (it.src && it.dst), "surs_tensors_pack: item %d has a null %s", i, it.src ? "destination" : "source");
    }
    return SURS_OK;
}

extern "C" int surs_tensors_pack(const SursPackItem *items, int n_items, void *stream) {
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_tensors_pack: a null table of %d items", n_items);
    if (n_items == 0) return SURS_OK;
    hipLaunchKernelGGL(pack_kernel, dim3(OP_GRID), dim3(OP_THREADS), 0, as_stream(stream), items, n_items);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_tensors_pack_host(const SursPackItem *items, int n_items) {
    const int rc = surs_tensors_pack_check(items, n_items);
    if (rc) return rc;
    for (int i = 0; i < n_items; ++i)
        for (long long e = 0; e < items[i].n; ++e) items[i].dst[e] = items[i].src[e];
    return SURS_OK;
}
