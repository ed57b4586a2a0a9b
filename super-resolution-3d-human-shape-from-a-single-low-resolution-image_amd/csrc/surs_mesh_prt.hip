// Per-vertex precomputed radiance transfer (include/surs.h "mesh PRT"): a brute-force visibility integral over a set of directions,
// the decomposition of surs_mesh_contains (rays for points) with the arithmetic of surs_mesh_prt.h.  No lists, no atomics.
//
//   mesh_prt_rays_kernel     one lane per ray g = v D + k, 256 consecutive rays a workgroup.  All faces stream through LDS PRT_CHUNK at
//                            a time: the workgroup runs prt_prepare on the chunk (three float4 a triangle), and after a barrier every
//                            lane reads the same record (LDS broadcast) and runs prt_hit.  Any-hit: a wave looks at its lanes every 16
//                            triangles and leaves the chunk once none of them still looks for a hit; the workgroup leaves the face loop
//                            at a chunk boundary once no wave does.  A boolean OR does not depend on the order or on where it stops, so
//                            the exits cannot change a bit.  The wave's 64 answers ("n . d > 0 and nothing hit") leave as two 32-bit
//                            words of its ballot: bit g of the workspace, written once, by plain vector stores.
//   mesh_prt_sum_kernel      one lane per vertex: its D bits in direction order through prt_term, then the scale.
//   surs_mesh_prt_host       the same header looped on the host: what the kernels are held against bit for bit.
// The workspace is ceil(nv D / 32) words whatever the number of face chunks.  A vertex's ray never looks at another vertex's, and the
// bits are only a transport, so a vertex's coefficients depend neither on nv, nor on its place in the array, nor on the workspace.
#include "surs_common.h"
#include "surs_mesh_prt.h"

#include <cstdint>
#include <vector>

namespace {
using namespace surs;

constexpr int PRT_THREADS = 256;
constexpr int PRT_LOOK = 16;   // triangles between two looks at the wave's lanes
static_assert(PRT_CHUNK % PRT_THREADS == 0 && PRT_CHUNK % PRT_LOOK == 0, "whole passes of the workgroup, whole groups of a look");
static_assert(PRT_CHUNK * sizeof(PrtTri) <= 64 * 1024, "the chunk is static LDS");

union TriBits {
    PrtTri t;
    float4 q[3];
};

inline int clamp_index_h(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ inline int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// COUNT: the wave also counts the triangles it looked at (a wave-uniform number) and lane 0 stores it - the timing tool's variant;
// the instantiation without it is the kernel of surs_mesh_prt.
template <bool COUNT>
__global__ __launch_bounds__(PRT_THREADS) void mesh_prt_rays_kernel(const float *__restrict__ verts, int nv, const int32_t *__restrict__ faces,
                                                                     int nf, const float *__restrict__ normals,
                                                                     const float *__restrict__ dirs, int D, float offset, int total,
                                                                     int words, uint32_t *__restrict__ bits,
                                                                     uint32_t *__restrict__ wave_tests) {
    __shared__ float4 tri[PRT_CHUNK][3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = (int)blockIdx.x * PRT_THREADS + tid;   // total < 2^31 - 256 (checked by the caller)
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    int v = 0;
    bool cast = false;
    if (g < total) {
        v = g / D;
        const int k = g - v * D;
        const float *n = normals + (size_t)v * 3;
        d[0] = dirs[(size_t)k * 3], d[1] = dirs[(size_t)k * 3 + 1], d[2] = dirs[(size_t)k * 3 + 2];
        const bool ok = prt_origin(verts + (size_t)v * 3, n, offset, o);
        cast = ok && prt_cosine(n, d) > 0.0f;
    }
    bool hit = false;
    uint32_t looked = 0;
    for (int c0 = 0; c0 < nf; c0 += PRT_CHUNK) {
        // (a barrier too: the previous chunk has been read) - the same answer in every lane of the workgroup
        if (!__syncthreads_or(cast && !hit)) break;
        const int cnt = min(PRT_CHUNK, nf - c0);
        for (int j = tid; j < cnt; j += PRT_THREADS) {
            const int32_t *t = faces + (size_t)(c0 + j) * 3;
            const int i0 = clamp_index(t[0], nv), i1 = clamp_index(t[1], nv), i2 = clamp_index(t[2], nv);
            TriBits u;
            u.t = prt_prepare(verts + (size_t)i0 * 3, verts + (size_t)i1 * 3, verts + (size_t)i2 * 3, i0, i1, i2);
#pragma unroll
            for (int q = 0; q < 3; ++q) tri[j][q] = u.q[q];
        }
        __syncthreads();
        for (int j0 = 0; j0 < cnt; j0 += PRT_LOOK) {
            if (__ballot(cast && !hit) == 0ull) break;   // (the whole wave)
            const int j1 = min(j0 + PRT_LOOK, cnt);
            if (COUNT) looked += (uint32_t)(j1 - j0);
            for (int j = j0; j < j1; ++j) {
                TriBits u;
#pragma unroll
                for (int q = 0; q < 3; ++q) u.q[q] = tri[j][q];   // every lane the same address: LDS broadcast
                hit |= prt_hit(o, d, v, u.t);
            }
        }
    }
    const unsigned long long mask = __ballot(cast && !hit);
    const int word = g >> 5;   // lane 0 and lane 32 hold the wave's two word indices
    if ((lane & 31) == 0 && word < words) bits[word] = lane ? (uint32_t)(mask >> 32) : (uint32_t)mask;
    if (COUNT && lane == 0 && g < total) wave_tests[g >> 6] = looked;   // [ceil(total / 64)]: only a wave that holds a ray
}

__global__ __launch_bounds__(256) void mesh_prt_sum_kernel(const float *__restrict__ verts, int nv, const float *__restrict__ normals,
                                                            const float *__restrict__ dirs, int D, float offset,
                                                            const uint32_t *__restrict__ bits, float *__restrict__ prt) {
    const int v = (int)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const float *n = normals + (size_t)v * 3;
    float o[3], acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.0f;
    if (prt_origin(verts + (size_t)v * 3, n, offset, o)) {
        const int g0 = v * D;
        for (int k = 0; k < D; ++k) {
            const int g = g0 + k;
            if ((bits[g >> 5] >> (g & 31)) & 1u) {
                const float *d = dirs + (size_t)k * 3;
                prt_term(prt_cosine(n, d), d, acc);
            }
        }
    }
    const float s = prt_scale(D);
#pragma unroll
    for (int i = 0; i < 9; ++i) prt[(size_t)v * 9 + i] = acc[i] * s;
}

constexpr long long PRT_MAX_RAYS = (1ll << 31) - 2 * PRT_THREADS;

int prt_args(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs, int D, float offset,
             const float *prt) {
    SURS_REQUIRE(verts && faces && normals && dirs && prt, "verts, faces, normals, dirs and prt must not be NULL");
    SURS_REQUIRE(nv >= 1 && nf >= 1, "a mesh needs vertices and faces (nv %d, nf %d)", nv, nf);
    SURS_REQUIRE(D >= 1, "%d directions: at least one is needed", D);
    SURS_REQUIRE((long long)nv * D <= PRT_MAX_RAYS, "%d vertices x %d directions: at most %lld rays a call", nv, D, PRT_MAX_RAYS);
    SURS_REQUIRE(prt_finite(offset) && offset >= 0.0f, "offset %g: a finite value >= 0 is needed", (double)offset);
    return 0;
}
}  // namespace

extern "C" size_t surs_mesh_prt_workspace_bytes(int nv, int D) {
    if (nv < 1 || D < 1 || (long long)nv * D > PRT_MAX_RAYS) return 0;
    return align_up((size_t)ceil_div((long long)nv * D, 32) * sizeof(uint32_t), 256);
}

namespace {
int prt_launch(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs, int D, float offset,
               float *prt, void *workspace, size_t workspace_bytes, uint32_t *wave_tests, void *stream) {
    if (int e = prt_args(verts, nv, faces, nf, normals, dirs, D, offset, prt)) return e;
    const size_t need = surs_mesh_prt_workspace_bytes(nv, D);
    SURS_REQUIRE(workspace && workspace_bytes >= need, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int total = nv * D, words = ceil_div(total, 32);
    const dim3 grid(ceil_div(total, PRT_THREADS)), block(PRT_THREADS);
    if (wave_tests)
        hipLaunchKernelGGL(mesh_prt_rays_kernel<true>, grid, block, 0, st, verts, nv, faces, nf, normals, dirs, D, offset, total, words,
                           (uint32_t *)workspace, wave_tests);
    else
        hipLaunchKernelGGL(mesh_prt_rays_kernel<false>, grid, block, 0, st, verts, nv, faces, nf, normals, dirs, D, offset, total, words,
                           (uint32_t *)workspace, (uint32_t *)nullptr);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mesh_prt_sum_kernel, dim3(ceil_div(nv, 256)), dim3(256), 0, st, verts, nv, normals, dirs, D, offset,
                       (const uint32_t *)workspace, prt);
    SURS_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int surs_mesh_prt(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs, int D,
                             float offset, float *prt, void *workspace, size_t workspace_bytes, void *stream) {
    return prt_launch(verts, nv, faces, nf, normals, dirs, D, offset, prt, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int surs_mesh_prt_counted(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs,
                                     int D, float offset, float *prt, void *workspace, size_t workspace_bytes, uint32_t *wave_tests,
                                     void *stream) {
    SURS_REQUIRE(wave_tests, "wave_tests must not be NULL");
    return prt_launch(verts, nv, faces, nf, normals, dirs, D, offset, prt, workspace, workspace_bytes, wave_tests, stream);
}

extern "C" int surs_mesh_prt_host(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs,
                                  int D, float offset, float *prt, uint8_t *visible) {
    if (int e = prt_args(verts, nv, faces, nf, normals, dirs, D, offset, prt)) return e;
    std::vector<PrtTri> tris((size_t)nf);
    for (int f = 0; f < nf; ++f) {
        const int32_t *t = faces + (size_t)f * 3;
        const int i0 = clamp_index_h(t[0], nv), i1 = clamp_index_h(t[1], nv), i2 = clamp_index_h(t[2], nv);
        tris[f] = prt_prepare(verts + (size_t)i0 * 3, verts + (size_t)i1 * 3, verts + (size_t)i2 * 3, i0, i1, i2);
    }
    const float s = prt_scale(D);
    for (int v = 0; v < nv; ++v) {
        const float *n = normals + (size_t)v * 3;
        float o[3], acc[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const bool ok = prt_origin(verts + (size_t)v * 3, n, offset, o);
        for (int k = 0; k < D; ++k) {
            const float *d = dirs + (size_t)k * 3;
            bool lit = false;
            if (ok) {
                const float cosine = prt_cosine(n, d);
                if (cosine > 0.0f) {
                    bool hit = false;
                    for (int f = 0; f < nf && !hit; ++f) hit = prt_hit(o, d, v, tris[f]);
                    lit = !hit;
                    if (lit) prt_term(cosine, d, acc);
                }
            }
            if (visible) visible[(size_t)v * D + k] = lit ? 1 : 0;
        }
        for (int i = 0; i < 9; ++i) prt[(size_t)v * 9 + i] = acc[i] * s;
    }
    return 0;
}
