// Mesh distance (include/surs.h "mesh distance"): each point's distance to the nearest triangle of a mesh and that triangle's index,
// by brute force - the decomposition of surs_mesh_contains (surs_mesh_sample.hip) with the arithmetic of surs_mesh_distance.h.
//
//   mesh_distance_parts_kernel   grid = (point tiles of 256 lanes x 4 points in registers) x (face parts of SURS_MESH_FACES_PER_PART).
//                                A part's triangles go through md_prepare 256 at a time, one per lane, into LDS as seven float4 each;
//                                every lane then reads the same record (LDS broadcast) and runs md_dist2 on its four points.  The
//                                running (d2, face) per point - strict <, faces in order: the lowest face of a tie - goes to the
//                                part's slab of workspace [parts][n].
//   mesh_distance_reduce_kernel  per point the minimum over the parts in index order (strict < again), the square root, the face.
//   surs_mesh_distance_host      the same header looped on the host: what the kernels are held against bit for bit.
// No atomics, no acceleration structure; the parts are a function of nf alone and a point never looks at another point, so its two
// results do not depend on the batch it arrives in.  Arithmetic bound: 112 bytes of LDS per triangle per 1024 pairs.
// Built with the library's -ffp-contract=off: no product and sum of the header may become an fma the host does not form.
#include "surs_common.h"
#include "surs_mesh_distance.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {
using namespace surs;

constexpr int DIST_THREADS = 256;
constexpr int DIST_PPL = 4;                                  // points per lane
constexpr int DIST_TILE = DIST_THREADS * DIST_PPL;           // points per workgroup
constexpr int DIST_CHUNK = 256;                              // triangles staged in LDS at a time
constexpr int DIST_PART = SURS_MESH_FACES_PER_PART;          // triangles per face part
static_assert(DIST_PART % DIST_CHUNK == 0 && DIST_CHUNK == DIST_THREADS, "one staged triangle per thread");

struct DistEntry {   // one point's result in one part
    float d2;
    int32_t face;
};
static_assert(sizeof(DistEntry) == 8, "workspace entries are (fp32, int32)");

union RecordBits {
    MdRecord r;
    float4 q[7];
};

inline int clamp_index_h(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ inline int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ __launch_bounds__(DIST_THREADS) void mesh_distance_parts_kernel(const float *__restrict__ points, int n, int ld,
                                                                            const float *__restrict__ verts, int nv,
                                                                            const int32_t *__restrict__ faces, int nf,
                                                                            DistEntry *__restrict__ partial) {
    __shared__ float4 rec[DIST_CHUNK][7];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * DIST_TILE;
    const int part = blockIdx.y;
    const int f_begin = part * DIST_PART;
    const int f_end = min(nf, f_begin + DIST_PART);

    float px[DIST_PPL], py[DIST_PPL], pz[DIST_PPL], best[DIST_PPL];
    int best_face[DIST_PPL];
#pragma unroll
    for (int j = 0; j < DIST_PPL; ++j) {
        const int p = min(p0 + j * DIST_THREADS + tid, n - 1);   // lanes behind the end repeat the last point and store nothing
        const float *src = points + (size_t)p * ld;
        px[j] = src[0], py[j] = src[1], pz[j] = src[2];
        best[j] = INFINITY, best_face[j] = -1;
    }
    for (int c0 = f_begin; c0 < f_end; c0 += DIST_CHUNK) {
        const int cn = min(DIST_CHUNK, f_end - c0);
        __syncthreads();   // the previous chunk has been read
        if (tid < cn) {
            const int32_t *f = faces + (size_t)(c0 + tid) * 3;
            RecordBits u;
            u.r = md_prepare(verts + (size_t)clamp_index(f[0], nv) * 3, verts + (size_t)clamp_index(f[1], nv) * 3,
                             verts + (size_t)clamp_index(f[2], nv) * 3);
#pragma unroll
            for (int k = 0; k < 7; ++k) rec[tid][k] = u.q[k];
        }
        __syncthreads();
        for (int t = 0; t < cn; ++t) {
            RecordBits u;
#pragma unroll
            for (int k = 0; k < 7; ++k) u.q[k] = rec[t][k];   // every lane the same address: LDS broadcast
            const int face = c0 + t;
#pragma unroll
            for (int j = 0; j < DIST_PPL; ++j) {
                const float d2 = md_dist2(px[j], py[j], pz[j], u.r);
                const bool less = d2 < best[j];
                best[j] = less ? d2 : best[j];
                best_face[j] = less ? face : best_face[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < DIST_PPL; ++j) {
        const int p = p0 + j * DIST_THREADS + tid;
        if (p < n) {
            DistEntry e;
            e.d2 = best[j], e.face = best_face[j];
            partial[(size_t)part * n + p] = e;
        }
    }
}

__global__ __launch_bounds__(256) void mesh_distance_reduce_kernel(const DistEntry *__restrict__ partial, int n, int parts,
                                                                    float *__restrict__ dist, int32_t *__restrict__ face) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    float best = INFINITY;
    int best_face = -1;
    for (int k = 0; k < parts; ++k) {
        const DistEntry e = partial[(size_t)k * n + p];
        const bool less = e.d2 < best;
        best = less ? e.d2 : best;
        best_face = less ? e.face : best_face;
    }
    dist[p] = md_sqrt(best);
    if (face) face[p] = best_face;
}

int distance_args(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf) {
    SURS_REQUIRE(verts && faces, "verts and faces must not be NULL");
    SURS_REQUIRE(nv >= 1 && nf >= 1, "a mesh needs vertices and faces (nv %d, nf %d)", nv, nf);
    SURS_REQUIRE(n >= 0 && ld >= 3, "n %d must be >= 0 and ld %d >= 3", n, ld);
    return 0;
}
}  // namespace

extern "C" size_t surs_mesh_distance_workspace_bytes(int n, int nf) {
    if (n < 1 || nf < 1) return 0;
    return (size_t)surs_mesh_contains_parts(nf) * (size_t)n * sizeof(DistEntry);
}

extern "C" int surs_mesh_distance(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf,
                                  void *workspace, size_t workspace_bytes, float *dist, int32_t *face, void *stream) {
    if (int e = distance_args(points, n, ld, verts, nv, faces, nf)) return e;
    if (n == 0) return 0;
    SURS_REQUIRE(points && dist, "points and dist must not be NULL");
    const size_t need = surs_mesh_distance_workspace_bytes(n, nf);
    SURS_REQUIRE(workspace && workspace_bytes >= need, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int parts = surs_mesh_contains_parts(nf);
    SURS_REQUIRE(parts <= 65535, "%d faces make %d face parts; a launch takes 65535", nf, parts);
    hipStream_t st = as_stream(stream);
    DistEntry *partial = (DistEntry *)workspace;
    hipLaunchKernelGGL(mesh_distance_parts_kernel, dim3(ceil_div(n, DIST_TILE), parts), dim3(DIST_THREADS), 0, st, points, n, ld, verts, nv,
                       faces, nf, partial);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mesh_distance_reduce_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, partial, n, parts, dist, face);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_mesh_distance_host(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf,
                                       float *dist, int32_t *face) {
    if (int e = distance_args(points, n, ld, verts, nv, faces, nf)) return e;
    if (n == 0) return 0;
    SURS_REQUIRE(points && dist, "points and dist must not be NULL");
    std::vector<MdRecord> rec((size_t)nf);
    for (int f = 0; f < nf; ++f) {
        const int32_t *t = faces + (size_t)f * 3;
        rec[f] = md_prepare(verts + (size_t)clamp_index_h(t[0], nv) * 3, verts + (size_t)clamp_index_h(t[1], nv) * 3,
                            verts + (size_t)clamp_index_h(t[2], nv) * 3);
    }
    // strict < over the faces in order is what the parts (strict < inside, combined in index order) amount to
    for (int i = 0; i < n; ++i) {
        const float *p = points + (size_t)i * ld;
        float best = INFINITY;
        int best_face = -1;
        for (int f = 0; f < nf; ++f) {
            const float d2 = md_dist2(p[0], p[1], p[2], rec[f]);
            const bool less = d2 < best;
            best = less ? d2 : best;
            best_face = less ? f : best_face;
        }
        dist[i] = md_sqrt(best);
        if (face) face[i] = best_face;
    }
    return 0;
}
