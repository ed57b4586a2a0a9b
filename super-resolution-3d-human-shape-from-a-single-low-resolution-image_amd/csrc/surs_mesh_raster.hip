// Mesh raster (include/surs.h "mesh raster"): which triangle of a mesh each pixel of an orthographic view sees, its depth and its
// barycentric coordinates, and the normal map made from them - the decomposition of surs_mesh_distance (pixels for points) with the
// arithmetic of surs_mesh_raster.h.  No lists in memory, no atomics.
//
//   mesh_raster_prepare_kernel   one lane per face: mr_prepare, of which the 16-byte pixel box goes to the workspace.
//   mesh_raster_parts_kernel     grid = (pixel tiles of 32 x 32, four pixels per lane) x (face parts of the option raster_part).  A
//                                workgroup walks its part 256 faces at a time: each lane tests ONE face's box against the tile; the
//                                faces that overlap are ranked in FACE ORDER by wave ballot and prefix (the compaction of
//                                surs_sample_select) and their lanes run mr_prepare again, into LDS (five float4 a face).  After a
//                                barrier every lane reads the same record (LDS broadcast) and runs mr_cover on its four pixels, keeping
//                                (z', face, b1, b2) under mr_better.  The part's result goes to workspace [parts][h * w].
//   mesh_raster_reduce_kernel    per pixel the parts in index order under mr_better again: face, depth (NaN on background), bary.
//   mesh_shade_normals_kernel    one lane per pixel: mr_shade from face / bary.
//   surs_mesh_raster_host, surs_mesh_shade_normals_host   the same header looped on the host: what the kernels are held against bit
//                                for bit.
// The records are NOT kept in the workspace between the two kernels (80 bytes a face: 76 MiB for 10^6 faces); the lane that finds an
// overlap builds its face's record again, which the same function on the same input makes the same bits.  A triangle is built about
// once per tile it touches.  The part count is a function of nf and the option alone; a pixel never looks at another pixel, the box is
// part of mr_cover and the winner rule is free of order, so a pixel's results depend neither on the image it sits in, nor on the
// tile, the part size or the workspace.  Built with the library's -ffp-contract=off.
#include "surs_common.h"
#include "surs_mesh_raster.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {
using namespace surs;

constexpr int RAST_THREADS = 256;
constexpr int RAST_TILE = 32;                                  // pixels along a tile's side
constexpr int RAST_PPL = RAST_TILE * RAST_TILE / RAST_THREADS; // pixels per lane: rows ly, ly + 8, ly + 16, ly + 24 of column lx
constexpr int RAST_ROWS = RAST_THREADS / RAST_TILE;            // tile rows one pass of the workgroup covers
constexpr int RAST_CHUNK = 256;                                // faces tested at a time, one per lane
constexpr int RAST_MAX_SIDE = 8192;
static_assert(RAST_CHUNK == RAST_THREADS && RAST_PPL == 4 && RAST_ROWS == 8, "one tested face per thread, four pixels per lane");

struct View {
    float m[12];
};

struct RasterEntry {   // one pixel's result in one part
    float z;
    int32_t face;
    float b1, b2;
};
static_assert(sizeof(RasterEntry) == 16, "workspace entries are one float4");

union RecordBits {
    MrRecord r;
    float4 q[5];
};

inline int clamp_index_h(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ inline int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ inline MrRecord prepare_face(const float *__restrict__ verts, int nv, const int32_t *__restrict__ faces, int f, const View &view,
                                        int w, int h) {
    const int32_t *t = faces + (size_t)f * 3;
    int i0 = clamp_index(t[0], nv), i1 = clamp_index(t[1], nv), i2 = clamp_index(t[2], nv);
    mr_sort3(i0, i1, i2);
    return mr_prepare(verts + (size_t)i0 * 3, verts + (size_t)i1 * 3, verts + (size_t)i2 * 3, view.m, w, h);
}

__global__ __launch_bounds__(256) void mesh_raster_prepare_kernel(const float *__restrict__ verts, int nv, const int32_t *__restrict__ faces,
                                                                   int nf, View view, int w, int h, MrBox *__restrict__ boxes) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    boxes[f] = prepare_face(verts, nv, faces, f, view, w, h).box;
}

__global__ __launch_bounds__(RAST_THREADS) void mesh_raster_parts_kernel(const float *__restrict__ verts, int nv,
                                                                          const int32_t *__restrict__ faces, int nf, View view, int w, int h,
                                                                          int part_faces, int tiles_x, const MrBox *__restrict__ boxes,
                                                                          RasterEntry *__restrict__ partial) {
    __shared__ float4 rec[RAST_CHUNK][5];
    __shared__ int rec_face[RAST_CHUNK];
    __shared__ int wave_count[RAST_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = ((int)blockIdx.x % tiles_x) * RAST_TILE, ty0 = ((int)blockIdx.x / tiles_x) * RAST_TILE;
    const int part = blockIdx.y;
    const int f_begin = part * part_faces;
    const int f_end = min(nf, f_begin + part_faces);
    const int px = tx0 + (tid & (RAST_TILE - 1)), py0 = ty0 + tid / RAST_TILE;

    float best[RAST_PPL], best_b1[RAST_PPL], best_b2[RAST_PPL];
    int best_face[RAST_PPL];
#pragma unroll
    for (int k = 0; k < RAST_PPL; ++k) best[k] = -INFINITY, best_face[k] = -1, best_b1[k] = 0.0f, best_b2[k] = 0.0f;

    for (int c0 = f_begin; c0 < f_end; c0 += RAST_CHUNK) {
        const int f = c0 + tid;
        bool hit = false;
        if (f < f_end) {
            const MrBox b = boxes[f];
            hit = (b.xmin <= tx0 + RAST_TILE - 1) & (b.xmax >= tx0) & (b.ymin <= ty0 + RAST_TILE - 1) & (b.ymax >= ty0);
        }
        const unsigned long long mask = __ballot(hit);
        __syncthreads();   // the previous chunk's records and counts have been read
        if (lane == 0) wave_count[wave] = __popcll(mask);
        __syncthreads();
        int rank = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int v = 0; v < RAST_THREADS / 64; ++v) {
            const int c = wave_count[v];
            rank += v < wave ? c : 0;
            total += c;
        }
        if (total == 0) continue;   // (the whole workgroup: total is the same in every lane)
        if (hit) {
            RecordBits u;
            u.r = prepare_face(verts, nv, faces, f, view, w, h);
#pragma unroll
            for (int k = 0; k < 5; ++k) rec[rank][k] = u.q[k];
            rec_face[rank] = f;
        }
        __syncthreads();
        for (int t = 0; t < total; ++t) {
            RecordBits u;
#pragma unroll
            for (int k = 0; k < 5; ++k) u.q[k] = rec[t][k];   // every lane the same address: LDS broadcast
            const int face = rec_face[t];
#pragma unroll
            for (int k = 0; k < RAST_PPL; ++k) {
                float b1, b2, z;
                const bool covered = mr_cover(px, py0 + k * RAST_ROWS, u.r, &b1, &b2, &z);
                const bool better = mr_better(covered, z, best[k]);
                best[k] = better ? z : best[k];
                best_face[k] = better ? face : best_face[k];
                best_b1[k] = better ? b1 : best_b1[k];
                best_b2[k] = better ? b2 : best_b2[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RAST_PPL; ++k) {
        const int py = py0 + k * RAST_ROWS;
        if (px < w && py < h) {
            RasterEntry e;
            e.z = best[k], e.face = best_face[k], e.b1 = best_b1[k], e.b2 = best_b2[k];
            partial[((size_t)part * h + py) * w + px] = e;
        }
    }
}

__global__ __launch_bounds__(256) void mesh_raster_reduce_kernel(const RasterEntry *__restrict__ partial, int pixels, int parts,
                                                                  int32_t *__restrict__ face, float *__restrict__ depth,
                                                                  float *__restrict__ bary) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    RasterEntry best;
    best.z = -INFINITY, best.face = -1, best.b1 = 0.0f, best.b2 = 0.0f;
    for (int k = 0; k < parts; ++k) {
        const RasterEntry e = partial[(size_t)k * pixels + p];
        const bool better = mr_better(e.face >= 0, e.z, best.z);
        best.z = better ? e.z : best.z;
        best.face = better ? e.face : best.face;
        best.b1 = better ? e.b1 : best.b1;
        best.b2 = better ? e.b2 : best.b2;
    }
    face[p] = best.face;
    if (depth) depth[p] = best.face >= 0 ? best.z : NAN;
    if (bary) bary[(size_t)p * 2] = best.b1, bary[(size_t)p * 2 + 1] = best.b2;
}

struct NormalMatrix {
    float n[9];
};

__global__ __launch_bounds__(256) void mesh_shade_normals_kernel(const float *__restrict__ verts, int nv, const int32_t *__restrict__ faces,
                                                                  int nf, View view, const float *__restrict__ vertex_normals,
                                                                  NormalMatrix nm, const int32_t *__restrict__ face,
                                                                  const float *__restrict__ bary, int pixels, float *__restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const int f = face[p];
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if (f >= 0) {
        const int32_t *t = faces + (size_t)clamp_index(f, nf) * 3;
        int i0 = clamp_index(t[0], nv), i1 = clamp_index(t[1], nv), i2 = clamp_index(t[2], nv);
        mr_sort3(i0, i1, i2);
        const float *vn = vertex_normals;
        mr_shade(verts + (size_t)i0 * 3, verts + (size_t)i1 * 3, verts + (size_t)i2 * 3, view.m, vn ? vn + (size_t)i0 * 3 : nullptr,
                 vn ? vn + (size_t)i1 * 3 : nullptr, vn ? vn + (size_t)i2 * 3 : nullptr, nm.n, vn ? bary[(size_t)p * 2] : 0.0f,
                 vn ? bary[(size_t)p * 2 + 1] : 0.0f, rgb);
    }
    out[(size_t)p * 3] = rgb[0], out[(size_t)p * 3 + 1] = rgb[1], out[(size_t)p * 3 + 2] = rgb[2];
}

int mesh_args(const float *verts, int nv, const int32_t *faces, int nf, const float *view, int w, int h) {
    SURS_REQUIRE(verts && faces && view, "verts, faces and view must not be NULL");
    SURS_REQUIRE(nv >= 1 && nf >= 1, "a mesh needs vertices and faces (nv %d, nf %d)", nv, nf);
    SURS_REQUIRE(w >= 1 && h >= 1 && w <= RAST_MAX_SIDE && h <= RAST_MAX_SIDE, "an image of w %d x h %d: each must be in [1, %d]", w, h,
                 RAST_MAX_SIDE);
    return 0;
}

int shade_args(const float *vertex_normals, const float *normal_matrix, const int32_t *face, const float *bary, const float *out) {
    SURS_REQUIRE(face && out, "face and out must not be NULL");
    SURS_REQUIRE(!vertex_normals || (normal_matrix && bary), "vertex normals need the normal matrix and bary: neither may be NULL");
    return 0;
}

// faces per part: the option raster_part, checked; 0 with the error set
int part_faces() {
    const int part = option(OPT_RASTER_PART);
    if (part < RAST_CHUNK || part % RAST_CHUNK != 0) {
        fail(SURS_E_INVALID, "option raster_part %d: a positive multiple of %d is needed", part, RAST_CHUNK);
        return 0;
    }
    return part;
}

size_t boxes_bytes(int nf) { return align_up((size_t)nf * sizeof(MrBox), 256); }

View as_view(const float *view) {
    View v;
    for (int i = 0; i < 12; ++i) v.m[i] = view[i];
    return v;
}
}  // namespace

extern "C" int surs_mesh_raster_parts(int nf) {
    const int part = part_faces();
    if (nf < 1 || !part) return 0;
    return ceil_div(nf, part);
}

extern "C" size_t surs_mesh_raster_workspace_bytes(int w, int h, int nf) {
    const int parts = surs_mesh_raster_parts(nf);
    if (w < 1 || h < 1 || parts < 1) return 0;
    return boxes_bytes(nf) + (size_t)parts * (size_t)w * (size_t)h * sizeof(RasterEntry);
}

extern "C" int surs_mesh_raster(const float *verts, int nv, const int32_t *faces, int nf, const float *view, int w, int h, void *workspace,
                                size_t workspace_bytes, int32_t *face, float *depth, float *bary, void *stream) {
    if (int e = mesh_args(verts, nv, faces, nf, view, w, h)) return e;
    SURS_REQUIRE(face, "face must not be NULL");
    const int part = part_faces();
    if (!part) return SURS_E_INVALID;
    const int parts = ceil_div(nf, part);
    SURS_REQUIRE(parts <= 65535, "%d faces make %d face parts of %d; a launch takes 65535", nf, parts, part);
    const size_t need = surs_mesh_raster_workspace_bytes(w, h, nf);
    SURS_REQUIRE(workspace && workspace_bytes >= need, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    MrBox *boxes = (MrBox *)workspace;
    RasterEntry *partial = (RasterEntry *)((char *)workspace + boxes_bytes(nf));
    const View v = as_view(view);
    const int tiles_x = ceil_div(w, RAST_TILE), tiles_y = ceil_div(h, RAST_TILE);
    hipLaunchKernelGGL(mesh_raster_prepare_kernel, dim3(ceil_div(nf, 256)), dim3(256), 0, st, verts, nv, faces, nf, v, w, h, boxes);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mesh_raster_parts_kernel, dim3(tiles_x * tiles_y, parts), dim3(RAST_THREADS), 0, st, verts, nv, faces, nf, v, w, h,
                       part, tiles_x, boxes, partial);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mesh_raster_reduce_kernel, dim3(ceil_div((long long)w * h, 256)), dim3(256), 0, st, partial, w * h, parts, face, depth,
                       bary);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_mesh_shade_normals(const float *verts, int nv, const int32_t *faces, int nf, const float *view,
                                       const float *vertex_normals, const float *normal_matrix, const int32_t *face, const float *bary,
                                       int w, int h, float *out, void *stream) {
    if (int e = mesh_args(verts, nv, faces, nf, view, w, h)) return e;
    if (int e = shade_args(vertex_normals, normal_matrix, face, bary, out)) return e;
    NormalMatrix nm;
    for (int i = 0; i < 9; ++i) nm.n[i] = normal_matrix ? normal_matrix[i] : 0.0f;
    hipLaunchKernelGGL(mesh_shade_normals_kernel, dim3(ceil_div((long long)w * h, 256)), dim3(256), 0, as_stream(stream), verts, nv, faces,
                       nf, as_view(view), vertex_normals, nm, face, bary, w * h, out);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_mesh_raster_host(const float *verts, int nv, const int32_t *faces, int nf, const float *view, int w, int h,
                                     int32_t *face, float *depth, float *bary) {
    if (int e = mesh_args(verts, nv, faces, nf, view, w, h)) return e;
    SURS_REQUIRE(face, "face must not be NULL");
    const size_t pixels = (size_t)w * h;
    std::vector<float> best(pixels, -INFINITY), best_b(bary ? 0 : 2 * pixels);
    float *bb = bary ? bary : best_b.data();
    for (size_t p = 0; p < pixels; ++p) face[p] = -1, bb[2 * p] = 0.0f, bb[2 * p + 1] = 0.0f;
    // strict > over the faces in order is what the parts (strict > inside, combined in index order) amount to
    for (int f = 0; f < nf; ++f) {
        const int32_t *t = faces + (size_t)f * 3;
        int i0 = clamp_index_h(t[0], nv), i1 = clamp_index_h(t[1], nv), i2 = clamp_index_h(t[2], nv);
        mr_sort3(i0, i1, i2);
        const MrRecord r = mr_prepare(verts + (size_t)i0 * 3, verts + (size_t)i1 * 3, verts + (size_t)i2 * 3, view, w, h);
        for (int py = r.box.ymin; py <= r.box.ymax; ++py)
            for (int px = r.box.xmin; px <= r.box.xmax; ++px) {
                float b1, b2, z;
                const bool covered = mr_cover(px, py, r, &b1, &b2, &z);
                const size_t p = (size_t)py * w + px;
                if (mr_better(covered, z, best[p])) best[p] = z, face[p] = f, bb[2 * p] = b1, bb[2 * p + 1] = b2;
            }
    }
    if (depth)
        for (size_t p = 0; p < pixels; ++p) depth[p] = face[p] >= 0 ? best[p] : NAN;
    return 0;
}

extern "C" int surs_mesh_shade_normals_host(const float *verts, int nv, const int32_t *faces, int nf, const float *view,
                                            const float *vertex_normals, const float *normal_matrix, const int32_t *face,
                                            const float *bary, int w, int h, float *out) {
    if (int e = mesh_args(verts, nv, faces, nf, view, w, h)) return e;
    if (int e = shade_args(vertex_normals, normal_matrix, face, bary, out)) return e;
    const float *vn = vertex_normals;
    for (size_t p = 0; p < (size_t)w * h; ++p) {
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        if (face[p] >= 0) {
            const int32_t *t = faces + (size_t)clamp_index_h(face[p], nf) * 3;
            int i0 = clamp_index_h(t[0], nv), i1 = clamp_index_h(t[1], nv), i2 = clamp_index_h(t[2], nv);
            mr_sort3(i0, i1, i2);
            mr_shade(verts + (size_t)i0 * 3, verts + (size_t)i1 * 3, verts + (size_t)i2 * 3, view, vn ? vn + (size_t)i0 * 3 : nullptr,
                     vn ? vn + (size_t)i1 * 3 : nullptr, vn ? vn + (size_t)i2 * 3 : nullptr, normal_matrix, vn ? bary[2 * p] : 0.0f,
                     vn ? bary[2 * p + 1] : 0.0f, rgb);
        }
        out[3 * p] = rgb[0], out[3 * p + 1] = rgb[1], out[3 * p + 2] = rgb[2];
    }
    return 0;
}
