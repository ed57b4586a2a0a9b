// Training samples (include/surs.h "training samples"): what TrainDataset_LR_v2.select_sampling_method does per item on the
// host - area-weighted surface samples with Gaussian jitter, uniform box points, two inside / outside tests of the whole
// pool, the truncated selection and the displacement labels - as four device calls.
//
//   surs_mesh_contains     generalized winding number by brute force.  Grid = (point tiles) x (face parts); a part's
//                          triangles are staged in LDS (vertices gathered once per workgroup) and read back by broadcast
//                          (every lane the same address), CONTAINS_PPL points per lane stay in registers.  Each part writes
//                          its partial sum to workspace [parts][n]; a second kernel adds the parts in index order (double)
//                          and thresholds.  The parts are a function of nf alone and a point's partial sums never look at
//                          another point, so a point's bits do not depend on the batch it arrives in.
//   surs_mesh_area_cdf     per-face area and its inclusive prefix sum in double: one workgroup walks the faces in order.
//   surs_mesh_sample_pool  the pool of surface + box points from the package's counter PRNG (prng.py, restated below).
//   surs_sample_select     the selection rule and labels_disp: one workgroup, a counting walk, then a stable compaction
//                          with wave ballots; no host synchronisation.
// No float atomics, fixed summation orders: every call returns the same bits.
#include "surs_common.h"

#include <cmath>
#include <cstdint>

namespace {
using namespace surs;

// ---------------------------------------------------------------- counter PRNG (prng.py)
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;

unsigned long long fnv1a64(const char *name) {
    unsigned long long h = 0xCBF29CE484222325ull;
    for (const unsigned char *p = (const unsigned char *)name; *p; ++p) {
        h ^= *p;
        h *= 0x100000001B3ull;
    }
    return h;
}
unsigned long long stream_key(const char *name, unsigned long long seed) { return fnv1a64(name) ^ (seed * kGolden); }

__host__ __device__ inline unsigned long long splitmix64(unsigned long long x) {
    x += kGolden;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the top 24 bits of value i of a stream
__device__ inline unsigned int bits24(unsigned long long key, unsigned long long i) { return (unsigned int)(splitmix64(key + i) >> 40); }
__device__ inline float uniform01(unsigned long long key, unsigned long long i) { return (float)bits24(key, i) * (1.0f / 16777216.0f); }

__device__ inline int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// ---------------------------------------------------------------- contains
constexpr int CONTAINS_THREADS = 256;
constexpr int CONTAINS_PPL = 4;                                      // points per lane
constexpr int CONTAINS_TILE = CONTAINS_THREADS * CONTAINS_PPL;       // points per workgroup
constexpr int CONTAINS_CHUNK = 256;                                  // triangles staged in LDS at a time
constexpr int CONTAINS_PART = SURS_MESH_FACES_PER_PART;              // triangles per face part
static_assert(CONTAINS_PART % CONTAINS_CHUNK == 0 && CONTAINS_CHUNK == CONTAINS_THREADS, "one staged triangle per thread");

// atan2 for the winding sum, about 20 instructions where the library's takes about 45: t = min / max of the magnitudes through one
// v_rcp_f32, atan(t) = t P(t^2) on [0, 1] with a degree-8 P (least squares on Chebyshev nodes in float64: 1.2e-8 from atan; in
// fp32 arithmetic 1.1e-7 absolute, 1.4e-7 relative, the constant term exactly 1 so that a small angle keeps its relative accuracy),
// then the octant.  Finite for finite arguments other than (0, 0), which the caller excludes.
__device__ __forceinline__ float atan2_poly(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = mn * __builtin_amdgcn_rcpf(mx), s = t * t;
    float p = 2.834064187e-03f;
    p = fmaf(p, s, -1.600502990e-02f);
    p = fmaf(p, s, 4.258760810e-02f);
    p = fmaf(p, s, -7.495445758e-02f);
    p = fmaf(p, s, 1.063675433e-01f);
    p = fmaf(p, s, -1.420257092e-01f);
    p = fmaf(p, s, 1.999248415e-01f);
    p = fmaf(p, s, -3.333306611e-01f);
    p = fmaf(p, s, 1.0f);
    float r = t * p;
    r = ay > ax ? 1.57079632679489661923f - r : r;
    r = x < 0.0f ? 3.14159265358979323846f - r : r;
    return copysignf(r, y);
}

// The solid angle of triangle (a, b, c) seen from the origin is 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
// (van Oosterom & Strackee 1983).  Returns the atan2; a determinant of exactly zero (a vertex at the point, an edge through it)
// contributes 0 whatever the sign of the denominator.  The lengths come from v_sqrt_f32 as it is (1 ulp; the squares are
// far from the denormal range that sqrtf's scaling guards).
__device__ __forceinline__ float half_solid_angle(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                                  float cz) {
    const float la = __builtin_amdgcn_sqrtf(ax * ax + ay * ay + az * az), lb = __builtin_amdgcn_sqrtf(bx * bx + by * by + bz * bz),
                lc = __builtin_amdgcn_sqrtf(cx * cx + cy * cy + cz * cz);
    const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
    const float ab = ax * bx + ay * by + az * bz, bc = bx * cx + by * cy + bz * cz, ca = cx * ax + cy * ay + cz * az;
    const float den = la * lb * lc + ab * lc + bc * la + ca * lb;
    const float t = atan2_poly(det, den);
    return det == 0.0f ? 0.0f : t;
}

__global__ __launch_bounds__(CONTAINS_THREADS) void mesh_winding_parts_kernel(const float *__restrict__ points, int n, int ld,
                                                                                const float *__restrict__ verts, int nv,
                                                                                const int32_t *__restrict__ faces, int nf,
                                                                                float *__restrict__ partial) {
    // 3 x float4 per triangle: (v0, keep), (v1, -), (v2, -); keep = 0 for a zero-area triangle
    __shared__ float4 tri[CONTAINS_CHUNK][3];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * CONTAINS_TILE;
    const int part = blockIdx.y;
    const int f_begin = part * CONTAINS_PART;
    const int f_end = min(nf, f_begin + CONTAINS_PART);

    float px[CONTAINS_PPL], py[CONTAINS_PPL], pz[CONTAINS_PPL];
    double acc[CONTAINS_PPL];
#pragma unroll
    for (int j = 0; j < CONTAINS_PPL; ++j) {
        const int p = min(p0 + j * CONTAINS_THREADS + tid, n - 1);   // lanes behind the end repeat the last point and store nothing
        const float *src = points + (size_t)p * ld;
        px[j] = src[0], py[j] = src[1], pz[j] = src[2];
        acc[j] = 0.0;
    }
    for (int c0 = f_begin; c0 < f_end; c0 += CONTAINS_CHUNK) {
        const int cn = min(CONTAINS_CHUNK, f_end - c0);
        __syncthreads();   // the previous chunk has been read
        if (tid < cn) {
            const int32_t *f = faces + (size_t)(c0 + tid) * 3;
            const float *v0 = verts + (size_t)clamp_index(f[0], nv) * 3, *v1 = verts + (size_t)clamp_index(f[1], nv) * 3,
                        *v2 = verts + (size_t)clamp_index(f[2], nv) * 3;
            const float x0 = v0[0], y0 = v0[1], z0 = v0[2], x1 = v1[0], y1 = v1[1], z1 = v1[2], x2 = v2[0], y2 = v2[1], z2 = v2[2];
            const float ex = x1 - x0, ey = y1 - y0, ez = z1 - z0, gx = x2 - x0, gy = y2 - y0, gz = z2 - z0;
            const float nx = ey * gz - ez * gy, ny = ez * gx - ex * gz, nz = ex * gy - ey * gx;
            const float keep = (nx == 0.0f && ny == 0.0f && nz == 0.0f) ? 0.0f : 1.0f;
            tri[tid][0] = make_float4(x0, y0, z0, keep);
            tri[tid][1] = make_float4(x1, y1, z1, 0.0f);
            tri[tid][2] = make_float4(x2, y2, z2, 0.0f);
        }
        __syncthreads();
        float sum[CONTAINS_PPL];
#pragma unroll
        for (int j = 0; j < CONTAINS_PPL; ++j) sum[j] = 0.0f;
        for (int t = 0; t < cn; ++t) {
            const float4 a = tri[t][0], b = tri[t][1], c = tri[t][2];   // every lane the same address: LDS broadcast
            if (a.w == 0.0f) continue;                                  // (the same for the whole workgroup)
#pragma unroll
            for (int j = 0; j < CONTAINS_PPL; ++j)
                sum[j] += half_solid_angle(a.x - px[j], a.y - py[j], a.z - pz[j], b.x - px[j], b.y - py[j], b.z - pz[j], c.x - px[j],
                                           c.y - py[j], c.z - pz[j]);
        }
        // a chunk's 256 terms in fp32, the chunks in double: the part's sum keeps fp32's per-term error, not 4096 roundings
#pragma unroll
        for (int j = 0; j < CONTAINS_PPL; ++j) acc[j] += (double)sum[j];
    }
#pragma unroll
    for (int j = 0; j < CONTAINS_PPL; ++j) {
        const int p = p0 + j * CONTAINS_THREADS + tid;
        if (p < n) partial[(size_t)part * n + p] = (float)acc[j];
    }
}

__global__ __launch_bounds__(256) void mesh_winding_reduce_kernel(const float *__restrict__ partial, int n, int parts,
                                                                   unsigned char *__restrict__ inside, float *__restrict__ winding) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double s = 0.0;
    for (int k = 0; k < parts; ++k) s += (double)partial[(size_t)k * n + p];
    const float w = (float)(s * 0.15915494309189535);   // 2 atan2 / (4 pi) = atan2 / (2 pi)
    inside[p] = fabsf(w) > 0.5f ? 1 : 0;
    if (winding) winding[p] = w;
}

// ---------------------------------------------------------------- area cdf
constexpr int CDF_THREADS = 1024;

__device__ inline double face_area(const float *__restrict__ verts, int nv, const int32_t *__restrict__ f) {
    const float *v0 = verts + (size_t)clamp_index(f[0], nv) * 3, *v1 = verts + (size_t)clamp_index(f[1], nv) * 3,
                *v2 = verts + (size_t)clamp_index(f[2], nv) * 3;
    const double ex = (double)v1[0] - (double)v0[0], ey = (double)v1[1] - (double)v0[1], ez = (double)v1[2] - (double)v0[2];
    const double gx = (double)v2[0] - (double)v0[0], gy = (double)v2[1] - (double)v0[1], gz = (double)v2[2] - (double)v0[2];
    const double nx = ey * gz - ez * gy, ny = ez * gx - ex * gz, nz = ex * gy - ey * gx;
    return 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
}

// One workgroup, CDF_THREADS faces per round, the rounds in order: inclusive scan inside the wave (shuffles), the wave totals
// through LDS, the running total carried in a register every thread holds.
__global__ __launch_bounds__(CDF_THREADS) void mesh_area_cdf_kernel(const float *__restrict__ verts, int nv,
                                                                     const int32_t *__restrict__ faces, int nf,
                                                                     double *__restrict__ cdf) {
    __shared__ double wave_total[CDF_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double carry = 0.0;
    for (int f0 = 0; f0 < nf; f0 += CDF_THREADS) {
        const int f = f0 + tid;
        double v = f < nf ? face_area(verts, nv, faces + (size_t)f * 3) : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double up = __shfl_up(v, d, 64);
            if (lane >= d) v += up;
        }
        __syncthreads();   // the previous round's totals have been read
        if (lane == 63) wave_total[wave] = v;
        __syncthreads();
        double before = carry, all = carry;
#pragma unroll
        for (int w = 0; w < CDF_THREADS / 64; ++w) {
            const double t = wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        if (f < nf) cdf[f] = before + v;
        carry = all;
    }
}

// ---------------------------------------------------------------- pool
struct PoolKeys {
    unsigned long long face, r1, r2, jitter_r, jitter_t, box, shuffle;
};
struct Box {
    float lo[3], hi[3];
};

__global__ __launch_bounds__(256) void mesh_sample_pool_kernel(const float *__restrict__ verts, int nv,
                                                                const int32_t *__restrict__ faces, int nf,
                                                                const double *__restrict__ cdf, PoolKeys keys, int n_surface,
                                                                int n_box, float sigma, Box box, float *__restrict__ points,
                                                                long long *__restrict__ sort_keys, int32_t *__restrict__ face_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_surface + n_box) return;
    // the shuffle is the order of these keys; the sign bit is flipped so that a signed 64-bit sort orders them as unsigned
    sort_keys[i] = (long long)(splitmix64(keys.shuffle + (unsigned long long)i) ^ 0x8000000000000000ull);
    float p[3];
    if (i < n_surface) {
        const double target = (double)uniform01(keys.face, i) * cdf[nf - 1];
        int lo = 0, hi = nf - 1;   // the first face whose cdf exceeds the target: a zero-area face is never chosen
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        if (face_out) face_out[i] = lo;
        const int32_t *f = faces + (size_t)lo * 3;
        const float *v0 = verts + (size_t)clamp_index(f[0], nv) * 3, *v1 = verts + (size_t)clamp_index(f[1], nv) * 3,
                    *v2 = verts + (size_t)clamp_index(f[2], nv) * 3;
        float r1 = uniform01(keys.r1, i), r2 = uniform01(keys.r2, i);
        if (r1 + r2 > 1.0f) r1 = 1.0f - r1, r2 = 1.0f - r2;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[c] = v0[c] + r1 * (v1[c] - v0[c]) + r2 * (v2[c] - v0[c]);
            if (sigma != 0.0f) {
                // Box-Muller; the logarithm's argument is (k + 1) / 2^24: never 0
                const unsigned long long k = 3ull * i + c;
                const float u = (float)(bits24(keys.jitter_r, k) + 1u) * (1.0f / 16777216.0f);
                const float z = sqrtf(-2.0f * logf(u)) * cosf(6.28318530717958647692f * uniform01(keys.jitter_t, k));
                p[c] += sigma * z;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            p[c] = box.lo[c] + uniform01(keys.box, 3ull * (i - n_surface) + c) * (box.hi[c] - box.lo[c]);
    }
    points[(size_t)i * 3 + 0] = p[0], points[(size_t)i * 3 + 1] = p[1], points[(size_t)i * 3 + 2] = p[2];
}

// ---------------------------------------------------------------- select
constexpr int SELECT_THREADS = SURS_SAMPLE_SELECT_CHUNK;
static_assert(SELECT_THREADS == 1024, "sixteen waves");

// counts of set flags among the workgroup's threads before this one, and in the whole workgroup (two flags at once)
__device__ __forceinline__ void block_ranks(bool a, bool b, int (*wsum)[2], int &rank_a, int &rank_b, int &total_a, int &total_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ma = __ballot(a), mb = __ballot(b), below = (1ull << lane) - 1ull;
    __syncthreads();   // the previous round's sums have been read
    if (lane == 0) wsum[wave][0] = __popcll(ma), wsum[wave][1] = __popcll(mb);
    __syncthreads();
    rank_a = __popcll(ma & below), rank_b = __popcll(mb & below), total_a = 0, total_b = 0;
#pragma unroll
    for (int w = 0; w < SELECT_THREADS / 64; ++w) {
        const int ta = wsum[w][0], tb = wsum[w][1];
        if (w < wave) rank_a += ta, rank_b += tb;
        total_a += ta, total_b += tb;
    }
}

__global__ __launch_bounds__(SELECT_THREADS) void sample_select_kernel(const float *__restrict__ pool, int ld, int n_pool,
                                                                         const unsigned char *__restrict__ in_hr,
                                                                         const unsigned char *__restrict__ in_lr, int n,
                                                                         float *__restrict__ samples_hr, float *__restrict__ labels_hr,
                                                                         float *__restrict__ samples_lr, float *__restrict__ labels_disp,
                                                                         int32_t *__restrict__ counts) {
    __shared__ int wsum[SELECT_THREADS / 64][2];
    const int tid = threadIdx.x, half = n / 2;
    // walk 1: how many points each mesh holds
    int nin_hr = 0, nin_lr = 0;
    for (int i0 = 0; i0 < n_pool; i0 += SELECT_THREADS) {
        const int i = i0 + tid;
        int ra, rb, ta, tb;
        block_ranks(i < n_pool && in_hr[i] != 0, i < n_pool && in_lr[i] != 0, wsum, ra, rb, ta, tb);
        nin_hr += ta, nin_lr += tb;
    }
    // the rule of the reference: more than N/2 inside -> N/2 of each; otherwise all inside, then N - nin outside
    const int nout_hr = n_pool - nin_hr, nout_lr = n_pool - nin_lr;
    const int sel_in_hr = nin_hr > half ? half : nin_hr, sel_out_hr = min(nin_hr > half ? half : n - nin_hr, nout_hr);
    const int sel_in_lr = nin_lr > half ? half : nin_lr, sel_out_lr = min(nin_lr > half ? half : n - nin_lr, nout_lr);
    // labels_disp: entry i of each half is rewritten for i < len(inside_LR) (and an outside point of that rank exists)
    const int disp_in = sel_in_lr, disp_out = min(sel_in_lr, sel_out_lr);
    // walk 2: stable compaction, inside first
    int seen_hr = 0, seen_lr = 0;
    for (int i0 = 0; i0 < n_pool; i0 += SELECT_THREADS) {
        const int i = i0 + tid;
        const bool live = i < n_pool, fh = live && in_hr[i] != 0, fl = live && in_lr[i] != 0;
        int ra, rb, ta, tb;
        block_ranks(fh, fl, wsum, ra, rb, ta, tb);
        if (live) {
            const float x = pool[(size_t)i * ld], y = pool[(size_t)i * ld + 1], z = pool[(size_t)i * ld + 2];
            const int r_hr = fh ? seen_hr + ra : i - (seen_hr + ra);   // rank among the inside / the outside points of HR
            const int col_hr = fh ? (r_hr < sel_in_hr ? r_hr : -1) : (r_hr < sel_out_hr ? sel_in_hr + r_hr : -1);
            if (col_hr >= 0) {
                samples_hr[col_hr] = x, samples_hr[n + col_hr] = y, samples_hr[2 * n + col_hr] = z;
                labels_hr[col_hr] = fh ? 1.0f : 0.0f;
            }
            const int r_lr = fl ? seen_lr + rb : i - (seen_lr + rb);
            const int col_lr = fl ? (r_lr < sel_in_lr ? r_lr : -1) : (r_lr < sel_out_lr ? sel_in_lr + r_lr : -1);
            if (col_lr >= 0) samples_lr[col_lr] = x, samples_lr[n + col_lr] = y, samples_lr[2 * n + col_lr] = z;
            // "inside_points_LR[i] in outside_points_HR" / "outside_points_LR[i] in inside_points_HR": the point's HR flag
            if (fl && r_lr < disp_in) labels_disp[r_lr] = fh ? 1.0f : 0.0f;
            if (!fl && r_lr < disp_out) labels_disp[half + r_lr] = fh ? 1.0f : 0.0f;
        }
        seen_hr += ta, seen_lr += tb;
    }
    // what the walk did not write: the untouched ones and zeros of labels_disp, and the columns behind a short selection
    for (int i = tid; i < half; i += SELECT_THREADS) {
        if (i >= disp_in) labels_disp[i] = 1.0f;
        if (i >= disp_out) labels_disp[half + i] = 0.0f;
    }
    for (int i = sel_in_hr + sel_out_hr + tid; i < n; i += SELECT_THREADS)
        samples_hr[i] = 0.0f, samples_hr[n + i] = 0.0f, samples_hr[2 * n + i] = 0.0f, labels_hr[i] = 0.0f;
    for (int i = sel_in_lr + sel_out_lr + tid; i < n; i += SELECT_THREADS)
        samples_lr[i] = 0.0f, samples_lr[n + i] = 0.0f, samples_lr[2 * n + i] = 0.0f;
    if (counts && tid == 0) counts[0] = sel_in_hr, counts[1] = sel_out_hr, counts[2] = sel_in_lr, counts[3] = sel_out_lr;
}

int mesh_args(const float *verts, int nv, const int32_t *faces, int nf) {
    SURS_REQUIRE(verts && faces, "verts and faces must not be NULL");
    SURS_REQUIRE(nv >= 1 && nf >= 1, "a mesh needs vertices and faces (nv %d, nf %d)", nv, nf);
    return 0;
}
}  // namespace

extern "C" int surs_mesh_contains_parts(int nf) { return nf < 1 ? 0 : surs::ceil_div(nf, CONTAINS_PART); }

extern "C" size_t surs_mesh_contains_workspace_bytes(int n, int nf) {
    if (n < 1 || nf < 1) return 0;
    return (size_t)surs_mesh_contains_parts(nf) * (size_t)n * sizeof(float);
}

extern "C" int surs_mesh_contains(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf,
                                  void *workspace, size_t workspace_bytes, unsigned char *inside, float *winding, void *stream) {
    if (int e = mesh_args(verts, nv, faces, nf)) return e;
    SURS_REQUIRE(n >= 0 && ld >= 3, "n %d must be >= 0 and ld %d >= 3", n, ld);
    if (n == 0) return 0;
    SURS_REQUIRE(points && inside, "points and inside must not be NULL");
    const size_t need = surs_mesh_contains_workspace_bytes(n, nf);
    SURS_REQUIRE(workspace && workspace_bytes >= need, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int parts = surs_mesh_contains_parts(nf);
    SURS_REQUIRE(parts <= 65535, "%d faces make %d face parts; a launch takes 65535", nf, parts);
    hipStream_t st = as_stream(stream);
    float *partial = (float *)workspace;
    hipLaunchKernelGGL(mesh_winding_parts_kernel, dim3(ceil_div(n, CONTAINS_TILE), parts), dim3(CONTAINS_THREADS), 0, st, points, n, ld,
                       verts, nv, faces, nf, partial);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mesh_winding_reduce_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, partial, n, parts, inside, winding);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_mesh_area_cdf(const float *verts, int nv, const int32_t *faces, int nf, double *cdf, void *stream) {
    if (int e = mesh_args(verts, nv, faces, nf)) return e;
    SURS_REQUIRE(cdf, "cdf must not be NULL");
    hipLaunchKernelGGL(mesh_area_cdf_kernel, dim3(1), dim3(CDF_THREADS), 0, as_stream(stream), verts, nv, faces, nf, cdf);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_mesh_sample_pool(const float *verts, int nv, const int32_t *faces, int nf, const double *cdf,
                                     unsigned long long seed, int n_surface, int n_box, float sigma, const float *b_min,
                                     const float *b_max, float *points, long long *sort_keys, int32_t *face_index, void *stream) {
    if (int e = mesh_args(verts, nv, faces, nf)) return e;
    SURS_REQUIRE(n_surface >= 0 && n_box >= 0 && (long long)n_surface + n_box < (1ll << 30), "n_surface %d, n_box %d", n_surface, n_box);
    if (n_surface + n_box == 0) return 0;
    SURS_REQUIRE(cdf && points && sort_keys && b_min && b_max, "cdf, points, sort_keys, b_min and b_max must not be NULL");
    PoolKeys k;
    k.face = stream_key("train_samples_face", seed);
    k.r1 = stream_key("train_samples_r1", seed);
    k.r2 = stream_key("train_samples_r2", seed);
    k.jitter_r = stream_key("train_samples_jitter_radius", seed);
    k.jitter_t = stream_key("train_samples_jitter_angle", seed);
    k.box = stream_key("train_samples_box", seed);
    k.shuffle = stream_key("train_samples_shuffle", seed);
    Box box;
    for (int c = 0; c < 3; ++c) box.lo[c] = b_min[c], box.hi[c] = b_max[c];
    hipLaunchKernelGGL(mesh_sample_pool_kernel, dim3(ceil_div(n_surface + n_box, 256)), dim3(256), 0, as_stream(stream), verts, nv, faces,
                       nf, cdf, k, n_surface, n_box, sigma, box, points, sort_keys, face_index);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_sample_select(const float *pool, int ld, int n_pool, const unsigned char *inside_hr, const unsigned char *inside_lr,
                                  int n, float *samples_hr, float *labels_hr, float *samples_lr, float *labels_disp, int32_t *counts,
                                  void *stream) {
    SURS_REQUIRE(n >= 2 && n % 2 == 0, "num_sample_inout %d must be even (labels_disp is two halves of N / 2)", n);
    SURS_REQUIRE(n_pool >= 0 && ld >= 3, "n_pool %d must be >= 0 and ld %d >= 3", n_pool, ld);
    SURS_REQUIRE((n_pool == 0 || (pool && inside_hr && inside_lr)) && samples_hr && labels_hr && samples_lr && labels_disp,
                 "pool, flags and outputs must not be NULL");
    hipLaunchKernelGGL(sample_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, as_stream(stream), pool, ld, n_pool, inside_hr, inside_lr, n,
                       samples_hr, labels_hr, samples_lr, labels_disp, counts);
    SURS_LAUNCH_CHECK();
    return 0;
}
