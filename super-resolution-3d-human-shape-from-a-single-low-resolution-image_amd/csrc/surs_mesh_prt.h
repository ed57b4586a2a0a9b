// Per-vertex precomputed radiance transfer (include/surs.h "mesh PRT"), ONCE for host and device: the kernels of surs_mesh_prt.hip
// call prt_prepare once per triangle of a chunk and prt_hit once per (ray, triangle) pair, surs_mesh_prt_host loops the same
// functions, and prt_term / prt_finish turn a vertex's visibility bits into its nine coefficients on both sides.  __host__ __device__;
// the library builds with -ffp-contract=off, so every operation below is one IEEE rounding and host and device give the same bits.
// No fused multiply-add anywhere: products and sums as written.
//
//   * Definition.  prt[v][i] = (4 pi / D) sum_k V(v, d_k) max(0, n . d_k) Y_i(d_k), k = 0 .. D - 1 in index order, one fp32 accumulator
//     per coefficient; a term with n . d_k <= 0 is skipped, the scale 12.566371f / (float)D is applied once, at the end.
//   * Basis.  prt_sh9: bands 0 - 2 of the real spherical harmonics in the order l (l + 1) + m.
//   * Ray.  origin = v + offset n (component by component: one product, one sum), direction d_k as given (not normalised again).
//   * Triangle.  Moeller - Trumbore without the division: with s the sign of det = e1 . (d x e2), the pair hits where |det| > 0,
//     s u >= 0, s v >= 0, s (u + v) <= |det| (edges inclusive) and s t > 0.  A triangle with a zero (e1 x e2) or a non-finite
//     coordinate is prepared as e1 = e2 = 0: its det is an exact 0 for every ray and it hits nothing.
//   * Own faces.  A triangle that lists the ray's vertex as a corner - compared by INDEX - is skipped.
//   * A vertex whose position or normal is not finite gets prt = 0.
//   * Any-hit: V is a boolean OR over the triangles, free of order, so the loops may stop at the first hit.
#pragma once
#include "../../include/surs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SURS_PRT_HD __host__ __device__
#else
#define SURS_PRT_HD
#endif

namespace surs {

constexpr int PRT_CHUNK = SURS_MESH_PRT_CHUNK;   // triangles staged in LDS at a time: 3 x 16 bytes each, 24 KiB

// 3 x 16 bytes, read as three float4 (every lane the same address: LDS broadcast)
struct PrtTri {
    float ax, ay, az, e1x;
    float e1y, e1z, e2x, e2y;
    float e2z;
    int32_t i0, i1, i2;   // the corners' vertex indices (clamped to [0, nv))
};
static_assert(sizeof(PrtTri) == 3 * 16, "three float4");

SURS_PRT_HD inline bool prt_finite(float x) { return x - x == 0.0f; }

SURS_PRT_HD inline void prt_sh9(float x, float y, float z, float *Y) {
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y, Y[2] = 0.488603f * z, Y[3] = 0.488603f * x;
    Y[4] = 1.092548f * (x * y), Y[5] = 1.092548f * (y * z), Y[6] = 0.315392f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.092548f * (x * z), Y[8] = 0.546274f * (x * x - y * y);
}

SURS_PRT_HD inline float prt_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

SURS_PRT_HD inline PrtTri prt_prepare(const float *a, const float *b, const float *c, int i0, int i1, int i2) {
    PrtTri t;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    // (a sum is finite only where every term is)
    const bool finite = prt_finite(((((((((a[0] + a[1]) + a[2]) + e1x) + e1y) + e1z) + e2x) + e2y) + e2z) + ((nx + ny) + nz));
    const bool ok = finite && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
    t.ax = ok ? a[0] : 0.0f, t.ay = ok ? a[1] : 0.0f, t.az = ok ? a[2] : 0.0f;
    t.e1x = ok ? e1x : 0.0f, t.e1y = ok ? e1y : 0.0f, t.e1z = ok ? e1z : 0.0f;
    t.e2x = ok ? e2x : 0.0f, t.e2y = ok ? e2y : 0.0f, t.e2z = ok ? e2z : 0.0f;
    t.i0 = i0, t.i1 = i1, t.i2 = i2;
    return t;
}

// does the ray (o, d) of vertex `self` hit the triangle at t > 0?  Selects only, no branch.
SURS_PRT_HD inline bool prt_hit(const float *o, const float *d, int self, const PrtTri &t) {
    const float px = d[1] * t.e2z - d[2] * t.e2y, py = d[2] * t.e2x - d[0] * t.e2z, pz = d[0] * t.e2y - d[1] * t.e2x;
    const float det = (t.e1x * px + t.e1y * py) + t.e1z * pz;
    const float sx = o[0] - t.ax, sy = o[1] - t.ay, sz = o[2] - t.az;
    const float u = (sx * px + sy * py) + sz * pz;
    const float qx = sy * t.e1z - sz * t.e1y, qy = sz * t.e1x - sx * t.e1z, qz = sx * t.e1y - sy * t.e1x;
    const float v = (d[0] * qx + d[1] * qy) + d[2] * qz;
    const float w = (t.e2x * qx + t.e2y * qy) + t.e2z * qz;
    const bool neg = det < 0.0f;
    const float ad = neg ? -det : det, su = neg ? -u : u, sv = neg ? -v : v, sw = neg ? -w : w;
    const bool own = (self == t.i0) | (self == t.i1) | (self == t.i2);
    return (!own) & (ad > 0.0f) & (su >= 0.0f) & (sv >= 0.0f) & (su + sv <= ad) & (sw > 0.0f);
}

// a vertex's ray set-up: is the vertex usable at all (finite position and normal)?  origin = v + offset n.
SURS_PRT_HD inline bool prt_origin(const float *v, const float *n, float offset, float *o) {
    o[0] = v[0] + offset * n[0], o[1] = v[1] + offset * n[1], o[2] = v[2] + offset * n[2];
    return prt_finite((((((o[0] + o[1]) + o[2]) + n[0]) + n[1]) + n[2]));
}

// n . d_k of a usable vertex; the pair casts a ray (and can contribute) only where it is > 0
SURS_PRT_HD inline float prt_cosine(const float *n, const float *d) { return prt_dot(n, d); }

// one visible direction's term added to the nine accumulators
SURS_PRT_HD inline void prt_term(float cosine, const float *d, float *acc) {
    float Y[9];
    prt_sh9(d[0], d[1], d[2], Y);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 9; ++i) acc[i] = acc[i] + cosine * Y[i];
}

SURS_PRT_HD inline float prt_scale(int D) { return 12.566371f / (float)D; }

}  // namespace surs
