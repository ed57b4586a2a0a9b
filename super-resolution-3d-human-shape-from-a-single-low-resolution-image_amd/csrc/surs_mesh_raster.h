// The triangle rasteriser of the normal reprojection error (include/surs.h "mesh raster"), ONCE for host and device: the kernels of
// surs_mesh_raster.hip call mr_prepare once per triangle and mr_cover once per (pixel, triangle) pair, surs_mesh_raster_host loops the
// same two functions on the host, and mr_shade turns a pixel's winning face into its normal on both sides.  __host__ __device__; the
// library builds with -ffp-contract=off and fp32 division and square root are correctly rounded on both sides, so every operation
// below is one IEEE rounding and host and device give the same bits.  No fused multiply-add anywhere: products and sums as written.
//
//   * View.  M is a row-major 3 x 4 matrix, (x', y', z') = M (x, y, z, 1): orthographic, x', y' in [-1, 1] over the image, y' grows
//     DOWNWARDS, the camera looks from the +z' side: of two surfaces over a pixel the one with the LARGER z' is seen.
//   * Pixel units.  sx = (x' + 1) (w / 2) - 1/2, sy = (y' + 1) (h / 2) - 1/2: pixel (i, j) is sampled at its centre x' = (2j + 1) / w
//     - 1, y' = (2i + 1) / h - 1, which is (sx, sy) = (j, i) - an integer, exact in fp32.
//   * Record.  Every division is in mr_prepare.  The three barycentric coordinates are three edge functions, each measured from a
//     vertex of ITS OWN edge (b1 and b2 from vertex 0, b0 from vertex 1) and scaled by 1 / (signed projected area): the sign of each
//     is the sign of its own cross product whatever the rounding of the area, and a pixel centre on a vertex gets an exact 0.  The
//     area's sign is in the scale, so either winding is accepted and nothing is culled.  z' is the plane z0 + b1 dz1 + b2 dz2.
//   * Box.  The integer pixels [ceil(min), floor(max)] of the projected vertices, clamped to the image.  A triangle with zero
//     projected area, a non-finite coordinate, an area whose reciprocal leaves fp32's range or a box off the image is FLAGGED
//     (ok = 0) and gets the empty box (MR_EMPTY_MIN, -1): it covers nothing.
//   * Cover.  A pixel is covered where it lies in the box and b0, b1, b2 >= 0 (edges inclusive); selects only, no branch.  The box
//     is part of the test, so a pixel's answer does not depend on who enumerates the pixels (a tile of the kernel, the box loop of
//     the host) nor on the image it sits in.
//   * Vertex order.  The callers hand a triangle's vertices over in ASCENDING INDEX order (mr_sort3), whatever order the face lists
//     them in: a mesh and its copy with every face turned round give the same bits, and (b1, b2) are the weights of the vertex with
//     the middle and with the largest index.
//   * Winner.  The largest z', the LOWEST face index among equals: a strict > over the faces in order (mr_better).
#pragma once
#include "../../include/surs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SURS_MR_HD __host__ __device__
#else
#define SURS_MR_HD
#endif

namespace surs {

constexpr int MR_EMPTY_MIN = 1 << 30;   // the empty box: [MR_EMPTY_MIN, -1] in x and y

struct MrBox {
    int32_t xmin, xmax, ymin, ymax;
};
static_assert(sizeof(MrBox) == 16, "one int4");

// 5 x 16 bytes, read as five float4 (every lane the same address: LDS broadcast)
struct MrRecord {
    float x0, y0, x1, y1;      // vertices 0 and 1 in pixel units
    float a1, c1, a2, c2;      // b1 = a1 qx + c1 qy, b2 = a2 qx + c2 qy, q = pixel - vertex 0
    float a0, c0, z0, dz1;     // b0 = a0 rx + c0 ry, r = pixel - vertex 1;  z' = z0 + b1 dz1 + b2 dz2
    float dz2, ok, pad0, pad1; // ok = 1 where the triangle can cover a pixel, 0 where it is flagged
    MrBox box;
};
static_assert(sizeof(MrRecord) == 5 * 16, "five float4");

// a face's three vertex indices in ascending order
SURS_MR_HD inline void mr_sort3(int &a, int &b, int &c) {
    int t;
    if (b < a) t = a, a = b, b = t;
    if (c < b) t = b, b = c, c = t;
    if (b < a) t = a, a = b, b = t;
}

SURS_MR_HD inline bool mr_finite(float x) { return x - x == 0.0f; }
SURS_MR_HD inline float mr_min3(float a, float b, float c) {
    float m = b < a ? b : a;
    return c < m ? c : m;
}
SURS_MR_HD inline float mr_max3(float a, float b, float c) {
    float m = b > a ? b : a;
    return c > m ? c : m;
}

// one row of M applied to a vertex: ((m0 x + m1 y) + m2 z) + m3
SURS_MR_HD inline float mr_row(const float *m, const float *v) { return ((m[0] * v[0] + m[1] * v[1]) + m[2] * v[2]) + m[3]; }

SURS_MR_HD inline void mr_project(const float *v, const float *M, float *out) {
    out[0] = mr_row(M, v), out[1] = mr_row(M + 4, v), out[2] = mr_row(M + 8, v);
}

SURS_MR_HD inline MrRecord mr_prepare(const float *v0, const float *v1, const float *v2, const float *M, int w, int h) {
    MrRecord r;
    float p0[3], p1[3], p2[3];
    mr_project(v0, M, p0), mr_project(v1, M, p1), mr_project(v2, M, p2);
    const float hw = 0.5f * (float)w, hh = 0.5f * (float)h;
    const float x0 = (p0[0] + 1.0f) * hw - 0.5f, y0 = (p0[1] + 1.0f) * hh - 0.5f;
    const float x1 = (p1[0] + 1.0f) * hw - 0.5f, y1 = (p1[1] + 1.0f) * hh - 0.5f;
    const float x2 = (p2[0] + 1.0f) * hw - 0.5f, y2 = (p2[1] + 1.0f) * hh - 0.5f;
    const float d1x = x1 - x0, d1y = y1 - y0, d2x = x2 - x0, d2y = y2 - y0, ex = x2 - x1, ey = y2 - y1;
    const float area = d1x * d2y - d1y * d2x;
    const float inv = 1.0f / area;
    const float lo_x = __builtin_ceilf(mr_min3(x0, x1, x2)), hi_x = __builtin_floorf(mr_max3(x0, x1, x2));
    const float lo_y = __builtin_ceilf(mr_min3(y0, y1, y2)), hi_y = __builtin_floorf(mr_max3(y0, y1, y2));
    const float bx0 = lo_x > 0.0f ? lo_x : 0.0f, bx1 = hi_x < (float)(w - 1) ? hi_x : (float)(w - 1);
    const float by0 = lo_y > 0.0f ? lo_y : 0.0f, by1 = hi_y < (float)(h - 1) ? hi_y : (float)(h - 1);
    // (a sum is finite only where every term is)
    const bool finite = mr_finite((((((((x0 + y0) + x1) + y1) + x2) + y2) + p0[2]) + p1[2]) + p2[2]);
    const bool ok = finite && area != 0.0f && mr_finite(inv) && bx0 <= bx1 && by0 <= by1;
    const float s = ok ? inv : 0.0f;
    r.x0 = x0, r.y0 = y0, r.x1 = x1, r.y1 = y1;
    r.a1 = d2y * s, r.c1 = -d2x * s;
    r.a2 = -d1y * s, r.c2 = d1x * s;
    r.a0 = -ey * s, r.c0 = ex * s;
    r.z0 = ok ? p0[2] : 0.0f, r.dz1 = ok ? p1[2] - p0[2] : 0.0f, r.dz2 = ok ? p2[2] - p0[2] : 0.0f;
    r.ok = ok ? 1.0f : 0.0f, r.pad0 = r.pad1 = 0.0f;
    if (!ok) r.x0 = r.y0 = r.x1 = r.y1 = 0.0f;
    r.box.xmin = ok ? (int32_t)bx0 : MR_EMPTY_MIN, r.box.xmax = ok ? (int32_t)bx1 : -1;
    r.box.ymin = ok ? (int32_t)by0 : MR_EMPTY_MIN, r.box.ymax = ok ? (int32_t)by1 : -1;
    return r;
}

// is pixel (px, py) - column, row - covered?  b1, b2 and z are the pair's values whether it is or not.
SURS_MR_HD inline bool mr_cover(int px, int py, const MrRecord &r, float *b1, float *b2, float *z) {
    const float fx = (float)px, fy = (float)py;
    const float qx = fx - r.x0, qy = fy - r.y0, rx = fx - r.x1, ry = fy - r.y1;
    const float w1 = qx * r.a1 + qy * r.c1;
    const float w2 = qx * r.a2 + qy * r.c2;
    const float w0 = rx * r.a0 + ry * r.c0;
    *b1 = w1, *b2 = w2;
    *z = (r.z0 + w1 * r.dz1) + w2 * r.dz2;
    return (px >= r.box.xmin) & (px <= r.box.xmax) & (py >= r.box.ymin) & (py <= r.box.ymax) & (w0 >= 0.0f) & (w1 >= 0.0f) &
           (w2 >= 0.0f);
}

// the winner rule: does a covered pair (z) displace the running best?  Faces are offered in index order, so a strict > keeps the
// lowest index of a tie; a NaN z never wins.
SURS_MR_HD inline bool mr_better(bool covered, float z, float best) { return covered & (z > best); }

// a vector scaled to unit length and turned to face the camera (z' >= 0); (0, 0, 1) where it has no length
SURS_MR_HD inline void mr_unit_facing(float nx, float ny, float nz, float *out) {
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float l = __builtin_sqrtf(nn);
    const bool has = (l > 0.0f) & mr_finite(l);
    const float d = has ? l : 1.0f;
    float ux = nx / d, uy = ny / d, uz = nz / d;
    const bool flip = uz < 0.0f;
    ux = flip ? -ux : ux, uy = flip ? -uy : uy, uz = flip ? -uz : uz;
    out[0] = has ? ux : 0.0f, out[1] = has ? uy : 0.0f, out[2] = has ? uz : 1.0f;
}

// The colour 0.5 n + 0.5 of a pixel won by the triangle (v0, v1, v2) at barycentrics (b1, b2).  Flat (vn0 == nullptr): n is the
// cross product of the projected edges (x', y', z').  Smooth: n = N ((1 - b1 - b2) vn0 + b1 vn1 + b2 vn2), N the row-major 3 x 3
// normal matrix.
SURS_MR_HD inline void mr_shade(const float *v0, const float *v1, const float *v2, const float *M, const float *vn0, const float *vn1,
                                const float *vn2, const float *N, float b1, float b2, float *rgb) {
    float n[3];
    if (vn0 == nullptr) {
        float p0[3], p1[3], p2[3];
        mr_project(v0, M, p0), mr_project(v1, M, p1), mr_project(v2, M, p2);
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        mr_unit_facing(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, n);
    } else {
        const float b0 = (1.0f - b1) - b2;
        const float mx = (b0 * vn0[0] + b1 * vn1[0]) + b2 * vn2[0];
        const float my = (b0 * vn0[1] + b1 * vn1[1]) + b2 * vn2[1];
        const float mz = (b0 * vn0[2] + b1 * vn1[2]) + b2 * vn2[2];
        mr_unit_facing((N[0] * mx + N[1] * my) + N[2] * mz, (N[3] * mx + N[4] * my) + N[5] * mz, (N[6] * mx + N[7] * my) + N[8] * mz, n);
    }
    rgb[0] = 0.5f * n[0] + 0.5f, rgb[1] = 0.5f * n[1] + 0.5f, rgb[2] = 0.5f * n[2] + 0.5f;
}

}  // namespace surs
