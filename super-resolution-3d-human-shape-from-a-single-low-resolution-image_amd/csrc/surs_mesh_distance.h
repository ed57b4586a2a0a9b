// The point-triangle distance of the mesh metrics (include/surs.h "mesh distance"), ONCE for host and device: the kernel of
// surs_mesh_distance.hip calls md_dist2 once per (point, triangle) pair on records that md_prepare built when the triangle was
// staged in LDS, surs_mesh_distance_host loops the same two functions on the host.  __host__ __device__, so both compile the same
// arithmetic; the library builds with -ffp-contract=off and fp32 division and square root are correctly rounded on both sides, so
// every operation below is one IEEE rounding and host and device give the same bits.  The fused multiply-adds are EXPLICIT (md_fma);
// minima and clamps are selects written out (fminf / fmaxf may return either zero of a (-0, +0) pair).
//
// The formula is tests/mesh_ref.py::surface_distance's: the minimum over the three edges of |x - clamp(s, 0, 1) e|^2, x the point seen
// from the edge's first vertex, s = x.e / e.e; replaced by (ap.n)^2 / n.n where the triangle has an area and the projection onto its
// plane falls inside.  No squared lengths are subtracted anywhere.  All DIVISIONS are in md_prepare, once per triangle: md_dist2 has
// none, and no branch (selects only).
//   * Each edge is measured from its own first vertex (ab from a, bc from b, ca from c), and bp = ap - ab, cp = ap - ac are formed
//     from the very differences the record holds: at a vertex the point's offset is exactly zero, s = 0 and the distance is exactly 0.
//   * The three plane products (ap.n and the barycentric coordinates ap.mb, ap.mc) are plain products and sums, not fused: where the
//     terms of such a sum cancel by symmetry (a point on an axis-aligned face, on the diagonal of a square) the rounded products
//     cancel exactly too, and the point gets exactly 0 from BOTH triangles of the pair - the tie then goes to the lower face index.
//   * A triangle is "flat" where n.n is 0 (or so small or so large that n.n or its reciprocal leaves fp32's range): it is its three
//     segments.  An edge of length 0 has inv 0: s = 0, the segment is its first vertex; a repeated vertex is a point.  A NaN s (0 x inf)
//     is clamped to 0.  The result is finite for finite input whose squared distances fp32 can hold.
//   * A point with a NaN or infinite coordinate gets NaN or +inf from every triangle: never below the running minimum.
#pragma once
#include "../../include/surs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SURS_MD_HD __host__ __device__
#else
#define SURS_MD_HD
#endif

namespace surs {

// 7 x 16 bytes, read as seven float4 (every lane the same address: LDS broadcast)
struct MdRecord {
    float ax, ay, az, inv_nn;        // vertex a;            1 / n.n (0: flat)
    float abx, aby, abz, inv_ab;     // b - a;               1 / |ab|^2 (0: a == b)
    float acx, acy, acz, inv_ca;     // c - a;               1 / |ca|^2
    float bcx, bcy, bcz, inv_bc;     // c - b;               1 / |bc|^2
    float nx, ny, nz, keep;          // n = ab x ac;         keep = 1 where the plane term may replace the edges, 0 for a flat triangle
    float mbx, mby, mbz, pad0;       // (ac x n) / n.n:      wb = ap.mb
    float mcx, mcy, mcz, pad1;       // (n x ab) / n.n:      wc = ap.mc
};
static_assert(sizeof(MdRecord) == 7 * 16, "seven float4");

SURS_MD_HD inline float md_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }   // a b + c, one rounding
SURS_MD_HD inline float md_sqrt(float x) { return __builtin_sqrtf(x); }

SURS_MD_HD inline float md_inv_len2(float x, float y, float z) {
    const float l = md_fma(z, z, md_fma(y, y, x * x));
    const float inv = 1.0f / l;
    return (l > 0.0f && inv <= 3.402823466e+38f) ? inv : 0.0f;
}

SURS_MD_HD inline MdRecord md_prepare(const float *v0, const float *v1, const float *v2) {
    MdRecord r;
    r.ax = v0[0], r.ay = v0[1], r.az = v0[2];
    r.abx = v1[0] - v0[0], r.aby = v1[1] - v0[1], r.abz = v1[2] - v0[2];
    r.acx = v2[0] - v0[0], r.acy = v2[1] - v0[1], r.acz = v2[2] - v0[2];
    r.bcx = v2[0] - v1[0], r.bcy = v2[1] - v1[1], r.bcz = v2[2] - v1[2];
    r.inv_ab = md_inv_len2(r.abx, r.aby, r.abz);
    r.inv_bc = md_inv_len2(r.bcx, r.bcy, r.bcz);
    r.inv_ca = md_inv_len2(r.acx, r.acy, r.acz);
    r.nx = r.aby * r.acz - r.abz * r.acy, r.ny = r.abz * r.acx - r.abx * r.acz, r.nz = r.abx * r.acy - r.aby * r.acx;
    const float nn = r.nx * r.nx + r.ny * r.ny + r.nz * r.nz;
    const float inv = 1.0f / nn;
    const bool ok = nn > 0.0f && nn <= 3.402823466e+38f && inv <= 3.402823466e+38f;
    const float den = ok ? nn : 1.0f;
    r.inv_nn = ok ? inv : 0.0f;
    r.keep = ok ? 1.0f : 0.0f;
    r.mbx = (r.acy * r.nz - r.acz * r.ny) / den, r.mby = (r.acz * r.nx - r.acx * r.nz) / den, r.mbz = (r.acx * r.ny - r.acy * r.nx) / den;
    r.mcx = (r.ny * r.abz - r.nz * r.aby) / den, r.mcy = (r.nz * r.abx - r.nx * r.abz) / den, r.mcz = (r.nx * r.aby - r.ny * r.abx) / den;
    r.pad0 = r.pad1 = 0.0f;
    return r;
}

// |x - clamp(s, 0, 1) e|^2, s = (x.e) inv: 11 operations
SURS_MD_HD inline float md_segment(float x, float y, float z, float ex, float ey, float ez, float inv) {
    float s = md_fma(z, ez, md_fma(y, ey, x * ex)) * inv;
    s = s > 0.0f ? s : 0.0f;     // a NaN becomes 0
    s = s < 1.0f ? s : 1.0f;
    const float dx = md_fma(-s, ex, x), dy = md_fma(-s, ey, y), dz = md_fma(-s, ez, z);
    return md_fma(dz, dz, md_fma(dy, dy, dx * dx));
}

// squared distance from p to the record's triangle
SURS_MD_HD inline float md_dist2(float px, float py, float pz, const MdRecord &r) {
    const float apx = px - r.ax, apy = py - r.ay, apz = pz - r.az;
    const float bpx = apx - r.abx, bpy = apy - r.aby, bpz = apz - r.abz;
    const float cpx = apx - r.acx, cpy = apy - r.acy, cpz = apz - r.acz;
    const float d_ab = md_segment(apx, apy, apz, r.abx, r.aby, r.abz, r.inv_ab);
    const float d_bc = md_segment(bpx, bpy, bpz, r.bcx, r.bcy, r.bcz, r.inv_bc);
    const float d_ca = md_segment(cpx, cpy, cpz, -r.acx, -r.acy, -r.acz, r.inv_ca);
    float d2 = d_ab;
    d2 = d_bc < d2 ? d_bc : d2;
    d2 = d_ca < d2 ? d_ca : d2;
    const float t = apx * r.nx + apy * r.ny + apz * r.nz;
    const float wb = apx * r.mbx + apy * r.mby + apz * r.mbz;
    const float wc = apx * r.mcx + apy * r.mcy + apz * r.mcz;
    const bool inside = (r.keep != 0.0f) & (wb >= 0.0f) & (wc >= 0.0f) & (wb + wc <= 1.0f);
    const float plane = t * t * r.inv_nn;
    return inside ? plane : d2;
}

}  // namespace surs
