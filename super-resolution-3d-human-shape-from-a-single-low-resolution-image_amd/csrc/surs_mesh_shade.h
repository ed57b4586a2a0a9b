// Colour shading of a rastered view (include/surs.h "mesh shading"), ONCE for host and device: the kernels of surs_mesh_shade.hip run
// sh_pixel once per pixel and sh_resolve once per resolved pixel, the _host entries loop the same functions.  __host__ __device__; the
// library builds with -ffp-contract=off, fp32 division is correctly rounded on both sides, and NOTHING here calls a math library:
// log2, exp2 and so the gamma are the short fp32 polynomials below (sh_log2, sh_exp2), because powf and log2f of the host's and the
// device's libraries do not round alike.  Host and device give the same bits.
//
//   * Corners.  The raster's: a face's three vertices in ASCENDING INDEX order (mr_sort3), (b1, b2) the weights of the middle and the
//     largest index, b0 = (1 - b1) - b2.  faces_uv is given in the FACE's own corner order, as the OBJ lists it; sh_pixel carries each
//     corner's UV index through the same sort, so the caller permutes nothing.
//   * UV.  uv = (b0 uv0 + b1 uv1) + b2 uv2.  A non-finite uv is taken as 0.
//   * Pyramid.  Four levels, packed one after the other (sh_level_offset): level 0 is u8 / 255, each further level the 2 x 2 mean
//     ((a + b) + (c + d)) / 4 of the level above.  Rows as in the image file: row 0 is the TOP of the image.
//   * Lookup.  x = u W - 1/2, y = (1 - v) H - 1/2 (texel centres at (i + 1/2) / size; v = 0 is the LAST row, the OBJ convention), both
//     clamped to [-1, size]; bilinear between floor and floor + 1, indices clamped to the edge; then a linear blend between levels
//     l and l + 1.
//   * Mip level.  Constant per face: lambda = clamp(1/2 log2(A_tex / A_pix), 0, 3), A_tex the face's UV area in level-0 texels, A_pix
//     its projected area in pixels of this raster (the halves cancel).  l = floor(lambda); a ratio that is no number above 1 gives
//     level 0, a ratio >= 64 level 3.
//   * Transfer.  With prt: p_i = (b0 prt0_i + b1 prt1_i) + b2 prt2_i, and `light` is in prt's frame (the mesh's).  Without: the
//     blend of the three vertex normals, turned by the row-major 3 x 3 normal_matrix and scaled to unit length ((0, 0, 1) where it has
//     none), gives p_i = A_l Y_i(n), A = (pi, 2 pi / 3, pi / 4): the unshadowed limit of surs_mesh_prt; `light` is then in the frame the
//     matrix turns into.
//   * Colour.  s_c = fma(p_i, light[i][c], s_c) for i = 0 .. 8 from s_c = 0; g_c = sh_gamma(s_c) = max(s_c, 0) ^ (1 / 2.2);
//     rgb_c = clamp(albedo_c g_c, 0, 1); a = 1.  Background (face < 0): (0, 0, 0, 0).
//   * Resolve.  The m x m sub-samples of a pixel are added in row-major order in fp32, divided by m m, multiplied by 255 and rounded
//     to nearest, ties to even; mask is the alpha channel's byte.
#pragma once
#include "surs_mesh_prt.h"
#include "surs_mesh_raster.h"

namespace surs {

constexpr int SH_LEVELS = 4;
constexpr int SH_MAX_TEX = 16384;

struct ShadeArgs {
    const float *verts;
    const int32_t *faces;
    int nv, nf;
    const int32_t *faces_uv;   // nullable with pyramid
    const float *uvs;          // nullable with pyramid
    int nuv;
    const float *prt;          // [nv][9] or NULL
    const float *normals;      // [nv][3], read where prt is NULL
    const float *pyramid;      // packed levels or NULL
    int tw, th, w, h;
    float view[12], nm[9], light[27];
};

union ShWord {
    float f;
    uint32_t u;
};
SURS_MR_HD inline uint32_t sh_bits(float x) {
    ShWord w;
    w.f = x;
    return w.u;
}
SURS_MR_HD inline float sh_float(uint32_t b) {
    ShWord w;
    w.u = b;
    return w.f;
}

// floats before level l of the packed pyramid of a w x h texture
SURS_MR_HD inline size_t sh_level_offset(int w, int h, int l) {
    size_t off = 0;
    for (int i = 0; i < l; ++i) off += (size_t)3 * (size_t)(w >> i) * (size_t)(h >> i);
    return off;
}

// log2 of a normal, positive, finite x: x = 2^e m, m in (sqrt(1/2), sqrt(2)], log2 m = (2 / ln 2) atanh z, z = (m - 1) / (m + 1),
// |z| <= 0.1716, atanh by its series up to z^9 (the next term is below 4e-10).
SURS_MR_HD inline float sh_log2(float x) {
    const uint32_t b = sh_bits(x);
    int e = (int)(b >> 23) - 127;
    float m = sh_float((b & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421354f) m = m * 0.5f, e += 1;
    const float z = (m - 1.0f) / (m + 1.0f), z2 = z * z;
    const float p = (((0.111111112f * z2 + 0.142857149f) * z2 + 0.2f) * z2 + 0.333333343f) * z2 + 1.0f;
    return (float)e + 2.88539004f * (z * p);
}

// 2^y, y clamped to [-126, 126]: y = n + f, |f| <= 1/2, 2^f = exp(f ln 2) by its series up to the sixth power (the next term is
// below 1.3e-7 of the value), times 2^n built from its exponent bits.
SURS_MR_HD inline float sh_exp2(float y) {
    y = y < -126.0f ? -126.0f : (y > 126.0f ? 126.0f : y);
    const float n = __builtin_floorf(y + 0.5f);
    const float t = (y - n) * 0.693147182f;
    const float p = (((((0.00138888892f * t + 0.00833333377f) * t + 0.0416666679f) * t + 0.166666672f) * t + 0.5f) * t + 1.0f) * t + 1.0f;
    return p * sh_float((uint32_t)((int)n + 127) << 23);
}

// max(s, 0) ^ (1 / 2.2); 0 for anything that is not above 1e-30 (NaN included), values above 1e30 taken as 1e30
SURS_MR_HD inline float sh_gamma(float s) {
    if (!(s > 1e-30f)) return 0.0f;
    s = s > 1e30f ? 1e30f : s;
    return sh_exp2(sh_log2(s) * 0.454545468f);
}

// the face's mip level l in 0 .. 3 and the weight of level l + 1 (0 at l = 3) from the two areas
SURS_MR_HD inline void sh_mip(float a_tex, float a_pix, int *level, float *frac) {
    const float r = a_tex / a_pix;
    *level = 0, *frac = 0.0f;
    if (!(r > 1.0f)) return;
    if (r >= 64.0f) {
        *level = 3;
        return;
    }
    const float lambda = 0.5f * sh_log2(r);
    const float l = __builtin_floorf(lambda);
    const int li = (int)l;
    *level = li < 0 ? 0 : (li > 2 ? 2 : li);
    *frac = lambda - (float)*level;
    *frac = *frac < 0.0f ? 0.0f : (*frac > 1.0f ? 1.0f : *frac);
}

SURS_MR_HD inline int sh_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// bilinear lookup in one level (W x H x 3 floats at `level`)
SURS_MR_HD inline void sh_bilinear(const float *level, int W, int H, float u, float v, float *rgb) {
    float x = u * (float)W - 0.5f, y = (1.0f - v) * (float)H - 0.5f;
    x = x < -1.0f ? -1.0f : (x > (float)W ? (float)W : x);
    y = y < -1.0f ? -1.0f : (y > (float)H ? (float)H : y);
    const float xf = __builtin_floorf(x), yf = __builtin_floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int x0 = sh_clampi((int)xf, W), x1 = sh_clampi((int)xf + 1, W);
    const int y0 = sh_clampi((int)yf, H), y1 = sh_clampi((int)yf + 1, H);
    const float *r0 = level + (size_t)y0 * W * 3, *r1 = level + (size_t)y1 * W * 3;
    for (int c = 0; c < 3; ++c) {
        const float top = r0[x0 * 3 + c] * (1.0f - fx) + r0[x1 * 3 + c] * fx;
        const float bot = r1[x0 * 3 + c] * (1.0f - fx) + r1[x1 * 3 + c] * fx;
        rgb[c] = top * (1.0f - fy) + bot * fy;
    }
}

// the trilinear lookup: level l blended with level l + 1
SURS_MR_HD inline void sh_texture(const float *pyramid, int tw, int th, float u, float v, int level, float frac, float *rgb) {
    u = mr_finite(u) ? u : 0.0f, v = mr_finite(v) ? v : 0.0f;
    sh_bilinear(pyramid + sh_level_offset(tw, th, level), tw >> level, th >> level, u, v, rgb);
    if (frac > 0.0f && level + 1 < SH_LEVELS) {
        float up[3];
        sh_bilinear(pyramid + sh_level_offset(tw, th, level + 1), tw >> (level + 1), th >> (level + 1), u, v, up);
        for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] * (1.0f - frac) + up[c] * frac;
    }
}

// three (vertex, uv) index pairs ordered by ascending vertex index: mr_sort3 with the uv index carried along
SURS_MR_HD inline void sh_sort3(int *i, int *j) {
    int t;
    if (i[1] < i[0]) t = i[0], i[0] = i[1], i[1] = t, t = j[0], j[0] = j[1], j[1] = t;
    if (i[2] < i[1]) t = i[1], i[1] = i[2], i[2] = t, t = j[1], j[1] = j[2], j[2] = t;
    if (i[1] < i[0]) t = i[0], i[0] = i[1], i[1] = t, t = j[0], j[0] = j[1], j[1] = t;
}

// the analytic transfer vector of a unit normal: A_l Y_i(n)
SURS_MR_HD inline void sh_analytic(float nx, float ny, float nz, float *p) {
    prt_sh9(nx, ny, nz, p);
    p[0] = 3.14159274f * p[0];
    for (int i = 1; i < 4; ++i) p[i] = 2.09439516f * p[i];
    for (int i = 4; i < 9; ++i) p[i] = 0.785398185f * p[i];
}

// one pixel: the winner `f` of the raster (-1: background) and its (b1, b2) -> rgba[4]; shading[3] (nullable) gets s_c before the gamma
SURS_MR_HD inline void sh_pixel(const ShadeArgs &a, int f, float b1, float b2, float *rgba, float *shading) {
    rgba[0] = rgba[1] = rgba[2] = rgba[3] = 0.0f;
    if (shading) shading[0] = shading[1] = shading[2] = 0.0f;
    if (f < 0) return;
    f = sh_clampi(f, a.nf);
    int i[3], j[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) i[k] = sh_clampi(a.faces[(size_t)f * 3 + k], a.nv);
    if (a.pyramid)
        for (int k = 0; k < 3; ++k) j[k] = sh_clampi(a.faces_uv[(size_t)f * 3 + k], a.nuv);
    sh_sort3(i, j);
    const float b0 = (1.0f - b1) - b2;
    float albedo[3] = {1.0f, 1.0f, 1.0f};
    if (a.pyramid) {
        const float *t0 = a.uvs + (size_t)j[0] * 2, *t1 = a.uvs + (size_t)j[1] * 2, *t2 = a.uvs + (size_t)j[2] * 2;
        const float u = (b0 * t0[0] + b1 * t1[0]) + b2 * t2[0], v = (b0 * t0[1] + b1 * t1[1]) + b2 * t2[1];
        const float du1 = t1[0] - t0[0], dv1 = t1[1] - t0[1], du2 = t2[0] - t0[0], dv2 = t2[1] - t0[1];
        const float cuv = du1 * dv2 - dv1 * du2;
        float p0[3], p1[3], p2[3];
        mr_project(a.verts + (size_t)i[0] * 3, a.view, p0), mr_project(a.verts + (size_t)i[1] * 3, a.view, p1);
        mr_project(a.verts + (size_t)i[2] * 3, a.view, p2);
        const float hw = 0.5f * (float)a.w, hh = 0.5f * (float)a.h;
        const float x0 = (p0[0] + 1.0f) * hw - 0.5f, y0 = (p0[1] + 1.0f) * hh - 0.5f;
        const float x1 = (p1[0] + 1.0f) * hw - 0.5f, y1 = (p1[1] + 1.0f) * hh - 0.5f;
        const float x2 = (p2[0] + 1.0f) * hw - 0.5f, y2 = (p2[1] + 1.0f) * hh - 0.5f;
        const float cpix = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0);
        int level;
        float frac;
        sh_mip((cuv < 0.0f ? -cuv : cuv) * ((float)a.tw * (float)a.th), cpix < 0.0f ? -cpix : cpix, &level, &frac);
        sh_texture(a.pyramid, a.tw, a.th, u, v, level, frac, albedo);
    }
    float p[9];
    if (a.prt) {
        const float *q0 = a.prt + (size_t)i[0] * 9, *q1 = a.prt + (size_t)i[1] * 9, *q2 = a.prt + (size_t)i[2] * 9;
        for (int k = 0; k < 9; ++k) p[k] = (b0 * q0[k] + b1 * q1[k]) + b2 * q2[k];
    } else {
        const float *n0 = a.normals + (size_t)i[0] * 3, *n1 = a.normals + (size_t)i[1] * 3, *n2 = a.normals + (size_t)i[2] * 3;
        const float mx = (b0 * n0[0] + b1 * n1[0]) + b2 * n2[0];
        const float my = (b0 * n0[1] + b1 * n1[1]) + b2 * n2[1];
        const float mz = (b0 * n0[2] + b1 * n1[2]) + b2 * n2[2];
        const float *N = a.nm;
        const float nx = (N[0] * mx + N[1] * my) + N[2] * mz, ny = (N[3] * mx + N[4] * my) + N[5] * mz;
        const float nz = (N[6] * mx + N[7] * my) + N[8] * mz;
        const float l = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
        const bool has = (l > 0.0f) & mr_finite(l);
        const float d = has ? l : 1.0f;
        sh_analytic(has ? nx / d : 0.0f, has ? ny / d : 0.0f, has ? nz / d : 1.0f, p);
    }
    for (int c = 0; c < 3; ++c) {
        float s = 0.0f;
        for (int k = 0; k < 9; ++k) s = __builtin_fmaf(p[k], a.light[k * 3 + c], s);
        if (shading) shading[c] = s;
        const float g = albedo[c] * sh_gamma(s);
        rgba[c] = g > 0.0f ? (g < 1.0f ? g : 1.0f) : 0.0f;
    }
    rgba[3] = 1.0f;
}

SURS_MR_HD inline uint8_t sh_byte(float mean) {
    const float q = __builtin_rintf(mean * 255.0f);
    return (uint8_t)(q > 0.0f ? (q < 255.0f ? q : 255.0f) : 0.0f);
}

// resolved pixel (ox, oy) of an image whose sub-sample image rgba is W = w m floats-of-four wide
SURS_MR_HD inline void sh_resolve(const float *rgba, int W, int m, int ox, int oy, uint8_t *rgb, uint8_t *mask) {
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int sy = 0; sy < m; ++sy)
        for (int sx = 0; sx < m; ++sx) {
            const float *s = rgba + ((size_t)(oy * m + sy) * W + (size_t)(ox * m + sx)) * 4;
            for (int c = 0; c < 4; ++c) sum[c] = sum[c] + s[c];
        }
    const float n = (float)(m * m);
    for (int c = 0; c < 3; ++c) rgb[c] = sh_byte(sum[c] / n);
    if (mask) *mask = sh_byte(sum[3] / n);
}

}  // namespace surs
