// Colour shading of a rastered view (include/surs.h "mesh shading"): the texture pyramid, the per-pixel colour from the raster's face /
// bary, and the box resolve of the sub-samples, each one lane per output element around the arithmetic of surs_mesh_shade.h.
//
//   texture_level0_kernel    one lane per texel channel: u8 / 255.
//   texture_down_kernel      one lane per texel channel of level l: the 2 x 2 mean of level l - 1 (one launch per level).
//   mesh_shade_prt_kernel    one lane per pixel: sh_pixel.
//   image_resolve_kernel     one lane per resolved pixel: sh_resolve.
//   the _host entries        the same header looped on the host: what the kernels are held against bit for bit.
// Nothing here depends on surs_mesh_prt.hip: without a prt array the shading is analytic.
#include "surs_common.h"
#include "surs_mesh_shade.h"

#include <cstdint>

namespace {
using namespace surs;

constexpr int SHADE_MAX_SIDE = 8192;

__global__ __launch_bounds__(256) void texture_level0_kernel(const uint8_t *__restrict__ tex, size_t n, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)tex[i] / 255.0f;
}

SURS_MR_HD inline float down_texel(const float *src, int sw, int x, int y, int c) {
    const float *r0 = src + ((size_t)(2 * y) * sw + (size_t)(2 * x)) * 3 + c, *r1 = r0 + (size_t)sw * 3;
    return ((r0[0] + r0[3]) + (r1[0] + r1[3])) * 0.25f;
}

__global__ __launch_bounds__(256) void texture_down_kernel(const float *__restrict__ src, int dw, int dh, float *__restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)dw * dh * 3) return;
    const int c = (int)(i % 3);
    const size_t t = i / 3;
    dst[i] = down_texel(src, dw * 2, (int)(t % dw), (int)(t / dw), c);
}

__global__ __launch_bounds__(256) void mesh_shade_prt_kernel(ShadeArgs a, const int32_t *__restrict__ face, const float *__restrict__ bary,
                                                              int pixels, float *__restrict__ rgba) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    float out[4];
    sh_pixel(a, face[p], bary[(size_t)p * 2], bary[(size_t)p * 2 + 1], out, nullptr);
    float *o = rgba + (size_t)p * 4;
    o[0] = out[0], o[1] = out[1], o[2] = out[2], o[3] = out[3];
}

__global__ __launch_bounds__(256) void image_resolve_kernel(const float *__restrict__ rgba, int w, int h, int m, uint8_t *__restrict__ rgb,
                                                             uint8_t *__restrict__ mask) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x;
    if (p >= w * h) return;
    uint8_t c[3], a;
    sh_resolve(rgba, w * m, m, p % w, p / w, c, &a);
    rgb[(size_t)p * 3] = c[0], rgb[(size_t)p * 3 + 1] = c[1], rgb[(size_t)p * 3 + 2] = c[2];
    if (mask) mask[p] = a;
}

int pyramid_args(const uint8_t *tex, int w, int h, const float *levels) {
    SURS_REQUIRE(tex && levels, "tex and levels must not be NULL");
    SURS_REQUIRE(w >= 8 && h >= 8 && w % 8 == 0 && h % 8 == 0 && w <= SH_MAX_TEX && h <= SH_MAX_TEX,
                 "a texture of w %d x h %d: each must be a multiple of 8 in [8, %d]", w, h, SH_MAX_TEX);
    return 0;
}

int shade_args(const int32_t *face, const float *bary, const float *verts, int nv, const int32_t *faces, int nf, const float *view,
               const int32_t *faces_uv, const float *uvs, int nuv, const float *prt, const float *normals, const float *normal_matrix,
               const float *light, const float *pyramid, int tw, int th, int w, int h, const float *rgba, ShadeArgs *a) {
    SURS_REQUIRE(face && bary && verts && faces && view && light && rgba, "face, bary, verts, faces, view, light and rgba must not be NULL");
    SURS_REQUIRE(nv >= 1 && nf >= 1, "a mesh needs vertices and faces (nv %d, nf %d)", nv, nf);
    SURS_REQUIRE(w >= 1 && h >= 1 && w <= SHADE_MAX_SIDE && h <= SHADE_MAX_SIDE, "an image of w %d x h %d: each must be in [1, %d]", w, h,
                 SHADE_MAX_SIDE);
    SURS_REQUIRE(prt || (normals && normal_matrix), "without prt the vertex normals and the normal matrix are needed");
    if (pyramid) {
        SURS_REQUIRE(faces_uv && uvs && nuv >= 1, "a texture needs faces_uv and uvs (nuv %d)", nuv);
        SURS_REQUIRE(tw >= 8 && th >= 8 && tw % 8 == 0 && th % 8 == 0 && tw <= SH_MAX_TEX && th <= SH_MAX_TEX,
                     "a texture of w %d x h %d: each must be a multiple of 8 in [8, %d]", tw, th, SH_MAX_TEX);
    }
    a->verts = verts, a->faces = faces, a->nv = nv, a->nf = nf;
    a->faces_uv = pyramid ? faces_uv : nullptr, a->uvs = pyramid ? uvs : nullptr, a->nuv = pyramid ? nuv : 0;
    a->prt = prt, a->normals = prt ? nullptr : normals, a->pyramid = pyramid;
    a->tw = tw, a->th = th, a->w = w, a->h = h;
    for (int i = 0; i < 12; ++i) a->view[i] = view[i];
    for (int i = 0; i < 9; ++i) a->nm[i] = prt ? 0.0f : normal_matrix[i];
    for (int i = 0; i < 27; ++i) a->light[i] = light[i];
    return 0;
}

int resolve_args(const float *rgba, int w, int h, int m, const uint8_t *rgb) {
    SURS_REQUIRE(rgba && rgb, "rgba and rgb must not be NULL");
    SURS_REQUIRE(m >= 1 && m <= 8, "%d x %d sub-samples a pixel: 1 .. 8 are built", m, m);
    SURS_REQUIRE(w >= 1 && h >= 1 && w * m <= SHADE_MAX_SIDE && h * m <= SHADE_MAX_SIDE,
                 "an image of w %d x h %d at %d sub-samples a side: each side must be in [1, %d]", w, h, m, SHADE_MAX_SIDE);
    return 0;
}
}  // namespace

extern "C" size_t surs_texture_pyramid_floats(int w, int h) {
    if (w < 8 || h < 8 || w % 8 || h % 8 || w > SH_MAX_TEX || h > SH_MAX_TEX) return 0;
    return sh_level_offset(w, h, SH_LEVELS);
}

extern "C" int surs_texture_pyramid(const uint8_t *tex, int w, int h, float *levels, void *stream) {
    if (int e = pyramid_args(tex, w, h, levels)) return e;
    hipStream_t st = as_stream(stream);
    const size_t n0 = (size_t)w * h * 3;
    hipLaunchKernelGGL(texture_level0_kernel, dim3(ceil_div((long long)n0, 256)), dim3(256), 0, st, tex, n0, levels);
    SURS_LAUNCH_CHECK();
    for (int l = 1; l < SH_LEVELS; ++l) {
        const int dw = w >> l, dh = h >> l;
        hipLaunchKernelGGL(texture_down_kernel, dim3(ceil_div((long long)dw * dh * 3, 256)), dim3(256), 0, st,
                           levels + sh_level_offset(w, h, l - 1), dw, dh, levels + sh_level_offset(w, h, l));
        SURS_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int surs_texture_pyramid_host(const uint8_t *tex, int w, int h, float *levels) {
    if (int e = pyramid_args(tex, w, h, levels)) return e;
    const size_t n0 = (size_t)w * h * 3;
    for (size_t i = 0; i < n0; ++i) levels[i] = (float)tex[i] / 255.0f;
    for (int l = 1; l < SH_LEVELS; ++l) {
        const int dw = w >> l, dh = h >> l;
        const float *src = levels + sh_level_offset(w, h, l - 1);
        float *dst = levels + sh_level_offset(w, h, l);
        for (int y = 0; y < dh; ++y)
            for (int x = 0; x < dw; ++x)
                for (int c = 0; c < 3; ++c) dst[((size_t)y * dw + x) * 3 + c] = down_texel(src, dw * 2, x, y, c);
    }
    return 0;
}

extern "C" int surs_mesh_shade_prt(const int32_t *face, const float *bary, const float *verts, int nv, const int32_t *faces, int nf,
                                   const float *view, const int32_t *faces_uv, const float *uvs, int nuv, const float *prt,
                                   const float *normals, const float *normal_matrix, const float *light, const float *pyramid, int tw,
                                   int th, int w, int h, float *rgba, void *stream) {
    ShadeArgs a;
    if (int e = shade_args(face, bary, verts, nv, faces, nf, view, faces_uv, uvs, nuv, prt, normals, normal_matrix, light, pyramid, tw, th,
                           w, h, rgba, &a))
        return e;
    hipLaunchKernelGGL(mesh_shade_prt_kernel, dim3(ceil_div((long long)w * h, 256)), dim3(256), 0, as_stream(stream), a, face, bary, w * h,
                       rgba);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_mesh_shade_prt_host(const int32_t *face, const float *bary, const float *verts, int nv, const int32_t *faces, int nf,
                                        const float *view, const int32_t *faces_uv, const float *uvs, int nuv, const float *prt,
                                        const float *normals, const float *normal_matrix, const float *light, const float *pyramid,
                                        int tw, int th, int w, int h, float *rgba, float *shading) {
    ShadeArgs a;
    if (int e = shade_args(face, bary, verts, nv, faces, nf, view, faces_uv, uvs, nuv, prt, normals, normal_matrix, light, pyramid, tw, th,
                           w, h, rgba, &a))
        return e;
    for (size_t p = 0; p < (size_t)w * h; ++p)
        sh_pixel(a, face[p], bary[2 * p], bary[2 * p + 1], rgba + 4 * p, shading ? shading + 3 * p : nullptr);
    return 0;
}

extern "C" int surs_image_resolve(const float *rgba, int w, int h, int m, uint8_t *rgb, uint8_t *mask, void *stream) {
    if (int e = resolve_args(rgba, w, h, m, rgb)) return e;
    hipLaunchKernelGGL(image_resolve_kernel, dim3(ceil_div((long long)w * h, 256)), dim3(256), 0, as_stream(stream), rgba, w, h, m, rgb,
                       mask);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_image_resolve_host(const float *rgba, int w, int h, int m, uint8_t *rgb, uint8_t *mask) {
    if (int e = resolve_args(rgba, w, h, m, rgb)) return e;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) sh_resolve(rgba, w * m, m, x, y, rgb + ((size_t)y * w + x) * 3, mask ? mask + (size_t)y * w + x : nullptr);
    return 0;
}
