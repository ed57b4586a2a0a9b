// Training images (include/surs.h "training images"): the per-pixel and per-output arithmetic of every stage, one statement for the
// kernels of surs_train_image.hip and for their _host twins.  Each function restates what Pillow does to ONE 8-bit value or pixel;
// what Pillow computes in double per image (filter weights, box lengths) is done on the host, into the plan's tables.  An RGB pixel
// travels as one dword, r | g << 8 | b << 16: LDS tiles of pixels are dword arrays, no byte-wide LDS access.
// Built with the library's -ffp-contract=off: the float and double expressions below round as written, on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TI_HD __host__ __device__
#else
#define TI_HD
#endif

namespace surs {

constexpr int TI_PRECISION_BITS = 22;   // fractional bits of a resample weight (Pillow: 32 - 8 - 2)
constexpr int TI_TILE = 32;             // output pixels along a tile's side, resample and blur
constexpr int TI_SPAN = 80;             // source pixels a resample tile may need along one axis (bicubic at 1/2: 72)
constexpr int TI_JITTER_PIXELS = 1024;  // pixels of one jitter workgroup = of one partial sum of L
constexpr int TI_BLUR_MAX_RADIUS = 20;  // integer box radius per pass the blur tile's halo is sized for

enum { TI_BRIGHTNESS = 0, TI_CONTRAST = 1, TI_SATURATION = 2, TI_HUE = 3 };

TI_HD inline uint32_t ti_pack(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }
TI_HD inline int ti_ch(uint32_t v, int c) { return (int)((v >> (8 * c)) & 255u); }

// ImageOps.expand(pad, fill 0) and the horizontal flip as an index map: pixel (ix, iy) of the padded, flipped image
TI_HD inline bool ti_source_index(int src_w, int src_h, int pad, int flip, int ix, int iy, size_t *index) {
    const int px = (flip ? src_w + 2 * pad - 1 - ix : ix) - pad, py = iy - pad;
    if (px < 0 || px >= src_w || py < 0 || py >= src_h) return false;
    *index = (size_t)py * src_w + px;
    return true;
}

TI_HD inline uint32_t ti_fetch_rgb(const uint8_t *src, int src_w, int src_h, int pad, int flip, int ix, int iy) {
    size_t i;
    if (!ti_source_index(src_w, src_h, pad, flip, ix, iy, &i)) return 0;
    return ti_pack(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
}

TI_HD inline int ti_fetch_mask(const uint8_t *src, int src_w, int src_h, int pad, int flip, int ix, int iy) {
    size_t i;
    if (ix < 0 || iy < 0 || !ti_source_index(src_w, src_h, pad, flip, ix, iy, &i)) return 0;
    return src[i];
}

// Resample.c: clip8 of a fixed-point sum
TI_HD inline int ti_clip8(int v) {
    v >>= TI_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One output pixel of one pass: sum px[i * stride] * k[i] per channel, from 2^21, then clip8
TI_HD inline uint32_t ti_dot(const uint32_t *px, int stride, const int32_t *k, int len) {
    int s0 = 1 << (TI_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < len; ++i) {
        const uint32_t v = px[(size_t)i * stride];
        const int kk = k[i];
        s0 += ti_ch(v, 0) * kk, s1 += ti_ch(v, 1) * kk, s2 += ti_ch(v, 2) * kk;
    }
    return ti_pack(ti_clip8(s0), ti_clip8(s1), ti_clip8(s2));
}

// ToTensor, Normalize(0.5, 0.5) and the mask product: surs_image_prepare's arithmetic
TI_HD inline float ti_prepare(int mask, int value) {
    const float m = (float)mask / 255.0f;
    float v = (float)value / 255.0f;
    v = (v - 0.5f) / 0.5f;
    return m * v;
}

// Image.blend(degenerate, image, f) on one byte (Blend.c)
TI_HD inline int ti_blend(int d, int x, float f) {
    const float t = (float)d + f * (float)(x - d);
    if (f >= 0.0f && f <= 1.0f) return (int)(uint8_t)t;
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)(uint8_t)t;
}

// convert("L") of an RGB pixel (Convert.c L24)
TI_HD inline int ti_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ImageEnhance.Contrast's degenerate value from the exact sum of L
TI_HD inline int ti_contrast_mean(unsigned long long sum_l, long long count) { return (int)((double)sum_l / (double)count + 0.5); }

// convert("HSV") of an RGB pixel (Convert.c rgb2hsv_row): float variables, double constants
TI_HD inline void ti_rgb2hsv(int r, int g, int b, int *ph, int *ps, int *pv) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    *pv = maxc;
    if (minc == maxc) {
        *ph = 0, *ps = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc)
        h = bc - gc;
    else if (g == maxc)
        h = (float)(2.0 + (double)rc - (double)bc);
    else
        h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    int uh = (int)((double)h * 255.0), us = (int)((double)s * 255.0);
    *ph = uh < 0 ? 0 : (uh > 255 ? 255 : uh);
    *ps = us < 0 ? 0 : (us > 255 ? 255 : us);
}

TI_HD inline int ti_round_clip8(double v) {
    const int i = (int)round(v);
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}

// convert("RGB") of an HSV pixel (Convert.c hsv2rgb)
TI_HD inline void ti_hsv2rgb(int h, int s, int v, int *pr, int *pg, int *pb) {
    if (s == 0) {
        *pr = *pg = *pb = v;
        return;
    }
    const double h6 = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const int p = ti_round_clip8((double)(float)v * (1.0 - (double)fs));
    const int q = ti_round_clip8((double)(float)v * (1.0 - (double)(fs * f)));
    const int t = ti_round_clip8((double)(float)v * (1.0 - (double)fs * (1.0 - (double)f)));
    switch (i % 6) {
        case 0: *pr = v, *pg = t, *pb = p; break;
        case 1: *pr = q, *pg = v, *pb = p; break;
        case 2: *pr = p, *pg = v, *pb = t; break;
        case 3: *pr = p, *pg = q, *pb = v; break;
        case 4: *pr = t, *pg = p, *pb = v; break;
        default: *pr = v, *pg = p, *pb = q; break;
    }
}

// One colour-jitter op on one pixel; mean: the contrast op's degenerate value
TI_HD inline void ti_jitter_op(int kind, float f, int shift, int mean, int *r, int *g, int *b) {
    if (kind == TI_BRIGHTNESS) {
        *r = ti_blend(0, *r, f), *g = ti_blend(0, *g, f), *b = ti_blend(0, *b, f);
    } else if (kind == TI_CONTRAST) {
        *r = ti_blend(mean, *r, f), *g = ti_blend(mean, *g, f), *b = ti_blend(mean, *b, f);
    } else if (kind == TI_SATURATION) {
        const int l = ti_luma(*r, *g, *b);
        *r = ti_blend(l, *r, f), *g = ti_blend(l, *g, f), *b = ti_blend(l, *b, f);
    } else {
        int h, s, v;
        ti_rgb2hsv(*r, *g, *b, &h, &s, &v);
        ti_hsv2rgb((h + shift) & 255, s, v, r, g, b);
    }
}

// One output pixel of one extended-box pass (BoxBlur.c), in the windowed form: the sums are integers, so Pillow's running sum
// gives these bits.  line[(i - origin) * stride] is pixel i of the line, n its length; edges replicate.
TI_HD inline uint32_t ti_box(const uint32_t *line, int stride, int origin, int x, int n, int radius, uint32_t ww, uint32_t fw) {
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    for (int k = -radius; k <= radius; ++k) {
        int i = x + k;
        i = i < 0 ? 0 : (i >= n ? n - 1 : i);
        const uint32_t v = line[(size_t)(i - origin) * stride];
        a0 += (uint32_t)ti_ch(v, 0), a1 += (uint32_t)ti_ch(v, 1), a2 += (uint32_t)ti_ch(v, 2);
    }
    int il = x - radius - 1, ir = x + radius + 1;
    il = il < 0 ? 0 : il;
    ir = ir >= n ? n - 1 : ir;
    const uint32_t vl = line[(size_t)(il - origin) * stride], vr = line[(size_t)(ir - origin) * stride];
    const uint32_t b0 = a0 * ww + (uint32_t)(ti_ch(vl, 0) + ti_ch(vr, 0)) * fw;
    const uint32_t b1 = a1 * ww + (uint32_t)(ti_ch(vl, 1) + ti_ch(vr, 1)) * fw;
    const uint32_t b2 = a2 * ww + (uint32_t)(ti_ch(vl, 2) + ti_ch(vr, 2)) * fw;
    return ti_pack((int)(uint8_t)((b0 + (1u << 23)) >> 24), (int)(uint8_t)((b1 + (1u << 23)) >> 24),
                   (int)(uint8_t)((b2 + (1u << 23)) >> 24));
}

}  // namespace surs
