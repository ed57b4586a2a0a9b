// Training images (include/surs.h "training images"): the image half of a training item on the device, with the arithmetic of
// surs_train_image.h.
//
//   ti_resample_kernel<false>  geometry: grid = tiles of 32 x 32 output pixels of the crop window.  A workgroup stages the source pixels
//                              its tile needs (the host's tile spans, at most 80 x 80) through LDS as dwords r | g << 8 | b << 16,
//                              with pad and flip folded into the fetch; the horizontal pass writes [rows needed][32] dwords to LDS,
//                              8-bit rounded; the vertical pass reads them.  The mask is a NEAREST gather from the host's index tables.
//   ti_resample_kernel<true>   the half-size pair: the same two passes (BICUBIC tables), the NEAREST mask and ti_prepare, fp32 out.
//   ti_jitter_kernel           1024 pixels a workgroup, every op per pixel in registers.  Where the ops hold a contrast, a first launch
//                              runs the ops in front of it and writes one uint32 sum of L per workgroup; the second launch's
//                              workgroups each add ALL partial sums (integers: any order gives the same sum), form the mean in double
//                              and run the contrast and the ops behind it.  No atomics, nothing read back.
//   ti_blur_kernel<VERT>       tiles of 32 lines x 32 positions plus a halo of 3 (radius + 1) positions each way in LDS (dwords); the
//                              three box passes of one direction ping-pong between two LDS images, each pass 8-bit rounded, the
//                              range shrinking by radius + 1 a pass.  Lanes run along x in both directions.
//   *_host                     the same header looped on the host: what the kernels are held against bit for bit, and what
//                              tests/test_train_images_host.py holds against Pillow.
#include "surs_common.h"
#include "surs_train_image.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace {
using namespace surs;

constexpr int TI_THREADS = 256;
static_assert(TI_JITTER_PIXELS == 4 * TI_THREADS, "four pixels per lane");

// ------------------------------------------------------------------------------------------------ host: tables

double filter_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

double filter_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int axis_ksize(int in_size, int out_size, int filter) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = (filter == SURS_FILTER_BICUBIC ? 2.0 : 1.0) * filterscale;
    return (int)ceil(support) * 2 + 1;
}

struct AxisLayout {
    int ksize, tiles;
    size_t off_b, off_k, off_n, off_t, end;
};

AxisLayout axis_layout(int in_size, int full, int window, int filter, size_t base) {
    AxisLayout a;
    a.ksize = axis_ksize(in_size, full, filter);
    a.tiles = ceil_div(window, TI_TILE);
    a.off_b = base;
    a.off_k = a.off_b + sizeof(int32_t) * 2 * (size_t)window;
    a.off_n = a.off_k + sizeof(int32_t) * (size_t)a.ksize * window;
    a.off_t = a.off_n + sizeof(int32_t) * (size_t)window;
    a.end = a.off_t + sizeof(int32_t) * 2 * (size_t)a.tiles;
    return a;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc and Geometry.c ImagingScaleAffine for the window [w0, w0 + window) of an axis
// resampled from in_size to full; false where a tile's span exceeds TI_SPAN
bool axis_tables(int in_size, int full, int w0, int window, int filter, const AxisLayout &a, char *tables) {
    int32_t *bounds = (int32_t *)(tables + a.off_b), *kk = (int32_t *)(tables + a.off_k), *nn = (int32_t *)(tables + a.off_n),
            *tt = (int32_t *)(tables + a.off_t);
    const double scale = (double)in_size / full;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == SURS_FILTER_BICUBIC ? 2.0 : 1.0) * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> k(a.ksize);
    // nearest: xo accumulated by repeated addition from the FIRST pixel of the full line, as ImagingScaleAffine does
    std::vector<int32_t> nearest(full > 0 ? full : 0);
    double xo = 0.0 + scale * 0.5;
    for (int x = 0; x < full; ++x) {
        const int xin = xo < 0.0 ? -1 : (int)xo;
        nearest[x] = xin >= 0 && xin < in_size ? xin : -1;
        xo += scale;
    }
    for (int t = 0; t < a.tiles; ++t) tt[2 * t] = 0, tt[2 * t + 1] = 0;
    for (int o = 0; o < window; ++o) {
        const int xx = w0 + o;
        int32_t *ko = kk + (size_t)o * a.ksize;
        for (int x = 0; x < a.ksize; ++x) ko[x] = 0;
        if (xx < 0 || xx >= full) {
            bounds[2 * o] = 0, bounds[2 * o + 1] = 0, nn[o] = -1;
            continue;
        }
        nn[o] = nearest[xx];
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > a.ksize) return false;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            const double w = filter == SURS_FILTER_BICUBIC ? filter_bicubic(arg) : filter_bilinear(arg);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            ko[x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << TI_PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << TI_PRECISION_BITS));
        }
        bounds[2 * o] = xmin, bounds[2 * o + 1] = xmax;
        int32_t *span = tt + 2 * (o / TI_TILE);
        if (span[1] == 0)
            span[0] = xmin, span[1] = xmin + xmax;
        else {
            if (xmin < span[0]) span[0] = xmin;
            if (xmin + xmax > span[1]) span[1] = xmin + xmax;
        }
    }
    for (int t = 0; t < a.tiles; ++t)
        if (tt[2 * t + 1] - tt[2 * t] > TI_SPAN) return false;
    return true;
}

int resample_plan(int src_w, int src_h, int pad, int flip, int full_w, int full_h, int filter, int x0, int y0, int out_w, int out_h,
                  SursImageResample *r, void *tables, size_t tables_bytes, size_t base, size_t *used) {
    SURS_REQUIRE(r, "r must not be NULL");
    SURS_REQUIRE(src_w >= 1 && src_h >= 1 && pad >= 0 && full_w >= 1 && full_h >= 1 && out_w >= 1 && out_h >= 1,
                 "a resample of %d x %d (pad %d) to %d x %d, window %d x %d: every size must be >= 1", src_w, src_h, pad, full_w, full_h,
                 out_w, out_h);
    SURS_REQUIRE(src_w <= 16384 && src_h <= 16384 && pad <= 16384 && full_w <= 32768 && full_h <= 32768 && out_w <= 16384 &&
                     out_h <= 16384 && x0 > -32768 && x0 < 32768 && y0 > -32768 && y0 < 32768,
                 "a resample of %d x %d (pad %d) to %d x %d, window %d x %d at (%d, %d): a side beyond 16384", src_w, src_h, pad, full_w,
                 full_h, out_w, out_h, x0, y0);
    SURS_REQUIRE(filter == SURS_FILTER_BILINEAR || filter == SURS_FILTER_BICUBIC, "filter %d: BILINEAR (2) or BICUBIC (3) is needed", filter);
    const AxisLayout ax = axis_layout(src_w + 2 * pad, full_w, out_w, filter, base);
    const AxisLayout ay = axis_layout(src_h + 2 * pad, full_h, out_h, filter, ax.end);
    SURS_REQUIRE(ay.end < (1ull << 31), "tables of %zu bytes", ay.end);
    r->src_w = src_w, r->src_h = src_h, r->pad = pad, r->flip = flip ? 1 : 0, r->full_w = full_w, r->full_h = full_h;
    r->x0 = x0, r->y0 = y0, r->out_w = out_w, r->out_h = out_h, r->filter = filter, r->ksize_x = ax.ksize, r->ksize_y = ay.ksize;
    r->off_xb = (int)ax.off_b, r->off_xk = (int)ax.off_k, r->off_xn = (int)ax.off_n, r->off_xt = (int)ax.off_t;
    r->off_yb = (int)ay.off_b, r->off_yk = (int)ay.off_k, r->off_yn = (int)ay.off_n, r->off_yt = (int)ay.off_t;
    r->reserved = 0;
    if (used) *used = ay.end - base;
    if (!tables) return 0;
    SURS_REQUIRE(tables_bytes >= ay.end, "tables of %zu bytes, %zu needed", tables_bytes, ay.end);
    const bool ok = axis_tables(src_w + 2 * pad, full_w, x0, out_w, filter, ax, (char *)tables) &&
                    axis_tables(src_h + 2 * pad, full_h, y0, out_h, filter, ay, (char *)tables);
    SURS_REQUIRE(ok, "a resample of %d x %d to %d x %d: a tile of %d outputs needs more than %d source pixels along an axis",
                 src_w + 2 * pad, src_h + 2 * pad, full_w, full_h, TI_TILE, TI_SPAN);
    return 0;
}

int resample_args(const SursImageResample *r, const void *tables, const void *src, const void *out) {
    SURS_REQUIRE(r && tables && src && out, "r, tables, the source and out must not be NULL");
    SURS_REQUIRE(r->src_w >= 1 && r->src_h >= 1 && r->out_w >= 1 && r->out_h >= 1 && r->ksize_x >= 1 && r->ksize_y >= 1 && r->pad >= 0,
                 "a resample that surs_image_resample_plan did not fill");
    return 0;
}

// BoxBlur.c _gaussian_blur_radius and ImagingHorizontalBoxBlur's constants: float variables, double constants
void blur_constants(double gaussian_radius, int *radius, unsigned *ww, unsigned *fw) {
    const float r = (float)gaussian_radius;
    const float sigma2 = r * r / 3;
    const float L = (float)sqrt(12.0 * (double)sigma2 + 1.0);
    const float l = (float)floor(((double)L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float box = l + a;
    if (!(box > 0.0f)) {
        *radius = 0, *ww = 0, *fw = 0;   // radius 0 is a copy
        return;
    }
    *radius = (int)box;
    *ww = (uint32_t)((float)(uint32_t)(1 << 24) / (box * 2 + 1));
    *fw = ((uint32_t)(1 << 24) - (uint32_t)(*radius * 2 + 1) * *ww) / 2;
}

struct TiOps {
    int n;
    int kind[4];
    float f[4];
    int shift;
};

// the ops [first, last) of a plan
TiOps ops_range(const SursTrainImagePlan *p, int first, int last) {
    TiOps o;
    o.n = 0, o.shift = p->hue_shift;
    for (int i = 0; i < 4; ++i) o.kind[i] = 0, o.f[i] = 1.0f;
    for (int i = first; i < last; ++i) o.kind[o.n] = p->op_kind[i], o.f[o.n] = p->op_factor[i], ++o.n;
    return o;
}

int contrast_at(const SursTrainImagePlan *p) {
    for (int i = 0; i < p->n_ops; ++i)
        if (p->op_kind[i] == SURS_JITTER_CONTRAST) return i;
    return -1;
}

int plan_ops_args(const SursTrainImagePlan *p) {
    SURS_REQUIRE(p, "plan must not be NULL");
    SURS_REQUIRE(p->n_ops >= 0 && p->n_ops <= 4, "a plan of %d jitter ops", p->n_ops);
    for (int i = 0; i < p->n_ops; ++i) SURS_REQUIRE(p->op_kind[i] >= 0 && p->op_kind[i] <= 3, "jitter op kind %d", p->op_kind[i]);
    SURS_REQUIRE(p->blur_radius >= 0 && p->blur_radius <= TI_BLUR_MAX_RADIUS, "a box radius of %d per pass: at most %d", p->blur_radius,
                 TI_BLUR_MAX_RADIUS);
    return 0;
}

int image_args(const void *in, int w, int h, const void *out) {
    SURS_REQUIRE(in && out, "the image and out must not be NULL");
    SURS_REQUIRE(w >= 1 && h >= 1 && w <= 16384 && h <= 16384, "an image of w %d x h %d: each must be in [1, 16384]", w, h);
    return 0;
}

size_t image_bytes(int w, int h) { return align_up((size_t)w * h * 3, 256); }
size_t mask_bytes(int w, int h) { return align_up((size_t)w * h, 256); }
int jitter_groups(int w, int h) { return ceil_div((long long)w * h, TI_JITTER_PIXELS); }
size_t partial_bytes(int w, int h) { return align_up((size_t)jitter_groups(w, h) * sizeof(uint32_t), 256); }

// ------------------------------------------------------------------------------------------------ kernels

template <bool PREPARE>
__global__ __launch_bounds__(TI_THREADS) void ti_resample_kernel(SursImageResample r, const char *__restrict__ tables,
                                                                  const uint8_t *__restrict__ src_rgb, const uint8_t *__restrict__ src_mask,
                                                                  uint8_t *__restrict__ out_rgb, uint8_t *__restrict__ out_mask,
                                                                  float *__restrict__ out_f) {
    __shared__ uint32_t s_src[TI_SPAN * TI_SPAN];
    __shared__ uint32_t s_mid[TI_SPAN * TI_TILE];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * TI_TILE, oy0 = blockIdx.y * TI_TILE;
    const int cols = min(TI_TILE, r.out_w - ox0), rows = min(TI_TILE, r.out_h - oy0);
    const int32_t *xb = (const int32_t *)(tables + r.off_xb), *xk = (const int32_t *)(tables + r.off_xk);
    const int32_t *yb = (const int32_t *)(tables + r.off_yb), *yk = (const int32_t *)(tables + r.off_yk);
    int sx_lo = 0, sy_lo = 0, sx_n = 0, sy_n = 0;
    if (src_rgb) {
        const int32_t *xt = (const int32_t *)(tables + r.off_xt) + 2 * blockIdx.x, *yt = (const int32_t *)(tables + r.off_yt) + 2 * blockIdx.y;
        sx_lo = xt[0], sy_lo = yt[0];
        sx_n = max(0, min(TI_SPAN, xt[1] - sx_lo)), sy_n = max(0, min(TI_SPAN, yt[1] - sy_lo));
        for (int i = tid; i < sx_n * sy_n; i += TI_THREADS) {
            const int yy = i / sx_n, xx = i - yy * sx_n;
            s_src[yy * TI_SPAN + xx] = ti_fetch_rgb(src_rgb, r.src_w, r.src_h, r.pad, r.flip, sx_lo + xx, sy_lo + yy);
        }
        __syncthreads();
        for (int i = tid; i < sy_n * TI_TILE; i += TI_THREADS) {
            const int yy = i / TI_TILE, c = i % TI_TILE;
            if (c >= cols) continue;
            const int off = xb[2 * (ox0 + c)] - sx_lo;
            int len = min(xb[2 * (ox0 + c) + 1], r.ksize_x);
            if (off < 0 || off + len > sx_n) len = 0;   // (tables of another plan: stay inside the tile)
            s_mid[yy * TI_TILE + c] = ti_dot(s_src + yy * TI_SPAN + off, 1, xk + (size_t)(ox0 + c) * r.ksize_x, len);
        }
        __syncthreads();
    }
    const int32_t *xn = (const int32_t *)(tables + r.off_xn), *yn = (const int32_t *)(tables + r.off_yn);
    for (int i = tid; i < rows * TI_TILE; i += TI_THREADS) {
        const int rr = i / TI_TILE, c = i % TI_TILE;
        if (c >= cols) continue;
        uint32_t v = 0;
        if (src_rgb) {
            const int off = yb[2 * (oy0 + rr)] - sy_lo;
            int len = min(yb[2 * (oy0 + rr) + 1], r.ksize_y);
            if (off < 0 || off + len > sy_n) len = 0;
            v = ti_dot(s_mid + off * TI_TILE + c, TI_TILE, yk + (size_t)(oy0 + rr) * r.ksize_y, len);
        }
        int m = 0;
        if (src_mask) m = ti_fetch_mask(src_mask, r.src_w, r.src_h, r.pad, r.flip, xn[ox0 + c], yn[oy0 + rr]);
        const size_t o = (size_t)(oy0 + rr) * r.out_w + ox0 + c;
        if (PREPARE) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out_f[o * 3 + ch] = ti_prepare(m, ti_ch(v, ch));
        } else {
            if (out_rgb) out_rgb[o * 3] = (uint8_t)ti_ch(v, 0), out_rgb[o * 3 + 1] = (uint8_t)ti_ch(v, 1), out_rgb[o * 3 + 2] = (uint8_t)ti_ch(v, 2);
            if (out_mask) out_mask[o] = (uint8_t)m;
        }
    }
}

__global__ __launch_bounds__(TI_THREADS) void ti_jitter_kernel(const uint8_t *in, uint8_t *out, long long npix, TiOps ops,
                                                                const uint32_t *__restrict__ partials_in, int n_partials,
                                                                uint32_t *__restrict__ partials_out) {
    __shared__ unsigned long long s_sum[TI_THREADS];
    const int tid = threadIdx.x;
    int mean = 0;
    if (partials_in) {   // the first op is the contrast: every workgroup adds all partial sums of L
        unsigned long long s = 0;
        for (int i = tid; i < n_partials; i += TI_THREADS) s += partials_in[i];
        s_sum[tid] = s;
        __syncthreads();
        for (int step = TI_THREADS / 2; step > 0; step >>= 1) {
            if (tid < step) s_sum[tid] += s_sum[tid + step];
            __syncthreads();
        }
        mean = ti_contrast_mean(s_sum[0], npix);
        __syncthreads();
    }
    unsigned long long lsum = 0;
#pragma unroll
    for (int k = 0; k < TI_JITTER_PIXELS / TI_THREADS; ++k) {
        const long long p = ((long long)blockIdx.x * (TI_JITTER_PIXELS / TI_THREADS) + k) * TI_THREADS + tid;
        if (p >= npix) continue;
        int r = in[p * 3], g = in[p * 3 + 1], b = in[p * 3 + 2];
        for (int i = 0; i < ops.n; ++i) ti_jitter_op(ops.kind[i], ops.f[i], ops.shift, mean, &r, &g, &b);
        if (out) out[p * 3] = (uint8_t)r, out[p * 3 + 1] = (uint8_t)g, out[p * 3 + 2] = (uint8_t)b;
        lsum += (unsigned)ti_luma(r, g, b);
    }
    if (partials_out) {
        s_sum[tid] = lsum;
        __syncthreads();
        for (int step = TI_THREADS / 2; step > 0; step >>= 1) {
            if (tid < step) s_sum[tid] += s_sum[tid + step];
            __syncthreads();
        }
        if (tid == 0) partials_out[blockIdx.x] = (uint32_t)s_sum[0];   // at most 1024 * 255
    }
}

// positions run along the blurred direction, lines across it; lanes along x in both directions
template <bool VERT>
__global__ __launch_bounds__(TI_THREADS) void ti_blur_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int w, int h,
                                                              int radius, uint32_t ww, uint32_t fw) {
    extern __shared__ uint32_t s_buf[];
    const int tid = threadIdx.x;
    const int halo = 3 * (radius + 1), np = TI_TILE + 2 * halo;
    const int n = VERT ? h : w, nl = VERT ? w : h;
    const int p0 = (VERT ? blockIdx.y : blockIdx.x) * TI_TILE, l0 = (VERT ? blockIdx.x : blockIdx.y) * TI_TILE;
    const int lo = p0 - halo;
    const int stride = VERT ? TI_TILE : 1, line_stride = VERT ? 1 : np;
    uint32_t *a = s_buf, *b = s_buf + TI_TILE * np;
    const int total = TI_TILE * np;
    for (int i = tid; i < total; i += TI_THREADS) {
        const int pp = VERT ? i / TI_TILE : i % np, ll = VERT ? i % TI_TILE : i / np;
        const int pos = lo + pp, line = l0 + ll;
        if (pos < 0 || pos >= n || line >= nl) continue;
        const uint8_t *q = in + ((size_t)(VERT ? pos : line) * w + (VERT ? line : pos)) * 3;
        a[pp * stride + ll * line_stride] = ti_pack(q[0], q[1], q[2]);
    }
    __syncthreads();
    for (int pass = 0; pass < 3; ++pass) {
        const int margin = (2 - pass) * (radius + 1);
        const uint32_t *src = pass == 1 ? b : a;
        uint32_t *dst = pass == 0 ? b : a;
        for (int i = tid; i < total; i += TI_THREADS) {
            const int pp = VERT ? i / TI_TILE : i % np, ll = VERT ? i % TI_TILE : i / np;
            const int pos = lo + pp, line = l0 + ll;
            if (pos < p0 - margin || pos >= p0 + TI_TILE + margin || pos < 0 || pos >= n || line >= nl) continue;
            const uint32_t v = ti_box(src + ll * line_stride, stride, lo, pos, n, radius, ww, fw);
            if (pass < 2) {
                dst[pp * stride + ll * line_stride] = v;
            } else {
                uint8_t *q = out + ((size_t)(VERT ? pos : line) * w + (VERT ? line : pos)) * 3;
                q[0] = (uint8_t)ti_ch(v, 0), q[1] = (uint8_t)ti_ch(v, 1), q[2] = (uint8_t)ti_ch(v, 2);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ launches

int launch_resample(bool prepare, const SursImageResample &r, const void *tables, const uint8_t *rgb, const uint8_t *mask, uint8_t *out_rgb,
                    uint8_t *out_mask, float *out_f, hipStream_t st) {
    const dim3 grid(ceil_div(r.out_w, TI_TILE), ceil_div(r.out_h, TI_TILE));
    if (prepare)
        hipLaunchKernelGGL(ti_resample_kernel<true>, grid, dim3(TI_THREADS), 0, st, r, (const char *)tables, rgb, mask, out_rgb, out_mask, out_f);
    else
        hipLaunchKernelGGL(ti_resample_kernel<false>, grid, dim3(TI_THREADS), 0, st, r, (const char *)tables, rgb, mask, out_rgb, out_mask, out_f);
    SURS_LAUNCH_CHECK();
    return 0;
}

int launch_jitter(const SursTrainImagePlan *p, const uint8_t *in, int w, int h, uint32_t *partials, uint8_t *out, hipStream_t st) {
    const long long npix = (long long)w * h;
    const int groups = jitter_groups(w, h);
    const int at = contrast_at(p);
    if (at < 0) {
        hipLaunchKernelGGL(ti_jitter_kernel, dim3(groups), dim3(TI_THREADS), 0, st, in, out, npix, ops_range(p, 0, p->n_ops),
                           (const uint32_t *)nullptr, 0, (uint32_t *)nullptr);
        SURS_LAUNCH_CHECK();
        return 0;
    }
    // the ops in front of the contrast (none: the launch only sums), with the partial sums of L of what they leave
    hipLaunchKernelGGL(ti_jitter_kernel, dim3(groups), dim3(TI_THREADS), 0, st, in, at > 0 ? out : (uint8_t *)nullptr, npix,
                       ops_range(p, 0, at), (const uint32_t *)nullptr, 0, partials);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ti_jitter_kernel, dim3(groups), dim3(TI_THREADS), 0, st, at > 0 ? (const uint8_t *)out : in, out, npix,
                       ops_range(p, at, p->n_ops), (const uint32_t *)partials, groups, (uint32_t *)nullptr);
    SURS_LAUNCH_CHECK();
    return 0;
}

int launch_blur(const SursTrainImagePlan *p, const uint8_t *in, int w, int h, uint8_t *tmp, uint8_t *out, hipStream_t st) {
    const size_t lds = (size_t)2 * TI_TILE * (TI_TILE + 6 * (p->blur_radius + 1)) * sizeof(uint32_t);
    const dim3 grid(ceil_div(w, TI_TILE), ceil_div(h, TI_TILE));
    hipLaunchKernelGGL(ti_blur_kernel<false>, grid, dim3(TI_THREADS), lds, st, in, tmp, w, h, p->blur_radius, p->blur_ww, p->blur_fw);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ti_blur_kernel<true>, grid, dim3(TI_THREADS), lds, st, (const uint8_t *)tmp, out, w, h, p->blur_radius, p->blur_ww,
                       p->blur_fw);
    SURS_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ host twins

void resample_host(const SursImageResample &r, const char *tables, const uint8_t *rgb, const uint8_t *mask, uint8_t *out_rgb, uint8_t *out_mask,
                   float *out_f) {
    const int32_t *xb = (const int32_t *)(tables + r.off_xb), *xk = (const int32_t *)(tables + r.off_xk);
    const int32_t *yb = (const int32_t *)(tables + r.off_yb), *yk = (const int32_t *)(tables + r.off_yk);
    const int32_t *xn = (const int32_t *)(tables + r.off_xn), *yn = (const int32_t *)(tables + r.off_yn);
    const int in_w = r.src_w + 2 * r.pad;
    std::vector<uint32_t> row(in_w), mid;
    int y_lo = 0, y_hi = 0;
    if (rgb) {
        for (int o = 0; o < r.out_h; ++o) {
            if (!yb[2 * o + 1]) continue;
            if (y_hi == 0) y_lo = yb[2 * o];
            y_lo = yb[2 * o] < y_lo ? yb[2 * o] : y_lo;
            y_hi = yb[2 * o] + yb[2 * o + 1] > y_hi ? yb[2 * o] + yb[2 * o + 1] : y_hi;
        }
        mid.resize((size_t)(y_hi - y_lo) * r.out_w);
        for (int y = y_lo; y < y_hi; ++y) {
            for (int x = 0; x < in_w; ++x) row[x] = ti_fetch_rgb(rgb, r.src_w, r.src_h, r.pad, r.flip, x, y);
            for (int o = 0; o < r.out_w; ++o)
                mid[(size_t)(y - y_lo) * r.out_w + o] = ti_dot(row.data() + xb[2 * o], 1, xk + (size_t)o * r.ksize_x, xb[2 * o + 1]);
        }
    }
    for (int oy = 0; oy < r.out_h; ++oy)
        for (int ox = 0; ox < r.out_w; ++ox) {
            uint32_t v = 0;
            if (rgb && yb[2 * oy + 1])
                v = ti_dot(mid.data() + (size_t)(yb[2 * oy] - y_lo) * r.out_w + ox, r.out_w, yk + (size_t)oy * r.ksize_y, yb[2 * oy + 1]);
            int m = 0;
            if (mask) m = ti_fetch_mask(mask, r.src_w, r.src_h, r.pad, r.flip, xn[ox], yn[oy]);
            const size_t o = (size_t)oy * r.out_w + ox;
            if (out_f)
                for (int ch = 0; ch < 3; ++ch) out_f[o * 3 + ch] = ti_prepare(m, ti_ch(v, ch));
            if (out_rgb) out_rgb[o * 3] = (uint8_t)ti_ch(v, 0), out_rgb[o * 3 + 1] = (uint8_t)ti_ch(v, 1), out_rgb[o * 3 + 2] = (uint8_t)ti_ch(v, 2);
            if (out_mask) out_mask[o] = (uint8_t)m;
        }
}

void jitter_host(const SursTrainImagePlan *p, const uint8_t *in, int w, int h, uint8_t *out) {
    const size_t npix = (size_t)w * h;
    const int at = contrast_at(p);
    const int first_end = at < 0 ? p->n_ops : at;
    unsigned long long sum_l = 0;
    for (size_t i = 0; i < npix; ++i) {
        int r = in[3 * i], g = in[3 * i + 1], b = in[3 * i + 2];
        for (int k = 0; k < first_end; ++k) ti_jitter_op(p->op_kind[k], p->op_factor[k], p->hue_shift, 0, &r, &g, &b);
        out[3 * i] = (uint8_t)r, out[3 * i + 1] = (uint8_t)g, out[3 * i + 2] = (uint8_t)b;
        sum_l += (unsigned)ti_luma(r, g, b);
    }
    if (at < 0) return;
    const int mean = ti_contrast_mean(sum_l, (long long)npix);
    for (size_t i = 0; i < npix; ++i) {
        int r = out[3 * i], g = out[3 * i + 1], b = out[3 * i + 2];
        for (int k = at; k < p->n_ops; ++k) ti_jitter_op(p->op_kind[k], p->op_factor[k], p->hue_shift, mean, &r, &g, &b);
        out[3 * i] = (uint8_t)r, out[3 * i + 1] = (uint8_t)g, out[3 * i + 2] = (uint8_t)b;
    }
}

void blur_host(const SursTrainImagePlan *p, const uint8_t *in, int w, int h, uint8_t *out) {
    const size_t npix = (size_t)w * h;
    std::vector<uint32_t> a(npix), b(npix);
    for (size_t i = 0; i < npix; ++i) a[i] = ti_pack(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
    if (p->blur_ww) {
        for (int pass = 0; pass < 3; ++pass) {
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) b[(size_t)y * w + x] = ti_box(a.data() + (size_t)y * w, 1, 0, x, w, p->blur_radius, p->blur_ww, p->blur_fw);
            a.swap(b);
        }
        for (int pass = 0; pass < 3; ++pass) {
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) b[(size_t)y * w + x] = ti_box(a.data() + x, w, 0, y, h, p->blur_radius, p->blur_ww, p->blur_fw);
            a.swap(b);
        }
    }
    for (size_t i = 0; i < npix; ++i) out[3 * i] = (uint8_t)ti_ch(a[i], 0), out[3 * i + 1] = (uint8_t)ti_ch(a[i], 1), out[3 * i + 2] = (uint8_t)ti_ch(a[i], 2);
}

int chain_args(const SursTrainImagePlan *p, const void *tables, const void *rgb, const void *mask, const void *hr, const void *lr) {
    if (int e = plan_ops_args(p)) return e;
    SURS_REQUIRE(tables && rgb && mask && hr && lr, "tables, rgb, mask, img_hr and img_lr must not be NULL");
    SURS_REQUIRE(p->w >= 2 && p->h >= 2 && p->lr.src_w == p->w && p->lr.src_h == p->h && p->lr.out_w == p->w / 2 && p->lr.out_h == p->h / 2,
                 "a plan that surs_train_image_plan did not fill (HR image %d x %d)", p->w, p->h);
    SURS_REQUIRE(!p->augment || (p->geo.out_w == p->w && p->geo.out_h == p->h), "a plan whose geometry window is not its HR image");
    return 0;
}
}  // namespace

extern "C" int surs_image_resample_plan(int src_w, int src_h, int pad, int flip, int full_w, int full_h, int filter, int x0, int y0, int out_w,
                                        int out_h, SursImageResample *r, void *tables, size_t tables_bytes, size_t base, size_t *used) {
    return resample_plan(src_w, src_h, pad, flip, full_w, full_h, filter, x0, y0, out_w, out_h, r, tables, tables_bytes, base, used);
}

extern "C" int surs_train_image_plan(int src_w, int src_h, int augment, int pad, int flip, int full_w, int full_h, int x0, int y0, int out_w,
                                     int out_h, const int *order, const double *factor, int active, double blur_radius,
                                     SursTrainImagePlan *plan, void *tables, size_t tables_bytes) {
    SURS_REQUIRE(plan, "plan must not be NULL");
    SursTrainImagePlan p;
    memset(&p, 0, sizeof(p));
    p.augment = augment ? 1 : 0;
    size_t base = 0, used = 0;
    if (p.augment) {
        SURS_REQUIRE(order && factor, "order and factor must not be NULL");
        int seen = 0;
        for (int i = 0; i < 4; ++i) {
            SURS_REQUIRE(order[i] >= 0 && order[i] <= 3 && !(seen & (1 << order[i])), "order is no permutation of 0..3");
            seen |= 1 << order[i];
        }
        for (int i = 0; i < 4; ++i) {
            const int k = order[i];
            if (!(active & (1 << k))) continue;
            SURS_REQUIRE(std::isfinite(factor[k]), "jitter factor %d is not finite", k);
            p.op_kind[p.n_ops] = k;
            p.op_factor[p.n_ops] = k == SURS_JITTER_HUE ? 0.0f : (float)factor[k];
            if (k == SURS_JITTER_HUE) p.hue_shift = (int)(factor[k] * 255.0) & 255;
            ++p.n_ops;
        }
        SURS_REQUIRE(blur_radius >= 0.0 && blur_radius < 1e4, "a blur radius of %g", blur_radius);
        blur_constants(blur_radius, &p.blur_radius, &p.blur_ww, &p.blur_fw);
        SURS_REQUIRE(p.blur_radius <= TI_BLUR_MAX_RADIUS, "a blur radius of %g makes a box radius of %d per pass: at most %d", blur_radius,
                     p.blur_radius, TI_BLUR_MAX_RADIUS);
        if (int e = resample_plan(src_w, src_h, pad, flip, full_w, full_h, SURS_FILTER_BILINEAR, x0, y0, out_w, out_h, &p.geo, tables,
                                  tables_bytes, 0, &used))
            return e;
        base = used;
        p.w = out_w, p.h = out_h;
    } else {
        p.w = src_w, p.h = src_h;
    }
    SURS_REQUIRE(p.w >= 2 && p.h >= 2, "an HR image of %d x %d has no half-size image", p.w, p.h);
    if (int e = resample_plan(p.w, p.h, 0, 0, p.w / 2, p.h / 2, SURS_FILTER_BICUBIC, 0, 0, p.w / 2, p.h / 2, &p.lr, tables, tables_bytes, base,
                              &used))
        return e;
    p.tables_bytes = base + used;
    *plan = p;
    return 0;
}

extern "C" size_t surs_train_images_workspace_bytes(const SursTrainImagePlan *plan) {
    if (!plan || plan->w < 1 || plan->h < 1) return 0;
    return 2 * image_bytes(plan->w, plan->h) + mask_bytes(plan->w, plan->h) + partial_bytes(plan->w, plan->h);
}

extern "C" int surs_train_images(const SursTrainImagePlan *plan, const void *tables, const unsigned char *rgb, const unsigned char *mask,
                                 void *workspace, size_t workspace_bytes, float *img_hr, float *img_lr, void *stream) {
    if (int e = chain_args(plan, tables, rgb, mask, img_hr, img_lr)) return e;
    const size_t need = surs_train_images_workspace_bytes(plan);
    SURS_REQUIRE(workspace && workspace_bytes >= need, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int w = plan->w, h = plan->h;
    uint8_t *buf_a = (uint8_t *)workspace, *buf_b = buf_a + image_bytes(w, h), *mask_hr = buf_b + image_bytes(w, h);
    uint32_t *partials = (uint32_t *)(mask_hr + mask_bytes(w, h));
    const uint8_t *render = rgb, *mask_cur = mask;
    if (plan->augment) {
        if (int e = launch_resample(false, plan->geo, tables, rgb, mask, buf_a, mask_hr, nullptr, st)) return e;
        render = buf_a, mask_cur = mask_hr;
        if (plan->n_ops)
            if (int e = launch_jitter(plan, buf_a, w, h, partials, buf_a, st)) return e;
        if (plan->blur_ww)   // x passes into buf_b, y passes back
            if (int e = launch_blur(plan, buf_a, w, h, buf_b, buf_a, st)) return e;
    }
    if (int e = launch_resample(true, plan->lr, tables, render, mask_cur, nullptr, nullptr, img_lr, st)) return e;
    return surs_image_prepare(render, mask_cur, h, w, img_hr, 3, stream);
}

extern "C" int surs_image_resample(const SursImageResample *r, const void *tables, const unsigned char *rgb, unsigned char *out, void *stream) {
    if (int e = resample_args(r, tables, rgb, out)) return e;
    return launch_resample(false, *r, tables, rgb, nullptr, out, nullptr, nullptr, as_stream(stream));
}

extern "C" int surs_image_nearest(const SursImageResample *r, const void *tables, const unsigned char *mask, unsigned char *out, void *stream) {
    if (int e = resample_args(r, tables, mask, out)) return e;
    return launch_resample(false, *r, tables, nullptr, mask, nullptr, out, nullptr, as_stream(stream));
}

extern "C" int surs_image_jitter(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, void *workspace,
                                 size_t workspace_bytes, unsigned char *out, void *stream) {
    if (int e = plan_ops_args(plan)) return e;
    if (int e = image_args(rgb, w, h, out)) return e;
    SURS_REQUIRE(workspace && workspace_bytes >= partial_bytes(w, h), "workspace of %zu bytes, %zu needed", workspace_bytes, partial_bytes(w, h));
    return launch_jitter(plan, rgb, w, h, (uint32_t *)workspace, out, as_stream(stream));
}

extern "C" int surs_image_blur(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, unsigned char *tmp, unsigned char *out,
                               void *stream) {
    if (int e = plan_ops_args(plan)) return e;
    if (int e = image_args(rgb, w, h, out)) return e;
    SURS_REQUIRE(tmp && tmp != rgb && tmp != out && rgb != out, "rgb, tmp and out must be three distinct arrays");
    if (!plan->blur_ww) {
        SURS_HIP_CHECK(hipMemcpyAsync(out, rgb, (size_t)w * h * 3, hipMemcpyDeviceToDevice, as_stream(stream)));
        return 0;
    }
    return launch_blur(plan, rgb, w, h, tmp, out, as_stream(stream));
}

extern "C" int surs_train_images_host(const SursTrainImagePlan *plan, const void *tables, const unsigned char *rgb, const unsigned char *mask,
                                      float *img_hr, float *img_lr) {
    if (int e = chain_args(plan, tables, rgb, mask, img_hr, img_lr)) return e;
    const int w = plan->w, h = plan->h;
    std::vector<uint8_t> buf_a, buf_b, mask_hr;
    const uint8_t *render = rgb, *mask_cur = mask;
    if (plan->augment) {
        buf_a.resize((size_t)w * h * 3), mask_hr.resize((size_t)w * h);
        resample_host(plan->geo, (const char *)tables, rgb, mask, buf_a.data(), mask_hr.data(), nullptr);
        if (plan->n_ops) jitter_host(plan, buf_a.data(), w, h, buf_a.data());
        if (plan->blur_ww) {
            buf_b.resize((size_t)w * h * 3);
            blur_host(plan, buf_a.data(), w, h, buf_b.data());
            buf_a.swap(buf_b);
        }
        render = buf_a.data(), mask_cur = mask_hr.data();
    }
    resample_host(plan->lr, (const char *)tables, render, mask_cur, nullptr, nullptr, img_lr);
    for (size_t i = 0; i < (size_t)w * h; ++i)
        for (int ch = 0; ch < 3; ++ch) img_hr[3 * i + ch] = ti_prepare(mask_cur[i], render[3 * i + ch]);
    return 0;
}

extern "C" int surs_image_resample_host(const SursImageResample *r, const void *tables, const unsigned char *rgb, unsigned char *out) {
    if (int e = resample_args(r, tables, rgb, out)) return e;
    resample_host(*r, (const char *)tables, rgb, nullptr, out, nullptr, nullptr);
    return 0;
}

extern "C" int surs_image_nearest_host(const SursImageResample *r, const void *tables, const unsigned char *mask, unsigned char *out) {
    if (int e = resample_args(r, tables, mask, out)) return e;
    resample_host(*r, (const char *)tables, nullptr, mask, nullptr, out, nullptr);
    return 0;
}

extern "C" int surs_image_jitter_host(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, unsigned char *out) {
    if (int e = plan_ops_args(plan)) return e;
    if (int e = image_args(rgb, w, h, out)) return e;
    jitter_host(plan, rgb, w, h, out);
    return 0;
}

extern "C" int surs_image_blur_host(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, unsigned char *out) {
    if (int e = plan_ops_args(plan)) return e;
    if (int e = image_args(rgb, w, h, out)) return e;
    blur_host(plan, rgb, w, h, out);
    return 0;
}

extern "C" int surs_image_hsv_host(const unsigned char *in, long long n, int inverse, unsigned char *out) {
    SURS_REQUIRE(in && out && n >= 0, "in and out must not be NULL");
    for (long long i = 0; i < n; ++i) {
        int a, b, c;
        if (inverse)
            ti_hsv2rgb(in[3 * i], in[3 * i + 1], in[3 * i + 2], &a, &b, &c);
        else
            ti_rgb2hsv(in[3 * i], in[3 * i + 1], in[3 * i + 2], &a, &b, &c);
        out[3 * i] = (uint8_t)a, out[3 * i + 1] = (uint8_t)b, out[3 * i + 2] = (uint8_t)c;
    }
    return 0;
}
