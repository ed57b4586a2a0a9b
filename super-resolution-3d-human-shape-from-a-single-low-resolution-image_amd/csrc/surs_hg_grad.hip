// Backward primitives of the hourglass encoder (image_filter_lr) for gfx950 (MI355X): include/surs.h, "hourglass gradients".
//   surs_groupnorm_fold        GroupNorm(32) statistics (a SursGnStats, or none: the map itself) -> mean[32], rstd[32], scale[c], shift[c]
//   surs_groupnorm_relu_grad   the backward of out = relu(GroupNorm32(x; gamma, beta)): dx (+)=, dgamma, dbeta
//   surs_avgpool2_grad         the transpose of surs_avgpool2
//   surs_bicubic_up2_grad      the transpose of surs_bicubic_up2(align_corners = 1)
// The convolutions between them are surs_sr_grad.hip's.  fp32 with fp32 accumulation, no atomics, every sum in an order that depends
// on the shapes alone: two calls give the same bits wherever the buffers lie.
//
// The ReLU mask is RECOMPUTED: z = x * scale + shift with the forward's own fp32 coefficients, in the expression of the convolutions'
// staging (surs_encoder.hip: fmaxf(v * scale + shift, 0.f), a multiply and an add - the library is built with -ffp-contract=off), so
// the backward's mask is the forward's, element for element; z == 0 and z == -0 take the negative side.  gn_affine() below is that
// expression; the coefficient arithmetic of surs_groupnorm_fold is gn_fold_to_lds' (statistics) / gn_finish_kernel's (none) of
// surs_encoder.hip, operation for operation, so that scale and shift come out with the bits the forward's kernels formed in LDS.
//
// GroupNorm + ReLU backward, m = hw * c / 32 elements per group, xh = (x - mean) * rstd, gy = g where z > 0 else 0:
//   dgamma[c] = sum_p gy xh          dbeta[c] = sum_p gy
//   s1[grp] = sum_{c in grp} gamma[c] dbeta[c]      s2[grp] = sum_{c in grp} gamma[c] dgamma[c]
//   dx = rstd * (gy * gamma - s1 / m - xh * s2 / m)
// Reduction pass: the pixels are cut into parts of GG_PART = 64 consecutive pixels; workgroup z reads g and x of its part once (16
// bytes per lane: a lane keeps one channel quad and walks the part's pixels 256 / (c / 4) apart), folds its pixel lanes in lane
// order through LDS and writes [c][2] sums to slab z; ggrad_finish_kernel adds slab 0, 1, 2, ... in this order per channel, stores
// (or adds, accumulate = 1) dgamma / dbeta and forms s1 / m, s2 / m per group over the group's channels in channel order.  Apply
// pass: one lane per pixel and channel quad reads g and x once and writes dx once.
#include <hip/hip_runtime.h>

#include "surs_common.h"

namespace surs {
namespace hggrad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GG_PART = 64;   // pixels per part of the GroupNorm gradient's reduction (include/surs.h)

// the GroupNorm + ReLU pre-activation as the convolutions' staging forms it (surs_encoder.hip)
__device__ __forceinline__ float gn_affine(float v, float scale, float shift) { return v * scale + shift; }

// ---------------------------------------------------------------- surs_groupnorm_fold
struct FoldArgs {
    const double *sums; int pitch, g1, g2, slots0, slots1, slots2;
    int hw, c; float eps;
    const float *gamma, *beta;
    float *mean, *rstd, *scale, *shift;
};

// one workgroup of 256: gn_fold_to_lds' arithmetic (eight threads per group, thread `sub` adds the slots sub, sub + 8, ... in order,
// then a butterfly over the eight)
__global__ __launch_bounds__(256) void fold_stats_kernel(FoldArgs a) {
    const int tid = threadIdx.x, g = tid >> 3, sub = tid & 7, cgi = a.c / 32;
    const int slots = (a.g1 <= 0 || g < a.g1) ? a.slots0 : (g < a.g2 ? a.slots1 : a.slots2);
    const double2 *pg = reinterpret_cast<const double2 *>(a.sums) + (size_t)g * (a.pitch > 0 ? a.pitch : a.slots0);
    double S = 0, SS = 0;
    for (int base = 0; base < slots; base += 64) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int sl = base + sub + 8 * u;
            v[u] = sl < slots ? pg[sl] : double2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            S += v[u].x;
            SS += v[u].y;
        }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        S += __shfl_xor(S, o);
        SS += __shfl_xor(SS, o);
    }
    const double n = (double)a.hw * cgi;
    const double mean = S / n;
    double var = SS / n - mean * mean;
    if (var < 0) var = 0;
    const double rstd = 1.0 / sqrt(var + (double)a.eps);
    if (sub == 0) {
        a.mean[g] = (float)mean;
        a.rstd[g] = (float)rstd;
    }
    for (int k = sub; k < cgi; k += 8) {
        const int ch = g * cgi + k;
        a.scale[ch] = (float)(rstd * a.gamma[ch]);
        a.shift[ch] = (float)(a.beta[ch] - mean * rstd * a.gamma[ch]);
    }
}

// a map without statistics: the partial sums surs_groupnorm_coeffs_ws left in its scratch ([32][split][2] doubles), folded as its
// second launch folds them (one wave per group: lane l adds partials l, l + 64, ... in order, then a butterfly from 32 down)
__global__ __launch_bounds__(64) void fold_partials_kernel(const double *__restrict__ partial, int split, int hw, int c, float eps,
                                                           float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    const int g = blockIdx.x, lane = threadIdx.x, cg = c / 32;
    double S = 0, SS = 0;
    for (int sp = lane; sp < split; sp += 64) {
        S += partial[((size_t)g * split + sp) * 2 + 0];
        SS += partial[((size_t)g * split + sp) * 2 + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        S += __shfl_xor(S, o);
        SS += __shfl_xor(SS, o);
    }
    const double n = (double)hw * cg;
    const double mean = S / n;
    double var = SS / n - mean * mean;
    if (var < 0) var = 0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    if (lane == 0) {
        mean_out[g] = (float)mean;
        rstd_out[g] = (float)rstd;
    }
}

// ---------------------------------------------------------------- surs_groupnorm_relu_grad
struct GgArgs {
    const float *g, *x;       // [hw][c], pitches g_ld, x_ld
    int hw, c, g_ld, x_ld;
    const float *mean, *rstd, *scale, *shift, *gamma;
    float *part;              // [parts][c][2]
    float *coef;              // [32][2]: s1 / m, s2 / m
    float *dx; int dx_ld, add;
};

// grid: parts; 256 threads = (256 / (c / 4)) pixel lanes x (c / 4) channel quads
__global__ __launch_bounds__(256) void ggrad_reduce_kernel(GgArgs a) {
    __shared__ float red[256][8];
    const int tid = threadIdx.x, c4 = a.c / 4, ppl = 256 / c4, q = tid % c4, pl = tid / c4, cg = a.c / 32;
    const int p0 = (int)blockIdx.x * GG_PART, p1 = min(a.hw, p0 + GG_PART);
    const f32x4 sc = *reinterpret_cast<const f32x4 *>(a.scale + 4 * q), sh = *reinterpret_cast<const f32x4 *>(a.shift + 4 * q);
    float mq[4], rq[4];   // (64 channels: a quad holds two groups)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mq[k] = a.mean[(4 * q + k) / cg];
        rq[k] = a.rstd[(4 * q + k) / cg];
    }
    float sb[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = p0 + pl; p < p1; p += ppl) {
        const f32x4 gv = *reinterpret_cast<const f32x4 *>(a.g + (size_t)p * a.g_ld + 4 * q);
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(a.x + (size_t)p * a.x_ld + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gy = gn_affine(xv[k], sc[k], sh[k]) > 0.f ? gv[k] : 0.f;
            const float xh = (xv[k] - mq[k]) * rq[k];
            sb[k] += gy;
            sg[k] += gy * xh;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        red[tid][k] = sb[k];
        red[tid][4 + k] = sg[k];
    }
    __syncthreads();
    for (int ch = tid; ch < a.c; ch += 256) {   // the pixel lanes of channel ch, in lane order
        float B = 0.f, G = 0.f;
        for (int l = 0; l < ppl; ++l) {
            B += red[l * c4 + ch / 4][ch % 4];
            G += red[l * c4 + ch / 4][4 + ch % 4];
        }
        float *o = a.part + ((size_t)blockIdx.x * a.c + ch) * 2;
        o[0] = B;
        o[1] = G;
    }
}

// one workgroup of c threads: slab 0 + slab 1 + ... per channel, then the group sums over the group's channels in channel order
__global__ __launch_bounds__(256) void ggrad_finish_kernel(const float *__restrict__ part, int parts, int c, int hw,
                                                           const float *__restrict__ gamma, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta, int accumulate, float *__restrict__ coef) {
    __shared__ float wb[256], wg[256];
    const int ch = threadIdx.x, cg = c / 32;
    if (ch < c) {
        float B = part[(size_t)ch * 2], G = part[(size_t)ch * 2 + 1];
        for (int z = 1; z < parts; ++z) {
            B += part[((size_t)z * c + ch) * 2];
            G += part[((size_t)z * c + ch) * 2 + 1];
        }
        dbeta[ch] = accumulate ? dbeta[ch] + B : B;
        dgamma[ch] = accumulate ? dgamma[ch] + G : G;
        wb[ch] = gamma[ch] * B;
        wg[ch] = gamma[ch] * G;
    }
    __syncthreads();
    if (ch < 32) {
        float s1 = 0.f, s2 = 0.f;
        for (int k = 0; k < cg; ++k) {
            s1 += wb[ch * cg + k];
            s2 += wg[ch * cg + k];
        }
        const float m = (float)hw * (float)cg;
        coef[2 * ch] = s1 / m;
        coef[2 * ch + 1] = s2 / m;
    }
}

// one thread per pixel and channel quad
__global__ __launch_bounds__(256) void ggrad_apply_kernel(GgArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = a.c / 4, cg = a.c / 32;
    if (i >= (long long)a.hw * c4) return;
    const long long p = i / c4;
    const int q = (int)(i - p * c4);
    const f32x4 gv = *reinterpret_cast<const f32x4 *>(a.g + p * a.g_ld + 4 * q);
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(a.x + p * a.x_ld + 4 * q);
    const f32x4 sc = *reinterpret_cast<const f32x4 *>(a.scale + 4 * q), sh = *reinterpret_cast<const f32x4 *>(a.shift + 4 * q);
    const f32x4 ga = *reinterpret_cast<const f32x4 *>(a.gamma + 4 * q);
    float *d = a.dx + p * a.dx_ld + 4 * q;
    f32x4 r;
    if (a.add) r = *reinterpret_cast<const f32x4 *>(d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int grp = (4 * q + k) / cg;
        const float rstd = a.rstd[grp];
        const float gy = gn_affine(xv[k], sc[k], sh[k]) > 0.f ? gv[k] : 0.f;
        const float xh = (xv[k] - a.mean[grp]) * rstd;
        const float v = rstd * (gy * ga[k] - a.coef[2 * grp] - xh * a.coef[2 * grp + 1]);
        r[k] = a.add ? r[k] + v : v;
    }
    *reinterpret_cast<f32x4 *>(d) = r;
}

// ---------------------------------------------------------------- surs_avgpool2_grad: one thread per element quad of dx
__global__ __launch_bounds__(256) void avgpool2_grad_kernel(const float *__restrict__ g, int h, int w, int c, int g_ld, float *__restrict__ dx,
                                                            int dx_ld, int add) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = c / 4, W = 2 * w;
    if (i >= (long long)(2 * h) * W * c4) return;
    const long long pix = i / c4;
    const int q = (int)(i - pix * c4), y = (int)(pix / W), x = (int)(pix - (long long)y * W);
    const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + ((long long)(y >> 1) * w + (x >> 1)) * g_ld + 4 * q);
    float *d = dx + pix * dx_ld + 4 * q;
    f32x4 r;
    if (add) r = *reinterpret_cast<const f32x4 *>(d);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = add ? r[k] + 0.25f * gv[k] : 0.25f * gv[k];
    *reinterpret_cast<f32x4 *>(d) = r;
}

// ---------------------------------------------------------------- surs_bicubic_up2_grad
// cubic_coeffs of surs_encoder.hip (PyTorch's cubic convolution, A = -0.75), expression for expression
__device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
    const float A = -0.75f;
    float x = t + 1.0f;
    c[0] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
    x = t;
    c[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    x = 1.0f - t;
    c[2] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    x = 2.0f - t;
    c[3] = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}

// the weight output coordinate o of an axis (n -> 2 n, align_corners) puts on source pixel s: the forward's coordinate and coefficient
// expressions, its clamped taps that fall on s summed in tap order
__device__ __forceinline__ float up2_weight(int o, int s, int n, float step) {
    const float r = step * (float)o;
    const int i0 = (int)floorf(r);
    float cf[4];
    cubic_coeffs(r - (float)i0, cf);
    float wsum = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (min(max(i0 - 1 + a, 0), n - 1) == s) wsum += cf[a];
    return wsum;
}

// the output coordinates that can reach source pixel s: floor(step o) - 1 <= s <= floor(step o) + 2 before clamping, one more on
// each side for the rounding of step o; step == 0 (n == 1): all of them
__device__ __forceinline__ void up2_range(int s, int n, float step, int &lo, int &hi) {
    const int no = 2 * n;
    if (step <= 0.f) {
        lo = 0;
        hi = no - 1;
        return;
    }
    lo = max(0, (int)floorf((float)(s - 2) / step) - 1);
    hi = min(no - 1, (int)ceilf((float)(s + 2) / step) + 1);
}

constexpr int UP2_TAPS = 20;   // 4 / step + 4 <= 16 output coordinates per source pixel (step >= 1 / 3 for n >= 2), with room

// gather form: one thread per source pixel and channel quad; output rows ascending, output columns ascending inside a row
__global__ __launch_bounds__(256) void bicubic_up2_grad_kernel(const float *__restrict__ g, int h, int w, int c, int g_ld,
                                                               float *__restrict__ dx, int dx_ld, int add) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = c / 4, ho = 2 * h, wo = 2 * w;
    if (i >= (long long)h * w * c4) return;
    const long long pix = i / c4;
    const int q = (int)(i - pix * c4), sy = (int)(pix / w), sx = (int)(pix - (long long)sy * w);
    const float ystep = ho > 1 ? (float)(h - 1) / (float)(ho - 1) : 0.f;
    const float xstep = wo > 1 ? (float)(w - 1) / (float)(wo - 1) : 0.f;
    int ylo, yhi, xlo, xhi;
    up2_range(sy, h, ystep, ylo, yhi);
    up2_range(sx, w, xstep, xlo, xhi);
    xhi = min(xhi, xlo + UP2_TAPS - 1);
    float wx[UP2_TAPS];
#pragma unroll
    for (int b = 0; b < UP2_TAPS; ++b) wx[b] = xlo + b <= xhi ? up2_weight(xlo + b, sx, w, xstep) : 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = up2_weight(oy, sy, h, ystep);
        if (wy == 0.f) continue;
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < UP2_TAPS; ++b) {
            if (xlo + b > xhi || wx[b] == 0.f) continue;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(g + ((long long)oy * wo + xlo + b) * g_ld + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] += wx[b] * v[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += wy * r[k];
    }
    float *d = dx + pix * dx_ld + 4 * q;
    if (add) {
        const f32x4 o = *reinterpret_cast<const f32x4 *>(d);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = o[k] + acc[k];
    }
    *reinterpret_cast<f32x4 *>(d) = acc;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace hggrad
}  // namespace surs

using namespace surs;
using namespace surs::hggrad;

extern "C" int surs_groupnorm_fold(const SursGnStats *stats, const float *x, int hw, int c, int x_ld, float eps, const float *gamma,
                                   const float *beta, float *mean, float *rstd, float *scale, float *shift, void *scratch, void *stream) {
    SURS_REQUIRE(gamma && beta && mean && rstd && scale && shift, "groupnorm_fold: null argument");
    SURS_REQUIRE(hw >= 1 && c >= 32 && c <= 1024 && c % 32 == 0, "groupnorm_fold: GroupNorm(32) of 32..1024 channels, a multiple of 32");
    if (stats && stats->sums) {
        SURS_REQUIRE(stats->slots[0] > 0 && (stats->g1 <= 0 || (stats->g1 <= stats->g2 && stats->g2 <= 32 && stats->slots[1] > 0 &&
                                                                 stats->slots[2] > 0)),
                     "groupnorm_fold: bad statistics");
        FoldArgs a{stats->sums, stats->pitch, stats->g1, stats->g2, stats->slots[0], stats->slots[1], stats->slots[2], hw, c, eps,
                   gamma, beta, mean, rstd, scale, shift};
        hipLaunchKernelGGL(fold_stats_kernel, dim3(1), dim3(256), 0, as_stream(stream), a);
        SURS_LAUNCH_CHECK();
        return 0;
    }
    SURS_REQUIRE(x && scratch, "groupnorm_fold: a map without statistics needs the map and surs_groupnorm_scratch_bytes() of scratch");
    if (int rc = surs_groupnorm_coeffs_ws(x, hw, c, x_ld, 32, eps, gamma, beta, scale, shift, scratch, stream)) return rc;
    const int split = (int)(surs_groupnorm_scratch_bytes() / (sizeof(double) * 64 * 2));
    hipLaunchKernelGGL(fold_partials_kernel, dim3(32), dim3(64), 0, as_stream(stream), (const double *)scratch, split, hw, c, eps, mean, rstd);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t surs_groupnorm_relu_grad_workspace_bytes(int hw, int c) {
    if (hw < 1 || (c != 64 && c != 128 && c != 256)) return 0;
    const size_t parts = ((size_t)hw + GG_PART - 1) / GG_PART;
    return (parts * c * 2 + 64) * sizeof(float) + 256;
}

extern "C" int surs_groupnorm_relu_grad(const float *g, int g_ld, const float *x, int x_ld, int hw, int c, const float *mean,
                                        const float *rstd, const float *scale, const float *shift, const float *gamma, float *dx,
                                        int dx_ld, int add, float *dgamma, float *dbeta, int accumulate, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    SURS_REQUIRE(g && x && mean && rstd && scale && shift && gamma && dx && dgamma && dbeta && workspace, "groupnorm_relu_grad: null argument");
    SURS_REQUIRE(hw >= 1 && (c == 64 || c == 128 || c == 256), "groupnorm_relu_grad: %d channels (64, 128 and 256 are supported)", c);
    SURS_REQUIRE((long long)hw * 64 < (1ll << 31), "groupnorm_relu_grad: shape too large");
    SURS_REQUIRE(g_ld >= c && x_ld >= c && dx_ld >= c && g_ld % 4 == 0 && x_ld % 4 == 0 && dx_ld % 4 == 0 && aligned16(g) && aligned16(x) &&
                 aligned16(dx) && aligned16(scale) && aligned16(shift) && aligned16(gamma),
                 "groupnorm_relu_grad: pitches of at least c and multiples of 4, 16-byte aligned pixels and vectors");
    const size_t need = surs_groupnorm_relu_grad_workspace_bytes(hw, c);
    char *base = (char *)align_up((size_t)workspace, 256);
    SURS_REQUIRE(need - 256 + (size_t)(base - (char *)workspace) <= workspace_bytes, "groupnorm_relu_grad: workspace too small: %zu bytes needed", need);
    const int parts = ceil_div(hw, GG_PART);
    float *coef = (float *)base, *part = coef + 64;
    GgArgs a{g, x, hw, c, g_ld, x_ld, mean, rstd, scale, shift, gamma, part, coef, dx, dx_ld, add ? 1 : 0};
    hipLaunchKernelGGL(ggrad_reduce_kernel, dim3(parts), dim3(256), 0, as_stream(stream), a);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ggrad_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const float *)part, parts, c, hw, gamma, dgamma, dbeta,
                       accumulate ? 1 : 0, coef);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ggrad_apply_kernel, dim3(ceil_div((long long)hw * (c / 4), 256)), dim3(256), 0, as_stream(stream), a);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_avgpool2_grad(const float *g, int h, int w, int c, int g_ld, float *dx, int dx_ld, int add, void *stream) {
    SURS_REQUIRE(g && dx && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "avgpool2_grad: bad argument (c must be a multiple of 4)");
    SURS_REQUIRE(g_ld >= c && dx_ld >= c && g_ld % 4 == 0 && dx_ld % 4 == 0 && aligned16(g) && aligned16(dx),
                 "avgpool2_grad: pitches of at least c and multiples of 4, 16-byte aligned pixels");
    const long long count = 4ll * h * w * (c / 4);
    SURS_REQUIRE(count < (1ll << 31) * 256, "avgpool2_grad: shape too large");
    hipLaunchKernelGGL(avgpool2_grad_kernel, dim3(ceil_div(count, 256)), dim3(256), 0, as_stream(stream), g, h, w, c, g_ld, dx, dx_ld, add ? 1 : 0);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_bicubic_up2_grad(const float *g, int h, int w, int c, int g_ld, float *dx, int dx_ld, int add, void *stream) {
    SURS_REQUIRE(g && dx && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "bicubic_up2_grad: bad argument (c must be a multiple of 4)");
    SURS_REQUIRE(g_ld >= c && dx_ld >= c && g_ld % 4 == 0 && dx_ld % 4 == 0 && aligned16(g) && aligned16(dx),
                 "bicubic_up2_grad: pitches of at least c and multiples of 4, 16-byte aligned pixels");
    const long long count = (long long)h * w * (c / 4);
    SURS_REQUIRE(count < (1ll << 31) * 256 && h < (1 << 20) && w < (1 << 20), "bicubic_up2_grad: shape too large");
    hipLaunchKernelGGL(bicubic_up2_grad_kernel, dim3(ceil_div(count, 256)), dim3(256), 0, as_stream(stream), g, h, w, c, g_ld, dx, dx_ld,
                       add ? 1 : 0);
    SURS_LAUNCH_CHECK();
    return 0;
}
