// Backward primitives of the super-resolution network's convolutions for gfx950 (MI355X): include/surs.h, "super-resolution
// gradients".  Three entry points:
//   surs_conv_grad_weight       dW[co][ci][ky][kx] = sum_p dZ[p][co] X[p stride + (ky, kx) - pad][ci],  db[co] = sum_p dZ[p][co]
//   surs_conv_grad_input        dX[q][ci] (+)= sum_{co, ky, kx} dZ[(q + pad - (ky, kx)) / stride][co] W[co][ci][ky][kx]
//   surs_pixel_unshuffle2_grad  the transpose of surs_pixel_shuffle2 with the derivative of its two LeakyReLUs
// with dZ[p][co] = g[p][co] * (y[p][co] > 0 ? 1 : slope) formed WHILE the operand is staged (y: the layer's stored output, nullable):
// no activation derivative is a pass of its own.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 on fp32 operands with fp32 accumulation, whatever --precision says (gradient operands reach
// 1e-12, where an f16 operand split flushes to zero).  Both products are implicit GEMMs on the tile of surs_grad_tile.h, which
// describes its LDS layout, bank conflicts, pipeline and edge rule; the input gradient stages A k-contiguously (walk_k).
//   weight gradient   rows: co;  columns: n = tap * cin + ci, plus ONE column (n = k k cin) whose B operand is 1: the bias gradient is
//                     a column of the same product, in the same order.  Reduction: the output pixels, in parts of SG_PART = 1024
//                     pixels in row-major order (parts = ceil(ho wo / 1024): a function of the map size alone).  Part z writes its
//                     [cout][k k cin + 1] tile set to slab z of the workspace; wgrad_reduce_kernel adds slab 0, 1, 2, ... in this order
//                     and stores (or adds, accumulate = 1) into the plain torch layout.
//   input gradient    rows: the input pixels;  columns: ci;  reduction: k = tap * cout + co, taps in (ky, kx) order, one workgroup
//                     per output tile walks all of it in order.  Stride 2 is the transposed form: a tap contributes where
//                     q + pad - (ky, kx) is even in both coordinates.  The weights are read in place from the plain layout.
// Determinism: no atomics; every sum is taken in the order above, which depends on the shapes alone - two calls give the same bits
// wherever the buffers lie.
#include <hip/hip_runtime.h>

#include "surs_common.h"
#include "surs_grad_tile.h"

namespace surs {
namespace srgrad {

constexpr int SG_PART = 1024;   // output pixels per part of the weight gradient's reduction (include/surs.h)

struct WArgs {
    const float *g, *y, *x;   // g, y [ho][wo][cout] (pitches g_ld, y_ld; y nullable), x [h][w][cin] (pitch x_ld)
    int ho, wo, cout, g_ld, y_ld, h, w, cin, x_ld, ks, stride, pad;
    float slope;
    float *part;              // [parts][cout][N]
    int N;                    // ks ks cin + 1
};

// grid: (column tiles, row tiles, parts)
__global__ __launch_bounds__(256) void wgrad_kernel(WArgs a) {
    __shared__ float As[GT_KT][GT_LDS], Bs[GT_KT][GT_LDS];
    const TileLanes t = tile_lanes();
    const int m0 = blockIdx.y * GT_TILE, n0 = blockIdx.x * GT_TILE;
    const int P = a.ho * a.wo;
    const int kbeg = (int)blockIdx.z * SG_PART, kend = min(P, kbeg + SG_PART);
    // both operands are staged along the row (walk_rows): this thread's row / column is the same for every j
    const int co = m0 + walk_rows(t.tid, 0).row, n = n0 + walk_rows(t.tid, 0).row;
    const bool co_ok = co < a.cout;
    const int nw = a.ks * a.ks * a.cin;
    const int tap = n < nw ? n / a.cin : 0, ci = n < nw ? n - tap * a.cin : 0;
    const int ky = tap / a.ks - a.pad, kx = tap % a.ks - a.pad;
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = k0 + walk_rows(t.tid, j).k;
            float va = 0.0f, vb = 0.0f;
            if (p < kend) {
                if (co_ok) {
                    va = a.g[(long long)p * a.g_ld + co];
                    if (a.y) va = dleaky(va, a.y[(long long)p * a.y_ld + co], a.slope);
                }
                if (n < nw) {
                    const int oy = p / a.wo, ox = p - oy * a.wo;
                    const int iy = oy * a.stride + ky, ix = ox * a.stride + kx;
                    if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) vb = a.x[((long long)iy * a.w + ix) * a.x_ld + ci];
                } else if (n == nw) {
                    vb = 1.0f;
                }
            }
            ra[j] = va;
            rb[j] = vb;
        }
    };
    const f32x16 acc = tile_product<false, false>(As, Bs, zero16(), t, kbeg, kend, ra, rb, fetch);
    const int col = n0 + t.wn * 32 + t.li;
    if (col >= a.N) return;
    float *C = a.part + (long long)blockIdx.z * a.cout * a.N;
    for_each_acc(acc, t, m0 + t.wm * 32, [&](int row, float v) {
        if (row < a.cout) C[(long long)row * a.N + col] = v;
    });
}

// second stage: slab 0 + slab 1 + ... in this order, into the plain layout [cout][cin][ks][ks] and db [cout]
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, int parts, int cout, int cin, int kk, int N,
                                                           float *__restrict__ dw, float *__restrict__ db, int accumulate) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, count = (long long)cout * N;
    if (i >= count) return;
    const float s = sum_slabs(part, count, parts, i);
    const int m = (int)(i / N), n = (int)(i - (long long)m * N);
    float *dst;
    if (n == kk * cin) {
        if (!db) return;
        dst = db + m;
    } else {
        const int tap = n / cin, ci = n - tap * cin;
        dst = dw + ((long long)m * cin + ci) * kk + tap;
    }
    *dst = accumulate ? *dst + s : s;
}

struct DArgs {
    const float *g, *y, *wt;  // g, y [ho][wo][cout]; wt [cout][cin][ks][ks]
    int ho, wo, cout, g_ld, y_ld, h, w, cin, ks, stride, pad;
    float slope;
    float *dx;                // [h][w][cin], pitch dx_ld
    int dx_ld, add;
};

// grid: (row tiles over the input pixels, column tiles over cin)
__global__ __launch_bounds__(256) void dgrad_kernel(DArgs a) {
    __shared__ float As[GT_KT][GT_LDS], Bs[GT_KT][GT_LDS];
    const TileLanes t = tile_lanes();
    const int m0 = blockIdx.x * GT_TILE, n0 = blockIdx.y * GT_TILE;
    const int M = a.h * a.w, K = a.ks * a.ks * a.cout, kk2 = a.ks * a.ks;
    // A: k is the contiguous index (co), walk_k: this thread's k is the same for every j, its rows are 16 apart
    const int ka = walk_k(t.tid, 0).k;
    int qy[4], qx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + walk_k(t.tid, j).row;
        qy[j] = m < M ? m / a.w : -(1 << 20);   // (a row past the map matches no output pixel)
        qx[j] = m < M ? m - qy[j] * a.w : 0;
    }
    // B: walk_rows: this thread's column (ci) is the same for every j
    const int ci = n0 + walk_rows(t.tid, 0).row;
    const bool ci_ok = ci < a.cin;
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + ka;
        const int tap = k / a.cout, co = k - tap * a.cout;
        const int ky = tap / a.ks - a.pad, kx = tap % a.ks - a.pad;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float va = 0.0f;
            const int ny = qy[j] - ky, nx = qx[j] - kx;   // = oy stride, ox stride
            if (k < K && ny >= 0 && nx >= 0 && (a.stride == 1 || ((ny | nx) & 1) == 0)) {
                const int oy = a.stride == 1 ? ny : ny >> 1, ox = a.stride == 1 ? nx : nx >> 1;
                if (oy < a.ho && ox < a.wo) {
                    const long long p = (long long)oy * a.wo + ox;
                    va = a.g[p * a.g_ld + co];
                    if (a.y) va = dleaky(va, a.y[p * a.y_ld + co], a.slope);
                }
            }
            ra[j] = va;
            const int kb = k0 + walk_rows(t.tid, j).k;
            float vb = 0.0f;
            if (kb < K && ci_ok) {
                const int tb = kb / a.cout, cb = kb - tb * a.cout;
                vb = a.wt[((long long)cb * a.cin + ci) * kk2 + tb];
            }
            rb[j] = vb;
        }
    };
    const f32x16 acc = tile_product<true, false>(As, Bs, zero16(), t, 0, K, ra, rb, fetch);
    const int col = n0 + t.wn * 32 + t.li;
    if (col >= a.cin) return;
    for_each_acc(acc, t, m0 + t.wm * 32, [&](int row, float v) {
        if (row >= M) return;
        float *d = a.dx + (long long)row * a.dx_ld + col;
        *d = a.add ? *d + v : v;
    });
}

// dz[y][x][4 c + 2 dy + dx] = g[2 y + dy][2 x + dx][c] * (o[2 y + dy][2 x + dx][c] > 0 ? 1 : slope); one thread per element of dz
__global__ __launch_bounds__(256) void unshuffle2_grad_kernel(const float *__restrict__ g, int h, int w, int c, int g_ld,
                                                              const float *__restrict__ o, int o_ld, float slope, float *__restrict__ dz,
                                                              int dz_ld) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)h * w * 4 * c) return;
    const int k = (int)(i % (4 * c));
    const long long pix = i / (4 * c);
    const int x = (int)(pix % w), y = (int)(pix / w);
    const int ch = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
    const long long op = (long long)(2 * y + dy) * (2 * w) + 2 * x + dx;
    dz[pix * dz_ld + k] = dleaky(g[op * g_ld + ch], o[op * o_ld + ch], slope);
}

static int check_conv(int ho, int wo, int h, int w, int cin, int cout, int ks, int stride) {
    SURS_REQUIRE(ks == 1 || ks == 3, "convolution gradient: kernel size %d (1 and 3 are supported)", ks);
    SURS_REQUIRE(stride == 1 || (stride == 2 && ks == 3), "convolution gradient: stride %d with a %d x %d kernel (1, or 2 with 3 x 3)", stride, ks, ks);
    SURS_REQUIRE(cin >= 1 && cout >= 1 && h >= 1 && w >= 1, "convolution gradient: empty shape");
    const int pad = ks / 2;
    SURS_REQUIRE(ho == (h + 2 * pad - ks) / stride + 1 && wo == (w + 2 * pad - ks) / stride + 1,
                 "convolution gradient: a %d x %d input gives a %d x %d output, not %d x %d", h, w, (h + 2 * pad - ks) / stride + 1,
                 (w + 2 * pad - ks) / stride + 1, ho, wo);
    SURS_REQUIRE((long long)h * w < (1ll << 30) && (long long)ks * ks * cin < (1ll << 24) && cout < (1 << 24), "convolution gradient: shape too large");
    return 0;
}

}  // namespace srgrad
}  // namespace surs

using namespace surs;
using namespace surs::srgrad;

extern "C" size_t surs_conv_grad_weight_workspace_bytes(int ho, int wo, int cin, int cout, int ksize) {
    if (ho < 1 || wo < 1 || cin < 1 || cout < 1 || (ksize != 1 && ksize != 3)) return 0;
    const size_t parts = ((size_t)ho * wo + SG_PART - 1) / SG_PART;
    return parts * cout * ((size_t)ksize * ksize * cin + 1) * sizeof(float) + 256;
}

extern "C" int surs_conv_grad_weight(const float *g, int ho, int wo, int cout, int g_ld, const float *y, int y_ld, float slope,
                                     const float *x, int h, int w, int cin, int x_ld, int ksize, int stride, float *dw, float *db,
                                     int accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    SURS_REQUIRE(g && x && dw && workspace, "convolution weight gradient: null argument");
    if (int rc = check_conv(ho, wo, h, w, cin, cout, ksize, stride)) return rc;
    SURS_REQUIRE(g_ld >= cout && x_ld >= cin && (!y || y_ld >= cout), "convolution weight gradient: a pitch below the channel count");
    const size_t need = surs_conv_grad_weight_workspace_bytes(ho, wo, cin, cout, ksize);
    char *base = (char *)align_up((size_t)workspace, 256);
    SURS_REQUIRE(need - 256 + (size_t)(base - (char *)workspace) <= workspace_bytes, "convolution weight gradient: workspace too small: %zu bytes needed", need);
    const int parts = ceil_div((long long)ho * wo, SG_PART), kk = ksize * ksize, N = kk * cin + 1;
    WArgs a{g, y, x, ho, wo, cout, g_ld, y_ld, h, w, cin, x_ld, ksize, stride, ksize / 2, slope, (float *)base, N};
    SURS_REQUIRE(parts <= 65535 && ceil_div(cout, GT_TILE) <= 65535, "convolution weight gradient: shape too large");
    hipLaunchKernelGGL(wgrad_kernel, dim3(ceil_div(N, GT_TILE), ceil_div(cout, GT_TILE), parts), dim3(256), 0, as_stream(stream), a);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(ceil_div((long long)cout * N, 256)), dim3(256), 0, as_stream(stream), (const float *)base,
                       parts, cout, cin, kk, N, dw, db, accumulate ? 1 : 0);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_conv_grad_input(const float *g, int ho, int wo, int cout, int g_ld, const float *y, int y_ld, float slope,
                                    const float *weight, int cin, int ksize, int stride, float *dx, int h, int w, int dx_ld, int add,
                                    void *stream) {
    SURS_REQUIRE(g && weight && dx, "convolution input gradient: null argument");
    if (int rc = check_conv(ho, wo, h, w, cin, cout, ksize, stride)) return rc;
    SURS_REQUIRE(g_ld >= cout && dx_ld >= cin && (!y || y_ld >= cout), "convolution input gradient: a pitch below the channel count");
    DArgs a{g, y, weight, ho, wo, cout, g_ld, y_ld, h, w, cin, ksize, stride, ksize / 2, slope, dx, dx_ld, add ? 1 : 0};
    SURS_REQUIRE(ceil_div(cin, GT_TILE) <= 65535, "convolution input gradient: shape too large");
    hipLaunchKernelGGL(dgrad_kernel, dim3(ceil_div((long long)h * w, GT_TILE), ceil_div(cin, GT_TILE)), dim3(256), 0, as_stream(stream), a);
    SURS_LAUNCH_CHECK();
    return 0;
}

extern "C" int surs_pixel_unshuffle2_grad(const float *g, int h, int w, int c, int g_ld, const float *y, int y_ld, float slope, float *dz,
                                          int dz_ld, void *stream) {
    SURS_REQUIRE(g && y && dz && h >= 1 && w >= 1 && c >= 1, "pixel-unshuffle gradient: bad argument");
    SURS_REQUIRE(g_ld >= c && y_ld >= c && dz_ld >= 4 * c, "pixel-unshuffle gradient: a pitch below the channel count");
    const long long count = (long long)h * w * 4 * c;
    SURS_REQUIRE(count < (1ll << 31) * 256, "pixel-unshuffle gradient: shape too large");
    hipLaunchKernelGGL(unshuffle2_grad_kernel, dim3(ceil_div(count, 256)), dim3(256), 0, as_stream(stream), g, h, w, c, g_ld, y, y_ld, slope,
                       dz, dz_ld);
    SURS_LAUNCH_CHECK();
    return 0;
}
