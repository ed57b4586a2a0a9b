// Device repack (include/surs.h, "device repack"): the packed images of the forward rebuilt on the device from the plain fp32
// parameters, byte for byte what the host packers of surs_pack.cpp give.
//   surs_conv_repack         surs_conv_pack_weights / _x2 / _x3 of a whole table of convolutions, one launch
//   surs_conv1x1_merge       the stack joint's W_bl + W_al W_l in double (EncoderWeights' next{s})
//   surs_mlp_repack          every section of the surs_mlp_pack blob
//   surs_mlp_repack_generic  the images of surs_mlp_pack_generic
// Built with the library's -ffp-contract=off: the split remainders (w - hi, and b1frag's after a multiplication) must not become an fma.
#include "surs_common.h"
#include "surs_repack_gather.h"

namespace surs {

// ------------------------------------------------------------------ convolutions
// Source [cout][cin][taps] has taps fastest; `packed` [tap][cin_pad][cout_pad] has cout fastest, x2 / x3 [part][tap][cin_pad / 16]
// [cout_pad][16] the 16-channel chunk.  A tile is 64 output channels x RP_CH(k) chunks of 16 input channels x all taps: 144 (3x3) or
// 64 (1x1) consecutive floats of 64 source rows, through LDS (rows padded by one float: the transposed reads of 64 rows at one column
// fall on 64 different banks).  Loads: runs of 576 / 256 B; stores: 256 B per (tap, cin) of `packed`, 2 KiB per (part, tap, chunk) of
// x2 / x3 in 16-byte pieces.  Resources (hipcc -Rpass-analysis=kernel-resource-usage): 37 120 B of LDS, 256 threads.
// The grid is fixed (RP_GRID workgroups striding over the tiles): the table and its tile total are on the device and the entry takes
// (items, n, stream) only, so a table of a few tiles launches workgroups that read the total and leave - microseconds, accepted.
constexpr int RP_TILE_CO = 64, RP_THREADS = 256, RP_ROW_MAX = 144, RP_GRID = 2048;
__host__ __device__ inline int rp_chunks(int ksize) { return ksize == 3 ? 1 : 4; }   // 16-channel chunks per tile

__host__ __device__ inline int rp_conv_tiles(int cout, int cin, int ksize) {
    if (cout < 1 || cin < 1 || (ksize != 1 && ksize != 3)) return 0;
    const int nch = (cin + 15) / 16, CH = rp_chunks(ksize);
    return ((cout + 63) / 64) * ((nch + CH - 1) / CH);
}

__device__ inline void rp_store_split(const float (&v)[8], uint16_t *x2, uint16_t *x3, size_t per_part, size_t idx) {
    if (x2) {
        alignas(16) uint16_t hi[8], lo[8];
        for (int i = 0; i < 8; ++i) rp_split2(v[i], hi[i], lo[i]);
        *(uint4 *)(x2 + idx) = *(const uint4 *)hi;
        *(uint4 *)(x2 + per_part + idx) = *(const uint4 *)lo;
    }
    if (x3) {
        alignas(16) uint16_t p[3][8];
        for (int i = 0; i < 8; ++i) {
            uint16_t u[3];
            rp_split3(v[i], u);
            p[0][i] = u[0], p[1][i] = u[1], p[2][i] = u[2];
        }
        for (int part = 0; part < 3; ++part) *(uint4 *)(x3 + part * per_part + idx) = *(const uint4 *)p[part];
    }
}

__global__ __launch_bounds__(RP_THREADS) void conv_repack_kernel(const SursRepackItem *__restrict__ items, int n) {
    __shared__ float tile[RP_TILE_CO * (RP_ROW_MAX + 1)];
    const int total = items[n - 1].tile_end;
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        // the item of tile t: the first whose tile_end is beyond t (uniform over the workgroup)
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].tile_end > t) hi = mid;
            else lo = mid + 1;
        }
        const SursRepackItem it = items[lo];
        const int taps = it.ksize * it.ksize, CH = rp_chunks(it.ksize), nch = (it.cin + 15) / 16, cin_pad = nch * 16;
        const int cout_pad = (it.cout + 63) / 64 * 64, groups = (nch + CH - 1) / CH;
        const int local = t - (it.tile_end - (cout_pad / 64) * groups);
        const int o0 = (local / groups) * RP_TILE_CO, ch0 = (local % groups) * CH, c0 = ch0 * 16;
        const int width = 16 * CH * taps, rs = width + 1;   // floats of a source row in the tile; LDS row pitch
        const size_t row_len = (size_t)it.cin * taps;

        for (int i = threadIdx.x; i < RP_TILE_CO * width; i += RP_THREADS) {
            const int r = i / width, j = i - r * width;
            const bool in = o0 + r < it.cout && c0 + j / taps < it.cin;
            tile[r * rs + j] = in ? it.w[(size_t)(o0 + r) * row_len + (size_t)c0 * taps + j] : 0.0f;
        }
        __syncthreads();
        if (it.packed) {
            for (int i = threadIdx.x; i < RP_TILE_CO * 16 * CH * taps; i += RP_THREADS) {
                const int r = i & 63, ct = i >> 6, cc = ct % (16 * CH), tap = ct / (16 * CH);
                if (c0 + cc < cin_pad) it.packed[((size_t)tap * cin_pad + c0 + cc) * cout_pad + o0 + r] = tile[r * rs + cc * taps + tap];
            }
        }
        if (it.x2 || it.x3) {
            const size_t per_part = (size_t)taps * nch * cout_pad * 16;
            for (int i = threadIdx.x; i < RP_TILE_CO * 2 * CH * taps; i += RP_THREADS) {
                const int half = i & 1, r = (i >> 1) & 63, ct = i >> 7, chl = ct % CH, tap = ct / CH;
                if (ch0 + chl >= nch) continue;
                float v[8];
                for (int e = 0; e < 8; ++e) v[e] = tile[r * rs + (chl * 16 + half * 8 + e) * taps + tap];
                const size_t idx = (((size_t)tap * nch + ch0 + chl) * cout_pad + o0 + r) * 16 + half * 8;
                rp_store_split(v, (uint16_t *)it.x2, (uint16_t *)it.x3, per_part, idx);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ the stack joint
// One thread per output: row o of W (blocks 0..255) and the bias (block 256).  Products of two floats are exact in double.
__global__ __launch_bounds__(256) void conv1x1_merge_kernel(const float *__restrict__ w_bl, const float *__restrict__ b_bl,
                                                              const float *__restrict__ w_al, const float *__restrict__ b_al,
                                                              const float *__restrict__ w_l, const float *__restrict__ b_l, int d,
                                                              float *__restrict__ w_out, float *__restrict__ b_out) {
    const int i = threadIdx.x;
    if (blockIdx.x < 256) {
        const int o = blockIdx.x;
        double s = 0.0;
        for (int k = 0; k < d; ++k) s += (double)w_al[(size_t)o * d + k] * (double)w_l[(size_t)k * 256 + i];
        w_out[o * 256 + i] = (float)((double)w_bl[o * 256 + i] + s);
    } else {
        double s = 0.0;
        for (int k = 0; k < d; ++k) s += (double)w_al[(size_t)i * d + k] * (double)b_l[k];
        b_out[i] = (float)((double)b_bl[i] + s + (double)b_al[i]);
    }
}

// ------------------------------------------------------------------ classifier blobs: one lane per destination element
__global__ __launch_bounds__(256) void mlp_small_kernel(MlpSrc s, MlpBlobHeader h, char *base, int dtype) {
    rp_small_elem(s, h, base, dtype, blockIdx.y, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void mlp_kmajor_kernel(MlpSrc s, MlpBlobHeader h, char *base) {
    rp_kmajor_elem(s, h, base, blockIdx.y, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void mlp_core_kernel(MlpSrc s, MlpBlobHeader h, char *base, int dtype) {
    rp_core_elem(s, h, base, dtype, blockIdx.y, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void mlp_w1t_kernel(MlpSrc s, MlpBlobHeader h, char *base, int dtype) {
    rp_w1t_elem(s, h, base, dtype, blockIdx.x * 256u + threadIdx.x);
}

struct GenTables {
    const float *const *W[2];
    const float *const *B[2];
};
__global__ __launch_bounds__(256) void mlp_generic_kernel(GenLayout lay, GenTables s, int c0_lr, int c0_hr, char *base) {
    const int m = blockIdx.y / GEN_MAX_LAYERS, l = blockIdx.y % GEN_MAX_LAYERS;
    if (l >= lay.n_layers[m]) return;
    rp_generic_elem(lay.layer[m][l], m ? c0_hr : c0_lr, s.W[m][l], s.B[m][l], base, blockIdx.x * 256u + threadIdx.x);
}

}  // namespace surs

using namespace surs;

extern "C" int surs_conv_repack_tiles(int cout, int cin, int ksize) { return rp_conv_tiles(cout, cin, ksize); }

extern "C" int surs_conv_repack(const SursRepackItem *items, int n, void *stream) {
    SURS_REQUIRE(items && n > 0, "surs_conv_repack: an empty table");
    hipLaunchKernelGGL(conv_repack_kernel, dim3(RP_GRID), dim3(RP_THREADS), 0, as_stream(stream), items, n);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_conv1x1_merge(const float *w_bl, const float *b_bl, const float *w_al, const float *b_al, const float *w_l,
                                  const float *b_l, int d, float *w_out, float *b_out, void *stream) {
    SURS_REQUIRE(w_bl && b_bl && w_al && b_al && w_l && b_l && w_out && b_out, "surs_conv1x1_merge: null pointer");
    SURS_REQUIRE(d >= 1, "surs_conv1x1_merge: d = %d", d);
    hipLaunchKernelGGL(conv1x1_merge_kernel, dim3(257), dim3(256), 0, as_stream(stream), w_bl, b_bl, w_al, b_al, w_l, b_l, d, w_out, b_out);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_mlp_repack(int dtype, const float *const *w_lr, const float *const *b_lr, const float *const *w_hr,
                               const float *const *b_hr, void *blob, void *stream) {
    SURS_REQUIRE(dtype == SURS_BF16 || dtype == SURS_F16, "surs_mlp_repack: dtype %d is neither SURS_BF16 nor SURS_F16", dtype);
    SURS_REQUIRE(w_lr && b_lr && w_hr && b_hr && blob, "surs_mlp_repack: null pointer");
    const MlpBlobHeader h = blob_layout((uint32_t)dtype);
    const MlpSrc s = {{w_lr, w_hr}, {b_lr, b_hr}};
    char *base = (char *)blob;
    hipStream_t st = as_stream(stream);
    const unsigned kmajor_max = (unsigned)C_G * CC_PAD;   // the largest of the nine k-major matrices
    hipLaunchKernelGGL(mlp_kmajor_kernel, dim3(ceil_div(kmajor_max, 256), RP_KMAJOR_SECTIONS), dim3(256), 0, st, s, h, base);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mlp_small_kernel, dim3(ceil_div(RP_SMALL_MAX, 256), RP_SMALL_SECTIONS), dim3(256), 0, st, s, h, base, dtype);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mlp_core_kernel, dim3(ceil_div(RP_CORE_HALVES, 256), 2), dim3(256), 0, st, s, h, base, dtype);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mlp_w1t_kernel, dim3(ceil_div(2 * D1 * D2, 256)), dim3(256), 0, st, s, h, base, dtype);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

// The element writers of surs_repack_gather.h run over every index on the HOST (all pointers host pointers): what the kernels above do
// with one lane per element, as plain loops - so that the gather form is held against surs_mlp_pack / surs_mlp_pack_generic without a
// device (tests/test_repack_gather_host.py).
extern "C" int surs_mlp_repack_host(int dtype, const float *const *w_lr, const float *const *b_lr, const float *const *w_hr,
                                    const float *const *b_hr, void *blob) {
    SURS_REQUIRE(dtype == SURS_BF16 || dtype == SURS_F16, "surs_mlp_repack_host: dtype %d is neither SURS_BF16 nor SURS_F16", dtype);
    SURS_REQUIRE(w_lr && b_lr && w_hr && b_hr && blob, "surs_mlp_repack_host: null pointer");
    const MlpBlobHeader h = blob_layout((uint32_t)dtype);
    const MlpSrc s = {{w_lr, w_hr}, {b_lr, b_hr}};
    char *base = (char *)blob;
    for (int y = 0; y < RP_KMAJOR_SECTIONS; ++y)
        for (uint32_t i = 0; rp_kmajor_elem(s, h, base, y, i); ++i) {}
    for (int y = 0; y < RP_SMALL_SECTIONS; ++y)
        for (uint32_t i = 0; rp_small_elem(s, h, base, dtype, y, i); ++i) {}
    for (int m = 0; m < 2; ++m)
        for (uint32_t i = 0; rp_core_elem(s, h, base, dtype, m, i); ++i) {}
    for (uint32_t i = 0; rp_w1t_elem(s, h, base, dtype, i); ++i) {}
    return SURS_OK;
}

extern "C" int surs_mlp_repack_generic_host(const SursMlpShape *lr, const float *const *w_lr, const float *const *b_lr,
                                            const SursMlpShape *hr, const float *const *w_hr, const float *const *b_hr, void *blob) {
    SURS_REQUIRE(lr && hr && w_lr && b_lr && w_hr && b_hr && blob, "surs_mlp_repack_generic_host: null pointer");
    GenLayout lay;
    SURS_REQUIRE(gen_layout(*lr, *hr, lay) == 0, "surs_mlp_repack_generic_host: unsupported SurfaceClassifier shape");
    const float *const *W[2] = {w_lr, w_hr}, *const *B[2] = {b_lr, b_hr};
    for (int m = 0; m < 2; ++m)
        for (int l = 0; l < lay.n_layers[m]; ++l)
            for (uint32_t i = 0; rp_generic_elem(lay.layer[m][l], (m ? hr : lr)->dims[0], W[m][l], B[m][l], (char *)blob, i); ++i) {}
    return SURS_OK;
}

extern "C" int surs_mlp_repack_generic(const SursMlpShape *lr, const float *const *w_lr, const float *const *b_lr, const SursMlpShape *hr,
                                       const float *const *w_hr, const float *const *b_hr, void *blob, void *stream) {
    SURS_REQUIRE(lr && hr, "surs_mlp_repack_generic: null shape");
    SURS_REQUIRE(w_lr && b_lr && w_hr && b_hr && blob, "surs_mlp_repack_generic: null pointer");
    GenLayout lay;
    const int rc = gen_layout(*lr, *hr, lay);
    if (rc) {
        char buf[160];
        return fail(SURS_E_INVALID, "unsupported SurfaceClassifier shape: %s", gen_shape_error(rc, *lr, buf));
    }
    size_t most = 0;
    for (int m = 0; m < 2; ++m)
        for (int l = 0; l < lay.n_layers[m]; ++l) {
            const GenLayer &g = lay.layer[m][l];
            const size_t per_part = (size_t)(g.k1pad + g.k2pad) * g.mpad;
            if (per_part > most) most = per_part;
        }
    const GenTables s = {{w_lr, w_hr}, {b_lr, b_hr}};
    hipLaunchKernelGGL(mlp_generic_kernel, dim3(ceil_div((long long)most, 256), 2 * GEN_MAX_LAYERS), dim3(256), 0, as_stream(stream), lay,
                       s, lr->dims[0], hr->dims[0], (char *)blob);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}
