// Classifier gradients for gfx950 (MI355X): d error / d (every mlp_lr.* and mlp_hr.* parameter) of SuRSNet.forward's loss, the
// encoder frozen (lib/model/SuRSNet.py:131-187, 196-266, lib/model/SurfaceClassifier.py:45-81; single view, orthogonal projection).
//
// Per image, stack s and chunk of GR_CHUNK points (the same index range of both point sets, because q_s enters mlp_hr index by index):
//   gather        X0 [points][c0] fp32 rows [D lr | 64 hr | z (| q)] of both classifiers, the in-image masks
//   training fwd  H_l = LeakyReLU(H_{l-1} W_l^T (+ X0 W_l,skip^T) + b_l), every H_l kept fp32 in the workspace; mlp_lr first (its
//                 masked sigmoid q is the last input channel of mlp_hr), then mlp_hr
//   output stage  d logit of both classifiers from predictions, labels, masks and the loss weights
//   per layer, in reverse, mlp_hr first (its d q is the third source of mlp_lr's gradient):
//                 db += sum_points dZ;  dW += dZ^T In (reduction over the points, split into fixed parts);
//                 dZ_prev = (dZ W[:, :k1]) * LeakyReLU'(H_prev);  the skip part is needed for the q column only (d q)
//
// Arithmetic: ONE GEMM kernel on the fp32-MFMA tile of surs_grad_tile.h (its arithmetic, LDS layout, pipeline and edge rule are
// described there) - fp32-grade whatever --precision says; fp32 inputs keep fp32's exponent range and all 24 bits.  Operands are
// addressed by two strides each so that X W^T, dZ W and dZ^T In are the same code.
// Determinism: no float atomics.  The reduction over the points of a chunk is split into parts of GR_CHUNK / splits points (splits
// depends on the layer's shape only), every part's product goes to its own slab of the workspace, and a second kernel adds the slabs
// in order to the output; chunks, stacks and (accumulate = 1) images follow each other on the stream in a fixed order.
// Workspace: a function of the two shapes alone (surs_mlp_grad_workspace_bytes), whatever n.
//
// Feature-map gradients (surs_mlp_grad_features; nothing below runs when the maps are not asked for):
//   dX0 [points][D + 64] = d error / d (the sampled part of the classifier's input row): dZ_0 W_0[:, :D + 64] plus dZ_l W_l[:, k1 : k1 +
//                 D + 64] of every skip layer, each product added when backward() visits its layer (EPI_ACC; the first visit overwrites).
//                 The z and q columns go to no map and are not formed; d q keeps coming from dq_kernel, so that the parameter
//                 gradients have the bits of the call without maps.
//   scatter       the transpose of sample(), per chunk and classifier, for the lr map of the stack and the hr map:
//                 taps_sort_kernel  one workgroup per map: entry e = 4 point + tap gets key (pixel << 13) | e (all ones: tap outside
//                                   the map) and its weight; bitonic sort of the keys in LDS.  The keys are unique, so the sorted
//                                   order is a function of the points alone.
//                 run_sum_kernel    one wave per run of equal pixel, lanes along the channels: sum_e w_e dX0[point_e] in key order
//                                   (fmaf), then ONE plain read-modify-write of the map row.
//                 A pixel belongs to one run per launch and launches are serial on the stream: no float atomics, a fixed order.
#include <hip/hip_runtime.h>

#include "surs_common.h"
#include "surs_grad_tile.h"
#include "surs_mlp_generic.h"

namespace surs {
namespace grad {

constexpr int GR_CHUNK = 2048;       // points per chunk
constexpr int GR_MAX_SPLITS = 16;    // parts of the point reduction (GR_CHUNK / 16 = 128 points at least)
constexpr int GR_MAX_STACKS = 64;

// ------------------------------------------------------------------------------------------------ gather
// projection, mask, z_feat and grid_sample's bilinear taps (align_corners=True, zeros padding) exactly as the point evaluators of
// surs_query.hip compute them (project_point, in_image, bilinear_taps, tap_sum)
struct GatherArgs {
    const float *pts;     // [3][n]
    long long n, p0;      // points of the image, first point of the chunk
    int nc;               // points of the chunk
    float calib[12];
    float zmul, zdiv;
    const float *feat_lr, *feat_hr;
    int hl, wl, hh, wh, D, c0;
    float *x0;            // [nc][c0]
    float *mask;          // [nc]
};

__device__ __forceinline__ float sample(const float *fm, int H, int W, int C, int ch, float u, float v) {
    const float ix = ((u + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((v + 1.0f) / 2.0f) * (float)(H - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    const float w0 = (vy0 && vx0) ? ((float)x1 - ix) * ((float)y1 - iy) : 0.0f;
    const float w1 = (vy0 && vx1) ? (ix - (float)x0) * ((float)y1 - iy) : 0.0f;
    const float w2 = (vy1 && vx0) ? ((float)x1 - ix) * (iy - (float)y0) : 0.0f;
    const float w3 = (vy1 && vx1) ? (ix - (float)x0) * (iy - (float)y0) : 0.0f;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
    float a = 0.0f;
    a += fm[((long long)cy0 * W + cx0) * C + ch] * w0;
    a += fm[((long long)cy0 * W + cx1) * C + ch] * w1;
    a += fm[((long long)cy1 * W + cx0) * C + ch] * w2;
    a += fm[((long long)cy1 * W + cx1) * C + ch] * w3;
    return a;
}

// one wave per point, lanes along its channels (a tap is one contiguous read)
__global__ __launch_bounds__(256) void gather_kernel(GatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.nc) return;
    const long long t = a.p0 + p;
    const float px = a.pts[t], py = a.pts[a.n + t], pz = a.pts[2 * a.n + t];
    const float *c = a.calib;
    const float X = c[3] + ((c[0] * px + c[1] * py) + c[2] * pz);
    const float Y = c[7] + ((c[4] * px + c[5] * py) + c[6] * pz);
    const float Z = c[11] + ((c[8] * px + c[9] * py) + c[10] * pz);
    const bool in = X >= -1.0f && X <= 1.0f && Y >= -1.0f && Y <= 1.0f;
    float *row = a.x0 + (long long)p * a.c0;
    for (int ch = lane; ch < a.D + GEN_C_HR; ch += 64)
        row[ch] = ch < a.D ? sample(a.feat_lr, a.hl, a.wl, a.D, ch, X, Y) : sample(a.feat_hr, a.hh, a.wh, GEN_C_HR, ch - a.D, X, Y);
    if (lane == 0) {
        row[a.D + GEN_C_HR] = Z * a.zmul / a.zdiv;
        a.mask[p] = in ? 1.0f : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------ the GEMM
// C(m, n) = sum_k A(m, k) B(k, n) over up to two k segments, A(m, k) = A[m a_rs + k a_cs], B(k, n) = B[k b_rs + n b_cs].
enum { EPI_FWD = 0, EPI_DIN = 1, EPI_PART = 2, EPI_ACC = 3 };
struct GemmSeg {
    const float *A, *B;
    long long a_rs, a_cs, b_rs, b_cs;
    int K;
};
struct GemmArgs {
    GemmSeg seg[2];
    int nseg, M, N;
    float *C;             // [M][ldc] (EPI_PART: slab blockIdx.z, c_slab floats apart)
    long long ldc, c_slab;
    int part_len;         // EPI_PART: k range of slab z = [z part_len, min(K, (z + 1) part_len))
    const float *aux;     // EPI_FWD: bias [N];  EPI_DIN: the activations H [M][ld_aux] whose sign selects LeakyReLU's slope
    long long ld_aux;
    int leaky;            // EPI_FWD: LeakyReLU(0.01) on the result (every layer but the last)
    int add;              // EPI_ACC: C += the product (0: C = the product)
};

// AK: A's k index is the contiguous one (else its m index); BK: the same for B (else its n index) - walk_k or walk_rows
template <bool AK, bool BK, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
    __shared__ float As[GT_KT][GT_LDS], Bs[GT_KT][GT_LDS];
    const TileLanes t = tile_lanes();
    const int m0 = blockIdx.y * GT_TILE, n0 = blockIdx.x * GT_TILE;
    constexpr auto walk_a = AK ? walk_k : walk_rows, walk_b = BK ? walk_k : walk_rows;
    f32x16 acc = zero16();
    for (int s = 0; s < g.nseg; ++s) {
        const GemmSeg sg = g.seg[s];
        int kbeg = 0, kend = sg.K;
        if (EPI == EPI_PART) {
            kbeg = (int)blockIdx.z * g.part_len;
            kend = min(sg.K, kbeg + g.part_len);
        }
        float ra[4], rb[4];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const TileCell ca = walk_a(t.tid, j), cb = walk_b(t.tid, j);
                const int m = m0 + ca.row, ka = k0 + ca.k, n = n0 + cb.row, kb = k0 + cb.k;
                ra[j] = (m < g.M && ka < kend) ? sg.A[(long long)m * sg.a_rs + (long long)ka * sg.a_cs] : 0.0f;
                rb[j] = (n < g.N && kb < kend) ? sg.B[(long long)kb * sg.b_rs + (long long)n * sg.b_cs] : 0.0f;
            }
        };
        acc = tile_product<AK, BK>(As, Bs, acc, t, kbeg, kend, ra, rb, fetch);
    }
    float *C = g.C;
    if (EPI == EPI_PART) C += (long long)blockIdx.z * g.c_slab;
    const int col = n0 + t.wn * 32 + t.li;
    if (col >= g.N) return;
    const float bias = EPI == EPI_FWD ? g.aux[col] : 0.0f;
    for_each_acc(acc, t, m0 + t.wm * 32, [&](int row, float v) {
        if (row >= g.M) return;
        if (EPI == EPI_FWD) {
            v += bias;
            if (g.leaky) v = v > 0.0f ? v : 0.01f * v;
        } else if (EPI == EPI_DIN) {
            v = dleaky(v, g.aux[(long long)row * g.ld_aux + col], 0.01f);
        } else if (EPI == EPI_ACC) {
            if (g.add) v += C[(long long)row * g.ldc + col];
        }
        C[(long long)row * g.ldc + col] = v;
    });
}

template <bool AK, bool BK, int EPI>
static int launch_gemm(hipStream_t st, const GemmArgs &g, int slabs) {
    if (g.M <= 0 || g.N <= 0) return 0;
    hipLaunchKernelGGL((gemm_kernel<AK, BK, EPI>), dim3(ceil_div(g.N, GT_TILE), ceil_div(g.M, GT_TILE), slabs), dim3(256), 0, st, g);
    SURS_LAUNCH_CHECK();
    return 0;
}

// second stage of the point reduction: out[i] += slab 0 + slab 1 + ... in this order
__global__ __launch_bounds__(256) void add_slabs_kernel(const float *__restrict__ part, long long slab, int slabs, long long count,
                                                        float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    out[i] += sum_slabs(part, slab, slabs, i);
}

// db[o] += sum over the chunk's points of dZ[p][o]: 64 columns per workgroup, 4 row groups (row = group, group + 4, ...) summed in order
__global__ __launch_bounds__(256) void bias_grad_kernel(const float *__restrict__ dz, int nc, int m, float *__restrict__ gb) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6, o = blockIdx.x * 64 + c;
    float s = 0.0f;
    if (o < m)
        for (int p = rg; p < nc; p += 4) s += dz[(long long)p * m + o];
    part[rg][c] = s;
    __syncthreads();
    if (rg == 0 && o < m) gb[o] += ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// dq[p] += sum_o dZ[p][o] w[o ldw]: the q column of a layer-0 or skip weight; a wave per point, lanes along o, fixed butterfly
__global__ __launch_bounds__(256) void dq_kernel(const float *__restrict__ dz, int nc, int m, const float *__restrict__ w, long long ldw,
                                                 float *__restrict__ dq) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= nc) return;
    float s = 0.0f;
    for (int o = lane; o < m; o += 64) s += dz[(long long)p * m + o] * w[(long long)o * ldw];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) dq[p] += s;
}

// ------------------------------------------------------------------------------------------------ scatter to the feature maps
constexpr int SC_ENTRIES = 4 * GR_CHUNK;            // taps of a chunk
constexpr int SC_SHIFT = 13;                        // key = (pixel << SC_SHIFT) | entry
constexpr unsigned long long SC_NONE = ~0ull;       // a tap outside the map: sorts behind every pixel
static_assert(SC_ENTRIES == 1 << SC_SHIFT, "an entry must fit the key's low bits");

struct ScatterArgs {
    const float *pts;     // [3][n]: the classifier's own point set
    long long n, p0;
    int nc, pow2;         // points of the chunk; the power of two the sort runs on (>= 4 nc)
    float calib[12];
    int H[2], W[2], C[2], col[2];   // map 0: the stack's lr map (columns [0, D) of dX0), map 1: the hr map (columns [D, D + 64))
    float *map[2];        // [H][W][C]
    const float *dx0;     // [nc][ld]
    int ld;
    unsigned long long *keys;   // [2][SC_ENTRIES] sorted
    float *wts;                 // [2][SC_ENTRIES] by entry
};

// NB compare-exchange steps of bitonic stage k on s[0, P), strides j, j / 2, ... j >> (NB - 1) (all >= 1): a thread takes the 2^NB
// keys whose indices differ in exactly those NB bits, so no key is touched by two threads.  The direction bit k lies above them.
template <int NB>
__device__ __forceinline__ void sort_steps(unsigned long long *s, int P, int k, int j) {
    const int jl = j >> (NB - 1), sh = __ffs(jl) - 1;
    for (int g = threadIdx.x; g < (P >> NB); g += 1024) {
        const int base = ((g >> sh) << (sh + NB)) | (g & (jl - 1));
        const bool up = (base & k) == 0;
        unsigned long long v[1 << NB];
#pragma unroll
        for (int t = 0; t < (1 << NB); ++t) v[t] = s[base + t * jl];
#pragma unroll
        for (int b = NB - 1; b >= 0; --b)
#pragma unroll
            for (int t = 0; t < (1 << NB); ++t)
                if (!(t & (1 << b))) {
                    const unsigned long long x = v[t], y = v[t | (1 << b)];
                    const bool sw = (x > y) == up;
                    v[t] = sw ? y : x;
                    v[t | (1 << b)] = sw ? x : y;
                }
#pragma unroll
        for (int t = 0; t < (1 << NB); ++t) s[base + t * jl] = v[t];
    }
}

// Entry e = 4 p + t of map blockIdx.x: tap t of sample() - (x0, y0), (x1, y0), (x0, y1), (x1, y1) - with its weight, validity test
// and arithmetic; then the sort.  A tap whose x or y index falls outside the map gets no key: it is never written.
__global__ __launch_bounds__(1024) void taps_sort_kernel(ScatterArgs a) {
    __shared__ unsigned long long s[SC_ENTRIES];
    const int mp = blockIdx.x, tid = threadIdx.x;
    const int H = a.H[mp], W = a.W[mp], P = a.pow2;
    const float *c = a.calib;
    for (int e = tid; e < P; e += 1024) {
        unsigned long long key = SC_NONE;
        if (e < 4 * a.nc) {
            const long long t = a.p0 + (e >> 2);
            const float px = a.pts[t], py = a.pts[a.n + t], pz = a.pts[2 * a.n + t];
            const float u = c[3] + ((c[0] * px + c[1] * py) + c[2] * pz);
            const float v = c[7] + ((c[4] * px + c[5] * py) + c[6] * pz);
            const float ix = ((u + 1.0f) / 2.0f) * (float)(W - 1);
            const float iy = ((v + 1.0f) / 2.0f) * (float)(H - 1);
            const float fx = floorf(ix), fy = floorf(iy);
            const bool finite = fabsf(fx) < 1.0e9f && fabsf(fy) < 1.0e9f;   // (else the int conversion means nothing: no tap is valid)
            const int x0 = finite ? (int)fx : -2, y0 = finite ? (int)fy : -2, x1 = x0 + 1, y1 = y0 + 1;
            const int xt = (e & 1) ? x1 : x0, yt = (e & 2) ? y1 : y0;
            const float wx = (e & 1) ? ix - (float)x0 : (float)x1 - ix;
            const float wy = (e & 2) ? iy - (float)y0 : (float)y1 - iy;
            if (finite && xt >= 0 && xt < W && yt >= 0 && yt < H) {
                key = ((unsigned long long)((long long)yt * W + xt) << SC_SHIFT) | (unsigned long long)e;
                a.wts[mp * SC_ENTRIES + e] = wx * wy;
            }
        }
        s[e] = key;
    }
    __syncthreads();
    // bitonic sort; the compare-exchange steps of strides j, j / 2, j / 4 of a stage run on 8 keys in registers per pass over LDS:
    // 35 passes over the 64 KiB for 8192 keys instead of 91
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0;) {
            const int nb = j >= 4 ? 3 : (j == 2 ? 2 : 1);
            if (nb == 3) sort_steps<3>(s, P, k, j);
            else if (nb == 2) sort_steps<2>(s, P, k, j);
            else sort_steps<1>(s, P, k, j);
            __syncthreads();
            j >>= nb;
        }
    for (int e = tid; e < 4 * a.nc; e += 1024) a.keys[mp * SC_ENTRIES + e] = s[e];
}

// One wave per sorted position i of map blockIdx.y; the wave at the first position of a pixel's run sums the run and writes the row.
__global__ __launch_bounds__(256) void run_sum_kernel(ScatterArgs a) {
    const int lane = threadIdx.x & 63, mp = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), ne = 4 * a.nc;
    if (i >= ne) return;
    const unsigned long long *keys = a.keys + mp * SC_ENTRIES;
    const unsigned long long k0 = keys[i];
    if (k0 == SC_NONE) return;
    const unsigned long long pix = k0 >> SC_SHIFT;
    if (i > 0 && (keys[i - 1] >> SC_SHIFT) == pix) return;
    const float *wts = a.wts + mp * SC_ENTRIES;
    const int C = a.C[mp];
    float *row = a.map[mp] + (long long)pix * C;
    for (int c0 = 0; c0 < C; c0 += 256) {   // 4 channels per lane and pass: one pass for every D up to 256
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = i; j < ne; ++j) {
            const unsigned long long k = keys[j];
            if ((k >> SC_SHIFT) != pix) break;   // (SC_NONE's pixel is above every map's)
            const int e = (int)(k & (SC_ENTRIES - 1));
            const float w = wts[e];
            const float *src = a.dx0 + (long long)(e >> 2) * a.ld + a.col[mp] + c0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 64 * r + lane;
                if (c0 + ch < C) acc[r] = fmaf(w, src[ch], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = c0 + 64 * r + lane;
            if (ch < C) row[ch] += acc[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------ output stages
struct OutArgs {
    int nc;
    long long p0;                      // first point of the chunk in the image's arrays
    const float *logit_lr, *logit_hr;  // [nc]
    const float *mask_mr, *mask_sr;    // [nc]
    const float *lab_lr, *lab_hr;      // [n] of the image: what q / r are held against
    float c1, c2, cd;                  // 2 mlp1 / (S M), 2 mlp2 / (S M), 2 dispweight / M on the last stack (else 0)
    float *x0_hr;                      // [nc][c0_hr]: q goes into its last column
    int c0_hr;
    float *q, *sig_lr;                 // [nc]
    float *dl_lr, *dl_hr, *dq;         // [nc]
    float *pred_lr, *pred_hr;          // nullable, this stack's row of the image's [S][n]
};

// after mlp_lr's forward: q = mask_mr sigmoid(logit_lr), the last input channel of mlp_hr
__global__ __launch_bounds__(256) void lr_out_kernel(OutArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nc) return;
    const float sg = 1.0f / (1.0f + expf(-a.logit_lr[p]));
    const float q = a.mask_mr[p] * sg;
    a.sig_lr[p] = sg;
    a.q[p] = q;
    a.x0_hr[(long long)p * a.c0_hr + a.c0_hr - 1] = q;
    if (a.pred_lr) a.pred_lr[a.p0 + p] = q;
}

// after mlp_hr's forward: r, d logit_hr, the direct part of d q (mlp_lr's own term and the displacement term); dq starts at zero
__global__ __launch_bounds__(256) void hr_out_kernel(OutArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nc) return;
    const float sg = 1.0f / (1.0f + expf(-a.logit_hr[p]));
    const float m = a.mask_sr[p], r = m * sg, q = a.q[p];
    const float ll = a.lab_lr[a.p0 + p], lh = a.lab_hr[a.p0 + p];
    const float disp = a.cd * ((r - q) - (lh - ll));
    a.dl_hr[p] = m * (sg * (1.0f - sg)) * (a.c2 * (r - lh) + disp);
    a.dl_lr[p] = a.c1 * (q - ll) - disp;
    a.dq[p] = 0.0f;
    if (a.pred_hr) a.pred_hr[a.p0 + p] = r;
}

// after mlp_hr's backward: d logit_lr = mask_mr sigmoid' (direct part + d q through mlp_hr's last input channel)
__global__ __launch_bounds__(256) void lr_dlogit_kernel(OutArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.nc) return;
    const float sg = a.sig_lr[p];
    a.dl_lr[p] = a.mask_mr[p] * (sg * (1.0f - sg)) * (a.dl_lr[p] + a.dq[p]);
}

// ------------------------------------------------------------------------------------------------ host side
struct Net {           // one classifier
    int L, c0, dims[GEN_MAX_LAYERS + 1], in[GEN_MAX_LAYERS], res[GEN_MAX_LAYERS];
};

static void net_of(const SursMlpShape &s, Net &n) {
    n.L = s.n_layers;
    n.c0 = s.dims[0];
    for (int l = 0; l <= n.L; ++l) n.dims[l] = s.dims[l];
    for (int l = 0; l < n.L; ++l) {
        n.res[l] = (s.res_mask >> l) & 1u;
        n.in[l] = n.dims[l] + (n.res[l] ? n.c0 : 0);
    }
}

// parts of the point reduction of a [m][k] weight gradient: enough workgroups to fill the chip, a function of the shape only
static int splits_of(int m, int k) {
    const int tiles = ceil_div(m, GT_TILE) * ceil_div(k, GT_TILE);
    int s = 1;
    while (s < GR_MAX_SPLITS && tiles * s < 768) s *= 2;
    return s;
}

struct Plan {          // workspace offsets in floats
    size_t x0[2], h[2][GEN_MAX_LAYERS], logit[2], dz[2], slabs, vec, total;
    size_t maxw;
    size_t dx0, keys, wts, total_feat;   // surs_mlp_grad_features' own part, behind `total`: the offsets above do not move
};

static void plan_of(const Net (&net)[2], Plan &p) {
    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t at = off;
        off += (floats + 63) / 64 * 64;
        return at;
    };
    size_t maxw = 1, slabs = 0;
    for (int m = 0; m < 2; ++m) {
        p.x0[m] = take((size_t)GR_CHUNK * net[m].c0);
        for (int l = 1; l < net[m].L; ++l) {
            p.h[m][l] = take((size_t)GR_CHUNK * net[m].dims[l]);
            if ((size_t)net[m].dims[l] > maxw) maxw = net[m].dims[l];
        }
        p.logit[m] = take(GR_CHUNK);
        for (int l = 0; l < net[m].L; ++l) {
            const size_t s = (size_t)splits_of(net[m].dims[l + 1], net[m].in[l]) * net[m].dims[l + 1] * net[m].in[l];
            if (s > slabs) slabs = s;
        }
    }
    p.maxw = maxw;
    p.dz[0] = take((size_t)GR_CHUNK * maxw);
    p.dz[1] = take((size_t)GR_CHUNK * maxw);
    p.slabs = take(slabs);
    p.vec = take((size_t)8 * GR_CHUNK);   // mask_mr, mask_sr, q, sig_lr, dl_lr, dl_hr, dq, spare
    p.total = off;
    // dX0 of one classifier at a time (mlp_hr's is scattered before mlp_lr's backward starts); c0 - 1 >= D + 64 of either classifier
    p.dx0 = take((size_t)GR_CHUNK * (net[0].c0 - 1));
    p.keys = take((size_t)2 * SC_ENTRIES * 2);   // 64-bit keys of both maps
    p.wts = take((size_t)2 * SC_ENTRIES);
    p.total_feat = off;
}

static int check_pair(const SursMlpShape *lr, const SursMlpShape *hr) {
    SURS_REQUIRE(lr && hr, "null shape");
    GenLayout lay;
    const int rc = gen_layout(*lr, *hr, lay);
    char why[160];
    SURS_REQUIRE(rc == 0, "unsupported SurfaceClassifier shape: %s", gen_shape_error(rc, *lr, why));
    return 0;
}

// training forward of classifier m on the chunk's nc points
static int forward(hipStream_t st, const Net &n, float *ws, const Plan &p, int m, int nc, const float *const *w, const float *const *b) {
    for (int l = 0; l < n.L; ++l) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        const float *in = l == 0 ? ws + p.x0[m] : ws + p.h[m][l];
        g.seg[0] = GemmSeg{in, w[l], n.dims[l], 1, 1, n.in[l], n.dims[l]};
        g.nseg = 1;
        if (n.res[l]) {
            g.seg[1] = GemmSeg{ws + p.x0[m], w[l] + n.dims[l], n.c0, 1, 1, n.in[l], n.c0};
            g.nseg = 2;
        }
        g.M = nc;
        g.N = n.dims[l + 1];
        const bool last = l == n.L - 1;
        g.C = last ? ws + p.logit[m] : ws + p.h[m][l + 1];
        g.ldc = g.N;
        g.aux = b[l];
        g.leaky = last ? 0 : 1;
        const int rc = launch_gemm<true, true, EPI_FWD>(st, g, 1);
        if (rc) return rc;
    }
    return 0;
}

// dX0 [nc][nf] (+)= dZ [nc][mo] W[:, col : col + nf], W [mo][kin]
static int input_grad(hipStream_t st, const float *dz, int nc, int mo, const float *w, int kin, int col, int nf, float *dx0, bool add) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.seg[0] = GemmSeg{dz, w + col, mo, 1, kin, 1, mo};
    g.nseg = 1;
    g.M = nc;
    g.N = nf;
    g.C = dx0;
    g.ldc = nf;
    g.add = add ? 1 : 0;
    return launch_gemm<true, false, EPI_ACC>(st, g, 1);
}

// backward of classifier m: dl [nc] = d logit; gradients added to gw / gb; dq (hr only): += d error / d (last input channel);
// dx0 (nullable) [nc][nf] = d error / d (the first nf input channels), every layer's part added as the layer is visited
static int backward(hipStream_t st, const Net &n, float *ws, const Plan &p, int m, int nc, const float *const *w, const float *dl,
                    float *const *gw, float *const *gb, float *dq, float *dx0, int nf) {
    const float *dz = dl;
    bool have_dx0 = false;
    for (int l = n.L - 1; l >= 0; --l) {
        const int mo = n.dims[l + 1], k1 = n.dims[l], kin = n.in[l];
        hipLaunchKernelGGL(bias_grad_kernel, dim3(ceil_div(mo, 64)), dim3(256), 0, st, dz, nc, mo, gb[l]);
        SURS_LAUNCH_CHECK();
        // dW += dZ^T [H_l | X0]: slab z = the points [z part_len, (z + 1) part_len) of the chunk
        const int splits = splits_of(mo, kin), part_len = GR_CHUNK / splits;
        const int slabs = min(splits, ceil_div(nc, part_len));
        const long long slab = (long long)mo * kin;
        for (int s = 0; s < (n.res[l] ? 2 : 1); ++s) {
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            const float *in = (s == 1 || l == 0) ? ws + p.x0[m] : ws + p.h[m][l];
            const int kw = s == 1 ? n.c0 : k1;
            g.seg[0] = GemmSeg{dz, in, 1, mo, kw, 1, nc};
            g.nseg = 1;
            g.M = mo;
            g.N = kw;
            g.C = ws + p.slabs + (s == 1 ? k1 : 0);
            g.ldc = kin;
            g.c_slab = slab;
            g.part_len = part_len;
            const int rc = launch_gemm<false, false, EPI_PART>(st, g, slabs);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(add_slabs_kernel, dim3(ceil_div(slab, 256)), dim3(256), 0, st, ws + p.slabs, slab, slabs, slab, gw[l]);
        SURS_LAUNCH_CHECK();
        if (dq) {   // the q column: the last of layer 0's own inputs, the last of a skip segment
            if (l == 0) {
                hipLaunchKernelGGL(dq_kernel, dim3(ceil_div(nc, 4)), dim3(256), 0, st, dz, nc, mo, w[l] + n.c0 - 1, (long long)kin, dq);
                SURS_LAUNCH_CHECK();
            }
            if (n.res[l]) {
                hipLaunchKernelGGL(dq_kernel, dim3(ceil_div(nc, 4)), dim3(256), 0, st, dz, nc, mo, w[l] + k1 + n.c0 - 1, (long long)kin, dq);
                SURS_LAUNCH_CHECK();
            }
        }
        if (dx0) {   // the skip segment, then layer 0's own inputs
            if (n.res[l]) {
                const int rc = input_grad(st, dz, nc, mo, w[l], kin, k1, nf, dx0, have_dx0);
                if (rc) return rc;
                have_dx0 = true;
            }
            if (l == 0) {
                const int rc = input_grad(st, dz, nc, mo, w[l], kin, 0, nf, dx0, have_dx0);
                if (rc) return rc;
            }
        }
        if (l >= 1) {   // dZ of the layer below = (dZ W[:, :k1]) * LeakyReLU'(H_l)
            GemmArgs g;
            memset(&g, 0, sizeof(g));
            float *out = ws + p.dz[l & 1];
            g.seg[0] = GemmSeg{dz, w[l], mo, 1, kin, 1, mo};
            g.nseg = 1;
            g.M = nc;
            g.N = k1;
            g.C = out;
            g.ldc = k1;
            g.aux = ws + p.h[m][l];
            g.ld_aux = k1;
            const int rc = launch_gemm<true, false, EPI_DIN>(st, g, 1);
            if (rc) return rc;
            dz = out;
        }
    }
    return 0;
}

}  // namespace grad
}  // namespace surs

using namespace surs;
using namespace surs::grad;

extern "C" size_t surs_mlp_grad_workspace_bytes(const SursMlpShape *lr, const SursMlpShape *hr) {
    if (check_pair(lr, hr)) return 0;
    Net net[2];
    net_of(*lr, net[0]);
    net_of(*hr, net[1]);
    Plan p;
    plan_of(net, p);
    return p.total * sizeof(float);
}

extern "C" size_t surs_mlp_grad_features_workspace_bytes(const SursMlpShape *lr, const SursMlpShape *hr) {
    if (check_pair(lr, hr)) return 0;
    Net net[2];
    net_of(*lr, net[0]);
    net_of(*hr, net[1]);
    Plan p;
    plan_of(net, p);
    return p.total_feat * sizeof(float);
}

extern "C" int surs_mlp_grad_features(const float *points_mr, const float *points_sr, int n, const float *calib_mr,
                                      const float *calib_sr, float zmul, float zdiv, int num_stacks, const float *const *feat_lr, int hl,
                                      int wl, const float *feat_hr, int hh, int wh, const SursMlpShape *lr, const SursMlpShape *hr,
                                      const float *const *w_lr, const float *const *b_lr, const float *const *w_hr,
                                      const float *const *b_hr, const float *lab_lr, const float *lab_hr, const float *loss_weights,
                                      long long m_total, int accumulate, float *const *gw_lr, float *const *gb_lr, float *const *gw_hr,
                                      float *const *gb_hr, float *pred_lr, float *pred_hr, float *const *gfeat_lr, float *gfeat_hr,
                                      int accumulate_features, void *workspace, size_t workspace_bytes, void *stream) {
    const bool feat = gfeat_lr || gfeat_hr;
    SURS_REQUIRE(!feat || (gfeat_lr && gfeat_hr), "gfeat_lr and gfeat_hr come together");
    SURS_REQUIRE(n >= 0, "negative point count");
    SURS_REQUIRE(num_stacks >= 1 && num_stacks <= GR_MAX_STACKS, "num_stacks must be between 1 and %d", GR_MAX_STACKS);
    SURS_REQUIRE(m_total >= 1 && m_total >= n, "the denominator M must be at least n (and 1)");
    SURS_REQUIRE(calib_mr && calib_sr && feat_lr && feat_hr && loss_weights && w_lr && b_lr && w_hr && b_hr && gw_lr && gb_lr && gw_hr &&
                 gb_hr, "null argument");
    SURS_REQUIRE(hl > 0 && wl > 0 && hh > 0 && wh > 0, "bad sizes");
    int rc = check_pair(lr, hr);
    if (rc) return rc;
    Net net[2];
    net_of(*lr, net[0]);
    net_of(*hr, net[1]);
    Plan p;
    plan_of(net, p);
    const float *const *w[2] = {w_lr, w_hr}, *const *b[2] = {b_lr, b_hr};
    float *const *gw[2] = {gw_lr, gw_hr}, *const *gb[2] = {gb_lr, gb_hr};
    for (int m = 0; m < 2; ++m)
        for (int l = 0; l < net[m].L; ++l) SURS_REQUIRE(w[m][l] && b[m][l] && gw[m][l] && gb[m][l], "null weight or gradient pointer");
    for (int s = 0; s < num_stacks; ++s) SURS_REQUIRE(feat_lr[s], "null feature map");
    for (int s = 0; feat && s < num_stacks; ++s) SURS_REQUIRE(gfeat_lr[s], "null feature-map gradient");
    hipStream_t st = as_stream(stream);
    const int D = gen_hg_dim(*lr), nf = D + GEN_C_HR;
    if (feat && !accumulate_features) {
        for (int s = 0; s < num_stacks; ++s) SURS_HIP_CHECK(hipMemsetAsync(gfeat_lr[s], 0, sizeof(float) * hl * wl * D, st));
        SURS_HIP_CHECK(hipMemsetAsync(gfeat_hr, 0, sizeof(float) * hh * wh * GEN_C_HR, st));
    }
    if (!accumulate)
        for (int m = 0; m < 2; ++m)
            for (int l = 0; l < net[m].L; ++l) {
                SURS_HIP_CHECK(hipMemsetAsync(gw[m][l], 0, sizeof(float) * net[m].dims[l + 1] * net[m].in[l], st));
                SURS_HIP_CHECK(hipMemsetAsync(gb[m][l], 0, sizeof(float) * net[m].dims[l + 1], st));
            }
    if (n == 0) return 0;
    SURS_REQUIRE(points_mr && points_sr && lab_lr && lab_hr, "null argument");
    const size_t need = (feat ? p.total_feat : p.total) * sizeof(float);
    SURS_REQUIRE(workspace && workspace_bytes >= need, "workspace too small: %zu bytes needed", need);
    float *ws = (float *)workspace;
    float *vec = ws + p.vec;
    float *dx0 = feat ? ws + p.dx0 : nullptr;
    // the transpose of the gather of classifier m's rows: both maps, this chunk
    auto scatter = [&](int m, int s, long long p0, int nc) -> int {
        ScatterArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.pts = m ? points_sr : points_mr;
        sa.n = n;
        sa.p0 = p0;
        sa.nc = nc;
        sa.pow2 = 4;
        while (sa.pow2 < 4 * nc) sa.pow2 *= 2;
        for (int i = 0; i < 12; ++i) sa.calib[i] = (m ? calib_sr : calib_mr)[i];
        sa.H[0] = hl, sa.W[0] = wl, sa.C[0] = D, sa.col[0] = 0, sa.map[0] = gfeat_lr[s];
        sa.H[1] = hh, sa.W[1] = wh, sa.C[1] = GEN_C_HR, sa.col[1] = D, sa.map[1] = gfeat_hr;
        sa.dx0 = dx0;
        sa.ld = nf;
        sa.keys = (unsigned long long *)(ws + p.keys);
        sa.wts = ws + p.wts;
        hipLaunchKernelGGL(taps_sort_kernel, dim3(2), dim3(1024), 0, st, sa);
        SURS_LAUNCH_CHECK();
        hipLaunchKernelGGL(run_sum_kernel, dim3(ceil_div(4 * nc, 4), 2), dim3(256), 0, st, sa);
        SURS_LAUNCH_CHECK();
        return 0;
    };
    const double sm = (double)num_stacks * (double)m_total;
    for (int s = 0; s < num_stacks; ++s)
        for (long long p0 = 0; p0 < n; p0 += GR_CHUNK) {
            const int nc = (int)((n - p0) < GR_CHUNK ? (n - p0) : GR_CHUNK);
            for (int m = 0; m < 2; ++m) {
                GatherArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.pts = m ? points_sr : points_mr;
                ga.n = n;
                ga.p0 = p0;
                ga.nc = nc;
                for (int i = 0; i < 12; ++i) ga.calib[i] = (m ? calib_sr : calib_mr)[i];
                ga.zmul = zmul;
                ga.zdiv = zdiv;
                ga.feat_lr = feat_lr[s];
                ga.feat_hr = feat_hr;
                ga.hl = hl;
                ga.wl = wl;
                ga.hh = hh;
                ga.wh = wh;
                ga.D = D;
                ga.c0 = net[m].c0;
                ga.x0 = ws + p.x0[m];
                ga.mask = vec + m * GR_CHUNK;
                hipLaunchKernelGGL(gather_kernel, dim3(ceil_div(nc, 4)), dim3(256), 0, st, ga);
                SURS_LAUNCH_CHECK();
            }
            OutArgs oa;
            memset(&oa, 0, sizeof(oa));
            oa.nc = nc;
            oa.p0 = p0;
            oa.logit_lr = ws + p.logit[0];
            oa.logit_hr = ws + p.logit[1];
            oa.mask_mr = vec;
            oa.mask_sr = vec + GR_CHUNK;
            oa.lab_lr = lab_lr;
            oa.lab_hr = lab_hr;
            oa.c1 = (float)(2.0 * (double)loss_weights[0] / sm);
            oa.c2 = (float)(2.0 * (double)loss_weights[1] / sm);
            oa.cd = s == num_stacks - 1 ? (float)(2.0 * (double)loss_weights[2] / (double)m_total) : 0.0f;
            oa.x0_hr = ws + p.x0[1];
            oa.c0_hr = net[1].c0;
            oa.q = vec + 2 * GR_CHUNK;
            oa.sig_lr = vec + 3 * GR_CHUNK;
            oa.dl_lr = vec + 4 * GR_CHUNK;
            oa.dl_hr = vec + 5 * GR_CHUNK;
            oa.dq = vec + 6 * GR_CHUNK;
            oa.pred_lr = pred_lr ? pred_lr + (long long)s * n : nullptr;
            oa.pred_hr = pred_hr ? pred_hr + (long long)s * n : nullptr;
            const dim3 og(ceil_div(nc, 256));
            if ((rc = forward(st, net[0], ws, p, 0, nc, w[0], b[0]))) return rc;
            hipLaunchKernelGGL(lr_out_kernel, og, dim3(256), 0, st, oa);
            SURS_LAUNCH_CHECK();
            if ((rc = forward(st, net[1], ws, p, 1, nc, w[1], b[1]))) return rc;
            hipLaunchKernelGGL(hr_out_kernel, og, dim3(256), 0, st, oa);
            SURS_LAUNCH_CHECK();
            if ((rc = backward(st, net[1], ws, p, 1, nc, w[1], oa.dl_hr, gw[1], gb[1], oa.dq, dx0, nf))) return rc;
            if (feat && (rc = scatter(1, s, p0, nc))) return rc;
            hipLaunchKernelGGL(lr_dlogit_kernel, og, dim3(256), 0, st, oa);
            SURS_LAUNCH_CHECK();
            if ((rc = backward(st, net[0], ws, p, 0, nc, w[0], oa.dl_lr, gw[0], gb[0], nullptr, dx0, nf))) return rc;
            if (feat && (rc = scatter(0, s, p0, nc))) return rc;
        }
    return 0;
}

extern "C" int surs_mlp_grad(const float *points_mr, const float *points_sr, int n, const float *calib_mr, const float *calib_sr,
                             float zmul, float zdiv, int num_stacks, const float *const *feat_lr, int hl, int wl, const float *feat_hr,
                             int hh, int wh, const SursMlpShape *lr, const SursMlpShape *hr, const float *const *w_lr,
                             const float *const *b_lr, const float *const *w_hr, const float *const *b_hr, const float *lab_lr,
                             const float *lab_hr, const float *loss_weights, long long m_total, int accumulate, float *const *gw_lr,
                             float *const *gb_lr, float *const *gw_hr, float *const *gb_hr, float *pred_lr, float *pred_hr,
                             void *workspace, size_t workspace_bytes, void *stream) {
    return surs_mlp_grad_features(points_mr, points_sr, n, calib_mr, calib_sr, zmul, zdiv, num_stacks, feat_lr, hl, wl, feat_hr, hh, wh,
                                  lr, hr, w_lr, b_lr, w_hr, b_hr, lab_lr, lab_hr, loss_weights, m_total, accumulate, gw_lr, gb_lr, gw_hr,
                                  gb_hr, pred_lr, pred_hr, nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}
