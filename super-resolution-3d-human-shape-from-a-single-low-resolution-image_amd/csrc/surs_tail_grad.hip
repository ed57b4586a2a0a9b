// The data gradient of a stack tail's joint for gfx950 (MI355X): include/surs.h, "stack-tail gradients".
//   out = l(a),  next = previous + bl(a) + al(out)      (a = relu(bn_end(conv_last(ll))), [p][256]; out [p][D])
//   surs_tail_joint_grad:   dOut = G_out + G_next W_al                 [p][D]
//                           dA   = dOut W_l + G_next W_bl              [p][256]
// in ONE launch per tile of pixels, where the chain of three surs_conv_grad_input calls (k = 1; the second and third adding into
// their target) reads G_next twice and reads and rewrites dA once more.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 on fp32 operands with fp32 accumulation, as every gradient of this library.  A workgroup of eight
// waves owns a tile of TJ_ROWS pixels: 64 for D <= 256, 32 above (the two resident operands - the tile of G_next, 256 columns, and the
// tile of dOut, D columns rounded up to 16 - are 64 x (257 + 257) words = 128.5 KiB of the 160 KiB at D = 256 and would be 192.5 KiB at
// D = 512; 32 x (257 + 513) words = 96.3 KiB).  Both live in LDS pixel-major with an ODD pitch, so a half-wave's fragment read (32
// pixels, one k) lands on 32 different banks.  The weights are read in place from the plain layout, [k][n] with n contiguous for all
// three products (W_al [256][D], W_l [D][256], W_bl [256][256]): a wave owns 32 output columns that no other wave of the workgroup
// reads, so they go from L2 to registers (a half-wave reads 128 consecutive bytes), sixteen k ahead of the matrix pipe, and with 64
// rows feed two accumulators each.
//   1. the tile of G_next is staged once (16-byte loads; a row past p repeats the last row inside and is never stored); it feeds both
//      products.  The tile of G_out goes where dOut will live.
//   2. dOut: wave v takes the column blocks v, v + 8, ... of ceil(D / 32); per element the accumulator starts at 0, adds
//      G_next[p][c] W_al[c][d] for c = 0 .. 255 in this order (one rounding per product and sum: a k-ordered fmaf chain), and G_out[p][d]
//      is added LAST: dOut = G_out + acc.  It is stored once to memory and kept in LDS (columns D .. up to the next multiple of 16
//      zero).  Without G_next: dOut = G_out, a copy; without G_out: dOut = acc.
//   3. dA: wave v takes the column block v of 8; ONE accumulator, starting at 0: dOut[p][d] W_l[d][j] for d = 0 .. D - 1 in this order,
//      then G_next[p][c] W_bl[c][j] for c = 0 .. 255 (nothing more without G_next).
// No atomics; the order above depends on D alone: two calls give the same bits wherever the buffers lie.
#include <hip/hip_runtime.h>

#include "surs_common.h"
#include "surs_grad_tile.h"   // f32x16, zero16, the accumulator layout (for_each_acc)

namespace surs {
namespace tailgrad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TJ_C = 256;            // channels of a, next, previous
constexpr int TJ_LDG = TJ_C + 1;     // LDS pitch of the G_next tile (odd)
constexpr int TJ_THREADS = 512;

struct JArgs {
    const float *g_out, *g_next;     // [p][D] / [p][256], nullable
    const float *w_al, *w_l, *w_bl;  // [256][D], [D][256], [256][256]
    int p, D, go_ld, gn_ld;
    float *d_out, *d_a;
    int do_ld, da_ld;
};

// acc[b] += A[32 b + row][0 .. K) W[0 .. K)[n0 + column], k ascending.  A: LDS, pitch lda, columns up to the next multiple of 16 of K
// readable, and finite in the rows that count; W: [K][N] in memory, pitch ldw; rows k >= K and columns >= N count as zero.  The loads
// are UNCONDITIONAL (index clamped into the matrix) and the zeros are put in when a step's values become the current ones: a load
// under a lane-dependent condition becomes a branch with a wait behind it, four round trips to L2 per step in front of the matrix
// pipe instead of eight loads in flight beside it.
template <int RB>
__device__ __forceinline__ void product(f32x16 (&acc)[RB], const float *A, int lda, const float *__restrict__ W, int ldw, int K, int N, int n0,
                                        int kh, int li) {
    const int col = n0 + li;
    const bool col_ok = col < N;
    const float *Wc = W + (col_ok ? col : N - 1);
    float rb[8], rn[8];
    auto fetch = [&](int k0, float (&r)[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = Wc[(long long)min(k0 + 2 * u + kh, K - 1) * ldw];
    };
    auto mask = [&](int k0, float (&r)[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = (col_ok && k0 + 2 * u + kh < K) ? r[u] : 0.0f;
    };
    fetch(0, rb);
    mask(0, rb);
    for (int k0 = 0; k0 < K; k0 += 16) {
        const bool more = k0 + 16 < K;
        if (more) fetch(k0 + 16, rn);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int b = 0; b < RB; ++b)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(32 * b + li) * lda + k0 + 2 * u + kh], rb[u], acc[b], 0, 0, 0);
        if (more) {
#pragma unroll
            for (int u = 0; u < 8; ++u) rb[u] = rn[u];
            mask(k0 + 16, rb);
        }
    }
}

// grid: tiles of 32 RB pixels; 512 threads; dynamic LDS: 32 RB (TJ_LDG + ldo) floats, ldo = round_up(D, 16) + 1
template <int RB>
__global__ __launch_bounds__(TJ_THREADS) void tail_joint_kernel(JArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tj_smem[];
    constexpr int ROWS = 32 * RB;
    const TileLanes t = tile_lanes();
    const int tid = t.tid, wave = tid >> 6, kh = t.kh, li = t.li;
    const int D = a.D, D16 = (D + 15) / 16 * 16, ldo = D16 + 1;
    float *Gs = tj_smem, *Os = tj_smem + ROWS * TJ_LDG;
    const long long m0 = (long long)blockIdx.x * ROWS;
    const int valid = (int)min((long long)ROWS, a.p - m0);   // rows of the tile inside the map (>= 1)
    const bool has_next = a.g_next != nullptr, has_out = a.g_out != nullptr;

    // 1. the tiles of G_next and of G_out (into dOut's place), and the zero columns behind dOut's D.  A row past p repeats the last
    //    row inside (unconditional loads): a row of the tile reaches its own row of the results only, and those rows are never stored.
    if (has_next) {
        const float *gn = a.g_next + m0 * a.gn_ld;
#pragma unroll 8
        for (int i = tid; i < ROWS * (TJ_C / 4); i += TJ_THREADS) {
            const int r = i / (TJ_C / 4), q = i - r * (TJ_C / 4);
            const f32x4 v = *reinterpret_cast<const f32x4 *>(gn + (long long)min(r, valid - 1) * a.gn_ld + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) Gs[r * TJ_LDG + 4 * q + k] = v[k];
        }
    }
    if (has_out) {
        const float *go = a.g_out + m0 * a.go_ld;
#pragma unroll 8
        for (int i = tid; i < ROWS * D; i += TJ_THREADS) {
            const int r = i / D, c = i - r * D;
            Os[r * ldo + c] = go[(long long)min(r, valid - 1) * a.go_ld + c];
        }
    }
    for (int i = tid; i < ROWS * (D16 - D); i += TJ_THREADS) {
        const int r = i / (D16 - D), c = D + (i - r * (D16 - D));
        Os[r * ldo + c] = 0.0f;
    }
    __syncthreads();

    // 2. dOut = G_out + G_next W_al: to memory once, and to LDS (each element read and rewritten by the lane that owns it)
    for (int nb = wave; nb * 32 < D; nb += TJ_THREADS / 64) {
        f32x16 acc[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) acc[b] = zero16();
        if (has_next) product<RB>(acc, Gs, TJ_LDG, a.w_al, D, TJ_C, D, nb * 32, kh, li);
        const int col = nb * 32 + li;
        if (col < D) {
            float *dout = a.d_out + m0 * a.do_ld;   // (tile-local 32-bit offsets from a uniform base)
#pragma unroll
            for (int b = 0; b < RB; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 32 * b + 8 * q + 4 * kh + r;   // for_each_acc written out: as a lambda, 159 VGPRs at RB = 2, not 141
                        float v = acc[b][4 * q + r];
                        if (has_out) {
                            const float g = Os[row * ldo + col];
                            v = has_next ? g + v : g;
                        }
                        Os[row * ldo + col] = v;
                        if (row < valid) dout[row * a.do_ld + col] = v;
                    }
        }
    }
    __syncthreads();

    // 3. dA = dOut W_l + G_next W_bl in one accumulator
    {
        f32x16 acc[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b) acc[b] = zero16();
        product<RB>(acc, Os, ldo, a.w_l, TJ_C, D, TJ_C, wave * 32, kh, li);
        if (has_next) product<RB>(acc, Gs, TJ_LDG, a.w_bl, TJ_C, TJ_C, TJ_C, wave * 32, kh, li);
        const int col = wave * 32 + li;
        float *da = a.d_a + m0 * a.da_ld;
#pragma unroll
        for (int b = 0; b < RB; ++b)
            for_each_acc(acc[b], t, 32 * b, [&](int row, float v) {
                if (row < valid) da[row * a.da_ld + col] = v;
            });
    }
}

template <int RB>
int launch(const JArgs &a, hipStream_t st) {
    const int rows = 32 * RB, ldo = (a.D + 15) / 16 * 16 + 1;
    const size_t lds = sizeof(float) * rows * (TJ_LDG + ldo);
    static DeviceOnce once;
    if (once.first())
        SURS_HIP_CHECK(hipFuncSetAttribute((const void *)tail_joint_kernel<RB>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(tail_joint_kernel<RB>, dim3(ceil_div(a.p, rows)), dim3(TJ_THREADS), lds, st, a);
    SURS_LAUNCH_CHECK();
    return 0;
}

}  // namespace tailgrad
}  // namespace surs

using namespace surs;
using namespace surs::tailgrad;

extern "C" int surs_tail_joint_grad(const float *g_out, int g_out_ld, const float *g_next, int g_next_ld, const float *w_al, const float *w_l,
                                    const float *w_bl, int p, int d, float *d_out, int d_out_ld, float *d_a, int d_a_ld, void *stream) {
    SURS_REQUIRE(g_out || g_next, "tail_joint_grad: both gradients are missing");
    SURS_REQUIRE(w_l && d_out && d_a && (!g_next || (w_al && w_bl)), "tail_joint_grad: null argument");
    SURS_REQUIRE(p >= 1 && p < (1 << 24) && d >= 1 && d <= 512, "tail_joint_grad: %d pixels, D = %d (D: 1 .. 512)", p, d);
    SURS_REQUIRE((!g_out || g_out_ld >= d) && d_out_ld >= d && d_a_ld >= TJ_C, "tail_joint_grad: a pitch below the channel count");
    SURS_REQUIRE(!g_next || (g_next_ld >= TJ_C && g_next_ld % 4 == 0 && (reinterpret_cast<size_t>(g_next) & 15) == 0),
                 "tail_joint_grad: g_next: 256 channels, a pitch that is a multiple of 4, 16-byte aligned pixels");
    const JArgs a{g_out, g_next, w_al, w_l, w_bl, p, d, g_out_ld, g_next_ld, d_out, d_a, d_out_ld, d_a_ld};
    return d <= 256 ? launch<2>(a, as_stream(stream)) : launch<1>(a, as_stream(stream));
}
