// The 64 x 64 fp32-MFMA tile of the gradient GEMMs for gfx950 (MI355X), stated once: gemm_kernel (surs_mlp_grad.hip), wgrad_kernel and
// dgrad_kernel (surs_sr_grad.hip) are this tile with their own loaders and epilogues; tail_joint_kernel (surs_tail_grad.hip) shares the
// accumulator layout.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 on fp32 operands with fp32 accumulation - a k-ordered fmaf chain per output element, whatever
// --precision says (gradient operands reach 1e-12 and below, where an f16 operand split flushes them to zero).
// Tile: GT_TILE x GT_TILE outputs per workgroup of four waves (32 x 32 each, wave (wm, wn)), k step GT_KT through two LDS arrays
// [GT_KT][GT_LDS], k-major: A as [k][row], B as [k][column].  The kernel's fetch zero-fills the edges: no size need be a multiple.
// Bank conflicts count per 32-lane half over 64 banks: a half's fragment read is 32 consecutive words of one row; a staging write
// along the row (walk_rows) is 64 consecutive words; the k-contiguous staging write (walk_k: 16 rows x 2 columns per half) lands on
// banks 4 k + column, all different because of the 68-word pitch.
// Pipeline: the next step's operands are in flight in four registers per operand and thread while the matrix pipe works on this step;
// one workgroup walks [kbeg, kend) of an output tile in order, and nothing here depends on where a buffer lies.
#pragma once
#include <hip/hip_runtime.h>

namespace surs {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int GT_TILE = 64, GT_KT = 16, GT_LDS = 68;
__device__ __forceinline__ f32x16 zero16() { return (f32x16)(0.0f); }

// wave (wm, wn) of the 2 x 2 waves of a 256-thread tile; lane = 32 kh + li: k half and row / column of the 32 x 32 x 2 fragment
// (tail_joint_kernel's eight waves use kh and li only)
struct TileLanes { int tid, wm, wn, kh, li; };

__device__ __forceinline__ TileLanes tile_lanes() {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return TileLanes{tid, wave >> 1, wave & 1, lane >> 5, lane & 31};
}

// The two ways 256 threads stage a 64 x 16 operand tile, element e = tid + 256 j (j = 0 .. 3), so that neighbouring threads read
// neighbouring addresses: walk_rows, (row e & 63, k e >> 6), where the operand's row (B: column) index is the contiguous one; walk_k,
// (row e >> 4, k e & 15), where k is.  In (tid, j) form: hipcc does not know tid < 256 and keeps four indices per operand for e's.
struct TileCell { int row, k; };
constexpr TileCell walk_rows(int tid, int j) { return TileCell{tid & 63, (tid >> 6) + 4 * j}; }
constexpr TileCell walk_k(int tid, int j) { return TileCell{(tid >> 4) + 16 * j, tid & 15}; }

constexpr bool walk_covers_tile(TileCell (*walk)(int, int)) {
    bool seen[GT_KT][GT_TILE] = {};
    for (int j = 0; j < 4; ++j)
        for (int tid = 0; tid < 256; ++tid) {
            const TileCell c = walk(tid, j);
            if (c.row < 0 || c.row >= GT_TILE || c.k < 0 || c.k >= GT_KT || seen[c.k][c.row]) return false;
            seen[c.k][c.row] = true;
        }
    return true;
}
static_assert(walk_covers_tile(walk_rows) && walk_covers_tile(walk_k), "a staging walk must touch every cell of the tile exactly once");

// Returns acc + A[:, kbeg .. kend) B[kbeg .. kend), :], k ascending.  fetch(k0): step k0's operands into ra / rb, every load under its own
// test against the edges and kend (zero otherwise), so that the prologue fetch of an empty range reads nothing.  They are staged by
// walk_k (AK / BK) or walk_rows.  The accumulator goes in and out by value: through a reference gemm_kernel takes 12 more registers.
template <bool AK, bool BK, class Fetch>
__device__ __forceinline__ f32x16 tile_product(float (&As)[GT_KT][GT_LDS], float (&Bs)[GT_KT][GT_LDS], f32x16 acc, const TileLanes &t, int kbeg,
                                               int kend, const float (&ra)[4], const float (&rb)[4], const Fetch &fetch) {
    fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += GT_KT) {
        __syncthreads();   // the previous step's fragments have been read
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const TileCell ca = AK ? walk_k(t.tid, j) : walk_rows(t.tid, j), cb = BK ? walk_k(t.tid, j) : walk_rows(t.tid, j);
            As[ca.k][ca.row] = ra[j];
            Bs[cb.k][cb.row] = rb[j];
        }
        __syncthreads();   // this step's operands are in LDS
        if (k0 + GT_KT < kend) fetch(k0 + GT_KT);   // in flight while the matrix pipe works on this step
#pragma unroll
        for (int kk = 0; kk < GT_KT; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + t.kh][t.wm * 32 + t.li], Bs[kk + t.kh][t.wn * 32 + t.li], acc, 0, 0, 0);
    }
    return acc;
}

// acc[4 q + r] = row 8 q + 4 kh + r, column li of a wave's 32 x 32 tile: f(m0 + row, value) for the sixteen elements in q, r order
template <class F>
__device__ __forceinline__ void for_each_acc(f32x16 acc, const TileLanes &t, int m0, const F &f) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) f(m0 + 8 * q + 4 * t.kh + r, acc[4 * q + r]);
}

// v * LeakyReLU'(z) from the stored y = LeakyReLU(z), which has z's sign; at exactly 0 the negative side's slope, as torch.  One product
// with the selected factor (v * 1 is v, bit for bit): selecting between v and slope * v made hipcc wait for v's load before issuing y's
__device__ __forceinline__ float dleaky(float v, float y, float slope) { return v * (y > 0.0f ? 1.0f : slope); }

// slab 0 + slab 1 + ... of element i, in this order; slabs `stride` floats apart
__device__ __forceinline__ float sum_slabs(const float *__restrict__ part, long long stride, int slabs, long long i) {
    float s = part[i];
    for (int z = 1; z < slabs; ++z) s += part[z * stride + i];
    return s;
}

}  // namespace surs
