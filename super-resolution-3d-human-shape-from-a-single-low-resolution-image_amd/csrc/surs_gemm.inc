// The layer GEMM of the point path (included by surs_query.hip inside namespace surs, after split3_bf16 and the vector
// typedefs): gemm_x3g_kernel, one family of 256-point LDS-DMA tiles on split operands (one f16, two f16 or three bf16 parts),
// rvec_small_kernel, the same products for the small batches of the column kernels' affine part, and rvec_fused_kernel, the same
// products for the bf16 sweep's large batches with the operand formed in the kernel.  DESIGN.md section 4.3.
// ------------------------------------------------------------------------------------------------
// Workgroup -> output tile for the layer GEMMs.  The point tile (128 columns of X, up to 1360 x 128 values) is the big
// operand and every row block of the layer re-reads it, so the row blocks of one point tile must run together and on
// ONE XCD (its L2 then serves the re-reads; with the row index slow every layer read its input M/128 times from HBM).
// Workgroup ids go round-robin over the 8 XCDs: XCD x takes the logical range [x*per, (x+1)*per), row block fastest.
// The grid is 8*per workgroups, per = ceil(mblocks*nblocks / 8).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool gemm_block_tile(int mblocks, int nblocks, int &mb, int &nb) {
    const unsigned total = (unsigned)mblocks * (unsigned)nblocks, per = gridDim.x >> 3;
    const unsigned logical = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    mb = (int)(logical % (unsigned)mblocks);
    nb = (int)(logical / (unsigned)mblocks);
    return logical < total;
}

static inline unsigned gemm_grid(int mblocks, long long nblocks) {
    const long long total = (long long)mblocks * nblocks;
    return (unsigned)(((total + 7) / 8) * 8);
}

struct SplitSeg {
    const unsigned short *base;   // [3][ktiles][np][16]
    long long part;               // halfwords between parts
    int ktiles;
};

// ------------------------------------------------------------------------------------------------
// The layer kernel: Ys[m][n] = split(act(sum_k W[k][m] X[k][n] + bias[m])), or an fp32 output (see OUT below); both operands
// arrive as split images (weights from the packer, activations from gather_kernel and this kernel's epilogue).  A 128 x 128
// tile (4 waves, 16-byte loads straight into registers) leaves the matrix pipe idle because the operands cannot be fetched
// fast enough - 36 KB of L2 reads per 96 MFMAs is 48 B/clk/CU at full MFMA rate; the 9 loads of a step took 2000 cycles to
// issue.  Here one workgroup of 8 waves owns a 256 x 256 output tile, both operands go through LDS once per workgroup (48 KB
// per 384 MFMAs = 16 B/clk/CU), and the staging is LDS-DMA (global_load_lds_dwordx4, no staging registers) into a 3-stage
// ring, two stages in flight:
//   stage = [3 parts][8 pieces] weights + [3 parts][8 pieces] points, a piece = 32 rows x 16 k = 1 KB = one wave-wide DMA;
//   the weight image is fragment-ordered (surs_pack.cpp) so a weight piece IS an MFMA A operand in lane order; a point
//   piece is put in the same order by the DMA's per-lane source address (lane (h, r) fetches half h of row r).
//   Wave w issues piece w of every part of both operands: 6 DMAs per stage.
// Waves 2 (rows) x 4 (columns), wave tile 128 x 64 = 4 x 2 MFMA tiles, 128 accumulator registers.
// Synchronisation is by hand (cdna_hip_programming.md, "Pipelining across barriers"): fragment reads are asm ds_read_b128
// with counted lgkmcnt waits, the step barrier is a raw s_barrier behind `s_waitcnt vmcnt(6)` = "my DMAs of this step
// have landed, those of the next may still fly"; the compiler sees no LDS read and therefore adds no vmcnt(0) of its own.
// ------------------------------------------------------------------------------------------------
constexpr int G3_STAGES = 3;
constexpr int g3_stage_bytes(int bm, int np_ = 3) { return np_ * ((bm / 32) + 8) * 1024; }   // weights [parts][bm/32] + points [parts][8] pieces
constexpr int g3_lds_bytes(int bm, int np_ = 3) { return G3_STAGES * g3_stage_bytes(bm, np_); }

// How an fp32 operand is carried through the matrix pipe (both give fp32-grade results, DESIGN.md 4.3):
//   SplitKind<3>  three bf16 parts (24 significant bits, fp32's exponent range), six products per MAC
//   SplitKind<2>  two f16 parts (22 bits; |x| < 65504), three products per MAC: half the MFMA work, two thirds of the bytes
template <int NP> struct SplitKind;
// SplitKind<1>: ONE f16 part - not fp32-grade (11 significant bits): the affine-part GEMM of the reduced-precision column kernels
template <> struct SplitKind<1> {
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ f32x16 mfma(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void split(float x, unsigned short (&p)[1]) { p[0] = __builtin_bit_cast(unsigned short, (_Float16)x); }
};
template <> struct SplitKind<3> {
    typedef bf16x8_t vec8;
    static __device__ __forceinline__ f32x16 mfma(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void split(float x, unsigned short (&p)[3]) { split3_bf16(x, p[0], p[1], p[2]); }
};
template <> struct SplitKind<2> {
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ f32x16 mfma(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void split(float x, unsigned short (&p)[2]) {
        asm volatile("" : "+v"(x));   // (one value feeds the conversion and the remainder: see split2_f16 in surs_grid_v5.inc)
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)__builtin_fmaf((float)hi, -1.0f, x);   // x - hi exactly (v_fma_mix_f32), then rounded
        p[0] = __builtin_bit_cast(unsigned short, hi);
        p[1] = __builtin_bit_cast(unsigned short, lo);
    }
};

// NW = 8 waves (2 x 4); BM = 256 or 128 rows per workgroup (128: the last hidden layer, M = 128, and the column constants of
// the sweep, M = 2944); OUT: G3_SPLIT = bias, LeakyReLU, split image for the next layer; G3_F32 = bias, LeakyReLU, fp32
// [m][n] (in front of mlp_last_kernel / the view mean); G3_F32_T = bias only, fp32 transposed [n][ldy] (the column constants,
// the affine part's R).  The tile is always 256 points wide.  NP = parts per operand.
enum { G3_SPLIT = 0, G3_F32 = 1, G3_F32_T = 2 };
template <int NW, int BM, int OUT, int NP = 3>
__global__ __launch_bounds__(NW * 64) void gemm_x3g_kernel(const unsigned short *__restrict__ W3, int M, int Ktot, SplitSeg s1,
                                                           SplitSeg s2, long long np, const float *__restrict__ bias,
                                                           float *__restrict__ Y, long long ldy,
                                                           unsigned short *__restrict__ Ys, long long ys_part, int nblocks) {
    typedef SplitKind<NP> SK;
    typedef typename SK::vec8 vec8;
    constexpr int AP = BM / 32;              // weight pieces per part and stage
    constexpr int TI = AP / 2;               // MFMA row tiles per wave
    constexpr int ASZ = NP * AP * 1024;      // bytes of weights per stage; the points follow
    constexpr int G3_STAGE = g3_stage_bytes(BM, NP);
    static_assert(NW == 8, "eight waves, 2 x 4");
    static_assert(TI == 4 || TI == 2, "wave tile is 128 or 64 rows");
    static_assert(NP >= 1 && NP <= 3, "one f16 part (not fp32-grade), two f16 parts or three bf16 parts");
    extern __shared__ __attribute__((aligned(16))) unsigned char g3_smem[];
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    typedef const __attribute__((address_space(1))) void gptr_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int kh = lane >> 5, li = lane & 31;
    int mb, nb;
    {   // same XCD-aware order as gemm_block_tile
        const unsigned mblocks = (unsigned)M / (unsigned)BM, total = mblocks * (unsigned)nblocks, per = gridDim.x >> 3;
        const unsigned logical = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
        if (logical >= total) return;
        mb = (int)(logical % mblocks);
        nb = (int)(logical / mblocks);
    }
    const long long n0 = (long long)nb * 256;
    const int m0 = mb * BM;
    const int ktiles = s1.ktiles + s2.ktiles;
    const size_t per_part = (size_t)Ktot * M;
    lds_u8 *smem = (lds_u8 *)g3_smem;
    const unsigned lds0 = (unsigned)(size_t)smem;

    f32x16 acc[TI][2];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // DMA d of this wave and step kt, nd per wave and stage (a multiple of NP: one NP-th goes out behind each product of phase 1):
    //   BM 256: piece `wave` of part d>>1 of the weights (d even) / points (d odd), nd = 2 NP;
    //   BM 128: the same for waves 0-3; waves 4-7 piece `wave` of part d of the points only, nd = NP.
    // A points piece is fetched with lane (h, r) on half h of row r, so it lands in LDS in fragment order like the weights.
    const int piece = wave & 7;
    const bool both = BM == 256 || wave < 4;
    const int nd = both ? 2 * NP : NP;
    const unsigned short *wsrc = W3 + ((size_t)(m0 + 32 * piece)) * 16 + lane * 8;
    auto issue1 = [&](int kt, int d) {
        const int p = both ? d >> 1 : d;
        // (the else arm is always true, waves 4-7 of BM 128 fetch points only; simpler spellings of it compile to other code)
        const bool points = both ? (d & 1) : (NW == 8 || wave >= 8);
        lds_u8 *stage = smem + (kt % G3_STAGES) * G3_STAGE + piece * 1024;
        if (!points) {
            const unsigned short *wk = wsrc + (size_t)kt * M * 16 + p * per_part;
            __builtin_amdgcn_global_load_lds((gptr_t *)wk, (__attribute__((address_space(3))) void *)(stage + p * (AP * 1024)), 16, 0, 0);
        } else {
            const bool first = kt < s1.ktiles;
            const unsigned short *xb = first ? s1.base : s2.base;
            const long long xpart = first ? s1.part : s2.part;
            const int k = first ? kt : kt - s1.ktiles;
            const unsigned short *xsrc = xb + ((long long)k * np + n0 + 32 * piece) * 16 + (li * 16 + kh * 8) + p * xpart;
            __builtin_amdgcn_global_load_lds((gptr_t *)xsrc, (__attribute__((address_space(3))) void *)(stage + ASZ + p * 8192), 16, 0, 0);
        }
    };
    auto issue = [&](int kt) {
        for (int d = 0; d < nd; ++d) issue1(kt, d);
    };

    issue(0);
    if (ktiles > 1) issue(1);
    // fragment addresses inside a stage: weights piece TI wm + i, points piece 2 wn + j, both at lane * 16
    const unsigned a_off = lds0 + (unsigned)(wm * TI * 1024 + lane * 16);
    const unsigned b_off = lds0 + (unsigned)ASZ + (unsigned)(wn * 2048 + lane * 16);
    vec8 a[TI][NP], b[2][NP];
    auto mm = [&](int pa, int pb) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // G3_F32_T: the operands swapped - the same dot products, the result tile transposed (register 4g + r = point
                // 8g + 4kh + r, the lane's column = weight row li), so that the epilogue's stores run along the output rows
                if constexpr (OUT == G3_F32_T) acc[i][j] = SK::mfma(b[j][pb], a[i][pa], acc[i][j]);
                else acc[i][j] = SK::mfma(a[i][pa], b[j][pb], acc[i][j]);
            }
    };
#ifdef SURS_G3_NO_LDS   // experiment: timing without the fragment reads (results are wrong)
#define G3_RD(dst, addr, off) asm volatile("" : "=v"(dst) : "v"(addr) : "memory")
#else
#define G3_RD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#endif
// waits for everything but the n youngest LDS reads; naming the fragments ties their uses to the wait
#define G3_WAIT4(n, pa, pb) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(a[0][pa]), "+v"(a[1][pa]), "+v"(a[2][pa]), "+v"(a[3][pa]), "+v"(b[0][pb]), "+v"(b[1][pb]))
#define G3_WAIT2(n, pa, pb) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(a[0][pa]), "+v"(a[1][pa]), "+v"(b[0][pb]), "+v"(b[1][pb]))
    // A step = phase 1 (fragment reads of stage kt, the first NP products - weight part NP-1-t with point part t - behind each
    // of them an NP-th of the DMAs of stage kt+2, where their issue cost is shared with the matrix pipe) + phase 2 (the
    // remaining products, registers only).  Three bf16 parts: (2,0) (1,1) (0,2) | (1,0) (0,1) (0,0); two f16 parts: (1,0) (0,1) |
    // (0,0).  Fragments are read in order of first use.
    auto phase1 = [&](int kt) {
#ifdef SURS_G3_NO_DMA   // experiment: timing without the in-loop DMAs (results are wrong)
        const bool more = false;
#else
        const bool more = kt + 2 < ktiles;
#endif
        const unsigned sa = a_off + (unsigned)((kt % G3_STAGES) * G3_STAGE);
        const unsigned sb = b_off + (unsigned)((kt % G3_STAGES) * G3_STAGE);
        constexpr int PA = AP * 1024;   // bytes between the weight parts of a stage
#pragma unroll
        for (int t = 0; t < NP; ++t) {
            constexpr int dummy = 0; (void)dummy;
            G3_RD(a[0][NP - 1 - t], sa + (unsigned)((NP - 1 - t) * PA), 0); G3_RD(a[1][NP - 1 - t], sa + (unsigned)((NP - 1 - t) * PA), 1024);
            if constexpr (TI == 4) { G3_RD(a[2][NP - 1 - t], sa + (unsigned)((NP - 1 - t) * PA), 2048); G3_RD(a[3][NP - 1 - t], sa + (unsigned)((NP - 1 - t) * PA), 3072); }
            G3_RD(b[0][t], sb + (unsigned)(t * 8192), 0); G3_RD(b[1][t], sb + (unsigned)(t * 8192), 1024);
        }
#pragma unroll
        for (int t = 0; t < NP; ++t) {
            // everything but the reads of the later products has to be there: (NP - 1 - t) * (TI + 2) reads may still fly
            if constexpr (NP == 3 && TI == 4) { if (t == 0) G3_WAIT4(12, 2, 0); else if (t == 1) G3_WAIT4(6, 1, 1); else G3_WAIT4(0, 0, 2); }
            if constexpr (NP == 3 && TI == 2) { if (t == 0) G3_WAIT2(8, 2, 0); else if (t == 1) G3_WAIT2(4, 1, 1); else G3_WAIT2(0, 0, 2); }
            if constexpr (NP == 2 && TI == 4) { if (t == 0) G3_WAIT4(6, 1, 0); else G3_WAIT4(0, 0, 1); }
            if constexpr (NP == 2 && TI == 2) { if (t == 0) G3_WAIT2(4, 1, 0); else G3_WAIT2(0, 0, 1); }
            if constexpr (NP == 1 && TI == 4) G3_WAIT4(0, 0, 0);
            if constexpr (NP == 1 && TI == 2) G3_WAIT2(0, 0, 0);
            mm(NP - 1 - t, t);
            __builtin_amdgcn_sched_barrier(0);
            if (more)
                for (int d = t * nd / NP; d < (t + 1) * nd / NP; ++d) issue1(kt + 2, d);
        }
    };
    auto phase2 = [&](int kt) {
        if constexpr (NP == 3) {
            mm(1, 0);
            mm(0, 1);
        }
        if constexpr (NP > 1) mm(0, 0);   // (one part: phase 1 was the whole product)
        __builtin_amdgcn_sched_barrier(0);
    };
    // step barrier: my DMAs of stage kt have landed (those of stage kt+1 may be in flight); after the barrier everybody's
    // have, and everybody has finished reading stage kt-1, whose buffer the DMAs of stage kt+2 overwrite
    auto step_barrier = [&](int kt) {
#ifdef SURS_G3_NO_DMA
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
#else
        if (kt + 1 < ktiles) {
            if (nd == 6) asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
            else if (nd == 4) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
            else if (nd == 3) asm volatile("s_waitcnt vmcnt(3)\n\ts_barrier" ::: "memory");
            else if (nd == 1) asm volatile("s_waitcnt vmcnt(1)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
        } else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
#endif
    };
    // Waves w and w+4 share a SIMD.  Half of them run barrier, phase 1, phase 2; the others barrier, phase 2 of
    // the PREVIOUS step (its operands are in registers), phase 1: while one wave waits for its fragment reads or issues
    // DMAs another one has MFMAs to issue (step 5200 -> 4600 cycles, measured with in-kernel cycle stamps; 3072 = MFMA time).
    if (((wave >> 2) & 1) == 0) {
        for (int kt = 0; kt < ktiles; ++kt) {
            step_barrier(kt);
            phase1(kt);
            phase2(kt);
        }
    } else {
        step_barrier(0);
        phase1(0);
        for (int kt = 1; kt < ktiles; ++kt) {
            step_barrier(kt);
            phase2(kt - 1);
            phase1(kt);
        }
        phase2(ktiles - 1);
    }

#undef G3_RD
#undef G3_WAIT4
#undef G3_WAIT2
    // epilogue: acc[i][j][4g + r] is row 32i + 8g + 4kh + r of the wave's rows, column 32j + li; bias, LeakyReLU, split,
    // pair lanes l / l+32 (v_permlane32_swap) so each owns 8 consecutive rows = 16 bytes of the next layer's operand
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long n = n0 + wn * 64 + j * 32 + li;
            const int mrow = m0 + wm * (TI * 32) + i * 32;
            if constexpr (OUT == G3_F32_T) {
                // transposed tile (see mm): 32 lanes write 128 consecutive bytes of one output row [n][ldy]
                const long long nb0 = n0 + wn * 64 + j * 32 + 4 * kh;
                const float bm = bias[mrow + li];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Y[(nb0 + 8 * g + r) * ldy + mrow + li] = acc[i][j][4 * g + r] + bm;
                continue;
            }
            float v[16];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = acc[i][j][4 * g + r] + bias[mrow + 8 * g + 4 * kh + r];
                    v[4 * g + r] = t > 0.0f ? t : 0.01f * t;
                }
            if constexpr (OUT == G3_F32) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Y[(long long)(mrow + 8 * g + 4 * kh + r) * ldy + n] = v[4 * g + r];
            } else
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                unsigned e[NP][2], o[NP][2];
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    unsigned short x0[NP], x1[NP], y0[NP], y1[NP];
                    SK::split(v[8 * q + 2 * d], x0);
                    SK::split(v[8 * q + 2 * d + 1], x1);
                    SK::split(v[8 * q + 4 + 2 * d], y0);
                    SK::split(v[8 * q + 4 + 2 * d + 1], y1);
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        e[p][d] = (unsigned)x0[p] | ((unsigned)x1[p] << 16);
                        o[p][d] = (unsigned)y0[p] | ((unsigned)y1[p] << 16);
                    }
                }
                unsigned short *dst = Ys + ((long long)((mrow >> 4) + q) * np + n) * 16 + kh * 8;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const auto t0 = __builtin_amdgcn_permlane32_swap(e[p][0], o[p][0], false, false);
                    const auto t1 = __builtin_amdgcn_permlane32_swap(e[p][1], o[p][1], false, false);
                    u32x4 w = {t0[0], t1[0], t0[1], t1[1]};
                    *reinterpret_cast<u32x4 *>(dst + p * ys_part) = w;
                }
            }
        }
}



// The affine part's GEMM, R = W1 (g . [a0 | w0z | w0p]) (run_column_batch), for SMALL batches (<= 1024 columns: the ~ 100 runs of a
// surs_query_points_columns call, small slabs, the coarse octree levels).  The 256 x 256-tile kernel above gives such a batch 4 - 6
// workgroups walking K = 1024 - a latency chain of 62 us (two f16 parts) / 34 us (one) per classifier, a quarter of a 50 000-point call
// of the reference's loop.  Here a workgroup takes 64 points x 128 rows (a wave 64 x 32: two accumulator tiles), both classifiers in ONE
// launch (80 workgroups for 256 columns); no LDS: weights and points are read as MFMA fragments straight from their images (16 bytes per
// lane, L2 resident), four k-steps ahead.  The SAME products in the same order on the same instruction as gemm_x3g_kernel<.., G3_F32_T>
// (operands swapped: the tile comes out transposed and its stores run along the output rows): the same bits.
struct RvecSmallArgs {
    const unsigned short *w[2];     // weights of lr / hr: [NP][64 k-tiles][512 / 32 row pieces][64 lanes][8] (MFMA fragment order)
    const unsigned short *g[2];     // points of lr / hr: [NP][64 k-tiles][npm][16], parts g_part[m] halfwords apart
    long long g_part[2];
    long long npm[2];               // points = vectors x columns (a multiple of 64)
    float *r[2];                    // out: [npm][512]
    int wgs0;                       // workgroups of lr (the rest: hr)
};
template <int NP>
__global__ __launch_bounds__(256) void rvec_small_kernel(RvecSmallArgs a) {
    typedef SplitKind<NP> SK;
    typedef typename SK::vec8 vec8;
    constexpr int KT = D1 / 16, PF = 4;
    static_assert(KT % PF == 0, "k-steps in rounds of the prefetch depth");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kh = lane >> 5, li = lane & 31;
    const int m = (int)blockIdx.x >= a.wgs0 ? 1 : 0;
    const int wg = m ? (int)blockIdx.x - a.wgs0 : (int)blockIdx.x;
    const long long npm = a.npm[m];
    const long long n0 = (long long)(wg >> 2) * 64;        // 64 points
    const int m0 = (wg & 3) * 128 + wave * 32;             // 32 of the 512 rows
    const size_t w_part = (size_t)D1 * D2;
    // (the weight image is in A-fragment order: [part][k-tile][row / 32][lane][8] - surs_pack.cpp)
    const unsigned short *wp = a.w[m] + (size_t)(m0 / 32) * 512 + lane * 8;       // + kt * D2 * 16 + p * w_part
    const unsigned short *xp = a.g[m] + ((size_t)n0 + li) * 16 + kh * 8;          // + (kt * npm + 32 j) * 16 + p * g_part
    const long long g_part = a.g_part[m];
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.0f;
    vec8 wf[PF][NP], xf[PF][2][NP];
    auto fetch = [&](int kt, int s) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            wf[s][p] = *reinterpret_cast<const vec8 *>(wp + (size_t)kt * D2 * 16 + p * w_part);
#pragma unroll
            for (int j = 0; j < 2; ++j) xf[s][j][p] = *reinterpret_cast<const vec8 *>(xp + ((size_t)kt * npm + 32 * j) * 16 + p * g_part);
        }
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) fetch(s, s);
    for (int k0 = 0; k0 < KT; k0 += PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            // gemm_x3g_kernel's order: phase 1 = (weight part NP - 1 - t, point part t), t = 0 .. NP - 1; phase 2 = the rest
            vec8 w_[NP], x_[2][NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                w_[p] = wf[s][p];
                x_[0][p] = xf[s][0][p];
                x_[1][p] = xf[s][1][p];
            }
            if (k0 + PF + s < KT) fetch(k0 + PF + s, s);
#pragma unroll
            for (int t = 0; t < NP; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = SK::mfma(x_[j][t], w_[NP - 1 - t], acc[j]);
            if (NP == 3) {
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = SK::mfma(x_[j][0], w_[1], acc[j]);
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = SK::mfma(x_[j][1], w_[0], acc[j]);
            }
            if (NP >= 2) {
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = SK::mfma(x_[j][0], w_[0], acc[j]);
            }
        }
    }
    // register 4 g + r of tile j = point n0 + 32 j + 8 g + 4 kh + r, the lane's column = row m0 + li (bias: zero - added as the other
    // kernel adds its zero bias)
    float *out = a.r[m];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(n0 + 32 * j + 4 * kh + 8 * gq + r) * D2 + m0 + li] = acc[j][4 * gq + r] + 0.0f;
}

// The affine part's GEMM of the bf16 sweep's LARGE batches (one f16 part, > 1024 columns), with its point operand formed in the
// kernel: R = W1 (g . [a0 | w0z | w0p]) straight from the column constants.  colsum_prepare_kernel + two gemm_x3g launches wrote the
// g-scaled f16 image to HBM (335 MB per batch of 32 768 columns) only to read it back once; here the image exists only in LDS.
//   * A workgroup (8 waves) takes 64 columns x 256 of the 512 rows, ALL five vectors of its columns, in two phases: lr (2 vectors
//     = 128 points = 4 point tiles), then hr (3 vectors = 192 points = 6 tiles).  The phases share nothing but the columns (lr reads
//     a0_lr and w0z_lr, hr a0_hr, w0z_hr and w0p_hr), so running them one after the other keeps the accumulators at 6 tiles = 96
//     registers where both together would need 160.  The two row blocks of a column tile are neighbours in gemm_block_tile's
//     order: same XCD, same time - HBM sees a column's a0 once, the second block reads it from L2.
//   * A step = eight k-tiles = 128 channels = 512 consecutive bytes of a column's a0 (four whole cache lines: no half line is left
//     to L2).  Thread (columns fc + 16 q, quad of channels) loads four f32x4 of a0 a step ahead of their use, takes the same
//     channels of w0z / w0p from LDS (copied there once per phase), forms g and the g-scaled values with colsum_prepare_kernel's
//     expressions, converts with SplitKind<1>::split and writes 8 bytes per vector into the stage, which is laid out as the MFMA
//     fragments of the point operand ([k-tile][point tile][half kh][point][8 halfwords], 16 bytes of padding behind every half so
//     that the k-tiles of a wave's writes fall into different banks): a fragment read is one ds_read_b128.  Two stages; the stage
//     of step s + 1 is written behind the barrier that ends step s - 1, a column group behind each of the first four k-tiles'
//     products (plain loads, ds_write, __syncthreads: no counted waits).
//   * A wave takes 32 rows x all point tiles: its weight fragment (h.wt2[m][1], the f16(w) plane in A-fragment order) is its
//     own, read from L2 straight into registers eight k-tiles ahead - 8 KB of weights per k-tile and workgroup.  (The vector
//     memory counter retires in order: a weight fragment that was sent for behind an a0 load cannot be used before that load has
//     come back from HBM, so the weights' distance is what the a0 loads get.)  The fragments of k-tile t + 1 are read while the
//     products of k-tile t run.
// The SAME products in the same order on the same instruction as gemm_x3g_kernel<8, 256, G3_F32_T, 1> and rvec_small_kernel<1>
// (operands swapped, k-tiles ascending, one product per MAC, + 0 for the zero bias): the same bits.
struct RvecFusedArgs {
    const float *cc;                // column constants [ncp][CC_PAD] (rows beyond the batch's columns: anything)
    const float *zvec;
    const unsigned short *w[2];     // weights of lr / hr, first plane: [64 k-tiles][512 / 32 row pieces][64 lanes][8]
    float *r[2];                    // out: [nvec * ncp][512]
    float zmid;
    int tiles;                      // ncp / 64
};
constexpr int RVF_COLS = 64, RVF_ROWS = 256, RVF_THREADS = 512;
constexpr int RVF_KS = 8;                                  // k-tiles per step: 128 channels = 512 bytes of a column's a0
constexpr int RVF_PIECE = 1040, RVF_HALF = 528;            // a fragment in LDS: two halves (kh) of 32 points x 16 bytes, 16 bytes of padding behind each
constexpr int RVF_STAGE_BYTES = RVF_KS * 6 * RVF_PIECE;    // x six point tiles (hr)
constexpr int RVF_Z_BYTES = 2 * D1 * 4;                    // w0z and w0p of the phase's classifier
constexpr int RVF_LDS_BYTES = 2 * RVF_STAGE_BYTES + RVF_Z_BYTES;

template <int M>
__device__ __forceinline__ void rvec_fused_phase(const RvecFusedArgs &a, unsigned char *smem, int col0, int m0) {
    typedef SplitKind<1> SK;
    typedef SK::vec8 vec8;
    constexpr int NV = M ? 3 : 2, NT = 2 * NV;   // vectors per column; 32-point tiles of the 64 columns (NV of them per wave)
    constexpr int KS = RVF_KS, STEPS = D1 / (16 * KS), KT = D1 / 16, PF = RVF_KS, NQ = RVF_COLS / 16, PS = RVF_PIECE;
    static_assert(KS * NT * PS <= RVF_STAGE_BYTES && STEPS % 2 == 0 && KS == PF && KS >= NQ && KS % 2 == 0, "stage size; steps in pairs");
    const int tid = threadIdx.x, lane = tid & 63, kh = lane >> 5, li = lane & 31;
    // forming: thread = (columns fc + 16 q, quad fq of the step's 128 channels): 32 lanes read 512 consecutive bytes of a column;
    // k-tile fq >> 2 of the step, halfwords 4 (fq & 3) .. + 3 of the point's 16 = half (fq & 3) >> 1 of the fragment, bytes
    // 8 (fq & 1) .. + 7 of the lane's 16
    const int fc = tid >> 5, fq = tid & 31;
    const float *crow = a.cc + (size_t)(col0 + fc) * CC_PAD + (M ? CC_A0_HR : CC_A0_LR) + 4 * fq;
    const float zmid = a.zmid;
    float *zs = reinterpret_cast<float *>(smem + 2 * RVF_STAGE_BYTES);   // [w0z | w0p][1024]
    {   // (everybody has left the previous phase's last form: the barrier that ended its last step)
        const int v = tid >> 8, c = 4 * (tid & 255);
        if (M || v == 0)
            *reinterpret_cast<f32x4 *>(zs + v * D1 + c) =
                *reinterpret_cast<const f32x4 *>(a.zvec + (v ? ZV_W0P_HR : (M ? ZV_W0Z_HR : ZV_W0Z_LR)) + c);
    }
    const unsigned wbase = (unsigned)(((fq >> 2) * NT * PS) + (((fq & 3) >> 1) * RVF_HALF) + (fq & 1) * 8);
    auto load = [&](int s, int q) {
        return *reinterpret_cast<const f32x4 *>(crow + (size_t)(16 * q) * CC_PAD + 16 * KS * s);
    };
    // the values of column fc + 16 q and the step's channels 4 fq .. + 3 (wz, wp: the same channels of w0z, w0p) into the stage
    auto form = [&](int q, const f32x4 a0, const f32x4 wz, const f32x4 wp, unsigned char *stage) {
        unsigned short hw[NV][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // (colsum_prepare_kernel's expressions)
            float g, val[3];
            if constexpr (M) {
                g = fmaf(0.5f, wp[e], fmaf(zmid, wz[e], a0[e])) > 0.0f ? 1.0f : 0.01f;
                val[2] = g * wp[e];
            } else {
                g = fmaf(zmid, wz[e], a0[e]) > 0.0f ? 1.0f : 0.01f;
                val[2] = 0.0f;
            }
            val[0] = g * a0[e];
            val[1] = g * wz[e];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                unsigned short p[1];
                SK::split(val[v], p);
                hw[v][e] = p[0];
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int p = (fc + 16 * q) * NV + v;   // point = column * vectors + vector
            *reinterpret_cast<u32x2 *>(stage + wbase + (unsigned)((p >> 5) * PS + (p & 31) * 16)) =
                u32x2{(unsigned)hw[v][0] | ((unsigned)hw[v][1] << 16), (unsigned)hw[v][2] | ((unsigned)hw[v][3] << 16)};
        }
    };
    auto zload = [&](int s, f32x4 &wz, f32x4 &wp) {
        wz = *reinterpret_cast<const f32x4 *>(zs + 16 * KS * s + 4 * fq);
        wp = wz;
        if constexpr (M) wp = *reinterpret_cast<const f32x4 *>(zs + D1 + 16 * KS * s + 4 * fq);
    };
    // (the weight image is in A-fragment order: [k-tile][row / 32][lane][8] - surs_pack.cpp)
    const unsigned short *wp_ = a.w[M] + (size_t)(m0 / 32) * 512 + lane * 8;   // + kt * D2 * 16
    auto wload = [&](int kt) { return *reinterpret_cast<const vec8 *>(wp_ + (size_t)kt * D2 * 16); };
    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.0f;
    vec8 wf[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) wf[k] = wload(k);
    f32x4 ring[NQ];   // a0 of the step to be formed next, sent for again as soon as it has been formed (a step ahead of its use)
#pragma unroll
    for (int q = 0; q < NQ; ++q) ring[q] = load(0, q);
    __syncthreads();   // (w0z, w0p)
    {
        f32x4 wz, wp;
        zload(0, wz, wp);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            form(q, ring[q], wz, wp, smem);
            ring[q] = load(1, q);
        }
    }
    __syncthreads();
    const unsigned char *rd = smem + kh * RVF_HALF + li * 16;
    vec8 x[2][NT];   // the fragments of k-tile t in x[t & 1], read while the products of k-tile t - 1 run
#pragma unroll
    for (int j = 0; j < NT; ++j) x[0][j] = *reinterpret_cast<const vec8 *>(rd + j * PS);
    // (no branches in the loop: the loads and the form beyond the end repeat the last step's - into registers and a stage nobody reads)
#pragma unroll 1
    for (int s2 = 0; s2 < STEPS; s2 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int s = s2 + u;
            // stage u holds step s; everybody has finished reading the other one (step s - 1): step s + 1 is written there, a column
            // group behind each of the first k-tiles' products, and its a0 sent for again
            const int sf = s + 1 < STEPS ? s + 1 : STEPS - 1, sl = s + 2 < STEPS ? s + 2 : STEPS - 1;
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                const int kt = KS * s + t;
                if (t + 1 < KS) {
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        x[(t + 1) & 1][j] = *reinterpret_cast<const vec8 *>(rd + u * RVF_STAGE_BYTES + ((t + 1) * NT + j) * PS);
                }
                __builtin_amdgcn_sched_barrier(0);
                const vec8 w = wf[t];
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = SK::mfma(x[t & 1][j], w, acc[j]);
                if (t < NQ) {
                    f32x4 wz, wp;
                    zload(sf, wz, wp);
                    form(t, ring[t], wz, wp, smem + (u ^ 1) * RVF_STAGE_BYTES);
                    ring[t] = load(sl, t);
                }
                wf[t] = wload(kt + PF < KT ? kt + PF : KT - 1);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NT; ++j) x[0][j] = *reinterpret_cast<const vec8 *>(rd + (u ^ 1) * RVF_STAGE_BYTES + j * PS);
        }
    }
    // register 4 g + r of tile j = point 32 j + 8 g + 4 kh + r of the workgroup's NV x 64, the lane's column = row m0 + li (+ 0: the
    // other kernels' zero bias)
    float *out = a.r[M] + (size_t)col0 * NV * D2 + m0 + li;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(32 * j + 4 * kh + 8 * gq + r) * D2] = acc[j][4 * gq + r] + 0.0f;
}

__global__ __launch_bounds__(RVF_THREADS) void rvec_fused_kernel(RvecFusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rvf_smem[];
    int mb, nb;
    if (!gemm_block_tile(D2 / RVF_ROWS, a.tiles, mb, nb)) return;   // (the whole workgroup)
    const int col0 = nb * RVF_COLS, m0 = mb * RVF_ROWS + (int)(threadIdx.x >> 6) * 32;   // a wave: 32 rows x all point tiles
    rvec_fused_phase<0>(a, rvf_smem, col0, m0);
    rvec_fused_phase<1>(a, rvf_smem, col0, m0);
}
