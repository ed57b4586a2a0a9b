// Included by surs_query.hip inside namespace surs, after surs_grid_v10.inc (uses the helpers of surs_grid_restated.inc).
//
// Grid column kernel, version 12 (reduced-precision sweep): v10's arithmetic, bit for bit, as TWO workgroups of four waves per
// compute unit, with layer 1 STREAMED into layer 2 by chunks of 32 rows (the design NOTES R4.3 left for "a later round"; what it
// measured, what was tried on top and the power-limit reading of the result: NOTES R5.2, R5.3).
//
// Why.  In v10 one workgroup owns the CU and its eight waves walk the same phases together: while they classify, build the list,
// generate residuals, publish activations or reduce layer 4 the matrix pipes idle (busy 0.38).  Every earlier attempt to put a
// second tile under those phases lost to ONE number: y1 of a 128-voxel tile is 512 rows x 128 voxels x 2 B = 128 KiB of the CU's
// 160 KiB of LDS.  But layer 2 consumes y1 sixteen rows per k-step, and a row of y1 costs only the affine k-step + the listed
// channels of layer 1.  So y1 never exists as a whole here:
//
//     for chunk j = 0 .. 15 (rows 32 j .. 32 j + 31 of y1 = layer-2 k-steps 2 j, 2 j + 1):
//         layer 1 of the chunk (wave w = column tile w: one 32 x 32 accumulator tile, 1 + |listed| / 16 MFMAs),
//         LeakyReLU + convert -> ring[j & 1] (8 KiB), barrier,
//         layer 2's k-steps 2 j, 2 j + 1 (wave w = rows [64 w, 64 w + 64): its 128 accumulator registers live across the chunks)
//
// with layer 1 of chunk j + 1 issued in front of layer 2 of chunk j (one barrier per chunk).  What layer 1 needs per chunk:
//   * A operand: the 64-byte pieces [64 j, 64 j + 64) of the listed channels' rows of W1t - a SLICE of 1 KiB per k-step, fetched
//     two chunks ahead with plain global loads into registers (wave w: k-steps w, w + 4, ..), stored to a double-buffered LDS
//     image whose 64-byte row stride makes the transposing reads (ds_read_b64_tr_b16) conflict-free as it lies;
//   * B operand: the residual fragments of the wave's OWN column tile - generated once per tile by the wave that uses them, from
//     the listed channels' constants which the classification leaves compacted in LDS (six ds_read_b128 per fragment instead of
//     v10's 24 dependent ds_read_b32), the first V12_KR = 4 k-steps' kept in registers, the rest (up to V12_KCAP) in a wave-private
//     LDS area; no barrier between generation and use;
//   * the affine part's A fragment of the chunk's row tile: ONE 16-byte load per lane, one chunk ahead, from the workgroup's fragment
//     image in global memory.  The fragment depends on column, classifier and chunk only, so the per-column part builds the column's
//     32 fragments ONCE from the R vectors and b1 (v12_affine_build: 8 fragment lanes per thread, v10's expressions and slot order)
//     instead of every wave in every z tile (16 times per column and classifier: 794 vector instructions and 80 loads per tile).  The
//     image (32 KiB per workgroup) lies in the g-scaled split image of the workspace, dead since the R GEMMs, behind the overflow list;
//     it is written and read by waves of ONE workgroup on one CU, published by the barrier that ends the per-column part.
// LDS per workgroup: ring 16 KiB + slices 2 x 8 KiB + residual fragments 4 x 4 KiB + compacted constants 1.5 KiB, overlaid by y2
// (64 KiB) once layer 2 is done; + 6.1 KiB of small tables = 71 808 B: two workgroups per CU, whose phases drift apart - one's
// vector / LDS phases run under the other's MFMAs.  256 registers per wave, none spilled: every per-lane value that is needed at
// the END of an item (or in the per-column part) is made there from fresh_lane() instead of living through the item (NOTES R6.5).
// As shipped (hipcc -O3 -ffp-contract=off, gfx950): bf16 66 688 B of code, 251 registers, no scratch; fp16 66 424 B, 249, none -
// 4 674 vector instructions per tile without the 928 MFMAs (NOTES "affine fragments once per column").  The layer-0 constants (a0, w0z, w0p) are no longer copied to LDS: the classification reads them from
// L2 (they are only needed there and, compacted, for the listed channels).
//
// Same list order (v7's), same k order in every layer, same four layer-4 partial sums: v12 reproduces v10's bits
// (tests/test_gpu_fullvolume.py).  A tile that lists more than 16 KCAP = 128 channels (either classifier) is not evaluated here: the
// workgroup appends it to a list, and kernel v10 in its tile mode runs over that list right behind this launch (same bits; a slow
// path inside this kernel lengthened live ranges on the path every other tile takes: 33 -> 200 spilled registers).  The host's
// probe sends fields that list that many channels per tile to v10 as a whole.
constexpr int V12_THREADS = 256;
#ifndef SURS_V12_KR
#define SURS_V12_KR 4   // (per 128-plane slab, round 5 - with 16 - 38 spilled registers -: 0 -> 27.3 ms, 3 -> 27.6, 6 -> 30.4; round 6, once nothing
                        //  was spilled any more: 0 -> 27.15, 2 -> 26.85; and with the item's lane index made per item: 2 -> 26.32, 4 -> 26.13,
                        //  5 / 6 the same as 4 (6 spills two registers): the LDS pipe is as busy as the matrix pipe;
                        //  with the affine fragments read from the per-column image: 4 -> 25.40, 25.29, 5 -> 25.24, 25.30, 6 -> 25.25, 25.22: within the spread)
#endif
#ifndef SURS_V12_KCAP
#define SURS_V12_KCAP 8   // (round 6, 128-plane slab, same box, same hash: 9 -> 28.80 ms, 8 -> 28.55, 7 -> 28.7; 16 spilled registers against 23;
                          //  with the per-column fragment image: 9 -> 25.50, 25.36, 8 -> 25.40, 25.29)
#endif
constexpr int V12_KR = SURS_V12_KR, V12_KCAP = SURS_V12_KCAP;
static_assert(V12_KR <= V12_KCAP, "register-resident k-steps are a prefix of the staged ones");
constexpr int V12_NSL = (V12_KCAP + 3) / 4;              // slice k-steps per wave
constexpr int V12_RING = 0;                              // [2][2 k-steps][4 column tiles][1 KiB]
constexpr int V12_SLICE = 16384;                         // [2][KCAP][16 channels][64 B]
constexpr int V12_BOV = V12_SLICE + 2 * V12_KCAP * 1024; // [KCAP - KR][4 column tiles][1 KiB]: residual fragments beyond the registers
constexpr int V12_LISTC = V12_BOV + (V12_KCAP - V12_KR) * 4096;   // a0, w0z, w0p of the listed channels: 3 x [16 KCAP] fp32
constexpr int V12_NLC = 16 * V12_KCAP;
constexpr int V12_YEND = (V12_LISTC + 3 * V12_NLC * 4) > 65536 ? (V12_LISTC + 3 * V12_NLC * 4) : 65536;   // (y2: [0, 65536))
constexpr int V12_W4C = V12_YEND;                        // w4c_lr[128], w4c_hr[128]
constexpr int V12_SC = V12_W4C + 1024;                   // a4_lr, a4_hr, w4z_lr, w4z_hr, w4p_hr
constexpr int V12_PART = V12_SC + 64;                    // layer-4 partial sums [4][128]
constexpr int V12_LIST = V12_PART + 2048;                // ushort [1024 + 16]
constexpr int V12_CNT = V12_LIST + (1024 + 16) * 2;      // wave counts [4], the column slot
constexpr int V12_ZTAB = V12_CNT + 32;                   // the tile's zf [128] and p_lr [128]
constexpr int GRID12_LDS_BYTES = V12_ZTAB + 1024;
static_assert(V12_LISTC % 16 == 0 && GRID12_LDS_BYTES <= 81920, "two workgroups per CU");

#ifdef SURS_V3_TRACE
// diagnostic builds: wave 0 of workgroup SURS_V12_TRACE_WG (default 100) sums, over every item it runs, the cycles between the
// stamps (g_v12_acc[M][i] = phase ending at stamp i, [M][0] = items, [M][15] = residual k-steps); the single-tile stamps of the
// v3 trace as well
__device__ unsigned long long g_v12_acc[2][16];
#ifndef SURS_V12_TRACE_WG
#define SURS_V12_TRACE_WG 100
#endif
#define V12_STAMP(i)                                                          \
    do {                                                                      \
        if (v12_tr) g_v3_trace[(i) + 16 * M] = __builtin_readcyclecounter(); \
        if (v12_ac) {                                                         \
            const unsigned long long now_ = __builtin_readcyclecounter();    \
            if ((i) == 0) g_v12_acc[M][0] += 1; else g_v12_acc[M][(i)] += now_ - v12_t0; \
            v12_t0 = now_;                                                    \
        }                                                                     \
    } while (0)
#else
#define V12_STAMP(i) do { } while (0)
#endif

// ---- the affine part's A fragments of a column: the workgroup's image in global memory [classifier 2][chunk 16][lane 64][16 B]
constexpr int V12_AIMG_MLP = 16 * 64 * 16;         // one classifier's 16 chunks
constexpr int V12_AIMG_BYTES = 2 * V12_AIMG_MLP;   // 32 KiB per workgroup

// The A fragment of one 32-row chunk for fragment lane (row = lane & 31, half hh = lane >> 5), v10's slot order, from the column's
// vectors R and b1: raw = {RA[row], RB[row], RC[row] (hr), b1[row]}.
template <int DT, int M>
__device__ __forceinline__ typename HalfT<DT>::vec8 v12_affine_frag(const float (&raw)[4], unsigned hh) {
    typedef typename HalfT<DT>::vec8 vec8;
    typedef typename HalfT<DT>::elem elem;
    const elem zero = (elem)0.0f;
    elem pa[3], pb[3], pc[3] = {zero, zero, zero};
    split3_elem<DT>(raw[0] + raw[3], pa);
    split3_elem<DT>(raw[1], pb);
    if (M) split3_elem<DT>(raw[2], pc);
    const vec8 flo = {pa[0], pa[1], pa[2], pb[0], pb[0], pb[1], pb[0], pb[1]};
    const vec8 fhi = {pb[2], pc[0], pc[0], pc[1], pc[0], pc[1], pc[2], zero};
    const vec8 r = hh ? fhi : flo;
    return r;
}

// The column's 32 fragments, built by the workgroup's 256 threads: wave w the chunks w, w + 4, w + 8, w + 12 of both classifiers,
// lane = fragment lane.  Called between the two barriers of the per-column part: every wave's loads of the previous column's image
// have returned (the last one is consumed in stage 15 of the column's last item), and the barrier that ends the per-column part
// publishes the stores to the workgroup's other waves (one CU, one L1: workgroup scope).  All loads first: the image may alias R for
// all the compiler knows, and a load behind a store would wait for one more trip to L2 per fragment.
template <int DT>
__device__ __forceinline__ void v12_affine_build(const float *rv_lr /* [2][512] */, const float *rv_hr /* [3][512] */, const float *zvec,
                                                 char *img, int wave, unsigned fl) {
    typedef typename HalfT<DT>::vec8 vec8;
    const unsigned o = 128u * (unsigned)wave + (fl & 31u) * 4u;   // + 512 i: row 32 (w + 4 i) + (lane & 31)
    const char *rl = reinterpret_cast<const char *>(rv_lr) + o, *rh = reinterpret_cast<const char *>(rv_hr) + o;
    const char *bl = reinterpret_cast<const char *>(zvec + ZV_B1_LR) + o, *bh = reinterpret_cast<const char *>(zvec + ZV_B1_HR) + o;
    auto f = [](const char *p, int imm) { return *reinterpret_cast<const float *>(p + imm); };
    float raw[2][4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        raw[0][i][0] = f(rl, 512 * i);
        raw[0][i][1] = f(rl, 4 * D2 + 512 * i);
        raw[0][i][2] = 0.0f;
        raw[0][i][3] = f(bl, 512 * i);
        raw[1][i][0] = f(rh, 512 * i);
        raw[1][i][1] = f(rh, 4 * D2 + 512 * i);
        raw[1][i][2] = f(rh, 8 * D2 + 512 * i);
        raw[1][i][3] = f(bh, 512 * i);
    }
    char *dst = img + 1024u * (unsigned)wave + 16u * fl;   // + M * V12_AIMG_MLP + 4096 i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<vec8 *>(dst + 4096 * i) = v12_affine_frag<DT, 0>(raw[0][i], fl >> 5);
        *reinterpret_cast<vec8 *>(dst + V12_AIMG_MLP + 4096 * i) = v12_affine_frag<DT, 1>(raw[1][i], fl >> 5);
    }
}

// Every per-lane offset below is a 32-bit value derived, inside the item, from ONE opaque copy of the lane index: hipcc hoists
// whatever depends on the lane index alone out of the tile and column loops (hundreds of values: fragment addresses, list positions,
// 64-bit pointers) and then spills them - kernel-long live ranges for what is one VALU instruction away.  Global loads are
// (uniform base) + (32-bit per-lane offset) + immediate; LDS accesses (one per-lane base) + immediate.
template <int DT, int M>
__device__ __forceinline__ bool grid_mlp_v12(const char *__restrict__ wbase /* this MLP's 42 slabs */,
                                             const float *__restrict__ gcc /* this column's constants (global) */,
                                             const float *__restrict__ gzv /* z-vectors (global) */,
                                             const unsigned short *__restrict__ w1t /* this MLP's W1t [1024][512] */,
                                             const char *aimg /* this column's and MLP's affine A fragments: [16 chunks][64 lanes][16 B] */,
                                             float zmid, float zlo, float zhi, float plo, float phi, char *smem, int wave, int lane_in,
                                             float (&logit)[4], unsigned &ksteps) {
    typedef HalfT<DT> H;
    typedef typename H::vec8 vec8;
    typedef typename H::elem elem;
    unsigned lz = 0;
    asm volatile("" : "+s"(lz));
    gcc += lz;
    gzv += lz;
    wbase += lz;
    w1t += lz;
    aimg += lz;
    constexpr int GA0 = M ? CC_A0_HR : CC_A0_LR, GW0Z = M ? ZV_W0Z_HR : ZV_W0Z_LR, GW0P = ZV_W0P_HR;
    constexpr int W4C = V12_W4C + 512 * M;
    constexpr int GA2 = M ? CC_A2_HR : CC_A2_LR, GA3 = M ? CC_A3_HR : CC_A3_LR;
    constexpr int GW2Z = M ? ZV_W2Z_HR : ZV_W2Z_LR, GW2P = ZV_W2P_HR,
                  GW3Z = M ? ZV_W3Z_HR : ZV_W3Z_LR, GW3P = ZV_W3P_HR;
    const unsigned ol = opaque((unsigned)lane_in);                // THE lane index of this item
    const unsigned uw = (unsigned)wave;                           // wave-uniform
    const unsigned hh = ol >> 5;
    const unsigned lane16 = ol * 16u;
    // global loads: uniform base + 32-bit per-lane byte offset + immediate
    auto gld4 = [&](const void *base, unsigned voff, int imm) { return *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(base) + (size_t)voff + imm); };
    auto gldw = [&](unsigned voff, int imm) { return *reinterpret_cast<const vec8 *>(wbase + (size_t)voff + imm); };
    auto lds4 = [&](unsigned off, int imm) { return *reinterpret_cast<const f32x4 *>(smem + off + imm); };
    auto ldsB = [&](unsigned off, int imm) { return *reinterpret_cast<const vec8 *>(smem + off + imm); };
    auto cvt8 = [&](const f32x16 &t, int u) {
        // (v10's: scalar products, one maximum per value - same bits, and faster beside MFMAs than v_pk_mul_f32)
        vec8 b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (elem)lrelu01(t[8 * u + j]);
        return b;
    };
#ifdef SURS_V3_TRACE
    const bool v12_tr = g_v3_trace_on && blockIdx.x == 0 && wave == 0 && lane_in == 0;
    const bool v12_ac = blockIdx.x == SURS_V12_TRACE_WG && wave == 0 && lane_in == 0;
    unsigned long long v12_t0 = 0;
#endif
    V12_STAMP(0);
    const unsigned tid = uw * 64u + ol;
    unsigned short *list = reinterpret_cast<unsigned short *>(smem + V12_LIST);
    float *lc = reinterpret_cast<float *>(smem + V12_LISTC);   // a0 [NLC], w0z [NLC], w0p [NLC]
    int *cnt = reinterpret_cast<int *>(smem + V12_CNT);

    // ================= classification (v10's, four channels per thread, constants from L2) =================
    const unsigned ch0 = 4u * tid;   // = 256 wave + 4 lane: the list comes out in v7's order
    // (fetching them one item ahead, behind the previous item's layer 3, was measured: 12 more registers alive at the item's start
    //  cost more in the stream than the hidden L2 latency gave back - 30.5 against 29.6 ms per 128-plane slab)
    const f32x4 ca4 = gld4(gcc, ch0 * 4u, GA0 * 4), cz4 = gld4(gzv, ch0 * 4u, GW0Z * 4);
    f32x4 cp4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (M) cp4 = gld4(gzv, ch0 * 4u, GW0P * 4);
    // layer 2's accumulator-initialisation constants of this wave's first row tile: issued here, used behind the list (their L2
    // latency passes under the classification and the two barriers)
    const unsigned c2o = (hh * 4u + uw * 64u) * 4u;   // layer-2 output channel 64 w + 32 rt + 8 g + 4 h + r
    f32x4 c2v[4], wz2v[4], wp2v[4];
    auto acc2_consts = [&](int rt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            c2v[g] = gld4(gcc, c2o, (GA2 + 32 * rt + 8 * g) * 4);
            wz2v[g] = gld4(gzv, c2o, (GW2Z + 32 * rt + 8 * g) * 4);
            if (M) wp2v[g] = gld4(gzv, c2o, (GW2P + 32 * rt + 8 * g) * 4);
        }
    };
    acc2_consts(0);
    unsigned flags = 0, upper = 0;   // upper: the channel's branch at mid column is the identity (g = 1)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float xm = fmaf(zmid, cz4[i], ca4[i]);
        if (M) xm = fmaf(0.5f, cp4[i], xm);
        upper |= (xm > 0.0f) ? (1u << i) : 0u;
        const float t0 = cz4[i] * zlo, t1 = cz4[i] * zhi;
        float mn = ca4[i] + fminf(t0, t1), mx = ca4[i] + fmaxf(t0, t1);
        if (M) {
            const float u0 = cp4[i] * plo, u1 = cp4[i] * phi;
            mn += fminf(u0, u1);
            mx += fmaxf(u0, u1);
        }
        const bool constant = (xm > 0.0f) ? (mn > 0.0f) : (mx <= 0.0f);
        flags |= constant ? 0u : (1u << i);
    }
    unsigned long long bl[4];
    int nb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bl[i] = __ballot(flags & (1u << i));
        nb[i] = __popcll(bl[i]);
    }
    if (ol == 0) cnt[wave] = (nb[0] + nb[1]) + (nb[2] + nb[3]);
    __syncthreads();   // wave counts
    int base = 0, E = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cnt[i];
        base += (i < wave) ? c : 0;
        E += c;
    }
    E = __builtin_amdgcn_readfirstlane(E);
    const int ks = (E + 15) >> 4;              // residual k-steps of this tile
    if (ks > V12_KCAP) return false;           // (workgroup-uniform) more listed channels than the stream stages: the tile goes to v10
    ksteps += (unsigned)ks;
#ifdef SURS_V3_TRACE
    if (v12_ac) g_v12_acc[M][15] += (unsigned long long)ks;
#endif
    {
        const unsigned long long lt = (1ull << ol) - 1ull;
        int pos = base;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (flags & (1u << i)) {
                const int e = pos + __popcll(bl[i] & lt);
                list[e] = (unsigned short)(ch0 + i);
                if (e < V12_NLC) {
                    // the constants leave with the sign that turns the residual into ONE clamp: v10's
                    //     res = g ? -0.99 min(x, 0) : 0.99 max(x, 0),  x = a0 + w0z zf (+ w0p p)
                    // is 0.99 max(s x, 0) with s = g ? -1 : +1, and s x is the same fma chain on the negated constants (negation
                    // is exact, the roundings are symmetric): the same bits for five vector instructions per channel and lane
                    // instead of thirteen (sign tests, bound selects, a median) - and the residuals sit on every item's critical path:
                    // 29.5 -> 28.5 ms per 128-plane slab
                    const float sg = (upper & (1u << i)) ? -1.0f : 1.0f;
                    lc[e] = sg * ca4[i];
                    lc[V12_NLC + e] = sg * cz4[i];
                    lc[2 * V12_NLC + e] = sg * cp4[i];
                }
            }
            pos += nb[i];
        }
        if (tid < 16) {   // padding up to the k-step: channel 0's weights, zero residual (finite constants)
            const int e = E + (int)tid;
            list[e] = 0;
            if (e < V12_NLC) lc[e] = lc[V12_NLC + e] = lc[2 * V12_NLC + e] = 0.0f;
        }
    }
    __syncthreads();   // list
    V12_STAMP(1);
#ifdef SURS_V3_TRACE
    if (v12_tr) g_v3_trace[48 + M] = (unsigned long long)E;
#endif
    const int ksl = ks;   // k-steps staged through LDS slices

    // ================= slices of chunks 0 and 1: wave w fetches the k-steps w, w + 4, .. =================
    const char *w1b = reinterpret_cast<const char *>(w1t);
    unsigned soff[V12_NSL];
    const unsigned slw = (unsigned)V12_SLICE + lane16 + uw * 1024u;     // + (buf * KCAP + 4 i) * 1024
    u32x4 s0[V12_NSL], s1[V12_NSL];
#pragma unroll
    for (int i = 0; i < V12_NSL; ++i) {
        const int s = wave + 4 * i;
        soff[i] = 0;
        if (s < ksl) {
            soff[i] = (unsigned)list[16 * s + (ol >> 2)] * 1024u + 16u * (ol & 3u);
            s0[i] = *reinterpret_cast<const u32x4 *>(w1b + (size_t)soff[i]);
            s1[i] = *reinterpret_cast<const u32x4 *>(w1b + (size_t)soff[i] + 64);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ================= layer 2's accumulators: rows [64 w, 64 w + 64) = row tiles 2 w, 2 w + 1 (the first one while the slices fly)
    const unsigned zt = (unsigned)V12_ZTAB + (ol & 31u) * 4u;   // the tile's table: zf [ct * 32], p [128 + ct * 32]
    auto ztab = [&](int imm) { return *reinterpret_cast<const float *>(smem + zt + imm * 4); };
    f32x16 acc2[2][4];
    auto acc2_init = [&](int rt) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const float zfc = ztab(ct * 32), pc = M ? ztab(128 + ct * 32) : 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = fmaf(zfc, wz2v[g][r], c2v[g][r]);
                    if (M) t = fmaf(pc, wp2v[g][r], t);
                    acc2[rt][ct][4 * g + r] = t;
                }
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) asm volatile("" : "+v"(acc2[rt][ct]));
    };
    acc2_init(0);
    __builtin_amdgcn_sched_barrier(0);
    acc2_consts(1);
#pragma unroll
    for (int i = 0; i < V12_NSL; ++i) {
        const int s = wave + 4 * i;
        if (s < ksl) {
            *reinterpret_cast<u32x4 *>(smem + slw + (4 * i) * 1024) = s0[i];
            *reinterpret_cast<u32x4 *>(smem + slw + (V12_KCAP + 4 * i) * 1024) = s1[i];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ================= the wave's own column tile: affine B fragment, residual B fragments =================
    const float zf_own = *reinterpret_cast<const float *>(smem + zt + uw * 128u);
    const float p_own = M ? *reinterpret_cast<const float *>(smem + zt + 512u + uw * 128u) : 0.0f;
    vec8 bi;
    {
        const elem zero = (elem)0.0f, one = (elem)1.0f;
        elem z[3], p[3] = {zero, zero, zero};
        split3_elem<DT>(zf_own, z);
        if (M) split3_elem<DT>(p_own, p);
        const vec8 lo = {one, one, one, z[0], z[1], z[0], z[2], z[1]};
        const vec8 hi = {z[0], p[0], p[1], p[0], p[2], p[1], p[0], zero};
        bi = hh ? hi : lo;
    }
    const unsigned lcb = (unsigned)V12_LISTC + hh * 32u;   // entries 16 s + 8 h .. + 7: + s * 64
    auto residual = [&](int s) {   // (v10's values; the listed channels' signed constants lie compacted: b128 reads, broadcast;
                                   //  the padding entries' constants are zero: residual zero)
        float ca[8], cz[8], cp[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4 a = lds4(lcb, s * 64 + q * 16), z = lds4(lcb, V12_NLC * 4 + s * 64 + q * 16);
            f32x4 p = {0.0f, 0.0f, 0.0f, 0.0f};
            if (M) p = lds4(lcb, 2 * V12_NLC * 4 + s * 64 + q * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ca[4 * q + r] = a[r];
                cz[4 * q + r] = z[r];
                cp[4 * q + r] = p[r];
            }
        }
        vec8 bf;
        constexpr float K99 = 1.0f - 0.01f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = fmaf(zf_own, cz[j], ca[j]);
            if (M) x = fmaf(p_own, cp[j], x);
            float r = K99 * fmaxf(x, 0.0f);
            SURS_ISA_PIN(r);   // (rounded to fp32, then converted - as in v10: no v_fma_mixlo_f16 fold of the product)
            bf[j] = (elem)r;
        }
        return bf;
    };
    vec8 bres[V12_KR > 0 ? V12_KR : 1];
#pragma unroll
    for (int s = 0; s < V12_KR; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bres[s][j] = (elem)0.0f;
        if (s < ks) bres[s] = residual(s);
    }
    const unsigned bov = (unsigned)V12_BOV + lane16 + uw * 1024u;     // + (s - KR) * 4096
#pragma unroll
    for (int s = V12_KR; s < V12_KCAP; ++s)
        if (s < ks) *reinterpret_cast<vec8 *>(smem + bov + (s - V12_KR) * 4096) = residual(s);
    V12_STAMP(2);
    __builtin_amdgcn_sched_barrier(0);
    acc2_init(1);
    __builtin_amdgcn_sched_barrier(0);
    // ---- the affine part's A fragment of a chunk's row tile: ONE 16-byte load per lane from the image the per-column part built
    //      (v12_affine_build): (a UNIFORM base stepped by the chunk's 1 KiB, in scalar registers) + (32-bit per-lane offset), no
    //      immediate and no vector instruction (NOTES "affine fragments once per column": the forms hipcc made of the others).
    vec8 anext;
    unsigned al16 = lane16;   // (a copy of its own, re-made opaque in place in front of every load: the 64-bit extension of a value made
                              //  once per item is hoisted into a register PAIR, and the load then takes a 64-bit vector add per chunk)
    auto affine_load = [&](int j) {
        const char *cb = aimg + 1024 * j;
        asm volatile("" : "+s"(cb), "+v"(al16));
        typedef const __attribute__((address_space(1))) char global_char;   // (behind the asm the pointer's address space is unknown: a FLAT load otherwise)
        typedef const __attribute__((address_space(1))) vec8 global_vec8;
        anext = *(global_vec8 *)((global_char *)cb + (size_t)al16);
    };
    affine_load(0);
    vec8 ai = anext;
    // ---- layer 2's weights: per k-step the fragments of row tiles 2 w, 2 w + 1 (2 KiB of the k-step's 8 KiB); each fragment is
    //      reloaded in place, for the next stage, right after its last MFMA of this stage
    vec8 a2[2][2];   // [k-step of the stage][row tile]
    unsigned vb = opaque(lane16 + (unsigned)(V3_F_L2 * 1024) + 2048u * uw);
#pragma unroll
    for (int u = 0; u < 2; ++u) {   // k-steps 0, 1: consumed in stage 1
        a2[u][0] = gldw(vb, 0);
        a2[u][1] = gldw(vb, 1024);
        vb = opaque(vb + 8192u);
    }
    __syncthreads();   // slices of chunks 0, 1 visible
    V12_STAMP(3);

    // ================= the stream: stage j = layer 1 of chunk j, layer 2 of chunk j - 1 =================
    const unsigned trb = (unsigned)V12_SLICE + (8u * hh + ((ol & 15u) >> 2)) * 64u + (16u * ((ol >> 4) & 1u) + 4u * (ol & 3u)) * 2u;
    auto ldA = [&](int buf, int s) {
        typedef short v4s __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) v4s lds_v4s;
        const char *b = smem + trb + (buf * V12_KCAP + s) * 1024;
        const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)b);
        const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)(b + 256));
        typedef short v8s __attribute__((ext_vector_type(8)));
        const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(vec8, r);
    };
    const unsigned yw = lane16 + uw * 1024u;          // ring writes: + buf * 8192 + u * 4096; ring reads: lane16 + buf * 8192 + (u * 4 + ct) * 1024
    u32x4 sreg[V12_NSL];
    f32x16 acc1;
#pragma unroll
    for (int j = 0; j <= 16; ++j) {
        // ---- top: the slices of chunk j + 1 (fetched during stage j - 1) into the buffer stage j - 1 read; fetch chunk j + 2
        if (j >= 1 && j + 1 <= 15) {
#pragma unroll
            for (int i = 0; i < V12_NSL; ++i)
                if (wave + 4 * i < ksl) *reinterpret_cast<u32x4 *>(smem + slw + (((j + 1) & 1) * V12_KCAP + 4 * i) * 1024) = sreg[i];
        }
        if (j + 2 <= 15) {
#pragma unroll
            for (int i = 0; i < V12_NSL; ++i)
                if (wave + 4 * i < ksl) sreg[i] = *reinterpret_cast<const u32x4 *>(w1b + (size_t)soff[i] + 64 * (j + 2));
        }
        if (j + 1 <= 15) affine_load(j + 1);
        vec8 bc[4];
        if (j >= 1) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bc[ct] = ldsB(lane16, V12_RING + ((j - 1) & 1) * 8192 + ct * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- layer 1 of chunk j: the affine k-step, then the listed k-steps in list order (operands read three k-steps at a time)
        if (j <= 15) {
            f32x16 z;
#pragma unroll
            for (int q = 0; q < 16; ++q) z[q] = 0.0f;
            vec8 af[3], bf[3];
            auto read3 = [&](int g) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int s = 3 * g + t;
                    if (s < V12_KCAP) {
                        af[t] = ldA(j & 1, s);
                        if (s >= V12_KR) bf[t] = ldsB(bov, (s - V12_KR) * 4096);
                    }
                }
            };
            if (ks > 0) read3(0);
            acc1 = H::mfma(ai, bi, z);
#pragma unroll
            for (int g = 0; g < (V12_KCAP + 2) / 3; ++g) {
                if (ks > 3 * g) {
                    if (g > 0) read3(g);
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const int s = 3 * g + t;
                        if (s < V12_KCAP && s < ks) acc1 = H::mfma(af[t], s < V12_KR ? bres[s < V12_KR ? s : 0] : bf[t], acc1);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- layer 2 on chunk j - 1 (k-steps 2 (j - 1), + 1); the chunk just computed is converted and stored under it
        if (j >= 1) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) {
                        acc2[rt][ct] = H::mfma(a2[u][rt], bc[ct], acc2[rt][ct]);
                        if (rt == 1 && u == 0) bc[ct] = ldsB(lane16, V12_RING + ((j - 1) & 1) * 8192 + (4 + ct) * 1024);
                        if (ct == 3 && j + 1 <= 16) {   // k-step 2 j + u, consumed in stage j + 1
                            a2[u][rt] = gldw(vb, rt * 1024);
                            if (rt == 1) vb = opaque(vb + 8192u);
                        }
                        if (j <= 15 && rt == 0 && ct == 1)
                            *reinterpret_cast<vec8 *>(smem + yw + V12_RING + (j & 1) * 8192 + u * 4096) = cvt8(acc1, u);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<vec8 *>(smem + yw + V12_RING + (j & 1) * 8192 + u * 4096) = cvt8(acc1, u);
        }
        if (j + 1 <= 15) ai = anext;
        __builtin_amdgcn_sched_barrier(0);
        if (j <= 15) __syncthreads();   // chunk j in the ring; everyone is done with ring[(j - 1) & 1] and slice buffer j & 1
#ifdef SURS_V3_TRACE
        if (j == 8) V12_STAMP(4);
#endif
    }
    V12_STAMP(5);
    // ================= publish y2 (over the ring and the slices: every wave must be done with them); layer 3's first loads before it
    const unsigned rt3 = uw;                                        // layer-3 row tile of this wave
    vec8 a3r[8];
    unsigned vc = opaque(lane16 + (unsigned)(V3_F_L3 * 1024) + 1024u * rt3);
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        a3r[q] = gldw(vc, 0);
        vc = opaque(vc + 4096u);
    }
    f32x4 c3v[4], wz3v[4], wp3v[4];
    {
        const unsigned c3o = (hh * 4u + rt3 * 32u) * 4u;   // layer-3 output channel 32 w + 8 g + 4 h + r
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            c3v[g] = gld4(gcc, c3o, (GA3 + 8 * g) * 4);
            wz3v[g] = gld4(gzv, c3o, (GW3Z + 8 * g) * 4);
            if (M) wp3v[g] = gld4(gzv, c3o, (GW3P + 8 * g) * 4);
        }
    }
    __syncthreads();
    {
        const unsigned yw2 = lane16 + uw * 16384u;  // row tiles 2 w, 2 w + 1 = k-step slots 4 w .. 4 w + 3
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    *reinterpret_cast<vec8 *>(smem + yw2 + ((2 * rt + u) * 4 + ct) * 1024) = cvt8(acc2[rt][ct], u);
    }
    V12_STAMP(6);
    // ================= layer 3: row tile w, K = 256 (16 k-steps) =================
    f32x16 acc3[4];
    const float *zt3 = reinterpret_cast<const float *>(smem + V12_ZTAB) + (fresh_lane() & 31u);   // (not `zt`: it would live through the stream)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const float zfc = zt3[ct * 32], pc = M ? zt3[128 + ct * 32] : 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = fmaf(zfc, wz3v[g][r], c3v[g][r]);
                if (M) v = fmaf(pc, wp3v[g][r], v);
                acc3[ct][4 * g + r] = v;
            }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) asm volatile("" : "+v"(acc3[ct]));
    __syncthreads();  // y2 visible
    V12_STAMP(7);
    {
        vec8 b3[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) b3[ct] = ldsB(lane16, ct * 1024);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                acc3[ct] = H::mfma(a3r[s & 7], b3[ct], acc3[ct]);
                if (ct == 0 && s + 7 < 16) a3r[(s + 7) & 7] = gldw(vc, 0);
                if (s + 1 < 16) b3[ct] = ldsB(lane16, ((s + 1) * 4 + ct) * 1024);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (s + 7 < 16) vc = opaque(vc + 4096u);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    V12_STAMP(8);
    // ================= layer 4: 128 -> 1; this wave holds channels [32 w, +32) of all 128 points =================
    float *part = reinterpret_cast<float *>(smem + V12_PART);
    const unsigned c3 = hh * 16u + rt3 * 128u;                     // LDS constants indexed by layer-3 output channel
    {
        // (the weights once, the four column tiles' sums side by side, then the exchanges and the stores: written per column tile the
        //  compiler re-read the weights behind every store and waited for each read)
        f32x4 w4v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) w4v[g] = lds4(c3, W4C + 4 * (8 * g));
        float ps[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            float p = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) p = fmaf(w4v[g][r], lrelu01(acc3[ct][4 * g + r]), p);
            ps[ct] = p;
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) ps[ct] += __shfl_xor(ps[ct], 32);
        if (ol < 32) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) part[rt3 * 128 + ct * 32 + ol] = ps[ct];
        }
    }
    // (the tile's z / p table is read in front of the barrier: wave 0 rewrites it for the next item right behind it)
    const float *sc = reinterpret_cast<const float *>(smem + V12_SC);
    const float a4 = sc[M], w4z = sc[2 + M], w4p = sc[4];
    float y4[4];
    {
        // The two fmas are pinned as scalar instructions.  Left alone hipcc pairs column tiles (0, 1) and (2, 3) into
        // v_pk_fma_f32 .. op_sel:[0,1,0] (both halves multiply by the HIGH register of the (w4z, w4p) pair), and on MI355X the LOW half
        // of that instruction came back without its product in lanes 48 - 63 - only with a second workgroup resident on the CU,
        // a few tiles per thousand, every input register verified afterwards (the hunt: NOTES R5.1).
        float zz[4], pp[4];
        const float *zt_late = reinterpret_cast<const float *>(smem + V12_ZTAB) + (fresh_lane() & 31u);   // (not `zt`: see fresh_lane)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            zz[ct] = zt_late[ct * 32];
            pp[ct] = M ? zt_late[128 + ct * 32] : 0.0f;
        }
#ifndef SURS_ABL_NO_ISA_PINS
        asm volatile("" : "+v"(zz[0]), "+v"(zz[1]), "+v"(zz[2]), "+v"(zz[3]), "+v"(pp[0]), "+v"(pp[1]), "+v"(pp[2]), "+v"(pp[3]));
#endif
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            y4[ct] = fmaf(zz[ct], w4z, a4);
            SURS_ISA_PIN(y4[ct]);
            if (M) y4[ct] = fmaf(pp[ct], w4p, y4[ct]);
            SURS_ISA_PIN(y4[ct]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const unsigned pt = ct * 32 + (fresh_lane() & 31u);
        const float s = ((part[pt] + part[128 + pt]) + part[256 + pt]) + part[384 + pt];
        logit[ct] = y4[ct] + s;
    }
    V12_STAMP(9);
    return true;
}

template <int DT>
__global__ __launch_bounds__(V12_THREADS, 2) void grid_mlp_kernel_v12(GridArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *w4s = reinterpret_cast<float *>(smem + V12_W4C);
    float *scs = reinterpret_cast<float *>(smem + V12_SC);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    w4s[tid] = a.zvec[ZV_W4C_LR + tid];
    if (tid < 3) scs[2 + tid] = a.zvec[ZV_W4Z_LR + tid];   // w4z_lr, w4z_hr, w4p_hr
    const int nzc = (a.rz + 127) / 128;
    const char *w_lr = a.core, *w_hr = a.core + (size_t)SLABS_PER_MLP * SLAB_BYTES;
    const unsigned short *w1t = reinterpret_cast<const unsigned short *>(a.w1t);
    auto zf_of = [&](int k) {
        const double zt = a.dz * (double)k;
        const float zw = (float)(zt + a.z0);
        const float Z = a.c23 + a.c22 * zw;
        return Z * a.zmul / a.zdiv;
    };
#ifdef SURS_V3_TRACE
    if (tid == 0 && blockIdx.x == 0) {
        g_v3_trace[40] = __builtin_amdgcn_s_memtime();
        g_v3_trace[41] = __builtin_amdgcn_s_memrealtime();
    }
    unsigned long long wg_t0 = 0, wg_r0 = 0;
    if (tid == 0 && blockIdx.x == SURS_V12_TRACE_WG) {
        wg_t0 = __builtin_amdgcn_s_memtime();
        wg_r0 = __builtin_amdgcn_s_memrealtime();
    }
    int ncol_done = 0;
#endif
    unsigned ksteps = 0;   // residual k-steps of layer 1 this workgroup ran (both MLPs): the executed-FLOP statistic
    int *colslot = reinterpret_cast<int *>(smem + V12_CNT + 16);
    float *ztab = reinterpret_cast<float *>(smem + V12_ZTAB);
    for (;;) {
        if (tid == 0) *colslot = (int)atomicAdd(a.colctr, 1u);
        __syncthreads();  // everyone is done with the previous column's constants; the next column's index is there
        // (LDS addresses and lane indices of this per-column part are made inside the loop: kept across it they were spilled)
        unsigned slot_off = V12_CNT + 16;
        asm volatile("" : "+s"(slot_off));
        const int col = *reinterpret_cast<const int *>(smem + slot_off);
        if (col >= a.ncols) break;
#ifdef SURS_V3_TRACE
        ++ncol_done;
#endif
        const float *src = a.cc + (size_t)col * CC_PAD;
        {
            const unsigned fl = fresh_lane();
            unsigned sc_off = V12_SC;
            asm volatile("" : "+s"(sc_off));
            if (wave == 0 && fl < 2) reinterpret_cast<float *>(smem + sc_off)[fl] = src[CC_A4_LR + fl];
        }
        const float cmask = a.colmask[col];
        const float *rv_lr = a.rvec_lr + (size_t)col * (2 * D2), *rv_hr = a.rvec_hr + (size_t)col * (3 * D2);
        const int cnt = a.kcount ? __builtin_amdgcn_readfirstlane(a.kcount[col]) : a.rz;
        const unsigned short *kl = a.klist ? a.klist + (size_t)col * a.rz : nullptr;
        // the column's affine A fragments, once for its z tiles and waves (a column without items builds none)
        char *aimg = a.aimg + (size_t)blockIdx.x * V12_AIMG_BYTES;
        if (cnt > 0) {
            const unsigned fl = fresh_lane();
            v12_affine_build<DT>(rv_lr, rv_hr, a.zvec, aimg, wave, fl);
        }
        __syncthreads();   // the column's constants and its fragment image are there
        for (int zc = 0; zc < nzc; ++zc) {
            if (zc * 128 >= cnt) break;
#ifdef SURS_V3_TRACE
            if (tid == 0 && blockIdx.x == 0) g_v3_trace_on = (ncol_done == 1 && zc == 1);
#endif
            float zf[4], l[4];
            const int l31 = (int)(fresh_lane() & 31u);
            int kz[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) kz[ct] = zc * 128 + ct * 32 + l31;
            if (kl) {   // (a branch on the uniform pointer: as a select its condition sat in a vector register for the whole column)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) kz[ct] = (int)kl[kz[ct] < cnt ? kz[ct] : cnt - 1];
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) zf[ct] = zf_of(kz[ct] * a.zstride);
            if (wave == 0) {   // (lanes 32 .. 63 hold the same values: the table's writers are lanes 0 .. 31)
                const unsigned fl = fresh_lane();
                if (fl < 32) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) ztab[ct * 32 + fl] = zf[ct];
                }
            }
            const float ze0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zf[0]), 0));
            const float ze1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zf[3]), 31));
            const float zlo = fminf(ze0, ze1), zhi = fmaxf(ze0, ze1);
            // a tile that lists more channels than the stream stages (either classifier) is handed, whole, to kernel v10's tile
            // mode, which runs behind this launch on the tiles listed here: same bits, and no slow path in this kernel
            unsigned kst = 0;
            bool done = grid_mlp_v12<DT, 0>(w_lr, src, a.zvec, w1t, aimg, a.zmid, zlo, zhi, 0.0f, 0.0f, smem, wave, (int)fresh_lane(), l, kst);
            if (!done) {
                if (tid == 0) {
                    const unsigned t = atomicAdd(a.ovf_count, 1u);
                    a.ovf_list[2 * t] = col;
                    a.ovf_list[2 * t + 1] = zc;
                }
                continue;
            }
            float p_lr[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) p_lr[ct] = cmask * (1.0f / (1.0f + expf(-l[ct])));
            if (wave == 0) {
                const unsigned fl = fresh_lane();
                if (fl < 32) {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) ztab[128 + ct * 32 + fl] = p_lr[ct];
                }
            }
            // the box of p over the tile's 128 voxels (every wave holds the same values: lanes 0..31 x 4)
            float plo = fminf(fminf(p_lr[0], p_lr[1]), fminf(p_lr[2], p_lr[3]));
            float phi = fmaxf(fmaxf(p_lr[0], p_lr[1]), fmaxf(p_lr[2], p_lr[3]));
            {
                auto dpp = [](float v, auto ctrl) {
                    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, false));
                };
                using QP1 = std::integral_constant<int, 0xB1>;    // quad_perm [1,0,3,2]
                using QP2 = std::integral_constant<int, 0x4E>;    // quad_perm [2,3,0,1]
                using RHM = std::integral_constant<int, 0x141>;   // row_half_mirror
                using RM = std::integral_constant<int, 0x140>;    // row_mirror
                plo = fminf(plo, dpp(plo, QP1()));
                phi = fmaxf(phi, dpp(phi, QP1()));
                plo = fminf(plo, dpp(plo, QP2()));
                phi = fmaxf(phi, dpp(phi, QP2()));
                plo = fminf(plo, dpp(plo, RHM()));
                phi = fmaxf(phi, dpp(phi, RHM()));
                plo = fminf(plo, dpp(plo, RM()));
                phi = fmaxf(phi, dpp(phi, RM()));
                const float l0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, plo), 0));
                const float l1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, plo), 16));
                const float h0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, phi), 0));
                const float h1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, phi), 16));
                plo = fminf(l0, l1);
                phi = fmaxf(h0, h1);
            }
            done = grid_mlp_v12<DT, 1>(w_hr, src, a.zvec, w1t + (size_t)D1 * D2, aimg + V12_AIMG_MLP, a.zmid, zlo, zhi, plo, phi, smem, wave, (int)fresh_lane(), l, kst);
            if (!done) {
                if (tid == 0) {
                    const unsigned t = atomicAdd(a.ovf_count, 1u);
                    a.ovf_list[2 * t] = col;
                    a.ovf_list[2 * t + 1] = zc;
                }
                continue;
            }
            ksteps += kst;
#ifdef SURS_V12_DEBUG_KS   // diagnostic builds: vol_lr receives the tile's residual k-steps of both classifiers instead of p_lr
            const float out_dbg = (float)kst;
#endif
            {
                const float lw = wave == 0 ? l[0] : (wave == 1 ? l[1] : (wave == 2 ? l[2] : l[3]));
                const float out_hr = cmask * (1.0f / (1.0f + expf(-lw)));
                const int fl = (int)fresh_lane();   // (not `lane`: the address below would be carried - and spilled - across the item)
                const int k = zc * 128 + wave * 32 + (fl & 31);
                const float out_lr = ztab[128 + wave * 32 + (fl & 31)];   // (the tile's p_lr, still in its table: not carried across the hr pass)
                if (k < a.rz) {
                    float *dst = (fl < 32) ? a.vol_lr : a.vol_hr;
#ifdef SURS_V12_DEBUG_KS
                    dst[(size_t)col * a.rz + k] = (fl < 32) ? out_dbg : out_hr;
#else
                    dst[(size_t)col * a.rz + k] = (fl < 32) ? out_lr : out_hr;
#endif
                }
            }
        }
    }
    if (a.kstat && tid == 0) atomicAdd(a.kstat, (unsigned long long)ksteps);
#ifdef SURS_V3_TRACE
    if (tid == 0 && blockIdx.x == 0) {
        g_v3_trace[42] = __builtin_amdgcn_s_memtime();
        g_v3_trace[43] = __builtin_amdgcn_s_memrealtime();
    }
    if (tid == 0 && blockIdx.x == SURS_V12_TRACE_WG) {   // this workgroup's life in shader cycles and in 100 MHz ticks
        g_v12_acc[0][13] += __builtin_amdgcn_s_memtime() - wg_t0;
        g_v12_acc[0][14] += __builtin_amdgcn_s_memrealtime() - wg_r0;
    }
#endif
}
