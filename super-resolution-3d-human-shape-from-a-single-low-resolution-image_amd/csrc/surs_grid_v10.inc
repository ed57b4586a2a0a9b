// Included by surs_query.hip inside namespace surs, after surs_grid_restated.inc (uses its LDS map and helpers).
//
// Grid column kernel, version 10 (the default reduced-precision sweep): v7's arithmetic (layer 1 restated along the column:
// per-column affine part through one MFMA k-step + the residuals of the listed channels; layers 2-4 dense) on EIGHT waves per
// workgroup instead of four.
//
// Why.  v7 runs one wave per SIMD with all 512 registers.  Its matrix pipe is busy 35 % of the time: between the MFMA loops
// sit serial VALU / LDS phases (classification, residual generation, the two activation publishes, layer 4) that a lone
// wave issues at one vector instruction per 4 cycles - half of what the SIMD can take - and that need an 8-cycle
// v_accvgpr_read per layer-1 output because 256 accumulator registers only fit as AGPRs.  With the dense layer 1 gone the
// tile no longer needs 256 accumulators per wave: eight waves split the output channels twice as fine,
//
//     layer 1 row tiles w, w + 8  2 row tiles x 4 column tiles = 128 accumulator registers
//     layer 2 rows [32w, 32w+32)   1 x 4 = 64
//     layer 3 row tile w >> 1, column tiles 2(w & 1), 2(w & 1) + 1 = 32
//
// every wave fits 256 registers (two waves per SIMD), every accumulator is an ordinary VGPR (no accumulator reads, the
// compiler sees every MFMA hazard: no asm MFMAs, no hand-placed s_nop), the two waves of a SIMD fill each other's issue
// slots in the vector phases.  A weight fragment still feeds four MFMAs in layers 1 and 2 (the L2 -> CU stream is unchanged);
// the activations are read from LDS by eight waves instead of four.
//
// Same tile (128 voxels of a column), same LDS map as v7.  The channel list is built in v7's order (the wave pair 2W, 2W + 1
// covers the 256 channels of v7's wave W), every layer sums in v7's k order and layer 4 forms the same four partial sums, so
// v10 reproduces v7's bits: tools/gpu_v10_check.py (R = 24 ... 512, bf16 and f16) and tests/test_gpu_fullvolume.py.
//
// What did NOT pay (DESIGN.md 4.1d): a software pipeline across items (the next item's classification, list and residual
// fragments in the slots between this item's layer-2 MFMAs, its weight gather under layer 3 / 4) - bit-identical, 147 ms
// against this kernel's 131 ms at 512^3: the two waves of a SIMD run the same slots at the same time, so the inserted vector
// work stalls both MFMA streams instead of hiding under them, and the LDS-DMA in flight forces asm LDS reads (read + wait in
// one statement, or the compiler spills the destination before the data has arrived) that cannot be software-pipelined.
constexpr int V10_THREADS = 512;
constexpr int GRID10_LDS_BYTES = V7_CNT + 48;   // wave counts [8], the column slot
static_assert(GRID10_LDS_BYTES <= 163840, "LDS budget");

template <int DT, int M>
__device__ __forceinline__ void grid_mlp_v10(const char *__restrict__ wbase /* this MLP's 42 slabs */,
                                             const float *__restrict__ gcc /* this column's constants (global) */,
                                             const float *__restrict__ gzv /* z-vectors (global) */,
                                             const unsigned short *__restrict__ w1t /* this MLP's W1t [1024][512] */,
                                             const float *__restrict__ rvec /* this column's and MLP's vectors RA, RB[, RC]: [2 | 3][512] */,
                                             long long rld,
                                             float zmid, float zlo, float zhi, char *smem, int wave, int lane,
                                             const float (&zf)[4], const float (&pin)[4], float (&logit)[4], unsigned &ksteps) {
    typedef HalfT<DT> H;
    typedef typename H::vec8 vec8;
    typedef typename H::elem elem;
    unsigned lz = 0;
    asm volatile("" : "+s"(lz));
    gcc += lz;
    gzv += lz;
    wbase += lz;
    w1t += lz;
    rvec += lz;
    constexpr int A0 = V3_A0 + 4096 * M, W0Z = V3_W0 + 4096 * M, W0P = V3_W0 + 8192, W4C = V3_W4C + 512 * M;
    constexpr int GA2 = M ? CC_A2_HR : CC_A2_LR, GA3 = M ? CC_A3_HR : CC_A3_LR;
    constexpr int GW2Z = M ? ZV_W2Z_HR : ZV_W2Z_LR, GW2P = ZV_W2P_HR,
                  GW3Z = M ? ZV_W3Z_HR : ZV_W3Z_LR, GW3P = ZV_W3P_HR;
    const unsigned h16 = opaque((unsigned)(lane >> 5) * 16u);
    const unsigned lane16 = opaque((unsigned)lane * 16u);
    const unsigned uw = (unsigned)wave;  // wave-uniform
    const int hh = lane >> 5;
    char *ybase = smem + lane16;                                 // B fragments: + (slot*4 + ct) * 1024
    const unsigned hq = (unsigned)(lane >> 5) * 4u;               // channel offset 4h (floats)
    const unsigned rt3 = uw >> 1;                                 // layer-3 row tile of this wave
    const float *gz2 = gzv + (hq + uw * 32u), *gc2 = gcc + (hq + uw * 32u);     // layer-2 output channel 32w + ..
    const float *gz3 = gzv + (hq + rt3 * 32u), *gc3 = gcc + (hq + rt3 * 32u);   // layer-3 output channel 32 (w >> 1) + ..
    char *c3 = smem + (h16 + rt3 * 128u);                        // LDS constants indexed by layer-3 output channel
    auto ld4 = [&](const char *base, int byte_off) { return *reinterpret_cast<const f32x4 *>(base + byte_off); };
    auto gl4 = [&](const float *base, int float_off) { return *reinterpret_cast<const f32x4 *>(base + float_off); };
    auto ldB = [&](int byte_base, int slot, int ct) { return *reinterpret_cast<const vec8 *>(ybase + byte_base + (slot * 4 + ct) * 1024); };
    auto cvt8 = [&](const f32x16 &t, int u) {
        // LeakyReLU = max(x, 0.01 x): one v_mul_f32 and one maximum per value (lrelu01).  Not the products two at a time: beside
        // MFMAs a v_pk_mul_f32 costs more than the two v_mul_f32 it replaces, and its result needs a wait state before the
        // maximum that reads it (measured on kernel v12's slab: NOTES, "Column kernels: one maximum per LeakyReLU")
        vec8 b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = (elem)lrelu01(t[8 * u + j]);
        return b;
    };
    auto ldw = [&](unsigned voff, int imm) { return *reinterpret_cast<const vec8 *>(wbase + (size_t)voff + imm); };

    // ================= layer 1 =================
#ifdef SURS_V3_TRACE
    const bool v7_tr = g_v3_trace_on && blockIdx.x == 0 && wave == 0 && lane == 0;
#endif
    V7_STAMP(0);
    const int tid = wave * 64 + lane;
    unsigned short *list = reinterpret_cast<unsigned short *>(smem + V7_LIST);
    int *cnt = reinterpret_cast<int *>(smem + V7_CNT);
    // the affine part's A fragments of this wave's two row tiles (w, w + 8), built here from the column's vectors R = W1 (g . [a0 |
    // w0z | w0p]) - first, so that the loads' latency passes under the classification.  Lane (r, h) of row tile T holds, for row
    // 32 T + r, the three 16-bit parts a, b, c of (b1 + RA, RB, RC) in the slot order  h = 0: a0 a1 a2 b0 b0 b1 b0 b1,
    // h = 1: b2 c0 c0 c1 c0 c1 c2 0  (the B operand pairs them with 1 1 1 z0 z1 z0 z2 z1 | z0 p0 p1 p0 p2 p1 p0 0: all products
    // of parts down to 2^-24 relative).  (Until round 4 a kernel of its own wrote these fragments, 32 KiB per column, to HBM.)
    vec8 ai[2];
#ifdef SURS_ABL_NO_AFFINE_BUILD   // timing ablation only (wrong results): what does building the fragments in the kernel cost?
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int j = 0; j < 8; ++j) ai[rt][j] = (elem)(float)(lane + rt);
#else
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const int row = 32 * ((int)uw + 8 * rt) + (lane & 31);
        const float *rp = rvec + row;
        const elem zero = (elem)0.0f;
        elem pa[3], pb[3], pc[3] = {zero, zero, zero};
        split3_elem<DT>(rp[0] + gzv[(M ? ZV_B1_HR : ZV_B1_LR) + row], pa);
        split3_elem<DT>(rp[D2], pb);
        if (M) split3_elem<DT>(rp[2 * D2], pc);
        const vec8 flo = {pa[0], pa[1], pa[2], pb[0], pb[0], pb[1], pb[0], pb[1]};
        const vec8 fhi = {pb[2], pc[0], pc[0], pc[1], pc[0], pc[1], pc[2], zero};
        ai[rt] = hh ? fhi : flo;
    }
#endif
    // ---- which channels need their residual over this tile: box of (zf, p) over the tile's 128 voxels
    float plo = 0.0f, phi = 0.0f;
    if (M) {
        // every wave holds the same 128 values: lanes 0..31 x 4 (lanes 32..63 repeat them); rows of 16 lanes through DPP
        plo = fminf(fminf(pin[0], pin[1]), fminf(pin[2], pin[3]));
        phi = fmaxf(fmaxf(pin[0], pin[1]), fmaxf(pin[2], pin[3]));
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
    // thread (wave, lane) classifies channels 256 (w >> 1) + 4 lane + 2 (w & 1) + {0, 1}: the wave pair (2W, 2W + 1) covers the 256
    // channels of v7's wave W, and the list comes out in v7's order (per 256-channel block: the flagged channels = 0 mod 4 in
    // lane order, then 1, 2, 3 mod 4) - chunks and k-steps hold the same channels in the same slots, so layer 1's sums run in
    // the same order and v10 reproduces v7's bits
    const int ch0 = 256 * (wave >> 1) + 4 * lane + 2 * (wave & 1);
    unsigned flags = 0;
    {
        const f32x2 ca = *reinterpret_cast<const f32x2 *>(smem + A0 + ch0 * 4);
        const f32x2 cz = *reinterpret_cast<const f32x2 *>(smem + W0Z + ch0 * 4);
        f32x2 cp = {0.0f, 0.0f};
        if (M) cp = *reinterpret_cast<const f32x2 *>(smem + W0P + ch0 * 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float xm = fmaf(zmid, cz[i], ca[i]);
            if (M) xm = fmaf(0.5f, cp[i], xm);
            const float t0 = cz[i] * zlo, t1 = cz[i] * zhi;
            float mn = ca[i] + fminf(t0, t1), mx = ca[i] + fmaxf(t0, t1);
            if (M) {
                const float u0 = cp[i] * plo, u1 = cp[i] * phi;
                mn += fminf(u0, u1);
                mx += fmaxf(u0, u1);
            }
            const bool constant = (xm > 0.0f) ? (mn > 0.0f) : (mx <= 0.0f);
            flags |= constant ? 0u : (1u << i);
        }
    }
    const unsigned long long b0 = __ballot(flags & 1u), b1 = __ballot(flags & 2u);
    const int n0 = __popcll(b0);
    if (lane == 0) cnt[wave] = n0 + __popcll(b1);
    V7_STAMP(10);
    __syncthreads();   // wave counts
    int base = 0, E = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = cnt[i];
        base += (i < wave) ? c : 0;
        E += c;
    }
    E = __builtin_amdgcn_readfirstlane(E);
    ksteps += (unsigned)(E + 15) >> 4;
    {
        const unsigned long long lt = (1ull << lane) - 1ull;
        if (flags & 1u) list[base + __popcll(b0 & lt)] = (unsigned short)ch0;
        if (flags & 2u) list[base + n0 + __popcll(b1 & lt)] = (unsigned short)(ch0 + 1);
        if (tid < V7_CH) list[E + tid] = 0;   // padding up to the chunk size: channel 0's weights, zero residual
    }
    __syncthreads();   // list
    V7_STAMP(1);
#ifdef SURS_V3_TRACE
    if (v7_tr) g_v3_trace[48 + M] = (unsigned long long)E;
#endif
    f32x16 acc1[2][4];
    {
        typedef __attribute__((address_space(3))) char lds_char;
        const unsigned lds0 = (unsigned)(size_t)(lds_char *)smem;
        // transposed A-fragment reads (ds_read_b64_tr_b16), as in v7; this wave's rows of W1 are columns [64w, 64w + 64) of the
        // gathered channel rows: row tile w + 8 rt = columns [32 (w + 8 rt), + 32): + 64 w bytes, + rt * 512 B
        const unsigned tr_off = (unsigned)((8 * (lane >> 5) + ((lane & 15) >> 2)) * V7_STRIDE + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2) + 64u * uw;
        char *trb0 = smem + opaque(V7_A + tr_off), *trb1 = smem + opaque(V7_A + 48 * V7_STRIDE + tr_off);
        auto ldA = [&](int s, int rt) {
            typedef short v4s __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) v4s lds_v4s;
            const char *b = (s < 3 ? trb0 : trb1) + ((s % 3) * 16 * V7_STRIDE + rt * 512);
            const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)b);
            const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s *)(b + 4 * V7_STRIDE));
            typedef short v8s __attribute__((ext_vector_type(8)));
            const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            return __builtin_bit_cast(vec8, r);
        };
        char *bbase = smem + opaque(V7_B + (unsigned)lane * 16u);     // B fragments: + (s * 4 + ct) * 1024
        // residual generation: this wave column tile w & 3 of the k-steps (w >> 2), + 2, + 4
        const unsigned ctw = uw & 3u;
        const float zf_own = ctw == 0 ? zf[0] : (ctw == 1 ? zf[1] : (ctw == 2 ? zf[2] : zf[3]));
        const float p_own = ctw == 0 ? pin[0] : (ctw == 1 ? pin[1] : (ctw == 2 ? pin[2] : pin[3]));
        const unsigned bst = lds0 + (unsigned)V7_B + (unsigned)lane * 16u + 1024u * ctw;   // own B fragments: + s * 4096
        const int nch = E > 0 ? (E + V7_CH - 1) / V7_CH : 1;   // (an empty list still runs the affine k-step)
#pragma unroll 1
        for (int q = 0; q < nch; ++q) {
            const int rem = E - V7_CH * q;
            const int ks = rem >= V7_CH ? V7_KS : ((rem + 15) >> 4);   // k-steps of this chunk
            // ---- the list entries this wave needs: rows 16 s + 2 w, + 1 of the gather, channels 16 s' + 8 h .. + 7 of its
            //      residual units (ordinary LDS reads: they must precede the LDS-DMA, see v7)
            const unsigned short *lq = list + V7_CH * q;
            unsigned gid[V7_KS];
            u32x4 rid[3];
#pragma unroll
            for (int s = 0; s < V7_KS; ++s) gid[s] = *reinterpret_cast<const unsigned *>(lq + 16 * s + 2 * wave);
#pragma unroll
            for (int i = 0; i < 3; ++i) rid[i] = *reinterpret_cast<const u32x4 *>(lq + 16 * ((wave >> 2) + 2 * i) + 8 * hh);
            auto gather = [&](int s) {
                if (s < ks) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const unsigned cid = (gid[s] >> (16 * k)) & 0xffffu;
                        const char *src = reinterpret_cast<const char *>(w1t) + (size_t)(cid * 1024u + lane16);
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                         (__attribute__((address_space(3))) void *)(smem + V7_A + (16 * s + 2 * wave + k) * V7_STRIDE), 16, 0, 0);
                    }
                }
            };
            auto residuals = [&](int i) {
                const int s = (wave >> 2) + 2 * i;
                if (s < ks) {
                    const int e0 = V7_CH * q + 16 * s + 8 * hh;
                    float ca[8], cz[8], cp[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned ad = lds0 + (unsigned)A0 + 4u * ((rid[i][j >> 1] >> (16 * (j & 1))) & 0xffffu);
                        asm volatile("ds_read_b32 %0, %1" : "=v"(ca[j]) : "v"(ad));
                        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(cz[j]) : "v"(ad), "n"(W0Z - A0));
                        if (M) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(cp[j]) : "v"(ad), "n"(W0P - A0));
                        else cp[j] = 0.0f;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(ca[0]), "+v"(ca[1]), "+v"(ca[2]), "+v"(ca[3]), "+v"(ca[4]), "+v"(ca[5]), "+v"(ca[6]), "+v"(ca[7]),
                                   "+v"(cz[0]), "+v"(cz[1]), "+v"(cz[2]), "+v"(cz[3]), "+v"(cz[4]), "+v"(cz[5]), "+v"(cz[6]), "+v"(cz[7]),
                                   "+v"(cp[0]), "+v"(cp[1]), "+v"(cp[2]), "+v"(cp[3]), "+v"(cp[4]), "+v"(cp[5]), "+v"(cp[6]), "+v"(cp[7]));
                    vec8 bf;
                    constexpr float K99 = 1.0f - 0.01f, INF = __builtin_inff();
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float xm = fmaf(zmid, cz[j], ca[j]);
                        if (M) xm = fmaf(0.5f, cp[j], xm);
                        const bool g1 = xm > 0.0f;
                        const float lo = g1 ? -INF : 0.0f, hi = g1 ? 0.0f : INF;
                        const float c = (e0 + j < E) ? (g1 ? -K99 : K99) : 0.0f;
                        float x = fmaf(zf_own, cz[j], ca[j]);
                        if (M) x = fmaf(p_own, cp[j], x);
                        // (the product rounded to fp32, THEN converted: left alone hipcc folds some of these products - one element in
                        //  eight of the f16 instance - into v_fma_mixlo_f16, a single rounding of the exact product, and the kernel's
                        //  bits depend on which; kernel v12 forms the same value another way and is held to this one bit for bit)
                        float r = c * __builtin_amdgcn_fmed3f(x, lo, hi);
                        SURS_ISA_PIN(r);
                        bf[j] = (elem)r;
                    }
                    const unsigned ad = bst + (unsigned)s * 4096u;
                    asm volatile("ds_write_b128 %0, %1" : : "v"(ad), "v"(bf) : "memory");
                }
            };
            gather(0);
            gather(1);
            gather(2);
            __builtin_amdgcn_sched_barrier(0);
            if (q == 0) {
                // ---- the affine part through the matrix pipe (see v7): one k-step of the three 16-bit parts of (b1 + RA, RB, RC)
                //      against those of (1, zf, p)
                vec8 bi[4];
                const elem zero = (elem)0.0f, one = (elem)1.0f;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    elem z[3], p[3] = {zero, zero, zero};
                    split3_elem<DT>(zf[ct], z);
                    if (M) split3_elem<DT>(pin[ct], p);
                    const vec8 lo = {one, one, one, z[0], z[1], z[0], z[2], z[1]};
                    const vec8 hi = {z[0], p[0], p[1], p[0], p[2], p[1], p[0], zero};
                    bi[ct] = hh ? hi : lo;
                }
                f32x16 z;
#pragma unroll
                for (int j = 0; j < 16; ++j) z[j] = 0.0f;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc1[rt][ct] = H::mfma(ai[rt], bi[ct], z);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (q == 0) V7_STAMP(11);
            residuals(0);
            __builtin_amdgcn_sched_barrier(0);
            gather(3);
            gather(4);
            gather(5);
            __builtin_amdgcn_sched_barrier(0);
            residuals(1);
            __builtin_amdgcn_sched_barrier(0);
            residuals(2);
            __builtin_amdgcn_sched_barrier(0);
            if (q == 0) V7_STAMP(12);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __syncthreads();
            if (q == 0) V7_STAMP(13);
#pragma unroll
            for (int s = 0; s < V7_KS; ++s)
                if (s < ks) {
                    vec8 a[2], b[4];
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) a[rt] = ldA(s, rt);
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) b[ct] = *reinterpret_cast<const vec8 *>(bbase + (s * 4 + ct) * 1024);
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) acc1[rt][ct] = H::mfma(a[rt], b[ct], acc1[rt][ct]);
                }
            __syncthreads();
            if (q == 0) V7_STAMP(14);
        }
    }
    vec8 bc[4];
    // ---- publish y1.  Wave w holds layer-1 row tiles w (acc1[0]) and w + 8 (acc1[1]) = layer-2 k-steps 2w, 2w + 1 and 2w + 16,
    //      2w + 17: the first 16 k-steps of layer 2 only need every wave's tile 0, so only that half is converted in front of
    //      layer 2; tile 1 is converted in the slots between the MFMAs of k-steps 0 - 7 and becomes visible at a barrier in
    //      front of k-step 16.  Layer 2 still sums k-steps 0 .. 31 in order.
    //      (the loop's last barrier already retired the staging buffers that this overwrites)
    V7_STAMP(2);
    // layer 2's first weight fragments and accumulator-initialisation constants: issued here so that their L2 latency
    // passes under the conversion
    vec8 a2r[4];  // layer-2 weight ring: [k-step & 3], 3 k-steps ahead
    unsigned vb = opaque(lane16 + (unsigned)(V3_F_L2 * 1024) + 1024u * uw);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        a2r[q] = ldw(vb, 0);
        vb = opaque(vb + 8192u);
    }
    f32x4 c2v[4], wz2v[4], wp2v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        c2v[g] = gl4(gc2, GA2 + 8 * g);
        wz2v[g] = gl4(gz2, GW2Z + 8 * g);
        if (M) wp2v[g] = gl4(gz2, GW2P + 8 * g);
    }
    __builtin_amdgcn_sched_barrier(0);
    char *yw = smem + (lane16 + uw * 8192u);  // slots 2w, 2w + 1 (tile 0); + 65536: slots 2w + 16, 2w + 17 (tile 1)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<vec8 *>(yw + V3_Y + (u * 4 + ct) * 1024) = cvt8(acc1[0][ct], u);
    V7_STAMP(3);
    // ================= layer 2: rows [32w, 32w+32), K = 512 (32 k-steps) =================
    f32x16 acc2[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t = fmaf(zf[ct], wz2v[g][r], c2v[g][r]);
                if (M) t = fmaf(pin[ct], wp2v[g][r], t);
                acc2[ct][4 * g + r] = t;
            }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) asm volatile("" : "+v"(acc2[ct]));   // computed here, not in the loop's first slots
    __syncthreads();  // tile 0 of every wave (k-steps 0 .. 15) visible
    V7_STAMP(4);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bc[ct] = ldB(V3_Y, 0, ct);
    // 4 MFMAs per k-step; fillers: the weight load of k-step s + 3 in slot 0, each B fragment re-loaded in place (next
    // k-step) right after its MFMA - except across the barrier in front of k-step 16 - and, in k-steps 0 .. 7, one of the
    // eight fragments of tile 1 converted and stored
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        if (s == 16) {
            __syncthreads();   // tile 1 of every wave (k-steps 16 .. 31) visible
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bc[ct] = ldB(V3_Y, 16, ct);
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            acc2[ct] = H::mfma(a2r[s & 3], bc[ct], acc2[ct]);
            if (ct == 0 && s + 3 < 32) a2r[(s + 3) & 3] = ldw(vb, 0);
            if (s + 1 < 32 && s + 1 != 16) bc[ct] = ldB(V3_Y, s + 1, ct);
            if (s < 8 && ct == 1) {
                const int f = s;   // fragment (u = f >> 2, column tile f & 3) of tile 1
                *reinterpret_cast<vec8 *>(yw + V3_Y + 65536 + f * 1024) = cvt8(acc1[1][f & 3], f >> 2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (s + 3 < 32) vb = opaque(vb + 8192u);
        __builtin_amdgcn_sched_barrier(0);
    }
    V7_STAMP(5);
    // ---- publish y2 (into the Y region: every wave must be done reading y1 first); layer 3's first loads before it
    vec8 a3r[8];
    unsigned vc = opaque(lane16 + (unsigned)(V3_F_L3 * 1024) + 1024u * rt3);
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        a3r[q] = ldw(vc, 0);
        vc = opaque(vc + 4096u);
    }
    f32x4 c3v[4], wz3v[4], wp3v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        c3v[g] = gl4(gc3, GA3 + 8 * g);
        wz3v[g] = gl4(gz3, GW3Z + 8 * g);
        if (M) wp3v[g] = gl4(gz3, GW3P + 8 * g);
    }
    __syncthreads();
    {
        char *yw = smem + (lane16 + uw * 8192u);  // slots 2w, 2w+1
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<vec8 *>(yw + V3_Y + (u * 4 + ct) * 1024) = cvt8(acc2[ct], u);
    }
    V7_STAMP(6);
    // ================= layer 3: row tile w >> 1, column tiles 2(w & 1) + {0, 1}, K = 256 (16 k-steps) =================
    const unsigned ct0 = 2u * (uw & 1u);
    const float zf3[2] = {ct0 ? zf[2] : zf[0], ct0 ? zf[3] : zf[1]};
    const float pin3[2] = {ct0 ? pin[2] : pin[0], ct0 ? pin[3] : pin[1]};
    f32x16 acc3[2];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = fmaf(zf3[t], wz3v[g][r], c3v[g][r]);
                if (M) v = fmaf(pin3[t], wp3v[g][r], v);
                acc3[t][4 * g + r] = v;
            }
#pragma unroll
    for (int t = 0; t < 2; ++t) asm volatile("" : "+v"(acc3[t]));
    __syncthreads();  // y2 visible
    V7_STAMP(7);
    char *yb3 = ybase + opaque(ct0 * 1024u);
    auto ldB3 = [&](int slot, int t) { return *reinterpret_cast<const vec8 *>(yb3 + V3_Y + (slot * 4 + t) * 1024); };
    vec8 b3[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) b3[0][t] = ldB3(0, t);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            acc3[t] = H::mfma(a3r[s & 7], b3[s & 1][t], acc3[t]);
            if (t == 0 && s + 7 < 16) a3r[(s + 7) & 7] = ldw(vc, 0);
            if (s + 1 < 16) b3[(s + 1) & 1][t] = ldB3(s + 1, t);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (s + 7 < 16) vc = opaque(vc + 4096u);
        __builtin_amdgcn_sched_barrier(0);
    }
    V7_STAMP(8);
    // ================= layer 4: 128 -> 1; this wave holds channels [32 rt3, +32) of its 64 points =================
    float *part = reinterpret_cast<float *>(smem + V3_PART);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float p = 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 w = ld4(c3, W4C + 4 * (8 * g));
#pragma unroll
            for (int r = 0; r < 4; ++r) p = fmaf(w[r], lrelu01(acc3[t][4 * g + r]), p);
        }
        p += __shfl_xor(p, 32);
        if (lane < 32) part[rt3 * 128 + (ct0 + t) * 32 + lane] = p;
    }
    __syncthreads();
    const float *sc = reinterpret_cast<const float *>(smem + V3_SC);
    const float a4 = sc[M], w4z = sc[2 + M], w4p = sc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int pt = ct * 32 + (lane & 31);
        const float s = ((part[pt] + part[128 + pt]) + part[256 + pt]) + part[384 + pt];
        float y4 = fmaf(zf[ct], w4z, a4);
        if (M) y4 = fmaf(pin[ct], w4p, y4);
        logit[ct] = y4 + s;
    }
    V7_STAMP(9);
}

template <int DT>
__global__ __launch_bounds__(V10_THREADS, 2) void grid_mlp_kernel_v10(GridArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *a0s = reinterpret_cast<float *>(smem + V3_A0);
    float *w0s = reinterpret_cast<float *>(smem + V3_W0);
    float *w4s = reinterpret_cast<float *>(smem + V3_W4C);
    float *scs = reinterpret_cast<float *>(smem + V3_SC);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (tile mode behind kernel v12 on a field whose tiles all fit v12's stream - the usual case -: nothing listed, nothing to set up.
    //  The launch is sized by the host, which cannot know: 48 us per batch with the set-up, measured in round 6)
    if (a.tile_list && *a.tile_count == 0) return;
    for (int i = tid; i < 3072; i += V10_THREADS) w0s[i] = a.zvec[ZV_W0Z_LR + i];
    if (tid < 256) w4s[tid] = a.zvec[ZV_W4C_LR + tid];
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
#endif
    unsigned ksteps = 0;   // residual k-steps of layer 1 this workgroup ran (both MLPs): the executed-FLOP statistic
    int *colslot = reinterpret_cast<int *>(smem + V7_CNT + 32);
#ifdef SURS_V3_TRACE
    int ncol_done = 0;
#endif
    for (;;) {
        if (tid == 0) *colslot = (int)atomicAdd(a.colctr, 1u);
        __syncthreads();  // everyone is done with the previous column's constants; the next column's index is there
        int col = *colslot;
        // tile mode (behind kernel v12): the work items are the (column, z tile) pairs v12 left in tile_list
        int zc_lo = 0, zc_hi = nzc;
        if (a.tile_list) {
            if ((unsigned)col >= *a.tile_count) break;
            zc_lo = a.tile_list[2 * col + 1];
            zc_hi = zc_lo + 1;
            col = a.tile_list[2 * col];
        } else if (col >= a.ncols) break;
#ifdef SURS_V3_TRACE
        ++ncol_done;
#endif
        const float *src = a.cc + (size_t)col * CC_PAD;
        for (int i = tid; i < 2048; i += V10_THREADS) a0s[i] = src[i];
        if (tid < 2) scs[tid] = src[CC_A4_LR + tid];
        const float cmask = a.colmask[col];
        const float *rv_lr = a.rvec_lr + (size_t)col * (2 * D2), *rv_hr = a.rvec_hr + (size_t)col * (3 * D2);
        // lattice sweeps: the column's items are its listed lattice points (ascending k), cnt of them, in tiles of 128; an item beyond
        // cnt repeats the last one (its result is dropped), so that a tile's z range stays that of its real items
        const int cnt = a.kcount ? __builtin_amdgcn_readfirstlane(a.kcount[col]) : a.rz;
        const unsigned short *kl = a.klist ? a.klist + (size_t)col * a.rz : nullptr;
        // point runs: the column's items are cnt consecutive points of the caller's array, from point cbase on
        const size_t cbase = a.colstart ? (size_t)a.colstart[col] : (size_t)col * a.rz;
        const int klim = a.colstart ? cnt : a.rz;
        __syncthreads();
        for (int zc = zc_lo; zc < zc_hi; ++zc) {
            if (zc * 128 >= cnt) break;
#ifdef SURS_V3_TRACE
            if (tid == 0 && blockIdx.x == 0) g_v3_trace_on = (ncol_done == 1 && zc == 1);
#endif
            float zf[4], p0[4], p_lr[4], p_hr[4], l[4];
            const int l31 = (int)(fresh_lane() & 31u);   // (made per item: see fresh_lane)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int e = zc * 128 + ct * 32 + l31;
                if (a.zpts) {
                    const float Z = a.c23 + a.c22 * a.zpts[cbase + (e < cnt ? e : cnt - 1)];
                    zf[ct] = Z * a.zmul / a.zdiv;
                } else
                    zf[ct] = zf_of((kl ? (int)kl[e < cnt ? e : cnt - 1] : e) * a.zstride);
                p0[ct] = 0.0f;
            }
            // the tile's first and last voxel: lane 0 of column tile 0, lane 31 of column tile 3
            const float ze0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zf[0]), 0));
            const float ze1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zf[3]), 31));
            const float zlo = fminf(ze0, ze1), zhi = fmaxf(ze0, ze1);
            grid_mlp_v10<DT, 0>(w_lr, src, a.zvec, w1t, rv_lr, a.rld_lr, a.zmid, zlo, zhi, smem, wave, (int)fresh_lane(), zf, p0, l, ksteps);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) p_lr[ct] = cmask * (1.0f / (1.0f + expf(-l[ct])));
            grid_mlp_v10<DT, 1>(w_hr, src, a.zvec, w1t + (size_t)D1 * D2, rv_hr, a.rld_hr, a.zmid, zlo, zhi, smem, wave, (int)fresh_lane(), zf, p_lr, l, ksteps);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) p_hr[ct] = cmask * (1.0f / (1.0f + expf(-l[ct])));
            if (wave < 4) {
                const float out_lr = wave == 0 ? p_lr[0] : (wave == 1 ? p_lr[1] : (wave == 2 ? p_lr[2] : p_lr[3]));
                const float out_hr = wave == 0 ? p_hr[0] : (wave == 1 ? p_hr[1] : (wave == 2 ? p_hr[2] : p_hr[3]));
                const int fl = (int)fresh_lane();   // (not `lane`: see fresh_lane)
                const int k = zc * 128 + wave * 32 + (fl & 31);
                if (k < klim) {
                    float *dst = (fl < 32) ? a.vol_lr : a.vol_hr;
                    dst[cbase + k] = (fl < 32) ? out_lr : out_hr;
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
#endif
}
