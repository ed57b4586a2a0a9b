// Fused point evaluator for SurfaceClassifier pairs of any supported shape (surs_mlp_generic.h), included at the end of
// surs_query.hip.  ONE launch per call: per tile of P points, projection -> in-image mask -> z_feat -> 4-tap bilinear gather of the
// D lr + 64 hr channels (the __device__ helpers gather_kernel uses; D = --hg_dim = dims_lr[0] - 65, 256 in the released model) ->
// mlp_lr -> masked sigmoid (= the last channel, D + 65, of the hr input) -> mlp_hr -> masked sigmoid.  Replaces lib/model/SuRSNet.py:131-187 and lib/model/SurfaceClassifier.py:53-81 for those shapes.
//
// Budget (gfx950: 160 KiB LDS per CU, 512 VGPR+AGPR per SIMD lane):
//   - The activations of a tile never leave the CU.  LDS holds the tile's input features fp32 [P][pad32(D + 66) + 4] (D = 256:
//     [P][352 + 4], the numbers of this paragraph; gen_max_hidden and fused_pb carry D) and ONE activation
//     buffer fp32 [P][max_hidden + 4]: a layer's outputs stay in the accumulators until every wave has finished reading its inputs
//     (barrier), then overwrite them.  So the widest padded hidden layer W, not (input + output), sets the tile:
//     P (W + 364) * 4 bytes <= 160 KiB  ->  P = 32 for W <= 896 (the 512-wide family: 112 128 B), P = 16 up to W = 2048 (154 368 B;
//     the released 1024-wide shape: 88 832 B, still one workgroup per CU).  fp32 activations, not pre-split parts: the same 4 bytes
//     as two f16 parts, 2/3 of three bf16 parts, and one layout for every operand split - each wave splits its B fragment once per
//     k step (8 values) and reuses it across its row tiles.
//   - 8 waves, one workgroup per CU.  Wave w owns output row tiles w, w + 8, ... (16 rows each, v_mfma_f32_16x16x32): at most
//     16 / PB tiles x PB point blocks = 64 accumulator registers per lane, whatever the width.
//   - Weights are read straight from L2 / MALL in A-fragment order (one contiguous 1 KiB wave load per tile, k step and part);
//     every weight is read once per tile of P points, so weight streaming (bytes of the blob's NP-part image / P per point) is
//     the limiter of this kernel, and P is what the LDS budget caps.
//   - Feature row stride pad32(D + 66) + 4 floats: 36 (D = 256, 356) or 4 modulo 64 words, depending on D.  Checked against the B
//     fragment's read (lane (q, c) reads 32 bytes at row c, word 8 q, as two ds_read_b128; MI355X: four groups of 16 lanes per
//     instruction, bank = word mod 64): each group holds 8 lanes of one q and 8 of the next, rows {0-3, 12-15} against {4-11}, and for
//     every 16-byte-aligned stride one pair of those rows lands 8 words apart - one extra LDS cycle per group for residue 36 and
//     for residue 4 alike, as for every pad that is a multiple of 4 (residues 0 and 32: 7 and 3).  No aligned stride is free of it,
//     both residues cost the same, so the pad stays 4 for every D; the released D's stride is the 356 it was.
//   - D is a launch argument (FeatDims): the gather runs a wave per point with its lanes along the point's D + 64 channels, so a tap
//     stays one contiguous read of 4 D bytes and nothing divides by a run-time count.
// Arithmetic: NP = 1 (one f16 product per MAC: --precision bf16 / fp16), 2 (two f16 parts, three products: fp32-grade, |x| <
// 65504) or 3 (three bf16 parts, six products: fp32-grade with fp32's range), products in gemm_x3g_kernel's order.  A point's
// sums run in one fixed order whatever tile or position it lands in (an MFMA output column depends on its own column only).
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage; tests/test_mlp_shapes_host.py reads it from the code object): 124-148
// VGPRs, 0 AGPRs, 0 bytes of scratch over the six <NP, PB> instantiations of each family (mlp_fused_kernel: D = 256, mlp_anyd_kernel:
// any other D; tests/test_hg_dim_host.py), LDS dynamic (above).
// Measured (MI355X, 50 000 random points, full-size feature maps, tools/gpu_shapes_time.py): the released shape 5.28 ms fp32-grade /
// 3.00 ms one product here against 1.00 / 0.56 ms on the layer kernels - P = 16 makes every tile stream the 9.6 MB two-part image
// (600 KB of L2 / MALL reads per point) from one 8-wave workgroup per CU; the 512-wide s1 (P = 32) 1.43 / 0.78 ms.

namespace surs {

constexpr int FU_WAVES = 8;

struct FusedArgs {
    PointSource src;
    long long n;
    const float *feat_lr;
    const float *feat_hr;
    int hl, wl, hh, wh;
    const char *blob;
    const float *p_lr;   // non-null: the hr classifier alone, channel 321 from here
    float *pred_hr, *pred_lr, *logit_hr, *logit_lr;
    int as;              // activation row stride (floats): max_hidden + 4
    int fs;              // feature row stride (floats): gen_feat_stride(D), D = lay.hg_dim
    GenLayout lay;
};

// The feature geometry of a launch: D lr channels, D + 64 gathered channels (z_feat behind them, then p_lr), the row stride.  FIXED:
// the released D = 256 as compile-time constants - mlp_fused_kernel / mlp_fused_views_kernel, instruction for instruction what they
// were when 256 was the only D; otherwise launch arguments - mlp_anyd_kernel / mlp_anyd_views_kernel, the same bodies.  (Run-time
// values in the one family, and a uniform branch between the two forms inside each instantiation, both measured 1 - 3 % slower on
// the released D's 512-wide shape: DESIGN.md section 10.)
constexpr int FU_FS_256 = 356;
template <bool FIXED> struct FeatDims {
    int c_lr, c_g, fs;
    __device__ __forceinline__ explicit FeatDims(const FusedArgs &a)
        : c_lr(FIXED ? C_LR : a.lay.hg_dim), c_g(FIXED ? C_G : a.lay.hg_dim + GEN_C_HR), fs(FIXED ? FU_FS_256 : a.fs) {}
};

// One gathered channel c of tile point p: the 4-tap bilinear sample of the lr (c < c_lr) or hr map at the point's projection.
// (the map sizes by value: selecting between fields of the kernel argument through a reference made hipcc fetch them per item)
__device__ __forceinline__ float gather_channel(const float *fl, const float *fh, int hl, int wl, int hh, int wh, int c_lr, float X, float Y,
                                                int c) {
    const bool hr = c >= c_lr;
    const float *fm = hr ? fh : fl;
    const int H = hr ? hh : hl, W = hr ? wh : wl, C = hr ? C_HR : c_lr, ch = hr ? c - c_lr : c;
    long long pix[4];
    float w[4], tv[4];
    bilinear_taps(X, Y, H, W, pix, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) tv[q] = fm[pix[q] * C + ch];
    return tap_sum(tv, w);
}

template <int NP> struct Mfma16;
template <> struct Mfma16<1> {
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16<2> : Mfma16<1> {};
template <> struct Mfma16<3> {
    typedef bf16x8_t vec8;
    static __device__ __forceinline__ f32x4 mfma(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// Layers l0 .. l1-1 of classifier m on the tile (LeakyReLU(0.01) between them), the last layer's row 0 into slog[P].  VIEWS
// (surs_mlp_fused_views.inc): layer mv's outputs - after its LeakyReLU unless it is the last layer - are not stored but added to
// vsum, the caller's running sum over the views (first: the first view, assigned); each wave owns the same output tiles for every
// view, so the sum stays in registers.
template <int NP, int PB, bool VIEWS>
__device__ __forceinline__ void fused_layers(const FusedArgs &a, const int fs, int m, int l0, int l1, float *feat, float *act, float *slog,
                                             int lane, int wave, f32x4 (&vsum)[16 / PB][PB], int mv, bool first) {
    typedef Mfma16<NP> MF;
    typedef typename MF::vec8 vec8;
    constexpr int TPW = 16 / PB;
    const int L = a.lay.n_layers[m];
    for (int l = l0; l < l1; ++l) {
        const GenLayer &g = a.lay.layer[m][l];
        const int mt = g.mpad / GEN_MT, k1t = g.k1pad / GEN_KT, kts = k1t + g.k2pad / GEN_KT;
        const unsigned short *wimg = (const unsigned short *)(a.blob + (NP == 1 ? g.w1 : (NP == 2 ? g.w2 : g.w3)));
        const size_t per_part = (size_t)kts * mt * 512;
        f32x4 acc[TPW][PB];
#pragma unroll
        for (int i = 0; i < TPW; ++i)
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) acc[i][pb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int kt = 0; kt < kts; ++kt) {
            // B fragment: lane (q, c) holds k = 8 q + j of point c of each 16-point block (layer 0 and the skip segment read the features)
            const bool first = kt < k1t;
            const float *src = first ? (l == 0 ? feat : act) + kt * GEN_KT : feat + (kt - k1t) * GEN_KT;
            const int ld = (first && l > 0) ? a.as : fs;
            vec8 b[PB][NP];
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                const float *x = src + (pb * 16 + (lane & 15)) * ld + 8 * (lane >> 4);
                const f32x4 x0 = *reinterpret_cast<const f32x4 *>(x), x1 = *reinterpret_cast<const f32x4 *>(x + 4);
                u16x8_t bits[NP];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    unsigned short parts[NP];
                    SplitKind<NP>::split(j < 4 ? x0[j] : x1[j - 4], parts);
#pragma unroll
                    for (int p = 0; p < NP; ++p) bits[p][j] = parts[p];
                }
#pragma unroll
                for (int p = 0; p < NP; ++p) b[pb][p] = __builtin_bit_cast(vec8, bits[p]);
            }
            const unsigned short *wk = wimg + (size_t)kt * mt * 512 + lane * 8;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int tile = wave + FU_WAVES * i;
                if (tile < mt) {
                    vec8 w[NP];
#pragma unroll
                    for (int p = 0; p < NP; ++p) w[p] = *reinterpret_cast<const vec8 *>(wk + (size_t)tile * 512 + p * per_part);
#pragma unroll
                    for (int pb = 0; pb < PB; ++pb) {
                        // gemm_x3g_kernel's order: (weight part NP-1-t, point part t), then (1,0) (0,1) for three parts, then (0,0)
#pragma unroll
                        for (int t = 0; t < NP; ++t) acc[i][pb] = MF::mfma(w[NP - 1 - t], b[pb][t], acc[i][pb]);
                        if (NP == 3) {
                            acc[i][pb] = MF::mfma(w[1], b[pb][0], acc[i][pb]);
                            acc[i][pb] = MF::mfma(w[0], b[pb][1], acc[i][pb]);
                        }
                        if (NP >= 2) acc[i][pb] = MF::mfma(w[0], b[pb][0], acc[i][pb]);
                    }
                }
            }
        }
        __syncthreads();   // every wave has read this layer's inputs: the outputs may overwrite them
        const float *bias = (const float *)(a.blob + g.bias);
        const bool last = l == L - 1;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int tile = wave + FU_WAVES * i;
            if (tile < mt) {
                const int row0 = tile * GEN_MT + 4 * (lane >> 4);   // C/D: point = lane & 15, rows row0 .. row0 + 3
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    const int pt = pb * 16 + (lane & 15);
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float y = acc[i][pb][r] + bias[row0 + r];
                        v[r] = (last || y >= 0.0f) ? y : y * 0.01f;
                    }
                    if (VIEWS && l == mv) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) vsum[i][pb][r] = first ? v[r] : vsum[i][pb][r] + v[r];
                    } else if (!last) *reinterpret_cast<f32x4 *>(act + pt * a.as + row0) = v;
                    else if (row0 == 0) slog[pt] = v[0];
                }
            }
        }
        __syncthreads();
    }
}

// One classifier on the tile: layers 0 .. L-1.
template <int NP, int PB>
__device__ __forceinline__ void fused_classifier(const FusedArgs &a, const int fs, int m, float *feat, float *act, float *slog, int lane,
                                                 int wave) {
    f32x4 unused[16 / PB][PB];
    fused_layers<NP, PB, false>(a, fs, m, 0, a.lay.n_layers[m], feat, act, slog, lane, wave, unused, -1, false);
}

// IO: where the lr feature map, the given lr occupancies and the outputs of THIS workgroup are - the launch argument itself, or the
// stack's FusedIo of surs_mlp_fused_stacks.inc; LR_ONLY (that file's lr-only form): the tile ends after mlp_lr.
template <int NP, int PB, bool FIXED, bool LR_ONLY = false, class IO = FusedArgs>
__device__ __forceinline__ void mlp_fused_body(const FusedArgs &a, float *fu_smem, const IO &io) {
    constexpr int P = 16 * PB;
    const FeatDims<FIXED> fd(a);
    const int c_lr = fd.c_lr, c_g = fd.c_g, fs = fd.fs;
    float *feat = fu_smem;                 // [P][fs]: D lr, 64 hr, z_feat, p_lr, zeros
    float *act = feat + P * fs;            // [P][as]
    float *sx = act + P * a.as, *sy = sx + P, *smask = sy + P, *slog = smask + P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long t0 = (long long)blockIdx.x * P;
    if (tid < P) {
        const long long t = t0 + tid;
        float X = 2.0f, Y = 2.0f, in = 0.0f, zf = 0.0f, pl = 0.0f;   // (past n: outside the image, every tap weighted zero)
        if (t < a.n) {
            float px, py, pz, Z;
            make_point(a.src, t, px, py, pz);
            project_point(a.src, px, py, pz, X, Y, Z);
            in = in_image(X, Y);
            zf = Z * a.src.zmul / a.src.zdiv;
            if (io.p_lr) pl = io.p_lr[t];
        }
        sx[tid] = X;
        sy[tid] = Y;
        smask[tid] = in;
        float *f = feat + tid * fs;
        f[c_g] = zf;
        f[c_g + 1] = pl;
        for (int c = c_g + 2; c < fs; ++c) f[c] = 0.0f;
    }
    __syncthreads();
    // gather: lanes along the channels of one point (a tap is one contiguous read: 1 KiB / 256 B for D = 256)
    if (FIXED) {
        for (int item = tid; item < P * c_g; item += FU_WAVES * 64) {
            const int p = item / c_g, c = item - p * c_g;
            feat[p * fs + c] = gather_channel(io.feat_lr, a.feat_hr, a.hl, a.wl, a.hh, a.wh, c_lr, sx[p], sy[p], c);
        }
    } else {   // a wave per point: no division by the run-time channel count
        for (int p = wave; p < P; p += FU_WAVES)
            for (int c = lane; c < c_g; c += 64)
                feat[p * fs + c] = gather_channel(io.feat_lr, a.feat_hr, a.hl, a.wl, a.hh, a.wh, c_lr, sx[p], sy[p], c);
    }
    __syncthreads();
    if (!io.p_lr) {
        fused_classifier<NP, PB>(a, fs, 0, feat, act, slog, lane, wave);
        if (tid < P) {
            const long long t = t0 + tid;
            const float lg = slog[tid];
            const float p = smask[tid] * (1.0f / (1.0f + expf(-lg)));
            feat[tid * fs + c_g + 1] = p;
            if (t < a.n) {
                io.pred_lr[t] = p;
                if (io.logit_lr) io.logit_lr[t] = lg;
            }
        }
        __syncthreads();
    }
    if (LR_ONLY) return;
    fused_classifier<NP, PB>(a, fs, 1, feat, act, slog, lane, wave);
    if (tid < P) {
        const long long t = t0 + tid;
        const float lg = slog[tid];
        if (t < a.n) {
            io.pred_hr[t] = smask[tid] * (1.0f / (1.0f + expf(-lg)));
            if (io.logit_hr) io.logit_hr[t] = lg;
        }
    }
}

template <int NP, int PB>
__global__ __launch_bounds__(FU_WAVES * 64) void mlp_fused_kernel(FusedArgs a) {   // D = 256
    extern __shared__ __attribute__((aligned(16))) float fu_smem[];
    mlp_fused_body<NP, PB, true>(a, fu_smem, a);
}

template <int NP, int PB>
__global__ __launch_bounds__(FU_WAVES * 64) void mlp_anyd_kernel(FusedArgs a) {    // any other D
    extern __shared__ __attribute__((aligned(16))) float fu_smem[];
    mlp_fused_body<NP, PB, false>(a, fu_smem, a);
}

// points per tile: 32 when the widest hidden layer leaves room for them in LDS, else 16
static int fused_pb(const GenLayout &lay) { return 32 * (lay.max_hidden + 4 + gen_feat_stride(lay.hg_dim)) * 4 + 4 * 32 * 4 <= GEN_LDS_BYTES ? 2 : 1; }
static int fused_lds_bytes(const GenLayout &lay, int pb) { return 16 * pb * ((lay.max_hidden + 4 + gen_feat_stride(lay.hg_dim)) * 4 + 16); }

static void fused_strides(FusedArgs &a) {
    a.as = a.lay.max_hidden + 4;
    a.fs = gen_feat_stride(a.lay.hg_dim);
}

// operand parts of this call: the calling thread's surs_set_operand_split_local (1: one f16 product), else the process setting
static int fused_parts() {
    if (t_split_call >= 1) return t_split_call;
    if (g_split_override) return g_split_override;
    return option(OPT_SPLIT_PARTS) == 3 ? 3 : 2;
}

template <int NP, int PB>
static int launch_fused_t(hipStream_t st, const FusedArgs &a, int lds) {
    if (a.lay.hg_dim != C_LR) {
        static DeviceOnce attr_anyd;
        if (attr_anyd.first())
            SURS_HIP_CHECK(hipFuncSetAttribute((const void *)mlp_anyd_kernel<NP, PB>, hipFuncAttributeMaxDynamicSharedMemorySize, lds > 65536 ? 160 * 1024 : 65536));
        hipLaunchKernelGGL((mlp_anyd_kernel<NP, PB>), dim3((unsigned)ceil_div(a.n, 16 * PB)), dim3(FU_WAVES * 64), lds, st, a);
        SURS_LAUNCH_CHECK();
        return 0;
    }
    static DeviceOnce attr;
    if (attr.first())
        SURS_HIP_CHECK(hipFuncSetAttribute((const void *)mlp_fused_kernel<NP, PB>, hipFuncAttributeMaxDynamicSharedMemorySize, lds > 65536 ? 160 * 1024 : 65536));
    hipLaunchKernelGGL((mlp_fused_kernel<NP, PB>), dim3((unsigned)ceil_div(a.n, 16 * PB)), dim3(FU_WAVES * 64), lds, st, a);
    SURS_LAUNCH_CHECK();
    return 0;
}

static int run_fused(hipStream_t st, FusedArgs &a) {
    if (a.n == 0) return 0;
    const int pb = fused_pb(a.lay), lds = fused_lds_bytes(a.lay, pb), parts = fused_parts();
    fused_strides(a);
    switch (parts * 2 + pb - 1) {
    case 2: return launch_fused_t<1, 1>(st, a, lds);
    case 3: return launch_fused_t<1, 2>(st, a, lds);
    case 4: return launch_fused_t<2, 1>(st, a, lds);
    case 5: return launch_fused_t<2, 2>(st, a, lds);
    case 6: return launch_fused_t<3, 1>(st, a, lds);
    default: return launch_fused_t<3, 2>(st, a, lds);
    }
}

static int fused_prepare(FusedArgs &a, const SursMlpShape *lr, const SursMlpShape *hr, const float *calib, float zmul, float zdiv,
                         const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const void *blob) {
    SURS_REQUIRE(lr && hr && calib && feat_lr && feat_hr && blob, "null argument");
    SURS_REQUIRE(hl > 0 && wl > 0 && hh > 0 && wh > 0, "bad sizes");
    memset(&a, 0, sizeof(a));
    const int rc = gen_layout(*lr, *hr, a.lay);
    char why[160];
    SURS_REQUIRE(rc == 0, "unsupported SurfaceClassifier shape: %s", gen_shape_error(rc, *lr, why));
    for (int i = 0; i < 12; ++i) a.src.calib[i] = calib[i];
    a.src.zmul = zmul;
    a.src.zdiv = zdiv;
    a.feat_lr = feat_lr;
    a.feat_hr = feat_hr;
    a.hl = hl;
    a.wl = wl;
    a.hh = hh;
    a.wh = wh;
    a.blob = (const char *)blob;
    return 0;
}

}  // namespace surs

extern "C" int surs_mlp_generic_info(const SursMlpShape *lr, const SursMlpShape *hr, int *tile_points, int *lds_bytes,
                                     unsigned long long *offsets) {
    SURS_REQUIRE(lr && hr, "null shape");
    GenLayout lay;
    const int rc = gen_layout(*lr, *hr, lay);
    char why[160];
    SURS_REQUIRE(rc == 0, "unsupported SurfaceClassifier shape: %s", gen_shape_error(rc, *lr, why));
    const int pb = fused_pb(lay);
    if (tile_points) *tile_points = 16 * pb;
    if (lds_bytes) *lds_bytes = fused_lds_bytes(lay, pb);
    if (offsets)
        for (int m = 0; m < 2; ++m)
            for (int l = 0; l < GEN_MAX_LAYERS; ++l) {
                const GenLayer &g = lay.layer[m][l];
                unsigned long long *o = offsets + (m * GEN_MAX_LAYERS + l) * 4;
                const bool used = l < lay.n_layers[m];
                o[0] = used ? g.w1 : 0;
                o[1] = used ? g.w2 : 0;
                o[2] = used ? g.w3 : 0;
                o[3] = used ? g.bias : 0;
            }
    return 0;
}

extern "C" int surs_query_points_generic(const float *points, int n, const float *calib, float zmul, float zdiv, const float *feat_lr,
                                         int hl, int wl, const float *feat_hr, int hh, int wh, const SursMlpShape *lr,
                                         const SursMlpShape *hr, const void *blob, const float *p_lr, float *pred_hr, float *pred_lr,
                                         float *logit_hr, float *logit_lr, void *stream) {
    SURS_REQUIRE(n >= 0, "negative point count");
    if (n == 0) return 0;
    SURS_REQUIRE(points && pred_hr && (p_lr || pred_lr), "null argument");
    FusedArgs a;
    int rc = fused_prepare(a, lr, hr, calib, zmul, zdiv, feat_lr, hl, wl, feat_hr, hh, wh, blob);
    if (rc) return rc;
    a.src.mode = 0;
    a.src.pts = points;
    a.src.ld = n;
    a.n = n;
    a.p_lr = p_lr;
    a.pred_hr = pred_hr;
    a.pred_lr = p_lr ? nullptr : pred_lr;
    a.logit_hr = logit_hr;
    a.logit_lr = p_lr ? nullptr : logit_lr;
    return run_fused(as_stream(stream), a);
}

extern "C" int surs_query_grid_generic(int i0, int i1, int ry, int rz, const double *mat, const float *calib, float zmul, float zdiv,
                                       const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const SursMlpShape *lr,
                                       const SursMlpShape *hr, const void *blob, float *vol_hr, float *vol_lr, void *stream) {
    SURS_REQUIRE(i0 >= 0 && i1 >= i0 && ry > 0 && rz > 0, "bad grid range");
    if (i1 == i0) return 0;
    SURS_REQUIRE(mat && vol_hr && vol_lr, "null argument");
    FusedArgs a;
    int rc = fused_prepare(a, lr, hr, calib, zmul, zdiv, feat_lr, hl, wl, feat_hr, hh, wh, blob);
    if (rc) return rc;
    a.src.mode = 1;   // flat voxel index base + t, z fastest (make_point: float64 coordinates, then float32)
    a.src.base = (long long)i0 * ry * rz;
    a.src.ry = ry;
    a.src.rz = rz;
    for (int i = 0; i < 12; ++i) a.src.mat[i] = mat[i];
    a.n = (long long)(i1 - i0) * ry * rz;
    a.pred_hr = vol_hr;
    a.pred_lr = vol_lr;
    return run_fused(as_stream(stream), a);
}
