// Fused multi-view evaluator for SurfaceClassifier pairs of any supported shape, included after surs_mlp_fused.inc.  ONE launch per
// call, V <= 64 views of one subject (points [V][3][n] / one grid seen by every view, calibs [V][12], feature maps [V][...]):
// SurfaceClassifier.py:53-81 with num_views > 1 and SuRSNet.py:131-187.  Per tile of P points and classifier (lr, then hr), with
// M = L / 2 its merge layer:
//   for every view v in order: projection with calib_v (its in-image bit kept in LDS, [P] x 64 bits), gather of the view's D + 64
//   channels + z_feat (+ channel D + 65 = view v's pred_lr for hr) into feat exactly as mlp_fused_kernel does, and into a running
//   sum fsum [P][fs] in LDS (fs = gen_feat_stride(D), 356 for the released D = 256) (each value is summed by the thread that gathered it); layers 0 .. M on them (fused_layers<VIEWS>:
//   layer M's outputs go into a running sum in the accumulating waves' registers - each wave owns the same output tiles for every
//   view -, not to LDS);
//   then the two means ((sum in view order) * (1 / V), as mean_views_kernel) into feat and act (or slog when M = L - 1: the mean
//   of the logits), layers M + 1 .. L - 1 once per point, and pred_v = mask_v * sigmoid(logit) for every view.
// The hr pass gathers every view again (the same bits; no per-view feature copy in LDS).  Same blob, same products and product
// order as mlp_fused_kernel: with V = 1 both give the same bits (the means are x * 1), and a point's result does not depend on its
// tile or position.
// Budget: LDS = P ((W + 4 + 2 * 356) * 4 + 24) bytes for the widest padded hidden layer W: P = 32 for W <= 544, P = 16 up to
// W = 1824 - the views limit (FV_WIDTH_LIMIT), below the single-view 2048 (D = 256's numbers; D > 256: fused_views_max_hidden).  Registers: the single-view kernel's + the 64 of the
// layer-M sum: 202-236 VGPRs, 0 AGPRs, 0 bytes of scratch over the six <NP, PB> instantiations.

namespace surs {

constexpr int FV_MAX_VIEWS = 64;

struct FusedViewsArgs {
    FusedArgs f;           // src: the points of view 0 (mode 0, view v at pts + 3 v ld) or the grid (mode 1); src.calib unused
    const float *calibs;   // device [V][12]: rows 0..2 of each view's calibration
    int V;
    int rows;              // prediction rows stored: V (points), 1 (grid: view 0's, lib/mesh_util.py:20-28)
    float inv;             // 1 / V
};

// view v's orthogonal projection of point t (project_point's arithmetic; the points of mode 0 are [V][3][ld])
__device__ __forceinline__ void view_project(const FusedViewsArgs &va, int v, long long t, float &X, float &Y, float &Z) {
    const PointSource &s = va.f.src;
    float px, py, pz;
    if (s.mode == 0) {
        const float *p = s.pts + (size_t)v * 3 * s.ld;
        px = p[t];
        py = p[s.ld + t];
        pz = p[2 * s.ld + t];
    } else {
        make_point(s, t, px, py, pz);
    }
    const float *c = va.calibs + 12 * v;
    X = c[3] + ((c[0] * px + c[1] * py) + c[2] * pz);
    Y = c[7] + ((c[4] * px + c[5] * py) + c[6] * pz);
    Z = c[11] + ((c[8] * px + c[9] * py) + c[10] * pz);
}

// the view mean of layer M's outputs (sum * inv) where fused_layers<VIEWS> would have stored them: act, or slog for the last layer
template <int PB>
__device__ __forceinline__ void store_view_mean(const FusedArgs &a, const GenLayer &g, bool last, float *act, float *slog,
                                                const f32x4 (&vsum)[16 / PB][PB], float inv, int lane, int wave) {
    const int mt = g.mpad / GEN_MT;
#pragma unroll
    for (int i = 0; i < 16 / PB; ++i) {
        const int tile = wave + FU_WAVES * i;
        if (tile < mt) {
            const int row0 = tile * GEN_MT + 4 * (lane >> 4);
#pragma unroll
            for (int pb = 0; pb < PB; ++pb) {
                const int pt = pb * 16 + (lane & 15);
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = vsum[i][pb][r] * inv;
                if (!last) *reinterpret_cast<f32x4 *>(act + pt * a.as + row0) = v;
                else if (row0 == 0) slog[pt] = v[0];
            }
        }
    }
}

template <int NP, int PB, bool FIXED>
__device__ __forceinline__ void mlp_fused_views_body(const FusedViewsArgs &va, float *fu_smem) {
    constexpr int P = 16 * PB, TPW = 16 / PB, NT = FU_WAVES * 64;
    const FusedArgs &a = va.f;
    const FeatDims<FIXED> fd(a);
    const int c_lr = fd.c_lr, c_g = fd.c_g, fs = fd.fs;
    float *feat = fu_smem;                 // [P][fs]: D lr, 64 hr, z_feat, p_lr, zeros
    float *fsum = feat + P * fs;           // [P][fs]: their running sum over the views
    float *act = fsum + P * fs;            // [P][as]
    float *sx = act + P * a.as, *sy = sx + P, *slog = sy + P, *sprob = slog + P;   // sprob: sigmoid of the lr logit
    unsigned long long *sbits = (unsigned long long *)(sprob + P);   // in-image bit of view v (8-byte aligned: P (2 fs + as) is even)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long t0 = (long long)blockIdx.x * P;
    const int V = va.V;
    if (tid < P)
        for (int c = c_g + 2; c < fs; ++c) feat[tid * fs + c] = 0.0f;
    for (int m = a.p_lr ? 1 : 0; m < 2; ++m) {
        const int L = a.lay.n_layers[m], M = L / 2;
        f32x4 vsum[TPW][PB];
        for (int v = 0; v < V; ++v) {
            if (tid < P) {
                const long long t = t0 + tid;
                float X = 2.0f, Y = 2.0f, in = 0.0f, zf = 0.0f, pl = 0.0f;   // (past n: outside the image, every tap weighted zero)
                if (t < a.n) {
                    float Z;
                    view_project(va, v, t, X, Y, Z);
                    in = in_image(X, Y);
                    zf = Z * a.src.zmul / a.src.zdiv;
                    if (m == 1) pl = a.p_lr ? a.p_lr[(size_t)v * a.n + t] : in * sprob[tid];
                }
                sx[tid] = X;
                sy[tid] = Y;
                sbits[tid] = (v == 0 ? 0ull : sbits[tid]) | ((unsigned long long)(in != 0.0f) << v);
                float *f = feat + tid * fs;
                float *fsm = fsum + tid * fs;
                f[c_g] = zf;
                f[c_g + 1] = pl;
                fsm[c_g] = v == 0 ? zf : fsm[c_g] + zf;
                fsm[c_g + 1] = v == 0 ? pl : fsm[c_g + 1] + pl;
            }
            __syncthreads();
            const float *fl = a.feat_lr + (size_t)v * a.hl * a.wl * c_lr, *fh = a.feat_hr + (size_t)v * a.hh * a.wh * C_HR;
            auto gather = [&](int p, int c) {
                const float x = gather_channel(fl, fh, a.hl, a.wl, a.hh, a.wh, c_lr, sx[p], sy[p], c);
                feat[p * fs + c] = x;
                fsum[p * fs + c] = v == 0 ? x : fsum[p * fs + c] + x;
            };
            if (FIXED) {
                for (int item = tid; item < P * c_g; item += NT) gather(item / c_g, item % c_g);
            } else {   // (a wave per point, as mlp_fused_kernel gathers)
                for (int p = wave; p < P; p += FU_WAVES)
                    for (int c = lane; c < c_g; c += 64) gather(p, c);
            }
            __syncthreads();
            fused_layers<NP, PB, true>(a, fs, m, 0, M + 1, feat, act, slog, lane, wave, vsum, M, v == 0);
        }
        // the view means (SurfaceClassifier.py:70-76): features into feat, layer M's outputs into act (the logits into slog)
        if (FIXED) {
            for (int item = tid; item < P * (c_g + 2); item += NT) {
                const int p = item / (c_g + 2), c = item - p * (c_g + 2);
                feat[p * fs + c] = fsum[p * fs + c] * va.inv;
            }
        } else {
            for (int p = wave; p < P; p += FU_WAVES)
                for (int c = lane; c < c_g + 2; c += 64) feat[p * fs + c] = fsum[p * fs + c] * va.inv;
        }
        store_view_mean<PB>(a, a.lay.layer[m][M], M == L - 1, act, slog, vsum, va.inv, lane, wave);
        __syncthreads();
        fused_layers<NP, PB, false>(a, fs, m, M + 1, L, feat, act, slog, lane, wave, vsum, -1, false);
        if (tid < P) {
            const long long t = t0 + tid;
            const float lg = slog[tid];
            const float s = 1.0f / (1.0f + expf(-lg));
            if (m == 0) sprob[tid] = s;
            if (t < a.n) {
                float *out = m == 0 ? a.pred_lr : a.pred_hr, *lo = m == 0 ? a.logit_lr : a.logit_hr;
                const unsigned long long bits = sbits[tid];
                for (int v = 0; v < va.rows; ++v) out[(size_t)v * a.n + t] = (((bits >> v) & 1ull) ? 1.0f : 0.0f) * s;
                if (lo) lo[t] = lg;
            }
        }
        __syncthreads();
    }
}

template <int NP, int PB>
__global__ __launch_bounds__(FU_WAVES * 64) void mlp_fused_views_kernel(FusedViewsArgs va) {   // D = 256
    extern __shared__ __attribute__((aligned(16))) float fu_smem[];
    mlp_fused_views_body<NP, PB, true>(va, fu_smem);
}

template <int NP, int PB>
__global__ __launch_bounds__(FU_WAVES * 64) void mlp_anyd_views_kernel(FusedViewsArgs va) {    // any other D
    extern __shared__ __attribute__((aligned(16))) float fu_smem[];
    mlp_fused_views_body<NP, PB, false>(va, fu_smem);
}

// points per tile: 32 when the widest hidden layer leaves room for them in LDS, else 16 (0: not even those - the views limit)
static int fused_views_point_bytes(const GenLayout &lay) { return (lay.max_hidden + 4 + 2 * gen_feat_stride(lay.hg_dim)) * 4 + 24; }
static int fused_views_pb(const GenLayout &lay) {
    const int b = fused_views_point_bytes(lay);
    return 32 * b <= GEN_LDS_BYTES ? 2 : (16 * b <= GEN_LDS_BYTES ? 1 : 0);
}
// the widest padded hidden layer a 16-point tile holds: 1824 up to the released D = 256 (whose two 356-float rows set it), less
// for a larger D (gen_max_hidden: 1312 at D = 512)
constexpr int FV_MAX_HIDDEN = ((GEN_LDS_BYTES / 16 - 24) / 4 - 4 - 2 * 356) / GEN_KT * GEN_KT;
#define FV_WIDTH_LIMIT "multi-view: hidden widths must be at most 1824 (the LDS of a 16-point tile)"
static_assert(FV_MAX_HIDDEN == 1824, "FV_WIDTH_LIMIT names this number");
static int fused_views_max_hidden(int D) { return gen_max_hidden(D, 2, 24, FV_MAX_HIDDEN); }
// refuses a pair whose widest hidden layer the multi-view tile cannot hold
static int fused_views_check_width(const GenLayout &lay) {
    SURS_REQUIRE(lay.max_hidden <= FV_MAX_HIDDEN, FV_WIDTH_LIMIT);
    SURS_REQUIRE(lay.max_hidden <= fused_views_max_hidden(lay.hg_dim),
                 "multi-view: hidden widths must be at most %d with hg_dim %d (the LDS of a 16-point tile)", fused_views_max_hidden(lay.hg_dim),
                 lay.hg_dim);
    return 0;
}
static int fused_views_lds_bytes(const GenLayout &lay, int pb) { return 16 * pb * fused_views_point_bytes(lay); }

template <int NP, int PB>
static int launch_fused_views_t(hipStream_t st, const FusedViewsArgs &a, int lds) {
    if (a.f.lay.hg_dim != C_LR) {
        static DeviceOnce attr_anyd;
        if (attr_anyd.first())
            SURS_HIP_CHECK(hipFuncSetAttribute((const void *)mlp_anyd_views_kernel<NP, PB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               lds > 65536 ? 160 * 1024 : 65536));
        hipLaunchKernelGGL((mlp_anyd_views_kernel<NP, PB>), dim3((unsigned)ceil_div(a.f.n, 16 * PB)), dim3(FU_WAVES * 64), lds, st, a);
        SURS_LAUNCH_CHECK();
        return 0;
    }
    static DeviceOnce attr;
    if (attr.first())
        SURS_HIP_CHECK(hipFuncSetAttribute((const void *)mlp_fused_views_kernel<NP, PB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           lds > 65536 ? 160 * 1024 : 65536));
    hipLaunchKernelGGL((mlp_fused_views_kernel<NP, PB>), dim3((unsigned)ceil_div(a.f.n, 16 * PB)), dim3(FU_WAVES * 64), lds, st, a);
    SURS_LAUNCH_CHECK();
    return 0;
}

static int run_fused_views(hipStream_t st, FusedViewsArgs &a) {
    if (a.f.n == 0) return 0;
    const int pb = fused_views_pb(a.f.lay), lds = fused_views_lds_bytes(a.f.lay, pb), parts = fused_parts();
    fused_strides(a.f);
    switch (parts * 2 + pb - 1) {
    case 2: return launch_fused_views_t<1, 1>(st, a, lds);
    case 3: return launch_fused_views_t<1, 2>(st, a, lds);
    case 4: return launch_fused_views_t<2, 1>(st, a, lds);
    case 5: return launch_fused_views_t<2, 2>(st, a, lds);
    case 6: return launch_fused_views_t<3, 1>(st, a, lds);
    default: return launch_fused_views_t<3, 2>(st, a, lds);
    }
}

static int fused_views_prepare(FusedViewsArgs &a, const SursMlpShape *lr, const SursMlpShape *hr, int num_views, const float *calibs,
                               float zmul, float zdiv, const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                               const void *blob) {
    SURS_REQUIRE(calibs, "null argument");
    static const float no_calib[12] = {};   // (every view's calibration comes from calibs)
    memset(&a, 0, sizeof(a));
    const int rc = fused_prepare(a.f, lr, hr, no_calib, zmul, zdiv, feat_lr, hl, wl, feat_hr, hh, wh, blob);
    if (rc) return rc;
    if (const int rcw = fused_views_check_width(a.f.lay)) return rcw;
    a.calibs = calibs;
    a.V = num_views;
    a.inv = 1.0f / (float)num_views;
    return 0;
}

}  // namespace surs

extern "C" int surs_mlp_generic_views_info(const SursMlpShape *lr, const SursMlpShape *hr, int num_views, int *tile_points,
                                           int *lds_bytes) {
    SURS_REQUIRE(lr && hr, "null shape");
    SURS_REQUIRE(num_views >= 1 && num_views <= FV_MAX_VIEWS, "num_views must be in [1, 64]");
    GenLayout lay;
    const int rc = gen_layout(*lr, *hr, lay);
    char why[160];
    SURS_REQUIRE(rc == 0, "unsupported SurfaceClassifier shape: %s", gen_shape_error(rc, *lr, why));
    if (const int rcw = fused_views_check_width(lay)) return rcw;
    const int pb = fused_views_pb(lay);
    if (tile_points) *tile_points = 16 * pb;
    if (lds_bytes) *lds_bytes = fused_views_lds_bytes(lay, pb);
    return 0;
}

extern "C" int surs_query_points_generic_views(const float *points, int n, int num_views, const float *calibs, float zmul, float zdiv,
                                               const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                                               const SursMlpShape *lr, const SursMlpShape *hr, const void *blob, const float *p_lr,
                                               float *pred_hr, float *pred_lr, float *logit_hr, float *logit_lr, void *stream) {
    SURS_REQUIRE(n >= 0, "negative point count");
    SURS_REQUIRE(num_views >= 1 && num_views <= FV_MAX_VIEWS, "num_views must be in [1, 64]");
    if (n == 0) return 0;
    SURS_REQUIRE(points && pred_hr && (p_lr || pred_lr), "null argument");
    FusedViewsArgs a;
    int rc = fused_views_prepare(a, lr, hr, num_views, calibs, zmul, zdiv, feat_lr, hl, wl, feat_hr, hh, wh, blob);
    if (rc) return rc;
    a.f.src.mode = 0;
    a.f.src.pts = points;
    a.f.src.ld = n;
    a.f.n = n;
    a.f.p_lr = p_lr;
    a.f.pred_hr = pred_hr;
    a.f.pred_lr = p_lr ? nullptr : pred_lr;
    a.f.logit_hr = logit_hr;
    a.f.logit_lr = p_lr ? nullptr : logit_lr;
    a.rows = num_views;
    return run_fused_views(as_stream(stream), a);
}

extern "C" int surs_query_grid_generic_views(int i0, int i1, int ry, int rz, const double *mat, int num_views, const float *calibs,
                                             float zmul, float zdiv, const float *feat_lr, int hl, int wl, const float *feat_hr, int hh,
                                             int wh, const SursMlpShape *lr, const SursMlpShape *hr, const void *blob, float *vol_hr,
                                             float *vol_lr, void *stream) {
    SURS_REQUIRE(i0 >= 0 && i1 >= i0 && ry > 0 && rz > 0, "bad grid range");
    SURS_REQUIRE(num_views >= 1 && num_views <= FV_MAX_VIEWS, "num_views must be in [1, 64]");
    if (i1 == i0) return 0;
    SURS_REQUIRE(mat && vol_hr && vol_lr, "null argument");
    FusedViewsArgs a;
    int rc = fused_views_prepare(a, lr, hr, num_views, calibs, zmul, zdiv, feat_lr, hl, wl, feat_hr, hh, wh, blob);
    if (rc) return rc;
    a.f.src.mode = 1;   // flat voxel index base + t, z fastest: the same voxels for every view
    a.f.src.base = (long long)i0 * ry * rz;
    a.f.src.ry = ry;
    a.f.src.rz = rz;
    for (int i = 0; i < 12; ++i) a.f.src.mat[i] = mat[i];
    a.f.n = (long long)(i1 - i0) * ry * rz;
    a.f.pred_hr = vol_hr;
    a.f.pred_lr = vol_lr;   // (view 0's row; the other views' pred_lr feed the hr pass from LDS)
    a.rows = 1;
    return run_fused_views(as_stream(stream), a);
}
