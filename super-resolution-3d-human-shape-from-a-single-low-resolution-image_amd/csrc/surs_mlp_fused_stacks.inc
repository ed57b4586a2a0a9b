// The fused point evaluator of surs_mlp_fused.inc over S feature maps of one image: what SuRSNet.query_mr / query_sr do in training
// mode, where filter_lr keeps every hourglass stack (lib/model/SuRSNet.py:101-110) and both classifiers run once per kept map
// (SuRSNet.py:149-157, 175-185): pass s reads im_feat_list_lr[s] and im_feat_list_hr[0]; stack s's masked lr prediction is the last
// input channel of stack s's hr classifier.  Included at the end of surs_query.hip, after surs_mlp_fused.inc.
//
// ONE launch per call for all stacks: grid = (point tiles, stacks); workgroup (x, y) is workgroup x of the single-map kernel on map
// y.  The S <= FU_MAX_STACKS lr map pointers travel in the launch argument (a table behind FusedArgs: blockIdx.y picks the entry
// with one scalar load); outputs are [S][n], and so is p_lr in the hr-only form.  The body is mlp_fused_body itself - the same
// instructions on the same values in the same order, so stack s's outputs are bit for bit surs_query_points_generic's on map s, for
// every operand split and both families (D = 256 / any other D) - instantiated with a FusedIo in place of the launch argument's own
// pointers; the single-map kernels keep reading theirs and stay instruction for instruction what they were.
// Forms: both classifiers (p_lr NULL, pred_hr given), hr only (p_lr [S][n] given) and lr only (pred_hr NULL: mlp_stacks_*<.., true>,
// the tile ends after mlp_lr - what forward() runs on points_hr, whose hr predictions nothing reads).
// Resources: those of the single-map kernels (no scratch: tests/test_forward_host.py reads it from the code object); LDS as there.

namespace surs {

constexpr int FU_MAX_STACKS = 8;

struct FusedStackArgs {
    FusedArgs f;                               // everything the stacks share; f.feat_lr, f.p_lr and the outputs: stack 0's
    const float *feat_lr[FU_MAX_STACKS];       // stack s's lr map
};

// mlp_fused_body's IO of one stack
struct FusedIo {
    const float *feat_lr, *p_lr;
    float *pred_hr, *pred_lr, *logit_hr, *logit_lr;
};

__device__ __forceinline__ FusedIo stack_io(const FusedStackArgs &a) {
    const int s = blockIdx.y;
    const size_t o = (size_t)s * (size_t)a.f.n;
    FusedIo io;
    io.feat_lr = a.feat_lr[s];
    io.p_lr = a.f.p_lr ? a.f.p_lr + o : nullptr;
    io.pred_hr = a.f.pred_hr ? a.f.pred_hr + o : nullptr;
    io.pred_lr = a.f.pred_lr ? a.f.pred_lr + o : nullptr;
    io.logit_hr = a.f.logit_hr ? a.f.logit_hr + o : nullptr;
    io.logit_lr = a.f.logit_lr ? a.f.logit_lr + o : nullptr;
    return io;
}

template <int NP, int PB, bool LR_ONLY>
__global__ __launch_bounds__(FU_WAVES * 64) void mlp_stacks_kernel(FusedStackArgs a) {        // D = 256
    extern __shared__ __attribute__((aligned(16))) float fu_smem[];
    mlp_fused_body<NP, PB, true, LR_ONLY>(a.f, fu_smem, stack_io(a));
}

template <int NP, int PB, bool LR_ONLY>
__global__ __launch_bounds__(FU_WAVES * 64) void mlp_stacks_anyd_kernel(FusedStackArgs a) {   // any other D
    extern __shared__ __attribute__((aligned(16))) float fu_smem[];
    mlp_fused_body<NP, PB, false, LR_ONLY>(a.f, fu_smem, stack_io(a));
}

template <int NP, int PB, bool LR_ONLY>
static int launch_stacks_t(hipStream_t st, const FusedStackArgs &a, int stacks, int lds) {
    const dim3 grid((unsigned)ceil_div(a.f.n, 16 * PB), (unsigned)stacks);
    if (a.f.lay.hg_dim != C_LR) {
        static DeviceOnce attr_anyd;
        if (attr_anyd.first())
            SURS_HIP_CHECK(hipFuncSetAttribute((const void *)mlp_stacks_anyd_kernel<NP, PB, LR_ONLY>, hipFuncAttributeMaxDynamicSharedMemorySize, lds > 65536 ? 160 * 1024 : 65536));
        hipLaunchKernelGGL((mlp_stacks_anyd_kernel<NP, PB, LR_ONLY>), grid, dim3(FU_WAVES * 64), lds, st, a);
        SURS_LAUNCH_CHECK();
        return 0;
    }
    static DeviceOnce attr;
    if (attr.first())
        SURS_HIP_CHECK(hipFuncSetAttribute((const void *)mlp_stacks_kernel<NP, PB, LR_ONLY>, hipFuncAttributeMaxDynamicSharedMemorySize, lds > 65536 ? 160 * 1024 : 65536));
    hipLaunchKernelGGL((mlp_stacks_kernel<NP, PB, LR_ONLY>), grid, dim3(FU_WAVES * 64), lds, st, a);
    SURS_LAUNCH_CHECK();
    return 0;
}

template <bool LR_ONLY>
static int run_stacks(hipStream_t st, FusedStackArgs &a, int stacks) {
    const int pb = fused_pb(a.f.lay), lds = fused_lds_bytes(a.f.lay, pb), parts = fused_parts();
    fused_strides(a.f);
    switch (parts * 2 + pb - 1) {
    case 2: return launch_stacks_t<1, 1, LR_ONLY>(st, a, stacks, lds);
    case 3: return launch_stacks_t<1, 2, LR_ONLY>(st, a, stacks, lds);
    case 4: return launch_stacks_t<2, 1, LR_ONLY>(st, a, stacks, lds);
    case 5: return launch_stacks_t<2, 2, LR_ONLY>(st, a, stacks, lds);
    case 6: return launch_stacks_t<3, 1, LR_ONLY>(st, a, stacks, lds);
    default: return launch_stacks_t<3, 2, LR_ONLY>(st, a, stacks, lds);
    }
}

}  // namespace surs

extern "C" int surs_query_points_generic_stacks(const float *points, int n, const float *calib, float zmul, float zdiv, int num_stacks,
                                                const float *const *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                                                const SursMlpShape *lr, const SursMlpShape *hr, const void *blob, const float *p_lr,
                                                float *pred_hr, float *pred_lr, float *logit_hr, float *logit_lr, void *stream) {
    SURS_REQUIRE(n >= 0, "negative point count");
    SURS_REQUIRE(num_stacks >= 1, "num_stacks must be at least 1");
    if (n == 0) return 0;
    SURS_REQUIRE(points && feat_lr, "null argument");
    SURS_REQUIRE(pred_hr || (pred_lr && !p_lr), "no output: pred_hr (both classifiers, or hr only with p_lr) or pred_lr alone (lr only)");
    SURS_REQUIRE(p_lr || pred_lr, "null argument: pred_lr");
    for (int s = 0; s < num_stacks; ++s) SURS_REQUIRE(feat_lr[s], "null feature map of stack %d", s);
    const bool lr_only = pred_hr == nullptr;
    // (more than FU_MAX_STACKS maps: one launch per table-full, the same kernels on the same values)
    for (int s0 = 0; s0 < num_stacks; s0 += FU_MAX_STACKS) {
        const int ns = num_stacks - s0 < FU_MAX_STACKS ? num_stacks - s0 : FU_MAX_STACKS;
        const size_t o = (size_t)s0 * (size_t)n;
        FusedStackArgs a;
        int rc = fused_prepare(a.f, lr, hr, calib, zmul, zdiv, feat_lr[s0], hl, wl, feat_hr, hh, wh, blob);
        if (rc) return rc;
        for (int s = 0; s < FU_MAX_STACKS; ++s) a.feat_lr[s] = feat_lr[s0 + (s < ns ? s : 0)];
        a.f.src.mode = 0;
        a.f.src.pts = points;
        a.f.src.ld = n;
        a.f.n = n;
        a.f.p_lr = p_lr ? p_lr + o : nullptr;
        a.f.pred_hr = lr_only ? nullptr : pred_hr + o;
        a.f.pred_lr = p_lr ? nullptr : pred_lr + o;
        a.f.logit_hr = (lr_only || !logit_hr) ? nullptr : logit_hr + o;
        a.f.logit_lr = (p_lr || !logit_lr) ? nullptr : logit_lr + o;
        rc = lr_only ? run_stacks<true>(as_stream(stream), a, ns) : run_stacks<false>(as_stream(stream), a, ns);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The released shape: the layer kernels of surs_query_points, once per stack, inside the library - one call, one workspace.
// ------------------------------------------------------------------------------------------------
extern "C" int surs_query_points_stacks(const float *points, int n, const float *calib, float zmul, float zdiv, int num_stacks,
                                        const float *const *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                                        const void *mlp_blob, void *workspace, size_t workspace_bytes, const float *p_lr, float *pred_hr,
                                        float *pred_lr, float *logit_hr, float *logit_lr, void *stream) {
    SURS_REQUIRE(n >= 0, "negative point count");
    SURS_REQUIRE(num_stacks >= 1, "num_stacks must be at least 1");
    if (n == 0) return 0;
    SURS_REQUIRE(points && calib && feat_lr && feat_hr && mlp_blob && workspace, "null argument");
    SURS_REQUIRE(pred_hr || (pred_lr && !p_lr), "no output: pred_hr (both classifiers, or hr only with p_lr) or pred_lr alone (lr only)");
    SURS_REQUIRE(p_lr || pred_lr, "null argument: pred_lr");
    SURS_REQUIRE(hl > 0 && wl > 0 && hh > 0 && wh > 0, "bad sizes");
    for (int s = 0; s < num_stacks; ++s) SURS_REQUIRE(feat_lr[s], "null feature map of stack %d", s);
    hipStream_t st = as_stream(stream);
    const long long np = (long long)ceil_div(n, 256) * 256;
    SURS_REQUIRE(workspace_bytes >= fp32_ws_bytes(np), "workspace too small: need %zu bytes", fp32_ws_bytes(np));
    const MlpBlobHeader h = blob_layout(SURS_BF16);
    PointSource src = point_source(0, 0, 0, nullptr, calib, zmul, zdiv);
    src.pts = points;
    src.ld = n;
    Fp32Workspace w = carve_fp32(workspace, np);
    int rc = zero_pad_rows(st, w);   // (once: no pass writes those rows)
    if (rc) return rc;
    const bool lr_only = pred_hr == nullptr;
    for (int s = 0; s < num_stacks; ++s) {
        const size_t o = (size_t)s * (size_t)n;
        rc = run_points_fp32(st, src, n, feat_lr[s], hl, wl, feat_hr, hh, wh, (const char *)mlp_blob, h, w, lr_only ? nullptr : pred_hr + o,
                             p_lr ? nullptr : pred_lr + o, (lr_only || !logit_hr) ? nullptr : logit_hr + o,
                             (p_lr || !logit_lr) ? nullptr : logit_lr + o, 0, p_lr ? p_lr + o : nullptr, lr_only);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The four terms of SuRSNet.forward's loss (lib/model/SuRSNet.py:196-236, 257-265) in one deterministic reduction.
//   0  get_error_lr      mean over stacks of MSE(pred_lr[s], lab_lr)          = sum_{s,i} (pred_lr[s][i] - lab_lr[i])^2 / (S M)
//   1  get_error_hr      the same of pred_hr, lab_hr
//   2  get_errorSR       L1 mean of img_sr - img_hr                           = sum_j |img_sr[j] - img_hr[j]| / K
//   3  get_error_disp_1  MSE(lab_hr - lab_lr, pred_hr[S-1] - pred_lr[S-1])
// The partition, the float64 tree and the second stage are surs_loss_reduce.h's (shared with surs_forward_losses_grad): a fixed
// partition, no atomics, two runs give the same bits.
// ------------------------------------------------------------------------------------------------
#include "surs_loss_reduce.h"

namespace surs {

__global__ __launch_bounds__(LOSS_THREADS) void loss_partial_kernel(const float *__restrict__ pred_lr, const float *__restrict__ pred_hr,
                                                                    int stacks, long long m, const float *__restrict__ lab_lr,
                                                                    const float *__restrict__ lab_hr, const float *__restrict__ img_sr,
                                                                    const float *__restrict__ img_hr, long long k,
                                                                    double *__restrict__ partial) {
    __shared__ double sh[4][LOSS_THREADS];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * LOSS_THREADS + tid, step = (long long)LOSS_BLOCKS * LOSS_THREADS;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    loss_points(v, pred_lr, pred_hr, stacks, m, lab_lr, lab_hr, first, step);
    if (img_sr && img_hr)
        for (long long j = first; j < k; j += step) v[2] += fabs((double)img_sr[j] - (double)img_hr[j]);
    loss_tree(v, sh, tid);
    if (tid < 4) partial[blockIdx.x * 4 + tid] = sh[tid][0];
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_final_kernel(const double *__restrict__ partial, int stacks, long long m, long long k,
                                                                  float w0, float w1, float w2, float w3, float *__restrict__ terms,
                                                                  float *__restrict__ total) {
    __shared__ double sh[4][LOSS_THREADS];
    loss_final(partial, stacks, m, k, w0, w1, w2, w3, terms, total, sh);
}

}  // namespace surs

extern "C" size_t surs_forward_losses_workspace_bytes(void) { return (size_t)LOSS_BLOCKS * 4 * sizeof(double); }

extern "C" int surs_forward_losses(const float *pred_lr, const float *pred_hr, int num_stacks, long long m, const float *lab_lr,
                                   const float *lab_hr, const float *img_sr, const float *img_hr, long long k, const float *weights,
                                   void *workspace, size_t workspace_bytes, float *terms, float *total, void *stream) {
    SURS_REQUIRE(num_stacks >= 1 && m >= 0 && k >= 0, "bad sizes");
    SURS_REQUIRE(workspace && terms, "null argument");
    SURS_REQUIRE(workspace_bytes >= surs_forward_losses_workspace_bytes(), "workspace too small: need %zu bytes",
                 surs_forward_losses_workspace_bytes());
    SURS_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0, "workspace must be 8-byte aligned");
    SURS_REQUIRE(!total || weights, "total needs the four weights");
    hipStream_t st = as_stream(stream);
    double *partial = (double *)workspace;
    hipLaunchKernelGGL(loss_partial_kernel, dim3(LOSS_BLOCKS), dim3(LOSS_THREADS), 0, st, pred_lr, pred_hr, num_stacks, m, lab_lr, lab_hr,
                       img_sr, img_hr, k, partial);
    SURS_LAUNCH_CHECK();
    const float w0 = weights ? weights[0] : 0.0f, w1 = weights ? weights[1] : 0.0f, w2 = weights ? weights[2] : 0.0f,
                w3 = weights ? weights[3] : 0.0f;
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, (const double *)partial, num_stacks, m, k, w0, w1, w2, w3,
                       terms, total);
    SURS_LAUNCH_CHECK();
    return 0;
}
