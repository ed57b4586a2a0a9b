// The reduction of SuRSNet.forward's loss, stated once for its two entries: surs_forward_losses (surs_mlp_fused_stacks.inc) and
// surs_forward_losses_grad (surs_train_step.hip), which must give the same bits on the same values.
// Stage 1: LOSS_BLOCKS workgroups of LOSS_THREADS threads; thread t of workgroup b takes elements (b LOSS_THREADS + t) + k LOSS_BLOCKS
// LOSS_THREADS in ascending k - a partition that depends on the sizes only -, float64 sums, then the workgroup's tree over LDS.
// Stage 2: one workgroup adds the LOSS_BLOCKS partial sums of each term in the same tree.  No atomics: two runs give the same bits.
#pragma once
#include "surs_common.h"

namespace surs {

constexpr int LOSS_BLOCKS = 256, LOSS_THREADS = 256;

__device__ __forceinline__ void loss_tree(double (&v)[4], double (*sh)[LOSS_THREADS], int tid) {
#pragma unroll
    for (int t = 0; t < 4; ++t) sh[t][tid] = v[t];
    __syncthreads();
    for (int d = LOSS_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) {
#pragma unroll
            for (int t = 0; t < 4; ++t) sh[t][tid] += sh[t][tid + d];
        }
        __syncthreads();
    }
}

// terms 0, 1 and 3 of one thread's share of the m points: v[0], v[1], v[3]
__device__ __forceinline__ void loss_points(double (&v)[4], const float *__restrict__ pred_lr, const float *__restrict__ pred_hr, int stacks,
                                            long long m, const float *__restrict__ lab_lr, const float *__restrict__ lab_hr,
                                            long long first, long long step) {
    const bool want_lr = pred_lr && lab_lr, want_hr = pred_hr && lab_hr, want_disp = want_lr && want_hr;
    for (long long i = first; i < m; i += step) {
        const double ll = want_lr ? (double)lab_lr[i] : 0.0, lh = want_hr ? (double)lab_hr[i] : 0.0;
        for (int s = 0; s < stacks; ++s) {
            if (want_lr) {
                const double d = (double)pred_lr[(size_t)s * m + i] - ll;
                v[0] += d * d;
            }
            if (want_hr) {
                const double d = (double)pred_hr[(size_t)s * m + i] - lh;
                v[1] += d * d;
            }
        }
        if (want_disp) {
            const size_t o = (size_t)(stacks - 1) * m + i;
            const double d = (lh - ll) - ((double)pred_hr[o] - (double)pred_lr[o]);
            v[3] += d * d;
        }
    }
}

// stage 2, the body of a one-workgroup kernel of LOSS_THREADS threads
__device__ __forceinline__ void loss_final(const double *__restrict__ partial, int stacks, long long m, long long k, float w0, float w1,
                                           float w2, float w3, float *__restrict__ terms, float *__restrict__ total,
                                           double (*sh)[LOSS_THREADS]) {
    static_assert(LOSS_BLOCKS == LOSS_THREADS, "one partial sum per thread");
    const int tid = threadIdx.x;
    double v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = partial[tid * 4 + t];
    loss_tree(v, sh, tid);
    if (tid == 0) {
        const double sm = (double)stacks * (double)m;
        const float e0 = m > 0 ? (float)(sh[0][0] / sm) : 0.0f, e1 = m > 0 ? (float)(sh[1][0] / sm) : 0.0f;
        const float e2 = k > 0 ? (float)(sh[2][0] / (double)k) : 0.0f, e3 = m > 0 ? (float)(sh[3][0] / (double)m) : 0.0f;
        terms[0] = e0;
        terms[1] = e1;
        terms[2] = e2;
        terms[3] = e3;
        // SuRSNet.py:265 in float32, left to right
        if (total) *total = w0 * e0 + w1 * e1 + w2 * e2 + w3 * e3;
    }
}

}  // namespace surs
