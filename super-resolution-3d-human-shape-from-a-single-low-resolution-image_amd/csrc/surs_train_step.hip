// What SuRSNet.forward_backward(encoder=True) and optim.Optimizer.step(guard=True) need besides the taped forwards and backwards
// (include/surs.h, "training step"):
//   surs_forward_losses_grad       surs_forward_losses with img_sr in the model's NHWC memory and img_hr as the dataset hands it (NCHW),
//                                  and the gradient of the weighted image term with respect to img_sr, in NHWC
//   surs_tensors_nonfinite         the lowest index of a device table of tensors that holds a NaN or an infinity
//   surs_tensors_nonfinite_host    the same predicate looped on the host
// Both are bandwidth-trivial (a few MB per step); what matters is that the loss keeps surs_forward_losses' bits - the partition, the
// float64 tree and the second stage are surs_loss_reduce.h's, over the NCHW index; only the address of img_sr differs - and that the
// guard's answer does not depend on scheduling: per-chunk results in the workspace, a minimum in chunk order, no atomics.
#include <cstdint>

#include "surs_common.h"
#include "surs_loss_reduce.h"
#include "surs_optim_update.h"
#include "surs_train_step.h"

namespace surs {

__global__ __launch_bounds__(LOSS_THREADS) void loss_grad_partial_kernel(const float *__restrict__ pred_lr, const float *__restrict__ pred_hr,
                                                                         int stacks, long long m, const float *__restrict__ lab_lr,
                                                                         const float *__restrict__ lab_hr, const float *__restrict__ img_sr,
                                                                         const float *__restrict__ img_hr, int channels, long long hw,
                                                                         long long k, float scale, float *__restrict__ d_img_sr,
                                                                         double *__restrict__ partial) {
    __shared__ double sh[4][LOSS_THREADS];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * LOSS_THREADS + tid, step = (long long)LOSS_BLOCKS * LOSS_THREADS;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    loss_points(v, pred_lr, pred_hr, stacks, m, lab_lr, lab_hr, first, step);
    if (img_sr && img_hr) {
        const long long chw = (long long)channels * hw;
        // j runs over the NCHW index [b][c][y][x] - img_hr's own order, and the order surs_forward_losses sums in; img_sr and d_img_sr
        // lie at [b][y][x][c]
        for (long long j = first; j < k; j += step) {
            const long long b = j / chw, r = j - b * chw, c = r / hw, p = r - c * hw;
            const long long a = b * chw + p * channels + c;
            const float s = img_sr[a], h = img_hr[j];
            v[2] += fabs((double)s - (double)h);
            if (d_img_sr) d_img_sr[a] = ts_l1_grad(s - h, scale);
        }
    }
    loss_tree(v, sh, tid);
    if (tid < 4) partial[blockIdx.x * 4 + tid] = sh[tid][0];
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_grad_final_kernel(const double *__restrict__ partial, int stacks, long long m,
                                                                       long long k, float w0, float w1, float w2, float w3,
                                                                       float *__restrict__ terms, float *__restrict__ total) {
    __shared__ double sh[4][LOSS_THREADS];
    loss_final(partial, stacks, m, k, w0, w1, w2, w3, terms, total, sh);
}

// ------------------------------------------------------------------------------------------------
// The non-finite guard.  A workgroup visit is a chunk of OU_CHUNK consecutive elements of one item, found by bisection of the
// chunk_end prefix, as surs_optim_step finds its chunks; the visit leaves the item's index, or TS_CLEAN, at the chunk's place in the
// workspace.  16-byte loads where the chunk is 16-byte aligned (chunks start at multiples of 4096 elements: the tensor's alignment).
// ------------------------------------------------------------------------------------------------
constexpr int TN_THREADS = 256, TN_GRID = 2048, TN_WAVES = TN_THREADS / 64;

typedef __attribute__((address_space(1))) const float gcfloat;
typedef float tn_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const tn_f32x4 gcf32x4;

__global__ __launch_bounds__(TN_THREADS) void nonfinite_chunks_kernel(const SursTensorRef *__restrict__ items, int n, int total,
                                                                      int *__restrict__ chunk_hit) {
    __shared__ int sh[TN_WAVES];
    const int tid = threadIdx.x;
    // Precondition: n >= 1 (items[n - 1] is read).  surs_tensors_nonfinite launches this kernel only with total > 0, which a table
    // without items cannot have.
    // (never beyond the workspace the host sized from ITS copy of the table)
    const int end = items[n - 1].chunk_end < total ? items[n - 1].chunk_end : total;
    for (int t = blockIdx.x; t < end; t += gridDim.x) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].chunk_end > t) hi = mid;
            else lo = mid + 1;
        }
        const SursTensorRef it = items[lo];
        const long long e0 = (long long)(t - (it.chunk_end - ou_chunks(it.n))) * OU_CHUNK;
        bool bad = false;
        if (it.p && e0 >= 0 && e0 < it.n) {                                     // (uniform over the workgroup)
            const int cnt = it.n - e0 < OU_CHUNK ? (int)(it.n - e0) : OU_CHUNK;
            gcfloat *p = (gcfloat *)(it.p + e0);
            if (((uintptr_t)p & 15) == 0) {
                const int n4 = cnt >> 2;
                for (int i = tid; i < n4; i += TN_THREADS) {
                    const tn_f32x4 x = ((gcf32x4 *)p)[i];
                    bad |= ts_nonfinite(x[0]) || ts_nonfinite(x[1]) || ts_nonfinite(x[2]) || ts_nonfinite(x[3]);
                }
                const int i = (n4 << 2) + tid;
                if (i < cnt) bad |= ts_nonfinite(p[i]);
            } else {
                for (int i = tid; i < cnt; i += TN_THREADS) bad |= ts_nonfinite(p[i]);
            }
        }
        const bool wave_bad = __any(bad);
        if ((tid & 63) == 0) sh[tid >> 6] = wave_bad;
        __syncthreads();
        if (tid == 0) {
            int any = 0;
            for (int w = 0; w < TN_WAVES; ++w) any |= sh[w];
            chunk_hit[t] = any ? lo : TS_CLEAN;
        }
        __syncthreads();
    }
}

// The minimum over the chunks: thread t takes chunks t, t + TN_THREADS, ... in ascending order, then a tree over LDS.  (A minimum of
// integers is the same in any order; the fixed order is kept so that the kernel reads like the loss's second stage.)
__global__ __launch_bounds__(TN_THREADS) void nonfinite_min_kernel(const int *__restrict__ chunk_hit, int total, int *__restrict__ result) {
    __shared__ int sh[TN_THREADS];
    const int tid = threadIdx.x;
    int v = TS_CLEAN;
    for (int t = tid; t < total; t += TN_THREADS) v = chunk_hit[t] < v ? chunk_hit[t] : v;
    sh[tid] = v;
    __syncthreads();
    for (int d = TN_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) sh[tid] = sh[tid + d] < sh[tid] ? sh[tid + d] : sh[tid];
        __syncthreads();
    }
    if (tid == 0) *result = sh[0] == TS_CLEAN ? -1 : sh[0];
}

// the table's check on a HOST copy; *total: its chunk count
static int tensors_check(const SursTensorRef *items, int n_items, long long *total) {
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_tensors_nonfinite: a null table of %d items", n_items);
    long long end = 0;
    for (int i = 0; i < n_items; ++i) {
        const SursTensorRef &it = items[i];
        SURS_REQUIRE(it.n >= 0 && it.n <= (long long)OU_CHUNK * 0x7fffffff, "surs_tensors_nonfinite: item %d has n = %lld", i, it.n);
        end += ou_chunks(it.n);
        SURS_REQUIRE(end <= 0x7fffffff && it.chunk_end == (int)end, "surs_tensors_nonfinite: item %d has chunk_end %d, the prefix sum is %lld",
                     i, it.chunk_end, end);
        SURS_REQUIRE(it.n == 0 || it.p, "surs_tensors_nonfinite: item %d has a null pointer", i);
    }
    *total = end;
    return SURS_OK;
}

}  // namespace surs

using namespace surs;

extern "C" size_t surs_forward_losses_grad_workspace_bytes(void) { return (size_t)LOSS_BLOCKS * 4 * sizeof(double); }

extern "C" int surs_forward_losses_grad(const float *pred_lr, const float *pred_hr, int num_stacks, long long m, const float *lab_lr,
                                        const float *lab_hr, const float *img_sr, const float *img_hr, int batch, int channels, int height,
                                        int width, const float *weights, void *workspace, size_t workspace_bytes, float *terms,
                                        float *total, float *d_img_sr, void *stream) {
    SURS_REQUIRE(num_stacks >= 1 && m >= 0, "surs_forward_losses_grad: bad sizes");
    SURS_REQUIRE(batch >= 0 && channels >= 1 && height >= 0 && width >= 0, "surs_forward_losses_grad: an image batch of %d x %d x %d x %d",
                 batch, channels, height, width);
    SURS_REQUIRE(workspace && terms, "surs_forward_losses_grad: null argument");
    SURS_REQUIRE(workspace_bytes >= surs_forward_losses_grad_workspace_bytes(), "surs_forward_losses_grad: workspace too small: need %zu bytes",
                 surs_forward_losses_grad_workspace_bytes());
    SURS_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0, "surs_forward_losses_grad: workspace must be 8-byte aligned");
    SURS_REQUIRE(!total || weights, "surs_forward_losses_grad: total needs the four weights");
    SURS_REQUIRE(!d_img_sr || (weights && img_sr && img_hr), "surs_forward_losses_grad: d_img_sr needs the weights and both images");
    SURS_REQUIRE(!d_img_sr || d_img_sr != img_sr, "surs_forward_losses_grad: d_img_sr must not be img_sr");
    const long long hw = (long long)height * width, k = (long long)batch * channels * hw;
    hipStream_t st = as_stream(stream);
    double *partial = (double *)workspace;
    const float w0 = weights ? weights[0] : 0.0f, w1 = weights ? weights[1] : 0.0f, w2 = weights ? weights[2] : 0.0f,
                w3 = weights ? weights[3] : 0.0f;
    hipLaunchKernelGGL(loss_grad_partial_kernel, dim3(LOSS_BLOCKS), dim3(LOSS_THREADS), 0, st, pred_lr, pred_hr, num_stacks, m, lab_lr,
                       lab_hr, img_sr, img_hr, channels, hw > 0 ? hw : 1, k, ts_l1_scale(w2, k), d_img_sr, partial);
    SURS_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_grad_final_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, (const double *)partial, num_stacks, m, k, w0, w1, w2,
                       w3, terms, total);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_forward_losses_grad_host(const float *img_sr, const float *img_hr, int batch, int channels, int height, int width,
                                             float w_sr, float *d_img_sr) {
    SURS_REQUIRE(img_sr && img_hr && d_img_sr, "surs_forward_losses_grad_host: null argument");
    SURS_REQUIRE(batch >= 0 && channels >= 1 && height >= 0 && width >= 0, "surs_forward_losses_grad_host: bad sizes");
    const long long hw = (long long)height * width, chw = channels * hw, k = batch * chw;
    const float scale = ts_l1_scale(w_sr, k);
    for (long long j = 0; j < k; ++j) {
        const long long b = j / chw, r = j - b * chw, c = r / hw, p = r - c * hw, a = b * chw + p * channels + c;
        d_img_sr[a] = ts_l1_grad(img_sr[a] - img_hr[j], scale);
    }
    return SURS_OK;
}

extern "C" size_t surs_tensors_nonfinite_workspace_bytes(long long total_chunks) {
    return total_chunks > 0 ? (size_t)total_chunks * sizeof(int) : 0;
}

extern "C" int surs_tensors_nonfinite_check(const SursTensorRef *items, int n_items, long long *total_chunks) {
    long long total = 0;
    const int rc = tensors_check(items, n_items, &total);
    if (rc) return rc;
    if (total_chunks) *total_chunks = total;
    return SURS_OK;
}

extern "C" int surs_tensors_nonfinite(const SursTensorRef *items, int n_items, long long total_chunks, void *workspace,
                                      size_t workspace_bytes, int *result, void *stream) {
    SURS_REQUIRE(result, "surs_tensors_nonfinite: null result");
    SURS_REQUIRE(n_items >= 0 && (items || n_items == 0), "surs_tensors_nonfinite: a null table of %d items", n_items);
    SURS_REQUIRE(total_chunks >= 0 && total_chunks <= 0x7fffffff, "surs_tensors_nonfinite: %lld chunks", total_chunks);
    SURS_REQUIRE(workspace_bytes >= surs_tensors_nonfinite_workspace_bytes(total_chunks) && (workspace || total_chunks == 0 || n_items == 0),
                 "surs_tensors_nonfinite: workspace too small: need %zu bytes", surs_tensors_nonfinite_workspace_bytes(total_chunks));
    SURS_REQUIRE((reinterpret_cast<size_t>(workspace) & 3) == 0, "surs_tensors_nonfinite: workspace must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const int total = n_items == 0 ? 0 : (int)total_chunks;
    if (total > 0) {
        hipLaunchKernelGGL(nonfinite_chunks_kernel, dim3(total < TN_GRID ? total : TN_GRID), dim3(TN_THREADS), 0, st, items, n_items, total,
                           (int *)workspace);
        SURS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(nonfinite_min_kernel, dim3(1), dim3(TN_THREADS), 0, st, (const int *)workspace, total, result);
    SURS_LAUNCH_CHECK();
    return SURS_OK;
}

extern "C" int surs_tensors_nonfinite_host(const SursTensorRef *items, int n_items, int *result) {
    SURS_REQUIRE(result, "surs_tensors_nonfinite_host: null result");
    long long total = 0;
    const int rc = tensors_check(items, n_items, &total);
    if (rc) return rc;
    *result = -1;
    for (int i = 0; i < n_items; ++i)
        for (long long e = 0; e < items[i].n; ++e)
            if (ts_nonfinite(items[i].p[e])) {
                *result = i;
                return SURS_OK;
            }
    return SURS_OK;
}
