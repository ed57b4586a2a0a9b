// The four optimisers of the reference's training script (apps/train_SuRS.py:54-72: SGD, ADAM, AMSgrad, RMSprop) as ONE-ELEMENT
// updates on fp32 values, in the order of operations of torch.optim's single-tensor path (torch/optim/{sgd,adam,rmsprop}.py, the
// branch that is neither capturable nor differentiable): the kernel of surs_optim.hip calls them with one lane per element (four
// per 16-byte access), surs_optim_step_host loops them on the host.  __host__ __device__, so both compile the same arithmetic; the
// library builds with -ffp-contract=off and fp32 division and square root are correctly rounded on both sides, so every operation
// below is one IEEE rounding and host and device give the same bits.  The fused multiply-adds are EXPLICIT (ou_fma), and stand where
// torch's own CPU kernels fuse: the closing product and sum of add(alpha), lerp and addcmul (p + (-lr) g, g + wd p, m + w (g - m),
// beta2 v + ((1 - beta2) g) g) are one rounding there; mul_().add_() and addcdiv are not.  With them the fp32 results are torch's
// fp32 results on the CPU but for its vectorised square root.  No powers here: the step-dependent scalars of SursOptimHyper
// (step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), the complements 1 - beta) are formed on the host in double.
#pragma once
#include "../../include/surs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SURS_HD __host__ __device__
#else
#define SURS_HD
#endif

namespace surs {

// state tensors a kind reads and writes (s0..): SGD buf (none without momentum) | ADAM m, v | AMSgrad m, v, vmax | RMSprop sq; -1: unknown
SURS_HD inline int ou_states(int kind, float momentum) {
    return kind == SURS_OPTIM_SGD ? (momentum != 0.0f ? 1 : 0) : kind == SURS_OPTIM_ADAM ? 2 : kind == SURS_OPTIM_AMSGRAD ? 3
         : kind == SURS_OPTIM_RMSPROP ? 1 : -1;
}

SURS_HD inline float ou_sqrt(float x) { return __builtin_sqrtf(x); }
SURS_HD inline float ou_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }   // a b + c, one rounding

// L2 weight decay in the gradient (grad.add(param, alpha=weight_decay); not AdamW's).  Skipped at 0, as torch skips it: 0 * inf
// would otherwise make a NaN of an infinite parameter's gradient.
SURS_HD inline float ou_decay(float g, float p, const SursOptimHyper &h) { return h.weight_decay != 0.0f ? ou_fma(h.weight_decay, p, g) : g; }

// dampening 0, no Nesterov.  buf is touched only with momentum != 0: buf = g' on the optimiser's first step (torch clones the
// gradient into an absent buffer), buf = momentum buf + g' afterwards.
SURS_HD inline void ou_sgd(float &p, float g, float &buf, const SursOptimHyper &h) {
    g = ou_decay(g, p, h);
    if (h.momentum != 0.0f) {
        buf = h.first_step ? g : buf * h.momentum + g;
        g = buf;
    }
    p = ou_fma(-h.lr, g, p);
}

// torch.maximum: a NaN on either side gives NaN (fmaxf would drop it)
SURS_HD inline float ou_max(float a, float b) { return (b > a || b != b) ? b : a; }

// exp_avg.lerp_(g', 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(g', g', value=1 - beta2); denom = sqrt(v) / bc2_sqrt + eps (eps outside
// the root); p.addcdiv_(m, denom, value=-step_size) = p - (step_size m) / denom.  AMSGRAD: vmax = maximum(vmax, v), denom from vmax.
template <bool AMSGRAD>
SURS_HD inline void ou_adam(float &p, float g, float &m, float &v, float &vmax, const SursOptimHyper &h) {
    g = ou_decay(g, p, h);
    m = ou_fma(h.beta1_c, g - m, m);
    v = ou_fma(h.beta2_c * g, g, v * h.beta2);
    float root = v;
    if (AMSGRAD) root = vmax = ou_max(vmax, v);
    const float denom = ou_sqrt(root) / h.bc2_sqrt + h.eps;
    p = p - (h.step_size * m) / denom;
}

// momentum 0, not centred: square_avg.mul_(alpha).addcmul_(g', g', value=1 - alpha); p.addcdiv_(g', sqrt(sq) + eps, value=-lr)
SURS_HD inline void ou_rmsprop(float &p, float g, float &sq, const SursOptimHyper &h) {
    g = ou_decay(g, p, h);
    sq = ou_fma(h.alpha_c * g, g, sq * h.alpha);
    p = p - (h.lr * g) / (ou_sqrt(sq) + h.eps);
}

// one element of any kind: s0, s1, s2 as ou_states counts them (the others are neither read nor written)
template <int KIND>
SURS_HD inline void ou_update(float &p, float g, float &s0, float &s1, float &s2, const SursOptimHyper &h) {
    if (KIND == SURS_OPTIM_SGD) ou_sgd(p, g, s0, h);
    else if (KIND == SURS_OPTIM_ADAM) ou_adam<false>(p, g, s0, s1, s2, h);
    else if (KIND == SURS_OPTIM_AMSGRAD) ou_adam<true>(p, g, s0, s1, s2, h);
    else ou_rmsprop(p, g, s0, h);
}

// The gradient a data-parallel step applies (surs_optim_step_ranks): rank r's value lies r * stride values of T behind rank 0's, and
// the result is ((g_0 + g_1) + ... + g_{R-1}) * scale - fp32 sums left to right STARTING FROM g_0 (0 + g_0 would turn a -0 into +0),
// then one fp32 product, skipped at scale == 1 - so that R == 1, scale == 1 returns g_0's bits untouched.  T is float, or the
// kernel's four-float vector (the same sums per component); P the pointer's value type (an address-space-qualified one on the
// device).  The loads of OU_RANK_UNROLL ranks are issued before the first of their adds: independent loads in flight, where one
// load per add would pay a memory latency per rank.  The order of the adds does not depend on the unroll.
constexpr int OU_RANK_UNROLL = 8;
constexpr int OU_MAX_RANKS = 64;

template <typename T, typename P>
SURS_HD inline T ou_rank_sum(const P *g, long long stride, int R, float scale) {
    T v[OU_RANK_UNROLL];
    T acc = g[0];
    for (int r0 = 0; r0 < R; r0 += OU_RANK_UNROLL) {
        const int c = R - r0 < OU_RANK_UNROLL ? R - r0 : OU_RANK_UNROLL;
#pragma unroll
        for (int j = 0; j < OU_RANK_UNROLL; ++j)
            if (j < c && r0 + j > 0) v[j] = g[(long long)(r0 + j) * stride];
#pragma unroll
        for (int j = 0; j < OU_RANK_UNROLL; ++j)
            if (j < c && r0 + j > 0) acc = acc + v[j];
    }
    if (scale != 1.0f) acc = acc * scale;
    return acc;
}

// elements per workgroup visit: 256 lanes x 4 floats x 4 rounds
constexpr int OU_CHUNK = 4096;
SURS_HD inline int ou_chunks(long long n) { return n <= 0 ? 0 : (int)((n + OU_CHUNK - 1) / OU_CHUNK); }

}  // namespace surs
