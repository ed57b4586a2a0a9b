// The per-element rules of surs_train_step.hip, __host__ __device__ so that the kernels and their host twins compile the same code
// (as surs_optim_update.h does for the optimiser).
#pragma once
#include "surs_optim_update.h"

namespace surs {

constexpr int TS_CLEAN = 0x7fffffff;   // a chunk without a non-finite value (no table has that many items)

// NaN or +-infinity: an all-ones exponent
SURS_HD inline bool ts_nonfinite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u; }

// d (srweight mean |img_sr - img_hr|) / d img_sr = scale sign(img_sr - img_hr) with scale = srweight / k, formed as torch forms it on
// the device when a tensor is divided by a host scalar (the backward of its mean, and `tensor / numel`): the fp32 reciprocal of k,
// then one fp32 product - (float)w_sr * (1.0f / (float)k).  That is NOT (float)w_sr / (float)k in general: for w_sr = 3, k = 105 the
// two differ in the last bit (measured: 0.02857143059 against 0.02857142873).  Both operations are single IEEE roundings, so host
// and device agree.
SURS_HD inline float ts_l1_scale(float w_sr, long long k) { return k > 0 ? w_sr * (1.0f / (float)k) : 0.0f; }

// sign(d) scale as a product, so that it has torch's bits: scale, -scale, and 0 scale at equality.  A NaN difference stays NaN
// (torch.sign gives 0 there: the one value on which this differs from the torch expression, on purpose - the guard must see it).
SURS_HD inline float ts_l1_grad(float d, float scale) {
    const float s = d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d == d ? 0.0f : d;
    return s * scale;
}

}  // namespace surs
