// Blob layout of SurfaceClassifier pairs of any supported shape (surs_mlp_pack_generic, the fused kernel of surs_mlp_fused.inc).
// The released shape keeps its own layout (surs_mlp_layout.h); this one is built from the runtime shape descriptors
// SursMlpShape (include/surs.h), mirroring lib/model/SurfaceClassifier.py:7-43 and SuRSNet.py:67-78.
//
// Per classifier m (0 = lr, 1 = hr) and layer l, input = [ y (k1 = dims[l] rows) | feature (dims[0] rows, skip layers only) ]:
//   k1pad = dims[l] padded to GEN_KT, k2pad = gen_c0pad(D) for a skip layer (else 0), mpad = dims[l + 1] padded to GEN_KT
//   (the output rows are the next layer's k rows: padding rows come out of the layer as exact zeros);
//   w1  one f16 part                  [kt][tile][lane][8] u16
//   w2  two f16 parts  (hi, lo)       [2][kt][tile][lane][8]
//   w3  three bf16 parts (sum exact)  [3][kt][tile][lane][8]
//   bias fp32 [mpad]
// kt = k step of 32 over [k1pad | k2pad], tile = 16 output rows: the 512 halves of one (kt, tile) are the A fragments of one
// v_mfma_f32_16x16x32_{f16,bf16} in lane order (lane l: row 16 tile + (l & 15), k = 32 kt + 8 (l >> 4) + j), so a wave-wide
// 16-byte load is contiguous. Weights outside the reference tensor are zero.
//
// D = dims_lr[0] - 65 is the encoder's --hg_dim (lib/model/HGFilters.py:166-174): a point's features are [D lr | 64 hr | z] (+ p_lr
// for hr), so the shape itself carries D and the feature segment is gen_c0pad(D) = D + 66 padded to GEN_KT wide: 352 for the
// released D = 256, whose blob is byte for byte what it was when 352 was a constant.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/surs.h"

namespace surs {

constexpr int GEN_MAX_LAYERS = 8;
constexpr int GEN_MAX_WIDTH = 2048;
constexpr int GEN_KT = 32;       // k per MFMA step (16x16x32)
constexpr int GEN_MT = 16;       // output rows per MFMA tile
constexpr int GEN_C_HR = 64;     // channels of the high-resolution feature map (the reference has no flag for them)
constexpr int GEN_D_MIN = 16, GEN_D_MAX = 512, GEN_D_STEP = 16;   // --hg_dim: the cin % 16 rule of the encoder's al{s} .. twice the released width
constexpr int GEN_LDS_BYTES = 160 * 1024;
#define GEN_HG_DIM_RULE "the supported values are the multiples of 16 from 16 to 512"

struct GenLayer {
    int m, mpad, k1, k1pad, k2pad, res;
    unsigned long long w1, w2, w3, bias;   // byte offsets in the blob
};

struct GenLayout {
    int n_layers[2];
    int max_hidden;        // widest padded hidden layer output (the activation rows a tile keeps in LDS), >= GEN_KT
    int hg_dim;            // D = dims_lr[0] - 65: the lr channels of a point's feature vector
    GenLayer layer[2][GEN_MAX_LAYERS];
    unsigned long long total;
};

inline int gen_pad(int v, int a) { return (v + a - 1) / a * a; }

// --hg_dim of a pair: the lr channels of a point's feature vector
inline int gen_hg_dim(const SursMlpShape &lr) { return lr.dims[0] - GEN_C_HR - 1; }
inline bool gen_hg_dim_ok(int D) { return D >= GEN_D_MIN && D <= GEN_D_MAX && D % GEN_D_STEP == 0; }
// feature segment of layer 0 and of a skip layer: [D lr | 64 hr | z | p_lr] padded to the k step
inline int gen_c0pad(int D) { return gen_pad(D + GEN_C_HR + 2, GEN_KT); }
// feature row stride in LDS (floats), see surs_mlp_fused.inc
inline int gen_feat_stride(int D) { return gen_c0pad(D) + 4; }
// The widest padded hidden layer a 16-point tile of the fused evaluators holds in LDS beside `rows` feature rows (1: single view,
// 2: multi-view, which keeps the running sum of the features too) and `extra` bytes of per-point arrays, at most `cap` - the limits
// 2048 / 1824 the released D = 256 has, which every D <= 256 keeps; a larger D leaves less (D = 512: 1920 / 1312).
inline int gen_max_hidden(int D, int rows, int extra, int cap) {
    const int w = ((GEN_LDS_BYTES / 16 - extra) / 4 - 4 - rows * gen_feat_stride(D)) / GEN_KT * GEN_KT;
    return w < cap ? w : cap;
}
inline int gen_max_hidden_single(int D) { return gen_max_hidden(D, 1, 16, GEN_MAX_WIDTH); }

// 0 if the pair is supported, otherwise a negative number naming the violated limit (gen_shape_error's message).
inline int gen_shape_check(const SursMlpShape &s, int m, int D) {
    if (s.n_layers < 1 || s.n_layers > GEN_MAX_LAYERS) return -1;
    if (!gen_hg_dim_ok(D) || s.dims[0] != D + GEN_C_HR + 1 + m) return -2;
    if (s.dims[s.n_layers] != 1) return -3;
    for (int l = 1; l < s.n_layers; ++l) {
        if (s.dims[l] < 1) return -4;
        if (s.dims[l] > gen_max_hidden_single(D)) return gen_max_hidden_single(D) < GEN_MAX_WIDTH ? -6 : -4;
    }
    if (s.res_mask >> s.n_layers) return -5;
    return 0;
}

// the message of gen_shape_check's code for a pair whose lr classifier is `lr` (buf: room for the ones that name numbers)
inline const char *gen_shape_error(int code, const SursMlpShape &lr, char (&buf)[160]) {
    switch (code) {
    case -1: return "number of layers must be between 1 and 8";
    case -2: return "input width must be hg_dim + 65 (lr) / hg_dim + 66 (hr), hg_dim a multiple of 16 from 16 to 512 (321 / 322 for the "
                    "released hg_dim 256)";
    case -3: return "last width must be 1";
    case -4: return "hidden widths must be between 1 and 2048";
    case -5: return "skip layers must be in [0, number of layers)";
    case -6:
        snprintf(buf, sizeof(buf), "hidden widths must be at most %d with hg_dim %d (the LDS of a 16-point tile)",
                 gen_max_hidden_single(gen_hg_dim(lr)), gen_hg_dim(lr));
        return buf;
    default: return "unsupported shape";
    }
}

// Fills `out` for a supported pair; returns 0, or gen_shape_check's code of the first classifier that is not supported.
inline int gen_layout(const SursMlpShape &lr, const SursMlpShape &hr, GenLayout &out) {
    memset(&out, 0, sizeof(out));
    const SursMlpShape *s[2] = {&lr, &hr};
    const int D = gen_hg_dim(lr);
    unsigned long long off = 256;   // (room for a copy of the layout's first bytes; offsets stay 256-byte aligned)
    out.max_hidden = GEN_KT;
    out.hg_dim = D;
    for (int m = 0; m < 2; ++m) {
        const int rc = gen_shape_check(*s[m], m, D);
        if (rc) return rc;
        out.n_layers[m] = s[m]->n_layers;
        for (int l = 0; l < s[m]->n_layers; ++l) {
            GenLayer &g = out.layer[m][l];
            g.res = (s[m]->res_mask >> l) & 1u;
            g.m = s[m]->dims[l + 1];
            g.mpad = gen_pad(g.m, GEN_KT);
            g.k1 = s[m]->dims[l];
            g.k1pad = gen_pad(g.k1, GEN_KT);
            g.k2pad = g.res ? gen_c0pad(D) : 0;
            const unsigned long long halves = (unsigned long long)(g.k1pad + g.k2pad) * g.mpad;
            g.w1 = off;
            off += (halves * 2 + 255) / 256 * 256;
            g.w2 = off;
            off += (halves * 4 + 255) / 256 * 256;
            g.w3 = off;
            off += (halves * 6 + 255) / 256 * 256;
            g.bias = off;
            off += ((unsigned long long)g.mpad * 4 + 255) / 256 * 256;
            if (l + 1 < s[m]->n_layers && g.mpad > out.max_hidden) out.max_hidden = g.mpad;
        }
    }
    out.total = off;
    return 0;
}

// Index (in halves, inside one part) of weight (row o, input k of the concatenated [k1pad | k2pad] input) in the A-fragment image.
inline size_t gen_frag_index(const GenLayer &g, int o, int k) {
    const int kt = k / GEN_KT, kk = k % GEN_KT, tile = o / GEN_MT;
    const int lane = (o % GEN_MT) + 16 * (kk / 8);
    return (((size_t)kt * (g.mpad / GEN_MT) + tile) * 64 + lane) * 8 + (kk % 8);
}

}  // namespace surs
