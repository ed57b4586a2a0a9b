// The host packers of surs_pack.cpp restated in GATHER form: every loop there is a bijection from source to destination, so each
// destination element names its one source (or is padding, zero).  The functions below write ONE destination element (with its
// split parts) from its index; the kernels of surs_repack.hip call them with one lane per element.  __host__ __device__, so the same
// arithmetic can be held against surs_mlp_pack / surs_mlp_pack_generic on the host, element by element.
#pragma once
#include <cstddef>
#include <cstdint>

#include "surs_mlp_generic.h"
#include "surs_mlp_layout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SURS_HD __host__ __device__
#else
#define SURS_HD
#endif

namespace surs {

// ---- roundings and splits: those of surs_pack.cpp
SURS_HD inline uint16_t rp_bf16(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
SURS_HD inline float rp_bf16_f32(uint16_t h) {
    const uint32_t v = (uint32_t)h << 16;
    float f;
    __builtin_memcpy(&f, &v, 4);
    return f;
}
SURS_HD inline uint16_t rp_f16(float f) {
    const _Float16 h = (_Float16)f;   // round to nearest even, subnormal results kept
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}
SURS_HD inline float rp_f16_f32(uint16_t u) {
    _Float16 h;
    __builtin_memcpy(&h, &u, 2);
    return (float)h;
}
SURS_HD inline void rp_split2(float w, uint16_t &hi, uint16_t &lo) {
    hi = rp_f16(w);
    lo = rp_f16(w - rp_f16_f32(hi));
}
SURS_HD inline void rp_split3(float w, uint16_t (&p)[3]) {
    float rest = w;
    for (int part = 0; part < 3; ++part) {
        p[part] = rp_bf16(rest);
        rest -= rp_bf16_f32(p[part]);
    }
}
SURS_HD inline uint16_t rp_cvt(int dtype, float f) { return dtype == SURS_F16 ? rp_f16(f) : rp_bf16(f); }

// ---- released shape (surs_mlp_layout.h)
struct MlpSrc {
    const float *const *W[2];   // per classifier: table of the five Conv1d weights [out][in]
    const float *const *B[2];   // and biases [out]
};

SURS_HD inline int rp_ymain(int l) { return l == 1 ? D1 : l == 2 ? D2 : l == 3 ? D3 : l == 4 ? D4 : 0; }
SURS_HD inline int rp_kin(int m, int l) { return l == 1 ? D1 : rp_ymain(l) + 321 + m; }   // Conv1d in_channels
SURS_HD inline int rp_mout(int l) { return l == 0 ? D1 : l == 1 ? D2 : l == 2 ? D3 : l == 3 ? D4 : 1; }
SURS_HD inline int rp_kpad(int l) { return l == 0 ? C0PAD : l == 1 ? D1 : l == 2 ? D2 + C0PAD : D3 + C0PAD; }

// wt[m][l][k][o]
SURS_HD inline float rp_wt(const MlpSrc &s, int m, int l, int k, int o) {
    const int kin = rp_kin(m, l);
    return k < kin ? s.W[m][l][(size_t)o * kin + k] : 0.0f;
}

// column cc of the column-constant matrix: (classifier, layer, row of that layer, first gathered column); false: padding
SURS_HD inline bool rp_cc(int cc, int &m, int &l, int &row, int &col0) {
    if (cc < CC_A2_LR) { m = cc >= CC_A0_HR; l = 0; row = cc - (m ? CC_A0_HR : CC_A0_LR); col0 = 0; return true; }
    if (cc < CC_A3_LR) { m = cc >= CC_A2_HR; l = 2; row = cc - (m ? CC_A2_HR : CC_A2_LR); col0 = D2; return true; }
    if (cc < CC_A4_LR) { m = cc >= CC_A3_HR; l = 3; row = cc - (m ? CC_A3_HR : CC_A3_LR); col0 = D3; return true; }
    if (cc < CC_N) { m = cc - CC_A4_LR; l = 4; row = 0; col0 = D4; return true; }
    return false;
}
SURS_HD inline float rp_wc(const MlpSrc &s, int k, int cc) {
    int m, l, row, col0;
    if (!rp_cc(cc, m, l, row, col0)) return 0.0f;
    return s.W[m][l][(size_t)row * rp_kin(m, l) + col0 + k];
}
SURS_HD inline float rp_bc(const MlpSrc &s, int cc) {
    int m, l, row, col0;
    if (!rp_cc(cc, m, l, row, col0)) return 0.0f;
    return s.B[m][l][row];
}

SURS_HD inline float rp_zvec(const MlpSrc &s, int i) {
    auto wz = [&](int m, int l, int o, int col) { return s.W[m][l][(size_t)o * rp_kin(m, l) + rp_ymain(l) + col]; };
    if (i < ZV_W0Z_HR) return wz(0, 0, i - ZV_W0Z_LR, 320);
    if (i < ZV_W0P_HR) return wz(1, 0, i - ZV_W0Z_HR, 320);
    if (i < ZV_B1_LR) return wz(1, 0, i - ZV_W0P_HR, 321);
    if (i < ZV_B1_HR) return s.B[0][1][i - ZV_B1_LR];
    if (i < ZV_W2Z_LR) return s.B[1][1][i - ZV_B1_HR];
    if (i < ZV_W2Z_HR) return wz(0, 2, i - ZV_W2Z_LR, 320);
    if (i < ZV_W2P_HR) return wz(1, 2, i - ZV_W2Z_HR, 320);
    if (i < ZV_W3Z_LR) return wz(1, 2, i - ZV_W2P_HR, 321);
    if (i < ZV_W3Z_HR) return wz(0, 3, i - ZV_W3Z_LR, 320);
    if (i < ZV_W3P_HR) return wz(1, 3, i - ZV_W3Z_HR, 320);
    if (i < ZV_W4C_LR) return wz(1, 3, i - ZV_W3P_HR, 321);
    if (i < ZV_W4C_HR) return s.W[0][4][i - ZV_W4C_LR];
    if (i < ZV_W4Z_LR) return s.W[1][4][i - ZV_W4C_HR];
    if (i == ZV_W4Z_LR) return wz(0, 4, 0, 320);
    if (i == ZV_W4Z_HR) return wz(1, 4, 0, 320);
    if (i == ZV_W4P_HR) return wz(1, 4, 0, 321);
    return 0.0f;
}

// The small fp32 sections, y = 0..7: bias[m][l] (y = 4 m + l); 8, 9: w4[m]; 10: bc; 11: zvec; 12: b1frag (16-bit).  Returns false
// beyond the section's end.
constexpr int RP_SMALL_SECTIONS = 13, RP_SMALL_MAX = 2 * (D2 / 32) * 512;
SURS_HD inline bool rp_small_elem(const MlpSrc &s, const MlpBlobHeader &h, char *base, int dtype, int y, uint32_t i) {
    if (y < 8) {
        const int m = y >> 2, l = y & 3;
        if (i >= (uint32_t)rp_mout(l)) return false;
        ((float *)(base + h.bias[m][l]))[i] = s.B[m][l][i];
    } else if (y < 10) {
        const int m = y - 8;
        if (i >= (uint32_t)(D4 + C0PAD + 1)) return false;
        ((float *)(base + h.w4[m]))[i] = i < (uint32_t)(D4 + 321 + m) ? s.W[m][4][i] : i == (uint32_t)(D4 + C0PAD) ? s.B[m][4][0] : 0.0f;
    } else if (y == 10) {
        if (i >= (uint32_t)CC_PAD) return false;
        ((float *)(base + h.bc))[i] = rp_bc(s, (int)i);
    } else if (y == 11) {
        if (i >= (uint32_t)ZV_N) return false;
        ((float *)(base + h.zvec))[i] = rp_zvec(s, (int)i);
    } else {
        // layer-1 biases as A fragments [2][D2 / 32][64 lanes][8]: three exact 16-bit parts in k-slots 0..2 of lanes 0..31.  The
        // remainders follow a multiplication: no fma (the library builds with -ffp-contract=off)
        if (i >= (uint32_t)RP_SMALL_MAX) return false;
        const int j = i & 7, lane = (i >> 3) & 63, T = (i >> 9) % (D2 / 32), m = (i >> 9) / (D2 / 32);
        uint16_t out = 0;
        if (lane < 32 && j < 3) {
            float rest = s.B[m][1][32 * T + lane] * (dtype == SURS_F16 ? B1FRAG_SCALE_F16 : B1FRAG_SCALE_BF16);
            for (int part = 0;; ++part) {
                out = rp_cvt(dtype, rest);
                if (part == j) break;
                rest -= dtype == SURS_F16 ? rp_f16_f32(out) : rp_bf16_f32(out);
            }
        }
        ((uint16_t *)(base + h.b1frag))[i] = out;
    }
    return true;
}

// The k-major matrices: y = 4 m + l: wt[m][l] [kpad][M], 8: wc [C_G][CC_PAD]; element i = k M + o (fp32) and the same value's two f16 /
// three bf16 parts at the A-fragment index [k / 16][o / 32][(k >> 3) & 1][o & 31][k & 7] of wt2 / wt3 (wc2 / wc3).
constexpr int RP_KMAJOR_SECTIONS = 9;
SURS_HD inline void rp_kmajor_shape(int y, int &kpad, int &M) {
    kpad = y < 8 ? rp_kpad(y & 3) : C_G;
    M = y < 8 ? rp_mout(y & 3) : CC_PAD;
}
SURS_HD inline bool rp_kmajor_elem(const MlpSrc &s, const MlpBlobHeader &h, char *base, int y, uint32_t i) {
    int kpad, M;
    rp_kmajor_shape(y, kpad, M);
    if (i >= (uint32_t)kpad * M) return false;
    const int k = i / M, o = i % M, m = (y >> 2) & 1, l = y & 3;
    const float w = y < 8 ? rp_wt(s, m, l, k, o) : rp_wc(s, k, o);
    ((float *)(base + (y < 8 ? h.wt[m][l] : h.wc)))[i] = w;
    const size_t per_part = (size_t)kpad * M;
    const size_t idx = ((((size_t)(k / 16) * (M / 32) + o / 32) * 2 + ((k >> 3) & 1)) * 32 + (o & 31)) * 8 + (k & 7);
    uint16_t *o2 = (uint16_t *)(base + (y < 8 ? h.wt2[m][l] : h.wc2)), *o3 = (uint16_t *)(base + (y < 8 ? h.wt3[m][l] : h.wc3));
    rp_split2(w, o2[idx], o2[per_part + idx]);
    uint16_t u[3];
    rp_split3(w, u);
    for (int part = 0; part < 3; ++part) o3[part * per_part + idx] = u[part];
    return true;
}

// The dense cores of one classifier: element i of its `core` image (layers 1..3 in a row, [k-step][row tile][64 lanes][8]) also names
// the two parts of `corex` (the same k order, [k-step][row tile][part][lane][8]) and one element of `core16` (the 16x16x32 shape).
constexpr uint32_t RP_CORE_HALVES = (uint32_t)SLABS_PER_MLP * (SLAB_BYTES / 2);
SURS_HD inline bool rp_core_elem(const MlpSrc &s, const MlpBlobHeader &h, char *base, int dtype, int m, uint32_t i) {
    if (i >= RP_CORE_HALVES) return false;
    const uint32_t l1 = (uint32_t)SLABS_L1 * (SLAB_BYTES / 2), l2 = l1 + (uint32_t)SLABS_L2 * (SLAB_BYTES / 2);
    const int L = i < l1 ? 0 : i < l2 ? 1 : 2;                 // layer L + 1
    const uint32_t first = L == 0 ? 0 : L == 1 ? l1 : l2, rem = i - first;
    const int rows = rp_mout(L + 1), ld = rp_kin(m, L + 1);
    const int j = rem & 7, lane = (rem >> 3) & 63, frag = rem >> 9;
    const float *W = s.W[m][L + 1];
    {   // 32x32x16: L1 natural k order inside a k-step, L2 / L3 the k order of an accumulator tile reused as B operand
        const int nT = rows / 32, st = frag / nT, T = frag % nT, r = lane & 31, hh = lane >> 5;
        const int k = L == 0 ? 16 * st + 8 * hh + j : 16 * st + 8 * (j >> 2) + 4 * hh + (j & 3);
        const float w = W[(size_t)(32 * T + r) * ld + k];
        ((uint16_t *)(base + h.core))[(size_t)m * RP_CORE_HALVES + i] = rp_cvt(dtype, w);
        uint16_t *cx = (uint16_t *)(base + h.corex) + (size_t)m * X_F_MLP * 512 + (size_t)first * 2;
        rp_split2(w, cx[((size_t)frag * 2 * 64 + lane) * 8 + j], cx[(((size_t)frag * 2 + 1) * 64 + lane) * 8 + j]);
    }
    {   // 16x16x32
        const int nT = rows / 16, st = frag / nT, T = frag % nT, n = lane & 15, q = lane >> 4;
        const int k = L == 0 ? 32 * st + 8 * q + j : 32 * st + 16 * (j >> 2) + 4 * q + (j & 3);
        ((uint16_t *)(base + h.core16))[(size_t)m * RP_CORE_HALVES + i] = rp_cvt(dtype, W[(size_t)(16 * T + n) * ld + k]);
    }
    return true;
}

// Layer-1 weights channel-major: element i = (m D1 + c) D2 + r of w1t, and the two f16 parts of w1tx [m][c][part][r].
SURS_HD inline bool rp_w1t_elem(const MlpSrc &s, const MlpBlobHeader &h, char *base, int dtype, uint32_t i) {
    if (i >= (uint32_t)2 * D1 * D2) return false;
    const int r = i % D2, c = (i / D2) % D1, m = i / (D1 * D2);
    const float w = s.W[m][1][(size_t)r * D1 + c];
    ((uint16_t *)(base + h.w1t))[i] = rp_cvt(dtype, w);
    uint16_t *wx = (uint16_t *)(base + h.w1tx);
    rp_split2(w, wx[(((size_t)m * D1 + c) * 2) * D2 + r], wx[(((size_t)m * D1 + c) * 2 + 1) * D2 + r]);
    return true;
}

// ---- any supported shape (surs_mlp_generic.h): element i of one part of layer g's A-fragment image - the inverse of gen_frag_index
// - and, for i < mpad, the bias.  W: the layer's Conv1d weight [m][k1 (+ c0)], c0 = dims[0].
SURS_HD inline bool rp_generic_elem(const GenLayer &g, int c0, const float *W, const float *B, char *base, uint32_t i) {
    const size_t per_part = (size_t)(g.k1pad + g.k2pad) * g.mpad;
    if (i >= per_part) return false;
    const int j = i & 7, lane = (i >> 3) & 63, nT = g.mpad / GEN_MT, tile = (i >> 9) % nT, kt = (i >> 9) / nT;
    const int o = tile * GEN_MT + (lane & 15), k = kt * GEN_KT + 8 * (lane >> 4) + j;
    const int kin = g.k1 + (g.res ? c0 : 0);
    float w = 0.0f;
    if (o < g.m) {
        if (k < g.k1) w = W[(size_t)o * kin + k];
        else if (g.res && k >= g.k1pad && k - g.k1pad < c0) w = W[(size_t)o * kin + g.k1 + (k - g.k1pad)];
    }
    uint16_t *w1 = (uint16_t *)(base + g.w1), *w2 = (uint16_t *)(base + g.w2), *w3 = (uint16_t *)(base + g.w3);
    w1[i] = rp_f16(w);
    rp_split2(w, w2[i], w2[per_part + i]);
    uint16_t u[3];
    rp_split3(w, u);
    for (int part = 0; part < 3; ++part) w3[part * per_part + i] = u[part];
    if (i < (uint32_t)g.mpad) ((float *)(base + g.bias))[i] = i < (uint32_t)g.m ? B[i] : 0.0f;
    return true;
}

}  // namespace surs
