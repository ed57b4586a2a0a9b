// The image encoder sequenced in C: surs_encoder_super_res / _filter_lr / _filter_hr / _forward (include/surs.h).
//
// Replaces, as ONE call each, what the reference runs as nn.Module graphs:
//   SuRSSR_v3.forward          lib/model/SuRSSR_v3.py:143-181   (ResBlock: lib/model/common.py:14-33)
//   HGFilter.forward low_res   lib/model/HGFilters.py:183-206   (ConvBlock :57-74, HourGlass :96-117)
//   HGFilter.forward high_res  lib/model/HGFilters.py:179-181
// Until round 6 the ~ 160 launches of an image were issued one by one from Python through ctypes (encoder.py, kept as the
// readable mirror and as the path of the non-default operand splits); a C-ABI consumer had to re-implement that sequencing.
// Here it is native: the same launches in the same order on the same tiles - the outputs equal encoder.py's bit for bit
// (tests/test_gpu_encoder_net.py) -, intermediates in a caller-supplied workspace, no allocation, no stream creation (the side
// streams of the hourglass fork are lent by the caller; without them the branches run one behind the other).
//
// Memory plan: a bump allocator over the workspace.  The super-resolution net reuses three buffers per stage for its residual
// blocks (one stream: reuse is ordered); filter_lr alternates between two arenas per stack (stack s + 2 starts after every
// kernel of stack s has been joined).  surs_encoder_workspace_bytes() runs the same sequencing with a counting allocator.
//
// ONE sequencing per network.  super_res() (over a plan of buffers), conv_block(), hourglass() and stack_tail() (with an optional
// tape) are the only launch lists of their networks: the inference calls, the train forwards of the gradient entry points further down and - run
// without launches - every size query and the backwards' address computation all go through them.  The layout of a tape is the
// order of the allocator's takes of that sequencing; the backwards walk the same plan / the same level table in reverse.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "surs_common.h"

using namespace surs;

namespace {

struct Map {   // NHWC fp32 view with channel pitch + the GroupNorm(32) statistics its producer(s) left (st.sums null: none)
    float *p = nullptr;
    int h = 0, w = 0, c = 0, ld = 0;
    SursGnStats st = {nullptr, 0, 0, 0, {0, 0, 0}};
    void set_stats(double *sums, int slots) { st = SursGnStats{sums, slots, 0, 0, {slots, slots, slots}}; }
    Map slice(int c0, int n) const { Map m = *this; m.p = p + c0; m.c = n; m.set_stats(nullptr, 0); return m; }
};

// a map over memory the arena did not hand out: a caller's buffer, or a view of another size into a shared one
Map input_map(const float *x, int h, int w, int c, int ld) {
    Map m;
    m.p = const_cast<float *>(x); m.h = h; m.w = w; m.c = c; m.ld = ld;
    return m;
}

struct Arena {
    char *base = nullptr;
    size_t off = 0, cap = 0, peak = 0;
    bool dry = false;
    void *take(size_t bytes) {
        off = align_up(off, 256);
        void *r = (dry ? reinterpret_cast<char *>(4096) : base) + off;   // (a dry run hands out addresses nobody dereferences)
        off += bytes;
        if (off > peak) peak = off;
        return r;
    }
    bool ok() const { return dry || off <= cap; }
};

struct Run {
    const SursEncoderNet *net;
    Arena *a;            // current arena
    hipStream_t st;      // current stream
    int parts;           // 2 (fp32-grade) or 1 (one f16 product per MAC in the 3x3 convolutions)
    bool dry;
    int rc = 0;
    // --norm batch: every norm site is y = x * scale + shift with constant coefficients (SursEncoderNet.bn_*): no map carries
    // statistics, no kernel computes any
    bool bn() const { return (net->flags & SURS_ENC_EXTENDED) && net->norm == SURS_NORM_BATCH; }

    Map map(int h, int w, int c) {
        Map m;
        m.h = h; m.w = w; m.c = c; m.ld = c;
        m.p = (float *)a->take((size_t)h * w * c * sizeof(float));
        return m;
    }
    double *stats_buf(int capacity) { return (double *)a->take((size_t)32 * capacity * 2 * sizeof(double)); }
    bool fail(int code) {
        if (code && !rc) rc = code;
        return rc != 0;
    }
};

struct Dry {   // a run without launches over a counting arena of its own: sizes, and the addresses of a layout
    Arena a;
    Run r;
    explicit Dry(const SursEncoderNet *net) : r{net, &a, nullptr, net->parts, true} { a.dry = true; }
    Dry(const Dry &) = delete;
};

Arena tape_arena(const void *tape, size_t bytes) {   // (a tape is 256-byte aligned: the entry points check)
    Arena a;
    a.base = (char *)const_cast<void *>(tape);
    a.cap = bytes;
    return a;
}

// a: the caller's workspace from its first 256-byte boundary on; false: fewer than `need` bytes are left behind it
bool workspace_arena(void *workspace, size_t workspace_bytes, size_t need, Arena &a) {
    a.base = (char *)align_up((size_t)workspace, 256);
    const size_t lead = (size_t)(a.base - (char *)workspace);
    if (need + lead > workspace_bytes) return false;
    a.cap = workspace_bytes - lead;
    return true;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// --scale: the bicubic enlargement in front of the super-resolution net (2 for callers without the extended fields)
inline int sr_scale(const SursEncoderNet *n) { return ((n->flags & SURS_ENC_EXTENDED) && n->sr_scale) ? n->sr_scale : 2; }
inline int per_stack_blocks(const SursEncoderNet *n) { return 3 * n->hg_depth + 1; }

// native.conv2d of encoder.py: the split-f16 kernels where they apply, the fp32 MFMA / direct kernels otherwise
void conv(Run &r, const Map &x, const SursConv &cw, Map &out, int stride, int act, float slope, const Map *residual,
          const float *in_scale = nullptr, const float *in_shift = nullptr) {
    out.set_stats(nullptr, 0);
    if (r.dry || r.rc) return;
    const bool thin = cw.ksize == 3 && stride == 1 && !in_scale && cw.cout <= 4 && cw.cin == 32;
    const bool x3 = cw.w_split && !thin && (stride == 1 || (stride == 2 && cw.ksize == 3)) && x.c % 16 == 0 && x.ld % 4 == 0 && aligned16(x.p);
    const float *res = residual ? residual->p : nullptr;
    const int res_ld = residual ? residual->ld : 0;
    int rc;
    if (x3 && r.parts == 1 && cw.ksize == 3)
        rc = surs_conv2d_nhwc_x1(x.p, x.h, x.w, x.c, x.ld, cw.w_split, cw.bias, out.p, cw.cout, out.ld, cw.ksize, stride, in_scale, in_shift,
                                 act, slope, res, res_ld, r.st);
    else if (x3)
        rc = surs_conv2d_nhwc_x2(x.p, x.h, x.w, x.c, x.ld, cw.w_split, cw.bias, out.p, cw.cout, out.ld, cw.ksize, stride, in_scale, in_shift,
                                 act, slope, res, res_ld, r.st);
    else
        rc = surs_conv2d_nhwc(x.p, x.h, x.w, x.c, x.ld, cw.w_packed, cw.bias, out.p, cw.cout, out.ld, cw.ksize, stride, in_scale, in_shift,
                              act, slope, res, res_ld, r.st);
    r.fail(rc);
}

// native.conv2d_gn: stride 1, GroupNorm(32) statistics handed from kernel to kernel (x's: one slot count for all groups)
void conv_gn(Run &r, const Map &x, const SursConv &cw, Map &out, const SursGroupNorm *gn, bool want_stats, const Map *residual = nullptr) {
    const int cap = cw.ksize == 1 ? (out.h * out.w + 127) / 128 : ((out.w + 31) / 32) * ((out.h + 3) / 4);
    double *sb = want_stats ? r.stats_buf(cap) : nullptr;
    out.set_stats(sb, 0);
    if (r.dry || r.rc) return;
    if (gn && (!x.st.sums || x.st.g1 > 0)) {
        r.fail(fail(SURS_E_INVALID, "encoder: a GroupNorm input carries no (single-kernel) statistics"));
        return;
    }
    int slots = 0;
    const int rc = surs_conv2d_nhwc_gn(r.parts, x.p, x.h, x.w, x.c, x.ld, cw.w_split, cw.bias, out.p, cw.cout, out.ld, cw.ksize, 1,
                                       gn ? x.st.sums : nullptr, gn ? x.st.slots[0] : 0, gn ? gn->gamma : nullptr, gn ? gn->beta : nullptr,
                                       1e-5f, 0, 0.0f, residual ? residual->p : nullptr, residual ? residual->ld : 0, sb, cap, &slots, r.st);
    if (r.fail(rc)) return;
    out.set_stats(sb, sb ? slots : 0);
}

inline int ew_capacity(long long items) {
    const long long n = (items + 1023) / 1024;
    return (int)(n < 512 ? n : 512);
}

void add3(Run &r, const Map &a, const Map &b, Map &out, bool want_stats) {
    const int cap = ew_capacity((long long)a.h * a.w * (a.c / 4));
    double *sb = want_stats ? r.stats_buf(cap) : nullptr;
    out.set_stats(sb, 0);
    if (r.dry || r.rc) return;
    int slots = 0;
    const int rc = want_stats ? surs_add3_gn(a.p, a.ld, b.p, b.ld, nullptr, 0, a.h * a.w, a.c, out.p, out.ld, sb, cap, &slots, r.st)
                              : surs_add3(a.p, a.ld, b.p, b.ld, nullptr, 0, a.h * a.w, a.c, out.p, out.ld, r.st);
    if (r.fail(rc)) return;
    out.set_stats(sb, slots);
}

Map avgpool2(Run &r, const Map &x, bool want_stats) {
    Map out = r.map(x.h / 2, x.w / 2, x.c);
    const int cap = ew_capacity((long long)out.h * out.w * (x.c / 4));
    double *sb = want_stats ? r.stats_buf(cap) : nullptr;
    out.set_stats(sb, 0);
    if (r.dry || r.rc) return out;
    int slots = 0;
    const int rc = want_stats ? surs_avgpool2_gn(x.p, x.h, x.w, x.c, x.ld, out.p, out.ld, sb, cap, &slots, r.st)
                              : surs_avgpool2(x.p, x.h, x.w, x.c, x.ld, out.p, out.ld, r.st);
    if (r.fail(rc)) return out;
    out.set_stats(sb, slots);
    return out;
}

void bicubic_up2(Run &r, const Map &x, bool align_corners, const Map *addend, Map &out, bool want_stats) {
    const int cap = ew_capacity((long long)out.h * out.w * (x.c / 4));
    double *sb = want_stats ? r.stats_buf(cap) : nullptr;
    out.set_stats(sb, 0);
    if (r.dry || r.rc) return;
    int slots = 0;
    const float *ad = addend ? addend->p : nullptr;
    const int ad_ld = addend ? addend->ld : 0;
    const int rc = want_stats ? surs_bicubic_up2_gn(x.p, x.h, x.w, x.c, x.ld, align_corners, ad, ad_ld, out.p, out.ld, sb, cap, &slots, r.st)
                              : surs_bicubic_up2(x.p, x.h, x.w, x.c, x.ld, align_corners, ad, ad_ld, out.p, out.ld, r.st);
    if (r.fail(rc)) return;
    out.set_stats(sb, slots);
}

// the statistics-free 2 x 2-block form (a BatchNorm hourglass's up1 + up2)
void bicubic_up2_block(Run &r, const Map &x, bool align_corners, const Map *addend, Map &out) {
    out.set_stats(nullptr, 0);
    if (r.dry || r.rc) return;
    r.fail(surs_bicubic_up2_block(x.p, x.h, x.w, x.c, x.ld, align_corners, addend ? addend->p : nullptr, addend ? addend->ld : 0, out.p, out.ld, r.st));
}

void bicubic_up(Run &r, const Map &x, int scale, Map &out) {
    out.set_stats(nullptr, 0);
    if (r.dry || r.rc) return;
    r.fail(surs_bicubic_up(x.p, x.h, x.w, x.c, x.ld, scale, 0, nullptr, 0, out.p, out.ld, r.st));
}

void pixel_shuffle2(Run &r, const Map &x, float slope, Map &out) {
    out.set_stats(nullptr, 0);
    if (r.dry || r.rc) return;
    r.fail(surs_pixel_shuffle2(x.p, x.h, x.w, x.c, x.ld, slope, out.p, out.ld, r.st));
}

constexpr int ACT = 1;
constexpr float LRELU = 0.2f, RELU = 0.0f;

// ---------------------------------------------------------------- SuRSSR_v3.forward (lib/model/SuRSSR_v3.py:143-181)
// ONE sequencing, super_res(), over a plan of buffers.  The inference plan keeps what nothing reads again in shared storage; the
// tape plan gives every layer a buffer of its own, for surs_encoder_super_res_backward to read.
struct SrStage {   // a stride-2 stage's maps in the order it writes them, all h x w x c
    int h, w, c, nb;   // nb: the residual blocks that run
    float *buf[2 * 64 + 2];
    Map at(int j) const { return input_map(buf[j], h, w, c, c); }
    Map a(int b) const { return at(2 * b); }        // a(0): down's output, a(b + 1): block b's output
    Map t(int b) const { return at(2 * b + 1); }    // block b's inner map (ReLU)
    Map u() const { return at(2 * nb + 1); }        // tail.0's output
};
struct SrPlan {
    Map up, fin, new3, new2, new1, new_fin;
    Map t_last;          // last.0's output (p null: the image is not wanted)
    Map shuffle_in[3];   // the convolutions in front of the shuffles: bott2's, ups2's, ups3's output
    SrStage st[3];
};

void sr_stage_shapes(const SursEncoderNet &n, int H2, int W2, SrPlan &m) {
    int hs = H2, ws = W2;
    for (int i = 0; i < 3; ++i) {
        hs = (hs + 2 - 3) / 2 + 1; ws = (ws + 2 - 3) / 2 + 1;
        m.st[i].h = hs; m.st[i].w = ws; m.st[i].c = n.down[i].cout;
        m.st[i].nb = n.residual ? n.n_block[i] : 0;
    }
}

// Inference: three rotating buffers per stage (one stream: reuse is ordered), a temporary of its own per shuffle, feature_lr /
// feature_hr written where the caller wants them.
void sr_inference_maps(Run &r, int H2, int W2, bool want_image, float *feature_lr, float *feature_hr, SrPlan &m) {
    const SursEncoderNet &n = *r.net;
    m.fin = r.map(H2, W2, 64);                                  // cat(h, up3)
    m.new3 = r.map(H2 / 2, W2 / 2, 128);                        // cat(d1_f, up2)
    m.new2 = input_map(feature_lr, H2 / 4, W2 / 4, 256, 256);   // cat(d2_f, up1): the caller's buffer
    m.new1 = r.map(H2 / 8, W2 / 8, 512);                        // cat(d3_f, bo)
    m.up = r.map(H2, W2, 3);
    sr_stage_shapes(n, H2, W2, m);
    for (SrStage &s : m.st) {
        float *three[3];
        for (float *&b : three) b = r.map(s.h, s.w, s.c).p;
        for (int j = 0; j < 2 * s.nb + 2; ++j) s.buf[j] = three[j % 3];   // (block b reads j = 2 b, writes 2 b + 1, then 2 b + 2)
    }
    m.shuffle_in[0] = r.map(m.new1.h, m.new1.w, n.bott2.cout);
    m.shuffle_in[1] = r.map(m.new2.h, m.new2.w, n.ups2.cout);
    m.shuffle_in[2] = r.map(m.new3.h, m.new3.w, n.ups3.cout);
    m.new_fin = input_map(feature_hr, H2, W2, 64, 64);
    m.t_last = want_image ? r.map(H2, W2, n.last0.cout) : Map();
}

// The tape: one buffer per layer.  THE LAYOUT OF THE TAPE IS THE ORDER OF THE TAKES BELOW - a function of the net and the image size
// alone, so the forward and the backward find the same addresses by running this function.
void sr_tape_maps(Run &r, int H2, int W2, SrPlan &m) {
    const SursEncoderNet &n = *r.net;
    m.up = r.map(H2, W2, 3);
    m.fin = r.map(H2, W2, 64);
    m.new3 = r.map(H2 / 2, W2 / 2, 128);
    m.new2 = r.map(H2 / 4, W2 / 4, 256);       // = feature_lr
    m.new1 = r.map(H2 / 8, W2 / 8, 512);
    m.new_fin = r.map(H2, W2, 64);             // = feature_hr
    m.t_last = r.map(H2, W2, n.last0.cout);
    const Map shared = r.map(H2 / 2, W2 / 2, 128);   // the shuffles' inputs share one buffer (ups3's is the largest); nothing reads it back
    m.shuffle_in[0] = input_map(shared.p, m.new1.h, m.new1.w, n.bott2.cout, n.bott2.cout);
    m.shuffle_in[1] = input_map(shared.p, m.new2.h, m.new2.w, n.ups2.cout, n.ups2.cout);
    m.shuffle_in[2] = input_map(shared.p, m.new3.h, m.new3.w, n.ups3.cout, n.ups3.cout);
    sr_stage_shapes(n, H2, W2, m);
    for (SrStage &s : m.st)
        for (int j = 0; j < 2 * s.nb + 2; ++j) s.buf[j] = r.map(s.h, s.w, s.c).p;
}

// stage's block b, convolution `which` (0: in front of the ReLU, 1: behind it) in SursEncoderNet.body / SursSrParams.body
inline int sr_body_index(const SursEncoderNet &n, int stage, int b, int which) {
    int b0 = 0;
    for (int i = 0; i < stage; ++i) b0 += n.n_block[i];
    return 2 * (b0 + b) + which;
}
inline const SursConv *sr_body(const SursEncoderNet &n, int stage, int b, int which) { return &n.body[sr_body_index(n, stage, b, which)]; }
inline const SursSrParam *sr_body(const SursEncoderNet &n, const SursSrParams *p, int stage, int b, int which) {
    return &p->body[sr_body_index(n, stage, b, which)];
}

// x: the image; m.up's size is sr_scale times x's (a dry run reads nothing of x)
void super_res(Run &r, const Map &x, const SrPlan &m, float *img_sr) {
    const SursEncoderNet &n = *r.net;
    Map up = m.up;
    if (sr_scale(&n) == 2) bicubic_up2(r, x, false, nullptr, up, false);
    else bicubic_up(r, x, sr_scale(&n), up);
    Map h = m.fin.slice(0, 32);
    conv(r, up, n.head, h, 1, ACT, LRELU, nullptr);
    auto stage = [&](int i, const Map &src, Map dst) {
        const SrStage &s = m.st[i];
        Map a = s.a(0), u = s.u();
        conv(r, src, n.down[i], a, 2, ACT, LRELU, nullptr);
        for (int b = 0; b < s.nb; ++b) {
            Map t = s.t(b), a2 = s.a(b + 1);
            conv(r, a, *sr_body(n, i, b, 0), t, 1, ACT, RELU, nullptr);
            conv(r, t, *sr_body(n, i, b, 1), a2, 1, 0, 0.0f, &a);
            a = a2;
        }
        conv(r, a, n.tail0[i], u, 1, ACT, LRELU, nullptr);
        conv(r, u, n.tail2[i], dst, 1, ACT, LRELU, nullptr);
        return dst;
    };
    Map d1_f = stage(0, h, m.new3.slice(0, 64));
    Map d2_f = stage(1, d1_f, m.new2.slice(0, 128));
    Map d3_f = stage(2, d2_f, m.new1.slice(0, 256));
    Map bo = m.new1.slice(256, 256);
    conv(r, d3_f, n.bottleneck, bo, 1, ACT, LRELU, nullptr);
    // conv -> LeakyReLU -> PixelShuffle -> LeakyReLU (the second LeakyReLU is fused into the shuffle)
    auto shuffle = [&](const Map &src, const SursConv &cw, Map t, Map dst) {
        conv(r, src, cw, t, 1, ACT, LRELU, nullptr);
        pixel_shuffle2(r, t, 0.2f, dst);
    };
    shuffle(m.new1, n.bott2, m.shuffle_in[0], m.new2.slice(128, 128));
    shuffle(m.new2, n.ups2, m.shuffle_in[1], m.new3.slice(64, 64));
    shuffle(m.new3, n.ups3, m.shuffle_in[2], m.fin.slice(32, 32));
    Map new_fin = m.new_fin;
    conv(r, m.fin, n.ups4, new_fin, 1, ACT, LRELU, nullptr);
    if (m.t_last.p) {
        Map t = m.t_last, o = input_map(img_sr, new_fin.h, new_fin.w, 3, 3);
        conv(r, new_fin, n.last0, t, 1, ACT, LRELU, nullptr);
        conv(r, t, n.last2, o, 1, 0, 0.0f, nullptr);
    }
}

// ---------------------------------------------------------------- ConvBlock (lib/model/HGFilters.py:29-74), in_planes == out_planes
// out = cat(o1, o2, o3) + x; GroupNorm + ReLU applied in each convolution's staging from statistics handed from kernel to kernel.
// THREE launches (default): every convolution writes its own value (the next one's input, with its statistics) AND its slice of the
// sum, with the sum's statistics for the ConvBlock that follows (surs_conv2d_nhwc_gn_sum) - no closing pass over the map.
// SURS_ENC_SEPARATE_SUM (net->flags): the four-launch form of rounds 4 - 5 (convolutions into the slices, then surs_add3_gn), whose
// bits encoder.py's sequencing reproduces.  A first block (x without statistics) takes GroupNorm coefficients from
// surs_groupnorm_coeffs' two launches in front of its first convolution (in front of all three in the separate-sum form).
// The folded BatchNorm coefficients (bn1, bn2, bn3) of a ConvBlock of the net, by the array the block lives in; null: GroupNorm.
const SursBatchNorm *batchnorm_of(const Run &r, const SursConvBlock *b) {
    const SursEncoderNet &n = *r.net;
    if (!r.bn()) return nullptr;
    if (b == &n.conv2) return n.bn_conv2;
    const ptrdiff_t nhg = (ptrdiff_t)n.num_stack * per_stack_blocks(&n);
    if (b >= n.hg && b < n.hg + nhg) return n.bn_hg + 3 * (b - n.hg);
    return n.bn_top_m + 3 * (b - n.top_m);
}

// What a ConvBlock leaves for its backward (surs_encoder_convblock_backward): its input, the raw cat(o1, o2, o3), the sum in a map
// of its own and, per norm site, the coefficient vectors surs_groupnorm_fold forms from what the forward's kernels folded themselves.
struct NormTape { float *mean, *rstd, *scale, *shift; };
struct BlockTape {
    Map x, cat, out;
    NormTape nt[3];
};

// t: record the block - the separate-sum forms only (the launches of the host mirror, encoder.py), the sum into a map of its own;
// a GroupNorm net's (the gradient entry points refuse --norm batch)
Map conv_block(Run &r, const SursConvBlock &b, const Map &x, bool want_stats, BlockTape *t = nullptr) {
    const int c = x.c;
    Map cat = r.map(x.h, x.w, c);
    Map out = t ? r.map(x.h, x.w, c) : cat;   // (without a tape the sum overwrites the slices)
    Map o1 = cat.slice(0, c / 2), o2 = cat.slice(c / 2, c / 4), o3 = cat.slice(3 * c / 4, c / 4);
    auto eligible = [&](const Map &m, const SursConv &cw) {
        return (cw.ksize == 1 || cw.ksize == 3) && cw.w_split && m.c % 32 == 0 && m.ld % 4 == 0 && aligned16(m.p);
    };
    const bool fused = c % 128 == 0 && eligible(x, b.conv[0]) && eligible(o1, b.conv[1]) && eligible(o2, b.conv[2]);
    auto coeffs = [&](const Map &m, const SursGroupNorm &g, float *&sc, float *&sh) {
        sc = (float *)r.a->take(sizeof(float) * m.c);
        sh = (float *)r.a->take(sizeof(float) * m.c);
        void *scratch = r.a->take(surs_groupnorm_scratch_bytes());
        if (!r.dry && !r.rc) r.fail(surs_groupnorm_coeffs_ws(m.p, m.h * m.w, m.c, m.ld, 32, 1e-5f, g.gamma, g.beta, sc, sh, scratch, r.st));
    };
    // (the second output is made by the kernels' whole-tile epilogue: maps of whole 8-row x 32-column x 64-channel tiles - every map
    //  of a 512 x 512 image's hourglass; smaller ones take the separate sum)
    const bool sum_in_conv = !t && fused && !(r.net->flags & SURS_ENC_SEPARATE_SUM) && b.conv[0].ksize == 3 && b.conv[1].ksize == 3 &&
                             b.conv[2].ksize == 3 && x.w % 32 == 0 && x.h % 8 == 0 && c % 256 == 0;
    if (const SursBatchNorm *bn = batchnorm_of(r, &b)) {
        // BatchNorm in eval mode: the three normalisations are the caller's constants in the convolutions' staging, the same launches
        // without a statistics epilogue, buffer or fold
        out.set_stats(nullptr, 0);
        if (sum_in_conv) {
            Map raw1 = r.map(x.h, x.w, c / 2), raw2 = r.map(x.h, x.w, c / 4);
            if (r.dry || r.rc) return out;
            r.fail(surs_conv2d_nhwc_sum(r.parts, x.p, x.h, x.w, c, x.ld, b.conv[0].w_split, b.conv[0].bias, bn[0].scale, bn[0].shift, raw1.p, c / 2,
                                        raw1.ld, x.p, x.ld, o1.p, out.ld, r.st));
            if (!r.rc)
                r.fail(surs_conv2d_nhwc_sum(r.parts, raw1.p, x.h, x.w, c / 2, raw1.ld, b.conv[1].w_split, b.conv[1].bias, bn[1].scale, bn[1].shift,
                                            raw2.p, c / 4, raw2.ld, x.p + c / 2, x.ld, o2.p, out.ld, r.st));
            if (!r.rc)
                r.fail(surs_conv2d_nhwc_sum(r.parts, raw2.p, x.h, x.w, c / 4, raw2.ld, b.conv[2].w_split, b.conv[2].bias, bn[2].scale, bn[2].shift,
                                            nullptr, c / 4, 0, x.p + 3 * c / 4, x.ld, o3.p, out.ld, r.st));
            return out;
        }
        const Map ins[3] = {x, o1, o2};
        Map outs[3] = {o1, o2, o3};
        for (int k = 0; k < 3; ++k) conv(r, ins[k], b.conv[k], outs[k], 1, 0, 0.0f, nullptr, bn[k].scale, bn[k].shift);
        add3(r, out, x, out, false);
        return out;
    }
    if (sum_in_conv) {
        const int cap = ((x.w + 31) / 32) * ((x.h + 3) / 4), cg = c / 32;
        Map raw1 = r.map(x.h, x.w, c / 2), raw2 = r.map(x.h, x.w, c / 4);
        double *S = want_stats ? r.stats_buf(cap) : nullptr;
        SursGnStats st1 = {r.stats_buf(cap), cap, 0, 0, {0, 0, 0}}, st2 = {r.stats_buf(cap), cap, 0, 0, {0, 0, 0}};
        float *sc = nullptr, *sh = nullptr;
        if (!x.st.sums) coeffs(x, b.bn[0], sc, sh);
        int sl[3] = {0, 0, 0};
        out.st = SursGnStats{S, cap, (c / 2) / cg, (3 * c / 4) / cg, {0, 0, 0}};
        if (r.dry || r.rc) return out;
        r.fail(surs_conv2d_nhwc_gn_sum(r.parts, x.p, x.h, x.w, c, x.ld, b.conv[0].w_split, b.conv[0].bias, x.st.sums ? &x.st : nullptr, sc, sh,
                                       b.bn[0].gamma, b.bn[0].beta, 1e-5f, raw1.p, c / 2, raw1.ld, &st1, x.p, x.ld, o1.p, out.ld, S, cap, 0, cg,
                                       &sl[0], r.st));
        if (!r.rc)
            r.fail(surs_conv2d_nhwc_gn_sum(r.parts, raw1.p, x.h, x.w, c / 2, raw1.ld, b.conv[1].w_split, b.conv[1].bias, &st1, nullptr, nullptr,
                                           b.bn[1].gamma, b.bn[1].beta, 1e-5f, raw2.p, c / 4, raw2.ld, &st2, x.p + c / 2, x.ld, o2.p, out.ld, S,
                                           cap, (c / 2) / cg, cg, &sl[1], r.st));
        if (!r.rc)
            r.fail(surs_conv2d_nhwc_gn_sum(r.parts, raw2.p, x.h, x.w, c / 4, raw2.ld, b.conv[2].w_split, b.conv[2].bias, &st2, nullptr, nullptr,
                                           b.bn[2].gamma, b.bn[2].beta, 1e-5f, nullptr, c / 4, 0, nullptr, x.p + 3 * c / 4, x.ld, o3.p, out.ld, S,
                                           cap, (3 * c / 4) / cg, cg, &sl[2], r.st));
        out.st.slots[0] = sl[0]; out.st.slots[1] = sl[1]; out.st.slots[2] = sl[2];
        if (!S) out.set_stats(nullptr, 0);
        return out;
    }
    Map ins[3] = {x, o1, o2}, outs[3] = {o1, o2, o3};
    if (t) {
        t->x = x; t->cat = cat; t->out = out;
        for (int k = 0; k < 3; ++k) {
            NormTape &v = t->nt[k];
            v.mean = (float *)r.a->take(sizeof(float) * 32);
            v.rstd = (float *)r.a->take(sizeof(float) * 32);
            v.scale = (float *)r.a->take(sizeof(float) * ins[k].c);
            v.shift = (float *)r.a->take(sizeof(float) * ins[k].c);
        }
    }
    auto fold = [&](int k, const SursGnStats *st, void *scratch) {   // the tape's vectors of norm k: from statistics, or from the map
        if (r.dry || r.rc) return;
        const NormTape &v = t->nt[k];
        r.fail(surs_groupnorm_fold(st, st ? nullptr : ins[k].p, x.h * x.w, ins[k].c, ins[k].ld, 1e-5f, b.bn[k].gamma, b.bn[k].beta, v.mean, v.rstd,
                                   v.scale, v.shift, scratch, r.st));
    };
    if (fused && x.st.sums && x.st.g1 == 0) {
        for (int k = 0; k < 3; ++k) {
            conv_gn(r, ins[k], b.conv[k], outs[k], &b.bn[k], k < 2);
            if (k < 2) ins[k + 1].st = outs[k].st;   // (the slice the next convolution reads, with the statistics this one left)
            if (t) fold(k, &ins[k].st, nullptr);
        }
        add3(r, cat, x, out, want_stats);
        return out;
    }
    void *scratch = t ? r.a->take(surs_groupnorm_scratch_bytes()) : nullptr;
    for (int k = 0; k < 3; ++k) {
        float *sc, *sh;
        if (t) {
            fold(k, nullptr, scratch);
            sc = t->nt[k].scale; sh = t->nt[k].shift;
        } else {
            coeffs(ins[k], b.bn[k], sc, sh);
        }
        conv(r, ins[k], b.conv[k], outs[k], 1, 0, 0.0f, nullptr, sc, sh);
    }
    add3(r, cat, x, out, want_stats && fused);
    return out;
}

struct Events {   // per host thread: the events of the hourglass forks (created once; an event is reusable once its waits are enqueued)
    hipEvent_t e[16] = {};
    int n = 0;
    hipEvent_t get(int i) {
        if (i >= 16) return nullptr;
        if (!e[i] && hipEventCreateWithFlags(&e[i], hipEventDisableTiming) != hipSuccess) e[i] = nullptr;
        return e[i];
    }
};
thread_local Events t_events;

// Where the blocks of an hourglass's levels are in the stack's block array: the module order of HourGlass._generate_network
// (lib/model/HGFilters.py:85-94; encoder.EncoderWeights, include/surs.h), b1_d, b2_d, [level d - 1 ...], b2_plus_1, b3_1, ..., b3_d.
// The forward, its tape and the backward all walk this one table.
struct HgLevel { int b1, b2, b2_plus, b3; };   // b2_plus: level 1 only
constexpr int HG_MAX_DEPTH = 4, HG_MAX_BLOCKS = 3 * HG_MAX_DEPTH + 1;
void hg_levels(int depth, HgLevel lv[HG_MAX_DEPTH + 1]) {   // lv[1 .. depth]
    for (int level = depth; level >= 1; --level) lv[level] = HgLevel{2 * (depth - level), 2 * (depth - level) + 1, -1, 2 * depth + level};
    lv[1].b2_plus = 2 * depth;
}

// HourGlass._forward (lib/model/HGFilters.py:96-117).  The two branches of a level are independent until their sum: with side
// streams lent by the caller the low-resolution one (pool -> ConvBlock -> [next level] -> ConvBlock) runs beside the
// full-resolution ConvBlock, ordered by events at the fork and the join.  tape (one stream only): where block i records itself,
// [3 depth + 1] in the order of `blocks`.
Map hourglass(Run &r, const SursConvBlock *blocks, int depth, const Map &x, const SursEncoderStreams *ss, BlockTape *tape = nullptr) {
    struct Fwd {
        Run &r; const SursConvBlock *blocks; const SursEncoderStreams *ss; BlockTape *tape;
        HgLevel lv[HG_MAX_DEPTH + 1];
        int ev = 0;
        Map block(int i, const Map &inp, bool want_stats) { return conv_block(r, blocks[i], inp, want_stats, tape ? tape + i : nullptr); }
        Map low_branch(int level, const Map &inp) {
            Map pooled = avgpool2(r, inp, !r.bn());
            Map low1 = block(lv[level].b2, pooled, true);
            Map low2 = level > 1 ? run(level - 1, low1) : block(lv[level].b2_plus, low1, true);
            return block(lv[level].b3, low2, false);
        }
        Map run(int level, const Map &inp) {
            hipStream_t side = (ss && level <= 4) ? (hipStream_t)ss->side[level - 1] : nullptr;
            hipEvent_t e_fork = nullptr, e_join = nullptr;
            if (side && !r.dry) {
                e_fork = t_events.get(ev++);
                e_join = t_events.get(ev++);
                if (!e_fork || !e_join) side = nullptr;
            }
            Map up1, low3;
            if (side && !r.dry && !r.rc) {
                hipStream_t cur = r.st;
                if (hipEventRecord(e_fork, cur) != hipSuccess || hipStreamWaitEvent(side, e_fork, 0) != hipSuccess)
                    r.fail(fail(SURS_E_HIP, "encoder: fork of the hourglass streams failed"));
                r.st = side;
                low3 = low_branch(level, inp);
                r.st = cur;
                up1 = block(lv[level].b1, inp, false);
                if (hipEventRecord(e_join, side) != hipSuccess || hipStreamWaitEvent(cur, e_join, 0) != hipSuccess)
                    r.fail(fail(SURS_E_HIP, "encoder: join of the hourglass streams failed"));
            } else {
                up1 = block(lv[level].b1, inp, false);
                low3 = low_branch(level, inp);
            }
            Map out = r.map(2 * low3.h, 2 * low3.w, low3.c);
            if (r.bn()) bicubic_up2_block(r, low3, true, &up1, out);
            else bicubic_up2(r, low3, true, &up1, out, true);   // up1 + up2
            return out;
        }
    } f{r, blocks, ss, tape};
    hg_levels(depth, f.lv);
    return f.run(depth, x);
}

// What a stack's tail leaves for its backward (surs_encoder_tail_backward): its input ll, conv_last's raw output t, the stack's output
// out = l(relu(bn_end(t))) and bn_end's four coefficient vectors.
struct TailTape {
    Map ll, t, out;
    NormTape nt;
};

// The tail of GroupNorm stack s: conv_last leaves bn_end's statistics; l (where the stack's output is wanted: out.p) and the merged
// next (not for the last stack; returned, with the statistics for the next hourglass) fold them.  The ONE launch list of the tail:
// filter_lr() below, surs_encoder_tail_train and surs_encoder_filter_lr_train (tape: plus one surs_groupnorm_fold for bn_end).
Map stack_tail(Run &r, int s, const Map &ll, const Map &previous, Map out, bool last, TailTape *tape = nullptr) {
    const SursEncoderNet &n = *r.net;
    Map t = r.map(ll.h, ll.w, n.conv_last[s].cout);
    conv_gn(r, ll, n.conv_last[s], t, nullptr, true);
    if (out.p) conv_gn(r, t, n.l[s], out, &n.bn_end[s], false);
    Map nx;
    if (!last) {
        nx = r.map(t.h, t.w, n.next[s].cout);
        conv_gn(r, t, n.next[s], nx, &n.bn_end[s], true, &previous);
    }
    if (tape) {
        tape->ll = ll; tape->t = t; tape->out = out;
        NormTape &v = tape->nt;
        v.mean = (float *)r.a->take(sizeof(float) * 32);
        v.rstd = (float *)r.a->take(sizeof(float) * 32);
        v.scale = (float *)r.a->take(sizeof(float) * t.c);
        v.shift = (float *)r.a->take(sizeof(float) * t.c);
        if (!r.dry && !r.rc)
            r.fail(surs_groupnorm_fold(&t.st, nullptr, t.h * t.w, t.c, t.ld, 1e-5f, n.bn_end[s].gamma, n.bn_end[s].beta, v.mean, v.rstd, v.scale,
                                       v.shift, nullptr, r.st));
    }
    return nx;
}

// HGFilter.forward, low_res (lib/model/HGFilters.py:183-206).  outs[s]: where stack s's output goes (NULL: not wanted; the last
// stack's is always wanted).  The tail of a stack is two launches (three where the stack's output is wanted): conv_last leaves
// bn_end's statistics, the pointwise convolutions behind it fold them; previous + bl(t') + al(l(t')) is ONE pointwise convolution
// (`next`, packed by the caller: W = W_bl + W_al W_l) with the sum in its epilogue.
void filter_lr(Run &r, const Map &feature_lr, float *const *outs, const SursEncoderStreams *ss, Arena *arenas /* [2] */) {
    const SursEncoderNet &n = *r.net;
    const int per_stack = per_stack_blocks(&n);   // three per level + b2_plus_1
    r.a = &arenas[1];
    Map previous = conv_block(r, n.conv2, feature_lr, true);
    for (int s = 0; s < n.num_stack; ++s) {
        r.a = &arenas[s & 1];
        r.a->off = 0;   // (the arena of stack s - 2: every kernel of that stack was joined before stack s - 1 started)
        Map hg = hourglass(r, n.hg + (size_t)s * per_stack, n.hg_depth, previous, ss);
        Map ll = conv_block(r, n.top_m[s], hg, false);
        const bool last = s == n.num_stack - 1;
        if (r.bn()) {   // the same pointwise launches with bn_end's constants, no statistics
            const SursBatchNorm &be = n.bn_end_bn[s];
            Map t = r.map(ll.h, ll.w, n.conv_last[s].cout);
            conv(r, ll, n.conv_last[s], t, 1, 0, 0.0f, nullptr);
            if (outs[s]) {
                Map o = input_map(outs[s], t.h, t.w, n.l[s].cout, n.l[s].cout);
                conv(r, t, n.l[s], o, 1, 0, 0.0f, nullptr, be.scale, be.shift);
            }
            if (!last) {
                Map nx = r.map(t.h, t.w, n.next[s].cout);
                conv(r, t, n.next[s], nx, 1, 0, 0.0f, &previous, be.scale, be.shift);
                previous = nx;
            }
            continue;
        }
        const Map nx = stack_tail(r, s, ll, previous, outs[s] ? input_map(outs[s], ll.h, ll.w, n.l[s].cout, n.l[s].cout) : Map(), last);
        if (!last) previous = nx;
    }
}

int check_net(const SursEncoderNet *n) {
    SURS_REQUIRE(n, "null network");
    SURS_REQUIRE(n->num_stack >= 1 && n->num_stack <= 16 && n->hg_depth >= 1 && n->hg_depth <= 4, "1..16 stacks, hourglass depth 1..4");
    SURS_REQUIRE(n->parts == 1 || n->parts == 2, "parts: 2 (fp32-grade) or 1");
    SURS_REQUIRE((n->flags & ~(SURS_ENC_SEPARATE_SUM | SURS_ENC_EXTENDED)) == 0, "unknown flags");
    for (int i = 0; i < 3; ++i) SURS_REQUIRE(n->n_block[i] >= 0 && n->n_block[i] <= 64, "bad n_block");
    if (!(n->flags & SURS_ENC_EXTENDED)) return 0;
    SURS_REQUIRE(n->norm == SURS_NORM_GROUP || n->norm == SURS_NORM_BATCH, "norm %d: the supported values are 'group' and 'batch'", n->norm);
    SURS_REQUIRE(n->sr_scale == 0 || (n->sr_scale >= SURS_SR_SCALE_MIN && n->sr_scale <= SURS_SR_SCALE_MAX),
                 "scale %d: the super-resolution factor must be an integer in 1..4", n->sr_scale);
    if (n->norm == SURS_NORM_BATCH) {
        SURS_REQUIRE(n->bn_conv2 && n->bn_hg && n->bn_top_m && n->bn_end_bn && n->hg && n->top_m, "BatchNorm net: null coefficient array");
        auto filled = [](const SursBatchNorm *a, int count) {
            for (int i = 0; i < count; ++i)
                if (!a[i].scale || !a[i].shift) return false;
            return true;
        };
        SURS_REQUIRE(filled(n->bn_conv2, 3) && filled(n->bn_hg, 3 * n->num_stack * per_stack_blocks(n)) && filled(n->bn_top_m, 3 * n->num_stack) &&
                     filled(n->bn_end_bn, n->num_stack), "BatchNorm net: a norm site without folded coefficients");
    }
    return 0;
}

// the size rule of the three stride-2 stages, on the enlarged image; factor 2: in its words of old, on the input
int check_image_size(const SursEncoderNet *n, int h, int w) {
    const int s = sr_scale(n);
    if (s == 2) {
        SURS_REQUIRE(h > 0 && w > 0 && h % 4 == 0 && w % 4 == 0, "input image height/width must be multiples of 4 (three stride-2 stages), got %dx%d", h, w);
        return 0;
    }
    SURS_REQUIRE(h > 0 && w > 0 && (s * h) % 8 == 0 && (s * w) % 8 == 0,
                 "input image %dx%d enlarged by the factor %d is %dx%d: the enlarged height/width must be multiples of 8 (three stride-2 stages)",
                 h, w, s, s * h, s * w);
    return 0;
}

float *const NOWHERE = reinterpret_cast<float *>(4096);   // a pointer for runs without launches

// the bytes super_res() takes from its workspace
size_t sr_inference_need(const SursEncoderNet *net, int eh, int ew, bool want_image) {
    Dry d(net);
    SrPlan m;
    sr_inference_maps(d.r, eh, ew, want_image, NOWHERE, NOWHERE, m);
    return d.a.peak;
}

// the bytes of each of filter_lr()'s two arenas: the same sequencing, counted
size_t filter_lr_half(const SursEncoderNet *net, int h, int w, int ld, float *const *outs) {
    Arena ar[2];
    ar[0].dry = ar[1].dry = true;
    Run r{net, &ar[0], nullptr, net->parts, true};
    filter_lr(r, input_map(NOWHERE, h, w, 256, ld), outs, nullptr, ar);
    return align_up(ar[0].peak > ar[1].peak ? ar[0].peak : ar[1].peak, 256);
}

}  // namespace

extern "C" size_t surs_encoder_workspace_bytes_enlarged(const SursEncoderNet *net, int eh, int ew) {
    if (!net || eh <= 0 || ew <= 0 || check_net(net)) return 0;
    // the stages run one after the other on one workspace: the largest of them; filter_lr = two arenas
    const size_t sr = align_up(sr_inference_need(net, eh, ew, true), 256);
    float *outs[16];
    for (int s = 0; s < 16; ++s) outs[s] = NOWHERE;
    const size_t half = filter_lr_half(net, eh / 4, ew / 4, 256, outs);
    return (sr > 2 * half ? sr : 2 * half) + 256;
}

extern "C" size_t surs_encoder_workspace_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || h <= 0 || w <= 0 || check_net(net)) return 0;
    return surs_encoder_workspace_bytes_enlarged(net, sr_scale(net) * h, sr_scale(net) * w);
}

extern "C" int surs_encoder_super_res(const SursEncoderNet *net, const float *x, int h, int w, int x_ld, int want_image, float *img_sr,
                                      float *feature_lr, float *feature_hr, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_net(net)) return rc;
    SURS_REQUIRE(x && feature_lr && feature_hr && workspace && (!want_image || img_sr), "null argument");
    if (int rc = check_image_size(net, h, w)) return rc;
    SURS_REQUIRE(x_ld >= 3, "input image: three channels");
    const int eh = sr_scale(net) * h, ew = sr_scale(net) * w;
    const size_t need = sr_inference_need(net, eh, ew, want_image != 0);
    Arena a;
    SURS_REQUIRE(workspace_arena(workspace, workspace_bytes, need, a), "workspace too small: %zu bytes needed", need + 256);
    Run r{net, &a, as_stream(stream), net->parts, false};
    SrPlan m;
    sr_inference_maps(r, eh, ew, want_image != 0, feature_lr, feature_hr, m);
    super_res(r, input_map(x, h, w, 3, x_ld), m, img_sr);
    return r.rc;
}

extern "C" int surs_encoder_filter_lr(const SursEncoderNet *net, const float *feature_lr, int h, int w, int ld, float *const *outs,
                                      void *workspace, size_t workspace_bytes, const SursEncoderStreams *streams, void *stream) {
    if (int rc = check_net(net)) return rc;
    SURS_REQUIRE(feature_lr && outs && workspace && outs[net->num_stack - 1], "null argument (the last stack's output is always wanted)");
    SURS_REQUIRE(h > 0 && w > 0 && h % (1 << net->hg_depth) == 0 && w % (1 << net->hg_depth) == 0, "feature_lr size must be a multiple of 2^hg_depth");
    SURS_REQUIRE(ld >= 256 && ld % 4 == 0 && aligned16(feature_lr), "feature_lr: 256 channels, 16-byte aligned pixels");
    for (int s = 0; s < net->num_stack; ++s) {   // --hg_dim: outs[s] is [h][w][l{s}.cout], pitch l{s}.cout
        const int d = net->l[s].cout;
        SURS_REQUIRE(d >= 16 && d <= 512 && d % 16 == 0, "hg_dim %d: the supported values are the multiples of 16 from 16 to 512", d);
    }
    const size_t half = filter_lr_half(net, h, w, ld, outs);
    Arena ar[2];
    SURS_REQUIRE(workspace_arena(workspace, workspace_bytes, 2 * half, ar[0]), "workspace too small: %zu bytes needed", 2 * half + 256);
    ar[0].cap = ar[1].cap = half;
    ar[1].base = ar[0].base + half;
    Run r{net, &ar[0], as_stream(stream), net->parts, false};
    filter_lr(r, input_map(feature_lr, h, w, 256, ld), outs, streams, ar);
    return r.rc;
}

extern "C" int surs_encoder_filter_hr(const SursEncoderNet *net, const float *feature_hr, int h, int w, int ld, float *out, void *stream) {
    if (int rc = check_net(net)) return rc;
    SURS_REQUIRE(feature_hr && out && h > 0 && w > 0, "null argument");
    Arena a;
    Run r{net, &a, as_stream(stream), net->parts, false};
    Map o = input_map(out, h, w, net->conv5.cout, net->conv5.cout);
    conv(r, input_map(feature_hr, h, w, net->conv5.cin, ld), net->conv5, o, 1, 0, 0.0f, nullptr);
    return r.rc;
}

extern "C" int surs_encoder_forward(const SursEncoderNet *net, const float *image, int h, int w, int x_ld, float *feature_lr,
                                    float *feature_hr, float *im_feat_lr, float *im_feat_hr, void *workspace, size_t workspace_bytes,
                                    const SursEncoderStreams *streams, void *stream) {
    if (int rc = check_net(net)) return rc;
    SURS_REQUIRE(im_feat_lr && im_feat_hr, "null argument");
    int rc = surs_encoder_super_res(net, image, h, w, x_ld, 0, nullptr, feature_lr, feature_hr, workspace, workspace_bytes, stream);
    if (rc) return rc;
    const int eh = sr_scale(net) * h, ew = sr_scale(net) * w;
    if ((rc = surs_encoder_filter_hr(net, feature_hr, eh, ew, 64, im_feat_hr, stream))) return rc;
    float *outs[16] = {};
    outs[net->num_stack - 1] = im_feat_lr;
    return surs_encoder_filter_lr(net, feature_lr, eh / 4, ew / 4, 256, outs, workspace, workspace_bytes, streams, stream);
}

// ---------------------------------------------------------------- super-resolution gradients (include/surs.h)
// surs_encoder_super_res_train is super_res() over the tape plan (sr_tape_maps(): ONE buffer per layer) + conv5;
// surs_encoder_super_res_backward walks the same maps in reverse on the primitives of surs_sr_grad.hip.
namespace {

// the shapes the backward's fixed channel slices rest on (the released SuRSSR_v3; the forward's cat() buffers assume the same)
int check_sr_shapes(const SursEncoderNet *n) {
    auto is = [](const SursConv &c, int cin, int cout, int k) { return c.cin == cin && c.cout == cout && c.ksize == k; };
    bool ok = is(n->head, 3, 32, 3) && is(n->down[0], 32, 32, 3) && is(n->down[1], 64, 64, 3) && is(n->down[2], 128, 128, 3) &&
              is(n->bottleneck, 256, 256, 3) && is(n->bott2, 512, 512, 3) && is(n->ups2, 256, 256, 3) && is(n->ups3, 128, 128, 3) &&
              is(n->ups4, 64, 64, 3) && n->last0.cin == 64 && n->last0.ksize == 3 && n->last2.cin == n->last0.cout && n->last2.cout == 3 &&
              n->last2.ksize == 3 && n->conv5.cin == 64 && n->conv5.ksize == 1 && n->conv5.cout >= 1;
    for (int i = 0; i < 3 && ok; ++i) {
        const int c = n->down[i].cout;
        ok = is(n->tail0[i], c, c, 3) && is(n->tail2[i], c, 2 * c, 3);
        for (int b = 0; ok && n->residual && b < n->n_block[i]; ++b) ok = n->body && is(*sr_body(*n, i, b, 0), c, c, 3) && is(*sr_body(*n, i, b, 1), c, c, 3);
    }
    SURS_REQUIRE(ok, "super-resolution gradients: the convolutions are not SuRSSR_v3's (head 3-32, stages of 32, 64, 128 channels, bott2 512-512, ...)");
    return 0;
}

int check_sr_train(const SursEncoderNet *net, int h, int w) {
    if (int rc = check_net(net)) return rc;
    SURS_REQUIRE(net->parts == 2, "super-resolution gradients: net->parts == 1 (the bf16 / f16 encoder) has no backward: training runs the "
                                  "fp32-grade forward (parts == 2)");
    if (int rc = check_sr_shapes(net)) return rc;
    return check_image_size(net, h, w);
}

constexpr float LRELU2 = 0.2f * 0.2f;   // LeakyReLU(LeakyReLU(z)) below zero

struct SrBack {
    Run &r;
    const SursSrParams *P, *G;
    int acc;
    void *wws = nullptr;        // the weight gradient's slabs
    size_t wws_bytes = 0, wws_need = 0;   // wws_need: the largest slab any wgrad() so far asked for

    // dW, db of the convolution x -> (pre-activation of) y from g = d L / d y
    void wgrad(const Map &g, const Map *y, float slope, const Map &x, const SursConv &cw, int stride, const SursSrParam &gp) {
        const size_t need = surs_conv_grad_weight_workspace_bytes(g.h, g.w, cw.cin, cw.cout, cw.ksize);
        if (need > wws_need) wws_need = need;
        if (r.dry || r.rc) return;
        r.fail(surs_conv_grad_weight(g.p, g.h, g.w, cw.cout, g.ld, y ? y->p : nullptr, y ? y->ld : 0, slope, x.p, x.h, x.w, cw.cin, x.ld, cw.ksize,
                                     stride, gp.weight, gp.bias, acc, wws, wws_bytes, r.st));
    }
    void dgrad(const Map &g, const Map *y, float slope, const SursConv &cw, const SursSrParam &p, int stride, const Map &dx, bool add) {
        if (r.dry || r.rc) return;
        r.fail(surs_conv_grad_input(g.p, g.h, g.w, cw.cout, g.ld, y ? y->p : nullptr, y ? y->ld : 0, slope, p.weight, cw.cin, cw.ksize, stride,
                                    dx.p, dx.h, dx.w, dx.ld, add ? 1 : 0, r.st));
    }
    // a layer no gradient reaches: its gradient is zero (accumulate: nothing to add)
    void zero(const SursConv &cw, const SursSrParam &gp) {
        if (r.dry || r.rc || acc) return;
        if (hipMemsetAsync(gp.weight, 0, sizeof(float) * cw.cout * cw.cin * cw.ksize * cw.ksize, r.st) != hipSuccess ||
            (gp.bias && hipMemsetAsync(gp.bias, 0, sizeof(float) * cw.cout, r.st) != hipSuccess))
            r.fail(fail(SURS_E_HIP, "super-resolution gradients: hipMemsetAsync failed"));
    }
    void copy(const float *src, const Map &dst) {   // dense map -> dense map
        if (r.dry || r.rc) return;
        if (hipMemcpyAsync(dst.p, src, sizeof(float) * dst.h * dst.w * dst.c, hipMemcpyDeviceToDevice, r.st) != hipSuccess)
            r.fail(fail(SURS_E_HIP, "super-resolution gradients: hipMemcpyAsync failed"));
    }
    void unshuffle(const Map &g_o, const Map &y, const Map &t) {   // g of a shuffle's output (stored: y) -> g of its input
        if (r.dry || r.rc) return;
        r.fail(surs_pixel_unshuffle2_grad(g_o.p, t.h, t.w, g_o.c, g_o.ld, y.p, y.ld, LRELU2, t.p, t.ld, r.st));
    }
    void add(const Map &g, const Map &into) {   // into += g
        if (r.dry || r.rc) return;
        r.fail(surs_add3(into.p, into.ld, g.p, g.ld, nullptr, 0, into.h * into.w, into.c, into.p, into.ld, r.st));
    }
};

// r.a: the workspace arena (the gradient maps, then the weight gradient's slabs)
void sr_backward(SrBack &run, const SrPlan &m, const float *g_img_sr, const float *g_feature_lr, const float *g_im_feat_hr) {
    Run &r = run.r;
    const SursEncoderNet &n = *r.net;
    const int H2 = m.fin.h, W2 = m.fin.w;
    Map g_newfin = r.map(H2, W2, 64), g_tlast = r.map(H2, W2, n.last0.cout), g_fin = r.map(H2, W2, 64);
    Map g_new3 = r.map(H2 / 2, W2 / 2, 128), g_new2 = r.map(H2 / 4, W2 / 4, 256), g_new1 = r.map(H2 / 8, W2 / 8, 512);
    Map dzt = r.map(H2 / 2, W2 / 2, 128);   // the gradient in front of a shuffle (ups3's is the largest)
    Map pq[2] = {r.map(H2 / 2, W2 / 2, 32), r.map(H2 / 2, W2 / 2, 32)};   // the two gradient maps a stage alternates between
    auto walk = [&](SrBack &k, const float *g_img, const float *g_lr, const float *g_hr) {
        const bool top = g_img || g_hr;   // does any gradient reach feature_hr?
        if (g_img) {
            const Map gi = input_map(g_img, H2, W2, 3, 3);
            k.wgrad(gi, nullptr, 1.0f, m.t_last, n.last2, 1, k.G->last2);
            k.dgrad(gi, nullptr, 1.0f, n.last2, k.P->last2, 1, g_tlast, false);
            k.wgrad(g_tlast, &m.t_last, LRELU, m.new_fin, n.last0, 1, k.G->last0);
            k.dgrad(g_tlast, &m.t_last, LRELU, n.last0, k.P->last0, 1, g_newfin, false);
        } else {
            k.zero(n.last2, k.G->last2);
            k.zero(n.last0, k.G->last0);
        }
        if (g_hr) {
            const Map gh = input_map(g_hr, H2, W2, n.conv5.cout, n.conv5.cout);
            k.wgrad(gh, nullptr, 1.0f, m.new_fin, n.conv5, 1, k.G->conv5);
            k.dgrad(gh, nullptr, 1.0f, n.conv5, k.P->conv5, 1, g_newfin, g_img != nullptr);
        } else {
            k.zero(n.conv5, k.G->conv5);
        }
        // a shuffle level: g of the shuffled slice `o` (stored output `y`) -> the convolution cw on src; the gradient of src replaces g_src
        auto unshuffle = [&](const Map &g_o, const Map &y, const Map &src, const SursConv &cw, const SursSrParam &p, const SursSrParam &gp,
                             const Map &g_src) {
            const Map t = input_map(dzt.p, src.h, src.w, cw.cout, cw.cout);
            k.unshuffle(g_o, y, t);
            k.wgrad(t, nullptr, 1.0f, src, cw, 1, gp);
            k.dgrad(t, nullptr, 1.0f, cw, p, 1, g_src, false);
        };
        if (top) {
            k.wgrad(g_newfin, &m.new_fin, LRELU, m.fin, n.ups4, 1, k.G->ups4);
            k.dgrad(g_newfin, &m.new_fin, LRELU, n.ups4, k.P->ups4, 1, g_fin, false);
            unshuffle(g_fin.slice(32, 32), m.fin.slice(32, 32), m.new3, n.ups3, k.P->ups3, k.G->ups3, g_new3);
            unshuffle(g_new3.slice(64, 64), m.new3.slice(64, 64), m.new2, n.ups2, k.P->ups2, k.G->ups2, g_new2);
            if (g_lr) k.add(input_map(g_lr, g_new2.h, g_new2.w, 256, 256), g_new2);   // feature_lr's own gradient joins ups2's
        } else {
            k.zero(n.ups4, k.G->ups4);
            k.zero(n.ups3, k.G->ups3);
            k.zero(n.ups2, k.G->ups2);
            k.copy(g_lr, g_new2);
        }
        unshuffle(g_new2.slice(128, 128), m.new2.slice(128, 128), m.new1, n.bott2, k.P->bott2, k.G->bott2, g_new1);
        {
            Map g_bo = g_new1.slice(256, 256), bo = m.new1.slice(256, 256), d3_f = m.new1.slice(0, 256);
            k.wgrad(g_bo, &bo, LRELU, d3_f, n.bottleneck, 1, k.G->bottleneck);
            k.dgrad(g_bo, &bo, LRELU, n.bottleneck, k.P->bottleneck, 1, g_new1.slice(0, 256), true);
        }
        // a stage in reverse: g_dst = d L / d dst (all consumers added), its input's gradient is added to (or, live == false, replaces) g_src
        auto stage = [&](int i, const Map &src, const Map &dst, const Map &g_dst, const Map &g_src, bool live) {
            const SrStage &s = m.st[i];
            const Map P = input_map(pq[0].p, s.h, s.w, s.c, s.c), Q = input_map(pq[1].p, s.h, s.w, s.c, s.c), u = s.u(), a0 = s.a(0);
            k.wgrad(g_dst, &dst, LRELU, u, n.tail2[i], 1, k.G->tail2[i]);
            k.dgrad(g_dst, &dst, LRELU, n.tail2[i], k.P->tail2[i], 1, P, false);
            k.wgrad(P, &u, LRELU, s.a(s.nb), n.tail0[i], 1, k.G->tail0[i]);
            k.dgrad(P, &u, LRELU, n.tail0[i], k.P->tail0[i], 1, Q, false);
            for (int b = s.nb - 1; b >= 0; --b) {   // a(b + 1) = body.2(relu(body.0(a(b)))) + a(b);  Q = d L / d a(b + 1) -> d L / d a(b)
                const SursConv &c0 = *sr_body(n, i, b, 0), &c2 = *sr_body(n, i, b, 1);
                const Map t = s.t(b);
                k.wgrad(Q, nullptr, 1.0f, t, c2, 1, *sr_body(n, k.G, i, b, 1));
                k.dgrad(Q, nullptr, 1.0f, c2, *sr_body(n, k.P, i, b, 1), 1, P, false);
                k.wgrad(P, &t, RELU, s.a(b), c0, 1, *sr_body(n, k.G, i, b, 0));
                k.dgrad(P, &t, RELU, c0, *sr_body(n, k.P, i, b, 0), 1, Q, true);
            }
            k.wgrad(Q, &a0, LRELU, src, n.down[i], 2, k.G->down[i]);
            if (g_src.p) k.dgrad(Q, &a0, LRELU, n.down[i], k.P->down[i], 2, g_src, live);
            if (!n.residual)
                for (int b = 0; b < n.n_block[i]; ++b) {   // blocks the forward does not run
                    k.zero(*sr_body(n, i, b, 0), *sr_body(n, k.G, i, b, 0));
                    k.zero(*sr_body(n, i, b, 1), *sr_body(n, k.G, i, b, 1));
                }
        };
        stage(2, m.new2.slice(0, 128), m.new1.slice(0, 256), g_new1.slice(0, 256), g_new2.slice(0, 128), true);
        stage(1, m.new3.slice(0, 64), m.new2.slice(0, 128), g_new2.slice(0, 128), g_new3.slice(0, 64), top);
        stage(0, m.fin.slice(0, 32), m.new3.slice(0, 64), g_new3.slice(0, 64), g_fin.slice(0, 32), top);
        Map h = m.fin.slice(0, 32);
        k.wgrad(g_fin.slice(0, 32), &h, LRELU, m.up, n.head, 1, k.G->head);
    };
    {   // the slabs: the largest any layer asks for - the walk itself without launches, every upstream gradient present
        Run rd = r;
        rd.dry = true;
        SrBack d{rd, run.P, run.G, run.acc};
        walk(d, NOWHERE, NOWHERE, NOWHERE);
        run.wws_bytes = d.wws_need;
        run.wws = r.a->take(run.wws_bytes);
    }
    if (r.dry || r.rc || !r.a->ok()) return;
    walk(run, g_img_sr, g_feature_lr, g_im_feat_hr);
}

size_t sr_tape_need(const SursEncoderNet *net, int eh, int ew) {
    Dry d(net);
    SrPlan m;
    sr_tape_maps(d.r, eh, ew, m);
    return align_up(d.a.peak, 256);
}

size_t sr_backward_need(const SursEncoderNet *net, int eh, int ew) {
    Dry t(net), d(net);
    SrPlan m;
    sr_tape_maps(t.r, eh, ew, m);
    static const SursSrParam no_body[2 * 3 * 64] = {};   // (a run without launches reads no parameter; it forms their addresses)
    SursSrParams none = {};
    none.body = no_body;
    SrBack k{d.r, &none, &none, 0};
    sr_backward(k, m, nullptr, nullptr, nullptr);
    return align_up(d.a.peak, 256) + 256;
}

bool sr_params_filled(const SursEncoderNet *n, const SursSrParams *p) {
    auto ok = [](const SursSrParam &q) { return q.weight && q.bias; };
    bool all = ok(p->head) && ok(p->bottleneck) && ok(p->bott2) && ok(p->ups2) && ok(p->ups3) && ok(p->ups4) && ok(p->last0) && ok(p->last2) &&
               ok(p->conv5);
    int nb = 0;
    for (int i = 0; i < 3; ++i) {
        all = all && ok(p->down[i]) && ok(p->tail0[i]) && ok(p->tail2[i]);
        nb += n->n_block[i];
    }
    if (nb && !p->body) return false;
    for (int b = 0; b < 2 * nb; ++b) all = all && ok(p->body[b]);
    return all;
}

}  // namespace

extern "C" size_t surs_encoder_sr_tape_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_sr_train(net, h, w)) return 0;
    return sr_tape_need(net, sr_scale(net) * h, sr_scale(net) * w);
}

extern "C" size_t surs_encoder_sr_backward_workspace_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_sr_train(net, h, w)) return 0;
    return sr_backward_need(net, sr_scale(net) * h, sr_scale(net) * w);
}

extern "C" int surs_encoder_super_res_train(const SursEncoderNet *net, const float *x, int h, int w, int x_ld, float *img_sr,
                                            float *feature_lr, float *feature_hr, float *im_feat_hr, void *tape, size_t tape_bytes,
                                            void *stream) {
    SURS_REQUIRE(net, "null network");
    if (int rc = check_sr_train(net, h, w)) return rc;
    SURS_REQUIRE(x && img_sr && feature_lr && feature_hr && im_feat_hr && tape, "super_res_train: null argument");
    SURS_REQUIRE(x_ld >= 3, "input image: three channels");
    SURS_REQUIRE(((size_t)tape & 255) == 0, "super_res_train: the tape must be 256-byte aligned");
    const int eh = sr_scale(net) * h, ew = sr_scale(net) * w;
    const size_t need = sr_tape_need(net, eh, ew);
    SURS_REQUIRE(need <= tape_bytes, "super_res_train: tape too small: %zu bytes needed", need);
    Arena a = tape_arena(tape, tape_bytes);
    Run r{net, &a, as_stream(stream), net->parts, false};
    SrPlan m;
    sr_tape_maps(r, eh, ew, m);
    super_res(r, input_map(x, h, w, 3, x_ld), m, img_sr);
    Map f = input_map(im_feat_hr, eh, ew, net->conv5.cout, net->conv5.cout);
    conv(r, m.new_fin, net->conv5, f, 1, 0, 0.0f, nullptr);
    if (r.rc) return r.rc;
    SURS_HIP_CHECK(hipMemcpyAsync(feature_lr, m.new2.p, sizeof(float) * m.new2.h * m.new2.w * 256, hipMemcpyDeviceToDevice, r.st));
    SURS_HIP_CHECK(hipMemcpyAsync(feature_hr, m.new_fin.p, sizeof(float) * m.new_fin.h * m.new_fin.w * 64, hipMemcpyDeviceToDevice, r.st));
    return 0;
}

extern "C" int surs_encoder_super_res_backward(const SursEncoderNet *net, const SursSrParams *params, const void *tape, int h, int w,
                                               const float *g_img_sr, const float *g_feature_lr, const float *g_im_feat_hr,
                                               const SursSrParams *grads, int accumulate, void *workspace, size_t workspace_bytes,
                                               void *stream) {
    SURS_REQUIRE(net, "null network");
    if (int rc = check_sr_train(net, h, w)) return rc;
    SURS_REQUIRE(params && grads && tape && workspace, "super_res_backward: null argument");
    SURS_REQUIRE(g_img_sr || g_feature_lr || g_im_feat_hr, "super_res_backward: no upstream gradient (all three are NULL)");
    SURS_REQUIRE(sr_params_filled(net, params) && sr_params_filled(net, grads), "super_res_backward: a null weight or bias pointer in params / grads");
    SURS_REQUIRE(((size_t)tape & 255) == 0, "super_res_backward: the tape must be 256-byte aligned");
    const int eh = sr_scale(net) * h, ew = sr_scale(net) * w;
    Arena t = tape_arena(tape, sr_tape_need(net, eh, ew));
    Run rt{net, &t, nullptr, net->parts, false};
    SrPlan m;
    sr_tape_maps(rt, eh, ew, m);
    Arena a;
    const size_t need = sr_backward_need(net, eh, ew);
    SURS_REQUIRE(workspace_arena(workspace, workspace_bytes, need - 256, a), "super_res_backward: workspace too small: %zu bytes needed", need);
    Run r{net, &a, as_stream(stream), net->parts, false};
    SrBack k{r, params, grads, accumulate ? 1 : 0};
    sr_backward(k, m, g_img_sr, g_feature_lr, g_im_feat_hr);
    return r.rc;
}

// ---------------------------------------------------------------- hourglass gradients (include/surs.h)
// surs_encoder_convblock_train / surs_encoder_hourglass_train run conv_block() / hourglass() above with a tape: the separate-sum
// form - the launches of the host mirror (encoder.py) for an input without statistics - with EVERY map kept (BlockTape).  THE
// LAYOUT OF THE TAPE IS THE ORDER OF THE ARENA TAKES OF THAT ONE SEQUENCING: the backward finds the addresses by running it without
// launches (hg_layout()), a function of the net and the size alone.
namespace {

struct HgBack {
    Run &r;
    int acc;
    Map G, A, T;               // a block's scratch: its gradient (the slices take the inner gradients), relu(norm(x)), d / d that
    void *wws = nullptr;       // the weight gradient's slabs
    size_t wws_bytes = 0;
    void *gws = nullptr;       // the GroupNorm gradient's parts
    size_t gws_bytes = 0;

    void alloc(int h, int w) {
        G = r.map(h, w, 256); A = r.map(h, w, 256); T = r.map(h, w, 256);
        wws_bytes = surs_conv_grad_weight_workspace_bytes(h, w, 256, 128, 3);
        wws = r.a->take(wws_bytes);
        gws_bytes = surs_groupnorm_relu_grad_workspace_bytes(h * w, 256);
        gws = r.a->take(gws_bytes);
    }
    void copy(const Map &src, const Map &dst) {   // dense map -> dense map
        if (r.dry || r.rc) return;
        if (hipMemcpyAsync(dst.p, src.p, sizeof(float) * src.h * src.w * src.c, hipMemcpyDeviceToDevice, r.st) != hipSuccess)
            r.fail(fail(SURS_E_HIP, "hourglass gradients: hipMemcpyAsync failed"));
    }
    // g = d L / d (the block's output), dense -> dx = d L / d (its input), dense, replaced; the parameters' gradients
    void block(const BlockTape &t, const SursHgBlockParams &P, const SursHgBlockParams &D, const Map &g, const Map &dx) {
        if (r.dry || r.rc) return;
        const int h = t.x.h, w = t.x.w, hw = h * w;
        const Map Gm = input_map(G.p, h, w, 256, 256);
        copy(g, dx);    // the identity path
        copy(g, Gm);
        const Map ins[3] = {t.x, t.cat.slice(0, 128), t.cat.slice(128, 64)};
        const int c0[3] = {0, 128, 192}, cout[3] = {128, 64, 64};
        for (int k = 2; k >= 0 && !r.rc; --k) {
            const int cin = ins[k].c;
            const Map a = input_map(A.p, h, w, cin, cin), d = input_map(T.p, h, w, cin, cin);
            const Map gk = Gm.slice(c0[k], cout[k]);
            r.fail(surs_scale_shift_act(ins[k].p, hw, cin, ins[k].ld, t.nt[k].scale, t.nt[k].shift, 1, a.p, a.ld, r.st));
            if (!r.rc)
                r.fail(surs_conv_grad_weight(gk.p, h, w, cout[k], gk.ld, nullptr, 0, 1.0f, a.p, h, w, cin, a.ld, 3, 1, D.weight[k], nullptr, acc,
                                             wws, wws_bytes, r.st));
            if (!r.rc)
                r.fail(surs_conv_grad_input(gk.p, h, w, cout[k], gk.ld, nullptr, 0, 1.0f, P.weight[k], cin, 3, 1, d.p, h, w, d.ld, 0, r.st));
            // into the gradient of the map this norm read: slice [0, 128) / [128, 192) of the block's gradient, or the input's
            const Map into = k == 0 ? dx : Gm.slice(c0[k - 1], cout[k - 1]);
            if (!r.rc)
                r.fail(surs_groupnorm_relu_grad(d.p, d.ld, ins[k].p, ins[k].ld, hw, cin, t.nt[k].mean, t.nt[k].rstd, t.nt[k].scale,
                                                t.nt[k].shift, P.gamma[k], into.p, into.ld, 1, D.gamma[k], D.beta[k], acc, gws, gws_bytes, r.st));
        }
    }
};

// hourglass() in reverse; tape: the stack's blocks as the forward recorded them
void hourglass_backward(HgBack &k, const BlockTape *tape, int depth, const SursHgBlockParams *P, const SursHgBlockParams *D, const Map &g,
                        const Map &dx) {
    struct Bwd {
        HgBack &k; const BlockTape *tape; const SursHgBlockParams *P, *D;
        HgLevel lv[HG_MAX_DEPTH + 1];
        void block(int i, const Map &g, const Map &dinp) { k.block(tape[i], P[i], D[i], g, dinp); }
        void run(int level, const Map &g, const Map &dinp) {
            Run &r = k.r;
            const HgLevel &l = lv[level];
            Map p = r.map(g.h / 2, g.w / 2, 256), q = r.map(g.h / 2, g.w / 2, 256);
            block(l.b1, g, dinp);
            if (!r.dry && !r.rc) r.fail(surs_bicubic_up2_grad(g.p, p.h, p.w, 256, g.ld, p.p, p.ld, 0, r.st));
            block(l.b3, p, q);
            if (level > 1) run(level - 1, q, p);
            else block(l.b2_plus, q, p);
            block(l.b2, p, q);
            if (!r.dry && !r.rc) r.fail(surs_avgpool2_grad(q.p, q.h, q.w, 256, q.ld, dinp.p, dinp.ld, 1, r.st));
        }
    } b{k, tape, P, D};
    hg_levels(depth, b.lv);
    b.run(depth, g, dx);
}

bool is_hg_block(const SursConvBlock &b) {
    auto is = [](const SursConv &c, int cin, int cout) { return c.cin == cin && c.cout == cout && c.ksize == 3 && c.w_split && !c.bias; };
    return is(b.conv[0], 256, 128) && is(b.conv[1], 128, 64) && is(b.conv[2], 64, 64) && b.bn[0].gamma && b.bn[0].beta && b.bn[1].gamma &&
           b.bn[1].beta && b.bn[2].gamma && b.bn[2].beta;
}

int check_hg_train(const SursEncoderNet *net, int h, int w, int depth) {
    SURS_REQUIRE(net, "null network");
    SURS_REQUIRE(!((net->flags & SURS_ENC_EXTENDED) && net->norm == SURS_NORM_BATCH), "hourglass gradients: --norm group only");
    if (int rc = check_net(net)) return rc;
    SURS_REQUIRE(net->parts == 2, "hourglass gradients: net->parts == 1 (the f16 encoder) has no backward: training runs the fp32-grade "
                                  "forward (parts == 2)");
    SURS_REQUIRE(h > 0 && w > 0 && h % (1 << depth) == 0 && w % (1 << depth) == 0 && (long long)h * w < (1ll << 22),
                 "hourglass gradients: a %d x %d map is not a multiple of 2^%d (or too large)", h, w, depth);
    return 0;
}

bool hg_params_filled(const SursHgBlockParams *p, int count) {
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k)
            if (!p[i].weight[k] || !p[i].gamma[k] || !p[i].beta[k]) return false;
    return true;
}

// the tape of a block (depth 0) or of a stack's hourglass: the input's copy, then the sequencing's maps
struct HgLayout {
    Map x, out;
    BlockTape blocks[HG_MAX_BLOCKS];   // in the order of the net's block array
};

// x (pitch ld): the input, copied into the tape in front of the launches; a run without launches lays the tape out
void hg_layout(Run &r, const SursConvBlock *blocks, int depth, int h, int w, HgLayout &L, const float *x = nullptr, int ld = 0) {
    L.x = r.map(h, w, 256);
    if (!r.dry && hipMemcpy2DAsync(L.x.p, sizeof(float) * 256, x, sizeof(float) * ld, sizeof(float) * 256, (size_t)h * w,
                                   hipMemcpyDeviceToDevice, r.st) != hipSuccess)
        r.fail(fail(SURS_E_HIP, "hourglass gradients: hipMemcpy2DAsync failed"));
    if (depth == 0) L.out = conv_block(r, blocks[0], L.x, false, &L.blocks[0]);
    else L.out = hourglass(r, blocks, depth, L.x, nullptr, L.blocks);
}

size_t hg_tape_need(const SursEncoderNet *net, const SursConvBlock *blocks, int depth, int h, int w) {
    Dry d(net);
    HgLayout L;
    hg_layout(d.r, blocks, depth, h, w, L);
    return align_up(d.a.peak, 256);
}

void hg_back_all(HgBack &k, const HgLayout &L, int depth, const SursHgBlockParams *P, const SursHgBlockParams *D, const Map &g, const Map &dx) {
    k.alloc(dx.h, dx.w);
    if (depth == 0) k.block(L.blocks[0], P[0], D[0], g, dx);
    else hourglass_backward(k, L.blocks, depth, P, D, g, dx);
}

size_t hg_backward_need(const SursEncoderNet *net, int depth, int h, int w) {
    Dry d(net);
    HgBack k{d.r, 0};
    HgLayout L;
    const SursHgBlockParams none[HG_MAX_BLOCKS] = {};   // (a run without launches reads no tape and no parameter)
    const Map g = input_map(nullptr, h, w, 256, 256);
    hg_back_all(k, L, depth, none, none, g, g);
    return align_up(d.a.peak, 256) + 256;
}

int hg_train(const SursEncoderNet *net, const SursConvBlock *blocks, int depth, const float *x, int h, int w, int ld, float *out, void *tape,
             size_t tape_bytes, void *stream, const char *what) {
    for (int i = 0; i < (depth ? 3 * depth + 1 : 1); ++i)
        SURS_REQUIRE(is_hg_block(blocks[i]), "%s: the block is not image_filter_lr's (3 x 3, 256 -> 128 / 64 / 64, no bias, GroupNorm)", what);
    SURS_REQUIRE(x && out && tape, "%s: null argument", what);
    SURS_REQUIRE(ld >= 256, "%s: a map of 256 channels", what);
    SURS_REQUIRE(((size_t)tape & 255) == 0, "%s: the tape must be 256-byte aligned", what);
    const size_t need = hg_tape_need(net, blocks, depth, h, w);
    SURS_REQUIRE(need <= tape_bytes, "%s: tape too small: %zu bytes needed", what, need);
    Arena a = tape_arena(tape, tape_bytes);
    Run r{net, &a, as_stream(stream), net->parts, false};
    HgLayout L;
    hg_layout(r, blocks, depth, h, w, L, x, ld);
    if (r.rc) return r.rc;
    SURS_HIP_CHECK(hipMemcpyAsync(out, L.out.p, sizeof(float) * h * w * 256, hipMemcpyDeviceToDevice, r.st));
    return 0;
}

int hg_backward(const SursEncoderNet *net, const SursConvBlock *blocks, int depth, const SursHgBlockParams *params, const void *tape, int h,
                int w, const float *g, float *dx, const SursHgBlockParams *grads, int accumulate, void *workspace, size_t workspace_bytes,
                void *stream, const char *what) {
    const int count = depth ? 3 * depth + 1 : 1;
    for (int i = 0; i < count; ++i)
        SURS_REQUIRE(is_hg_block(blocks[i]), "%s: the block is not image_filter_lr's (3 x 3, 256 -> 128 / 64 / 64, no bias, GroupNorm)", what);
    SURS_REQUIRE(params && grads && tape && g && dx && workspace, "%s: null argument", what);
    SURS_REQUIRE(hg_params_filled(params, count) && hg_params_filled(grads, count), "%s: a null pointer in params / grads", what);
    SURS_REQUIRE(((size_t)tape & 255) == 0 && aligned16(g) && aligned16(dx), "%s: the tape must be 256-byte aligned, the maps 16-byte", what);
    Arena t = tape_arena(tape, hg_tape_need(net, blocks, depth, h, w));
    Run rt{net, &t, nullptr, net->parts, true};   // (no launches: the addresses)
    HgLayout L;
    hg_layout(rt, blocks, depth, h, w, L);
    Arena a;
    const size_t need = hg_backward_need(net, depth, h, w);
    SURS_REQUIRE(workspace_arena(workspace, workspace_bytes, need - 256, a), "%s: workspace too small: %zu bytes needed", what, need);
    Run r{net, &a, as_stream(stream), net->parts, false};
    HgBack k{r, accumulate ? 1 : 0};
    hg_back_all(k, L, depth, params, grads, input_map(g, h, w, 256, 256), input_map(dx, h, w, 256, 256));
    return r.rc;
}

const SursConvBlock *stack_blocks(const SursEncoderNet *net, int stack) { return net->hg + (size_t)stack * per_stack_blocks(net); }

}  // namespace

extern "C" size_t surs_encoder_convblock_tape_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_hg_train(net, h, w, 0) || !is_hg_block(net->conv2)) return 0;
    return hg_tape_need(net, &net->conv2, 0, h, w);
}

extern "C" size_t surs_encoder_convblock_backward_workspace_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_hg_train(net, h, w, 0)) return 0;
    return hg_backward_need(net, 0, h, w);
}

extern "C" size_t surs_encoder_hourglass_tape_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_hg_train(net, h, w, net->hg_depth) || !net->hg) return 0;
    for (int i = 0; i < per_stack_blocks(net); ++i)
        if (!is_hg_block(net->hg[i])) return 0;
    return hg_tape_need(net, net->hg, net->hg_depth, h, w);
}

extern "C" size_t surs_encoder_hourglass_backward_workspace_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_hg_train(net, h, w, net->hg_depth)) return 0;
    return hg_backward_need(net, net->hg_depth, h, w);
}

extern "C" int surs_encoder_convblock_train(const SursEncoderNet *net, const SursConvBlock *block, const float *x, int h, int w, int ld,
                                            float *out, void *tape, size_t tape_bytes, void *stream) {
    SURS_REQUIRE(net && block, "convblock_train: null argument");
    if (int rc = check_hg_train(net, h, w, 0)) return rc;
    return hg_train(net, block, 0, x, h, w, ld, out, tape, tape_bytes, stream, "convblock_train");
}

extern "C" int surs_encoder_convblock_backward(const SursEncoderNet *net, const SursConvBlock *block, const SursHgBlockParams *params,
                                               const void *tape, int h, int w, const float *g, float *dx, const SursHgBlockParams *grads,
                                               int accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    SURS_REQUIRE(net && block, "convblock_backward: null argument");
    if (int rc = check_hg_train(net, h, w, 0)) return rc;
    return hg_backward(net, block, 0, params, tape, h, w, g, dx, grads, accumulate, workspace, workspace_bytes, stream, "convblock_backward");
}

extern "C" int surs_encoder_hourglass_train(const SursEncoderNet *net, int stack, const float *x, int h, int w, int ld, float *out,
                                            void *tape, size_t tape_bytes, void *stream) {
    SURS_REQUIRE(net && net->hg, "hourglass_train: null argument");
    if (int rc = check_hg_train(net, h, w, net->hg_depth)) return rc;
    SURS_REQUIRE(stack >= 0 && stack < net->num_stack, "hourglass_train: stack %d of %d", stack, net->num_stack);
    return hg_train(net, stack_blocks(net, stack), net->hg_depth, x, h, w, ld, out, tape, tape_bytes, stream, "hourglass_train");
}

extern "C" int surs_encoder_hourglass_backward(const SursEncoderNet *net, int stack, const SursHgBlockParams *params, const void *tape, int h,
                                               int w, const float *g, float *dx, const SursHgBlockParams *grads, int accumulate,
                                               void *workspace, size_t workspace_bytes, void *stream) {
    SURS_REQUIRE(net && net->hg, "hourglass_backward: null argument");
    if (int rc = check_hg_train(net, h, w, net->hg_depth)) return rc;
    SURS_REQUIRE(stack >= 0 && stack < net->num_stack, "hourglass_backward: stack %d of %d", stack, net->num_stack);
    return hg_backward(net, stack_blocks(net, stack), net->hg_depth, params, tape, h, w, g, dx, grads, accumulate, workspace, workspace_bytes,
                       stream, "hourglass_backward");
}

// ---------------------------------------------------------------- stack-tail gradients, and the whole low-resolution filter (include/surs.h)
// surs_encoder_tail_train runs stack_tail() above with a tape; surs_encoder_filter_lr_train runs conv_block(), hourglass() and
// stack_tail() in filter_lr()'s order on ONE tape (one stream, the separate-sum forms, every map kept).  As for the hourglass, the
// layout of a tape is the order of the arena takes of that sequencing, and the backwards find the addresses by running it dry.
namespace {

bool is_pointwise(const SursConv &c, int cin, int cout) { return c.cin == cin && c.cout == cout && c.ksize == 1 && c.w_split; }

int check_tail(const SursEncoderNet *net, int s, const char *what) {
    SURS_REQUIRE(net->conv_last && net->l && net->bn_end, "%s: null argument", what);
    SURS_REQUIRE(s >= 0 && s < net->num_stack, "%s: stack %d of %d", what, s, net->num_stack);
    const int d = net->l[s].cout;
    SURS_REQUIRE(d >= 16 && d <= 512 && d % 16 == 0, "hg_dim %d: the supported values are the multiples of 16 from 16 to 512", d);
    SURS_REQUIRE(is_pointwise(net->conv_last[s], 256, 256) && is_pointwise(net->l[s], 256, d) && net->bn_end[s].gamma && net->bn_end[s].beta &&
                 (s == net->num_stack - 1 || (net->next && is_pointwise(net->next[s], 256, 256))),
                 "%s: the tail of stack %d is not image_filter_lr's (1 x 1, 256 -> 256 -> hg_dim, GroupNorm)", what, s);
    return 0;
}

bool tail_param_filled(const SursHgTailParams &p, bool last) {
    return p.conv_last.weight && p.conv_last.bias && p.l.weight && p.l.bias && p.gamma && p.beta &&
           (last || (p.bl.weight && p.bl.bias && p.al.weight && p.al.bias));
}

// the tape of a tail: the input's copy, the stack's output, then the sequencing's maps
struct TailLayout {
    Map ll, out, next;
    TailTape T;
};

void tail_layout(Run &r, int s, int h, int w, TailLayout &L, const float *ll = nullptr, int ld = 0, const float *previous = nullptr,
                 int previous_ld = 0) {
    const SursEncoderNet &n = *r.net;
    L.ll = r.map(h, w, 256);
    if (!r.dry && hipMemcpy2DAsync(L.ll.p, sizeof(float) * 256, ll, sizeof(float) * ld, sizeof(float) * 256, (size_t)h * w,
                                   hipMemcpyDeviceToDevice, r.st) != hipSuccess)
        r.fail(fail(SURS_E_HIP, "stack-tail gradients: hipMemcpy2DAsync failed"));
    L.out = r.map(h, w, n.l[s].cout);
    L.next = stack_tail(r, s, L.ll, input_map(previous, h, w, 256, previous_ld), L.out, s == n.num_stack - 1, &L.T);
}

size_t tail_tape_need(const SursEncoderNet *net, int s, int h, int w) {
    Dry d(net);
    TailLayout L;
    tail_layout(d.r, s, h, w, L);
    return align_up(d.a.peak, 256);
}

struct TailBack {
    Run &r;
    int acc;
    Map A, DA, DO, DT;         // relu(bn_end(t)), d / d that, d / d out (the joint's), d / d t
    void *wws = nullptr;       // the weight gradients' slabs
    size_t wws_bytes = 0;
    void *gws = nullptr;       // the GroupNorm gradient's parts
    size_t gws_bytes = 0;

    void alloc(int h, int w, int d) {
        A = r.map(h, w, 256); DA = r.map(h, w, 256); DO = r.map(h, w, d); DT = r.map(h, w, 256);
        const int m = d > 256 ? d : 256;
        wws_bytes = surs_conv_grad_weight_workspace_bytes(h, w, m, m, 1);
        wws = r.a->take(wws_bytes);
        gws_bytes = surs_groupnorm_relu_grad_workspace_bytes(h * w, 256);
        gws = r.a->take(gws_bytes);
    }
    void wgrad(const Map &g, const Map &x, const SursSrParam &d) {
        if (!r.rc)
            r.fail(surs_conv_grad_weight(g.p, g.h, g.w, g.c, g.ld, nullptr, 0, 1.0f, x.p, x.h, x.w, x.c, x.ld, 1, 1, d.weight, d.bias, acc, wws,
                                         wws_bytes, r.st));
    }
    void zero(float *p, size_t count) {
        if (!r.rc && hipMemsetAsync(p, 0, sizeof(float) * count, r.st) != hipSuccess)
            r.fail(fail(SURS_E_HIP, "stack-tail gradients: hipMemsetAsync failed"));
    }
    // g_out = d L / d out, g_next = d L / d next (a map without memory counts as zero; not both) -> d_ll (dense, replaced) and the
    // parameters' gradients, in the order of include/surs.h
    void run(const TailTape &t, bool last, const SursHgTailParams &P, const SursHgTailParams &D, const Map &g_out, const Map &g_next,
             const Map &d_ll) {
        if (r.dry || r.rc) return;
        const int h = t.t.h, w = t.t.w, hw = h * w, d = t.out.c;
        const Map a = input_map(A.p, h, w, 256, 256), da = input_map(DA.p, h, w, 256, 256), dt = input_map(DT.p, h, w, 256, 256);
        const Map dout = input_map(DO.p, h, w, d, d);
        r.fail(surs_scale_shift_act(t.t.p, hw, 256, t.t.ld, t.nt.scale, t.nt.shift, 1, a.p, a.ld, r.st));
        if (!r.rc)
            r.fail(surs_tail_joint_grad(g_out.p, g_out.ld, g_next.p, g_next.ld, P.al.weight, P.l.weight, P.bl.weight, hw, d, dout.p, dout.ld,
                                        da.p, da.ld, r.st));
        if (g_next.p) {
            wgrad(g_next, t.out, D.al);
            wgrad(g_next, a, D.bl);
        } else if (!last && !acc) {   // next reaches nothing: bl and al get zero gradients
            zero(D.al.weight, (size_t)256 * d); zero(D.al.bias, 256); zero(D.bl.weight, 256 * 256); zero(D.bl.bias, 256);
        }
        wgrad(dout, a, D.l);
        if (!r.rc)
            r.fail(surs_groupnorm_relu_grad(da.p, da.ld, t.t.p, t.t.ld, hw, 256, t.nt.mean, t.nt.rstd, t.nt.scale, t.nt.shift, P.gamma, dt.p, dt.ld,
                                            0, D.gamma, D.beta, acc, gws, gws_bytes, r.st));
        wgrad(dt, t.ll, D.conv_last);
        if (!r.rc)
            r.fail(surs_conv_grad_input(dt.p, h, w, 256, dt.ld, nullptr, 0, 1.0f, P.conv_last.weight, 256, 1, 1, d_ll.p, h, w, d_ll.ld, 0, r.st));
    }
};

size_t tail_backward_need(const SursEncoderNet *net, int s, int h, int w) {
    Dry d(net);
    TailBack k{d.r, 0};
    k.alloc(h, w, net->l[s].cout);
    return align_up(d.a.peak, 256) + 256;
}

// ---- the whole filter: conv2, then per stack hourglass -> top_m -> tail, on one tape
constexpr int MAX_STACKS = 16;
struct FilterLayout {
    Map x, outs[MAX_STACKS];
    BlockTape conv2, top_m[MAX_STACKS], hg[MAX_STACKS][HG_MAX_BLOCKS];
    TailTape tail[MAX_STACKS];
};

void filter_layout(Run &r, int h, int w, FilterLayout &L, const float *x = nullptr, int ld = 0) {
    const SursEncoderNet &n = *r.net;
    L.x = r.map(h, w, 256);
    if (!r.dry && hipMemcpy2DAsync(L.x.p, sizeof(float) * 256, x, sizeof(float) * ld, sizeof(float) * 256, (size_t)h * w,
                                   hipMemcpyDeviceToDevice, r.st) != hipSuccess)
        r.fail(fail(SURS_E_HIP, "filter_lr gradients: hipMemcpy2DAsync failed"));
    Map previous = conv_block(r, n.conv2, L.x, true, &L.conv2);
    for (int s = 0; s < n.num_stack; ++s) {
        const bool last = s == n.num_stack - 1;
        Map hg = hourglass(r, n.hg + (size_t)s * per_stack_blocks(&n), n.hg_depth, previous, nullptr, L.hg[s]);
        Map ll = conv_block(r, n.top_m[s], hg, false, &L.top_m[s]);
        L.outs[s] = r.map(h, w, n.l[s].cout);
        const Map nx = stack_tail(r, s, ll, previous, L.outs[s], last, &L.tail[s]);
        if (!last) previous = nx;
    }
}

int check_filter_train(const SursEncoderNet *net, int h, int w, const char *what) {
    if (int rc = check_hg_train(net, h, w, net ? net->hg_depth : 0)) return rc;
    SURS_REQUIRE(net->hg && net->top_m, "%s: null argument", what);
    for (int s = 0; s < net->num_stack; ++s) {
        if (int rc = check_tail(net, s, what)) return rc;
        SURS_REQUIRE(is_hg_block(net->top_m[s]), "%s: a block is not image_filter_lr's", what);
        for (int i = 0; i < per_stack_blocks(net); ++i)
            SURS_REQUIRE(is_hg_block(net->hg[(size_t)s * per_stack_blocks(net) + i]), "%s: a block is not image_filter_lr's", what);
    }
    SURS_REQUIRE(is_hg_block(net->conv2), "%s: a block is not image_filter_lr's", what);
    return 0;
}

size_t filter_tape_need(const SursEncoderNet *net, int h, int w) {
    Dry d(net);
    std::unique_ptr<FilterLayout> L(new FilterLayout);
    filter_layout(d.r, h, w, *L);
    return align_up(d.a.peak, 256);
}

struct FilterBack {
    Run &r;
    int acc;
    HgBack k;
    TailBack tb;
    Map dll, dhg, dprev[2];

    FilterBack(Run &run, int accumulate) : r(run), acc(accumulate), k{run, accumulate}, tb{run, accumulate} {}
    void alloc(int h, int w) {
        int d = 0;
        for (int s = 0; s < r.net->num_stack; ++s) d = r.net->l[s].cout > d ? r.net->l[s].cout : d;
        k.alloc(h, w);
        tb.alloc(h, w, d);
        dll = r.map(h, w, 256); dhg = r.map(h, w, 256); dprev[0] = r.map(h, w, 256); dprev[1] = r.map(h, w, 256);
    }
    void zero_block(const SursHgBlockParams &D) {
        const size_t wn[3] = {128 * 256 * 9, 64 * 128 * 9, 64 * 64 * 9}, cn[3] = {256, 128, 64};
        for (int j = 0; j < 3; ++j) {
            tb.zero(D.weight[j], wn[j]); tb.zero(D.gamma[j], cn[j]); tb.zero(D.beta[j], cn[j]);
        }
    }
    // g_outs[s] = d L / d outs[s] (NULL: zero) -> d_x = d L / d feature_lr and every parameter's gradient.  Stack s, from the last:
    // tail (g_outs[s], d previous_{s+1}), top_m, hourglass; d previous_s = the hourglass's input gradient + d next_s (one fp32 sum)
    void run(const FilterLayout &L, const SursHgFilterParams &P, const SursHgFilterParams &D, const float *const *g_outs, const Map &d_x) {
        const SursEncoderNet &n = *r.net;
        const int S = n.num_stack, per = per_stack_blocks(&n), h = d_x.h, w = d_x.w;
        Map gnext;   // d L / d previous_{s + 1}; without memory: zero
        for (int s = S - 1; s >= 0; --s) {
            const bool last = s == S - 1;
            const int d = n.l[s].cout;
            const Map g_out = g_outs[s] ? input_map(g_outs[s], h, w, d, d) : Map();
            if (!g_out.p && !gnext.p) {   // nothing reaches this stack: zero gradients, and none for previous_s
                if (!acc && !r.dry) {
                    const SursHgTailParams &T = D.tail[s];
                    tb.zero(T.conv_last.weight, 256 * 256); tb.zero(T.conv_last.bias, 256); tb.zero(T.gamma, 256); tb.zero(T.beta, 256);
                    tb.zero(T.l.weight, (size_t)d * 256); tb.zero(T.l.bias, d);
                    if (!last) {
                        tb.zero(T.al.weight, (size_t)256 * d); tb.zero(T.al.bias, 256); tb.zero(T.bl.weight, 256 * 256); tb.zero(T.bl.bias, 256);
                    }
                    zero_block(D.top_m[s]);
                    for (int i = 0; i < per; ++i) zero_block(D.hg[(size_t)s * per + i]);
                }
                continue;
            }
            const Map &dp = dprev[s & 1];
            tb.run(L.tail[s], last, P.tail[s], D.tail[s], g_out, gnext, dll);
            k.block(L.top_m[s], P.top_m[s], D.top_m[s], dll, dhg);
            const size_t mark = r.a->off;   // (the levels' maps are taken per call)
            hourglass_backward(k, L.hg[s], n.hg_depth, P.hg + (size_t)s * per, D.hg + (size_t)s * per, dhg, dp);
            r.a->off = mark;
            if (gnext.p && !r.dry && !r.rc) r.fail(surs_add3(dp.p, dp.ld, gnext.p, gnext.ld, nullptr, 0, h * w, 256, dp.p, dp.ld, r.st));
            gnext = dp;
        }
        k.block(L.conv2, P.conv2, D.conv2, gnext, d_x);
    }
};

size_t filter_backward_need(const SursEncoderNet *net, int h, int w) {
    Dry d(net);
    FilterBack k(d.r, 0);
    std::unique_ptr<FilterLayout> L(new FilterLayout);
    const std::vector<SursHgBlockParams> blocks((size_t)net->num_stack * per_stack_blocks(net));
    const std::vector<SursHgTailParams> tails(net->num_stack);
    const SursHgFilterParams none = {SursHgBlockParams{}, blocks.data(), blocks.data(), tails.data()};
    float *g[MAX_STACKS];
    for (int s = 0; s < MAX_STACKS; ++s) g[s] = NOWHERE;
    k.alloc(h, w);
    k.run(*L, none, none, g, input_map(NOWHERE, h, w, 256, 256));
    return align_up(d.a.peak, 256) + 256;
}

}  // namespace

extern "C" size_t surs_encoder_tail_tape_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_hg_train(net, h, w, 0)) return 0;
    size_t need = 0;
    for (int s = 0; s < net->num_stack; ++s) {   // (the last stack's is the smaller one)
        if (check_tail(net, s, "tail_tape_bytes")) return 0;
        const size_t v = tail_tape_need(net, s, h, w);
        need = v > need ? v : need;
    }
    return need;
}

extern "C" size_t surs_encoder_tail_backward_workspace_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_hg_train(net, h, w, 0)) return 0;
    size_t need = 0;
    for (int s = 0; s < net->num_stack; ++s) {
        if (check_tail(net, s, "tail_backward_workspace_bytes")) return 0;
        const size_t v = tail_backward_need(net, s, h, w);
        need = v > need ? v : need;
    }
    return need;
}

extern "C" int surs_encoder_tail_train(const SursEncoderNet *net, int stack, const float *ll, int ll_ld, const float *previous, int previous_ld,
                                       int h, int w, float *out, float *next, void *tape, size_t tape_bytes, void *stream) {
    if (int rc = check_hg_train(net, h, w, 0)) return rc;
    if (int rc = check_tail(net, stack, "tail_train")) return rc;
    const bool last = stack == net->num_stack - 1;
    SURS_REQUIRE(ll && out && tape, "tail_train: null argument");
    SURS_REQUIRE(last ? (!previous && !next) : (previous && next), "tail_train: previous and next go with every stack but the last (stack %d of %d)",
                 stack, net->num_stack);
    SURS_REQUIRE(ll_ld >= 256 && (last || (previous_ld >= 256 && previous_ld % 4 == 0 && aligned16(previous))),
                 "tail_train: maps of 256 channels, 16-byte aligned pixels");
    SURS_REQUIRE(((size_t)tape & 255) == 0, "tail_train: the tape must be 256-byte aligned");
    const size_t need = tail_tape_need(net, stack, h, w);
    SURS_REQUIRE(need <= tape_bytes, "tail_train: tape too small: %zu bytes needed", need);
    Arena a = tape_arena(tape, tape_bytes);
    Run r{net, &a, as_stream(stream), net->parts, false};
    TailLayout L;
    tail_layout(r, stack, h, w, L, ll, ll_ld, previous, previous_ld);
    if (r.rc) return r.rc;
    SURS_HIP_CHECK(hipMemcpyAsync(out, L.out.p, sizeof(float) * h * w * L.out.c, hipMemcpyDeviceToDevice, r.st));
    if (!last) SURS_HIP_CHECK(hipMemcpyAsync(next, L.next.p, sizeof(float) * h * w * 256, hipMemcpyDeviceToDevice, r.st));
    return 0;
}

extern "C" int surs_encoder_tail_backward(const SursEncoderNet *net, int stack, const SursHgTailParams *params, const void *tape, int h, int w,
                                          const float *g_out, const float *g_next, float *d_ll, const SursHgTailParams *grads, int accumulate,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_hg_train(net, h, w, 0)) return rc;
    if (int rc = check_tail(net, stack, "tail_backward")) return rc;
    const bool last = stack == net->num_stack - 1;
    SURS_REQUIRE(params && grads && tape && d_ll && workspace, "tail_backward: null argument");
    SURS_REQUIRE(g_out || g_next, "tail_backward: both gradients are missing");
    SURS_REQUIRE(!(last && g_next), "tail_backward: the last stack has no next");
    SURS_REQUIRE(tail_param_filled(*params, last) && tail_param_filled(*grads, last), "tail_backward: a null pointer in params / grads");
    SURS_REQUIRE(((size_t)tape & 255) == 0 && aligned16(g_out) && aligned16(g_next) && aligned16(d_ll),
                 "tail_backward: the tape must be 256-byte aligned, the maps 16-byte");
    Arena t = tape_arena(tape, tail_tape_need(net, stack, h, w));
    Run rt{net, &t, nullptr, net->parts, true};   // (no launches: the addresses)
    TailLayout L;
    tail_layout(rt, stack, h, w, L);
    Arena a;
    const size_t need = tail_backward_need(net, stack, h, w);
    SURS_REQUIRE(workspace_arena(workspace, workspace_bytes, need - 256, a), "tail_backward: workspace too small: %zu bytes needed", need);
    Run r{net, &a, as_stream(stream), net->parts, false};
    TailBack k{r, accumulate ? 1 : 0};
    const int d = net->l[stack].cout;
    k.alloc(h, w, d);
    k.run(L.T, last, *params, *grads, input_map(g_out, h, w, d, d), input_map(g_next, h, w, 256, 256), input_map(d_ll, h, w, 256, 256));
    return r.rc;
}

extern "C" size_t surs_encoder_filter_lr_tape_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_filter_train(net, h, w, "filter_lr_tape_bytes")) return 0;
    return filter_tape_need(net, h, w);
}

extern "C" size_t surs_encoder_filter_lr_backward_workspace_bytes(const SursEncoderNet *net, int h, int w) {
    if (!net || check_filter_train(net, h, w, "filter_lr_backward_workspace_bytes")) return 0;
    return filter_backward_need(net, h, w);
}

extern "C" int surs_encoder_filter_lr_train(const SursEncoderNet *net, const float *feature_lr, int h, int w, int ld, float *const *outs,
                                            void *tape, size_t tape_bytes, void *stream) {
    if (int rc = check_filter_train(net, h, w, "filter_lr_train")) return rc;
    SURS_REQUIRE(feature_lr && outs && tape, "filter_lr_train: null argument");
    for (int s = 0; s < net->num_stack; ++s) SURS_REQUIRE(outs[s], "filter_lr_train: training keeps every stack's output");
    SURS_REQUIRE(ld >= 256, "filter_lr_train: a map of 256 channels");
    SURS_REQUIRE(((size_t)tape & 255) == 0, "filter_lr_train: the tape must be 256-byte aligned");
    const size_t need = filter_tape_need(net, h, w);
    SURS_REQUIRE(need <= tape_bytes, "filter_lr_train: tape too small: %zu bytes needed", need);
    Arena a = tape_arena(tape, tape_bytes);
    Run r{net, &a, as_stream(stream), net->parts, false};
    std::unique_ptr<FilterLayout> L(new FilterLayout);
    filter_layout(r, h, w, *L, feature_lr, ld);
    if (r.rc) return r.rc;
    for (int s = 0; s < net->num_stack; ++s)
        SURS_HIP_CHECK(hipMemcpyAsync(outs[s], L->outs[s].p, sizeof(float) * h * w * L->outs[s].c, hipMemcpyDeviceToDevice, r.st));
    return 0;
}

extern "C" int surs_encoder_filter_lr_backward(const SursEncoderNet *net, const SursHgFilterParams *params, const void *tape, int h, int w,
                                               const float *const *g_outs, float *d_feature_lr, const SursHgFilterParams *grads,
                                               int accumulate, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_filter_train(net, h, w, "filter_lr_backward")) return rc;
    SURS_REQUIRE(params && grads && tape && g_outs && d_feature_lr && workspace, "filter_lr_backward: null argument");
    const int S = net->num_stack, per = per_stack_blocks(net);
    bool any = false;
    for (int s = 0; s < S; ++s) {
        any = any || g_outs[s];
        SURS_REQUIRE(aligned16(g_outs[s]), "filter_lr_backward: the maps must be 16-byte aligned");
    }
    SURS_REQUIRE(any, "filter_lr_backward: every gradient is missing");
    for (const SursHgFilterParams *p : {params, grads}) {
        SURS_REQUIRE(p->hg && p->top_m && p->tail && hg_params_filled(&p->conv2, 1) && hg_params_filled(p->hg, S * per) &&
                     hg_params_filled(p->top_m, S), "filter_lr_backward: a null pointer in params / grads");
        for (int s = 0; s < S; ++s) SURS_REQUIRE(tail_param_filled(p->tail[s], s == S - 1), "filter_lr_backward: a null pointer in params / grads");
    }
    SURS_REQUIRE(((size_t)tape & 255) == 0 && aligned16(d_feature_lr), "filter_lr_backward: the tape must be 256-byte aligned, the maps 16-byte");
    Arena t = tape_arena(tape, filter_tape_need(net, h, w));
    Run rt{net, &t, nullptr, net->parts, true};   // (no launches: the addresses)
    std::unique_ptr<FilterLayout> L(new FilterLayout);
    filter_layout(rt, h, w, *L);
    Arena a;
    const size_t need = filter_backward_need(net, h, w);
    SURS_REQUIRE(workspace_arena(workspace, workspace_bytes, need - 256, a), "filter_lr_backward: workspace too small: %zu bytes needed", need);
    Run r{net, &a, as_stream(stream), net->parts, false};
    FilterBack k(r, accumulate ? 1 : 0);
    k.alloc(h, w);
    k.run(*L, *params, *grads, g_outs, input_map(d_feature_lr, h, w, 256, 256));
    return r.rc;
}
