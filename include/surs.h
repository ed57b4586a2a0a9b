/*
 * surs.h - C ABI of the MI355X-native SuRS occupancy-query hot path.
 *
 * The reference (marcopesavento/Super-resolution-3D-Human-Shape-from-a-Single-
 * Low-Resolution-Image) is pure Python on PyTorch: it has no FFI of its own.
 * The entry points below are what a binding for this path replaces, one per
 * ATen / scikit-image call on the path:
 *
 *   surs_conv2d_nhwc          nn.Conv2d 3x3 / 1x1        lib/net_util.py:94-97, lib/model/SuRSSR_v3.py:46-138,
 *                                                        lib/model/HGFilters.py:60-64,153-174
 *   surs_groupnorm_coeffs     nn.GroupNorm(32, C) stats  lib/model/HGFilters.py:41-45,140,164
 *   surs_avgpool2             F.avg_pool2d(x,2,2)        lib/model/HGFilters.py:101
 *   surs_bicubic_up2          bicubic x2, both alignments lib/model/HGFilters.py:115, lib/model/SuRSSR_v3.py:140
 *   surs_pixel_shuffle2       PixelShuffle(2)+LeakyReLU   lib/model/SuRSSR_v3.py:111-115
 *   surs_add3                 residual adds / cat         lib/model/HGFilters.py:66-74,117,203-206
 *   surs_query_points         query_mr+query_sr+get_preds lib/model/SuRSNet.py:131-187, lib/model/BaseSuRSNet.py:80-85,
 *                                                        lib/geometry.py:4-31, lib/model/DepthNormalizer.py:18,
 *                                                        lib/model/SurfaceClassifier.py:53-81
 *   surs_query_grid           create_grid + eval_grid + eval_func  lib/sdf.py:4-52, lib/mesh_util.py:16-34
 *   surs_mc_*                 measure.marching_cubes_lewiner(sdf, 0.5)  lib/mesh_util.py:40,45
 *                             (scikit-image 0.17.2, skimage/measure/_marching_cubes_lewiner.py)
 *
 * Conventions: plain pointers and sizes, no torch types.  Unless a parameter
 * is marked HOST, every pointer is a DEVICE pointer valid on the current HIP
 * device; work is enqueued on `stream` (a hipStream_t passed as void*, NULL =
 * the null stream) and the call returns without synchronising unless stated.
 * Return value: 0 on success, a negative SURS_E_* code otherwise;
 * surs_last_error() returns a thread-local message.  No exceptions cross the
 * ABI.  Image tensors are NHWC fp32 with an explicit channel pitch (`ld`, in
 * floats, >= C) so that a channel slice of a wider tensor (the reference's
 * torch.cat) is addressed in place.
 */
#ifndef SURS_H
#define SURS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SURS_ABI_VERSION 1

enum {
    SURS_OK = 0,
    SURS_E_INVALID = -1,   /* bad argument */
    SURS_E_HIP = -2,       /* HIP runtime error (message has the hipError string) */
    SURS_E_UNSUPPORTED = -3,
    SURS_E_LEVEL_RANGE = -4, /* marching cubes: level outside [min,max]  (skimage ValueError) */
    SURS_E_NO_SURFACE = -5,  /* marching cubes: no surface              (skimage RuntimeError) */
    SURS_E_CAPACITY = -6,    /* marching cubes: output buffers too small; counts are reported */
    SURS_E_NONFINITE = -7    /* marching cubes: the volume contains NaN (counts->vmin / vmax are NaN).  skimage would go on
                                silently; here it is how an overflow of the fp32-grade sweep's f16 range surfaces */
};

enum { SURS_F32 = 0, SURS_BF16 = 1, SURS_F16 = 2,  /* arithmetic of the dense MLP contractions */
       SURS_F32_GEMM = 3 };  /* surs_query_grid only: fp32 on the per-point layer kernels (bf16 x 3 split operands: fp32's exponent
                                range) even where the fp32-grade column kernel (f16 x 2 split: |activation| < 65504) applies */

int surs_abi_version(void);
const char *surs_last_error(void);
/* number of compute units / gcn arch name of the current device (arch_out: >= 32 bytes, HOST) */
int surs_device_info(int *cu_count, char *arch_out);

/* Options: every experiment / A-B switch of the library by name, in one table (csrc/surs_api.cpp) - nothing else in the library reads
 * the environment.  An option's environment variable (SURS_<NAME>; surs_set_option accepts either spelling) is read ONCE, when the
 * table is first used, as its initial value; surs_set_option changes it at any time, process-wide.  surs_option_name(i) /
 * surs_option_help(i), i = 0, 1, ... until NULL, list them.  Defaults are the product's configuration: none of them needs setting. */
int surs_set_option(const char *name, int value);
int surs_get_option(const char *name, int *value);
const char *surs_option_name(int index);
const char *surs_option_help(int index);

/* ------------------------------------------------------------------ encoder primitives */

/* y[:, :, 0:cout] (pitch y_ld) = act( conv_k(pre(x))[...] + bias ) (+ residual)
 *   pre(x) = relu(x * in_scale[c] + in_shift[c]) if in_scale != NULL (fused GroupNorm-apply + ReLU, zero padding
 *            applied AFTER it, as nn.Conv2d pads the normalised tensor), else x.
 *   ksize 1 or 3, padding ksize/2, stride 1 or 2.  wpacked: surs_conv_pack_weights layout.  bias nullable.
 *   act: 0 none, 1 leaky-relu with `slope` (slope 0 = ReLU), applied before the residual add.
 *   residual (nullable): same spatial size as y, pitch res_ld. */
int surs_conv2d_nhwc(const float *x, int h, int w, int cin, int x_ld, const float *wpacked, const float *bias, float *y,
                     int cout, int y_ld, int ksize, int stride, const float *in_scale, const float *in_shift, int act,
                     float slope, const float *residual, int res_ld, void *stream);
/* The same 3x3 / stride-1 convolution on the bf16 matrix pipe with fp32 accuracy: every operand is split into three bf16
 * parts (exactly) and the six significant partial products are accumulated in fp32 - 2.7x the fp32 MFMA rate.
 * wsplit: surs_conv_pack_weights_x3 layout (device). */
int surs_conv2d_nhwc_x3(const float *x, int h, int w, int cin, int x_ld, const void *wsplit, const float *bias, float *y,
                        int cout, int y_ld, int ksize, int stride, const float *in_scale, const float *in_shift, int act,
                        float slope, const float *residual, int res_ld, void *stream);
/* HOST helper for it: [3 parts][k*k][cin_pad/16][cout_pad][16] uint16 (bf16).  Returns bytes (query with out == NULL). */
size_t surs_conv_pack_weights_x3(const float *w, int cout, int cin, int ksize, void *out);
/* The same convolution with every operand as TWO f16 parts (hi + lo) and three products per MAC: half the matrix work of the
 * three-part form, 22 significant bits, operands below 65504 in magnitude; the encoder's default.  wsplit:
 * surs_conv_pack_weights_x2 layout ([2 parts][k*k][cin_pad/16][cout_pad][16] uint16, f16). */
int surs_conv2d_nhwc_x2(const float *x, int h, int w, int cin, int x_ld, const void *wsplit, const float *bias, float *y,
                        int cout, int y_ld, int ksize, int stride, const float *in_scale, const float *in_shift, int act,
                        float slope, const float *residual, int res_ld, void *stream);
size_t surs_conv_pack_weights_x2(const float *w, int cout, int cin, int ksize, void *out);
/* The same entry with ONE f16 part per operand (part 0 of the surs_conv_pack_weights_x2 image) and one product per MAC in the 3x3
 * kernels: 11 significant bits - NOT fp32-grade; a third of the matrix work.  The encoder of --precision bf16, whose sweep
 * rounds the features' contributions to 8 bits anyway; held to the acceptance bounds of tests/test_gpu_precision.py.  1x1 convolutions (HBM-bound) run the two-part kernel. */
int surs_conv2d_nhwc_x1(const float *x, int h, int w, int cin, int x_ld, const void *wsplit, const float *bias, float *y,
                        int cout, int y_ld, int ksize, int stride, const float *in_scale, const float *in_shift, int act,
                        float slope, const float *residual, int res_ld, void *stream);
/* The split-operand 3x3 kernels come in two tiles (8 rows x 64 channels, 4 x 32 for maps too small to fill the chip with the
 * first) that sum their partial products in different orders.  surs_conv_tile_scale(num, den) makes the calling thread's following
 * convolutions choose the tile as if their maps were num / den times as wide: a column strip of an image then reproduces the bits
 * of the full image's columns (one rank's share of a sharded encoder).  (1, 1) restores the default. */
int surs_conv_tile_scale(int num, int den);
/* HOST helper: repack a PyTorch [cout][cin][k][k] weight into the kernel layout [k*k][cin_pad][cout_pad] (floats).
 * Returns the number of floats written (query with out == NULL). */
size_t surs_conv_pack_weights(const float *w, int cout, int cin, int ksize, float *out);

/* GroupNorm statistics folded with the affine parameters into per-channel coefficients:
 * scale[c] = gamma[c]*rstd[g(c)], shift[c] = beta[c] - mean[g]*rstd[g]*gamma[c]   (biased variance, eps). */
int surs_groupnorm_coeffs(const float *x, int hw, int c, int x_ld, int groups, float eps, const float *gamma,
                          const float *beta, float *scale, float *shift, void *stream);
/* The same with the scratch of the partial sums supplied by the caller (surs_groupnorm_scratch_bytes() bytes, device): nothing is
 * allocated inside, so the two launches can be captured into a HIP graph (hipMalloc is not permitted on a capturing stream). */
size_t surs_groupnorm_scratch_bytes(void);
int surs_groupnorm_coeffs_ws(const float *x, int hw, int c, int x_ld, int groups, float eps, const float *gamma,
                             const float *beta, float *scale, float *shift, void *scratch, void *stream);
/* y = relu?(x*scale + shift) elementwise (GroupNorm apply when it is not followed by a conv) */
int surs_scale_shift_act(const float *x, int hw, int c, int x_ld, const float *scale, const float *shift, int relu,
                         float *y, int y_ld, void *stream);
int surs_avgpool2(const float *x, int h, int w, int c, int x_ld, float *y, int y_ld, void *stream);
/* y = bicubic_x2(x) (+ addend, nullable, pitch add_ld): A=-0.75, border-clamped taps */
int surs_bicubic_up2(const float *x, int h, int w, int c, int x_ld, int align_corners, const float *addend, int add_ld,
                     float *y, int y_ld, void *stream);
/* y = bicubic(x) enlarged by the integer factor `scale` in SURS_SR_SCALE_MIN..SURS_SR_SCALE_MAX (+ addend, nullable, pitch add_ld): nn.Upsample(
 * scale_factor = scale, mode = 'bicubic') with PyTorch's arithmetic - A = -0.75, border-clamped taps, the source coordinate
 * (float)(1 / scale) * (dst + 0.5) - 0.5 as a separately rounded fp32 multiply and subtract (align_corners = 0) -, one output element
 * per work item.  scale = 2 is surs_bicubic_up2 (the same kernels, the same bits); scale = 1 returns x. */
enum { SURS_SR_SCALE_MIN = 1, SURS_SR_SCALE_MAX = 4 };
int surs_bicubic_up(const float *x, int h, int w, int c, int x_ld, int scale, int align_corners, const float *addend, int add_ld,
                    float *y, int y_ld, void *stream);
/* surs_bicubic_up2 as 2 x 2 blocks of output pixels per work item (25 loads for four outputs instead of 64; the same bits): the form
 * surs_bicubic_up2_gn runs, without its statistics.  c % 4 == 0, 16-byte aligned rows. */
int surs_bicubic_up2_block(const float *x, int h, int w, int c, int x_ld, int align_corners, const float *addend, int add_ld, float *y,
                           int y_ld, void *stream);
/* y[2h+i][2w+j][c] = lrelu(x[h][w][4c+2i+j], slope)  (slope 1 = no activation) */
int surs_pixel_shuffle2(const float *x, int h, int w, int c4, int x_ld, float slope, float *y, int y_ld, void *stream);
/* y = a + b (+ c, nullable) */
int surs_add3(const float *a, int a_ld, const float *b, int b_ld, const float *c, int c_ld, int hw, int ch, float *y,
              int y_ld, void *stream);
/* GroupNorm(32, C) handed from kernel to kernel (ConvBlock, lib/model/HGFilters.py:57-74: three GroupNorm + ReLU + 3x3 convolutions
 * and a sum - four launches instead of ten).  A kernel that writes a map leaves the statistics of exactly the values it stored as
 * partial sums gn_out[32 groups][*gn_out_slots][2] (sum, sum of squares; doubles; *gn_out_slots <= gn_out_capacity is written to
 * the HOST int; one slot per workgroup, so the layout is a function of the shapes alone); the 3x3 convolution that consumes the map
 * folds them - every workgroup, in the same fixed order - into surs_groupnorm_coeffs' coefficients (same formulas) and applies
 * GroupNorm(gamma, beta, eps) + ReLU while staging.  Deterministic: no atomics.
 *   surs_conv2d_nhwc_gn: surs_conv2d_nhwc_x2 (parts = 2) / _x1 (parts = 1), 3x3 or 1x1 (1x1: the two-part kernel whatever `parts`),
 *   activation and residual as there; gn_in (nullable) = the statistics of x with their slot count, gamma / beta [cin], 32 | cin;
 *   gn_out (nullable) as above = the statistics of y after activation and residual, cout / 32 a power of two <= 32 (a buffer of
 *   ceil(w / 32) * ceil(h / 4) slots always suffices for 3x3, ceil(h * w / 128) for 1x1).
 *   surs_avgpool2_gn / surs_bicubic_up2_gn / surs_add3_gn: the elementwise kernels, the same values bit for bit, plus gn_out
 *   (C a power of two in [32, 1024], 16-byte aligned rows; at most 512 slots). */
int surs_conv2d_nhwc_gn(int parts, const float *x, int h, int w, int cin, int x_ld, const void *wsplit, const float *bias, float *y,
                        int cout, int y_ld, int ksize, int stride, const double *gn_in, int gn_in_slots, const float *gamma,
                        const float *beta, float eps, int act, float slope, const float *residual, int res_ld, double *gn_out,
                        int gn_out_capacity, int *gn_out_slots, void *stream);
int surs_avgpool2_gn(const float *x, int h, int w, int c, int x_ld, float *y, int y_ld, double *gn_out, int gn_out_capacity,
                     int *gn_out_slots, void *stream);
int surs_bicubic_up2_gn(const float *x, int h, int w, int c, int x_ld, int align_corners, const float *addend, int add_ld, float *y,
                        int y_ld, double *gn_out, int gn_out_capacity, int *gn_out_slots, void *stream);
int surs_add3_gn(const float *a, int a_ld, const float *b, int b_ld, const float *c, int c_ld, int hw, int ch, float *y, int y_ld,
                 double *gn_out, int gn_out_capacity, int *gn_out_slots, void *stream);
/* Input stage of the test path (lib/data/EvalDataset_LR_v2.py:227-243): rgb uint8 [h][w][3], mask uint8 [h][w] (device) ->
 * y[h][w][0:3] (pitch y_ld) = (mask / 255) * ((rgb / 255 - 0.5) / 0.5), float32, the reference's operations in its order
 * (ToTensor, Normalize(0.5, 0.5), mask multiply): bit-identical to its img_LR, already in the encoder's NHWC layout. */
int surs_image_prepare(const unsigned char *rgb, const unsigned char *mask, int h, int w, float *y, int y_ld, void *stream);
/* NCHW <-> NHWC(pitch ld) copies for the boundary tensors */
int surs_nchw_to_nhwc(const float *x, int c, int h, int w, float *y, int y_ld, void *stream);
int surs_nhwc_to_nchw(const float *x, int c, int h, int w, int x_ld, float *y, void *stream);

/* GroupNorm(32) statistics of a map as the kernels that wrote it left them: partial sums [32 groups][pitch][2] doubles (sum, sum of
 * squares).  A map written by ONE kernel has slots[0] slots in every group (g1 = g2 = 0).  A map written slice by slice by several
 * kernels, each with its own pixel tiling - a ConvBlock's cat(o1, o2, o3) + x -: groups [0, g1) hold slots[0], [g1, g2) slots[1],
 * [g2, 32) slots[2] slots. */
typedef struct SursGnStats { double *sums; int pitch, g1, g2; int slots[3]; } SursGnStats;
/* One 3x3 / stride-1 convolution of a ConvBlock (lib/model/HGFilters.py:57-73) with the block's closing sum in its epilogue:
 *   v  = conv(pre(x)) + bias,  pre = GroupNorm(gamma, beta, eps) + ReLU from gn_in's statistics, or from in_scale / in_shift, or none
 *   y  = v                      (nullable: the last convolution's own value is not read by anybody) + its statistics in gn_out
 *        (nullable; on entry gn_out->sums and ->pitch = capacity in slots, on return the slot counts)
 *   y2 = v + residual           the slice of out = cat(o1, o2, o3) + x this convolution makes, and - gn_out2 not NULL - the statistics
 *        of those values in the numbering of the WHOLE sum: group gn2_g0 + channel / gn2_cg, rows gn2_pitch slots apart,
 *        *gn2_slots = the slots this launch wrote per group.
 * The same tiles and bits as surs_conv2d_nhwc_gn followed by surs_add3_gn on the slice. */
int surs_conv2d_nhwc_gn_sum(int parts, const float *x, int h, int w, int cin, int x_ld, const void *wsplit, const float *bias,
                            const SursGnStats *gn_in, const float *in_scale, const float *in_shift, const float *gamma, const float *beta,
                            float eps, float *y, int cout, int y_ld, SursGnStats *gn_out, const float *residual, int res_ld, float *y2,
                            int y2_ld, double *gn_out2, int gn2_pitch, int gn2_g0, int gn2_cg, int *gn2_slots, void *stream);

/* surs_conv2d_nhwc_gn_sum without statistics on either side - pre = relu(x * in_scale + in_shift) (BatchNorm in eval mode folded to
 * constants; nullable: none), y = v (nullable), y2 = v + residual -: the same tiles, the same values, no sums formed or written. */
int surs_conv2d_nhwc_sum(int parts, const float *x, int h, int w, int cin, int x_ld, const void *wsplit, const float *bias,
                         const float *in_scale, const float *in_shift, float *y, int cout, int y_ld, const float *residual, int res_ld,
                         float *y2, int y2_ld, void *stream);
/* Calls so far, process-wide, into the entry points that compute or consume GroupNorm statistics (surs_groupnorm_coeffs*, surs_*_gn,
 * surs_conv2d_nhwc_gn_sum): a BatchNorm encoder makes none. */
long long surs_stats_calls(void);

/* ------------------------------------------------------------------ the encoder as ONE call per network
 * SuRSNet.super_res / filter_hr / filter_lr (lib/model/SuRSNet.py:101-129) = SuRSSR_v3.forward (lib/model/SuRSSR_v3.py:143-181),
 * HGFilter.forward high_res (lib/model/HGFilters.py:179-181) and low_res (:183-206; ConvBlock :29-74, HourGlass :76-120), sequenced
 * inside the library (csrc/surs_encoder_net.cpp): the launches of the primitives above in the reference's order, intermediates in
 * the caller's workspace, nothing allocated, no stream created.  The results equal the per-primitive sequencing of the host mirror
 * (encoder.py) bit for bit.  All weight pointers are DEVICE pointers in the layouts of the pack functions above; the struct itself
 * is HOST memory and is only read during the call. */
enum { SURS_ENC_SEPARATE_SUM = 1 };  /* SursEncoderNet.flags: a ConvBlock's closing sum as a pass of its own (surs_add3_gn: the four-launch
                                         form of rounds 4 - 5, whose bits the host mirror's per-launch sequencing reproduces) instead of in
                                         the three convolutions' epilogues (surs_conv2d_nhwc_gn_sum: the default) */
enum { SURS_ENC_EXTENDED = 2 };      /* SursEncoderNet.flags: the caller's struct has the fields behind `bn_end` (norm, sr_scale, bn_*) and
                                         they are read; without it the net is GroupNorm, x2 - whatever lies behind bn_end */
enum { SURS_NORM_GROUP = 0, SURS_NORM_BATCH = 1 };   /* SursEncoderNet.norm (--norm) */
typedef struct SursConv {
    const void *w_split;    /* surs_conv_pack_weights_x2 image (3x3 and 1x1), or NULL: only the fp32 kernel applies */
    const float *w_packed;  /* surs_conv_pack_weights image (the fp32 MFMA / direct kernels: 3 -> 32 head, 32 -> 3 tail) */
    const float *bias;      /* [cout] or NULL */
    int cin, cout, ksize, reserved;
} SursConv;
typedef struct SursGroupNorm { const float *gamma, *beta; } SursGroupNorm;           /* GroupNorm(32, C), eps 1e-5 */
typedef struct SursConvBlock { SursConv conv[3]; SursGroupNorm bn[3]; } SursConvBlock; /* ConvBlock with in_planes == out_planes */
typedef struct SursBatchNorm { const float *scale, *shift; } SursBatchNorm;          /* BatchNorm2d in eval mode, folded: [C] each */
typedef struct SursEncoderNet {
    int residual;           /* opt.residual: the ResBlocks of the super-resolution stages run */
    int n_block[3];         /* opt.n_block */
    int num_stack, hg_depth;
    int parts;              /* 2 = fp32-grade (two f16 parts, three products per MAC); 1 = one f16 product in the 3x3 convolutions */
    int flags;              /* SURS_ENC_* */
    /* super_resolution.* (SuRSSR_v3): head.0, down{1,2,3}.0, tail{1,2,3}.0 / .2, bottleneck.0, bott2.0, ups2.0, ups3.0, ups4.0,
     * last.0, last.2; body: body{i}.{b}.body.0, .body.2 for i = 1..3, b = 0..n_block[i-1]-1, in that order */
    SursConv head, down[3], tail0[3], tail2[3], bottleneck, bott2, ups2, ups3, ups4, last0, last2;
    const SursConv *body;
    SursConv conv5;         /* image_filter_hr.conv5 */
    SursConvBlock conv2;    /* image_filter_lr.conv2 */
    /* image_filter_lr.m{s}: per stack 3 * hg_depth + 1 blocks in module order b1_d, b2_d, [b1_{d-1}, b2_{d-1}, ...], b2_plus_1, b3_1, .., b3_d */
    const SursConvBlock *hg;
    const SursConvBlock *top_m;   /* [num_stack] */
    const SursConv *conv_last, *l, *next;   /* [num_stack]; next[s] = bl{s} + al{s} o l{s} merged (W_bl + W_al W_l), unused for the last stack */
    const SursGroupNorm *bn_end;  /* [num_stack] */
    /* ---- read only with SURS_ENC_EXTENDED in flags */
    int norm;               /* SURS_NORM_GROUP: the SursGroupNorm fields above apply.  SURS_NORM_BATCH (--norm batch): nn.BatchNorm2d in EVAL
                               mode at every norm site, folded by the caller to y = x * scale[c] + shift[c] (scale = weight / sqrt(running_var
                               + 1e-5), shift = bias - running_mean * scale); the SursGroupNorm fields are not read, no statistics are computed */
    int sr_scale;           /* --scale: the bicubic enlargement in front of the super-resolution net, SURS_SR_SCALE_MIN..MAX (0 = 2) */
    /* SURS_NORM_BATCH: the folded coefficients per site, three per ConvBlock (bn1, bn2, bn3) in the order of the block arrays above */
    const SursBatchNorm *bn_conv2;    /* [3] */
    const SursBatchNorm *bn_hg;       /* [3 * num_stack * (3 * hg_depth + 1)] */
    const SursBatchNorm *bn_top_m;    /* [3 * num_stack] */
    const SursBatchNorm *bn_end_bn;   /* [num_stack] */
} SursEncoderNet;
/* Streams the caller lends for the low-resolution branch of hourglass level 1..4 (NULL entries / NULL struct: the branches run one
 * behind the other on `stream`).  The library never creates a stream (a new stream shifts the hardware-queue assignment of every later one). */
typedef struct SursEncoderStreams { void *side[4]; } SursEncoderStreams;
/* bytes of workspace the calls below need for an h x w input image (0: bad arguments, a size the net cannot run included);
 * _enlarged: for an enlarged image of eh x ew = sr_scale * (h x w) pixels (what a caller of surs_encoder_filter_lr alone knows:
 * eh = 4 * feature_lr's height) */
size_t surs_encoder_workspace_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_workspace_bytes_enlarged(const SursEncoderNet *net, int eh, int ew);
/* x [h][w][3] (pitch x_ld) -> feature_lr [h/2][w/2][256], feature_hr [2h][2w][64] and, if want_image, img_sr [2h][2w][3] (dense).
 * With net->sr_scale = s: feature_lr [sh/4][sw/4][256], feature_hr and img_sr [sh][sw]; s * h and s * w must be multiples of 8. */
int surs_encoder_super_res(const SursEncoderNet *net, const float *x, int h, int w, int x_ld, int want_image, float *img_sr,
                           float *feature_lr, float *feature_hr, void *workspace, size_t workspace_bytes, void *stream);
/* feature_lr [h][w][256] (pitch ld) -> outs[s] [h][w][last_ch] (last_ch = l[s].cout = --hg_dim: a multiple of 16 from 16 to 512,
 * else SURS_E_INVALID; pitch last_ch, never rounded up) for every stack s with outs[s] != NULL (HOST array of num_stack device
 * pointers; the last one is required - eval keeps only it, training keeps all) */
int surs_encoder_filter_lr(const SursEncoderNet *net, const float *feature_lr, int h, int w, int ld, float *const *outs,
                           void *workspace, size_t workspace_bytes, const SursEncoderStreams *streams, void *stream);
/* feature_hr [h][w][64] (pitch ld) -> out [h][w][64] */
int surs_encoder_filter_hr(const SursEncoderNet *net, const float *feature_hr, int h, int w, int ld, float *out, void *stream);
/* the three in the order gen_mesh runs them (lib/train_util.py:57-59): image [h][w][3] -> feature_lr, feature_hr (kept: the caller's
 * buffers), im_feat_lr [h/2][w/2][last_ch] (last stack), im_feat_hr [2h][2w][64]; with net->sr_scale = s: [sh/4][sw/4] and [sh][sw] */
int surs_encoder_forward(const SursEncoderNet *net, const float *image, int h, int w, int x_ld, float *feature_lr, float *feature_hr,
                         float *im_feat_lr, float *im_feat_hr, void *workspace, size_t workspace_bytes,
                         const SursEncoderStreams *streams, void *stream);

/* ------------------------------------------------------------------ super-resolution gradients
 * The backward of super_resolution.* (SuRSSR_v3, lib/model/SuRSSR_v3.py:143-181) and of image_filter_hr.conv5
 * (lib/model/HGFilters.py:179-181): csrc/surs_sr_grad.hip (primitives) and csrc/surs_encoder_net.cpp (the network).  Every product
 * is an fp32-input MFMA with fp32 accumulation, whatever --precision says; no float atomics; two calls give the same bits wherever
 * the buffers, the workspace and the tape lie.  All maps are NHWC fp32 with a channel pitch; weights and their gradients are
 * DEVICE memory in the PLAIN torch layout [cout][cin][k][k], biases [cout].
 *
 * The activation derivative is taken from the STORED OUTPUT y of the layer while the gradient operand is read:
 *   dZ[p][co] = g[p][co] * (y[p][co] > 0 ? 1 : slope)      (y == NULL: dZ = g)
 * slope 0.2f: LeakyReLU(0.2); 0: ReLU; y == 0 and y == -0 take the negative side, as torch's in-place activations do.
 *
 * surs_conv_grad_weight: a k x k convolution (k = 1, or 3 with padding 1; stride 1, or 2 with k = 3) of x [h][w][cin] to [ho][wo][cout]:
 *   dw[co][ci][ky][kx] = sum_p dZ[p][co] x[p stride + (ky, kx) - pad][ci],   db[co] = sum_p dZ[p][co]   (db nullable)
 * Order of the sums: the output pixels p = oy wo + ox are cut into parts of 1024 consecutive pixels (parts = ceil(ho wo / 1024)); a
 * part is summed in steps of 16 pixels on the matrix unit, each part's result goes to its own slab of the workspace, and a second
 * kernel adds slab 0, 1, 2, ... in this order.  accumulate = 1: the result is added to what dw / db hold (the next image of a batch),
 * 0: it replaces it.  The bias gradient is one more column of the same product.
 * surs_conv_grad_input: the same convolution's  dx[q][ci] = sum_{ky, kx, co} dZ[(q + pad - (ky, kx)) / stride][co] w[co][ci][ky][kx]
 * over the output pixels that exist (stride 2: where the division is exact), summed per element in the order (ky, kx, co);
 * add = 1: added to what dx holds (the gradient of another consumer of the same map), 0: it replaces it.
 * surs_pixel_unshuffle2_grad: conv -> LeakyReLU -> PixelShuffle(2) -> LeakyReLU stores only the shuffled map y [2h][2w][c] (the forward
 * fuses the second LeakyReLU into surs_pixel_shuffle2); g is the gradient of y, dz [h][w][4c] the gradient of the convolution's result:
 *   dz[i][j][4 ch + 2 dy + dx] = g[2i + dy][2j + dx][ch] * (y[2i + dy][2j + dx][ch] > 0 ? 1 : slope),   slope = 0.2f * 0.2f here. */
size_t surs_conv_grad_weight_workspace_bytes(int ho, int wo, int cin, int cout, int ksize);   /* 0: bad arguments */
int surs_conv_grad_weight(const float *g, int ho, int wo, int cout, int g_ld, const float *y, int y_ld, float slope, const float *x,
                          int h, int w, int cin, int x_ld, int ksize, int stride, float *dw, float *db, int accumulate,
                          void *workspace, size_t workspace_bytes, void *stream);
int surs_conv_grad_input(const float *g, int ho, int wo, int cout, int g_ld, const float *y, int y_ld, float slope, const float *weight,
                         int cin, int ksize, int stride, float *dx, int h, int w, int dx_ld, int add, void *stream);
int surs_pixel_unshuffle2_grad(const float *g, int h, int w, int c, int g_ld, const float *y, int y_ld, float slope, float *dz, int dz_ld,
                               void *stream);

/* The plain fp32 parameters (or their gradients) of the super-resolution convolutions and conv5, in SursEncoderNet's order; HOST
 * struct of DEVICE pointers: weight [cout][cin][k][k], bias [cout]. */
typedef struct SursSrParam { float *weight, *bias; } SursSrParam;
typedef struct SursSrParams {
    SursSrParam head, down[3], tail0[3], tail2[3], bottleneck, bott2, ups2, ups3, ups4, last0, last2;
    const SursSrParam *body;   /* [2 * (n_block[0] + n_block[1] + n_block[2])]: body{i}.{b}.body.0, .body.2 */
    SursSrParam conv5;
} SursSrParams;
/* bytes of the tape / of the backward's workspace for an h x w input image: functions of the net and the size alone (0: refused) */
size_t surs_encoder_sr_tape_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_sr_backward_workspace_bytes(const SursEncoderNet *net, int h, int w);
/* surs_encoder_super_res(want_image = 1) followed by surs_encoder_filter_hr - the same kernels, tiles and operand split, the same bits
 * in img_sr [sh][sw][3], feature_lr [sh/4][sw/4][256], feature_hr [sh][sw][64], im_feat_hr [sh][sw][conv5.cout] (all dense) -, with
 * every map a backward step reads kept in `tape` (256-byte aligned device memory; one buffer per layer where the forward rotates
 * three).  net->parts must be 2: training runs the fp32-grade forward. */
int surs_encoder_super_res_train(const SursEncoderNet *net, const float *x, int h, int w, int x_ld, float *img_sr, float *feature_lr,
                                 float *feature_hr, float *im_feat_hr, void *tape, size_t tape_bytes, void *stream);
/* The gradients of L = <g_img_sr, img_sr> + <g_feature_lr, feature_lr> + <g_im_feat_hr, im_feat_hr> with respect to every parameter
 * of `params` (the weights the forward ran with, plain layout), from the tape of surs_encoder_super_res_train on an h x w image.
 * g_* are dense NHWC maps of the outputs' shapes, nullable: a missing one counts as zero and the layers only it reaches cost nothing
 * (their gradients are zero); all three missing is SURS_E_INVALID.  accumulate = 1 adds to what `grads` holds.  One stream, launches
 * in a fixed order: last.2, last.0, conv5, ups4, ups3, ups2, bott2, bottleneck, then stage 3, 2, 1 (tail.2, tail.0, the blocks
 * from the last to the first, down), head; the input gradient of head and of the bicubic enlargement is never formed. */
int surs_encoder_super_res_backward(const SursEncoderNet *net, const SursSrParams *params, const void *tape, int h, int w,
                                    const float *g_img_sr, const float *g_feature_lr, const float *g_im_feat_hr, const SursSrParams *grads,
                                    int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ hourglass gradients
 * The backward of image_filter_lr's ConvBlock (lib/model/HGFilters.py:29-74, in_planes == out_planes == 256: every block of the
 * low-resolution filter) and of its HourGlass module m{s} (:76-120): csrc/surs_hg_grad.hip (primitives) and
 * csrc/surs_encoder_net.cpp (the modules).  --norm group and net->parts == 2 only.  The rules of the super-resolution gradients
 * hold: fp32 with fp32 accumulation, no float atomics, two calls give the same bits wherever buffers, workspace and tape lie, NHWC
 * maps with a channel pitch (here: multiples of 4, 16-byte aligned pixels - every access is 16 bytes), parameters and their
 * gradients in the plain torch layout.  The stack's tail (conv_last, bn_end, l, bl, al): "stack-tail gradients" below.
 *
 * surs_groupnorm_fold: the four vectors of a GroupNorm(32) site - mean[32], rstd[32] (per group) and scale[c] = rstd gamma,
 * shift[c] = beta - mean rstd gamma (per channel) - from the statistics the producer of the map left (stats, the in-kernel fold of
 * the convolutions restated: the same formulas in double, the same order, the same float results) or, stats == NULL, from the map x
 * [hw][c] itself (surs_groupnorm_coeffs_ws' two launches, whose partial sums - scratch: surs_groupnorm_scratch_bytes() - a third
 * folds into mean and rstd in the order its second launch uses).  gamma is never divided by.
 *
 * surs_groupnorm_relu_grad: out = relu(z), z = x * scale + shift = GroupNorm32(x; gamma, beta); g = d L / d out, c = 64, 128 or 256.
 *   gy = g where z > 0 else 0 (z recomputed from x and the forward's scale / shift in the convolutions' staging expression, a
 *   multiply and an add: the forward's own mask; z == 0 and -0 take the negative side), xh = (x - mean) rstd, m = hw c / 32,
 *   dbeta[c] = sum_p gy,  dgamma[c] = sum_p gy xh,  s1[grp] = sum_{c in grp} gamma dbeta,  s2[grp] = sum_{c in grp} gamma dgamma,
 *   dx = rstd (gy gamma - s1 / m - xh s2 / m)      add = 1: added to what dx holds; accumulate = 1: dgamma / dbeta are added to.
 * Order of the sums: the pixels are cut into parts of 64 consecutive pixels; inside a part a channel's pixels are summed by
 * 1024 / c lanes, lane l taking pixels l, l + 1024 / c, ... in order, and the lanes are added in lane order; the parts are added in
 * the order 0, 1, 2, ...; s1 and s2 add the group's channels in channel order.  Two passes over g and x: one reads them for the
 * sums, one reads them again and writes dx.
 *
 * surs_avgpool2_grad: g [h][w][c] -> dx [2h][2w][c] (+)= 0.25 g[y / 2][x / 2], the transpose of surs_avgpool2.
 * surs_bicubic_up2_grad: g [2h][2w][c] -> dx [h][w][c], the transpose of surs_bicubic_up2(align_corners = 1) with the forward's own
 * fp32 coordinate and coefficient expressions (A = -0.75, border-clamped taps; the clamped taps of one output coordinate that fall
 * on one source pixel add their weights in tap order): dx[sy][sx] (+)= sum_oy Wy(oy, sy) (sum_ox Wx(ox, sx) g[oy][ox]), gathered
 * per element with oy ascending and, inside a row, ox ascending. */
int surs_groupnorm_fold(const SursGnStats *stats, const float *x, int hw, int c, int x_ld, float eps, const float *gamma,
                        const float *beta, float *mean, float *rstd, float *scale, float *shift, void *scratch, void *stream);
size_t surs_groupnorm_relu_grad_workspace_bytes(int hw, int c);   /* 0: bad arguments */
int surs_groupnorm_relu_grad(const float *g, int g_ld, const float *x, int x_ld, int hw, int c, const float *mean, const float *rstd,
                             const float *scale, const float *shift, const float *gamma, float *dx, int dx_ld, int add, float *dgamma,
                             float *dbeta, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
int surs_avgpool2_grad(const float *g, int h, int w, int c, int g_ld, float *dx, int dx_ld, int add, void *stream);
int surs_bicubic_up2_grad(const float *g, int h, int w, int c, int g_ld, float *dx, int dx_ld, int add, void *stream);

/* The plain fp32 parameters (or their gradients) of one ConvBlock, mirroring SursConvBlock; HOST struct of DEVICE pointers:
 * weight[k] = conv{k+1}.weight [cout][cin][3][3] (256 -> 128, 128 -> 64, 64 -> 64; no bias), gamma[k] / beta[k] = bn{k+1}.weight / .bias. */
typedef struct SursHgBlockParams { float *weight[3], *gamma[3], *beta[3]; } SursHgBlockParams;
/* bytes of the tape / of the backward's workspace of one block, and of one stack's hourglass (net->hg_depth levels), on an h x w
 * map: functions of the net and the size alone; 0: refused (h or w not a multiple of 2^hg_depth for the hourglass, --norm batch,
 * parts == 1). */
size_t surs_encoder_convblock_tape_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_convblock_backward_workspace_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_hourglass_tape_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_hourglass_backward_workspace_bytes(const SursEncoderNet *net, int h, int w);
/* The forward of `block` (any ConvBlock of the net: conv2, hg[i], top_m[s]) / of stack `stack`'s hourglass on x [h][w][256] (pitch
 * ld; it carries no statistics) into out [h][w][256] (dense): the launches of the inference forward in its separate-sum form (the
 * host mirror's; the hourglass on ONE stream) plus one surs_groupnorm_fold per norm site, the same bits.  The tape (256-byte aligned)
 * keeps, per block, the input, the raw cat(o1, o2, o3) - the closing sum writes a map of its own - and the four vectors of its
 * three norm sites; the joins of a level (average pool, bicubic + sum) are linear and need nothing. */
int surs_encoder_convblock_train(const SursEncoderNet *net, const SursConvBlock *block, const float *x, int h, int w, int ld, float *out,
                                 void *tape, size_t tape_bytes, void *stream);
int surs_encoder_hourglass_train(const SursEncoderNet *net, int stack, const float *x, int h, int w, int ld, float *out, void *tape,
                                 size_t tape_bytes, void *stream);
/* g = d L / d out (dense [h][w][256]) -> dx = d L / d x (dense, always produced) and the gradients of the module's parameters
 * (params / grads: one SursHgBlockParams for a block, 3 hg_depth + 1 in the stack's module order for an hourglass); accumulate = 1
 * adds to what grads holds.  One stream, launches in a fixed order.  A block: dx = g (the identity path); then for conv3, conv2,
 * conv1 in this order: relu(norm(input)) is materialised (surs_scale_shift_act), surs_conv_grad_weight, surs_conv_grad_input,
 * surs_groupnorm_relu_grad ADDED to the gradient of the map that norm read (slice [128, 192), slice [0, 128) of g's copy, dx).  A
 * level of the hourglass: b1 (into the level input's gradient), the bicubic transpose, b3, the level below (or b2_plus), b2, the
 * pool transpose ADDED onto the level input's gradient. */
int surs_encoder_convblock_backward(const SursEncoderNet *net, const SursConvBlock *block, const SursHgBlockParams *params, const void *tape,
                                    int h, int w, const float *g, float *dx, const SursHgBlockParams *grads, int accumulate,
                                    void *workspace, size_t workspace_bytes, void *stream);
int surs_encoder_hourglass_backward(const SursEncoderNet *net, int stack, const SursHgBlockParams *params, const void *tape, int h, int w,
                                    const float *g, float *dx, const SursHgBlockParams *grads, int accumulate, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ stack-tail gradients, and the whole low-resolution filter
 * The tail of stack s of image_filter_lr (lib/model/HGFilters.py:196-206), D = --hg_dim, p over the h w pixels:
 *   t = conv_last{s}(ll) [p][256],  a = relu(GroupNorm32(t; bn_end{s})) (never stored),  out = l{s}(a) [p][D],
 *   next = previous + bl{s}(a) + al{s}(out) [p][256]   (not for the last stack; ONE launch on the merged next{s} = W_bl + W_al W_l)
 * and its backward from G_out = d L / d out and G_next = d L / d next (either may be missing = zero; the last stack has no G_next):
 *   dOut = G_out + G_next W_al,   dA = dOut W_l + G_next W_bl,
 *   dW_al = G_next^T out, db_al = sum_p G_next;  dW_bl = G_next^T a, db_bl = sum_p G_next;  dW_l = dOut^T a, db_l = sum_p dOut,
 *   (dt, dgamma, dbeta) = surs_groupnorm_relu_grad(dA, t, bn_end's folded vectors),
 *   dW_cl = dt^T ll, db_cl = sum_p dt,  d ll = dt W_cl,  d previous = G_next (nothing is computed for it).
 * The gradients are those of the UN-MERGED bl, al, l; the forward runs the merged launch, so its values are the packed weights'.
 * csrc/surs_tail_grad.hip (the joint) and csrc/surs_encoder_net.cpp (the modules); the rules of the hourglass gradients hold:
 * --norm group and net->parts == 2 only, fp32 on v_mfma_f32_32x32x2_f32 with fp32 accumulation, no float atomics, the same bits on
 * every call wherever buffers, tape and workspace lie.
 *
 * surs_tail_joint_grad: dOut [p][D] and dA [p][256] in one launch (weights in the plain layout: w_al [256][D], w_l [D][256],
 * w_bl [256][256]; D = 1 .. 512, any p; g_next: pitch a multiple of 4, 16-byte aligned pixels).  A workgroup owns 64 pixels for
 * D <= 256 and 32 above; it stages its tile of g_next once for both products and keeps its tile of dOut in LDS.  Per element:
 *   dOut[p][d] = g_out[p][d] + S,  S = 0, then + g_next[p][c] w_al[c][d] for c = 0 .. 255 in this order (each step one fused
 *     multiply-add, one rounding); g_out is added last.  g_next == NULL: dOut = g_out (a copy); g_out == NULL: dOut = S.
 *   dA[p][j]: ONE accumulator from 0: + dOut[p][d] w_l[d][j] for d = 0 .. D - 1 in this order, then + g_next[p][c] w_bl[c][j] for
 *     c = 0 .. 255 in this order (g_next == NULL: nothing more).
 * Both missing is SURS_E_INVALID.  The chain it replaces - surs_conv_grad_input (k = 1) three times, the second and third adding
 * into their target - stays in the library and rounds dA's two sums separately. */
int surs_tail_joint_grad(const float *g_out, int g_out_ld, const float *g_next, int g_next_ld, const float *w_al, const float *w_l,
                         const float *w_bl, int p, int d, float *d_out, int d_out_ld, float *d_a, int d_a_ld, void *stream);

/* The plain fp32 parameters (or their gradients) of one stack's tail; HOST struct of DEVICE pointers: conv_last{s} [256][256][1][1],
 * l{s} [D][256][1][1], bl{s} [256][256][1][1], al{s} [256][D][1][1] with their biases, bn_end{s}.weight / .bias; bl and al are NULL
 * for the last stack. */
typedef struct SursHgTailParams { SursSrParam conv_last, l, bl, al; float *gamma, *beta; } SursHgTailParams;
/* every image_filter_lr.* parameter: conv2, hg [num_stack * (3 hg_depth + 1)] in SursEncoderNet.hg's order, top_m and tail [num_stack] */
typedef struct SursHgFilterParams {
    SursHgBlockParams conv2;
    const SursHgBlockParams *hg, *top_m;
    const SursHgTailParams *tail;
} SursHgFilterParams;
/* bytes of the tape / of the backward's workspace of a tail (the largest over the stacks) and of the whole filter on an h x w map:
 * functions of the net and the size alone, the sequencing run without launches; 0: refused (--norm batch, parts == 1, for the filter
 * h or w not a multiple of 2^hg_depth). */
size_t surs_encoder_tail_tape_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_tail_backward_workspace_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_filter_lr_tape_bytes(const SursEncoderNet *net, int h, int w);
size_t surs_encoder_filter_lr_backward_workspace_bytes(const SursEncoderNet *net, int h, int w);
/* The tail of stack `stack` on ll [h][w][256] (pitch ll_ld) and previous [h][w][256] (pitch previous_ld; NULL, with next, for the
 * last stack) into out [h][w][D] and next [h][w][256] (dense): surs_encoder_filter_lr's launches - the pointwise convolution
 * conv_last leaving bn_end's statistics, l, the merged next with the residual in its epilogue - plus one surs_groupnorm_fold, the
 * same bits.  The tape (256-byte aligned) keeps ll, t, out and bn_end's four vectors. */
int surs_encoder_tail_train(const SursEncoderNet *net, int stack, const float *ll, int ll_ld, const float *previous, int previous_ld, int h,
                            int w, float *out, float *next, void *tape, size_t tape_bytes, void *stream);
/* g_out [h][w][D], g_next [h][w][256] (dense, nullable, not both) -> d_ll [h][w][256] (dense, replaced) and the tail's parameter
 * gradients; accumulate = 1 adds to what grads holds.  One stream, launches in a fixed order: a = relu(norm(t))
 * (surs_scale_shift_act), surs_tail_joint_grad, surs_conv_grad_weight (k = 1) for al and bl (g_next missing: they are zeroed instead,
 * accumulate = 0), for l, surs_groupnorm_relu_grad, surs_conv_grad_weight and surs_conv_grad_input for conv_last. */
int surs_encoder_tail_backward(const SursEncoderNet *net, int stack, const SursHgTailParams *params, const void *tape, int h, int w,
                               const float *g_out, const float *g_next, float *d_ll, const SursHgTailParams *grads, int accumulate,
                               void *workspace, size_t workspace_bytes, void *stream);
/* HGFilter.forward (low_res) with ONE tape: conv2, then per stack hourglass -> top_m -> tail, the launches of surs_encoder_filter_lr
 * in its one-stream, separate-sum form (statistics handed from kernel to kernel as there) plus one surs_groupnorm_fold per norm
 * site; outs[s] [h][w][D] (HOST array of num_stack device pointers, ALL required: training keeps every stack's output). */
int surs_encoder_filter_lr_train(const SursEncoderNet *net, const float *feature_lr, int h, int w, int ld, float *const *outs, void *tape,
                                 size_t tape_bytes, void *stream);
/* g_outs[s] = d L / d outs[s] (HOST array; a NULL entry is zero, all NULL is SURS_E_INVALID) -> d_feature_lr [h][w][256] (dense) and
 * every parameter's gradient.  From the last stack to the first: the tail (g_outs[s], d previous_{s+1}), top_m, the hourglass;
 * previous_s has two consumers, the hourglass and the identity into next_s: d previous_s = (hourglass's input gradient) +
 * d previous_{s+1}, ONE fp32 sum of two terms (surs_add3); conv2 last.  A stack no gradient reaches costs nothing: its gradients are
 * zeroed (accumulate = 0). */
int surs_encoder_filter_lr_backward(const SursEncoderNet *net, const SursHgFilterParams *params, const void *tape, int h, int w,
                                    const float *const *g_outs, float *d_feature_lr, const SursHgFilterParams *grads, int accumulate,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ point evaluator */

/* HOST: pack the two SurfaceClassifier MLPs (lr: 321-1024-512-256-128-1, hr: 322-..., skip-concat at layers
 * 2,3,4; w[l] = Conv1d weight [out][in], b[l] = bias) into one blob that surs_query_* consume.  `dtype` selects
 * the element type of the dense cores used by the grid kernel (SURS_BF16 or SURS_F16).  Call with blob == NULL
 * to get the size in bytes.  The caller uploads the blob to device memory (256-byte aligned). */
size_t surs_mlp_pack(const float *const w_lr[5], const float *const b_lr[5], const float *const w_hr[5],
                     const float *const b_hr[5], int dtype, void *blob);

/* How the fp32 point path (surs_query_points, _views, surs_query_grid_indexed, the general-calibration sweep) carries its fp32
 * operands through the bf16 / f16 matrix pipe, process-wide: 2 = two f16 parts, three products per MAC (default: 1.6x the
 * rate, 22 significant bits, |activation| and |feature| < 65504), 3 = three bf16 parts, six products (24 bits, fp32's exponent
 * range), 0 = back to the default (or the SURS_SPLIT environment variable).  Both meet the 1e-4 logit tolerance. */
int surs_set_operand_split(int parts);
/* The same for the calling host thread only (0 = back to the process-wide setting); takes precedence over it.  The host mirror
 * uses it to repeat a query or a sweep on three bf16 parts after an f16 overflow (non-finite results).  parts = 1 (this call only):
 * surs_query_points / surs_query_points_hr run ONE f16 product per MAC (one f16 part per operand, 11 significant bits, a third of the
 * matrix work) - NOT fp32-grade: what SuRSNet.query_mr / query_sr of `--precision bf16 | fp16` evaluate arbitrary points with, as the
 * reference's MLP would in half precision (lib/model/SurfaceClassifier.py:53-81); every other entry point ignores it. */
int surs_set_operand_split_local(int parts);

/* Column kernel of surs_query_grid, process-wide (A/B comparisons and regression tests; a per-call choice goes through
 * surs_query_grid_opt): 0 = default (or the SURS_GRID_KERNEL / SURS_GRID_F32_KERNEL environment variables); reduced precision
 * 3 (dense layer 1), 10 (layer 1 restated along the column, eight waves), 12 (the default: 10's arithmetic and bits with layer 1
 * streamed into layer 2, two workgroups per compute unit); fp32-grade 5 (dense), 11 (restated) - DESIGN.md section 4. */
int surs_set_grid_kernel(int version);

/* How many of the 1024 layer-0 channels the default column kernels (layer 1 restated along the column) would
 * list per z tile (`tile` = 128 for the reduced precisions, 64 for SURS_F32) on this sweep: evaluated on the ry columns of axis-0
 * plane `i_plane` of the grid `mat` describes - every slab of one grid gives the same answer.  listed[0]: mean over (column,
 * tile) for the lr classifier, listed[1]: an upper bound for the hr classifier; both -1 where the column kernels do not apply.
 * `listed` is host memory; the call synchronises the stream.  The host mirror runs the dense column kernels (version 3 / 5) when
 * listed[0] exceeds 400.  Workspace as for surs_query_grid. */
int surs_query_grid_probe(int i_plane, int ry, int rz, int tile, const double *mat, const float *calib, float zmul, float zdiv,
                          const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob,
                          void *workspace, size_t workspace_bytes, float *listed, void *stream);

/* bytes of device workspace the two query entry points need for `max_points` points per call / grid batch */
size_t surs_query_workspace_bytes(int max_points);

/* query_mr + query_sr + get_preds for one view, fp32 arithmetic (f32 MFMA).
 *   points  [3][n] fp32 (x row, y row, z row), calib HOST [12] = rows 0..2 of the 4x4 calibration,
 *   zmul = loadSize/2 (integer division done by the caller), zdiv = z_size,
 *   feat_lr NHWC [hl][wl][c_lr=256] pitch c_lr, feat_hr NHWC [hh][wh][c_hr=64],
 *   outputs [n] each; logit_* nullable (pre-sigmoid, pre-mask). */
int surs_query_points(const float *points, int n, const float *calib, float zmul, float zdiv, const float *feat_lr,
                      int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob, void *workspace,
                      size_t workspace_bytes, float *pred_hr, float *pred_lr, float *logit_hr, float *logit_lr,
                      void *stream);

/* query_sr alone (lib/model/SuRSNet.py:161-187), for callers that pass it OTHER points than the preceding query_mr (the reference
 * only requires the same n): the hr classifier on `points`, its last input channel taken from p_lr [n] (device; the masked lr
 * occupancies query_mr left behind) instead of from an lr evaluation of these points.  Arguments as surs_query_points. */
int surs_query_points_hr(const float *points, int n, const float *calib, float zmul, float zdiv, const float *feat_lr,
                         int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob, void *workspace,
                         size_t workspace_bytes, const float *p_lr, float *pred_hr, float *logit_hr, void *stream);

/* ------------------------------------------------------------------ classifiers of any supported shape */

/* One SurfaceClassifier as the reference builds it from --mlp_dim_*, --mlp_res_layers_* and --no_residual
 * (lib/model/SuRSNet.py:67-78, lib/model/SurfaceClassifier.py:7-43): n_layers Conv1d layers of widths dims[0..n_layers];
 * bit l of res_mask = layer l sees cat(y, feature) (zero under no_residual, SurfaceClassifier.py:57-66).  Supported:
 * 1 <= n_layers <= 8, dims[0] = D + 65 (lr) / D + 66 (hr), dims[n_layers] = 1, hidden widths 1..2048, res_mask < 2^n_layers.
 * D = lr.dims[0] - 65 is the encoder's --hg_dim (lib/model/HGFilters.py:166-174: a point's features are [D lr | 64 hr | z], + p_lr for
 * hr): a multiple of 16 from 16 to 512, 256 (321 / 322) in the released model.  Every entry below that takes feat_lr with such a pair
 * reads it as [hl][wl][D], pitch D.  For D > 256 the LDS of a 16-point tile holds narrower hidden layers: at most
 * ((160 KiB / 16 - 16) / 4 - 4 - (pad32(D + 66) + 4)) rounded down to 32 (D = 512: 1920); the refusal names the limit and D. */
typedef struct SursMlpShape {
    int n_layers;
    int dims[9];
    unsigned res_mask;
} SursMlpShape;

/* HOST: pack both classifiers (w[l] = Conv1d weight [out][in], b[l] = bias, l < n_layers) into the blob of the fused evaluator
 * (csrc/surs_mlp_generic.h: per layer one f16 part, two f16 parts and three bf16 parts, zero-padded to the MFMA tile, fp32 bias).
 * blob == NULL: returns the size in bytes.  Returns 0 for an unsupported pair (surs_last_error names the limit). */
size_t surs_mlp_pack_generic(const SursMlpShape *lr, const float *const *w_lr, const float *const *b_lr, const SursMlpShape *hr,
                             const float *const *w_hr, const float *const *b_hr, void *blob);

/* HOST: how the fused evaluator runs this pair: *tile_points points per workgroup, *lds_bytes of LDS per workgroup, and (offsets,
 * nullable: [2][8][4] = byte offsets of the one-part, two-part, three-part images and the bias of classifier m, layer l) the blob
 * layout.  The fused kernel needs no device workspace. */
int surs_mlp_generic_info(const SursMlpShape *lr, const SursMlpShape *hr, int *tile_points, int *lds_bytes,
                          unsigned long long *offsets);

/* query_mr + query_sr + get_preds (lib/model/SuRSNet.py:131-187) for classifiers of any supported shape, in ONE launch per call:
 * projection, in-image mask, z_feat, bilinear gather, mlp_lr, masked sigmoid, mlp_hr, masked sigmoid per tile of points, the
 * activations in LDS.  Arguments as surs_query_points - but feat_lr is [hl][wl][D], D = lr->dims[0] - 65 (SursMlpShape; the octree's
 * indexed lattice points come through this entry too) -, plus the shapes and the blob of surs_mlp_pack_generic.  p_lr non-NULL: the hr
 * classifier alone, fed with p_lr [n] (query_sr on other points); pred_lr / logit_lr are then ignored.  Operand split as
 * surs_query_points: surs_set_operand_split_local (1 = one f16 product, 2 = two f16 parts, 3 = three bf16 parts) or the process
 * setting.  logit_* nullable (pre-sigmoid, pre-mask). */
int surs_query_points_generic(const float *points, int n, const float *calib, float zmul, float zdiv, const float *feat_lr, int hl,
                              int wl, const float *feat_hr, int hh, int wh, const SursMlpShape *lr, const SursMlpShape *hr,
                              const void *blob, const float *p_lr, float *pred_hr, float *pred_lr, float *logit_hr,
                              float *logit_lr, void *stream);

/* The dense sweep (create_grid + eval_grid + eval_func, lib/sdf.py:4-52, lib/mesh_util.py:16-34) of grid slab [i0, i1) with the
 * fused evaluator: voxel coordinates made in the kernel in float64 from `mat` (HOST, rows 0..2 of the grid matrix) and cast to
 * float32, as create_grid does.  feat_lr [hl][wl][D], D = lr->dims[0] - 65.  vol_hr / vol_lr [(i1-i0)][ry][rz]. */
int surs_query_grid_generic(int i0, int i1, int ry, int rz, const double *mat, const float *calib, float zmul, float zdiv,
                            const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const SursMlpShape *lr,
                            const SursMlpShape *hr, const void *blob, float *vol_hr, float *vol_lr, void *stream);

/* ------------------------------------------------------------------ every hourglass stack: the validation forward
 * In training mode filter_lr keeps every stack's feature map (lib/model/SuRSNet.py:101-110) and query_mr / query_sr evaluate the
 * classifiers once per kept map (SuRSNet.py:149-157, 175-185): pass s reads feat_lr[s] and the one hr map; stack s's masked lr
 * prediction is the last input channel of stack s's hr classifier.  The two entries below do that for the S = num_stacks >= 1 maps of
 * one image.  feat_lr: HOST array of S device pointers, each map [hl][wl][D]; outputs (and logits, nullable) are [S][n], row s =
 * stack s.  Three forms:
 *   both classifiers   p_lr NULL, pred_hr and pred_lr given
 *   hr only            p_lr [S][n] given (query_sr on other points than query_mr's: row s feeds stack s); pred_lr / logit_lr ignored
 *   lr only            pred_hr NULL, pred_lr given; logit_hr ignored (the pass of forward() whose hr predictions nothing reads)
 * Row s is bit for bit what the single-map entry writes for map s in the same form and operand split; S = 1 is the single-map entry. */

/* surs_query_points_generic over S maps in ONE launch (csrc/surs_mlp_fused_stacks.inc: grid = point tiles x stacks, the map pointers
 * in the launch argument, eight per launch - more maps: one launch per eight).  Other arguments as surs_query_points_generic. */
int surs_query_points_generic_stacks(const float *points, int n, const float *calib, float zmul, float zdiv, int num_stacks,
                                     const float *const *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                                     const SursMlpShape *lr, const SursMlpShape *hr, const void *blob, const float *p_lr, float *pred_hr,
                                     float *pred_lr, float *logit_hr, float *logit_lr, void *stream);

/* The released shape: the layer kernels of surs_query_points / surs_query_points_hr sequenced once per map inside the library, in one
 * call on one workspace (surs_query_workspace_bytes(n), whatever S).  Other arguments as surs_query_points. */
int surs_query_points_stacks(const float *points, int n, const float *calib, float zmul, float zdiv, int num_stacks,
                             const float *const *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob,
                             void *workspace, size_t workspace_bytes, const float *p_lr, float *pred_hr, float *pred_lr,
                             float *logit_hr, float *logit_lr, void *stream);

/* The four terms of SuRSNet.forward's loss (lib/model/SuRSNet.py:196-236) in one deterministic reduction (a fixed partition, float64
 * partial sums, a second stage in fixed order, no atomics: two runs give the same bits).  Device arrays:
 *   pred_lr, pred_hr [S][m] (S = num_stacks), lab_lr, lab_hr [m] - the labels the lr / hr predictions are held against -,
 *   img_sr, img_hr [k] in one common element order.
 *   terms[0] = mean over stacks of MSE(pred_lr[s], lab_lr)      get_error_lr
 *   terms[1] = the same of pred_hr and lab_hr                   get_error_hr
 *   terms[2] = mean |img_sr - img_hr|                           get_errorSR
 *   terms[3] = MSE(lab_hr - lab_lr, pred_hr[S-1] - pred_lr[S-1]) get_error_disp_1
 * A term whose inputs are NULL is 0 (terms[3] needs all four of the first group).  weights: HOST [4] (opt.mlp1, mlp2, srweight,
 * dispweight), total: device, both nullable: *total = w[0] terms[0] + w[1] terms[1] + w[2] terms[2] + w[3] terms[3] in float32, left to
 * right (SuRSNet.py:265).  workspace: surs_forward_losses_workspace_bytes() bytes, 8-byte aligned.  No synchronisation. */
size_t surs_forward_losses_workspace_bytes(void);
int surs_forward_losses(const float *pred_lr, const float *pred_hr, int num_stacks, long long m, const float *lab_lr,
                        const float *lab_hr, const float *img_sr, const float *img_hr, long long k, const float *weights,
                        void *workspace, size_t workspace_bytes, float *terms, float *total, void *stream);

/* ------------------------------------------------------------------ classifier gradients
 * d error / d (every conv{l}.weight and conv{l}.bias of mlp_lr and mlp_hr) of SuRSNet.forward's loss (lib/model/SuRSNet.py:131-187,
 * 196-266, lib/model/SurfaceClassifier.py:45-81), the encoder frozen; single view, orthogonal projection; csrc/surs_mlp_grad.hip.
 * With stacks s < S, q_s = in_img_mr sigmoid(mlp_lr(x_s(points_mr))) and r_s = in_img_sr sigmoid(mlp_hr([x_s(points_sr) | q_s])), q_s
 * taken index by index:
 *   error = w[0] mean_s MSE(q_s, lab_lr) + w[1] mean_s MSE(r_s, lab_hr) + w[2] MSE(lab_hr - lab_lr, r_{S-1} - q_{S-1})  (+ the
 *   super-resolution term, which does not depend on these parameters), every mean over m_total values.
 * mlp_lr's gradient has three sources: its own term, the displacement term and mlp_hr's last input channel.  LeakyReLU slope 0.01,
 * its derivative at exactly 0 the negative side's; a point outside the image contributes exactly zero.  fp32 operands on the
 * f32-input MFMA with fp32 accumulation whatever the operand split of the query entries; no float atomics and a fixed order of every
 * sum: two runs give the same bits.  Points go in chunks of 2048, so the workspace depends on the shapes only. */

/* Bytes of device workspace surs_mlp_grad needs for this pair, whatever n (0: unsupported pair, surs_last_error names the limit). */
size_t surs_mlp_grad_workspace_bytes(const SursMlpShape *lr, const SursMlpShape *hr);

/* The gradients of ONE image.  points_mr / points_sr [3][n] device (query_mr's and query_sr's points), calib_mr / calib_sr HOST [12]
 * rows of [R|t], zmul / zdiv as surs_query_points; feat_lr: HOST array of S = num_stacks device maps [hl][wl][D], feat_hr [hh][wh][64];
 * w_* / b_*: HOST arrays of n_layers device pointers to the plain fp32 Conv1d weights [out][in] and biases [out]; lab_lr / lab_hr [n]
 * device: what q / r are held against (the labels as SuRSNet stores them); loss_weights HOST [3] = opt.mlp1, opt.mlp2,
 * opt.dispweight; m_total = the number of points the batch's means run over (B n: one call per image with accumulate = 1 after the
 * first gives the batch's gradient).  accumulate 0: the outputs are overwritten, 1: added to.  gw_* / gb_*: HOST arrays of device
 * pointers, Conv1d layout [out][in] / [out] fp32.  pred_lr / pred_hr: nullable [S][n] device, q_s / r_s of the call's own forward.
 * workspace: surs_mlp_grad_workspace_bytes(lr, hr) bytes, 256-byte aligned.  No synchronisation. */
int surs_mlp_grad(const float *points_mr, const float *points_sr, int n, const float *calib_mr, const float *calib_sr, float zmul,
                  float zdiv, int num_stacks, const float *const *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                  const SursMlpShape *lr, const SursMlpShape *hr, const float *const *w_lr, const float *const *b_lr,
                  const float *const *w_hr, const float *const *b_hr, const float *lab_lr, const float *lab_hr,
                  const float *loss_weights, long long m_total, int accumulate, float *const *gw_lr, float *const *gb_lr,
                  float *const *gw_hr, float *const *gb_hr, float *pred_lr, float *pred_hr, void *workspace, size_t workspace_bytes,
                  void *stream);

/* The same call, and with it d error / d (the feature maps the point rows were sampled from): what an encoder's backward starts
 * from.  gfeat_lr: HOST array of num_stacks device maps [hl][wl][D] fp32, map s the gradient of feat_lr[s]; gfeat_hr [hh][wh][64]
 * fp32, the gradient of feat_hr.  accumulate_features 0: the call zeroes the maps first, 1: it adds to them - apart from
 * `accumulate`, because a batch sums the parameter gradients over its images while every image has maps of its own.  gfeat_lr and
 * gfeat_hr both NULL: exactly surs_mlp_grad (its launches, its bits, its workspace); one of them NULL is an error.  n == 0 with
 * accumulate_features 0 still zeroes the maps.  The parameter gradients and predictions have surs_mlp_grad's bits either way.
 * What is summed: per stack s, chunk of 2048 points and classifier, dX0 = d error / d (the sampled D + 64 channels of the
 * classifier's input row) = dZ_0 W_0[:, :D + 64] + sum over skip layers l of dZ_l W_l[:, k1 : k1 + D + 64] (fp32 MFMA products, added
 * layer by layer from the last layer to the first), scattered through the four bilinear taps of the gather (align_corners=True,
 * zeros padding: the same weights and validity tests; a tap outside the map is dropped, never clamped) - columns [0, D) to
 * gfeat_lr[s], columns [D, D + 64) to gfeat_hr.  Both classifiers write both maps: mlp_lr at points_mr, mlp_hr at points_sr.
 * Order: a pixel's contributions of one chunk and classifier are summed from 0 with fmaf in the order (point index, tap (x0,y0),
 * (x1,y0), (x0,y1), (x1,y1)) and added to the map element once; these partial sums arrive in the order stack, chunk, mlp_hr then
 * mlp_lr.  No float atomics: two calls give the same bits, wherever the buffers lie.
 * workspace: surs_mlp_grad_features_workspace_bytes(lr, hr) bytes where maps are given (a function of the shapes alone, neither of n
 * nor of the map sizes), 256-byte aligned. */
size_t surs_mlp_grad_features_workspace_bytes(const SursMlpShape *lr, const SursMlpShape *hr);
int surs_mlp_grad_features(const float *points_mr, const float *points_sr, int n, const float *calib_mr, const float *calib_sr,
                           float zmul, float zdiv, int num_stacks, const float *const *feat_lr, int hl, int wl, const float *feat_hr,
                           int hh, int wh, const SursMlpShape *lr, const SursMlpShape *hr, const float *const *w_lr,
                           const float *const *b_lr, const float *const *w_hr, const float *const *b_hr, const float *lab_lr,
                           const float *lab_hr, const float *loss_weights, long long m_total, int accumulate, float *const *gw_lr,
                           float *const *gb_lr, float *const *gw_hr, float *const *gb_hr, float *pred_lr, float *pred_hr,
                           float *const *gfeat_lr, float *gfeat_hr, int accumulate_features, void *workspace, size_t workspace_bytes,
                           void *stream);

/* Multi-view query of one subject (num_views = V in [1, 64], orthogonal projection) for classifiers of any supported shape, in ONE
 * launch per call (csrc/surs_mlp_fused_views.inc): lib/model/SurfaceClassifier.py:53-81 with num_views > 1 - layers 0 .. L/2 per
 * view on that view's features, then the view mean ((sum in view order) * (1/V)) of layer L/2's outputs and of the input features,
 * layers L/2 + 1 .. L-1 once per point (L = 1, 2: the mean of the logits) - and SuRSNet.py:131-187 (view v's prediction = in_img_v *
 * sigmoid(logit); the last channel (D + 65) of view v's hr input = view v's pred_lr).  points [V][3][n] (lib/train_util.py:40-51), calibs DEVICE
 * [V][12] (rows 0..2 of each view's calibration), feat_lr [V][hl][wl][D] (D = lr->dims[0] - 65), feat_hr [V][hh][wh][64]; pred_hr / pred_lr [V][n];
 * logit_hr / logit_lr [n] nullable (what the sigmoid takes).  p_lr [V][n] non-NULL: the hr classifier alone (query_sr on other
 * points), pred_lr / logit_lr ignored.  Operand split as surs_query_points_generic; V = 1 gives its bits. */
int surs_query_points_generic_views(const float *points, int n, int num_views, const float *calibs, float zmul, float zdiv,
                                    const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const SursMlpShape *lr,
                                    const SursMlpShape *hr, const void *blob, const float *p_lr, float *pred_hr, float *pred_lr,
                                    float *logit_hr, float *logit_lr, void *stream);

/* The dense sweep of a multi-view model (eval_grid over eval_func, lib/sdf.py:32-52, lib/mesh_util.py:20-28: every grid point seen
 * by every view, view 0's predictions kept) of grid slab [i0, i1) in one launch: voxels as surs_query_grid_generic, the other
 * arguments as surs_query_points_generic_views (feat_lr [V][hl][wl][D]); vol_hr / vol_lr [(i1-i0)][ry][rz] = view 0's rows. */
int surs_query_grid_generic_views(int i0, int i1, int ry, int rz, const double *mat, int num_views, const float *calibs, float zmul,
                                  float zdiv, const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                                  const SursMlpShape *lr, const SursMlpShape *hr, const void *blob, float *vol_hr, float *vol_lr,
                                  void *stream);

/* HOST: how the multi-view evaluator runs this pair for num_views views: *tile_points per workgroup and *lds_bytes of LDS per
 * workgroup, or SURS_E_INVALID naming the limit (num_views outside [1, 64], an unsupported shape, a hidden layer wider than 1824:
 * the tile keeps the features and their running view sum in LDS - for D = lr->dims[0] - 65 above 256 less, D = 512: 1312, the
 * message then names the limit and D).  The multi-view entries need no device workspace. */
int surs_mlp_generic_views_info(const SursMlpShape *lr, const SursMlpShape *hr, int num_views, int *tile_points, int *lds_bytes);

/* surs_query_points for point arrays that come as RUNS of equal (x, y): what the reference's dense sweep loop hands
 * query_mr / query_sr - 50 000 consecutive points of the flattened grid per call, z fastest (lib/sdf.py:32-45 batch_eval,
 * lib/mesh_util.py:20-28 eval_func) - i.e. ~ 98 columns of up to 512 points with one image position each.  Such a run is a column of
 * the sweep: the restated column kernels of surs_query_grid evaluate it (per-run constants from one gather + GEMM, layer 1 as the
 * affine part + the residuals of the listed channels), every point with its own z read from `points`.  No grid is assumed: runs are
 * found in the data (bit-equal x and y, z monotonic inside a run, cut at 4096 points).
 *   points [3][n] with row pitch ld >= n (a piece of a longer array), n <= 262 144; dtype = the blob's use: SURS_F32 (kernel v11,
 *   fp32-grade: logits within 1e-4 of surs_query_points'), SURS_BF16 / SURS_F16 (kernel v10: surs_query_grid's arithmetic);
 *   *columns = the number of runs evaluated, or 0 - NOTHING WAS WRITTEN, call surs_query_points - when the array holds fewer than
 *   2048 points or more than one run per 16 (SURS_F32) / 32 (SURS_BF16, SURS_F16) points - the layer kernels are the faster evaluator there -, z is not monotonic inside the runs, or the calibration lets the image position
 *   depend on z (calib[2], calib[6]) or the depth on x, y (calib[8], calib[9]).  Synchronises the stream once (the run count). */
/* Its run finder alone (tests, diagnostics): colstart[c] / kcount[c] = first point and length of run c (ints, room for n each), tiles =
 * (run, z tile) pairs of `tile` = 64 | 128 points (room for 2 n ints), meta[4] = {runs, work items - 0 and no lengths / work items when the
 * array holds more than one run per tile / 4 points -, z ascending violated, z descending violated}.  Device pointers; no synchronisation. */
int surs_point_runs(const float *points, long long ld, int n, int tile, int *colstart, int *kcount, int *tiles, int *meta, void *stream);
/* flag[0] (device) = 1 if a[0..n) or b[0..n) (b nullable) holds a NaN or an infinity, else 0: the check behind every query of the host
 * mirror (an activation beyond the f16 range of the two-part operand split surfaces as NaN; the query is then repeated on three bf16
 * parts).  One small launch; no synchronisation. */
int surs_nonfinite(const float *a, const float *b, long long n, int *flag, void *stream);
size_t surs_query_points_columns_workspace_bytes(void);
int surs_query_points_columns(const float *points, long long ld, int n, const float *calib, float zmul, float zdiv,
                              const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob,
                              int dtype, void *workspace, size_t workspace_bytes, float *pred_hr, float *pred_lr, int *columns,
                              void *stream);

/* The same for num_views > 1 and / or the perspective projection (SurfaceClassifier.forward's view mean after layer 2,
 * lib/model/SurfaceClassifier.py:70-76; reshape_sample_tensor, lib/train_util.py:40-51; perspective,
 * lib/geometry.py:34-48).  One subject (batch 1), V views:
 *   points  [V][3][n] (the caller repeats the samples per view as reshape_sample_tensor does), calibs HOST [V][12],
 *   projection 0 = orthogonal, 1 = perspective (x, y divided by the projected z),
 *   feat_lr NHWC [V][hl][wl][256], feat_hr NHWC [V][hh][wh][64],
 *   pred_hr / pred_lr [V][n]: the one prediction of the view-mean network under each view's in-image mask
 *   (`in_img[:, None].float() * mlp(...)`, SuRSNet.py:156,183), logit_* [n] nullable. */
int surs_query_points_views(const float *points, int n, int num_views, int projection, const float *calibs, float zmul,
                            float zdiv, const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                            const void *mlp_blob, void *workspace, size_t workspace_bytes, float *pred_hr, float *pred_lr,
                            float *logit_hr, float *logit_lr, void *stream);

/* The dense sweep of such a model as one call: eval_grid's batch loop (lib/sdf.py:32-52) over eval_func (lib/mesh_util.py:20-28 -
 * every batch of grid points repeated per view, query_mr + query_sr, view 0's predictions kept) for the slab [i0, i1) of the grid
 * `mat` (rows 0..2 of create_grid's matrix, HOST float64): the voxels are generated in the gather for every view's calibration,
 * 262 144 at a time; vol_* [(i1-i0)][ry][rz].  Same kernels and bits as surs_query_points_views on create_grid's points. */
size_t surs_query_grid_views_workspace_bytes(int num_views);
int surs_query_grid_views(int i0, int i1, int ry, int rz, const double *mat, int num_views, int projection, const float *calibs,
                          float zmul, float zdiv, const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                          const void *mlp_blob, void *workspace, size_t workspace_bytes, float *vol_hr, float *vol_lr, void *stream);
size_t surs_query_views_workspace_bytes(int max_points, int num_views);

/* Dense grid sweep: voxel (i,j,k), i in [i0,i1), j in [0,ry), k in [0,rz) has world position
 * p = float32( mat[:,0]*i + mat[:,1]*j + mat[:,2]*k + mat[:,3] )  (mat HOST [12] doubles = create_grid's
 * coords_matrix rows 0..2, evaluated in double like np.matmul on the float64 grid, then cast as eval_func does).
 * vol_hr / vol_lr: [(i1-i0)][ry][rz] fp32, z fastest (the flattening of lib/sdf.py:14-15,28).
 * dtype SURS_F32: fp32-grade results (logits within 1e-4 of the reference): on an axis-aligned orthographic sweep (the projected
 * X, Y do not depend on k: true for gen_mesh's calib) the fused column kernel with split-f16 operands, otherwise - and for
 * SURS_F32_GEMM - the arithmetic of surs_query_points.  SURS_BF16 / SURS_F16: the reduced-precision column kernel (axis-aligned
 * sweeps only; otherwise returns SURS_E_UNSUPPORTED). */
int surs_query_grid(int i0, int i1, int ry, int rz, const double *mat, const float *calib, float zmul, float zdiv,
                    const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob,
                    int dtype, void *workspace, size_t workspace_bytes, float *vol_hr, float *vol_lr, void *stream);
size_t surs_query_grid_workspace_bytes(int ry, int rz, int dtype);

/* The same sweep with per-call choices instead of process-wide ones (nothing global is read for a field that is set, nothing
 * global is written): `kernel` = column-kernel version (0 = the process setting / default; reduced precision 3, 10, 12;
 * fp32-grade 5, 11 - DESIGN.md 4), `operand_parts` = operand split of the fp32-grade GEMMs behind the sweep (0 = process
 * setting, 2 = two f16 parts, 3 = three bf16 parts).  opt == NULL behaves as surs_query_grid.  Safe to call from several host
 * threads on different streams. */
typedef struct SursGridOptions {
    int kernel;
    int operand_parts;
    int reserved[6];   /* must be zero */
} SursGridOptions;
int surs_query_grid_opt(int i0, int i1, int ry, int rz, const double *mat, const float *calib, float zmul, float zdiv,
                        const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh, const void *mlp_blob,
                        int dtype, void *workspace, size_t workspace_bytes, float *vol_hr, float *vol_lr,
                        const SursGridOptions *opt, void *stream);

/* Octree sweep (eval_grid_octree, lib/sdf.py:55-120), one level at a time; volumes are float64 [R][R][R] like the
 * reference's numpy arrays, `dirty` is uint8 [R][R][R].
 *   surs_octree_select     lattice points of stride `reso` that are still dirty -> idx[] (flat voxel indices, any
 *                          order), count (host; synchronises)                                 sdf.py:68-71
 *   surs_query_grid_indexed evaluate those voxels (fp32 arithmetic, as surs_query_points)       sdf.py:73
 *   surs_octree_scatter    sdf[idx] = pred, dirty[idx] = 0                                     sdf.py:73-74
 *   surs_octree_cells      the cell walk: blocks whose 8 corners span < threshold are set to (max+min)/2 and marked
 *                          clean, HR and LR sharing the one dirty mask                          sdf.py:81-117
 *   surs_f64_to_f32        the cast marching_cubes_lewiner applies to its input */
int surs_octree_select(const unsigned char *dirty, int R, int reso, long long *idx, int cap, int *count_dev, int *count_host,
                       void *stream);
/* select + evaluate + scatter of one level in ONE call, on the sweep's fp32-grade COLUMN kernel (axis-aligned orthographic sweeps:
 * the lattice points of stride `reso` form columns along axis 2 that share their image position, so the per-column constants
 * and the restated layer 1 of surs_query_grid apply).  A column's work items are its dirty lattice points in ascending order, 64
 * per tile; exactly the points lib/sdf.py:68-74 evaluates are evaluated and written (sdf = value, dirty = 0).  A point's value
 * depends on the point, on `reso` and - in the last bits, through the tile it shares - on which other points of its column are
 * dirty: the same dirty set gives the same bits.  kmid: axis-2 voxel index where the kernel takes its per-column LeakyReLU
 * branches (R / 2; any value gives the same function up to rounding).  counts (HOST, nullable, 3 values): dirty lattice points
 * evaluated, lattice columns that held them, 64-point tiles run.  Synchronises the stream once.  SURS_E_UNSUPPORTED for a
 * general calibration: use the three calls above and below. */
int surs_octree_level_columns(double *sdf_hr, double *sdf_lr, unsigned char *dirty, int R, int reso, int kmid, const double *mat,
                              const float *calib, float zmul, float zdiv, const float *feat_lr, int hl, int wl,
                              const float *feat_hr, int hh, int wh, const void *mlp_blob, void *workspace, size_t workspace_bytes,
                              long long *counts, void *stream);
/* The same with the level's evaluator chosen: dtype SURS_F32 = the fp32-grade column kernel (what surs_octree_level_columns runs),
 * SURS_BF16 / SURS_F16 = the 16-bit column kernel on the blob's cores - the octree sweep of `--precision bf16 | fp16`. */
int surs_octree_level_columns_dt(double *sdf_hr, double *sdf_lr, unsigned char *dirty, int R, int reso, int kmid, const double *mat,
                                 const float *calib, float zmul, float zdiv, const float *feat_lr, int hl, int wl,
                                 const float *feat_hr, int hh, int wh, const void *mlp_blob, int dtype, void *workspace,
                                 size_t workspace_bytes, long long *counts, void *stream);
size_t surs_octree_columns_workspace_bytes(int R);
int surs_query_grid_indexed(const long long *idx, int n, int ry, int rz, const double *mat, const float *calib, float zmul,
                            float zdiv, const float *feat_lr, int hl, int wl, const float *feat_hr, int hh, int wh,
                            const void *mlp_blob, void *workspace, size_t workspace_bytes, float *pred_hr, float *pred_lr,
                            void *stream);
int surs_octree_scatter(const long long *idx, int n, const float *pred_hr, const float *pred_lr, double *sdf_hr, double *sdf_lr,
                        unsigned char *dirty, void *stream);
size_t surs_octree_workspace_bytes(int R, int reso);
int surs_octree_cells(double *sdf_hr, double *sdf_lr, unsigned char *dirty, int R, int reso, double threshold, void *workspace,
                      size_t workspace_bytes, void *stream);
int surs_f64_to_f32(const double *a, float *b, long long n, void *stream);

/* HOST: write a Wavefront OBJ exactly as save_obj_mesh does (lib/mesh_util.py:53-61): 'v %.4f %.4f %.4f' per vertex,
 * then 'f a c b' per face with 1-based indices and the winding swapped.  verts float64 [n_verts][3], faces int32
 * [n_faces][3] (host pointers).  threads <= 0: use all hardware threads for the formatting. */
int surs_save_obj_mesh(const char *path, const double *verts, long long n_verts, const int32_t *faces, long long n_faces,
                       int threads);

/* Measurement aid (not on the reference's path): when enabled, every launch of the dominant kernel of
 * surs_query_grid's reduced-precision mode is bracketed by HIP events on its launch stream.  surs_profile_read
 * returns the number of timed launches, the sum of their durations (ms) and the voxels they evaluated, and resets. */
int surs_profile_enable(int on);
int surs_profile_read(double *launches, double *total_ms, double *points);
/* Column kernel v7 runs a data-dependent number of layer-1 k-steps.  tile_mlps: (z tile, MLP) pairs the timed launches
 * processed; ksteps: residual k-steps (16 listed channels each) they ran, not counting the affine k-step of every pair.
 * Call before surs_profile_read, which resets the counters. */
int surs_profile_read_ksteps(double *tile_mlps, double *ksteps);

/* ------------------------------------------------------------------ Lewiner marching cubes */

typedef struct {
    int32_t n_verts;   /* vertices produced (also when SURS_E_CAPACITY) */
    int32_t n_faces;   /* triangles produced */
    float vmin, vmax;  /* data range of the volume */
} surs_mc_counts;

size_t surs_mc_workspace_bytes(int n0, int n1, int n2);
/* Extract the level set of vol [n0][n1][n2] (fp32, axis 2 fastest) exactly as
 * skimage.measure.marching_cubes_lewiner(vol, level) with default arguments does: same vertices (fp32,
 * (axis0, axis1, axis2) order), same vertex numbering, same faces (int32, rows reversed for
 * gradient_direction='descent'), normals and values.  Outputs are device buffers of capacity cap_verts /
 * cap_faces; counts is a HOST struct filled before return (this call synchronises the stream).
 * normals / values nullable.  verts == NULL or faces == NULL: count-only call (fills counts, writes nothing).
 * SURS_E_CAPACITY: counts holds the sizes needed; the rows of verts / faces below the capacities are those of the whole
 * mesh, nothing is written behind them (normals / values are not final).  Like the success path it returns with the
 * stream synchronised: nothing of the call is still in flight, the buffers and the workspace may be released or reused. */
int surs_mc_lewiner(const float *vol, int n0, int n1, int n2, double level, void *workspace, size_t workspace_bytes,
                    float *verts, float *normals, float *values, int cap_verts, int32_t *faces, int cap_faces,
                    surs_mc_counts *counts, void *stream);

/* The same extraction, incrementally, for a volume that is produced slab by slab along axis 0 (the dense sweep writes
 * whole axis-0 planes in order): processes the cell layers [layer_begin, layer_end) - they read the voxel planes
 * layer_begin .. layer_end, which must be final - and appends their vertices / faces at run->n_verts / run->n_faces
 * (HOST struct, in/out; initialise to {0, 0, +FLT_MAX, -FLT_MAX}).  Called with contiguous increasing ranges that end
 * at n0 - 1, the outputs are identical to one surs_mc_lewiner call: Lewiner's sweep has axis 0 outermost, so vertex and
 * face numbering of a layer depend only on the layers before it.  Normals / values of a vertex keep accumulating from
 * later layers: read them after the last range and surs_mc_normalize.  The level-range / no-surface checks are the
 * caller's, from run->vmin / vmax / n_verts after the last range (after every range they are those of the planes
 * 0 .. layer_end read so far).  Synchronises the stream once per call.
 * SURS_E_CAPACITY leaves run advanced to the sizes needed so far (rows below the capacities are valid and the stream is
 * synchronised, as above). */
int surs_mc_lewiner_range(const float *vol, int n0, int n1, int n2, int layer_begin, int layer_end, double level,
                          void *workspace, size_t workspace_bytes, float *verts, float *normals, float *values, int cap_verts,
                          int32_t *faces, int cap_faces, surs_mc_counts *run, void *stream);
int surs_mc_normalize(float *normals, int n_verts, void *stream);

/* Slab mode (the grid split into contiguous axis-0 slabs over ranks, marching cubes per slab; the reference
 * has no counterpart - it runs lib/mesh_util.py:40,45 on the whole volume).  `vol` is ONE slab [n0][n1][n2] whose plane 0 is
 * plane `z_offset` of the whole grid and whose last plane is the next slab's first plane (the halo), except for the top
 * slab.  surs_mc_lewiner_range_slab is surs_mc_lewiner_range (vertices and faces only) with two differences: vertex
 * coordinates are those of the whole grid (bit-identical to the one-piece extraction), and for z_offset > 0 the first cell
 * layer does not create the vertices of the x- / y-edges in plane 0 - the slab below owns them - but references them as
 * -(2 + slot), slot = axis * n1 * n2 + y * n2 + x.  Vertex / face numbers are local to the slab (run starts at 0).
 * Afterwards: surs_mc_slab_top_ids copies the ids (local numbering) of the x- / y-edge vertices in the slab's last plane to
 * ids[2][n1][n2] (entries of edges the surface does not cross are undefined) - they go to the slab above; and
 * surs_mc_slab_fixup rewrites the slab's faces to the whole mesh's numbering: v >= 0 -> v + own_offset, v < 0 ->
 * below_ids[-v - 2] + below_offset, the offsets being the exclusive sums of the slabs' vertex counts.  Concatenating the
 * slabs' vertices and faces in slab order then gives exactly the one-piece result. */
int surs_mc_lewiner_range_slab(const float *vol, int n0, int n1, int n2, int layer_begin, int layer_end, double level,
                               void *workspace, size_t workspace_bytes, float *verts, int cap_verts, int32_t *faces, int cap_faces,
                               surs_mc_counts *run, int z_offset, void *stream);
int surs_mc_slab_top_ids(const void *workspace, size_t workspace_bytes, int n0, int n1, int n2, int32_t *ids, void *stream);
int surs_mc_slab_fixup(int32_t *faces, long long n_faces, int own_offset, const int32_t *below_ids, int below_offset, void *stream);

/* out[i] = mat[:3,:3] @ verts[i] + mat[:3,3] in float64 (mat HOST [12] doubles, rows 0..2 of the 4x4 index->world
 * matrix): the vertex transform of lib/mesh_util.py:42-43,47-48.  verts fp32 [n][3], out fp64 [n][3]. */
int surs_transform_points(const float *verts, int n, const double *mat, double *out, void *stream);

/* ---------------------------------------------------------------- training samples
 * What TrainDataset_LR_v2.select_sampling_method (lib/data/TrainDataset_LR_v2.py:357-438) makes per item, on the device:
 * the pool of jittered surface samples and box points, the inside / outside test of the pool against the HR and the LR mesh,
 * the truncated selection and the displacement labels.  A mesh is verts [nv][3] fp32 and faces [nf][3] int32 (indices are
 * clamped to [0, nv): a bad index reads a wrong vertex, never out of bounds).  Every call returns the same bits for the same
 * arguments (no atomics, fixed summation orders). */

/* Triangles per face part of surs_mesh_contains, and the pool entries surs_sample_select's workgroup takes per round. */
#define SURS_MESH_FACES_PER_PART 4096
#define SURS_SAMPLE_SELECT_CHUNK 1024

/* inside[i] = |w(p_i)| > 0.5, w the generalized winding number of the mesh around p_i = points[i * ld .. + 3] (ld >= 3):
 *     w(p) = 1/(4 pi) sum_f 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|),   a, b, c = v - p,
 * summed by brute force over all faces (no acceleration structure).  The absolute value makes a consistently inward-oriented
 * mesh answer like a parity test.  A zero-area triangle and a triangle with a vertex at p contribute 0: the result is finite
 * for finite input.  winding (nullable) receives w.  The faces are split into surs_mesh_contains_parts(nf) parts of
 * SURS_MESH_FACES_PER_PART - a function of nf alone -, each part's sum goes to workspace [parts][n] floats and the parts are
 * added in index order: a point's bits do not depend on n or on the other points of the call. */
int surs_mesh_contains_parts(int nf);
size_t surs_mesh_contains_workspace_bytes(int n, int nf);
int surs_mesh_contains(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf,
                       void *workspace, size_t workspace_bytes, unsigned char *inside, float *winding, void *stream);

/* cdf[f] = sum of the areas of faces 0 .. f, float64 [nf]; the area 0.5 |(v1 - v0) x (v2 - v0)| in float64 from the fp32
 * vertices. */
int surs_mesh_area_cdf(const float *verts, int nv, const int32_t *faces, int nf, double *cdf, void *stream);

/* One item's pool: points [n_surface + n_box][3] fp32, surface samples first, in generation order.  Every random number is
 * value i of a named stream of the package's counter PRNG (prng.py: splitmix64(fnv1a64(name) ^ seed * GOLDEN + i), top 24
 * bits / 2^24; the names are "train_samples_" + face, r1, r2, jitter_radius, jitter_angle, box, shuffle).
 * Surface sample i: the first face f with cdf[f] > u_face[i] * cdf[nf - 1]; (r1, r2) = (u_r1[i], u_r2[i]), reflected to
 * (1 - r1, 1 - r2) if r1 + r2 > 1; p = v0 + r1 (v1 - v0) + r2 (v2 - v0); coordinate c gains sigma * sqrt(-2 ln((k + 1) / 2^24))
 * cos(2 pi u_angle[3 i + c]), k the 24 bits of jitter_radius[3 i + c].  Box sample j: b_min + u_box[3 j + c] * (b_max - b_min).
 * b_min / b_max: HOST [3].  sort_keys [n_surface + n_box] int64 receives the shuffle stream's raw 64-bit value with the top bit
 * flipped: sorting them as signed integers (ties by index) is the shuffle.  face_index (nullable, int32 [n_surface]) receives
 * each surface sample's face. */
int surs_mesh_sample_pool(const float *verts, int nv, const int32_t *faces, int nf, const double *cdf, unsigned long long seed,
                          int n_surface, int n_box, float sigma, const float *b_min, const float *b_max, float *points,
                          long long *sort_keys, int32_t *face_index, void *stream);

/* The selection of lines 390-423 on the shuffled pool [n_pool] (row pitch ld >= 3) and its two flag arrays, n =
 * num_sample_inout (even).  Per mesh: more than n / 2 points inside -> the first n / 2 inside, then the first n / 2 outside;
 * otherwise all inside points, then the first n - nin outside; pool order kept.  samples_hr [3][n], labels_hr [n] (1 inside),
 * samples_lr [3][n]; labels_disp [n] = n / 2 ones then n / 2 zeros, entry i of each half overwritten for i < len(inside_LR)
 * with the HR flag of the i-th selected inside / outside LR point (the reference's `p in outside_points_HR` / `in
 * inside_points_HR`).  Where the pool has fewer outside points than the rule takes, the reference returns shorter arrays (or
 * fails in its loop); here the columns behind the selection are zero and counts (nullable, DEVICE int32 [4]) receives the
 * selected (inside HR, outside HR, inside LR, outside LR).  One launch, no host synchronisation. */
int surs_sample_select(const float *pool, int ld, int n_pool, const unsigned char *inside_hr, const unsigned char *inside_lr,
                       int n, float *samples_hr, float *labels_hr, float *samples_lr, float *labels_disp, int32_t *counts,
                       void *stream);

/* ---------------------------------------------------------------- mesh distance
 * How far a set of points lies from a mesh: what point-to-surface (P2S) and Chamfer distance are made of.  A mesh as in "training
 * samples" (indices clamped to [0, nv)); brute force over all faces, no acceleration structure, no atomics: the same arguments give
 * the same bits.
 *
 * dist[i] = sqrt(min_f d2(p_i, f)) (a correctly rounded square root), p_i = points[i * ld .. + 3] (ld >= 3), and face[i] (nullable)
 * the LOWEST face index that attains that minimum in fp32.  d2 is the squared distance to the triangle in fp32 (csrc/
 * surs_mesh_distance.h, one arithmetic for host and device): the minimum over the three edges of |x - clamp(s, 0, 1) e|^2, s = x.e /
 * e.e, replaced by (ap.n)^2 / n.n where the triangle has an area and the point's projection falls inside it; no squared lengths are
 * subtracted.  A zero-area triangle is its three segments, a repeated vertex a point: the result is finite for finite input.  A
 * point with a NaN or infinite coordinate gets dist = +inf and face = -1 (the initial value: every comparison with it is false).
 * The faces are split into surs_mesh_contains_parts(nf) parts of SURS_MESH_FACES_PER_PART - a function of nf alone -; each part
 * keeps its minimum with a strict < in face order and writes it to workspace [parts][n] entries of (fp32 d2, int32 face), and the
 * parts are combined in index order with a strict < again.  A point's two results do not depend on n, on ld, on its position in
 * the array or on the other points of the call.
 * SURS_E_INVALID, before anything is launched: n < 0, nf < 1, nv < 1, ld < 3, a NULL array, a workspace smaller than
 * surs_mesh_distance_workspace_bytes(n, nf) (which is 0 for n < 1 or nf < 1).  n == 0 is success and launches nothing.
 * surs_mesh_distance_host is the same header looped on the HOST (all pointers host pointers): the kernel's bits, no device. */
size_t surs_mesh_distance_workspace_bytes(int n, int nf);
int surs_mesh_distance(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf,
                       void *workspace, size_t workspace_bytes, float *dist, int32_t *face, void *stream);
int surs_mesh_distance_host(const float *points, int n, int ld, const float *verts, int nv, const int32_t *faces, int nf,
                            float *dist, int32_t *face);

/* ---------------------------------------------------------------- mesh raster
 * Which triangle of a mesh each pixel of an orthographic view sees, with its depth and barycentric coordinates, and the normal map
 * made from them: what the normal reprojection error of the papers (metrics.normal_error) is made of.  The reference renders these
 * maps with OpenGL (lib/renderer/gl); the camera conventions are those of its orthographic camera (lib/renderer/camera.py:149-156,
 * the ortho_ratio branch of get_gl_matrix) and of the calib product in lib/data/TrainDataset_LR_v2.py:242-254 and :315-316
 * (calib = trans_intrinsic . uv_intrinsic . scale_intrinsic . extrinsic; scale_intrinsic = diag(s, -s, s): y' downwards, a POSITIVE
 * z entry; --random_flip negates its x entry, :274).  A mesh as in
 * "training samples" (indices clamped to [0, nv)); brute force over all faces, no lists, no atomics: the same arguments give the same
 * bits.  The arithmetic is csrc/surs_mesh_raster.h, one for host and device.
 *
 * view[12] is a row-major 3 x 4 matrix, the top three rows of such a calib: (x', y', z') = view . (x, y, z, 1), orthographic, x' and
 * y' in [-1, 1] over the image, y' growing DOWNWARDS.  The camera looks from the +z' side: of two surfaces over a pixel the one with
 * the LARGER z' is seen.  The image has h rows and w columns; pixel (i, j) is sampled at its centre x' = (2j + 1) / w - 1, y' =
 * (2i + 1) / h - 1.  A pixel is covered by a triangle where all three barycentric coordinates of its centre are >= 0 (edges
 * inclusive, either winding, no culling); a triangle with zero projected area, a non-finite coordinate or no pixel centre in its
 * bounding box covers nothing.  The winner of a pixel is the covering triangle with the largest z', the LOWEST face index among equal
 * z' (a strict > over the faces in order).
 *   face  [h, w]     int32   the winner, -1 on background
 *   depth [h, w]     fp32    its z' at the pixel centre, NaN on background (nullable)
 *   bary  [h, w, 2]  fp32    the weights (b1, b2) of the winner's vertices with the middle and the largest INDEX (a face's three
 *                            vertices are taken in ascending index order, so a mesh and its copy with every face turned round
 *                            give the same bits); (0, 0) on background (nullable)
 * The faces are split into surs_mesh_raster_parts(nf) parts of the option raster_part (a multiple of 256) - a function of nf and the
 * option alone; the workspace holds a 16-byte pixel box per face and [parts][h * w] entries of (z', face, b1, b2), combined in index
 * order with the strict > again.  A pixel's results do not depend on the image it sits in, on the part size or on the workspace.
 *
 * surs_mesh_shade_normals writes out [h, w, 3] fp32: on a covered pixel the colour 0.5 n + 0.5 of the winner's unit normal n in the
 * VIEW frame, turned to face the camera (n_z' >= 0, whatever the triangle's orientation and the view's handedness); (0, 0, 0) on
 * background.  Without vertex_normals n is the cross product of the triangle's projected edges (flat); with vertex_normals [nv, 3] it
 * is normal_matrix[9] (row-major 3 x 3) times the barycentric blend of the three vertices' normals (smooth; bary is then needed).
 * SURS_E_INVALID, before anything is launched or written: a NULL array (depth, bary of the raster and vertex_normals are nullable;
 * normal_matrix and bary of the shading only where vertex_normals is NULL), w or h outside [1, 8192], nf < 1, nv < 1, an option
 * raster_part that is no positive multiple of 256, more than 65535 parts, a workspace smaller than
 * surs_mesh_raster_workspace_bytes(w, h, nf) (which is 0 for w, h or nf < 1).
 * The _host entries are the same header looped on the HOST (all pointers host pointers): the kernels' bits, no device. */
int surs_mesh_raster_parts(int nf);
size_t surs_mesh_raster_workspace_bytes(int w, int h, int nf);
int surs_mesh_raster(const float *verts, int nv, const int32_t *faces, int nf, const float *view, int w, int h, void *workspace,
                     size_t workspace_bytes, int32_t *face, float *depth, float *bary, void *stream);
int surs_mesh_shade_normals(const float *verts, int nv, const int32_t *faces, int nf, const float *view, const float *vertex_normals,
                            const float *normal_matrix, const int32_t *face, const float *bary, int w, int h, float *out, void *stream);
int surs_mesh_raster_host(const float *verts, int nv, const int32_t *faces, int nf, const float *view, int w, int h, int32_t *face,
                          float *depth, float *bary);
int surs_mesh_shade_normals_host(const float *verts, int nv, const int32_t *faces, int nf, const float *view,
                                 const float *vertex_normals, const float *normal_matrix, const int32_t *face, const float *bary, int w,
                                 int h, float *out);

/* ---------------------------------------------------------------- mesh PRT
 * Per-vertex precomputed radiance transfer: what a textured scan needs before its training views can be lit and rendered
 * (surs_amd/render.py, apps/render_data.py).  The reference's renderer (lib/renderer, OpenGL) reads such vectors from a ray-traced
 * preprocessing step it does not ship; this is that step, by brute force over all faces, stated independently:
 *   prt[v][i] = (4 pi / D) sum_k V(v, d_k) max(0, n_v . d_k) Y_i(d_k),     k = 0 .. D - 1 in index order, one fp32 accumulator each,
 * a term with n . d_k <= 0 skipped, the scale 12.566371f / D applied once at the end.  Y_0..8: the real spherical harmonics of bands
 * 0 - 2 in the order l (l + 1) + m: 0.282095; 0.488603 (y, z, x); 1.092548 xy, 1.092548 yz, 0.315392 (3 z^2 - 1), 1.092548 xz,
 * 0.546274 (x^2 - y^2).  V = 0 where the ray from v + offset n along d_k hits a triangle at t > 0 - Moeller-Trumbore, edges inclusive
 * (u >= 0, v >= 0, u + v <= 1), a triangle that lists v as a corner (by INDEX) skipped, a zero-area or non-finite triangle hitting
 * nothing -, else 1.  A vertex with a non-finite position or normal gets 0.  A mesh as in "training samples" (indices clamped to
 * [0, nv)); normals [nv, 3] unit vectors, dirs [D, 3] unit vectors (an argument: render.prt_directions makes the default set), prt
 * [nv, 9].  The arithmetic is csrc/surs_mesh_prt.h, one for host and device: the same arguments give the same bits, and a vertex's
 * bits depend neither on nv, nor on its place in the array, nor on the workspace.
 * The faces stream through LDS SURS_MESH_PRT_CHUNK at a time; the workspace holds one bit per (vertex, direction) pair,
 * surs_mesh_prt_workspace_bytes(nv, D) (0 for nv or D < 1 or more than 2^31 - 512 pairs), whatever the number of faces.
 * SURS_E_INVALID, before anything is launched or written: a NULL array, nv < 1, nf < 1, D < 1, more than 2^31 - 512 pairs, an offset
 * that is negative or not finite, a workspace that is too small.
 * surs_mesh_prt_host is the same header looped on the HOST (all pointers host pointers): the kernels' bits, no device; visible
 * (nullable) [nv, D] gets 1 where a pair contributed (n . d > 0 and nothing hit), else 0.
 * surs_mesh_prt_counted is surs_mesh_prt - the same bits - that also writes wave_tests [ceil(nv D / 64)] uint32 (device, not NULL):
 * the number of triangles each wave of 64 rays looked at before it left the face loop; 64 times their sum is the number of ray -
 * triangle tests executed (tools/gpu_render_time.py). */
#define SURS_MESH_PRT_CHUNK 512
size_t surs_mesh_prt_workspace_bytes(int nv, int D);
int surs_mesh_prt_counted(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs, int D,
                          float offset, float *prt, void *workspace, size_t workspace_bytes, uint32_t *wave_tests, void *stream);
int surs_mesh_prt(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs, int D, float offset,
                  float *prt, void *workspace, size_t workspace_bytes, void *stream);
int surs_mesh_prt_host(const float *verts, int nv, const int32_t *faces, int nf, const float *normals, const float *dirs, int D,
                       float offset, float *prt, uint8_t *visible);

/* ---------------------------------------------------------------- mesh shading
 * The colour of a rastered view: texture, spherical-harmonic lighting, gamma, and the box resolve that stands in for multisampling.
 * The arithmetic is csrc/surs_mesh_shade.h, one for host and device, and calls no math library (its log2 / exp2 are short fp32
 * polynomials): the same arguments give the same bits on both sides.
 *
 * surs_texture_pyramid: tex [h, w, 3] uint8, row 0 the TOP of the image -> levels, surs_texture_pyramid_floats(w, h) floats: level 0
 * (tex / 255) and three further levels, each the 2 x 2 mean of the one above, packed one after the other.  w and h multiples of 8 in
 * [8, 16384], else SURS_E_INVALID (and 0 floats).
 *
 * surs_mesh_shade_prt: face [h, w] and bary [h, w, 2] as surs_mesh_raster wrote them for (verts, faces, view, w, h) -> rgba [h, w, 4]
 * fp32.  Corners are the raster's (ascending vertex index); faces_uv [nf, 3] is given in the FACE's own corner order and permuted
 * inside the call.  Per covered pixel: uv = the barycentric blend of the corners' uvs [nuv, 2]; albedo = a trilinear lookup in
 * `pyramid` (tw x th; bilinear within a level, clamp to edge, texel centres at (i + 1/2) / size, v = 0 the LAST row), the level
 * lambda = clamp(1/2 log2(A_tex / A_pix), 0, 3) constant per face (A_tex: its uv area in level-0 texels, A_pix: its projected area in
 * pixels); s_c = sum_i p_i light[i][c] by fma in ascending i; rgb_c = clamp(albedo_c max(s_c, 0)^(1/2.2), 0, 1), a = 1; background
 * (0, 0, 0, 0).  pyramid NULL: albedo 1 (faces_uv, uvs not read).  p is the barycentric blend of prt [nv, 9] (light [9, 3] then in
 * prt's frame, the mesh's), or - prt NULL - A_l Y_i(n) of the blended vertex normals [nv, 3] turned by normal_matrix[9] (row-major
 * 3 x 3) and normalised, A = (pi, 2 pi / 3, pi / 4): the unshadowed limit of surs_mesh_prt (light then in the frame the matrix
 * turns into).  SURS_E_INVALID: a NULL array that is read, nv or nf < 1, w or h outside [1, 8192], a texture size as above.
 * The _host twin also writes shading [h, w, 3] (nullable): s_c before the gamma.
 *
 * surs_image_resolve: rgba [h m, w m, 4] -> rgb [h, w, 3] and mask [h, w] (nullable) uint8: the mean of a pixel's m x m sub-samples,
 * added in row-major order in fp32, times 255, rounded to nearest (ties to even); mask from the alpha channel.  m in [1, 8], w m and
 * h m in [1, 8192]. */
size_t surs_texture_pyramid_floats(int w, int h);
int surs_texture_pyramid(const uint8_t *tex, int w, int h, float *levels, void *stream);
int surs_texture_pyramid_host(const uint8_t *tex, int w, int h, float *levels);
int surs_mesh_shade_prt(const int32_t *face, const float *bary, const float *verts, int nv, const int32_t *faces, int nf,
                        const float *view, const int32_t *faces_uv, const float *uvs, int nuv, const float *prt, const float *normals,
                        const float *normal_matrix, const float *light, const float *pyramid, int tw, int th, int w, int h, float *rgba,
                        void *stream);
int surs_mesh_shade_prt_host(const int32_t *face, const float *bary, const float *verts, int nv, const int32_t *faces, int nf,
                             const float *view, const int32_t *faces_uv, const float *uvs, int nuv, const float *prt,
                             const float *normals, const float *normal_matrix, const float *light, const float *pyramid, int tw, int th,
                             int w, int h, float *rgba, float *shading);
int surs_image_resolve(const float *rgba, int w, int h, int m, uint8_t *rgb, uint8_t *mask, void *stream);
int surs_image_resolve_host(const float *rgba, int w, int h, int m, uint8_t *rgb, uint8_t *mask);

/* ---------------------------------------------------------------- device repack
 * The packed images the forward reads (surs_conv_pack_weights*, the blobs of surs_mlp_pack / surs_mlp_pack_generic) rebuilt ON THE
 * DEVICE from the plain fp32 parameters an optimiser has just stepped: the bytes the host packers give for the same values, without
 * the copy to the host, the scalar host loops and the upload.  Every pointer is a device pointer - tables of pointers included -,
 * every entry enqueues on `stream`, allocates nothing and never synchronises; destinations are written in place, so addresses held by
 * a SursEncoderNet or a captured graph stay valid.  Splits as on the host: hi = f16(w), lo = f16(w - hi), round to nearest even,
 * subnormal results kept; three parts: bf16, each the rounding of what the previous parts left. */

/* One convolution of a surs_conv_repack table.  w: plain [cout][cin][ksize][ksize]; packed / x2 / x3: the images of
 * surs_conv_pack_weights / _x2 / _x3, each nullable (not written).  tile_end: the number of tiles of this item and of every item in
 * front of it in the table (the inclusive prefix sum of surs_conv_repack_tiles) - how a workgroup finds its item. */
typedef struct SursRepackItem {
    const float *w;
    int cout, cin, ksize;
    int tile_end;
    float *packed;
    void *x2;
    void *x3;
} SursRepackItem;

/* tiles (64 output channels x 16 input channels of a 3x3, x 64 of a 1x1 convolution) of one item; 0 for an unsupported shape */
int surs_conv_repack_tiles(int cout, int cin, int ksize);
/* Writes every image the n items of the DEVICE table name, in full, padding included (a destination that held garbage is valid
 * afterwards), in ONE launch over the tiles of all items.  A source tile goes through LDS: loads are contiguous runs of the source's
 * rows, stores contiguous runs of the images.  ksize 1 or 3. */
int surs_conv_repack(const SursRepackItem *items, int n, void *stream);

/* The stack joint previous + bl(t) + al(l(t)) as one pointwise convolution (lib/model/HGFilters.py:203-206):
 * w_out [256][256] = w_bl + w_al [256][d] . w_l [d][256], b_out [256] = b_bl + w_al . b_l + b_al; the sums over the d (--hg_dim)
 * channels in double, in index order, then rounded to fp32.  w_out is the plain weight surs_conv_repack then packs. */
int surs_conv1x1_merge(const float *w_bl, const float *b_bl, const float *w_al, const float *b_al, const float *w_l, const float *b_l,
                       int d, float *w_out, float *b_out, void *stream);

/* Rewrites every section of an existing surs_mlp_pack blob (released shape) behind its header from the plain Conv1d weights
 * [out][in] and biases [out]: w_lr, b_lr, w_hr, b_hr are DEVICE tables of five device pointers each.  dtype: SURS_BF16 / SURS_F16, the
 * blob's own (the header is neither read nor written).  Byte for byte what surs_mlp_pack gives for the same values. */
int surs_mlp_repack(int dtype, const float *const *w_lr, const float *const *b_lr, const float *const *w_hr, const float *const *b_hr,
                    void *blob, void *stream);
/* The same for a surs_mlp_pack_generic blob: the one-, two- and three-part images and the biases of every layer, padding included
 * (lr, hr HOST; the tables DEVICE, n_layers pointers each). */
int surs_mlp_repack_generic(const SursMlpShape *lr, const float *const *w_lr, const float *const *b_lr, const SursMlpShape *hr,
                            const float *const *w_hr, const float *const *b_hr, void *blob, void *stream);
/* The two entries above as plain HOST loops over the same per-element arithmetic (csrc/surs_repack_gather.h): every pointer a HOST
 * pointer, no device needed.  What the gather form is held against the host packers with; not a path of the product. */
int surs_mlp_repack_host(int dtype, const float *const *w_lr, const float *const *b_lr, const float *const *w_hr,
                         const float *const *b_hr, void *blob);
int surs_mlp_repack_generic_host(const SursMlpShape *lr, const float *const *w_lr, const float *const *b_lr, const SursMlpShape *hr,
                                 const float *const *w_hr, const float *const *b_hr, void *blob);

/* ---------------------------------------------------------------- optimiser step
 * optimizerG.step() of the reference's training loop (apps/train_SuRS.py:54-72, :148) on the plain fp32 parameters: SGD (momentum,
 * dampening 0, no Nesterov), ADAM, AMSgrad and RMSprop (momentum 0, not centred), weight decay as an L2 term of the gradient
 * (g + wd p), in the order of operations of torch.optim's single-tensor path (csrc/surs_optim_update.h has the arithmetic, one
 * function per kind).  ONE launch updates every tensor of a device table in place; what it leaves is what surs_conv_repack /
 * surs_mlp_repack then pack.  Every element's new bits depend on its own old values alone: equal inputs give equal bits wherever
 * the buffers lie.  Non-finite gradients propagate as they do in torch. */
enum { SURS_OPTIM_SGD = 0, SURS_OPTIM_ADAM = 1, SURS_OPTIM_AMSGRAD = 2, SURS_OPTIM_RMSPROP = 3 };

/* One parameter tensor of a surs_optim_step table; every pointer a device pointer (a host pointer for surs_optim_step_host). */
typedef struct SursOptimItem {
    float *p;            /* value, updated in place */
    const float *g;      /* gradient, read only */
    float *s0, *s1, *s2; /* state, updated in place: SGD buf (NULL with momentum 0) | ADAM m, v | AMSgrad m, v, vmax | RMSprop sq;
                          * the ones a kind does not use are neither read nor written and may be NULL */
    long long n;         /* elements; 0 is legal and costs nothing */
    int chunk_end;       /* the inclusive prefix sum of surs_optim_chunks(n) over the table: how a workgroup finds its item */
    int reserved;
} SursOptimItem;

/* The hyper-parameters of one step: kernel ARGUMENTS, not table entries - a changed learning rate or step count uploads nothing.
 * The caller forms the step-dependent scalars in double and rounds them to fp32; the kernel takes no powers. */
typedef struct SursOptimHyper {
    int kind;            /* SURS_OPTIM_* */
    int first_step;      /* SGD with momentum: 1 on the optimiser's first step (buf = g), else 0 (buf = momentum buf + g) */
    float lr, weight_decay, momentum;
    float beta1_c;       /* 1 - beta1 */
    float beta2, beta2_c;/* beta2, 1 - beta2 */
    float alpha, alpha_c;/* RMSprop: alpha, 1 - alpha */
    float eps;
    float step_size;     /* ADAM / AMSgrad: lr / (1 - beta1^t), t the 1-based step */
    float bc2_sqrt;      /* ADAM / AMSgrad: sqrt(1 - beta2^t) */
} SursOptimHyper;

/* workgroup visits (chunks of 4096 elements) of an item of n elements: ceil(n / 4096), 0 for n <= 0 */
int surs_optim_chunks(long long n);
/* Checks a HOST copy of a table against `h`, as a caller does once when it builds the table: SURS_E_INVALID for an unknown kind, a
 * null p or g (of an item with n > 0), a missing state pointer the kind needs, n < 0, or a chunk_end that is not the prefix sum. */
int surs_optim_check(const SursOptimItem *items, int n_items, const SursOptimHyper *h);
/* One launch (256-thread workgroups, at most 2048, striding over the chunks of all items) on `stream`: items a DEVICE table, h
 * HOST.  16-byte loads and stores wherever every pointer of the item is 16-byte aligned at the chunk, scalar access otherwise and
 * for the n % 4 tail.  No LDS, no atomics, no allocation, no synchronisation.  Refuses (nothing launched) an unknown kind, a null
 * table and n_items < 0; n_items == 0 does nothing.  The table itself is on the device: surs_optim_check is its check. */
int surs_optim_step(const SursOptimItem *items, int n_items, const SursOptimHyper *h, void *stream);
/* The same arithmetic looped on the HOST (items a HOST table of HOST pointers), after surs_optim_check: nothing is written when it
 * refuses.  What the kernel is held against bit for bit, and torch.optim without a device; not a path of the product. */
int surs_optim_step_host(const SursOptimItem *items, int n_items, const SursOptimHyper *h);

/* The data-parallel step: R ranks have all-gathered their gradient slabs into one buffer, and the gradient of element i of an item
 * is read as g[i + r * rank_stride], r = 0 .. num_ranks - 1 (g points into rank 0's row).  The value handed to the unchanged
 * per-kind update is
 *     ((g_0 + g_1) + ... + g_{R-1}) * scale
 * - fp32 sums LEFT TO RIGHT IN RANK ORDER, starting from g_0 (not from zero: -0 stays -0), then ONE fp32 product with scale, skipped
 * when scale == 1.0f.  It is formed in registers in the pass that applies it and never written: no float atomics, no library
 * reduction whose order depends on a backend or a ring, and every rank computes the same bits from the same bytes.  Otherwise
 * surs_optim_step: its chunking, its grid, its 16-byte path (which here also needs rank_stride % 4 == 0; scalar access otherwise),
 * its refusals, and additionally SURS_E_INVALID for num_ranks outside 1 .. 64, rank_stride < 0 and a NaN scale.  num_ranks == 1 with
 * scale == 1.0f gives surs_optim_step's bits.  Non-finite gradients of any rank propagate (see surs_tensors_nonfinite for the guard:
 * run over the gathered buffer as num_ranks refs of one row each, the lowest index is the lowest offending rank). */
int surs_optim_step_ranks(const SursOptimItem *items, int n_items, const SursOptimHyper *h, int num_ranks, long long rank_stride,
                          float scale, void *stream);
/* The same loop on the HOST (host table, host pointers), after surs_optim_check and the checks above: what the kernel is held
 * against bit for bit. */
int surs_optim_step_ranks_host(const SursOptimItem *items, int n_items, const SursOptimHyper *h, int num_ranks, long long rank_stride,
                               float scale);

/* One tensor of a surs_tensors_pack table: n floats copied from src to dst (device pointers; host pointers for the host twin). */
typedef struct SursPackItem {
    const float *src;
    float *dst;
    long long n;         /* elements; 0 is legal and costs nothing */
    int chunk_end;       /* the inclusive prefix sum of surs_optim_chunks(n) over the table, as in SursOptimItem */
    int reserved;
} SursPackItem;

/* Checks a HOST copy of a table: SURS_E_INVALID for n < 0, a null src or dst of an item with n > 0, or a chunk_end that is not the
 * prefix sum.  Ranges must not overlap (not checked). */
int surs_tensors_pack_check(const SursPackItem *items, int n_items);
/* ONE launch on `stream` copies every item of the DEVICE table: how a rank's gradient tensors reach its send slab.  The optimiser
 * step's chunking and grid; 16-byte access where src and dst are both 16-byte aligned at the chunk, scalar otherwise and for the
 * n % 4 tail.  A copy: no sums, so no order to state.  n_items == 0 does nothing. */
int surs_tensors_pack(const SursPackItem *items, int n_items, void *stream);
/* The same copy on the HOST, after surs_tensors_pack_check: nothing is written when it refuses. */
int surs_tensors_pack_host(const SursPackItem *items, int n_items);

/* ---------------------------------------------------------------- training step
 * What one iteration of the reference's training loop (apps/train_SuRS.py:122-148) needs besides the taped forwards, their backwards
 * and the optimiser step: the loss with the gradient of its image term, and a guard against non-finite gradients
 * (csrc/surs_train_step.hip).
 *
 * surs_forward_losses_grad: surs_forward_losses on images in the layouts a training step has them in - img_sr [batch][height][width]
 * [channels], the model's own NHWC memory; img_hr [batch][channels][height][width], as the dataset hands it - with k = batch channels
 * height width.  terms and total are bit for bit what surs_forward_losses gives on the same values flattened in NCHW order: the same
 * partition over the NCHW index, the same float64 partial sums and second stage; only the address of img_sr differs.  d_img_sr
 * (nullable; [batch][height][width][channels], needs weights and both images, not img_sr itself): the gradient of weights[2] terms[2],
 * ((float)weights[2] * (1.0f / (float)k)) sign(img_sr - img_hr) - the fp32 reciprocal of k and one fp32 product, which is how torch
 * divides a device tensor by a host scalar, so these are the bits of weights[2] * l1_loss(img_sr, img_hr).backward(); the difference in
 * fp32, 0 at equality; a NaN difference gives NaN (torch.sign gives 0 there).  No atomics, no synchronisation. */
size_t surs_forward_losses_grad_workspace_bytes(void);
int surs_forward_losses_grad(const float *pred_lr, const float *pred_hr, int num_stacks, long long m, const float *lab_lr,
                             const float *lab_hr, const float *img_sr, const float *img_hr, int batch, int channels, int height,
                             int width, const float *weights, void *workspace, size_t workspace_bytes, float *terms, float *total,
                             float *d_img_sr, void *stream);
/* d_img_sr alone, looped on the HOST from the same per-element rule (every pointer a host pointer) */
int surs_forward_losses_grad_host(const float *img_sr, const float *img_hr, int batch, int channels, int height, int width, float w_sr,
                                  float *d_img_sr);

/* One tensor of a surs_tensors_nonfinite table: a device pointer (a host pointer for the host twin). */
typedef struct SursTensorRef {
    const float *p;
    long long n;         /* elements; 0 is legal and costs nothing */
    int chunk_end;       /* the inclusive prefix sum of surs_optim_chunks(n) over the table, as in SursOptimItem */
    int reserved;
} SursTensorRef;

/* Checks a HOST copy of a table (n < 0, a null pointer with n > 0, a chunk_end that is no prefix sum: SURS_E_INVALID) and returns
 * its chunk count through *total_chunks (nullable). */
int surs_tensors_nonfinite_check(const SursTensorRef *items, int n_items, long long *total_chunks);
size_t surs_tensors_nonfinite_workspace_bytes(long long total_chunks);
/* *result (device) = the lowest index of the DEVICE table `items` whose tensor holds a NaN or an infinity, or -1.  Two launches on
 * `stream`: 256-thread workgroups striding over the 4096-element chunks of all items (the chunking of surs_optim_step; 16-byte loads
 * where the chunk is 16-byte aligned) leave one int per chunk in the workspace, one workgroup takes their minimum in chunk order.
 * total_chunks: what surs_tensors_nonfinite_check returned for the table - the kernel visits no chunk beyond it.  No atomics, no
 * synchronisation; the caller reads the 4 bytes of *result when it needs the answer. */
int surs_tensors_nonfinite(const SursTensorRef *items, int n_items, long long total_chunks, void *workspace, size_t workspace_bytes,
                           int *result, void *stream);
/* The same predicate looped on the HOST (items a HOST table of HOST pointers, *result a host int), after the table's check. */
int surs_tensors_nonfinite_host(const SursTensorRef *items, int n_items, int *result);

/* ---------------------------------------------------------------- training images
 * The image half of a training item (lib/data/TrainDataset_LR_v2.py:258-342) from the decoded uint8 pixels of one view: pad, flip,
 * --random_scale resize, crop, torchvision's ColorJitter, --aug_blur, the BICUBIC / NEAREST half-size pair and the float32 step of
 * surs_image_prepare.  Every 8-bit intermediate is byte for byte what Pillow gives for the same parameters (INTEGRATION.md "Training
 * images" names the version checked); the arithmetic is csrc/surs_train_image.h, one for host and device.  What Pillow computes per
 * image in double - filter weights, nearest indices, box lengths - is computed by surs_train_image_plan on the HOST, into a plan (a
 * plain struct, a kernel argument) and a block of tables the caller copies to the device.  No float atomics, no host
 * synchronisation: equal arguments give equal bits.
 *
 * Images are tightly packed: rgb [h][w][3], mask [h][w], uint8.  Stages:
 *   geometry  ImageOps.expand(pad, fill 0), the horizontal flip and crop((x0, y0, x0 + out_w, y0 + out_h)) are index maps of the
 *             source fetch; in between, the render goes through Pillow's two-pass fixed-point resample (filter BILINEAR) to
 *             full_w x full_h and the mask through NEAREST (the affine-scale path).  Only the window is computed; it is 0 where it
 *             lies outside the resized image.  full size == padded size is a copy (weights 2^22 and 0), as in Pillow.
 *   jitter    n_ops of brightness / contrast / saturation (Image.blend with the degenerate image) and hue (8-bit HSV and back), in
 *             the plan's order.  The contrast mean is the exact integer sum of L over the image as it stands: one uint32 partial sum
 *             per workgroup of 1024 pixels into the workspace, added up by every workgroup of the second pass.
 *   blur      GaussianBlur(radius): three extended-box passes along x, then three along y, each rounded to 8 bits.
 *   pair      render_LR = BICUBIC to (w / 2, h / 2), mask_LR = NEAREST, fused with the float32 step; surs_image_prepare for HR.
 * With augment == 0 (phase test) only the pair runs, on the source as it is. */
enum { SURS_FILTER_NEAREST = 0, SURS_FILTER_BILINEAR = 2, SURS_FILTER_BICUBIC = 3 };   /* Pillow's numbers */
enum { SURS_JITTER_BRIGHTNESS = 0, SURS_JITTER_CONTRAST = 1, SURS_JITTER_SATURATION = 2, SURS_JITTER_HUE = 3 };

/* One resample: source, index maps, target size, window, and where its tables lie (byte offsets into the plan's table block).
 * Per axis: bounds [out][2] (first source index, count), weights [out][ksize], nearest [out] (-1: outside), tile spans [tiles][2]
 * (first and one-past-last source index any output of a 32-pixel tile reads); all int32. */
typedef struct SursImageResample {
    int src_w, src_h;          /* the stored source image */
    int pad, flip;             /* a zero border of pad pixels on every side, then a horizontal flip */
    int full_w, full_h;        /* the size the padded image is resampled to */
    int x0, y0, out_w, out_h;  /* the window of the resampled image that is computed */
    int filter;                /* SURS_FILTER_BILINEAR or SURS_FILTER_BICUBIC (the render); the mask is always NEAREST */
    int ksize_x, ksize_y;
    int off_xb, off_xk, off_xn, off_xt, off_yb, off_yk, off_yn, off_yt;
    int reserved;
} SursImageResample;

typedef struct SursTrainImagePlan {
    int augment;               /* 1: geometry, jitter, blur, pair; 0: pair only (geo is not read) */
    int w, h;                  /* the HR image: geo's window, or the source with augment 0 */
    SursImageResample geo, lr;
    int n_ops;                 /* jitter ops in the order applied */
    int op_kind[4];            /* SURS_JITTER_* */
    float op_factor[4];        /* the blend factor of the first three kinds */
    int hue_shift;             /* (int)(hue_factor * 255) & 255 */
    int blur_radius;           /* per box pass: integer part, ww and fw of BoxBlur.c; ww == 0: no blur */
    unsigned blur_ww, blur_fw;
    unsigned long long tables_bytes;
} SursTrainImagePlan;

/* Fills *r and, where `tables` is not NULL, its tables from byte `base` of the block on (a HOST block of tables_bytes); returns the
 * bytes the tables take through *used (nullable).  SURS_E_INVALID: sizes < 1, a filter other than the two above, a block too small,
 * or a tile that needs more than 80 source pixels along an axis (a reduction beyond about 2.2 for BICUBIC). */
int surs_image_resample_plan(int src_w, int src_h, int pad, int flip, int full_w, int full_h, int filter, int x0, int y0, int out_w,
                             int out_h, SursImageResample *r, void *tables, size_t tables_bytes, size_t base, size_t *used);
/* The plan of one view.  order[4]: torchvision's fn_idx; factor[4]: brightness, contrast, saturation, hue; bit k of active: op k
 * has a non-zero amount (the others are skipped, as torchvision skips None).  blur_radius: GaussianBlur's (0: none).  With augment 0
 * everything but src_w, src_h is ignored.  tables NULL: only *plan (with tables_bytes) is filled.  SURS_E_INVALID also for a box
 * radius per pass above 20 (a Gaussian radius above about 21.4) and an order that is no permutation. */
int surs_train_image_plan(int src_w, int src_h, int augment, int pad, int flip, int full_w, int full_h, int x0, int y0, int out_w,
                          int out_h, const int *order, const double *factor, int active, double blur_radius,
                          SursTrainImagePlan *plan, void *tables, size_t tables_bytes);
/* Two HR renders, the HR mask and the partial sums; 0 for a NULL plan */
size_t surs_train_images_workspace_bytes(const SursTrainImagePlan *plan);
/* The whole chain of one view on `stream`: tables, rgb, mask, workspace DEVICE.  img_hr [h][w][3], img_lr [h/2][w/2][3] fp32. */
int surs_train_images(const SursTrainImagePlan *plan, const void *tables, const unsigned char *rgb, const unsigned char *mask,
                      void *workspace, size_t workspace_bytes, float *img_hr, float *img_lr, void *stream);
/* The stages alone, for tests and tools.  jitter: workspace of surs_train_images_workspace_bytes; in == out is allowed.  blur: tmp
 * [h][w][3], in, tmp and out distinct. */
int surs_image_resample(const SursImageResample *r, const void *tables, const unsigned char *rgb, unsigned char *out, void *stream);
int surs_image_nearest(const SursImageResample *r, const void *tables, const unsigned char *mask, unsigned char *out, void *stream);
int surs_image_jitter(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, void *workspace, size_t workspace_bytes,
                      unsigned char *out, void *stream);
int surs_image_blur(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, unsigned char *tmp, unsigned char *out,
                    void *stream);
/* The same header looped on the HOST (every pointer a host pointer, no workspace): what the kernels are held against bit for bit,
 * and what is held against Pillow. */
int surs_train_images_host(const SursTrainImagePlan *plan, const void *tables, const unsigned char *rgb, const unsigned char *mask,
                           float *img_hr, float *img_lr);
int surs_image_resample_host(const SursImageResample *r, const void *tables, const unsigned char *rgb, unsigned char *out);
int surs_image_nearest_host(const SursImageResample *r, const void *tables, const unsigned char *mask, unsigned char *out);
int surs_image_jitter_host(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, unsigned char *out);
int surs_image_blur_host(const SursTrainImagePlan *plan, const unsigned char *rgb, int w, int h, unsigned char *out);
/* RGB -> Pillow's 8-bit HSV and back on n pixels of 3 bytes, host: the exhaustive check of the hue op's two conversions */
int surs_image_hsv_host(const unsigned char *in, long long n, int inverse, unsigned char *out);

#ifdef __cplusplus
}
#endif
#endif /* SURS_H */
