"""ctypes binding of libsurs_hip.so (the C ABI of include/surs.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C csrc``.
There is no fallback: if it is missing, or a call fails, this raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
from . import settings  # noqa: E402

LIB_PATH = settings.get("SURS_LIB_PATH") or os.path.join(_HERE, "libsurs_hip.so")   # override: timing experiments only
_lib = None

F32, BF16, F16, F32_GEMM = 0, 1, 2, 3
DTYPES = {"fp32": F32, "bf16": BF16, "fp16": F16, "f16": F16, "fp32x": F32_GEMM}


class SursError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("surs error %d: %s" % (code, msg))
        self.code = code


class LevelRangeError(ValueError):
    pass


class NoSurfaceError(RuntimeError):
    pass


class NonFiniteVolumeError(FloatingPointError):
    """The occupancy volume holds NaN values (marching cubes saw them).  With `--precision fp32` that is how an activation
    beyond the f16 range of the fp32-grade column kernel surfaces; reconstruction() then repeats the sweep on the layer
    kernels (fp32's exponent range)."""


class GridOptions(C.Structure):
    """SursGridOptions of include/surs.h: per-call column kernel / operand split of surs_query_grid_opt."""
    _fields_ = [("kernel", C.c_int), ("operand_parts", C.c_int), ("reserved", C.c_int * 6)]


class Conv(C.Structure):
    """SursConv of include/surs.h."""
    _fields_ = [("w_split", C.c_void_p), ("w_packed", C.c_void_p), ("bias", C.c_void_p), ("cin", C.c_int), ("cout", C.c_int),
                ("ksize", C.c_int), ("reserved", C.c_int)]


class GroupNorm(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p)]


class BatchNorm(C.Structure):
    """SursBatchNorm of include/surs.h: BatchNorm2d in eval mode folded to y = x * scale + shift."""
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p)]


class ConvBlock(C.Structure):
    _fields_ = [("conv", Conv * 3), ("bn", GroupNorm * 3)]


class EncoderNet(C.Structure):
    """SursEncoderNet of include/surs.h (device pointers of the packed weights; the arrays behind the pointer fields are kept alive by
    encoder.NativeNet)."""
    _fields_ = [("residual", C.c_int), ("n_block", C.c_int * 3), ("num_stack", C.c_int), ("hg_depth", C.c_int), ("parts", C.c_int),
                ("flags", C.c_int),
                ("head", Conv), ("down", Conv * 3), ("tail0", Conv * 3), ("tail2", Conv * 3), ("bottleneck", Conv), ("bott2", Conv),
                ("ups2", Conv), ("ups3", Conv), ("ups4", Conv), ("last0", Conv), ("last2", Conv),
                ("body", C.POINTER(Conv)), ("conv5", Conv), ("conv2", ConvBlock), ("hg", C.POINTER(ConvBlock)),
                ("top_m", C.POINTER(ConvBlock)), ("conv_last", C.POINTER(Conv)), ("l", C.POINTER(Conv)), ("next", C.POINTER(Conv)),
                ("bn_end", C.POINTER(GroupNorm)),
                # read only with ENC_EXTENDED in flags: --norm, --scale and the folded BatchNorm coefficients per norm site
                ("norm", C.c_int), ("sr_scale", C.c_int), ("bn_conv2", C.POINTER(BatchNorm)), ("bn_hg", C.POINTER(BatchNorm)),
                ("bn_top_m", C.POINTER(BatchNorm)), ("bn_end_bn", C.POINTER(BatchNorm))]


ENC_SEPARATE_SUM, ENC_EXTENDED = 1, 2     # SursEncoderNet.flags
NORM_GROUP, NORM_BATCH = 0, 1             # SursEncoderNet.norm
SR_SCALE_MIN, SR_SCALE_MAX = 1, 4         # SursEncoderNet.sr_scale / surs_bicubic_up


class SrParam(C.Structure):
    """SursSrParam of include/surs.h: one convolution's plain fp32 weight [cout][cin][k][k] and bias [cout] on the device."""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p)]


class SrParamsStruct(C.Structure):
    """SursSrParams of include/surs.h: the super-resolution convolutions and conv5 in SursEncoderNet's order."""
    _fields_ = [("head", SrParam), ("down", SrParam * 3), ("tail0", SrParam * 3), ("tail2", SrParam * 3), ("bottleneck", SrParam),
                ("bott2", SrParam), ("ups2", SrParam), ("ups3", SrParam), ("ups4", SrParam), ("last0", SrParam), ("last2", SrParam),
                ("body", C.POINTER(SrParam)), ("conv5", SrParam)]


class HgBlockParams(C.Structure):
    """SursHgBlockParams of include/surs.h: one ConvBlock's plain fp32 conv{1,2,3}.weight and bn{1,2,3}.weight / .bias on the device."""
    _fields_ = [("weight", C.c_void_p * 3), ("gamma", C.c_void_p * 3), ("beta", C.c_void_p * 3)]


class HgTailParams(C.Structure):
    """SursHgTailParams of include/surs.h: one stack tail's plain fp32 conv_last / l / bl / al (weight, bias) and bn_end.weight / .bias
    on the device; bl and al are NULL for the last stack."""
    _fields_ = [("conv_last", SrParam), ("l", SrParam), ("bl", SrParam), ("al", SrParam), ("gamma", C.c_void_p), ("beta", C.c_void_p)]


class HgFilterParams(C.Structure):
    """SursHgFilterParams of include/surs.h: every image_filter_lr.* parameter (the arrays behind the pointers are the caller's)."""
    _fields_ = [("conv2", HgBlockParams), ("hg", C.POINTER(HgBlockParams)), ("top_m", C.POINTER(HgBlockParams)),
                ("tail", C.POINTER(HgTailParams))]


class EncoderStreams(C.Structure):
    _fields_ = [("side", C.c_void_p * 4)]


class GnStats(C.Structure):
    """SursGnStats of include/surs.h."""
    _fields_ = [("sums", C.c_void_p), ("pitch", C.c_int), ("g1", C.c_int), ("g2", C.c_int), ("slots", C.c_int * 3)]


class McCounts(C.Structure):
    _fields_ = [("n_verts", C.c_int32), ("n_faces", C.c_int32), ("vmin", C.c_float), ("vmax", C.c_float)]


class MlpShape(C.Structure):
    """SursMlpShape of include/surs.h: one SurfaceClassifier's widths and skip layers."""
    _fields_ = [("n_layers", C.c_int), ("dims", C.c_int * 9), ("res_mask", C.c_uint)]


class RepackItem(C.Structure):
    """SursRepackItem of include/surs.h: one convolution of a surs_conv_repack table (device pointers; tile_end: the inclusive prefix
    sum of surs_conv_repack_tiles over the table)."""
    _fields_ = [("w", C.c_void_p), ("cout", C.c_int), ("cin", C.c_int), ("ksize", C.c_int), ("tile_end", C.c_int),
                ("packed", C.c_void_p), ("x2", C.c_void_p), ("x3", C.c_void_p)]


class OptimItem(C.Structure):
    """SursOptimItem of include/surs.h: one parameter tensor of a surs_optim_step table (chunk_end: the inclusive prefix sum of
    surs_optim_chunks(n) over the table)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("s0", C.c_void_p), ("s1", C.c_void_p), ("s2", C.c_void_p), ("n", C.c_longlong),
                ("chunk_end", C.c_int), ("reserved", C.c_int)]


class PackItem(C.Structure):
    """SursPackItem of include/surs.h: one tensor of a surs_tensors_pack table (chunk_end as in SursOptimItem)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_longlong), ("chunk_end", C.c_int), ("reserved", C.c_int)]


class TensorRef(C.Structure):
    """SursTensorRef of include/surs.h: one tensor of a surs_tensors_nonfinite table (chunk_end as in SursOptimItem)."""
    _fields_ = [("p", C.c_void_p), ("n", C.c_longlong), ("chunk_end", C.c_int), ("reserved", C.c_int)]


class OptimHyper(C.Structure):
    """SursOptimHyper of include/surs.h: one step's hyper-parameters, kernel arguments."""
    _fields_ = [("kind", C.c_int), ("first_step", C.c_int)] + [(k, C.c_float) for k in (
        "lr", "weight_decay", "momentum", "beta1_c", "beta2", "beta2_c", "alpha", "alpha_c", "eps", "step_size", "bc2_sqrt")]


class ImageResample(C.Structure):
    """SursImageResample of include/surs.h: one resample's source, index maps, target, window and table offsets."""
    _fields_ = [(k, C.c_int) for k in ("src_w", "src_h", "pad", "flip", "full_w", "full_h", "x0", "y0", "out_w", "out_h", "filter",
                                       "ksize_x", "ksize_y", "off_xb", "off_xk", "off_xn", "off_xt", "off_yb", "off_yk", "off_yn",
                                       "off_yt", "reserved")]


class TrainImagePlan(C.Structure):
    """SursTrainImagePlan of include/surs.h: one view's drawn parameters, a kernel argument."""
    _fields_ = [("augment", C.c_int), ("w", C.c_int), ("h", C.c_int), ("geo", ImageResample), ("lr", ImageResample), ("n_ops", C.c_int),
                ("op_kind", C.c_int * 4), ("op_factor", C.c_float * 4), ("hue_shift", C.c_int), ("blur_radius", C.c_int),
                ("blur_ww", C.c_uint), ("blur_fw", C.c_uint), ("tables_bytes", C.c_ulonglong)]


OPTIM_SGD, OPTIM_ADAM, OPTIM_AMSGRAD, OPTIM_RMSPROP = 0, 1, 2, 3     # SURS_OPTIM_* of include/surs.h
FILTER_NEAREST, FILTER_BILINEAR, FILTER_BICUBIC = 0, 2, 3            # SURS_FILTER_* of include/surs.h (Pillow's numbers)
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3     # SURS_JITTER_*
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_rsp, _tip = C.POINTER(ImageResample), C.POINTER(TrainImagePlan)
_shp = C.POINTER(MlpShape)
_SIGS = {
    "surs_abi_version": (C.c_int, []),
    "surs_last_error": (C.c_char_p, []),
    "surs_device_info": (C.c_int, [C.POINTER(C.c_int), C.c_char_p]),
    "surs_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "surs_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "surs_option_name": (C.c_char_p, [C.c_int]),
    "surs_option_help": (C.c_char_p, [C.c_int]),
    "surs_conv2d_nhwc": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp, _i, _vp]),
    "surs_conv_pack_weights": (_sz, [_vp, _i, _i, _i, _vp]),
    "surs_groupnorm_coeffs": (C.c_int, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "surs_groupnorm_coeffs_ws": (C.c_int, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "surs_groupnorm_scratch_bytes": (_sz, []),
    "surs_scale_shift_act": (C.c_int, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "surs_avgpool2": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "surs_bicubic_up2": (C.c_int, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "surs_bicubic_up": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "surs_bicubic_up2_block": (C.c_int, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "surs_conv2d_nhwc_sum": (C.c_int, [_i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp]),
    "surs_stats_calls": (C.c_longlong, []),
    "surs_encoder_workspace_bytes_enlarged": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_pixel_shuffle2": (C.c_int, [_vp, _i, _i, _i, _i, _f, _vp, _i, _vp]),
    "surs_add3": (C.c_int, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _vp]),
    "surs_image_prepare": (C.c_int, [_vp, _vp, _i, _i, _vp, _i, _vp]),
    "surs_nchw_to_nhwc": (C.c_int, [_vp, _i, _i, _i, _vp, _i, _vp]),
    "surs_nhwc_to_nchw": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "surs_conv2d_nhwc_x3": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp, _i, _vp]),
    "surs_conv_pack_weights_x3": (_sz, [_vp, _i, _i, _i, _vp]),
    "surs_conv2d_nhwc_x2": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp, _i, _vp]),
    "surs_conv_pack_weights_x2": (_sz, [_vp, _i, _i, _i, _vp]),
    "surs_conv_tile_scale": (C.c_int, [_i, _i]),
    "surs_conv2d_nhwc_x1": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _f, _vp, _i, _vp]),
    "surs_conv2d_nhwc_gn": (C.c_int, [_i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _f, _i, _f, _vp, _i,
                                      _vp, _i, C.POINTER(C.c_int), _vp]),
    "surs_avgpool2_gn": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _i, C.POINTER(C.c_int), _vp]),
    "surs_bicubic_up2_gn": (C.c_int, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, C.POINTER(C.c_int), _vp]),
    "surs_add3_gn": (C.c_int, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _i, _vp, _i, C.POINTER(C.c_int), _vp]),
    "surs_conv2d_nhwc_gn_sum": (C.c_int, [_i, _vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(GnStats), _vp, _vp, _vp, _vp, _f, _vp, _i, _i,
                                          C.POINTER(GnStats), _vp, _i, _vp, _i, _vp, _i, _i, _i, C.POINTER(C.c_int), _vp]),
    "surs_encoder_workspace_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_super_res": (C.c_int, [C.POINTER(EncoderNet), _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "surs_encoder_filter_lr": (C.c_int, [C.POINTER(EncoderNet), _vp, _i, _i, _i, C.POINTER(_vp), _vp, _sz, C.POINTER(EncoderStreams), _vp]),
    "surs_encoder_filter_hr": (C.c_int, [C.POINTER(EncoderNet), _vp, _i, _i, _i, _vp, _vp]),
    "surs_encoder_forward": (C.c_int, [C.POINTER(EncoderNet), _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(EncoderStreams), _vp]),
    "surs_conv_grad_weight_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "surs_conv_grad_weight": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "surs_conv_grad_input": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _i, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "surs_pixel_unshuffle2_grad": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _i, _vp]),
    "surs_encoder_sr_tape_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_sr_backward_workspace_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_super_res_train": (C.c_int, [C.POINTER(EncoderNet), _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "surs_encoder_super_res_backward": (C.c_int, [C.POINTER(EncoderNet), C.POINTER(SrParamsStruct), _vp, _i, _i, _vp, _vp, _vp,
                                                  C.POINTER(SrParamsStruct), _i, _vp, _sz, _vp]),
    "surs_groupnorm_fold": (C.c_int, [C.POINTER(GnStats), _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "surs_groupnorm_relu_grad_workspace_bytes": (_sz, [_i, _i]),
    "surs_groupnorm_relu_grad": (C.c_int, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "surs_avgpool2_grad": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "surs_bicubic_up2_grad": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "surs_encoder_convblock_tape_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_convblock_backward_workspace_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_hourglass_tape_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_hourglass_backward_workspace_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_convblock_train": (C.c_int, [C.POINTER(EncoderNet), C.POINTER(ConvBlock), _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "surs_encoder_hourglass_train": (C.c_int, [C.POINTER(EncoderNet), _i, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "surs_encoder_convblock_backward": (C.c_int, [C.POINTER(EncoderNet), C.POINTER(ConvBlock), C.POINTER(HgBlockParams), _vp, _i, _i, _vp,
                                                  _vp, C.POINTER(HgBlockParams), _i, _vp, _sz, _vp]),
    "surs_encoder_hourglass_backward": (C.c_int, [C.POINTER(EncoderNet), _i, C.POINTER(HgBlockParams), _vp, _i, _i, _vp, _vp,
                                                  C.POINTER(HgBlockParams), _i, _vp, _sz, _vp]),
    "surs_tail_joint_grad": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp]),
    "surs_encoder_tail_tape_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_tail_backward_workspace_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_filter_lr_tape_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_filter_lr_backward_workspace_bytes": (_sz, [C.POINTER(EncoderNet), _i, _i]),
    "surs_encoder_tail_train": (C.c_int, [C.POINTER(EncoderNet), _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "surs_encoder_tail_backward": (C.c_int, [C.POINTER(EncoderNet), _i, C.POINTER(HgTailParams), _vp, _i, _i, _vp, _vp, _vp,
                                             C.POINTER(HgTailParams), _i, _vp, _sz, _vp]),
    "surs_encoder_filter_lr_train": (C.c_int, [C.POINTER(EncoderNet), _vp, _i, _i, _i, C.POINTER(_vp), _vp, _sz, _vp]),
    "surs_encoder_filter_lr_backward": (C.c_int, [C.POINTER(EncoderNet), C.POINTER(HgFilterParams), _vp, _i, _i, C.POINTER(_vp), _vp,
                                                  C.POINTER(HgFilterParams), _i, _vp, _sz, _vp]),
    "surs_mlp_pack": (_sz, [_vp, _vp, _vp, _vp, _i, _vp]),
    "surs_mlp_pack_generic": (_sz, [_shp, _vp, _vp, _shp, _vp, _vp, _vp]),
    "surs_mlp_generic_info": (C.c_int, [_shp, _shp, C.POINTER(C.c_int), C.POINTER(C.c_int), _vp]),
    "surs_query_points_generic": (C.c_int, [_vp, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp]),
    "surs_query_grid_generic": (C.c_int, [_i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp, _vp, _vp]),
    "surs_mlp_generic_views_info": (C.c_int, [_shp, _shp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "surs_query_points_generic_views": (C.c_int, [_vp, _i, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp]),
    "surs_query_grid_generic_views": (C.c_int, [_i, _i, _i, _i, _vp, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp,
                                                _vp, _vp]),
    "surs_query_points_generic_stacks": (C.c_int, [_vp, _i, _vp, _f, _f, _i, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp, _vp, _vp,
                                                   _vp, _vp, _vp]),
    "surs_query_points_stacks": (C.c_int, [_vp, _i, _vp, _f, _f, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                           _vp]),
    "surs_forward_losses_workspace_bytes": (_sz, []),
    "surs_forward_losses": (C.c_int, [_vp, _vp, _i, C.c_longlong, _vp, _vp, _vp, _vp, C.c_longlong, _vp, _vp, _sz, _vp, _vp, _vp]),
    "surs_mlp_grad_workspace_bytes": (_sz, [_shp, _shp]),
    "surs_mlp_grad": (C.c_int, [_vp, _vp, _i, _vp, _vp, _f, _f, _i, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "surs_mlp_grad_features_workspace_bytes": (_sz, [_shp, _shp]),
    "surs_mlp_grad_features": (C.c_int, [_vp, _vp, _i, _vp, _vp, _f, _f, _i, _vp, _i, _i, _vp, _i, _i, _shp, _shp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, C.c_longlong, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "surs_set_operand_split": (C.c_int, [_i]),
    "surs_set_operand_split_local": (C.c_int, [_i]),
    "surs_set_grid_kernel": (C.c_int, [_i]),
    "surs_query_workspace_bytes": (_sz, [_i]),
    "surs_query_points": (C.c_int, [_vp, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "surs_query_points_columns": (C.c_int, [_vp, C.c_longlong, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _sz, _vp, _vp,
                                            C.POINTER(C.c_int), _vp]),
    "surs_query_points_columns_workspace_bytes": (_sz, []),
    "surs_nonfinite": (C.c_int, [_vp, _vp, C.c_longlong, _vp, _vp]),
    "surs_point_runs": (C.c_int, [_vp, C.c_longlong, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "surs_query_points_hr": (C.c_int, [_vp, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "surs_query_points_views": (C.c_int, [_vp, _i, _i, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp,
                                          _vp, _vp]),
    "surs_query_views_workspace_bytes": (_sz, [_i, _i]),
    "surs_query_grid_views": (C.c_int, [_i, _i, _i, _i, _vp, _i, _i, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp]),
    "surs_query_grid_views_workspace_bytes": (_sz, [_i]),
    "surs_query_grid": (C.c_int, [_i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _sz, _vp, _vp, _vp]),
    "surs_query_grid_opt": (C.c_int, [_i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _sz, _vp, _vp,
                                      C.POINTER(GridOptions), _vp]),
    "surs_query_grid_workspace_bytes": (_sz, [_i, _i, _i]),
    "surs_query_grid_probe": (C.c_int, [_i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp]),
    "surs_octree_select": (C.c_int, [_vp, _i, _i, _vp, _i, _vp, C.POINTER(C.c_int), _vp]),
    "surs_query_grid_indexed": (C.c_int, [_vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp]),
    "surs_octree_scatter": (C.c_int, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "surs_octree_level_columns": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _sz,
                                            C.POINTER(C.c_longlong), _vp]),
    "surs_octree_level_columns_dt": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _sz,
                                               C.POINTER(C.c_longlong), _vp]),
    "surs_octree_columns_workspace_bytes": (_sz, [_i]),
    "surs_octree_workspace_bytes": (_sz, [_i, _i]),
    "surs_octree_cells": (C.c_int, [_vp, _vp, _vp, _i, _i, C.c_double, _vp, _sz, _vp]),
    "surs_f64_to_f32": (C.c_int, [_vp, _vp, C.c_longlong, _vp]),
    "surs_save_obj_mesh": (C.c_int, [C.c_char_p, _vp, C.c_longlong, _vp, C.c_longlong, _i]),
    "surs_profile_enable": (C.c_int, [_i]),
    "surs_profile_read": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "surs_profile_read_ksteps": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "surs_mc_workspace_bytes": (_sz, [_i, _i, _i]),
    "surs_transform_points": (C.c_int, [_vp, _i, _vp, _vp, _vp]),
    "surs_mc_lewiner_range": (C.c_int, [_vp, _i, _i, _i, _i, _i, C.c_double, _vp, _sz, _vp, _vp, _vp, _i, _vp, _i,
                                        C.POINTER(McCounts), _vp]),
    "surs_mc_normalize": (C.c_int, [_vp, _i, _vp]),
    "surs_mc_lewiner_range_slab": (C.c_int, [_vp, _i, _i, _i, _i, _i, C.c_double, _vp, _sz, _vp, _i, _vp, _i, C.POINTER(McCounts), _i, _vp]),
    "surs_mc_slab_top_ids": (C.c_int, [_vp, _sz, _i, _i, _i, _vp, _vp]),
    "surs_mc_slab_fixup": (C.c_int, [_vp, C.c_longlong, _i, _vp, _i, _vp]),
    "surs_mc_lewiner": (C.c_int, [_vp, _i, _i, _i, C.c_double, _vp, _sz, _vp, _vp, _vp, _i, _vp, _i, C.POINTER(McCounts), _vp]),
    "surs_mesh_contains_parts": (C.c_int, [_i]),
    "surs_mesh_contains_workspace_bytes": (_sz, [_i, _i]),
    "surs_mesh_contains": (C.c_int, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp, _vp]),
    "surs_mesh_area_cdf": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp]),
    "surs_mesh_sample_pool": (C.c_int, [_vp, _i, _vp, _i, _vp, C.c_ulonglong, _i, _i, _f, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        _vp, _vp, _vp, _vp]),
    "surs_sample_select": (C.c_int, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "surs_mesh_distance_workspace_bytes": (_sz, [_i, _i]),
    "surs_mesh_distance": (C.c_int, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp, _vp]),
    "surs_mesh_distance_host": (C.c_int, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "surs_mesh_raster_parts": (C.c_int, [_i]),
    "surs_mesh_raster_workspace_bytes": (_sz, [_i, _i, _i]),
    "surs_mesh_raster": (C.c_int, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    "surs_mesh_shade_normals": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "surs_mesh_raster_host": (C.c_int, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "surs_mesh_shade_normals_host": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "surs_mesh_prt_workspace_bytes": (_sz, [_i, _i]),
    "surs_mesh_prt": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _sz, _vp]),
    "surs_mesh_prt_counted": (C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _i, _f, _vp, _vp, _sz, _vp, _vp]),
    "surs_mesh_prt_host":(C.c_int, [_vp, _i, _vp, _i, _vp, _vp, _i, _f, _vp, _vp]),
    "surs_texture_pyramid_floats": (_sz, [_i, _i]),
    "surs_texture_pyramid": (C.c_int, [_vp, _i, _i, _vp, _vp]),
    "surs_texture_pyramid_host": (C.c_int, [_vp, _i, _i, _vp]),
    "surs_mesh_shade_prt": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "surs_mesh_shade_prt_host": (C.c_int, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp,
                                           _vp]),
    "surs_image_resolve": (C.c_int, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "surs_image_resolve_host": (C.c_int, [_vp, _i, _i, _i, _vp, _vp]),
    "surs_conv_repack_tiles": (C.c_int, [_i, _i, _i]),
    "surs_conv_repack": (C.c_int, [_vp, _i, _vp]),
    "surs_conv1x1_merge": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "surs_mlp_repack": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "surs_mlp_repack_generic": (C.c_int, [_shp, _vp, _vp, _shp, _vp, _vp, _vp, _vp]),
    "surs_mlp_repack_host": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp]),
    "surs_mlp_repack_generic_host": (C.c_int, [_shp, _vp, _vp, _shp, _vp, _vp, _vp]),
    "surs_optim_chunks": (C.c_int, [C.c_longlong]),
    "surs_optim_check": (C.c_int, [_vp, _i, C.POINTER(OptimHyper)]),
    "surs_optim_step": (C.c_int, [_vp, _i, C.POINTER(OptimHyper), _vp]),
    "surs_optim_step_host": (C.c_int, [_vp, _i, C.POINTER(OptimHyper)]),
    "surs_optim_step_ranks": (C.c_int, [_vp, _i, C.POINTER(OptimHyper), _i, C.c_longlong, _f, _vp]),
    "surs_optim_step_ranks_host": (C.c_int, [_vp, _i, C.POINTER(OptimHyper), _i, C.c_longlong, _f]),
    "surs_tensors_pack_check": (C.c_int, [_vp, _i]),
    "surs_tensors_pack": (C.c_int, [_vp, _i, _vp]),
    "surs_tensors_pack_host": (C.c_int, [_vp, _i]),
    "surs_forward_losses_grad_workspace_bytes": (_sz, []),
    "surs_forward_losses_grad": (C.c_int, [_vp, _vp, _i, C.c_longlong, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp,
                                           _vp]),
    "surs_forward_losses_grad_host": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "surs_tensors_nonfinite_check": (C.c_int, [_vp, _i, C.POINTER(C.c_longlong)]),
    "surs_tensors_nonfinite_workspace_bytes": (_sz, [C.c_longlong]),
    "surs_tensors_nonfinite": (C.c_int, [_vp, _i, C.c_longlong, _vp, _sz, _vp, _vp]),
    "surs_tensors_nonfinite_host": (C.c_int, [_vp, _i, C.POINTER(C.c_int)]),
    "surs_image_resample_plan": (C.c_int, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _rsp, _vp, _sz, _sz, C.POINTER(_sz)]),
    "surs_train_image_plan": (C.c_int, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_double), _i,
                                        C.c_double, _tip, _vp, _sz]),
    "surs_train_images_workspace_bytes": (_sz, [_tip]),
    "surs_train_images": (C.c_int, [_tip, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "surs_image_resample": (C.c_int, [_rsp, _vp, _vp, _vp, _vp]),
    "surs_image_nearest": (C.c_int, [_rsp, _vp, _vp, _vp, _vp]),
    "surs_image_jitter": (C.c_int, [_tip, _vp, _i, _i, _vp, _sz, _vp, _vp]),
    "surs_image_blur": (C.c_int, [_tip, _vp, _i, _i, _vp, _vp, _vp]),
    "surs_train_images_host": (C.c_int, [_tip, _vp, _vp, _vp, _vp, _vp]),
    "surs_image_resample_host": (C.c_int, [_rsp, _vp, _vp, _vp]),
    "surs_image_nearest_host": (C.c_int, [_rsp, _vp, _vp, _vp]),
    "surs_image_jitter_host": (C.c_int, [_tip, _vp, _i, _i, _vp]),
    "surs_image_blur_host": (C.c_int, [_tip, _vp, _i, _i, _vp]),
    "surs_image_hsv_host": (C.c_int, [_vp, C.c_longlong, _i, _vp]),
}
MESH_FACES_PER_PART, SAMPLE_SELECT_CHUNK = 4096, 1024     # SURS_MESH_FACES_PER_PART, SURS_SAMPLE_SELECT_CHUNK of include/surs.h
MESH_PRT_CHUNK = 512     # SURS_MESH_PRT_CHUNK of include/surs.h
EXPORTS = sorted(_SIGS)


def lib():
    """The loaded library.  Raises if it has not been built (never falls back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libsurs_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or make -C %s/csrc)" % _HERE)
        # PyTorch first: its wheel carries its own HIP runtime (libamdhip64), and the library must bind to THAT copy - loaded
        # before torch, it would pull in /opt/rocm's, torch would then run on a second runtime in the same process, and the first
        # kernel launch fails with "no ROCm-capable device is detected" (seen with build() and smoke() in one process)
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)  # AttributeError if the library misses a declared entry point
            fn.restype = res
            fn.argtypes = args
        if l.surs_abi_version() != 1:
            raise ImportError("libsurs_hip.so has ABI version %d, expected 1" % l.surs_abi_version())
        _lib = l
    return _lib


def check(code):
    if code == 0:
        return
    msg = lib().surs_last_error().decode("utf-8", "replace")
    if code == -4:
        raise LevelRangeError("Surface level must be within volume data range.")
    if code == -5:
        raise NoSurfaceError("No surface found at the given iso value.")
    if code == -7:
        raise NonFiniteVolumeError("the occupancy volume contains NaN values")
    raise SursError(code, msg)
