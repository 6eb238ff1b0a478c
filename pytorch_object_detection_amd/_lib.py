"""ctypes binding of libfcosdet_hip.so (include/fcosdet.h).  Loading fails loudly; there is no fallback."""
from __future__ import annotations

import ctypes as C
import os

FD_MAX_SEG = 8
ACT_NONE, ACT_RELU, ACT_SILU, ACT_EXP, ACT_SIGMOID = 0, 1, 2, 3, 4
CONV_GENERIC, CONV_STEM = 0, 1
PREC_F32, PREC_F16X3, PREC_F16 = 0, 1, 2     # include/fcosdet.h FD_PREC_*
# include/fcosdet.h FD_TILE_*: the block tiles of the direct implicit-GEMM kernel (what autotune_conv chooses among) ...
TILES = {1: (128, 128), 2: (128, 64), 3: (64, 128), 4: (64, 64), 5: (128, 32), 6: (128, 96),
         7: (128, 128), 8: (128, 64), 9: (64, 128),   # 7-9: single-LDS-buffer variants
         10: (256, 128), 11: (256, 128),             # 8-wave tile (11: single LDS buffer)
         12: (128, 96),                              # 128x96, single LDS buffer
         13: (128, 128),                             # 128x128 with the 3x3 input patch staged in LDS (3x3 stride-1 'same' only)
         15: (64, 64)}                               # wave-autonomous 64x64 tiles, one wave per workgroup (1x1 stride-1 layers, needs w_frag)
# the tiles of TILES the FD_PREC_F16 instantiation of the direct kernel is built for: MUST follow `using F16 = Variant<...>` in csrc/fd_conv.hip (any other id of
# TILES is FD_E_UNSUPPORTED under FD_PREC_F16; FD_PREC_F32 and FD_PREC_F16X3 have them all)
F16_TILES = frozenset({1, 2, 3, 4, 5, 6, 7})
PATCH_TILE = 13
WAVE_TILE = 15
# ... and the kernels a tile id names, each with its own weight format (ops.WFormat); not members of TILES
WINO_TILE = 14      # Winograd F(2x2, 3x3) kernel (ops.pack_conv_weight_wino)
WINO4_TILE = 16     # Winograd F(4x4, 3x3) kernel (ops.pack_conv_weight_wino4)
NARROW_TILE = 17    # 3x3 stride-1 pad-1 convs with Cout <= 8 on the vector unit (fd_conv_narrow.hip; ops.pack_conv_weight_narrow)
F16K64_TILE = 18    # FD_PREC_F16 on K-tiles of 64 channels (fd_conv_f16.hip; ops.pack_conv_weight_f16k64)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FD_LIB: another build of the SAME library (development A/B runs: tools/gpu_ab.sh keeps its variants outside the package and never overwrites the product
# library).  It must export every entry point below -- there is still no fallback of any kind.
LIB_PATH = os.environ.get("FD_LIB") or os.path.join(_HERE, "csrc", "libfcosdet_hip.so")


class FdError(RuntimeError):
    """Error of the HIP path.  `rc` is the library's numeric return code (FD_E_INVAL -1, FD_E_UNSUPPORTED -2, FD_E_LAUNCH -3) when the
    error came out of a C-ABI call, else None (host-side contract violations)."""

    def __init__(self, msg: str = "", rc=None):
        super().__init__(msg)
        self.rc = rc


E_INVAL, E_UNSUPPORTED, E_LAUNCH = -1, -2, -3


class Segs(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("batch", C.c_int32), ("H", C.c_int32 * FD_MAX_SEG), ("W", C.c_int32 * FD_MAX_SEG),
                ("m_start", C.c_int32 * (FD_MAX_SEG + 1))]

    @staticmethod
    def make(batch: int, hw) -> "Segs":
        s = Segs()
        s.nseg, s.batch = len(hw), batch
        m = 0
        for i, (h, w) in enumerate(hw):
            s.H[i], s.W[i], s.m_start[i] = h, w, m
            m += batch * h * w
        for i in range(len(hw), FD_MAX_SEG + 1):
            s.m_start[i] = m
        return s

    @property
    def rows(self) -> int:
        return self.m_start[self.nseg]

    def level_hw(self):
        return [(self.H[i], self.W[i]) for i in range(self.nseg)]


class B2BParams(C.Structure):
    """fd_b2b_params (include/fcosdet.h): two 1x1 convs back to back in one launch."""
    _fields_ = [("x", C.c_void_p), ("w1_frag", C.c_void_p), ("scale1", C.c_void_p), ("shift1", C.c_void_p), ("res", C.c_void_p), ("y", C.c_void_p),
                ("w2_frag", C.c_void_p), ("scale2", C.c_void_p), ("shift2", C.c_void_p), ("z", C.c_void_p),
                ("x_cs", C.c_int32), ("x_co", C.c_int32), ("res_cs", C.c_int32), ("res_co", C.c_int32), ("y_cs", C.c_int32), ("y_co", C.c_int32),
                ("z_cs", C.c_int32), ("z_co", C.c_int32),
                ("K1", C.c_int32), ("N1", C.c_int32), ("N2", C.c_int32), ("act1", C.c_int32), ("act2", C.c_int32), ("reserved0", C.c_int32),
                ("rows", C.c_int64)]


class ConvParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("res", C.c_void_p),
                ("y", C.c_void_p),
                ("x_cs", C.c_int32), ("x_co", C.c_int32), ("res_cs", C.c_int32), ("res_co", C.c_int32),
                ("y_cs", C.c_int32), ("y_co", C.c_int32),
                ("Cin", C.c_int32), ("Cout", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("dil", C.c_int32),
                ("act", C.c_int32), ("act_c0", C.c_int32), ("mode", C.c_int32), ("tile", C.c_int32), ("tag", C.c_int32), ("ksplit", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("precision", C.c_int32), ("res_mode", C.c_int32),
                ("seg_param", C.c_float * FD_MAX_SEG), ("segs", Segs),
                ("out_H", C.c_int32), ("out_W", C.c_int32), ("sc_sy", C.c_int32), ("sc_sx", C.c_int32), ("sc_oy", C.c_int32),
                ("sc_ox", C.c_int32), ("sc_H", C.c_int32), ("sc_W", C.c_int32),
                ("gate", C.c_void_p), ("gate_cs", C.c_int32), ("reserved0", C.c_int32), ("w_frag", C.c_void_p),
                ("gn_stats", C.c_void_p), ("gn_groups", C.c_int32), ("gate_act", C.c_int32), ("gate_b", C.c_void_p),
                ("x2", C.c_void_p), ("x2_cs", C.c_int32), ("x2_co", C.c_int32), ("x2_Cin", C.c_int32), ("x2_stride", C.c_int32), ("x2_H", C.c_int32),
                ("x2_W", C.c_int32), ("wg_first", C.c_int32), ("wg_count", C.c_int32), ("sk_wgs", C.c_int32), ("io_f16", C.c_int32)]


class PackJob(C.Structure):
    _fields_ = [("w", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p), ("Cout", C.c_int32), ("Cin", C.c_int32),
                ("KH", C.c_int32), ("KW", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32)]


class WgradParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p),
                ("x_cs", C.c_int32), ("x_co", C.c_int32), ("dy_cs", C.c_int32), ("dy_co", C.c_int32),
                ("Cin", C.c_int32), ("Cout", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("dil", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("nsplit", C.c_int32), ("layout", C.c_int32),
                ("scale", C.c_void_p), ("segs", Segs), ("precision", C.c_int32), ("io_f16", C.c_int32)]


class AnchorParams(C.Structure):
    """fd_anchor_params (include/fcosdet.h): the anchor set of one input size, filled by the host (utill.utills.DataEncoder)."""
    _fields_ = [("fm_w", C.c_int32 * 5), ("fm_h", C.c_int32 * 5), ("grid_w", C.c_float * 5), ("grid_h", C.c_float * 5),
                ("wh", C.c_float * 2 * 9 * 5), ("num_anchors", C.c_int32)]


ANCHOR_MAX_GT, ANCHOR_MAX_CLASSES, ANCHOR_MAX_CAND = 256, 128, 1024     # include/fcosdet.h FD_ANCHOR_MAX_*

OPTIM_MAX_TENSORS, OPTIM_MAX_GROUPS, OPTIM_MAX_DROPS = 64, 8, 4           # include/fcosdet.h FD_OPTIM_MAX_*
OPTIM_LR_NONE, OPTIM_LR_TRAIN_PY, OPTIM_LR_TRAIN_NEW = 0, 1, 2            # FD_OPTIM_LR_*


class OptimState(C.Structure):
    """fd_optim_state: the optimizer's device block.  Never instantiated on the host: optim.py allocates sizeof() bytes on the device and views the fields."""
    _fields_ = [("global_step", C.c_int64), ("skip", C.c_int64), ("lr", C.c_double * OPTIM_MAX_GROUPS), ("applied", C.c_int64 * OPTIM_MAX_GROUPS),
                ("bc1", C.c_double * OPTIM_MAX_GROUPS), ("bc2", C.c_double * OPTIM_MAX_GROUPS)]


class OptimChunk(C.Structure):
    """fd_optim_chunk: up to OPTIM_MAX_TENSORS tensors of one update launch, passed to the kernel by value."""
    _fields_ = [("n", C.c_int32), ("reserved0", C.c_int32), ("p", C.c_void_p * OPTIM_MAX_TENSORS), ("g", C.c_void_p * OPTIM_MAX_TENSORS),
                ("s0", C.c_void_p * OPTIM_MAX_TENSORS), ("s1", C.c_void_p * OPTIM_MAX_TENSORS), ("numel", C.c_int64 * OPTIM_MAX_TENSORS)]


class OptimHyper(C.Structure):
    _fields_ = [("group", C.c_int32), ("nesterov", C.c_int32), ("decoupled_wd", C.c_int32), ("reserved0", C.c_int32),
                ("momentum", C.c_double), ("weight_decay", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class OptimBeginParams(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("adam", C.c_int32), ("rule", C.c_int32), ("n_drops", C.c_int32),
                ("lr_init", C.c_double), ("warmup_factor", C.c_double), ("gamma", C.c_double), ("warmup_steps", C.c_int64),
                ("drop_step", C.c_int64 * OPTIM_MAX_DROPS), ("drop_factor", C.c_double * OPTIM_MAX_DROPS),
                ("lr_value", C.c_double * OPTIM_MAX_GROUPS), ("lr_ptr", C.c_void_p * OPTIM_MAX_GROUPS), ("lr_ptr_f64", C.c_int32 * OPTIM_MAX_GROUPS),
                ("active", C.c_int32 * OPTIM_MAX_GROUPS), ("beta1", C.c_double * OPTIM_MAX_GROUPS), ("beta2", C.c_double * OPTIM_MAX_GROUPS)]


class GradChunk(C.Structure):
    """fd_grad_chunk: the gradients of one sum-of-squares launch, passed to the kernel by value."""
    _fields_ = [("n", C.c_int32), ("reserved0", C.c_int32), ("g", C.c_void_p * OPTIM_MAX_TENSORS), ("numel", C.c_int64 * OPTIM_MAX_TENSORS)]


class GradClip(C.Structure):
    """fd_grad_clip: the clip block on the device, written by fd_grad_clip_finish.  Never instantiated on the host: optim.py views the fields."""
    _fields_ = [("sumsq", C.c_double), ("total_norm", C.c_double), ("clip_coef", C.c_double), ("eff_scale", C.c_float), ("found", C.c_float),
                ("total_norm_f32", C.c_float), ("reserved0", C.c_float)]


AVG_SWA, AVG_EMA = 0, 1                                                   # include/fcosdet.h FD_AVG_*


class AvgState(C.Structure):
    """fd_avg_state: the averager's device block, written by fd_avg_begin.  Never instantiated on the host: optim.py allocates sizeof() bytes on the device."""
    _fields_ = [("apply", C.c_int64), ("weight", C.c_double), ("weight_f32", C.c_float), ("reserved0", C.c_float), ("reserved1", C.c_int64)]


class AvgBeginParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("reserved0", C.c_int32), ("decay", C.c_double), ("start_step", C.c_int64), ("every", C.c_int64)]


class AvgChunk(C.Structure):
    """fd_avg_chunk: up to OPTIM_MAX_TENSORS (averaged copy, model tensor) pairs of one update launch, passed to the kernel by value."""
    _fields_ = [("n", C.c_int32), ("reserved0", C.c_int32), ("avg", C.c_void_p * OPTIM_MAX_TENSORS), ("p", C.c_void_p * OPTIM_MAX_TENSORS),
                ("numel", C.c_int64 * OPTIM_MAX_TENSORS)]


class AvgCopyChunk(C.Structure):
    """fd_avg_copy_chunk: the buffers of one copy launch, passed to the kernel by value."""
    _fields_ = [("n", C.c_int32), ("reserved0", C.c_int32), ("dst", C.c_void_p * OPTIM_MAX_TENSORS), ("src", C.c_void_p * OPTIM_MAX_TENSORS),
                ("nbytes", C.c_int64 * OPTIM_MAX_TENSORS)]


JPEG_MAX_COMP = 3                                                         # include/fcosdet.h FD_JPEG_*
JPEG_R_NONE, JPEG_R_PROGRESSIVE, JPEG_R_ARITHMETIC, JPEG_R_PRECISION, JPEG_R_COMPONENTS, JPEG_R_RGB, JPEG_R_SAMPLING, JPEG_R_MULTISCAN, JPEG_R_DNL = range(9)
JPEG_REASONS = {JPEG_R_NONE: "supported", JPEG_R_PROGRESSIVE: "progressive (or another non-baseline) frame", JPEG_R_ARITHMETIC: "arithmetic coding",
                JPEG_R_PRECISION: "12-bit samples or 16-bit quantisation tables", JPEG_R_COMPONENTS: "a component count other than 1 or 3",
                JPEG_R_RGB: "an RGB stream (Adobe transform 0 or 'R','G','B' component ids)", JPEG_R_SAMPLING: "a sampling other than 4:4:4, 4:2:2, 4:2:0",
                JPEG_R_MULTISCAN: "several scans", JPEG_R_DNL: "height 0 (DNL)"}
JPEG_E_TRUNCATED, JPEG_E_MARKER, JPEG_E_HUFFMAN, JPEG_E_COEF_INDEX, JPEG_E_TABLE, JPEG_E_BUFFER, JPEG_E_UNSUPPORTED = -16, -17, -18, -19, -20, -21, -22
JPEG_ERRORS = {JPEG_E_TRUNCATED: "truncated stream", JPEG_E_MARKER: "malformed marker segment or restart marker", JPEG_E_HUFFMAN: "bits that match no Huffman code",
               JPEG_E_COEF_INDEX: "coefficient index past 63", JPEG_E_TABLE: "the scan names a table nothing defines", JPEG_E_BUFFER: "coefficient buffer too small",
               JPEG_E_UNSUPPORTED: "unsupported stream"}


class JpegInfo(C.Structure):
    """fd_jpeg_info: what fd_jpeg_parse reads from the headers of one stream."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("supported", C.c_int32), ("reason", C.c_int32),
                ("restart_interval", C.c_int32), ("h_samp", C.c_int32 * JPEG_MAX_COMP), ("v_samp", C.c_int32 * JPEG_MAX_COMP),
                ("h_max", C.c_int32), ("v_max", C.c_int32), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32),
                ("bw", C.c_int32 * JPEG_MAX_COMP), ("bh", C.c_int32 * JPEG_MAX_COMP), ("dc_tab", C.c_int32 * JPEG_MAX_COMP), ("ac_tab", C.c_int32 * JPEG_MAX_COMP),
                ("reserved0", C.c_int32 * 2), ("scan_offset", C.c_int64), ("coef_bytes", C.c_int64), ("qt", C.c_uint16 * 64 * JPEG_MAX_COMP),
                ("huff_defined", C.c_uint8 * 4 * 2), ("huff_bits", C.c_uint8 * 16 * 4 * 2), ("huff_vals", C.c_uint8 * 256 * 4 * 2)]


class JpegIdctJob(C.Structure):
    """fd_jpeg_idct_job: one image component of the IDCT launch."""
    _fields_ = [("coef_off", C.c_int64), ("plane_off", C.c_int64), ("bw", C.c_int32), ("bh", C.c_int32), ("qt", C.c_int32), ("reserved0", C.c_int32)]


class JpegColorJob(C.Structure):
    """fd_jpeg_color_job: one image of the upsampling + colour launch."""
    _fields_ = [("out", C.c_void_p), ("plane_off", C.c_int64 * JPEG_MAX_COMP), ("stride", C.c_int32 * JPEG_MAX_COMP), ("rows", C.c_int32 * JPEG_MAX_COMP),
                ("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("h_samp", C.c_int32), ("v_samp", C.c_int32), ("reserved0", C.c_int32)]


_lib = None

_P, _I, _F, _D, _L = C.c_void_p, C.c_int32, C.c_float, C.c_double, C.c_int64
_SIGS = {
    "fd_version": (_I, []),
    "fd_last_error": (C.c_char_p, []),
    "fd_conv2d_nhwc_f32": (_I, [C.POINTER(ConvParams), _P]),
    "fd_conv_narrow_nco": (_I, [_I]),
    "fd_conv_workgroups": (_I, [C.POINTER(ConvParams)]),
    "fd_conv_workgroups_live": (_I, [C.POINTER(ConvParams)]),
    "fd_conv1x1_b2b_f32": (_I, [C.POINTER(B2BParams), _P]),
    "fd_conv_workspace_bytes": (_L, [_L, _I, _I]),
    "fd_conv_sk_workspace_bytes": (_L, [_I]),
    "fd_mbconv_pool_bytes": (_L, [_I, _I, _I, _I, _I, _I]),
    "fd_mbconv_expand_dw_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_se_gate_from_pool": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "fd_conv_wgrad_workspace_bytes": (_L, [_L, _I, _I, _I, _I]),
    "fd_pack_conv_weight_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fd_pack_conv_weights_batch_f32": (_I, [_P, _I, _L, _P]),
    "fd_wino4_weight_bytes": (_L, [_I, _I]),
    "fd_wino4_pack_weights_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "fd_conv_weight_wave_bytes": (_L, [_I, _I]),
    "fd_pack_conv_weight_wave_f32": (_I, [_P, _P, _I, _I, _P]),
    "fd_wino_weight_bytes": (_L, [_I, _I]),
    "fd_wino_pack_weights_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "fd_conv2d_bwd_weight_f32": (_I, [C.POINTER(WgradParams), _P]),
    "fd_stem7x7_nhwc4": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fd_stem7x7_pool_nhwc4": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "fd_stem7x7_nchw3": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_stem7x7_wgrad_workspace_bytes": (_L, [_I, _I, _I]),
    "fd_stem7x7_bwd_weight_nhwc4": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _L, _I, _I, _I, _P]),
    "fd_nchw3_to_nhwc4": (_I, [_P, _P, _I, _I, _I, _P]),
    "fd_nhwc_to_nchw": (_I, [_P, _I, _I, _P, _I, _I, _I, _P]),
    "fd_preprocess_u8_nhwc4": (_I, [_P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _P]),
    "fd_boxes_rescale_xywh": (_I, [_P, _L, _F, _P]),
    "fd_maxpool_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_upsample2x_add_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fd_dwconv3x3_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(Segs), _P]),
    "fd_dwconv2d_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_dwconv2d_bwd_data_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_dwconv2d_wgrad_workspace_bytes": (_L, [_I, _I, _I, _I, _I]),
    "fd_dwconv2d_bwd_weight_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P]),
    "fd_dwconv_dilated_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(Segs), _P]),
    "fd_deform_im2col_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_deform_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_stem_conv_nhwc4": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_collate_u8_nhwc4": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _P]),
    "fd_resize_u8": (_I, [_P, _I, _I, _P, _I, _I, _P]),
    "fd_resize_collate_u8_nhwc4": (_I, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _P]),
    "fd_boxes_scale_batch": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "fd_augment_resize_collate_u8": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _P]),
    "fd_mosaic_collate_u8": (_I, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _P]),
    "fd_jitter_l_sums": (_I, [_P, _P, _P, _I, _L, _P]),
    "fd_color_jitter_u8": (_I, [_P, _I, _I, _P, _P, _P]),
    "fd_rotate_u8": (_I, [_P, _I, _I, _P, C.POINTER(_I), _P]),
    "fd_dwconv_dilated_wgrad_workspace_bytes": (_L, [C.POINTER(Segs), _I, _I]),
    "fd_dwconv_dilated_bwd_weight_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _P, _I, C.POINTER(Segs), _P, _P]),
    "fd_dwconv3x3_wgrad_workspace_bytes": (_L, [C.POINTER(Segs), _I]),
    "fd_dwconv3x3_bwd_weight_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _P, _I, C.POINTER(Segs), _P, _P]),
    "fd_groupnorm_workspace_bytes": (_L, [C.POINTER(Segs), _I]),
    "fd_groupnorm_act_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _F, _I, C.POINTER(Segs), _P, _P]),
    "fd_groupnorm_from_rowstats": (_I, [_P, _I, _I, _F, _P, _P, C.POINTER(Segs), _P, _P, _P]),
    "fd_groupnorm_apply_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _F, _I, C.POINTER(Segs), _P, _P]),
    "fd_groupnorm_stats_nhwc": (_I, [_P, _I, _I, _I, _I, _F, _P, _P, C.POINTER(Segs), _P, _P, _P]),
    "fd_coef_apply_nhwc": (_I, [_P, _I, _I, _P, _P, _I, _P, _I, _I, _I, _I, C.POINTER(Segs), _P]),
    "fd_dwconv3x3_gn_nhwc": (_I, [_P, _I, _I, _P, _P, _I, _P, _I, _I, _I, _P, _I, C.POINTER(Segs), _P]),
    "fd_groupnorm_bwd_workspace_bytes": (_L, [C.POINTER(Segs), _I]),
    "fd_groupnorm_act_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _I, _I, _F, _I, C.POINTER(Segs), _P, _P,
                                       _P]),
    "fd_se_workspace_bytes": (_L, [_I, _I, _I]),
    "fd_se_scale_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "fd_se_bwd_workspace_bytes": (_L, [_I, _I, _I]),
    "fd_se_scale_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "fd_act_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _L, _I, _I, _F, _P]),
    "fd_act_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _L, _I, _I, _F, _P]),
    "fd_act_bwd_nhwc_h": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _L, _I, _I, _F, _P]),
    "fd_maxpool_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_upsample2x_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fd_batchnorm_update_running": (_I, [_P, _L, _I, _F, _F, _P, _P, _P]),
    "fd_batchnorm_update_running_dev": (_I, [_P, _P, _I, _F, _F, _P, _P, _P]),
    "fd_batchnorm_sync_fwd_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _P, _P]),
    "fd_batchnorm_sync_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _L, _I, _F, _I, _I, _P, _D, _P, _P, _P]),
    "fd_batchnorm_train_workspace_bytes": (_L, [_L, _I]),
    "fd_batchnorm_train_fwd_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _F, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _L, _I, _F, _I, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_workspace_bytes": (_L, [_L, _I]),
    "fd_batchnorm_train_sync_fwd_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _F, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_bwd_nhwc": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _L, _I, _F, _I, _I, _P, _D, _P, _P, _L, _P]),
    "fd_batchnorm_train_res_fwd_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, _L, _I, _F, _I, _F, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_res_fwd_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _F, _P, _P, _P, _L, _P]),
    # the same six on f16 maps (x, res, y, dy, dx as _Float16): the fp32 forms' argument lists
    "fd_batchnorm_train_fwd_nhwc_h": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _F, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_bwd_nhwc_h": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _L, _I, _F, _I, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_fwd_nhwc_h": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _F, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_bwd_nhwc_h": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _L, _I, _F, _I, _I, _P, _D, _P, _P, _L, _P]),
    "fd_batchnorm_train_res_fwd_nhwc_h": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, _L, _I, _F, _I, _F, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_res_fwd_nhwc_h": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _F, _P, _P, _P, _L, _P]),
    # the cumulative-average siblings: `float momentum` replaced by the device pointer of num_batches_tracked
    "fd_batchnorm_update_running_cma": (_I, [_P, _L, _I, _P, _F, _P, _P, _P]),
    "fd_batchnorm_update_running_dev_cma": (_I, [_P, _P, _I, _P, _F, _P, _P, _P]),
    "fd_batchnorm_train_fwd_cma_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _P, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_res_fwd_cma_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, _L, _I, _F, _I, _P, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_fwd_cma_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _P, _P, _P, _P, _L, _P]),
    "fd_batchnorm_train_sync_res_fwd_cma_nhwc": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _P, _I, _I, _L, _I, _F, _I, _I, _P, _D, _P, _P, _P, _P, _L, _P]),
    "fd_sample_scale_add_nhwc": (_I, [_P, _I, _I, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "fd_stem_conv_wgrad_workspace_bytes": (_L, [_I, _I, _I, _I, _I, _I]),
    "fd_stem_conv_bwd_weight_nhwc4": (_I, [_P, _P, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fd_fcos_decode": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _I, _I, C.POINTER(Segs), C.POINTER(_I), _P, _P, _P, _P]),
    "fd_topk_workspace_bytes": (_L, [_I, _I, _I]),
    "fd_fcos_topk": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "fd_nms_workspace_bytes": (_L, [_I, _I]),
    "fd_batched_nms": (_I, [_P, _P, _P, _I, _I, _F, _D, _P, _P, _P, _P, _P, _P, _P]),
    "fd_box_nms_plus1": (_I, [_P, _P, _P, _I, _I, _F, _I, _P, _P, _P]),
    "fd_pairwise_iou": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "fd_clip_boxes": (_I, [_P, _L, _I, _I, _P]),
    "fd_pack_detections": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "fd_unpack_detections": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "fd_ltrb_iou_loss_fwd": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "fd_ltrb_iou_loss_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "fd_focal_workspace_bytes": (_L, [_I]),
    "fd_focal_loss_fwd": (_I, [_P, _P, _I, _I, _I, _F, _F, _P, _P, _P]),
    "fd_focal_loss_bwd": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _P, _P]),
    "fd_ltrb_quality": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "fd_quality_loss_workspace_bytes": (_L, [_I]),
    "fd_quality_loss_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P]),
    "fd_quality_loss_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P]),
    "fd_bce_logits_loss_fwd": (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "fd_bce_logits_loss_bwd": (_I, [_P, _P, _P, _P, _I, _I, _P, _P]),
    "fd_eval_ap_workspace_bytes": (_L, [_I, _I, _I, _I, _I]),
    "fd_eval_ap": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, C.POINTER(_F), _I, _I, _P, _P, _P, _P, _P, _P]),
    "fd_eval_coco_workspace_bytes": (_L, [_I, _I, _I, _I]),
    "fd_eval_coco": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _I, _P, _I, C.POINTER(_D), _I, C.POINTER(_D), _I, C.POINTER(_D), _I,
                          C.POINTER(_I), _I, _P, _P, _P, _P, _P]),
    "fd_fcos_gen_targets": (_I, [_P, _P, _I, C.POINTER(Segs), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _F, _P, _P, _P, _P]),
    "fd_atss_workspace_bytes": (_L, [_I, _I]),
    "fd_atss_gen_targets": (_I, [_P, _P, _I, C.POINTER(Segs), C.POINTER(_I), _I, _F, _F, _P, _P, _P, _P, _P, _P, _P]),
    "fd_simota_workspace_bytes": (_L, [_I, _I, _I]),
    "fd_simota_gen_targets": (_I, [_P, _P, _P, _I, _P, _P, _I, C.POINTER(Segs), C.POINTER(_I), _I, _F, _F, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fd_anchor_boxes": (_I, [C.POINTER(AnchorParams), _P, _I, _P]),
    "fd_anchor_encode": (_I, [C.POINTER(AnchorParams), _P, _P, _I, _I, _I, _P, _P, _P]),
    "fd_anchor_decode_workspace_bytes": (_L, [_I, _I, _I]),
    "fd_anchor_decode": (_I, [C.POINTER(AnchorParams), _P, _P, _I, _I, _I, _F, _F, _I, _P, _P, _P, _P, _P, _P, _P]),
    "fd_optim_begin": (_I, [_P, _P, C.POINTER(OptimBeginParams), _P]),
    "fd_optim_sgd_f32": (_I, [C.POINTER(OptimChunk), C.POINTER(OptimHyper), _P, _P, _P]),
    "fd_optim_adam_f32": (_I, [C.POINTER(OptimChunk), C.POINTER(OptimHyper), _P, _P, _P]),
    "fd_grad_sumsq_slots": (_I, [C.POINTER(GradChunk)]),
    "fd_grad_norm_workspace_bytes": (_L, [_I]),
    "fd_grad_sumsq_f32": (_I, [C.POINTER(GradChunk), _P, _I, _P]),
    "fd_grad_clip_finish": (_I, [_P, _I, _P, _P, _D, _P, _P]),
    "fd_avg_begin": (_I, [_P, _P, _P, _P, C.POINTER(AvgBeginParams), _P]),
    "fd_avg_update_f32": (_I, [C.POINTER(AvgChunk), _P, _P]),
    "fd_avg_copy_bytes": (_I, [C.POINTER(AvgCopyChunk), _P, _P]),
    "fd_jpeg_parse": (_I, [_P, _L, C.POINTER(JpegInfo)]),
    "fd_jpeg_entropy_decode": (_I, [_P, _L, C.POINTER(JpegInfo), _P, _L]),
    "fd_jpeg_idct_u8": (_I, [_P, _P, _I, _P, _L, _P, _I, _P, _L, _P]),
    "fd_jpeg_color_u8": (_I, [_P, _P, _I, _P, _L, _P]),
}
EXPORTS = tuple(_SIGS)


def lib() -> C.CDLL:
    """Load libfcosdet_hip.so once.  Raises FdError when it has not been built (python __graft_entry__.py / make)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FdError(f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # torch bundles its own libamdhip64: import it first so this library binds to the SAME HIP runtime
        # (two runtimes in one process => "no ROCm-capable device" / foreign stream handles)
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = lib().fd_last_error().decode(errors="replace")
        raise FdError(f"{what or 'libfcosdet_hip'} failed ({code}): {msg}", rc=int(code))
