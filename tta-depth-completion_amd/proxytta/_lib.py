"""ctypes binding of libptta_hip.so (C-ABI: include/ptta.h).

The product path has no CPU fallback: if the shared library is missing or cannot be loaded this
module raises, and every call that needs a GPU raises when no HIP device is present.
"""
import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_int64, c_uint64, c_void_p

# The binding does not touch the process environment.  The hosting process should export HIP_FORCE_DEV_KERNARG=1 before the HIP runtime
# initialises (kernel arguments in device memory; 0 costs 7 % of the replayed MSG_CHN step): bench.py does and reports it, INTEGRATION.md.

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libptta_hip.so')

PTTA_BACKBONE_MSG_CHN = 0
PTTA_BACKBONE_NLSPN = 1
PTTA_BACKBONE_COSTDCNET = 2
PTTA_NLSPN_LEGACY_OFFSET = 0x100
PTTA_NLSPN_SYNCBN_ADAPT = 0x200
PTTA_SYNCBN_ADAPT = 0x200
PTTA_ADAPT_META_ONLY = 0x400
PTTA_COSTDC_PLAIN = 0x800      # CostDCNet without the meta layer (with PTTA_ADAPT_META_ONLY: the source model)
PTTA_MSGCHN_PLAIN = 0x1000     # MSG_CHN without the meta layer: the source model (eval forward only)
PTTA_META_1LAYER = 0
PTTA_META_2LAYERS = 1
PTTA_META_NONE = 2             # NLSPN without the meta layer: the source model / the BatchNorm-adaptation baseline
PTTA_DTYPE_F32 = 0
PTTA_DTYPE_MIXED = 1
PTTA_HEAD_FORM_PLAIN = 0
PTTA_HEAD_FORM_SYNCBN = 1
# ptta_op_gconv / ptta_op_gconv_affine `flags`
PTTA_GCONV_VERT = 1
PTTA_GCONV_X1_W2 = 2
PTTA_GCONV_DGRAD = 4
PTTA_GCONV_AFF_ACT_FIRST = 8
PTTA_GCONV_AFF_RES_PLAIN = 16
PTTA_ABI_VERSION = 2           # include/ptta.h; checked against ptta_version() at load
CONV_S1, CONV_S2, CONV_T2 = 0, 1, 2


class Hparams(ctypes.Structure):
    _fields_ = [('lr', c_float), ('beta1', c_float), ('beta2', c_float), ('eps', c_float),
                ('weight_decay', c_float), ('w_sparse_depth', c_float), ('w_smoothness', c_float),
                ('w_cos', c_float), ('max_input_depth', c_float), ('max_predict_depth', c_float)]


class GbnView(ctypes.Structure):
    _fields_ = [('p', c_void_p), ('c', c_int), ('ld', c_int)]


class GbnArgs(ctypes.Structure):               # include/ptta.h ptta_gbn_args
    _fields_ = ([(n, c_int) for n in ('mode', 'b', 'h', 'w', 'npass', 'act', 'act_first', 'res_relu', 'acc_gx', 'acc_gres', 'world',
                                      'nblocks_in', 'repeats')] + [('eps', c_float), ('momentum', c_float)] +
                [(n, GbnView) for n in ('x', 'res', 'y', 'g', 'gx', 'gres')] +
                [(n, c_void_p) for n in ('gamma', 'beta', 'part_in', 'st', 'rm', 'rv', 'nbt', 'st_eval', 'dgamma', 'dbeta')])


class CdSbnArgs(ctypes.Structure):             # include/ptta.h ptta_cd_sbn_args
    _fields_ = ([(n, c_int) for n in ('mode', 'level', 'c', 'relu', 'repeats', 'world', 'acc_res')] +
                [(n, c_void_p) for n in ('f', 'res', 'y', 'g', 'gamma', 'beta', 'rm', 'rv', 'nbt', 'out', 'st', 'dgamma', 'dbeta', 'gx', 'gres')])


class PlaneArg(ctypes.Structure):              # include/ptta.h ptta_plane
    _fields_ = [('p', c_void_p), ('nb', c_int), ('norm', c_int), ('div', c_float), ('mean', c_float), ('stdv', c_float)]


class ConvInArgs(ctypes.Structure):            # include/ptta.h ptta_conv_in_args
    _fields_ = ([(n, c_int) for n in ('cin', 'cin_total', 'cin_first', 'transpose_flip', 'up_nb', 'mask_nb', 'add1_nb', 'a_bits_nb', 'zero_from_b', 'b',
                                      'h', 'w', 'dtype', 'naive', 'max_blocks')] + [('pl', PlaneArg * 3)] +
                [(n, c_void_p) for n in ('weight', 'bias', 'up', 'mask', 'mask_bits', 'add1', 'out_raw', 'out_sum', 'a_bits')])


class ConvOut1Args(ctypes.Structure):          # include/ptta.h ptta_conv_out1_args
    _fields_ = ([(n, c_int) for n in ('in_nb', 'src_cin_total', 'src_cin_index', 'from_conv_in', 'add_nb', 'relu_in', 'dtype', 'b', 'h', 'w', 'max_blocks')] +
                [(n, c_void_p) for n in ('in', 'weight', 'bias', 'add', 'out')])


class LossArgs(ctypes.Structure):              # include/ptta.h ptta_loss_args
    _fields_ = ([(n, c_int) for n in ('fwd', 'bwd', 'n', 'h', 'w', 'd')] + [('r', ctypes.c_longlong)] +
                [(n, c_float) for n in ('max_input_depth', 'w_sd', 'w_sm', 'w_cos')] +
                [(n, c_void_p) for n in ('depth', 'image', 'sparse', 'validity', 'emb', 'ref', 'loss_info', 'rowstats', 'gdepth', 'gref', 'coef')])


class HnGemmArgs(ctypes.Structure):            # include/ptta.h ptta_hn_gemm_args
    _fields_ = ([(n, c_int) for n in ('pro', 'epi', 'x_bf16', 'cpart_n')] + [('r', ctypes.c_longlong)] +
                [(n, c_void_p) for n in ('A', 'Af', 'Bref', 'rowstats', 'coef', 'X', 'W0', 'b0', 'pscale', 'pshift', 'W', 'bias', 'C', 'part', 'E', 'rs',
                                         'rowstats_out', 'cpart', 'escale', 'eshift', 'emean', 'einv', 'W0t', 'P', 'w_image')])


class HnMomentsArgs(ctypes.Structure):         # include/ptta.h ptta_hn_moments_args
    _fields_ = ([(n, c_int) for n in ('x_bf16', 'npass', 'bn')] + [('r', ctypes.c_longlong), ('eps', c_float), ('momentum', c_float)] +
                [(n, c_void_p) for n in ('X', 'W0', 'b0', 'part', 'gamma', 'beta', 'rm', 'rv', 'nbt', 'mean', 'inv', 'scale', 'shift')])


class GwgradViewArgs(ctypes.Structure):        # include/ptta.h ptta_gwgrad_view_args
    _fields_ = ([(n, c_int) for n in ('b', 'h', 'w', 'ci', 'co', 'ldx', 'ldg', 'gy_bf16')] +
                [(n, c_void_p) for n in ('x', 'gy', 'gw', 'gb', 'pw', 'mw', 'vw', 'pb', 'mb', 'vb', 'hyper', 'step', 'ticket')])


class LinearWgradArgs(ctypes.Structure):       # include/ptta.h ptta_linear_wgrad_args
    _fields_ = ([('r', ctypes.c_longlong), ('o', c_int), ('i', c_int)] +
                [(n, c_void_p) for n in ('G', 'Gh', 'gscale', 'gc1', 'gc2', 'gmean', 'ginv', 'X', 'xscale', 'xshift', 'dW', 'db')])


class SummaryArgs(ctypes.Structure):           # include/ptta.h ptta_summary_args
    _fields_ = ([(n, c_int) for n in ('n_show', 'height', 'width', 'n_images', 'rows', 'normalize', 'out_dtype')] + [('max_predict_depth', c_float)] +
                [('rev_mean', c_float * 3), ('rev_std', c_float * 3), ('image', c_void_p * 8), ('image_div255', c_void_p * 8)] +
                [(n, c_void_p) for n in ('output_depth', 'sparse_depth', 'validity_map', 'ground_truth', 'viridis', 'inferno', 'out')])


class ScoreArgs(ctypes.Structure):             # include/ptta.h ptta_score_args
    _fields_ = ([('depth', c_void_p), ('ground_truth', c_void_p)] +
                [(n, c_int) for n in ('n', 'height', 'width', 'win_y', 'win_x', 'win_height', 'win_width')] +
                [('min_evaluate_depth', c_float), ('max_evaluate_depth', c_float), ('rule', c_int)] +
                [(n, c_void_p) for n in ('state', 'batch_out', 'sample_out', 'sample_count_out')])


class AugmentArgs(ctypes.Structure):           # include/ptta.h ptta_augment_args
    _fields_ = ([(n, c_void_p) for n in ('image', 'sparse_depth', 'validity_map', 'ground_truth', 'loss_image', 'sparse_depth_out',
                                         'validity_map_out', 'ground_truth_out', 'image1', 'draws')] +
                [(n, c_int) for n in ('n', 'height', 'width', 'crop_height', 'crop_width', 'image_bilinear', 'scale_depth', 'pass2')] +
                [('scratch', c_void_p), ('scratch_bytes', c_int64)])


# ptta_augment_draw `flags`
PTTA_AUG_HFLIP, PTTA_AUG_VFLIP, PTTA_AUG_ROTATE, PTTA_AUG_RESIZE = 1, 2, 4, 8
PTTA_AUG_BRIGHTNESS, PTTA_AUG_CONTRAST, PTTA_AUG_GAMMA, PTTA_AUG_HUE, PTTA_AUG_SATURATION = 16, 32, 64, 128, 256

# ptta_score_args `rule`, the largest max_n a score state is sized for
PTTA_SCORE_RULE_ADAPT, PTTA_SCORE_RULE_VALIDATE = 0, 1
PTTA_SCORE_MAX_N = 4096

# ptta_summary_args `rows` / `out_dtype`, the size of ptta_summary_image_flag's buffer
PTTA_SUMMARY_MAX_IMAGES = 8
PTTA_SUMMARY_ROW_OUTPUT, PTTA_SUMMARY_ROW_SPARSE, PTTA_SUMMARY_ROW_GT = 1, 2, 4
PTTA_SUMMARY_OUT_F32_CHW, PTTA_SUMMARY_OUT_U8_HWC = 0, 1
PTTA_SUMMARY_FLAG_WORDS = 257

# ptta_op_loss `fwd` / `bwd`, ptta_op_conv_in's *form_host
LOSS_FWD = {'merged': 0, 'nocos': 1, 'split': 2, 'split_narrow': 3}
LOSS_BWD = {'none': 0, 'unfused': 1, 'fused': 2, 'counted': 3}
CONV_IN_FORMS = ('lds', 'lds_mask', 'direct', 'naive')

# ptta_op_cd_dense `op`
CD_OPS = {'pad_dual': 0, 'crop_avg': 1, 'scatter_dual_grad': 2, 'stage': 3, 'clamp': 4, 'fusion_fwd': 5, 'fusion_bwd': 6, 'pool_fwd': 7,
          'pool_bwd': 8, 'up_fwd': 9, 'up_bwd': 10, 'regress_fwd': 11, 'regress_bwd': 12, 'rows_fwd': 13, 'rows_bwd': 14}

# every symbol include/ptta.h declares: (name, restype, argtypes)
_P = c_void_p
SIGNATURES = [
    ('ptta_create', c_int, [POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Hparams)]),
    ('ptta_destroy', None, [_P]),
    ('ptta_last_error', c_char_p, [_P]),
    ('ptta_set_hparams', c_int, [_P, POINTER(Hparams), _P]),
    ('ptta_load_weights', c_int, [_P, c_char_p, _P, POINTER(c_int64), c_int, _P]),
    ('ptta_bind_adapted', c_int, [_P, c_char_p, _P, _P, _P]),
    ('ptta_set_adam_step', c_int, [_P, c_int, _P]),
    ('ptta_get_adam_step', c_int, [_P, POINTER(c_int), _P]),
    ('ptta_forward_train', c_int, [_P, _P, _P, _P, _P, _P, _P]),
    ('ptta_embedding_rows', c_int64, [_P]),
    ('ptta_forward_eval', c_int, [_P, _P, _P, _P, _P]),
    ('ptta_loss_forward', c_int, [_P, _P, _P, _P, _P, _P, _P, c_int64, c_float, c_float, c_float, _P, _P]),
    ('ptta_loss_backward', c_int, [_P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P, _P]),
    ('ptta_backward', c_int, [_P, _P, _P, _P, _P, _P]),
    ('ptta_set_grad', c_int, [_P, c_char_p, _P, c_int64, _P]),
    ('ptta_get_grad', c_int, [_P, c_char_p, _P, c_int64, _P]),
    ('ptta_adapted_count', c_int, [_P]),
    ('ptta_adapted_name', c_char_p, [_P, c_int, POINTER(c_int64)]),
    ('ptta_adapted_repeat', c_int, [_P, c_int]),
    ('ptta_adam_step', c_int, [_P, _P, _P, _P]),
    ('ptta_step', c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    ('ptta_step_pipelined', c_int, [_P] * 5 + [c_uint64] + [_P] * 2 + [c_uint64] + [_P] * 3),
    ('ptta_pipeline_stream', c_int, [_P, POINTER(c_void_p)]),
    ('ptta_forward_eval_last', c_int, [_P, _P, _P]),
    ('ptta_outlier_removal', c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P]),
    ('ptta_eval_metrics', c_int, [_P, _P, c_int64, c_float, c_float, _P, _P, _P]),
    ('ptta_mdconv_forward', c_int, [_P] * 6 + [c_int] * 15 + [_P]),
    ('ptta_mdconv_backward', c_int, [_P] * 11 + [c_int] * 15 + [_P]),
    ('ptta_set_image_norm', c_int, [_P, c_float, POINTER(c_float), POINTER(c_float)]),
    ('ptta_head_bind', c_int, [_P, c_char_p, _P, _P, _P]),
    ('ptta_head_set_hparams', c_int, [_P, c_float, c_float, c_float, c_float, c_float, c_float, c_int, _P]),
    ('ptta_head_reload', c_int, [_P, _P]),
    ('ptta_head_forward', c_int, [_P, _P, _P, c_int, _P, _P, _P]),
    ('ptta_head_backward', c_int, [_P, _P, _P]),
    ('ptta_head_adam_step', c_int, [_P, _P]),
    ('ptta_head_step', c_int, [_P, _P, _P, c_int, _P, _P]),
    ('ptta_head_get_grad', c_int, [_P, c_char_p, _P, c_int64, POINTER(c_int), _P]),
    ('ptta_head_set_form', c_int, [_P, c_int]),
    ('ptta_crop_flip', c_int, [_P, _P] + [c_int] * 6 + [_P] * 5),
    ('ptta_ingest_raw', c_int, [_P] * 8 + [c_int] * 5 + [_P, _P, c_float, _P]),
    ('ptta_egress_raw', c_int, [_P] * 6 + [c_int] * 5 + [_P, _P, c_float, c_float, _P]),
    ('ptta_inpaint_scratch_bytes', c_int64, [c_int, c_int, c_int, c_int]),
    ('ptta_inpaint_biharmonic', c_int, [_P, c_int, c_int, c_int, c_int, c_int, ctypes.c_double, _P, c_int64, _P, _P]),
    ('ptta_summary_grid_shape', c_int, [c_int, c_int, c_int, c_int, POINTER(c_int64), POINTER(c_int64)]),
    ('ptta_summary_image_flag', c_int, [_P, c_int64, _P, _P]),
    ('ptta_summary_compose', c_int, [POINTER(SummaryArgs), _P]),
    ('ptta_score_state_bytes', c_int64, [c_int]),
    ('ptta_score_reset', c_int, [_P, c_int64, _P]),
    ('ptta_score_accumulate', c_int, [POINTER(ScoreArgs), _P]),
    ('ptta_score_result', c_int, [_P, c_int64, _P, _P]),
    ('ptta_rotate', c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P]),
    ('ptta_resize_crop', c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    ('ptta_photometric', c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    ('ptta_photometric_full', c_int, [_P, _P, c_int, c_int, c_int] + [_P] * 12),
    ('ptta_add_noise', c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, c_float, c_int, _P]),
    ('ptta_remove_patches', c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    ('ptta_crop_pad', c_int, [_P, _P, c_int, c_int, c_int, c_int] + [_P] * 7 + [c_int, c_float, _P]),
    ('ptta_resize_pad', c_int, [_P, _P, c_int, c_int, c_int, c_int] + [_P] * 5 + [c_int, c_int, c_float, _P]),
    ('ptta_augment_scratch_bytes', c_int64, [c_int, c_int, c_int]),
    ('ptta_augment_frames', c_int, [POINTER(AugmentArgs), _P]),
    ('ptta_set_stat_sync', c_int, [_P, _P, _P, _P, c_int64, c_int]),
    ('ptta_rccl_unique_id', c_int, [_P]),
    ('ptta_rccl_comm_create', c_int, [_P, c_int, c_int, POINTER(c_void_p)]),
    ('ptta_rccl_comm_destroy', c_int, [_P]),
    ('ptta_rccl_allreduce_mean_f32', c_int, [_P, _P, c_int64, _P]),
    ('ptta_rccl_last_error', c_char_p, []),
    ('ptta_set_stat_sync_rccl', c_int, [_P, _P, _P, c_int64, c_int]),
    ('ptta_set_grad_sync_rccl', c_int, [_P, _P]),
    ('ptta_set_graph', c_int, [_P, c_int]),
    ('ptta_set_option', c_int, [_P, c_char_p, c_int]),
    ('ptta_get_option', c_int, [_P, c_char_p, POINTER(c_int)]),
    ('ptta_profile', c_int, [_P, c_int]),
    ('ptta_profile_read', c_int, [_P, c_int, POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                  POINTER(c_int64), _P]),
    ('ptta_debug_tensor', c_int, [_P, c_char_p, _P, c_int64, POINTER(c_int64), _P]),
    ('ptta_op_conv32', c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    ('ptta_op_conv32_chain', c_int, [_P] * 6 + [c_int] * 7 + [POINTER(c_float), _P]),
    ('ptta_op_conv32_pair', c_int, [_P] * 16 + [c_int] * 12 + [POINTER(c_int), _P]),
    ('ptta_op_conv32_tpair', c_int, [_P] * 16 + [c_int] * 14 + [POINTER(c_int), _P]),
    ('ptta_op_gwgrad', c_int, [_P, _P, _P, _P] + [c_int] * 7 + [POINTER(c_float), _P]),
    ('ptta_op_gconv', c_int, [_P, c_int, c_int, _P, c_int, c_int, _P, _P, _P] + [c_int] * 16 + [POINTER(ctypes.c_double), POINTER(c_int), _P]),
    ('ptta_op_gconv_affine', c_int, [_P, c_int, c_int, _P, c_int, c_int, _P, _P, _P] + [c_int] * 16 + [POINTER(ctypes.c_double), POINTER(c_int),
                                     _P, _P, _P, c_int, _P]),
    ('ptta_op_gbn', c_int, [POINTER(GbnArgs), _P]),
    ('ptta_cd_sparse_create', c_int, [POINTER(c_void_p), c_int, c_int, c_int]),
    ('ptta_cd_sparse_destroy', None, [_P]),
    ('ptta_cd_sparse_build', c_int, [_P, _P, c_float, _P]),
    ('ptta_cd_sparse_read', c_int, [_P, c_int, POINTER(c_int), _P, ctypes.c_longlong, _P, _P, _P]),
    ('ptta_op_cd_sparse_conv', c_int, [_P, _P, _P, _P] + [c_int] * 7 + [_P]),
    ('ptta_op_cd_sbn', c_int, [_P, POINTER(CdSbnArgs), _P]),
    ('ptta_op_cd_densify', c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    ('ptta_op_cd_dense', c_int, [c_int, _P, _P, _P, _P, POINTER(c_int), POINTER(c_float), _P]),
    ('ptta_op_conv_in', c_int, [POINTER(ConvInArgs), POINTER(c_int), _P]),
    ('ptta_op_conv_out1', c_int, [POINTER(ConvOut1Args), _P]),
    ('ptta_op_prep', c_int, [_P, c_float, _P, _P, _P, c_int, c_int, c_int, _P]),
    ('ptta_op_up2_1ch', c_int, [_P, _P, c_int, c_int, c_int, _P]),
    ('ptta_op_up2t_1ch', c_int, [_P, _P, c_int, c_int, c_int, _P]),
    ('ptta_op_up2t_32', c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    ('ptta_op_loss', c_int, [POINTER(LossArgs), _P]),
    ('ptta_nl_det_scratch_bytes', c_int64, [c_int, c_int, c_int]),
    ('ptta_op_nl_prop_bwd', c_int, [_P] * 8 + [c_int] * 4 + [_P, c_int, POINTER(c_float), _P]),
    ('ptta_op_nl_affinity_bwd', c_int, [_P, _P, _P, c_int, _P, _P, _P, _P] + [c_int] * 4 + [_P, _P]),
    ('ptta_op_hn_tiled_elems', ctypes.c_longlong, [ctypes.c_longlong]),
    ('ptta_op_hn_gemm', c_int, [POINTER(HnGemmArgs), _P]),
    ('ptta_op_hn_moments', c_int, [POINTER(HnMomentsArgs), _P]),
    ('ptta_op_hn_untile', c_int, [_P, _P, ctypes.c_longlong, _P]),
    ('ptta_op_head_bwd_finish', c_int, [_P, _P, _P, _P, ctypes.c_longlong, _P, c_int, c_int, _P]),
    ('ptta_op_wgrad32', c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P]),
    ('ptta_op_gwgrad_view', c_int, [POINTER(GwgradViewArgs), _P]),
    ('ptta_op_adam', c_int, [_P, _P, _P, _P, ctypes.c_longlong, _P, _P, _P]),
    ('ptta_op_adam_multi', c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ('ptta_op_ema_multi', c_int, [c_int, _P, _P, _P, _P, _P]),
    ('ptta_op_linear_wgrad', c_int, [POINTER(LinearWgradArgs), _P]),
    ('ptta_op_glinear_wgrad', c_int, [_P, c_int, c_int, _P, c_int, c_int, ctypes.c_longlong, _P, _P, _P]),
    ('ptta_version', c_int, []),
]

_lib = None


def load():
    """Load libptta_hip.so (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64: import it FIRST so that this library binds to the HIP runtime torch uses
    # (loading libptta_hip.so first would pull /opt/rocm's copy into the process and torch would then see no device)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('libptta_hip.so not found at %s: build it with `python -c "import '
                           '__graft_entry__ as g; g.build()"` — there is no CPU fallback' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    have = lib.ptta_version()
    if have != PTTA_ABI_VERSION:
        raise RuntimeError('%s has ABI version %d, this binding is written against %d (include/ptta.h PTTA_ABI_VERSION): rebuild it with '
                           '`make -C tta-depth-completion_amd/csrc`' % (LIB_PATH, have, PTTA_ABI_VERSION))
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    if rc != 0:
        msg = lib.ptta_last_error(handle).decode() if handle else ''
        raise RuntimeError('%s failed (%d): %s' % (what, rc, msg))


def ptr(t):
    """Device pointer of a contiguous torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous()
    return c_void_p(t.data_ptr())


__all__ = ['load', 'check', 'ptr', 'Hparams', 'GbnArgs', 'GbnView', 'CdSbnArgs', 'CD_OPS', 'PlaneArg', 'ConvInArgs', 'ConvOut1Args', 'LossArgs', 'HnGemmArgs', 'HnMomentsArgs', 'GwgradViewArgs', 'LinearWgradArgs', 'SummaryArgs', 'ScoreArgs', 'AugmentArgs',
           'LOSS_FWD', 'LOSS_BWD', 'CONV_IN_FORMS', 'SIGNATURES', 'LIB_PATH', 'byref']
