"""The C ABI of include/xvec_hip.h as ctypes sees it: the constants, the mirrors of the header's structs and ONE table of every
function's return and parameter types, which lib() applies to the loaded library once.  tests/test_abi_table.py reads the
header and holds this table to it.  Needs neither numpy nor torch nor the built library to import.
"""
import ctypes
import os
from ctypes import POINTER, c_int, c_int16

XV_OK = 0
XV_ERR_IO, XV_ERR_MODEL, XV_ERR_DEVICE, XV_ERR_ARG, XV_ERR_INTERNAL = 1, 2, 3, 4, 5
PREC_BF16X3, PREC_BF16, PREC_FP16, PREC_FP16X3, PREC_FP16X2, PREC_AUTO, PREC_FP16MX, PREC_FP16MX2, PREC_FP16X3E = range(9)
PREC_DEFAULT = -1   # XV_PREC_DEFAULT: the one policy of every entry point (fp16mx2 where the model allows, else fp16x3)
PRECISIONS = {"default": PREC_DEFAULT, "bf16x3": PREC_BF16X3, "bf16": PREC_BF16, "fp16": PREC_FP16, "fp16x3": PREC_FP16X3,
              "fp16x2": PREC_FP16X2, "auto": PREC_AUTO, "fp16mx": PREC_FP16MX, "fp16mx2": PREC_FP16MX2}
PRECISION_NAMES = {v: k for k, v in PRECISIONS.items()}
# MFMA issue time per algorithmic product in units of one fp16 16x16x32 pass (fp16mx: + one 4-bit 16x16x128 per four)
MFMA_PASSES = {"bf16x3": 3, "bf16": 1, "fp16": 1, "fp16x3": 3, "fp16x2": 2, "fp16mx": 1.25}
EPI_ACT, EPI_F32, EPI_STATS = 0, 1, 2


class XvError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("xvec_hip status %d: %s" % (status, msg))
        self.status = status


class ModelInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("input_dim", "output_dim", "left_context", "right_context",
                                              "min_frames", "num_layers", "output_is_segment", "reserved")]


class SegDesc(ctypes.Structure):
    _fields_ = [("hi", ctypes.c_void_p), ("lo", ctypes.c_void_p), ("ld", ctypes.c_int32),
                ("row_shift", ctypes.c_int32), ("k_len", ctypes.c_int32), ("gmax", ctypes.c_void_p),
                ("lo4", ctypes.c_void_p), ("lo4_scale", ctypes.c_void_p)]


class GemmDesc(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int32), ("epilogue", ctypes.c_int32), ("nseg", ctypes.c_int32),
                ("seg", SegDesc * 8),
                ("w_hi", ctypes.c_void_p), ("w_lo", ctypes.c_void_p), ("ldw", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("n_pad", ctypes.c_int32),
                ("bias", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("offset", ctypes.c_void_p),
                ("relu", ctypes.c_int32), ("bn", ctypes.c_int32),
                ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("ldo", ctypes.c_int32),
                ("out_f32", ctypes.c_void_p), ("ldf", ctypes.c_int32), ("m_valid", ctypes.c_int32),
                ("partial", ctypes.c_void_p), ("ldp", ctypes.c_int32), ("grp_range", ctypes.c_void_p),
                ("hip_stream", ctypes.c_void_p),
                ("w4", ctypes.c_void_p), ("ldw4", ctypes.c_int32), ("w4_scale", ctypes.c_void_p),
                ("gmax_out", ctypes.c_void_p),
                ("w4b", ctypes.c_void_p), ("ldw4b", ctypes.c_int32), ("w4b_scale", ctypes.c_void_p),
                ("out_lo4", ctypes.c_void_p), ("out_lo4_scale", ctypes.c_void_p),
                ("p8", ctypes.c_int32),
                ("out_range", ctypes.c_void_p), ("ksplit", ctypes.c_int32)]


class GemmPlanGroup(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("ld", "ksteps", "nshift", "shift0", "dstep", "wcol0", "wstride", "ld4s")]


class GemmPlan(ctypes.Structure):
    """xv_gemm_plan: what a kernel_tdnn_gemm call would launch (plan_gemm)"""
    _fields_ = [("refused", ctypes.c_int32), ("kernel", ctypes.c_char * 96)] + \
               [(n, ctypes.c_int32) for n in ("grid_x", "grid_y", "block", "lds_bytes", "mf", "lanes", "groups_per_xcd", "sk_mtiles",
                                              "p8_ktiles", "p8_ktiles_lo", "p8_whole", "stagger_units")] + \
               [("workspace_bytes", ctypes.c_int64), ("ngrp", ctypes.c_int32), ("ngrp_lo", ctypes.c_int32), ("lo_ksteps", ctypes.c_int32),
                ("grp", GemmPlanGroup * 16)]


class FirstLayerDesc(ctypes.Structure):
    """xv_first_layer_desc (row_offsets / dev_off are HOST arrays: keep the numpy arrays alive over the call)"""
    _fields_ = [("feats", ctypes.c_void_p), ("row_offsets", ctypes.c_void_p), ("dev_off", ctypes.c_void_p), ("B", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("pad_left", ctypes.c_int32), ("pad_right", ctypes.c_int32),
                ("dim", ctypes.c_int32), ("noff", ctypes.c_int32), ("off", ctypes.c_int32 * 8),
                ("w_hi", ctypes.c_void_p), ("w_lo", ctypes.c_void_p), ("ldw", ctypes.c_int32), ("seg_pad", ctypes.c_int32),
                ("n_pad", ctypes.c_int32), ("epi_prec", ctypes.c_int32),
                ("bias", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("offset", ctypes.c_void_p),
                ("relu", ctypes.c_int32), ("bn", ctypes.c_int32),
                ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("ldo", ctypes.c_int32),
                ("out_lo4", ctypes.c_void_p), ("out_lo4_scale", ctypes.c_void_p),
                ("gmax_out", ctypes.c_void_p), ("out_range", ctypes.c_void_p),
                ("row0", ctypes.c_int32), ("nrows", ctypes.c_int32), ("max_wgs", ctypes.c_int32),
                ("hip_stream", ctypes.c_void_p)]


class PrepInputDesc(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int32), ("feats", ctypes.c_void_p), ("src_off", ctypes.c_void_p), ("dev_off", ctypes.c_void_p),
                ("grp_utt", ctypes.c_void_p), ("rows", ctypes.c_int32), ("dim", ctypes.c_int32), ("ld", ctypes.c_int32),
                ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("pad_left", ctypes.c_int32), ("pad_right", ctypes.c_int32),
                ("zero_words", ctypes.c_void_p), ("n_zero_words", ctypes.c_int32), ("hip_stream", ctypes.c_void_p)]


class PoolFinaliseDesc(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int32), ("partial", ctypes.c_void_p), ("ldp", ctypes.c_int32),
                ("utt_grp0", ctypes.c_void_p), ("utt_grp1", ctypes.c_void_p), ("utt_count", ctypes.c_void_p),
                ("B", ctypes.c_int32), ("dim", ctypes.c_int32), ("var_floor", ctypes.c_float),
                ("out_hi", ctypes.c_void_p), ("out_lo", ctypes.c_void_p), ("ld", ctypes.c_int32), ("hip_stream", ctypes.c_void_p)]


class FrameOutputDesc(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("src16", ctypes.c_void_p), ("ld", ctypes.c_int32),
                ("out_row", ctypes.c_void_p), ("n_out", ctypes.c_int32), ("dim", ctypes.c_int32), ("log_softmax", ctypes.c_int32),
                ("out", ctypes.c_void_p), ("out_ld", ctypes.c_int32), ("hip_stream", ctypes.c_void_p)]


class Calibration(ctypes.Structure):
    """xv_calibration: what xv_ctx_calibrate measured and chose."""
    _fields_ = [("chosen", ctypes.c_int32), ("checked", ctypes.c_int32), ("err_mx", ctypes.c_float), ("err_mx2", ctypes.c_float),
                ("checked_mx", ctypes.c_int32), ("err_lite", ctypes.c_float), ("lite_mask", ctypes.c_uint64),
                ("err_holdout", ctypes.c_float), ("checked_holdout", ctypes.c_int32), ("lite_dropped", ctypes.c_int32),
                ("tail", ctypes.c_float)]

    def as_dict(self):
        d = {"chosen": PRECISION_NAMES.get(self.chosen, str(self.chosen)), "checked": self.checked, "checked_mx": self.checked_mx,
             "err_mx": self.err_mx, "err_mx2": self.err_mx2, "tail": self.tail}
        if self.lite_mask:
            d["lite_mask"] = int(self.lite_mask)
            d["err_lite"] = self.err_lite
            d["err_holdout"] = self.err_holdout
            d["checked_holdout"] = self.checked_holdout
        if self.lite_dropped:
            d["lite_dropped"] = self.lite_dropped
        return d


class MfccOptions(ctypes.Structure):
    """xv_mfcc_options; mfcc_options() gives Kaldi's defaults with keyword overrides."""
    _fields_ = [(n, ctypes.c_float) for n in ("sample_frequency", "frame_length_ms", "frame_shift_ms", "dither",
                                              "preemphasis_coefficient", "blackman_coeff")] + \
               [(n, ctypes.c_int32) for n in ("remove_dc_offset", "window_type", "round_to_power_of_two", "snip_edges", "num_mel_bins")] + \
               [("low_freq", ctypes.c_float), ("high_freq", ctypes.c_float), ("num_ceps", ctypes.c_int32),
                ("cepstral_lifter", ctypes.c_float), ("use_energy", ctypes.c_int32), ("raw_energy", ctypes.c_int32),
                ("energy_floor", ctypes.c_float)]


class VadOptions(ctypes.Structure):
    _fields_ = [("vad_energy_threshold", ctypes.c_float), ("vad_energy_mean_scale", ctypes.c_float),
                ("vad_proportion_threshold", ctypes.c_float), ("vad_frames_context", ctypes.c_int32)]


class ReverbOptions(ctypes.Structure):
    """xv_reverb_options; reverb_options() gives Kaldi's defaults with keyword overrides."""
    _fields_ = [("shift_output", ctypes.c_int32), ("normalize_output", ctypes.c_int32), ("duration", ctypes.c_float),
                ("volume", ctypes.c_float), ("input_wave_channel", ctypes.c_int32), ("rir_channel", ctypes.c_int32),
                ("noise_channel", ctypes.c_int32)]


ST, STR, VP, SZ = c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t   # xv_status; char*; any other pointer passed as an address
I32, I64, U64, F32, F64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
PI32, PI64, PU64, PF32, PF64, PVP = POINTER(I32), POINTER(I64), POINTER(U64), POINTER(F32), POINTER(F64), POINTER(VP)

# name -> (restype, argtypes) of every function the header declares, in its order.  A parameter is VP where the callers pass
# ndarray.ctypes.data integers, a typed POINTER where they pass byref() of a ctypes object.
SIGNATURES = {
    "xv_last_error": (STR, []),
    "xv_version": (STR, []),
    "xv_model_load": (ST, [VP, SZ, STR, STR, PVP]),
    "xv_model_load_rxfilename": (ST, [STR, STR, STR, PVP]),
    "xv_model_free": (None, [VP]),
    "xv_model_info": (ST, [VP, POINTER(ModelInfo)]),
    "xv_model_macs": (F64, [VP, I32]),
    "xv_model_describe": (SZ, [VP, STR, SZ]),
    "xv_model_pack": (ST, [VP, c_int, VP, POINTER(SZ)]),
    "xv_ctx_create": (ST, [VP, c_int, c_int, PVP]),
    "xv_ctx_create_from_blob": (ST, [VP, SZ, c_int, PVP]),
    "xv_ctx_create_from_device_blob": (ST, [VP, SZ, c_int, PVP]),
    "xv_ctx_free": (None, [VP]),
    "xv_ctx_info": (ST, [VP, POINTER(ModelInfo), PI32, PI32]),
    "xv_forward_batch": (ST, [VP, VP, VP, I32, VP]),
    "xv_forward_batch_device": (ST, [VP, VP, VP, I32, VP, I32, VP]),
    "xv_ctx_synchronize": (ST, [VP]),
    "xv_ctx_calibrate": (ST, [VP, VP, VP, I32, F32, POINTER(Calibration)]),
    "xv_ctx_set_fast_mode": (ST, [VP, I32]),
    "xv_ctx_fast_mode": (ST, [VP, PI32]),
    "xv_ctx_set_lite_layers": (ST, [VP, U64]),
    "xv_ctx_lite_layers": (ST, [VP, PU64]),
    "xv_calibrate_table": (ST, [VP, STR, I32, I32, I32, I32, F32, POINTER(Calibration)]),
    "xv_ctx_set_calibration": (ST, [VP, I32, F32]),
    "xv_calibration_file_read": (ST, [STR, PI32, PU64, PI32, PU64]),
    "xv_calibration_file_publish": (ST, [STR, U64, I32, U64, F32, STR, PI32, PU64, PI32, PU64]),
    "xv_ctx_model_fingerprint": (ST, [VP, PU64]),
    "xv_ctx_share_calibration": (ST, [VP, STR, F32, STR, PI32]),
    "xv_ctx_set_calibration_file": (ST, [VP, STR]),
    "xv_ctx_set_profiling": (ST, [VP, I32]),
    "xv_ctx_profile_report": (SZ, [VP, STR, SZ]),
    "xv_extract_utterances": (ST, [VP, VP, VP, I32, I32, I32, I32, VP, VP]),
    "xv_extract_table": (ST, [VP, STR, STR, I32, I32, I32, I32, PI64, PI64]),
    "xv_recognize_feature_pipeline": (ST, [STR, PI32, STR, SZ, STR, SZ, PI32, PI32, PI32]),
    "xv_frontend_cmvn_select": (ST, [VP, VP, VP, I32, VP, I32, I32, VP, VP]),
    "xv_plan_chunks": (ST, [I32, I32, I32, I32, I32, I32, VP, VP, VP, VP, PI32]),
    "xv_ctx_create_broadcast": (ST, [VP, POINTER(c_int), c_int, c_int, PVP]),
    "xv_backend_apply": (ST, [c_int, VP, I32, I32, VP, VP, I32, I32, I32, I32, VP, VP]),
    "xv_segment_mean": (ST, [c_int, VP, I32, I32, VP, VP, I32, I32, VP]),
    "xv_scatter_stats": (ST, [c_int, VP, I32, I32, VP, VP, I32, VP, VP, VP, VP]),
    "xv_plda_transform": (ST, [c_int, VP, I32, I32, VP, VP, VP, VP, I32, I32, VP, VP, VP]),
    "xv_plda_score": (ST, [c_int, VP, VP, I32, VP, I32, I32, VP, VP, I64, VP, VP]),
    "xv_lda_estimate": (ST, [I32, I64, VP, VP, VP, F64, F64, I32, VP, VP]),
    "xv_plda_estimate": (ST, [I32, I32, VP, VP, VP, VP, I32, VP, VP, VP, VP]),
    "xv_plda_adapt": (ST, [I32, I64, VP, VP, VP, VP, VP, F64, F64, F64, VP, VP, VP, VP]),
    "xv_mfcc_options_default": (None, [POINTER(MfccOptions)]),
    "xv_mfcc_num_frames": (I64, [POINTER(MfccOptions), I64]),
    "xv_mfcc_utt_seed": (U64, [STR]),
    "xv_mfcc_compute": (ST, [c_int, POINTER(MfccOptions), VP, VP, I32, VP, VP, VP]),
    "xv_mfcc_compute_i16": (ST, [c_int, POINTER(MfccOptions), VP, VP, I32, VP, VP, VP]),
    "xv_mfcc_kernel_time": (ST, [c_int, POINTER(MfccOptions), VP, VP, I32, I32, PF32]),
    "xv_vad_energy": (ST, [c_int, POINTER(VadOptions), VP, VP, I32, I32, VP]),
    "xv_wave_read": (ST, [STR, I32, PI32, POINTER(POINTER(c_int16)), PI64]),
    "xv_wave_free": (None, [POINTER(c_int16)]),
    "xv_reverb_options_default": (None, [POINTER(ReverbOptions)]),
    "xv_reverb_output_length": (I64, [POINTER(ReverbOptions), F32, I64, I64]),
    "xv_wav_reverberate": (ST, [c_int, POINTER(ReverbOptions), F32, VP, I32, VP, I32, VP, VP, I32, VP, VP, VP, I32, VP, VP, VP, VP, VP, VP, VP, VP]),
    "xv_reverb_kernel_time": (ST, [c_int, POINTER(ReverbOptions), F32, VP, I32, VP, I32, VP, VP, I32, VP, VP, VP, I32, VP, VP, VP, VP, I32, PF32]),
    "xv_recognize_wav_pipeline": (ST, [STR, PI32, STR, SZ]),
    "xv_wave_write": (ST, [STR, I32, VP, I64, PI64]),
    "xv_pack_mx_residual": (ST, [VP, VP, I32, I32, VP, VP, VP, VP, VP]),
    "xv_pack_mx_residual64": (ST, [VP, VP, I32, I32, VP, VP, VP, VP, VP]),
    "xv_pack_mx_weights": (ST, [VP, I32, I32, VP, VP, VP, VP, VP]),
    "xv_pack_mx_weights64": (ST, [VP, I32, I32, VP, VP, VP, VP, VP]),
    "xv_tile_mx_scales": (ST, [VP, I32, I32, I32, VP]),
    "xv_kernel_tdnn_gemm": (ST, [POINTER(GemmDesc)]),
    "xv_last_gemm_kernel": (STR, []),
    "xv_plan_gemm": (ST, [POINTER(GemmDesc), I32, POINTER(GemmPlan)]),
    "xv_plan_gemm_policy": (ST, [POINTER(GemmDesc), I32, I32, I32, I32, I32, POINTER(GemmPlan)]),
    "xv_compressed_size": (ST, [I32, I32, I32, POINTER(SZ), POINTER(STR)]),
    "xv_compress_matrices": (ST, [c_int, VP, VP, I32, I32, I32, VP, VP, VP]),
    "xv_compress_kernel_time": (ST, [c_int, VP, VP, I32, I32, I32, I32, PF32]),
    "xv_cmvn_sliding": (ST, [c_int, VP, VP, I32, I32, I32, I32, I32, VP]),
    "xv_cmvn_stats": (ST, [c_int, VP, VP, I32, I32, VP, VP]),
    "xv_cmvn_norm": (ST, [VP, I32, I32, I32, I32, VP, I32, VP, PI32]),
    "xv_cmvn_apply": (ST, [c_int, VP, VP, I32, I32, VP, VP, VP]),
    "xv_cmvn_apply_select": (ST, [c_int, VP, VP, I32, I32, VP, I32, VP, VP, VP, I32, VP]),
    "xv_recognize_cmvn_pipeline": (ST, [STR, PI32, STR, SZ]),
    "xv_cmvn_kernel_time": (ST, [c_int, VP, VP, I32, I32, I32, PF32, PF32]),
    "xv_add_deltas": (ST, [c_int, VP, VP, I32, I32, I32, I32, I32, VP, VP]),
    "xv_ubm_diag_create": (ST, [c_int, I32, I32, VP, VP, VP, PVP]),
    "xv_ubm_full_create": (ST, [c_int, I32, I32, VP, VP, VP, PVP]),
    "xv_ubm_destroy": (None, [VP]),
    "xv_ubm_gselect": (ST, [VP, VP, VP, I32, I32, VP, VP, VP]),
    "xv_ubm_post": (ST, [VP, VP, VP, I32, VP, I32, F32, VP, VP, VP, VP, VP, VP]),
    "xv_fgmm_to_gmm": (ST, [I32, I32, VP, VP, VP, VP, VP, VP]),
    "xv_fgmm_gconsts": (ST, [I32, I32, VP, VP, VP, VP, VP]),
    "xv_ubm_kernel_time": (ST, [VP, VP, VP, VP, I32, I32, F32, I32, VP]),
    "xv_ubm_full_gselect": (ST, [VP, VP, VP, I32, VP, I32, I32, VP, VP, VP]),
    "xv_ubm_frame_likes": (ST, [VP, VP, VP, I32, VP, I32, VP, VP]),
    "xv_vad_from_frame_likes": (ST, [I32, VP, I64, VP, VP, VP]),
    "xv_merge_vads": (ST, [VP, VP, I64, VP, I32, VP]),
    "xv_fgmm_acc_create": (ST, [c_int, I32, I32, STR, PVP]),
    "xv_fgmm_acc_destroy": (None, [VP]),
    "xv_fgmm_acc_add": (ST, [VP, VP, I32, VP, VP, VP]),
    "xv_fgmm_acc_add_gselect": (ST, [VP, VP, VP, I32, VP, I32, VP]),
    "xv_fgmm_acc_get": (ST, [VP, VP, VP, VP]),
    "xv_fgmm_est": (ST, [I32, I32, STR, VP, VP, VP, STR, F64, F64, F64, F64, I32, VP, VP, VP, VP, PI32, VP, VP, VP]),
    "xv_fgmm_acc_kernel_time": (ST, [VP, VP, VP, I32, VP, I32, I32, VP]),
    "xv_logprob_to_post": (ST, [c_int, VP, VP, I32, I32, VP, F32, I32, I32, I64, VP, VP, VP, PI64, PI64, VP]),
    "xv_logprob_to_post_kernel_time": (ST, [c_int, VP, I32, I32, STR, F32, I32, I32, VP]),
    "xv_fgmm_init_from_accs": (ST, [I32, I32, VP, VP, VP, I32, VP, VP, VP, VP, PI32, VP, PI32, VP]),
    "xv_dgmm_acc_create": (ST, [c_int, I32, I32, STR, PVP]),
    "xv_dgmm_acc_destroy": (None, [VP]),
    "xv_dgmm_acc_add": (ST, [VP, VP, I32, VP, VP, VP]),
    "xv_dgmm_acc_add_gselect": (ST, [VP, VP, VP, I32, VP, I32, VP, VP]),
    "xv_dgmm_acc_add_dense_post": (ST, [VP, VP, I32, VP]),
    "xv_dgmm_acc_add_dense": (ST, [VP, VP, VP, I32, VP]),
    "xv_dgmm_acc_get": (ST, [VP, VP, VP, VP]),
    "xv_dgmm_est": (ST, [I32, I32, STR, VP, VP, VP, STR, F64, F64, F64, I32, I32, F64, U64, VP, VP, VP, VP, PI32, VP, PI32, VP, VP, VP]),
    "xv_dgmm_acc_kernel_time": (ST, [VP, VP, VP, I32, VP, I32, I32, I32, VP]),
    "xv_ivex_create": (ST, [c_int, I32, I32, I32, VP, VP, VP, F64, PVP]),
    "xv_ivex_load": (ST, [c_int, STR, PVP]),
    "xv_ivex_destroy": (None, [VP]),
    "xv_ivex_info": (ST, [VP, PI32, PI32, PI32]),
    "xv_ivex_derived": (ST, [VP, VP, VP]),
    "xv_ivex_extract": (ST, [VP, VP, VP, I32, VP, VP, VP, F64, F64, VP, VP, VP, VP, VP, VP, VP]),
    "xv_ivex_read": (ST, [STR, PI32, PI32, PI32, VP, VP, VP, PF64]),
    "xv_ivex_write": (ST, [STR, I32, I32, I32, I32, VP, VP, VP, F64]),
    "xv_ivex_kernel_time": (ST, [VP, VP, VP, I32, VP, VP, VP, I32, VP]),
    "xv_ivex_acc_create": (ST, [VP, I32, I32, PVP]),
    "xv_ivex_acc_destroy": (None, [VP]),
    "xv_ivex_acc_add": (ST, [VP, VP, VP, I32, VP, VP, VP, VP]),
    "xv_ivex_acc_get": (ST, [VP, VP, VP, VP, VP, VP, VP, VP]),
    "xv_ivex_acc_pending": (ST, [VP, PI32, VP, VP, VP, VP]),
    "xv_ivex_acc_kernel_time": (ST, [VP, VP, VP, I32, VP, VP, VP, I32, VP]),
    "xv_ivex_rank_update": (ST, [c_int, VP, VP, VP, I32, I64, I64, I64, I64]),
    "xv_ivex_init": (ST, [I32, I32, VP, VP, VP, I32, U64, VP, VP, VP, PF64]),
    "xv_ivex_est": (ST, [I32, I32, I32, I32, VP, VP, VP, VP, VP, VP, VP, F64, F64, I32, I32, VP, VP, VP, PF64, VP, VP, VP]),
    "xv_ivex_stats_read": (ST, [STR, PI32, PI32, PI32, PI32, VP, VP, VP, VP, VP, VP, VP]),
    "xv_ivex_stats_write": (ST, [STR, I32, I32, I32, I32, I32, VP, VP, VP, VP, VP, VP, VP]),
    "xv_kernel_first_layer": (ST, [POINTER(FirstLayerDesc)]),
    "xv_kernel_prep_input": (ST, [POINTER(PrepInputDesc)]),
    "xv_kernel_pool_finalise": (ST, [POINTER(PoolFinaliseDesc)]),
    "xv_kernel_frame_output": (ST, [POINTER(FrameOutputDesc)]),
    "xv_bucket_sort": (ST, [I32, VP, I64, VP, I32, I32, VP, VP]),
}
ABI_SYMBOLS = list(SIGNATURES)

# The same for include/xvec_hip_asnorm.h, the companion header of score normalisation (tests/test_plda_dense_host.py holds this
# table to that header).
ASNORM_SIGNATURES = {
    "xv_plda_score_dense": (ST, [c_int, VP, VP, I32, VP, I32, I32, VP, VP, VP]),
    "xv_topn_stats": (ST, [c_int, VP, I64, I32, I32, VP, VP, VP]),
    "xv_plda_cohort_stats": (ST, [c_int, VP, VP, I32, VP, I32, I32, VP, I32, I32, VP, VP, VP]),
    "xv_plda_dense_plan": (ST, [I64, I64, I32, I64, PI64, PI64, PI64]),
}


class Nnet2Info(ctypes.Structure):
    """xv_nnet2_info_t (include/xvec_hip_nnet2.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("num_components", "num_updatable_components", "left_context", "right_context", "input_dim",
                                              "output_dim", "softmax_dim", "prior_dim", "num_layers", "max_plane_cols", "max_pre_cols",
                                              "halo")] + [("parameter_dim", ctypes.c_int64)]


# The same for include/xvec_hip_nnet2.h, the companion header of nnet-am-compute (tests/test_nnet2_abi_table.py holds this table to
# that header).
NNET2_SIGNATURES = {
    "xv_nnet2_open": (ST, [STR, PVP]),
    "xv_nnet2_close": (None, [VP]),
    "xv_nnet2_get_info": (ST, [VP, POINTER(Nnet2Info)]),
    "xv_nnet2_plan": (ST, [POINTER(Nnet2Info), I64, I64, I64, PI64, PI64, PI64]),
    "xv_nnet2_compute": (ST, [VP, c_int, VP, VP, I32, I32, I64, VP, PF32]),
    "xv_nnet2_compute_layers": (ST, [VP, c_int, VP, VP, I32, I32, I64, VP, VP]),
    "xv_nnet2_kernel_affine": (ST, [c_int, VP, I32, I32, VP, I32, VP, VP, I32, VP]),
    "xv_nnet2_kernel_row": (ST, [c_int, VP, I32, I32, I32, I32, I32, VP, VP]),
    "xv_nnet2_kernel_head": (ST, [c_int, VP, I32, I32, VP, I32, VP, I32, VP]),
}
COMPANION_SIGNATURES = dict(ASNORM_SIGNATURES, **NNET2_SIGNATURES)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    from . import LIB_PATH
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing - run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no Python/CPU fallback for the HIP path)" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (+ HSA runtime).  If torch is
    # going to be used in this process (tests, bench: device tensors / streams / torch.distributed) it must load
    # its runtime BEFORE libxvec_hip.so resolves the same soname, otherwise torch ends up on a mixed runtime and
    # reports "No HIP GPUs are available".  The command-line tools never load torch and use /opt/rocm's runtime.
    if os.environ.get("XVEC_NO_TORCH_PRELOAD", "") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(LIB_PATH)
    missing = [s for s in list(SIGNATURES) + list(COMPANION_SIGNATURES) if not hasattr(L, s)]
    if missing:
        raise ImportError("%s does not export: %s" % (LIB_PATH, missing))
    for name, (restype, argtypes) in list(SIGNATURES.items()) + list(COMPANION_SIGNATURES.items()):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = L
    return L


def _check(status):
    if status != XV_OK:
        raise XvError(status, lib().xv_last_error().decode(errors="replace"))


class _Handle:
    """Owner of one object of the library: _h is its handle, _destroy names the function that releases it."""
    _h = None
    _destroy = None

    def close(self):
        """Frees the object's device and host memory now (otherwise when the Python object is collected)."""
        if self._h and lib is not None:   # lib is None while the interpreter shuts down
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
