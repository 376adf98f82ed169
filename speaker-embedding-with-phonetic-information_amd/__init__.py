"""Host-side Python mirror of the C ABI in include/xvec_hip.h (ctypes; no torch types cross it).

The reference's interface for this path is a command line (Kaldi's `nnet3-xvector-compute`, call sites
egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:86-93); the product is the C++/HIP library
`libxvec_hip.so` plus the drop-in executables under bin/.  This module only exists so that tests/ and
bench.py can drive the same C ABI from Python; it contains no compute and no fallback: if the shared
library is missing or no gfx950 device is present, calls fail loudly.
"""
import ctypes
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# XVEC_LIB: an alternative build of the same library (kernel experiments: tools/ab_libs.sh); never set in production
LIB_PATH = os.environ.get("XVEC_LIB") or os.path.join(_HERE, "libxvec_hip.so")
BIN_DIR = os.path.join(_HERE, "bin")

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


# every symbol include/xvec_hip.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = [
    "xv_last_error", "xv_version", "xv_model_load", "xv_model_load_rxfilename", "xv_model_free", "xv_model_info",
    "xv_model_macs", "xv_model_describe", "xv_model_pack", "xv_ctx_create", "xv_ctx_create_from_blob",
    "xv_ctx_create_from_device_blob", "xv_ctx_free",
    "xv_ctx_info", "xv_forward_batch", "xv_forward_batch_device", "xv_ctx_synchronize", "xv_ctx_set_profiling",
    "xv_ctx_profile_report", "xv_extract_utterances", "xv_ctx_calibrate", "xv_ctx_set_fast_mode", "xv_ctx_fast_mode",
    "xv_calibrate_table", "xv_ctx_set_calibration", "xv_ctx_model_fingerprint", "xv_ctx_share_calibration",
    "xv_ctx_set_calibration_file", "xv_calibration_file_read", "xv_calibration_file_publish", "xv_recognize_feature_pipeline", "xv_ctx_set_lite_layers", "xv_ctx_lite_layers",
    "xv_extract_table", "xv_frontend_cmvn_select", "xv_plan_chunks", "xv_ctx_create_broadcast", "xv_kernel_tdnn_gemm",
    "xv_last_gemm_kernel", "xv_plan_gemm", "xv_plan_gemm_policy",
    "xv_backend_apply", "xv_segment_mean", "xv_scatter_stats", "xv_plda_transform", "xv_plda_score", "xv_lda_estimate",
    "xv_plda_estimate", "xv_plda_adapt",
    "xv_mfcc_options_default", "xv_mfcc_num_frames", "xv_mfcc_utt_seed", "xv_mfcc_compute", "xv_mfcc_compute_i16", "xv_mfcc_kernel_time", "xv_vad_energy",
    "xv_reverb_options_default", "xv_reverb_output_length", "xv_wav_reverberate", "xv_reverb_kernel_time", "xv_wave_write", "xv_recognize_wav_pipeline",
    "xv_compressed_size", "xv_compress_matrices", "xv_compress_kernel_time", "xv_cmvn_sliding",
    "xv_cmvn_stats", "xv_cmvn_norm", "xv_cmvn_apply", "xv_cmvn_apply_select", "xv_recognize_cmvn_pipeline", "xv_cmvn_kernel_time",
    "xv_add_deltas", "xv_ubm_diag_create", "xv_ubm_full_create", "xv_ubm_destroy", "xv_ubm_gselect", "xv_ubm_post",
    "xv_fgmm_to_gmm", "xv_fgmm_gconsts", "xv_ubm_kernel_time",
    "xv_ubm_full_gselect", "xv_ubm_frame_likes", "xv_vad_from_frame_likes", "xv_merge_vads",
    "xv_fgmm_acc_create", "xv_fgmm_acc_destroy", "xv_fgmm_acc_add", "xv_fgmm_acc_add_gselect", "xv_fgmm_acc_get", "xv_fgmm_est",
    "xv_fgmm_acc_kernel_time",
    "xv_logprob_to_post", "xv_logprob_to_post_kernel_time", "xv_fgmm_init_from_accs",
    "xv_dgmm_acc_create", "xv_dgmm_acc_destroy", "xv_dgmm_acc_add", "xv_dgmm_acc_add_gselect", "xv_dgmm_acc_add_dense_post",
    "xv_dgmm_acc_add_dense", "xv_dgmm_acc_get", "xv_dgmm_est", "xv_dgmm_acc_kernel_time",
    "xv_ivex_create", "xv_ivex_load", "xv_ivex_destroy", "xv_ivex_info", "xv_ivex_derived", "xv_ivex_extract", "xv_ivex_read",
    "xv_ivex_write", "xv_ivex_kernel_time",
    "xv_ivex_acc_create", "xv_ivex_acc_destroy", "xv_ivex_acc_add", "xv_ivex_acc_get", "xv_ivex_acc_pending", "xv_ivex_acc_kernel_time",
    "xv_ivex_rank_update", "xv_ivex_init", "xv_ivex_est", "xv_ivex_stats_read", "xv_ivex_stats_write",
    "xv_kernel_first_layer", "xv_kernel_prep_input", "xv_kernel_pool_finalise", "xv_kernel_frame_output", "xv_bucket_sort",
    "xv_wave_read", "xv_wave_free", "xv_pack_mx_residual", "xv_pack_mx_residual64", "xv_tile_mx_scales", "xv_pack_mx_weights", "xv_pack_mx_weights64",
]

_lib = None


def build(verbose=False):
    """Compile every HIP/C++ source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError("building libxvec_hip.so failed")
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
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
    L.xv_last_error.restype = ctypes.c_char_p
    L.xv_version.restype = ctypes.c_char_p
    L.xv_model_macs.restype = ctypes.c_double
    L.xv_model_macs.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    L.xv_model_describe.restype = ctypes.c_size_t
    L.xv_model_describe.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.xv_model_load.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p,
                                ctypes.POINTER(ctypes.c_void_p)]
    L.xv_model_load_rxfilename.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                           ctypes.POINTER(ctypes.c_void_p)]
    L.xv_model_free.argtypes = [ctypes.c_void_p]
    L.xv_model_free.restype = None
    L.xv_model_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ModelInfo)]
    L.xv_model_pack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    L.xv_ctx_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.xv_ctx_create_from_blob.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_void_p)]
    L.xv_ctx_create_from_device_blob.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_void_p)]
    L.xv_pack_mx_residual.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.xv_pack_mx_residual64.argtypes = L.xv_pack_mx_residual.argtypes
    L.xv_pack_mx_weights.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.xv_pack_mx_weights64.argtypes = L.xv_pack_mx_weights.argtypes
    L.xv_tile_mx_scales.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    L.xv_ctx_free.argtypes = [ctypes.c_void_p]
    L.xv_ctx_free.restype = None
    L.xv_ctx_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ModelInfo), ctypes.POINTER(ctypes.c_int32),
                              ctypes.POINTER(ctypes.c_int32)]
    L.xv_forward_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    L.xv_forward_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    L.xv_ctx_synchronize.argtypes = [ctypes.c_void_p]
    L.xv_ctx_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    L.xv_ctx_profile_report.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.xv_ctx_profile_report.restype = ctypes.c_size_t
    L.xv_extract_utterances.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.xv_ctx_create_broadcast.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_void_p)]
    L.xv_kernel_tdnn_gemm.argtypes = [ctypes.POINTER(GemmDesc)]
    L.xv_last_gemm_kernel.restype = ctypes.c_char_p
    L.xv_last_gemm_kernel.argtypes = []
    L.xv_kernel_first_layer.argtypes = [ctypes.POINTER(FirstLayerDesc)]
    L.xv_kernel_prep_input.argtypes = [ctypes.POINTER(PrepInputDesc)]
    L.xv_kernel_pool_finalise.argtypes = [ctypes.POINTER(PoolFinaliseDesc)]
    L.xv_kernel_frame_output.argtypes = [ctypes.POINTER(FrameOutputDesc)]
    L.xv_ctx_calibrate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_float,
                                   ctypes.POINTER(Calibration)]
    L.xv_ctx_set_fast_mode.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    L.xv_ctx_fast_mode.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    L.xv_ctx_set_lite_layers.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.xv_ctx_lite_layers.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    L.xv_calibrate_table.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_float, ctypes.POINTER(Calibration)]
    L.xv_ctx_set_calibration.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float]
    L.xv_ctx_model_fingerprint.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    L.xv_ctx_share_calibration.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_float, ctypes.c_char_p,
                                           ctypes.POINTER(ctypes.c_int32)]
    L.xv_ctx_set_calibration_file.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.xv_calibration_file_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    L.xv_calibration_file_publish.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float,
                                              ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    _lib = L
    return L


def _check(status):
    if status != XV_OK:
        raise XvError(status, lib().xv_last_error().decode(errors="replace"))


class Model:
    """Parsed nnet3 model lowered to a TDNN program (host only; works without a GPU)."""

    def __init__(self, raw=None, rxfilename=None, nnet_config=None, output_node=None):
        L = lib()
        self._h = ctypes.c_void_p()
        cfg = nnet_config.encode() if nnet_config else None
        node = output_node.encode() if output_node else None
        if raw is not None:
            buf = ctypes.create_string_buffer(bytes(raw), len(raw))
            _check(L.xv_model_load(buf, len(raw), cfg, node, ctypes.byref(self._h)))
        else:
            _check(L.xv_model_load_rxfilename(rxfilename.encode(), cfg, node, ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and lib is not None:   # lib is None while the interpreter shuts down
            lib().xv_model_free(self._h)
            self._h = ctypes.c_void_p()

    @property
    def info(self):
        mi = ModelInfo()
        _check(lib().xv_model_info(self._h, ctypes.byref(mi)))
        return mi

    def macs(self, frames):
        return lib().xv_model_macs(self._h, int(frames))

    def describe(self):
        n = lib().xv_model_describe(self._h, None, 0)
        buf = ctypes.create_string_buffer(n)
        lib().xv_model_describe(self._h, buf, n)
        return buf.value.decode()

    def pack(self, precision=PREC_DEFAULT):
        n = ctypes.c_size_t(0)
        _check(lib().xv_model_pack(self._h, precision, None, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        _check(lib().xv_model_pack(self._h, precision, buf, ctypes.byref(n)))
        return buf.raw[:n.value]


class Context:
    """Weights resident on one MI355X + workspaces.  Raises XvError(XV_ERR_DEVICE) without a gfx950 GPU."""

    def __init__(self, model=None, blob=None, device=0, precision=PREC_DEFAULT, device_blob=None):
        """device_blob = (device pointer as int, nbytes): the packed image already in this GPU's memory (e.g. the
        buffer a RCCL broadcast filled); the weights then never visit the host."""
        L = lib()
        self._h = ctypes.c_void_p()
        if device_blob is not None:
            _check(L.xv_ctx_create_from_device_blob(ctypes.c_void_p(int(device_blob[0])), int(device_blob[1]), device,
                                                    ctypes.byref(self._h)))
        elif blob is not None:
            self._blob = ctypes.create_string_buffer(bytes(blob), len(blob))
            _check(L.xv_ctx_create_from_blob(self._blob, len(blob), device, ctypes.byref(self._h)))
        else:
            _check(L.xv_ctx_create(model._h, device, precision, ctypes.byref(self._h)))
        mi = ModelInfo()
        p, d = ctypes.c_int32(), ctypes.c_int32()
        _check(L.xv_ctx_info(self._h, ctypes.byref(mi), ctypes.byref(p), ctypes.byref(d)))
        self.info, self.precision, self.device = mi, p.value, d.value

    def close(self):
        """Frees the context's device and pinned memory now (otherwise when the object is collected)."""
        if getattr(self, "_h", None) and self._h.value and lib is not None:
            lib().xv_ctx_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    def forward_batch(self, feats, row_offsets):
        """feats: float32 numpy [rows, input_dim]; row_offsets: int32 [B+1] -> numpy [B, output_dim]."""
        import numpy as np
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        offs = np.ascontiguousarray(row_offsets, dtype=np.int32)
        B = len(offs) - 1
        # segment-level models: one row per chunk; frame-level models: one row per input frame
        n_out = B if self.info.output_is_segment else int(offs[-1] - offs[0])
        out = np.empty((n_out, self.info.output_dim), dtype=np.float32)
        _check(lib().xv_forward_batch(self._h, feats.ctypes.data, offs.ctypes.data, B, out.ctypes.data))
        return out

    def forward_batch_device(self, feats_ptr, row_offsets, out_ptr, out_ld, stream=None):
        """Device pointers (ints); asynchronous on `stream` (a hipStream_t as int, None = context stream)."""
        import numpy as np
        offs = np.ascontiguousarray(row_offsets, dtype=np.int32)
        _check(lib().xv_forward_batch_device(self._h, feats_ptr, offs.ctypes.data, len(offs) - 1, out_ptr, out_ld,
                                             stream))

    def synchronize(self):
        _check(lib().xv_ctx_synchronize(self._h))

    def set_profiling(self, on):
        _check(lib().xv_ctx_set_profiling(self._h, 1 if on else 0))

    def profile_report(self):
        """[(label, launches, total_ms)] of everything recorded since the last call."""
        buf = ctypes.create_string_buffer(1 << 18)   # one call: reading the report resets it
        lib().xv_ctx_profile_report(self._h, buf, len(buf))
        rows = []
        for line in buf.value.decode().splitlines():
            label, calls, ms = line.split("\t")
            rows.append((label, int(calls), float(ms)))
        return rows

    def frontend(self, raw, raw_offsets, vad=None, cmn_window=300, center=True):
        """apply-cmvn-sliding (norm-vars=false) + select-voiced-frames on the device.  Returns (feats, offsets)."""
        import numpy as np
        raw = np.ascontiguousarray(raw, dtype=np.float32)
        offs = np.ascontiguousarray(raw_offsets, dtype=np.int32)
        n = len(offs) - 1
        out = np.empty_like(raw)
        out_off = np.zeros(n + 1, dtype=np.int32)
        v = None if vad is None else np.ascontiguousarray(vad, dtype=np.float32)
        L = lib()
        L.xv_frontend_cmvn_select.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_frontend_cmvn_select(self._h, raw.ctypes.data, offs.ctypes.data, n, None if v is None else v.ctypes.data,
                                         cmn_window, 1 if center else 0, out.ctypes.data, out_off.ctypes.data))
        return out[:out_off[-1]], out_off

    def extract_table(self, feature_rspecifier, vector_wspecifier, chunk_size=-1, min_chunk_size=100, pad_input=True,
                      batch_frames=0):
        """What one nnet3-xvector-compute process does, on this context.  Returns (done, failed)."""
        L = lib()
        L.xv_extract_table.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64)]
        done, failed = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(L.xv_extract_table(self._h, feature_rspecifier.encode(), vector_wspecifier.encode(), chunk_size,
                                  min_chunk_size, 1 if pad_input else 0, batch_frames, ctypes.byref(done),
                                  ctypes.byref(failed)))
        return done.value, failed.value

    def calibrate(self, feats, row_offsets, tol=7.5e-5):
        """xv_ctx_calibrate on host chunks: picks the fastest arithmetic whose embeddings stay within tol of the three-pass
        ones ON THESE CHUNKS and switches the context to it.  Returns {"chosen": name, "checked", "err_mx", "err_mx2"}."""
        import numpy as np
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        offs = np.ascontiguousarray(row_offsets, dtype=np.int32)
        c = Calibration()
        _check(lib().xv_ctx_calibrate(self._h, feats.ctypes.data, offs.ctypes.data, len(offs) - 1, tol, ctypes.byref(c)))
        return c.as_dict()

    def calibrate_table(self, feature_rspecifier, chunk_size=-1, min_chunk_size=100, pad_input=True, max_utts=64, tol=7.5e-5):
        """The same on the first chunk of the first max_utts utterances of a feature table."""
        c = Calibration()
        _check(lib().xv_calibrate_table(self._h, feature_rspecifier.encode(), chunk_size, min_chunk_size, 1 if pad_input else 0,
                                        max_utts, tol, ctypes.byref(c)))
        return c.as_dict()

    @property
    def fast_mode(self):
        """Name of the arithmetic the fast chunks run in right now (xv_ctx_fast_mode)."""
        p = ctypes.c_int32()
        _check(lib().xv_ctx_fast_mode(self._h, ctypes.byref(p)))
        return PRECISION_NAMES.get(p.value, str(p.value))

    def set_fast_mode(self, name):
        _check(lib().xv_ctx_set_fast_mode(self._h, PRECISIONS[name]))

    @property
    def lite_mask(self):
        """Layers (bit = index) that run the 1.25-pass arithmetic inside the fp16mx2 context (xv_ctx_lite_layers)."""
        m = ctypes.c_uint64()
        _check(lib().xv_ctx_lite_layers(self._h, ctypes.byref(m)))
        return int(m.value)

    def set_lite_mask(self, mask):
        _check(lib().xv_ctx_set_lite_layers(self._h, ctypes.c_uint64(int(mask))))

    def set_calibration(self, enable=True, tol=7.5e-5):
        """extract_table then calibrates on the head of its own table before the first batch."""
        _check(lib().xv_ctx_set_calibration(self._h, 1 if enable else 0, tol))

    @property
    def model_fingerprint(self):
        """Fingerprint of the packed model image this context runs (what a calibration file names)."""
        v = ctypes.c_uint64()
        _check(lib().xv_ctx_model_fingerprint(self._h, ctypes.byref(v)))
        return int(v.value)

    def share_calibration(self, path, tol=7.5e-5, note=None):
        """The shared choice of a recipe (xv_ctx_share_calibration): applies the file's choice when it exists, else publishes this
        context's current choice atomically and adopts what the file then holds.  Returns "read" / "published" / "adopted"."""
        out = ctypes.c_int32(-1)
        _check(lib().xv_ctx_share_calibration(self._h, os.fsencode(path), ctypes.c_float(tol), note.encode() if note else None,
                                              ctypes.byref(out)))
        return ("read", "published", "adopted")[out.value]

    def set_calibration_file(self, path):
        """extract_table applies / creates the shared calibration file before its first batch (None: off)."""
        _check(lib().xv_ctx_set_calibration_file(self._h, os.fsencode(path) if path else None))

    def extract_utterances(self, feats, row_offsets, chunk_size=-1, min_chunk_size=100, pad_input=True):
        import numpy as np
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        offs = np.ascontiguousarray(row_offsets, dtype=np.int32)
        n = len(offs) - 1
        out = np.zeros((n, self.info.output_dim), dtype=np.float32)
        ok = np.zeros(n, dtype=np.int32)
        _check(lib().xv_extract_utterances(self._h, feats.ctypes.data, offs.ctypes.data, n, chunk_size, min_chunk_size,
                                           1 if pad_input else 0, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)


class Watchdog:
    """Bounded wait for the start-up collective of a multi-rank job (the ONE broadcast of the packed weights, dist_extract.py /
    bench.py): a rank that never joins - died while loading, a link that is down - would otherwise leave the others inside
    the collective without a word until someone kills the job.  After `seconds` (XVEC_BCAST_TIMEOUT, default 120: the other
    ranks enter the broadcast while rank 0 still reads, lowers and packs the model - on a cold box that alone can take many seconds) the process
    prints what it was waiting for and EXITS with status 3; the launcher then tears the other ranks down.  A plain exit of a
    fresh-started process - nothing is re-executed (a process that has touched the GPU must never exec)."""

    def __init__(self, what, seconds=None):
        import threading
        if seconds is None:
            try:
                seconds = float(os.environ.get("XVEC_BCAST_TIMEOUT", "120"))
            except ValueError:
                seconds = 120.0
        self.what, self.seconds = what, seconds
        self._t = threading.Timer(seconds, self._fire)
        self._t.daemon = True
        self._t.start()

    def _fire(self):
        sys.stderr.write("ERROR (xvec_hip watchdog) rank %s: %s did not complete within %.0f s; exiting\n"
                         % (os.environ.get("RANK", "0"), self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def cancel(self):
        self._t.cancel()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.cancel()
        return False


def create_broadcast(model, devices, precision=PREC_DEFAULT):
    """xv_ctx_create_broadcast: one process, one context per listed GPU; the packed weights are uploaded to the first
    device and broadcast with ONE ncclBroadcast (RCCL), each context is built from the image its device received."""
    L = lib()
    n = len(devices)
    devs = (ctypes.c_int * n)(*devices)
    handles = (ctypes.c_void_p * n)()
    _check(L.xv_ctx_create_broadcast(model._h, devs, n, precision, handles))
    out = []
    for i in range(n):
        c = Context.__new__(Context)
        c._h = ctypes.c_void_p(handles[i])
        mi = ModelInfo()
        p, d = ctypes.c_int32(), ctypes.c_int32()
        _check(L.xv_ctx_info(c._h, ctypes.byref(mi), ctypes.byref(p), ctypes.byref(d)))
        c.info, c.precision, c.device = mi, p.value, d.value
        out.append(c)
    return out


def recognize_feature_pipeline(rspecifier):
    """The reference's feature pipeline as text (xv_recognize_feature_pipeline): {"feats", "vad", "cmn_window", "min_cmn_window",
    "center"} when the string is exactly `ark:apply-cmvn-sliding ... | select-voiced-frames ... |` with options the device
    front-end implements, else None."""
    L = lib()
    L.xv_recognize_feature_pipeline.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t,
                                                ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    found, w, mw, c = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    fb, vb = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    _check(L.xv_recognize_feature_pipeline(rspecifier.encode(), ctypes.byref(found), fb, 4096, vb, 4096, ctypes.byref(w), ctypes.byref(mw),
                                           ctypes.byref(c)))
    if not found.value:
        return None
    return {"feats": fb.value.decode(), "vad": vb.value.decode(), "cmn_window": w.value, "min_cmn_window": mw.value, "center": bool(c.value)}


def calibration_file_read(path):
    """The shared choice a calibration file holds: {"model": fingerprint, "precision": name, "lite_mask": int}, or None when the
    file does not exist (xv_calibration_file_read; XvError when it cannot be parsed)."""
    found, prec = ctypes.c_int32(0), ctypes.c_int32(-1)
    model, lite = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().xv_calibration_file_read(os.fsencode(path), ctypes.byref(found), ctypes.byref(model), ctypes.byref(prec),
                                          ctypes.byref(lite)))
    if not found.value:
        return None
    return {"model": int(model.value), "precision": PRECISION_NAMES.get(prec.value, str(prec.value)), "lite_mask": int(lite.value)}


def calibration_file_publish(path, model, precision, lite_mask=0, tol=7.5e-5, note=None):
    """Publishes a choice unless the file exists (atomic: the first of several concurrent publishers wins); returns
    (published, what the file holds afterwards)."""
    won, prec = ctypes.c_int32(0), ctypes.c_int32(-1)
    m, lite = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().xv_calibration_file_publish(os.fsencode(path), ctypes.c_uint64(model), PRECISIONS[precision], ctypes.c_uint64(lite_mask),
                                             ctypes.c_float(tol), note.encode() if note else None, ctypes.byref(won), ctypes.byref(m),
                                             ctypes.byref(prec), ctypes.byref(lite)))
    return bool(won.value), {"model": int(m.value), "precision": PRECISION_NAMES.get(prec.value, str(prec.value)),
                             "lite_mask": int(lite.value)}


def plan_chunks(num_rows, chunk_size, min_chunk_size, pad_input, min_net_frames, cap=4096):
    """[(start, len, left_pad, right_pad)] or None when the utterance counts as failed (host logic, no GPU)."""
    arr = [(ctypes.c_int32 * cap)() for _ in range(4)]
    n = ctypes.c_int32(0)
    L = lib()
    L.xv_plan_chunks.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    st = L.xv_plan_chunks(num_rows, chunk_size, min_chunk_size, 1 if pad_input else 0, min_net_frames, cap,
                          arr[0], arr[1], arr[2], arr[3], ctypes.byref(n))
    if st != XV_OK:
        return None
    return [(arr[0][i], arr[1][i], arr[2][i], arr[3][i]) for i in range(n.value)]


def backend_apply(x, mean=None, transform=None, normalize=False, scaleup=True, device=0, return_ratio=False):
    """Speaker-level back-end on the device: ivector-subtract-global-mean -> transform-vec -> ivector-normalize-length
    (egs/sre/v2/run_sre10.sh:238-241), each stage optional.  x: [n, dim] float32.  Returns [n, out_dim] (and the length
    ratios when asked)."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    mean_p = tr_p = None
    t_rows = t_cols = 0
    if mean is not None:
        mean = np.ascontiguousarray(mean, dtype=np.float32)
        if mean.shape != (dim,):
            raise XvError(XV_ERR_ARG, "mean has shape %s, vectors have dimension %d" % (mean.shape, dim))
        mean_p = mean.ctypes.data
    if transform is not None:
        transform = np.ascontiguousarray(transform, dtype=np.float32)
        t_rows, t_cols = transform.shape
        tr_p = transform.ctypes.data
    out = np.empty((n, t_rows if transform is not None else dim), dtype=np.float32)
    ratio = np.empty(n, dtype=np.float32)
    L = lib()
    L.xv_backend_apply.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_backend_apply(device, x.ctypes.data, n, dim, mean_p, tr_p, t_rows, t_cols, 1 if normalize else 0,
                              1 if scaleup else 0, out.ctypes.data, ratio.ctypes.data))
    return (out, ratio) if return_ratio else out


def segment_mean(x, segments, acc64=False, device=0):
    """ivector-mean on the device: row s of the result is the mean of x[segments[s]] (rows added in list order;
    fp32 accumulator like the per-speaker loop, fp64 with acc64=True like the global mean)."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    off = np.zeros(len(segments) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in segments])
    idx = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in segments]) if len(segments) else
                               np.zeros(0, np.int32), dtype=np.int32)
    out = np.empty((len(segments), dim), dtype=np.float32)
    L = lib()
    L.xv_segment_mean.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_segment_mean(device, x.ctypes.data, n, dim, off.ctypes.data, idx.ctypes.data if idx.size else None,
                             len(segments), 1 if acc64 else 0, out.ctypes.data))
    return out


def _segments(segments):
    import numpy as np
    off = np.zeros(len(segments) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in segments])
    idx = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in segments]) if len(segments) else
                               np.zeros(0, np.int32), dtype=np.int32)
    return off, idx


def scatter_stats(x, segments, device=0, return_ms=False):
    """Scatter statistics of the PLDA back-end on the device (fp64): segment s holds the rows x[segments[s]].  Returns
    (s_tot, sums, s_bet): sum of x_i x_i^T over every listed row [dim, dim], per-segment sums [n_seg, dim] and
    sum_s sums_s sums_s^T / n_s [dim, dim]; with return_ms also the kernel time."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    off, idx = _segments(segments)
    s_tot = np.empty((dim, dim)); s_bet = np.empty((dim, dim)); sums = np.empty((len(segments), dim))
    ms = ctypes.c_float(0)
    L = lib()
    L.xv_scatter_stats.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_scatter_stats(device, x.ctypes.data if n else None, n, dim, off.ctypes.data, idx.ctypes.data if idx.size else None,
                              len(segments), s_tot.ctypes.data, sums.ctypes.data if len(segments) else None, s_bet.ctypes.data,
                              ctypes.byref(ms)))
    return (s_tot, sums, s_bet, ms.value) if return_ms else (s_tot, sums, s_bet)


def plda_transform(x, transform, offset, psi, num=None, normalize=True, simple=False, device=0, return_ms=False):
    """Kaldi's Plda::TransformIvector on the device for every row of x [n, dim] (num: example count per row, default 1).
    Returns (y float32 [n, dim], scale float64 [n]) (and the kernel time with return_ms)."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    t = np.ascontiguousarray(transform, dtype=np.float64)
    off = np.ascontiguousarray(offset, dtype=np.float64)
    ps = np.ascontiguousarray(psi, dtype=np.float64)
    if t.shape != (dim, dim) or off.shape != (dim,) or ps.shape != (dim,):
        raise XvError(XV_ERR_ARG, "PLDA model shapes do not match the vectors' dimension %d" % dim)
    num = np.ascontiguousarray(np.ones(n) if num is None else num, dtype=np.float64)
    y = np.empty((n, dim), np.float32)
    scale = np.empty(n, np.float64)
    ms = ctypes.c_float(0)
    L = lib()
    L.xv_plda_transform.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 4 + \
        [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_plda_transform(device, x.ctypes.data, n, dim, t.ctypes.data, off.ctypes.data, ps.ctypes.data, num.ctypes.data,
                               1 if normalize else 0, 1 if simple else 0, y.ctypes.data, scale.ctypes.data, ctypes.byref(ms)))
    return (y, scale, ms.value) if return_ms else (y, scale)


def plda_score(u, num_u, v, psi, trials, device=0, return_ms=False):
    """Kaldi's Plda::LogLikelihoodRatio on the device: trials [m, 2] of (enrolment row of u, test row of v), u [n_u, dim]
    transformed enrolment vectors with example counts num_u, v [n_v, dim] transformed test vectors.  Returns float64 [m]."""
    import numpy as np
    u = np.ascontiguousarray(u, dtype=np.float32)
    v = np.ascontiguousarray(v, dtype=np.float32)
    num_u = np.ascontiguousarray(num_u, dtype=np.float64)
    ps = np.ascontiguousarray(psi, dtype=np.float64)
    tr = np.ascontiguousarray(np.asarray(trials, dtype=np.int32).reshape(-1, 2))
    dim = u.shape[1]
    scores = np.empty(len(tr), np.float64)
    ms = ctypes.c_float(0)
    L = lib()
    L.xv_plda_score.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_plda_score(device, u.ctypes.data, num_u.ctypes.data, u.shape[0], v.ctypes.data, v.shape[0], dim, ps.ctypes.data,
                           tr.ctypes.data if len(tr) else None, len(tr), scores.ctypes.data if len(tr) else None, ctypes.byref(ms)))
    return (scores, ms.value) if return_ms else scores


def lda_estimate(s_tot, s_bet, n, mean, lda_dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda's estimator on the host (no GPU needed) from the scatter statistics of n mean-subtracted
    vectors: the [lda_dim, dim + 1] float32 matrix [L | -L mean]."""
    import numpy as np
    s_tot = np.ascontiguousarray(s_tot, dtype=np.float64)
    s_bet = np.ascontiguousarray(s_bet, dtype=np.float64)
    mean = np.ascontiguousarray(mean, dtype=np.float32)
    dim = s_tot.shape[0]
    out = np.empty((lda_dim, dim + 1), np.float32)
    fl = ctypes.c_int32(0)
    L = lib()
    L.xv_lda_estimate.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_lda_estimate(dim, n, s_tot.ctypes.data, s_bet.ctypes.data, mean.ctypes.data, total_covariance_factor,
                             covariance_floor, lda_dim, out.ctypes.data if lda_dim > 0 else None, ctypes.byref(fl)))
    return out


def plda_estimate(sums, counts, s_tot, s_bet, num_em_iters=10):
    """ivector-compute-plda's EM on the host (no GPU needed) from per-speaker sums [n_spk, dim], counts [n_spk] and the
    scatter statistics of the same rows.  Returns (mean, transform, psi), float64."""
    import numpy as np
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    s_tot = np.ascontiguousarray(s_tot, dtype=np.float64)
    s_bet = np.ascontiguousarray(s_bet, dtype=np.float64)
    n_spk, dim = sums.shape
    mean = np.empty(dim); transform = np.empty((dim, dim)); psi = np.empty(dim)
    fl = ctypes.c_int32(0)
    L = lib()
    L.xv_plda_estimate.argtypes = [ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int32] + [ctypes.c_void_p] * 4
    _check(L.xv_plda_estimate(dim, n_spk, sums.ctypes.data, counts.ctypes.data, s_tot.ctypes.data, s_bet.ctypes.data, num_em_iters,
                              mean.ctypes.data, transform.ctypes.data, psi.ctypes.data, ctypes.byref(fl)))
    return mean, transform, psi


def plda_adapt(n, m, v, mean, transform, psi, mean_diff_scale=1.0, within_covar_scale=0.3, between_covar_scale=0.7):
    """ivector-adapt-plda's update on the host (no GPU needed) from the statistics of n unlabelled vectors, m = sum x [dim]
    and v = sum x x^T [dim, dim] (scatter_stats with one segment of every row: sums[0] and s_tot), and the model (mean,
    transform, psi).  Returns (mean, transform, psi, s), float64; s: the eigenvalues of the adaptation covariance in the
    space where the model's total covariance is I, descending."""
    import numpy as np
    m = np.ascontiguousarray(m, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    transform = np.ascontiguousarray(transform, dtype=np.float64)
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    dim = mean.shape[0]
    if m.shape != (dim,) or v.shape != (dim, dim) or transform.shape != (dim, dim) or psi.shape != (dim,):
        raise XvError(XV_ERR_ARG, "PLDA adaptation: statistics and model shapes do not agree on dimension %d" % dim)
    mean_out = np.empty(dim); transform_out = np.empty((dim, dim)); psi_out = np.empty(dim); s = np.empty(dim)
    L = lib()
    L.xv_plda_adapt.argtypes = [ctypes.c_int32, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_double] * 3 + \
        [ctypes.c_void_p] * 4
    _check(L.xv_plda_adapt(dim, int(n), m.ctypes.data, v.ctypes.data, mean.ctypes.data, transform.ctypes.data, psi.ctypes.data,
                           mean_diff_scale, within_covar_scale, between_covar_scale, mean_out.ctypes.data,
                           transform_out.ctypes.data, psi_out.ctypes.data, s.ctypes.data))
    return mean_out, transform_out, psi_out, s


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


WINDOW_TYPES = {"povey": 0, "hamming": 1, "hanning": 2, "rectangular": 3, "blackman": 4}
_MFCC_ALIASES = {"frame_length": "frame_length_ms", "frame_shift": "frame_shift_ms"}


def mfcc_options(**opts):
    """Kaldi's compute-mfcc-feats defaults (xv_mfcc_options_default) with overrides named like the command-line options
    (underscores for dashes): sample_frequency, frame_length, frame_shift, dither, preemphasis_coefficient, remove_dc_offset,
    window_type (a name), blackman_coeff, round_to_power_of_two, snip_edges, num_mel_bins, low_freq, high_freq, num_ceps,
    cepstral_lifter, use_energy, raw_energy, energy_floor."""
    L = lib()
    L.xv_mfcc_options_default.argtypes = [ctypes.POINTER(MfccOptions)]
    L.xv_mfcc_options_default.restype = None
    o = MfccOptions()
    L.xv_mfcc_options_default(ctypes.byref(o))
    names = {n for n, _ in MfccOptions._fields_}
    for k, v in opts.items():
        k = _MFCC_ALIASES.get(k, k)
        if k not in names:
            raise XvError(XV_ERR_ARG, "unknown MFCC option %r" % k)
        if k == "window_type" and isinstance(v, str):
            if v not in WINDOW_TYPES:
                raise XvError(XV_ERR_ARG, "Invalid window type %s" % v)
            v = WINDOW_TYPES[v]
        setattr(o, k, v)
    return o


def mfcc_num_frames(n_samples, **opts):
    """Frames Kaldi extracts from n_samples samples under these options (host only)."""
    L = lib()
    L.xv_mfcc_num_frames.argtypes = [ctypes.POINTER(MfccOptions), ctypes.c_int64]
    L.xv_mfcc_num_frames.restype = ctypes.c_int64
    o = opts["options"] if "options" in opts else mfcc_options(**opts)
    n = L.xv_mfcc_num_frames(ctypes.byref(o), int(n_samples))
    if n < 0:
        raise XvError(XV_ERR_ARG, L.xv_last_error().decode(errors="replace"))
    return int(n)


def utt_seed(key):
    """The 64-bit hash of an utterance key that keys the dither generator (xv_mfcc_utt_seed)."""
    L = lib()
    L.xv_mfcc_utt_seed.argtypes = [ctypes.c_char_p]
    L.xv_mfcc_utt_seed.restype = ctypes.c_uint64
    return int(L.xv_mfcc_utt_seed(key.encode()))


def mfcc(waves, keys=None, device=0, **opts):
    """MFCCs of a list of waveforms on the device (compute-mfcc-feats): waves are 1-d arrays in Kaldi's unscaled range, all
    int16 (converted on the device) or anything else (taken as float32).  keys name the utterances for the dither generator
    (default "0", "1", ...; unused with dither=0).  Returns a list of float32 [frames, num_ceps] arrays."""
    import numpy as np
    L = lib()
    o = opts.pop("options") if "options" in opts else mfcc_options(**opts)
    i16 = len(waves) > 0 and all(np.asarray(w).dtype == np.int16 for w in waves)
    dt = np.int16 if i16 else np.float32
    ws = [np.ascontiguousarray(w, dtype=dt).reshape(-1) for w in waves]
    off = np.zeros(len(ws) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(w) for w in ws])
    samples = np.concatenate(ws) if ws else np.zeros(0, dt)
    if samples.size == 0:
        samples = np.zeros(1, dt)
    if keys is None:
        keys = [str(i) for i in range(len(ws))]
    seeds = np.array([utt_seed(k) for k in keys], dtype=np.uint64)
    frames = [mfcc_num_frames(len(w), options=o) for w in ws]
    out = np.empty((max(1, sum(frames)), o.num_ceps), dtype=np.float32)
    row_off = np.zeros(len(ws) + 1, dtype=np.int32)
    fn = L.xv_mfcc_compute_i16 if i16 else L.xv_mfcc_compute
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(MfccOptions), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p]
    _check(fn(device, ctypes.byref(o), samples.ctypes.data, off.ctypes.data, len(ws), seeds.ctypes.data if len(ws) else None,
              out.ctypes.data, row_off.ctypes.data))
    assert list(np.diff(row_off)) == frames
    return [out[row_off[i]:row_off[i + 1]].copy() for i in range(len(ws))]


def vad(feats, device=0, vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_proportion_threshold=0.6, vad_frames_context=0):
    """Kaldi's energy VAD (compute-vad) on the device for a list of float32 [frames, dim] feature matrices (column 0 = log
    energy).  Returns a list of float32 [frames] arrays of 1.0 / 0.0."""
    import numpy as np
    L = lib()
    fs = [np.ascontiguousarray(f, dtype=np.float32) for f in feats]
    dim = fs[0].shape[1] if fs else 1
    if any(f.ndim != 2 or f.shape[1] != dim for f in fs):
        raise XvError(XV_ERR_ARG, "vad: every feature matrix must be [frames, %d]" % dim)
    off = np.zeros(len(fs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([f.shape[0] for f in fs])
    packed = np.concatenate(fs, axis=0) if fs else np.zeros((0, dim), np.float32)
    out = np.empty(max(1, int(off[-1])), dtype=np.float32)
    o = VadOptions(vad_energy_threshold, vad_energy_mean_scale, vad_proportion_threshold, vad_frames_context)
    L.xv_vad_energy.argtypes = [ctypes.c_int, ctypes.POINTER(VadOptions), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_vad_energy(device, ctypes.byref(o), packed.ctypes.data if packed.size else None, off.ctypes.data, len(fs), dim,
                           out.ctypes.data))
    return [out[off[i]:off[i + 1]].copy() for i in range(len(fs))]


def read_wave(rxfilename, channel=-1):
    """Reads a 16-bit PCM RIFF/WAVE from a file or a "cmd |" pipe the way compute-mfcc-feats does (xv_wave_read; host only).
    Returns (rate, int16 array of the chosen channel)."""
    import numpy as np
    L = lib()
    L.xv_wave_read.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(ctypes.POINTER(ctypes.c_int16)), ctypes.POINTER(ctypes.c_int64)]
    L.xv_wave_free.argtypes = [ctypes.POINTER(ctypes.c_int16)]
    L.xv_wave_free.restype = None
    rate, n = ctypes.c_int32(0), ctypes.c_int64(0)
    p = ctypes.POINTER(ctypes.c_int16)()
    _check(L.xv_wave_read(os.fsencode(rxfilename), channel, ctypes.byref(rate), ctypes.byref(p), ctypes.byref(n)))
    try:
        x = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int16)
    finally:
        L.xv_wave_free(p)
    return rate.value, x


def write_wave(wxfilename, samples, rate):
    """Writes a 1-d array as one channel of 16-bit PCM RIFF/WAVE to a file, "-" or "| cmd" (xv_wave_write; host only): values
    are truncated toward zero and saturated to the 16-bit range.  Returns how many were saturated."""
    import numpy as np
    L = lib()
    L.xv_wave_write.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    clipped = ctypes.c_int64(0)
    _check(L.xv_wave_write(os.fsencode(wxfilename), int(rate), x.ctypes.data if x.size else None, x.size, ctypes.byref(clipped)))
    return clipped.value


def recognize_cmvn_pipeline(rspecifier):
    """None, or the fields of the per-speaker feature pipeline nnet3-compute runs on the device instead of as commands
    (xv_recognize_cmvn_pipeline, csrc/fuse_pipe.h; host only): {"stats", "stats-is-table", "feats", "vad", "utt2spk", "norm-means",
    "norm-vars"}, all strings ("vad" / "utt2spk" empty when the string has none)."""
    L = lib()
    L.xv_recognize_cmvn_pipeline.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
    found = ctypes.c_int32(0)
    buf = ctypes.create_string_buffer(1 << 16)
    _check(L.xv_recognize_cmvn_pipeline(rspecifier.encode(), ctypes.byref(found), buf, len(buf)))
    if not found.value:
        return None
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def recognize_wav_pipeline(rxfilename):
    """None, or the fields of the wav-reverberate line compute-mfcc-feats would take over instead of running it
    (xv_recognize_wav_pipeline; host only): a dict of the "name=value" lines, e.g. "source", "impulse-response", "duration",
    "additive[0].rx", "additive[1].source"."""
    L = lib()
    L.xv_recognize_wav_pipeline.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
    found = ctypes.c_int32(0)
    buf = ctypes.create_string_buffer(1 << 16)
    _check(L.xv_recognize_wav_pipeline(rxfilename.encode(), ctypes.byref(found), buf, len(buf)))
    if not found.value:
        return None
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


class ReverbOptions(ctypes.Structure):
    """xv_reverb_options; reverb_options() gives Kaldi's defaults with keyword overrides."""
    _fields_ = [("shift_output", ctypes.c_int32), ("normalize_output", ctypes.c_int32), ("duration", ctypes.c_float),
                ("volume", ctypes.c_float), ("input_wave_channel", ctypes.c_int32), ("rir_channel", ctypes.c_int32),
                ("noise_channel", ctypes.c_int32)]


def reverb_options(**opts):
    """wav-reverberate's defaults (xv_reverb_options_default) with overrides named like the command-line options (underscores
    for dashes): shift_output, normalize_output, duration, volume, input_wave_channel, rir_channel, noise_channel."""
    L = lib()
    L.xv_reverb_options_default.argtypes = [ctypes.POINTER(ReverbOptions)]
    L.xv_reverb_options_default.restype = None
    o = ReverbOptions()
    L.xv_reverb_options_default(ctypes.byref(o))
    names = {n for n, _ in ReverbOptions._fields_}
    for k, v in opts.items():
        if k not in names:
            raise XvError(XV_ERR_ARG, "unknown wav-reverberate option %r" % k)
        setattr(o, k, v)
    return o


def reverb_output_length(n_samples, rir_len=0, rate=8000.0, **opts):
    """Samples wav-reverberate writes for an input of n_samples and a RIR of rir_len taps (0: none); host only."""
    L = lib()
    L.xv_reverb_output_length.argtypes = [ctypes.POINTER(ReverbOptions), ctypes.c_float, ctypes.c_int64, ctypes.c_int64]
    L.xv_reverb_output_length.restype = ctypes.c_int64
    o = opts["options"] if "options" in opts else reverb_options(**opts)
    return int(L.xv_reverb_output_length(ctypes.byref(o), float(rate), int(n_samples), int(rir_len)))


_REVERB_ARGTYPES = [ctypes.c_int, ctypes.POINTER(ReverbOptions), ctypes.c_float, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                    ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def _ragged(arrays, dtype):
    import numpy as np
    xs = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays]
    off = np.zeros(len(xs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in xs])
    flat = np.concatenate(xs) if xs else np.zeros(0, dtype)
    if flat.size == 0:
        flat = np.zeros(1, dtype)
    return flat, off


def reverberate(waves, rirs=None, additive=None, rate=8000.0, device=0, return_int16=False, kernel_time_reps=0, **opts):
    """wav-reverberate on the device for a list of waveforms (1-d arrays in the 16-bit range, all int16 or taken as float32).
    rirs: None, or one entry per waveform: None, an array (the impulse response as read from its file, not scaled), or an int
    index into `rir_list=` given among the options (utterances naming the same index share its spectra).  additive: None, or
    per waveform a list of (noise array, snr dB, start seconds).  Options are named like the command line's (shift_output,
    normalize_output, duration, volume).  Returns a list of float32 arrays (the signal before quantisation); with
    return_int16 a list of (float32, int16, clipped count).  kernel_time_reps > 0: returns the kernels' time in ms instead
    (xv_reverb_kernel_time)."""
    import numpy as np
    L = lib()
    rir_list = list(opts.pop("rir_list", []))
    o = opts.pop("options") if "options" in opts else reverb_options(**opts)
    i16 = len(waves) > 0 and all(np.asarray(w).dtype == np.int16 for w in waves)
    samples, off = _ragged(waves, np.int16 if i16 else np.float32)
    n = len(waves)
    utt_rir = np.full(max(1, n), -1, dtype=np.int32)
    if rirs is not None:
        if len(rirs) != n:
            raise XvError(XV_ERR_ARG, "reverberate: one RIR entry per waveform")
        for u, r in enumerate(rirs):
            if r is None:
                continue
            if isinstance(r, (int, np.integer)):
                utt_rir[u] = int(r)
            else:
                rir_list.append(r)
                utt_rir[u] = len(rir_list) - 1
    rir_flat, rir_off = _ragged(rir_list, np.float32)
    noise_list, add_noise, add_snr, add_start = [], [], [], []
    add_off = np.zeros(n + 1, dtype=np.int32)
    if additive is not None:
        if len(additive) != n:
            raise XvError(XV_ERR_ARG, "reverberate: one list of additive signals per waveform")
        for u, lst in enumerate(additive):
            for (x, snr, start) in (lst or []):
                noise_list.append(x)
                add_noise.append(len(noise_list) - 1)
                add_snr.append(snr)
                add_start.append(start)
            add_off[u + 1] = len(add_noise)
    noise_flat, noise_off = _ragged(noise_list, np.float32)
    add_noise = np.array(add_noise + [0], dtype=np.int32)
    add_snr = np.array(add_snr + [0], dtype=np.float32)
    add_start = np.array(add_start + [0], dtype=np.float32)
    lens = [reverb_output_length(off[u + 1] - off[u], rir_off[utt_rir[u] + 1] - rir_off[utt_rir[u]] if utt_rir[u] >= 0 else 0,
                                 rate, options=o) for u in range(n)]
    total = max(1, sum(max(0, x) for x in lens))
    common = (device, ctypes.byref(o), float(rate), samples.ctypes.data, 1 if i16 else 0, off.ctypes.data, n,
              rir_flat.ctypes.data, rir_off.ctypes.data, len(rir_list), utt_rir.ctypes.data,
              noise_flat.ctypes.data, noise_off.ctypes.data, len(noise_list), add_off.ctypes.data if additive is not None else None,
              add_noise.ctypes.data, add_snr.ctypes.data, add_start.ctypes.data)
    if kernel_time_reps > 0:
        L.xv_reverb_kernel_time.argtypes = _REVERB_ARGTYPES + [ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]
        ms = ctypes.c_float(0)
        _check(L.xv_reverb_kernel_time(*common, int(kernel_time_reps), ctypes.byref(ms)))
        return ms.value
    out = np.empty(total, dtype=np.float32)
    out16 = np.empty(total, dtype=np.int16) if return_int16 else None
    clipped = np.zeros(max(1, n), dtype=np.int64)
    out_off = np.zeros(n + 1, dtype=np.int64)
    L.xv_wav_reverberate.argtypes = _REVERB_ARGTYPES + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_wav_reverberate(*common, out_off.ctypes.data, out.ctypes.data, out16.ctypes.data if return_int16 else None,
                                clipped.ctypes.data))
    assert list(np.diff(out_off)) == [max(0, x) for x in lens]
    if return_int16:
        return [(out[out_off[u]:out_off[u + 1]].copy(), out16[out_off[u]:out_off[u + 1]].copy(), int(clipped[u])) for u in range(n)]
    return [out[out_off[u]:out_off[u + 1]].copy() for u in range(n)]


def _pack_matrices(mats, what):
    import numpy as np
    ms = [np.ascontiguousarray(m, dtype=np.float32) for m in mats]
    if any(m.ndim != 2 for m in ms):
        raise XvError(XV_ERR_ARG, "%s: every matrix must be two-dimensional" % what)
    widths = {m.shape[1] for m in ms if m.shape[0] > 0}
    if len(widths) > 1:
        raise XvError(XV_ERR_ARG, "%s: the matrices of one call share their column count" % what)
    cols = widths.pop() if widths else 0
    off = np.zeros(len(ms) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m.shape[0] if cols else 0 for m in ms])
    rows = [m for m in ms if m.shape[0] > 0 and cols]
    packed = np.concatenate(rows, axis=0) if rows else np.zeros((0, max(cols, 1)), np.float32)
    return np.ascontiguousarray(packed), off, cols


def compressed_size(rows, cols, method=1):
    """(bytes of the object that follows the token, "CM" / "CM2" / "CM3") of a rows x cols matrix: host only."""
    L = lib()
    n, fmt = ctypes.c_size_t(0), ctypes.c_char_p()
    L.xv_compressed_size.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.POINTER(ctypes.c_char_p)]
    _check(L.xv_compressed_size(rows, cols, method, ctypes.byref(n), ctypes.byref(fmt)))
    return int(n.value), fmt.value.decode()


def compress(mats, method=1, device=0, return_flags=False, kernel_time_reps=0):
    """Kaldi's compressed matrices (copy-feats --compress=true) of a list of float32 matrices that share their column count, on
    the device.  Returns a list of `bytes`, each what follows the "CM " / "CM2 " / "CM3 " token (compressed_size names the
    token); with return_flags also the list of flags that mark the matrices holding a value that is not finite, whose bytes
    mean nothing.  kernel_time_reps > 0: returns the kernels' time in ms instead (xv_compress_kernel_time)."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(mats, "compress")
    n = len(off) - 1
    common = [device, packed.ctypes.data if packed.size else None, off.ctypes.data, n, cols, method]
    types = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    if kernel_time_reps > 0:
        ms = ctypes.c_float(0)
        L.xv_compress_kernel_time.argtypes = types + [ctypes.c_int32, ctypes.POINTER(ctypes.c_float)]
        _check(L.xv_compress_kernel_time(*common, int(kernel_time_reps), ctypes.byref(ms)))
        return ms.value
    total = sum(compressed_size(int(off[u + 1] - off[u]), cols, method)[0] for u in range(n))
    out = np.zeros(max(1, total), dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int64)
    flags = np.zeros(max(1, n), dtype=np.int32)
    L.xv_compress_matrices.argtypes = types + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_compress_matrices(*common, out.ctypes.data, out_off.ctypes.data, flags.ctypes.data))
    assert int(out_off[n]) == total
    objs = [out[out_off[u]:out_off[u + 1]].tobytes() for u in range(n)]
    return (objs, [bool(f) for f in flags[:n]]) if return_flags else objs


def cmvn_sliding(mats, cmn_window=600, min_cmn_window=100, center=False, device=0):
    """apply-cmvn-sliding --norm-vars=false on the device, without a model: a list of float32 [frames, dim] matrices in, the
    same shapes out (the kernels of Context.frontend with every frame kept)."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(mats, "cmvn_sliding")
    n = len(off) - 1
    out = np.empty_like(packed)
    L.xv_cmvn_sliding.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                  ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_cmvn_sliding(device, packed.ctypes.data if packed.size else None, off.ctypes.data, n, max(cols, 1), cmn_window,
                             min_cmn_window, 1 if center else 0, out.ctypes.data if out.size else None))
    return [out[off[u]:off[u + 1]].copy() for u in range(n)]


def cmvn_stats(feats_list, device=0, kernel_time_reps=0):
    """Kaldi's CMVN statistics (compute-cmvn-stats) of a list of float32 [frames, cols] matrices that share their column count, summed
    on the device in fp64: a float64 array [n][2][cols + 1] - row 0 the column sums and the frame count, row 1 the sums of squares and
    0.  A matrix's statistics do not depend on the batch it is in.  kernel_time_reps > 0: (stats_ms, apply_ms) of xv_cmvn_kernel_time."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(feats_list, "cmvn_stats")
    n = len(off) - 1
    if cols < 1:
        raise XvError(XV_ERR_ARG, "cmvn_stats: no matrix with rows and columns")
    if kernel_time_reps > 0:
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        L.xv_cmvn_kernel_time.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        _check(L.xv_cmvn_kernel_time(device, packed.ctypes.data, off.ctypes.data, n, cols, int(kernel_time_reps), ctypes.byref(a),
                                     ctypes.byref(b)))
        return a.value, b.value
    stats = np.zeros((n, 2, cols + 1), dtype=np.float64)
    L.xv_cmvn_stats.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                ctypes.c_void_p]
    _check(L.xv_cmvn_stats(device, packed.ctypes.data if packed.size else None, off.ctypes.data, n, cols, stats.ctypes.data, None))
    return stats


def cmvn_norm(stats, norm_means=True, norm_vars=False, reverse=False, skip_dims=(), return_floored=False):
    """One [2][cols + 1] statistics matrix -> float32 [2][cols]: row 0 the offset, row 1 the scale of out = x * scale + offset
    (xv_cmvn_norm: fp64 arithmetic, host only)."""
    import numpy as np
    L = lib()
    st = np.ascontiguousarray(stats, dtype=np.float64)
    if st.ndim != 2 or st.shape[0] != 2 or st.shape[1] < 2:
        raise XvError(XV_ERR_ARG, "cmvn_norm: the statistics are a [2][cols + 1] matrix")
    cols = st.shape[1] - 1
    skip = np.ascontiguousarray(list(skip_dims), dtype=np.int32)
    norm = np.zeros((2, cols), dtype=np.float32)
    floored = ctypes.c_int32(0)
    L.xv_cmvn_norm.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                               ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    _check(L.xv_cmvn_norm(st.ctypes.data, cols, int(bool(norm_means)), int(bool(norm_vars)), int(bool(reverse)),
                          skip.ctypes.data if skip.size else None, int(skip.size), norm.ctypes.data, ctypes.byref(floored)))
    return (norm, int(floored.value)) if return_floored else norm


def apply_cmvn(feats_list, norms, utt_norm, device=0):
    """out = x * scale + offset on the device (apply-cmvn): matrix u of feats_list takes norms[utt_norm[u]] ([2][cols] each, as cmvn_norm
    returns them).  fp32, the product and the sum each rounded on their own.  Returns the list of normalised matrices."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(feats_list, "apply_cmvn")
    n = len(off) - 1
    nm = np.ascontiguousarray(norms, dtype=np.float32)
    un = np.ascontiguousarray(utt_norm, dtype=np.int32)
    if un.shape != (n,) or nm.ndim != 3 or nm.shape[1:] != (2, max(cols, 1)) or (n and (un.min() < 0 or un.max() >= nm.shape[0])):
        raise XvError(XV_ERR_ARG, "apply_cmvn: norms are [n_norms][2][cols] and utt_norm names one of them per matrix")
    out = np.empty_like(packed)
    L.xv_cmvn_apply.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_cmvn_apply(device, packed.ctypes.data if packed.size else None, off.ctypes.data, n, max(cols, 1), nm.ctypes.data,
                           un.ctypes.data, out.ctypes.data if out.size else None))
    return [out[off[u]:off[u + 1]].copy() for u in range(n)]


def apply_cmvn_select(feats_list, norms, utt_norm, sel_row, sel_utt, device=0):
    """The same map behind a row selection, as one launch (xv_cmvn_apply_select): row i of the result is row sel_row[i] of the
    packed matrices (an absolute row, inside matrix sel_utt[i]) times the scale plus the offset of norms[utt_norm[sel_utt[i]]].  A
    matrix without a selected row may have utt_norm -1.  Returns one float32 [len(sel_row), cols] matrix."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(feats_list, "apply_cmvn_select")
    n = len(off) - 1
    cols = max(cols, 1)
    nm = np.ascontiguousarray(norms, dtype=np.float32)
    un = np.ascontiguousarray(utt_norm, dtype=np.int32)
    sr = np.ascontiguousarray(sel_row, dtype=np.int32)
    su = np.ascontiguousarray(sel_utt, dtype=np.int32)
    if un.shape != (n,) or nm.ndim != 3 or nm.shape[1:] != (2, cols) or sr.ndim != 1 or sr.shape != su.shape:
        raise XvError(XV_ERR_ARG, "apply_cmvn_select: norms are [n_norms][2][cols], utt_norm has one entry per matrix, sel_row and sel_utt one per kept row")
    out = np.empty((sr.size, cols), dtype=np.float32)
    L.xv_cmvn_apply_select.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                       ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_cmvn_apply_select(device, packed.ctypes.data if packed.size else None, off.ctypes.data, n, cols,
                                  nm.ctypes.data if nm.size else None, int(nm.shape[0]), un.ctypes.data if un.size else None,
                                  sr.ctypes.data if sr.size else None, su.ctypes.data if su.size else None, int(sr.size),
                                  out.ctypes.data if out.size else None))
    return out


def add_deltas(feats_list, order=2, window=2, truncate=0, device=0):
    """add-deltas on the device: a list of float32 [frames, cols] matrices that share their column count in, the matrices of
    (order + 1) * (truncate or cols) columns out.  fp32, every product and every sum rounded on its own (csrc/ubm.h)."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(feats_list, "add_deltas")
    n = len(off) - 1
    if cols < 1:
        raise XvError(XV_ERR_ARG, "add_deltas: no matrix with rows and columns")
    oc = (order + 1) * (truncate if truncate > 0 else cols)
    out = np.zeros((packed.shape[0], max(oc, 1)), dtype=np.float32)
    L.xv_add_deltas.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_add_deltas(device, packed.ctypes.data, off.ctypes.data, n, cols, order, window, truncate, out.ctypes.data, None))
    return [out[off[u]:off[u + 1]].copy() for u in range(n)]


def fgmm_to_gmm(weights, means_invcovars, inv_covars):
    """fgmm-global-to-gmm on the host in fp64: weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2] (packed lower
    triangles) -> (gconsts [G], means_invvars [G][D], inv_vars [G][D]) of the diagonal image."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    b = np.ascontiguousarray(means_invcovars, dtype=np.float32)
    ic = np.ascontiguousarray(inv_covars, dtype=np.float32)
    if b.ndim != 2 or w.shape != (b.shape[0],) or ic.shape != (b.shape[0], b.shape[1] * (b.shape[1] + 1) // 2):
        raise XvError(XV_ERR_ARG, "fgmm_to_gmm: weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2]")
    g, d = b.shape
    gc, mi, iv = np.zeros(g, np.float32), np.zeros((g, d), np.float32), np.zeros((g, d), np.float32)
    L.xv_fgmm_to_gmm.argtypes = [ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 6
    _check(L.xv_fgmm_to_gmm(g, d, w.ctypes.data, b.ctypes.data, ic.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data))
    return gc, mi, iv


def fgmm_gconsts(weights, means_invcovars, inv_covars):
    """The gconsts the tools recompute after they read a full model (xv_fgmm_gconsts: fp64 on the host, stored as float32)."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    b = np.ascontiguousarray(means_invcovars, dtype=np.float32)
    ic = np.ascontiguousarray(inv_covars, dtype=np.float32)
    if b.ndim != 2 or w.shape != (b.shape[0],) or ic.shape != (b.shape[0], b.shape[1] * (b.shape[1] + 1) // 2):
        raise XvError(XV_ERR_ARG, "fgmm_gconsts: weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2]")
    gc = np.zeros(b.shape[0], np.float32)
    L.xv_fgmm_gconsts.argtypes = [ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 5
    _check(L.xv_fgmm_gconsts(b.shape[0], b.shape[1], w.ctypes.data, b.ctypes.data, ic.ctypes.data, gc.ctypes.data, None))
    return gc


class Ubm:
    """A GMM on one device, uploaded once (xv_ubm_diag_create / xv_ubm_full_create).  Ubm.diag(gconsts, means_invvars, inv_vars)
    selects Gaussians; Ubm.full(gconsts, means_invcovars, inv_covars_packed) turns a selection into posteriors."""

    def __init__(self, handle, num_gauss, dim, full):
        self._h, self.num_gauss, self.dim, self.is_full = handle, num_gauss, dim, full

    @classmethod
    def _create(cls, fn_name, device, gconsts, a, b, full):
        import numpy as np
        L = lib()
        gc = np.ascontiguousarray(gconsts, dtype=np.float32)
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if a.ndim != 2 or gc.shape != (a.shape[0],):
            raise XvError(XV_ERR_ARG, "Ubm: gconsts [G] and a [G][D] matrix")
        g, d = a.shape
        if b.shape != ((g, d * (d + 1) // 2) if full else (g, d)):
            raise XvError(XV_ERR_ARG, "Ubm: the second matrix does not have the model's shape")
        fn = getattr(L, fn_name)
        fn.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.POINTER(ctypes.c_void_p)]
        h = ctypes.c_void_p()
        _check(fn(device, g, d, gc.ctypes.data, a.ctypes.data, b.ctypes.data, ctypes.byref(h)))
        return cls(h, g, d, full)

    @classmethod
    def diag(cls, gconsts, means_invvars, inv_vars, device=0):
        return cls._create("xv_ubm_diag_create", device, gconsts, means_invvars, inv_vars, False)

    @classmethod
    def full(cls, gconsts, means_invcovars, inv_covars, device=0):
        return cls._create("xv_ubm_full_create", device, gconsts, means_invcovars, inv_covars, True)

    def close(self):
        if self._h:
            L = lib()
            L.xv_ubm_destroy.argtypes = [ctypes.c_void_p]
            L.xv_ubm_destroy.restype = None
            L.xv_ubm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gselect(self, feats_list, n, return_loglikes=False):
        """The n best Gaussians per frame, best first: a list of int32 [frames, n] (and of float32 log-likelihoods)."""
        import numpy as np
        L = lib()
        packed, off, cols = _pack_matrices(feats_list, "gselect")
        if cols != self.dim:
            raise XvError(XV_ERR_ARG, "gselect: the features have %d columns, the model %d" % (cols, self.dim))
        nu, rows = len(off) - 1, packed.shape[0]
        idx = np.zeros((rows, max(n, 1)), dtype=np.int32)
        ll = np.zeros((rows, max(n, 1)), dtype=np.float32)
        L.xv_ubm_gselect.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_ubm_gselect(self._h, packed.ctypes.data, off.ctypes.data, nu, n, idx.ctypes.data,
                                ll.ctypes.data if return_loglikes else None, None))
        sel = [idx[off[u]:off[u + 1]].copy() for u in range(nu)]
        return (sel, [ll[off[u]:off[u + 1]].copy() for u in range(nu)]) if return_loglikes else sel

    def post(self, feats_list, gselect_list, min_post=0.0, return_details=False):
        """Posteriors over the selected Gaussians: per utterance a list (one entry per frame) of (int32 indices, float32
        posteriors).  return_details: also the lists of log-likelihoods [frames, n] and of per-frame log-sums [frames]."""
        import numpy as np
        L = lib()
        packed, off, cols = _pack_matrices(feats_list, "post")
        if cols != self.dim:
            raise XvError(XV_ERR_ARG, "post: the features have %d columns, the model %d" % (cols, self.dim))
        gs = [np.ascontiguousarray(g, dtype=np.int32) for g in gselect_list]
        nu, rows = len(off) - 1, packed.shape[0]
        if nu == 0 or len(gs) != nu or any(g.ndim != 2 or g.shape[0] != off[u + 1] - off[u] or g.shape[1] != gs[0].shape[1] for u, g in enumerate(gs)):
            raise XvError(XV_ERR_ARG, "post: one [frames, n] selection per utterance, all of one n")
        n = gs[0].shape[1]
        sel = np.ascontiguousarray(np.concatenate(gs, axis=0))
        count = np.zeros(rows, dtype=np.int32)
        idx = np.zeros((rows, n), dtype=np.int32)
        post = np.zeros((rows, n), dtype=np.float32)
        ll = np.zeros((rows, n), dtype=np.float32)
        logsum = np.zeros(rows, dtype=np.float32)
        L.xv_ubm_post.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                  ctypes.c_float] + [ctypes.c_void_p] * 6
        _check(L.xv_ubm_post(self._h, packed.ctypes.data, off.ctypes.data, nu, sel.ctypes.data, n, float(min_post), count.ctypes.data,
                             idx.ctypes.data, post.ctypes.data, ll.ctypes.data, logsum.ctypes.data, None))
        out = [[(idx[t, :count[t]].copy(), post[t, :count[t]].copy()) for t in range(off[u], off[u + 1])] for u in range(nu)]
        if not return_details:
            return out
        return out, [ll[off[u]:off[u + 1]].copy() for u in range(nu)], [logsum[off[u]:off[u + 1]].copy() for u in range(nu)]

    def _selection(self, who, feats_list, gselect_list):
        import numpy as np
        packed, off, cols = _pack_matrices(feats_list, who)
        if cols != self.dim:
            raise XvError(XV_ERR_ARG, "%s: the features have %d columns, the model %d" % (who, cols, self.dim))
        nu = len(off) - 1
        if gselect_list is None:
            return packed, off, nu, None, 0
        gs = [np.ascontiguousarray(g, dtype=np.int32) for g in gselect_list]
        if nu == 0 or len(gs) != nu or any(g.ndim != 2 or g.shape[0] != off[u + 1] - off[u] or g.shape[1] != gs[0].shape[1] for u, g in enumerate(gs)):
            raise XvError(XV_ERR_ARG, "%s: one [frames, n] selection per utterance, all of one n" % who)
        return packed, off, nu, np.ascontiguousarray(np.concatenate(gs, axis=0)), gs[0].shape[1]

    def rerank(self, feats_list, gselect_list, n, return_loglikes=False, return_ms=False):
        """Second-stage selection by a full model (fgmm-gselect --gselect=): the min(n, n_in) best of every frame's preselection,
        best first, as a list of int32 [frames, min(n, n_in)] (and of the float32 log-likelihoods; return_ms: and the device
        times {sort, scores, rerank} in ms)."""
        import numpy as np
        L = lib()
        packed, off, nu, sel, n_in = self._selection("rerank", feats_list, gselect_list)
        if sel is None:
            raise XvError(XV_ERR_ARG, "rerank: a preselection is needed")
        keep = max(1, min(n, n_in))
        rows = packed.shape[0]
        idx = np.zeros((rows, keep), dtype=np.int32)
        ll = np.zeros((rows, keep), dtype=np.float32)
        ms = (ctypes.c_float * 3)()
        L.xv_ubm_full_gselect.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_ubm_full_gselect(self._h, packed.ctypes.data, off.ctypes.data, nu, sel.ctypes.data, n_in, n, idx.ctypes.data,
                                     ll.ctypes.data if return_loglikes else None, ms if return_ms else None))
        out = [[idx[off[u]:off[u + 1]].copy() for u in range(nu)]]
        if return_loglikes:
            out.append([ll[off[u]:off[u + 1]].copy() for u in range(nu)])
        if return_ms:
            out.append(dict(zip(("sort", "full", "rerank"), [float(x) for x in ms])))
        return out[0] if len(out) == 1 else tuple(out)

    def frame_likes(self, feats_list, gselect_list=None, average=False):
        """Per-frame log-likelihoods of a full model over each frame's selection (fgmm-global-get-frame-likes): a list of float32
        [frames].  gselect_list None: every component, for models of at most 64.  average: one float32 per utterance instead, the
        frames summed in float64 in frame order, divided by their number and rounded once."""
        import numpy as np
        L = lib()
        packed, off, nu, sel, n = self._selection("frame_likes", feats_list, gselect_list)
        likes = np.zeros(packed.shape[0], dtype=np.float32)
        L.xv_ubm_frame_likes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_ubm_frame_likes(self._h, packed.ctypes.data, off.ctypes.data, nu, None if sel is None else sel.ctypes.data, n,
                                    likes.ctypes.data, None))
        per_utt = [likes[off[u]:off[u + 1]].copy() for u in range(nu)]
        if not average:
            return per_utt
        out = []
        for v in per_utt:
            tot = 0.0
            for x in v.tolist():
                tot += x
            out.append(np.float32(tot / len(v)) if len(v) else np.float32(0.0))
        return out


def vad_from_frame_likes(likes, priors=None, map=None):
    """compute-vad-from-frame-likes on the host: likes is one float32 [frames] array per class; frame t gets the first class j that
    maximises likes[j][t] + log(priors[j]) (map[j] when a map, a sequence of one label per class, is given), as float32."""
    import numpy as np
    L = lib()
    cls = [np.ascontiguousarray(v, dtype=np.float32) for v in likes]
    if not cls or any(v.ndim != 1 or v.shape != cls[0].shape for v in cls):
        raise XvError(XV_ERR_ARG, "vad_from_frame_likes: one [frames] array per class, all of one length")
    n = len(cls)
    pr = None if priors is None else np.ascontiguousarray(priors, dtype=np.float32)
    mp = None if map is None else np.ascontiguousarray(map, dtype=np.int32)
    if (pr is not None and pr.shape != (n,)) or (mp is not None and mp.shape != (n,)):
        raise XvError(XV_ERR_ARG, "vad_from_frame_likes: %d classes need %d priors and %d map entries" % (n, n, n))
    ptrs = (ctypes.c_void_p * n)(*[v.ctypes.data for v in cls])
    out = np.zeros(cls[0].shape[0], dtype=np.float32)
    L.xv_vad_from_frame_likes.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_vad_from_frame_likes(n, ptrs, out.shape[0], None if pr is None else pr.ctypes.data, None if mp is None else mp.ctypes.data,
                                     out.ctypes.data))
    return out


def merge_vads(a, b, map=None):
    """merge-vads on the host: 1 where both are 1 without a map; with a map, a sequence of (a, b, c) triples, the pair (a, b)
    gives c and a pair that is not in the map is an error that names it."""
    import numpy as np
    L = lib()
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.ndim != 1 or a.shape != b.shape:
        raise XvError(XV_ERR_ARG, "merge_vads: two [frames] arrays of one length")
    tri = np.zeros((0, 3), dtype=np.int32) if map is None else np.ascontiguousarray(map, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(a.shape[0], dtype=np.float32)
    L.xv_merge_vads.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_merge_vads(a.ctypes.data, b.ctypes.data, a.shape[0], tri.ctypes.data if len(tri) else None, len(tri), out.ctypes.data))
    return out


def ubm_kernel_time(diag, full, feats_list, n=20, min_post=0.025, reps=5):
    """{deltas, gselect, sort, full, softmax} kernel times in ms of one batch (xv_ubm_kernel_time: the best of reps)."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(feats_list, "ubm_kernel_time")
    ms = (ctypes.c_float * 5)()
    L.xv_ubm_kernel_time.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_float, ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_ubm_kernel_time(diag._h, full._h, packed.ctypes.data, off.ctypes.data, len(off) - 1, n, float(min_post), reps, ms))
    return dict(zip(("deltas", "gselect", "sort", "full", "softmax"), [float(x) for x in ms]))


class FgmmAccumulator:
    """The fp64 accumulators of full-covariance UBM training on one device (xv_fgmm_acc_create): occ [G], mean [G][D] and the packed
    lower triangles cov [G][D (D + 1) / 2].  flags: letters of "mvw" (v implies m, m implies w)."""

    def __init__(self, num_gauss, dim, flags="mvw", device=0):
        L = lib()
        self._h = ctypes.c_void_p()
        self.num_gauss, self.dim, self.flags = int(num_gauss), int(dim), flags
        L.xv_fgmm_acc_create.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _check(L.xv_fgmm_acc_create(device, self.num_gauss, self.dim, flags.encode(), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            L = lib()
            L.xv_fgmm_acc_destroy.argtypes = [ctypes.c_void_p]
            L.xv_fgmm_acc_destroy.restype = None
            L.xv_fgmm_acc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _feats(self, feats, who):
        import numpy as np
        x = np.ascontiguousarray(feats, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise XvError(XV_ERR_ARG, "%s: the features are not [frames, %d]" % (who, self.dim))
        return x

    def accumulate(self, feats, post):
        """One call: feats [frames, D]; post: per frame (indices, posteriors), as Ubm.post returns them for one utterance."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "accumulate")
        if len(post) != x.shape[0]:
            raise XvError(XV_ERR_ARG, "accumulate: one (indices, posteriors) pair per frame")
        off = np.zeros(x.shape[0] + 1, dtype=np.int32)
        for t, (i, _) in enumerate(post):
            off[t + 1] = off[t] + len(i)
        idx = np.ascontiguousarray(np.concatenate([np.asarray(i, np.int32) for i, _ in post]) if len(post) else np.zeros(0), dtype=np.int32)
        w = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32) for _, p in post]) if len(post) else np.zeros(0), dtype=np.float32)
        L.xv_fgmm_acc_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_fgmm_acc_add(self._h, x.ctypes.data, x.shape[0], off.ctypes.data, idx.ctypes.data, w.ctypes.data))

    def accumulate_gselect(self, full, feats, gselect):
        """The fused E-step: the posteriors of full.post(min_post=0) over gselect [frames, n] never leave the device.  Returns the
        per-frame log-sums, float32 [frames]."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "accumulate_gselect")
        gs = np.ascontiguousarray(gselect, dtype=np.int32)
        if gs.ndim != 2 or gs.shape[0] != x.shape[0]:
            raise XvError(XV_ERR_ARG, "accumulate_gselect: a [frames, n] selection")
        logsum = np.zeros(x.shape[0], dtype=np.float32)
        L.xv_fgmm_acc_add_gselect.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.c_void_p]
        _check(L.xv_fgmm_acc_add_gselect(self._h, full._h, x.ctypes.data, x.shape[0], gs.ctypes.data, gs.shape[1], logsum.ctypes.data))
        return logsum

    def get(self):
        """(occ [G], mean [G, D], cov [G, D (D + 1) / 2]) as float64."""
        import numpy as np
        L = lib()
        g, d = self.num_gauss, self.dim
        occ, mean, cov = np.zeros(g), np.zeros((g, d)), np.zeros((g, d * (d + 1) // 2))
        L.xv_fgmm_acc_get.argtypes = [ctypes.c_void_p] * 4
        _check(L.xv_fgmm_acc_get(self._h, occ.ctypes.data, mean.ctypes.data, cov.ctypes.data))
        return occ, mean, cov

    def kernel_time(self, full, feats, gselect, reps=5):
        """{sort, full, softmax, acc} kernel times in ms of one fused call (xv_fgmm_acc_kernel_time: the best of reps).  Every run adds
        to the accumulators."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "kernel_time")
        gs = np.ascontiguousarray(gselect, dtype=np.int32)
        ms = (ctypes.c_float * 4)()
        L.xv_fgmm_acc_kernel_time.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_void_p]
        _check(L.xv_fgmm_acc_kernel_time(self._h, full._h, x.ctypes.data, x.shape[0], gs.ctypes.data, gs.shape[1], reps, ms))
        return dict(zip(("sort", "full", "softmax", "acc"), [float(v) for v in ms]))


def fgmm_est(weights, means_invcovars, inv_covars, occ, mean, cov, acc_flags="mvw", update_flags="mvw", min_gaussian_weight=1e-5,
             min_gaussian_occupancy=100.0, variance_floor=0.001, max_condition=1e5, remove_low_count_gaussians=True):
    """The M-step of fgmm-global-est on host arrays (xv_fgmm_est, fp64): dict(weights, means_invcovars, inv_covars, gconsts) of the
    Gaussians that survive, removed (indices), floored (eigenvalues, Gaussians), objf_before, objf_after, count."""
    import numpy as np
    L = lib()
    w = np.array(weights, dtype=np.float32)
    b = np.array(means_invcovars, dtype=np.float32)
    ic = np.array(inv_covars, dtype=np.float32)
    if b.ndim != 2 or w.shape != (b.shape[0],) or ic.shape != (b.shape[0], b.shape[1] * (b.shape[1] + 1) // 2):
        raise XvError(XV_ERR_ARG, "fgmm_est: weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2]")
    g, d = b.shape
    o = np.ascontiguousarray(occ, dtype=np.float64)
    m = np.ascontiguousarray(mean, dtype=np.float64)
    c = np.ascontiguousarray(cov, dtype=np.float64)
    if o.shape != (g,) or m.shape != (g, d) or c.shape != ic.shape:
        raise XvError(XV_ERR_ARG, "fgmm_est: occ [G], mean [G][D], cov [G][D (D + 1) / 2]")
    gc = np.zeros(g, np.float32)
    removed = np.zeros(g, np.int32)
    floored = np.zeros(2, np.int32)
    objf = np.zeros(3)
    left = ctypes.c_int32()
    L.xv_fgmm_est.argtypes = ([ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p] + [ctypes.c_void_p] * 3 + [ctypes.c_char_p] + [ctypes.c_double] * 4
                              + [ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_void_p] * 3)
    _check(L.xv_fgmm_est(g, d, acc_flags.encode(), o.ctypes.data, m.ctypes.data, c.ctypes.data, update_flags.encode(), min_gaussian_weight,
                         min_gaussian_occupancy, variance_floor, max_condition, int(bool(remove_low_count_gaussians)), w.ctypes.data, b.ctypes.data,
                         ic.ctypes.data, gc.ctypes.data, ctypes.byref(left), removed.ctypes.data, floored.ctypes.data, objf.ctypes.data))
    k = left.value
    return dict(weights=w[:k].copy(), means_invcovars=b[:k].copy(), inv_covars=ic[:k].copy(), gconsts=gc[:k].copy(),
                removed=removed[:g - k].tolist(), floored=(int(floored[0]), int(floored[1])), objf_before=float(objf[0]),
                objf_after=float(objf[1]), count=float(objf[2]))


def logprob_to_post(logprobs_list, keys, min_post=0.01, random_prune=True, frame_budget=0, device=0, return_details=False):
    """logprob-to-post on the device (xv_logprob_to_post): per utterance a list (one entry per row) of (int32 columns, float32
    weights), columns ascending.  keys: the utterance keys, which key the random pruning.  frame_budget: rows per launch (0: the
    default); the result does not depend on it.  return_details: also dict(num_nan, ms=(count, scan, write))."""
    import numpy as np
    L = lib()
    packed, off, cols = _pack_matrices(logprobs_list, "logprob_to_post")
    nu, rows = len(off) - 1, packed.shape[0]
    if len(keys) != nu:
        raise XvError(XV_ERR_ARG, "logprob_to_post: one key per matrix")
    if rows == 0:
        out = [[] for _ in range(nu)]
        return (out, dict(num_nan=0, ms=(0.0, 0.0, 0.0))) if return_details else out
    ckeys = (ctypes.c_char_p * max(nu, 1))(*[k.encode() for k in keys])
    pair_off = np.zeros(rows + 1, dtype=np.int64)
    need, num_nan = ctypes.c_int64(0), ctypes.c_int64(0)
    ms = (ctypes.c_float * 3)()
    L.xv_logprob_to_post.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_float,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    capacity = min(rows * cols, max(1 << 16, rows * 64))
    while True:
        idx = np.zeros(capacity, dtype=np.int32)
        w = np.zeros(capacity, dtype=np.float32)
        _check(L.xv_logprob_to_post(device, packed.ctypes.data, off.ctypes.data, nu, cols, ckeys, float(min_post), int(bool(random_prune)),
                                    int(frame_budget), capacity, pair_off.ctypes.data, idx.ctypes.data, w.ctypes.data, ctypes.byref(need),
                                    ctypes.byref(num_nan), ms))
        if need.value <= capacity:
            break
        capacity = need.value
    out = [[(idx[pair_off[t]:pair_off[t + 1]].copy(), w[pair_off[t]:pair_off[t + 1]].copy()) for t in range(off[u], off[u + 1])] for u in range(nu)]
    return (out, dict(num_nan=int(num_nan.value), ms=tuple(float(v) for v in ms))) if return_details else out


def logprob_to_post_kernel_time(logprobs, key="utt", min_post=0.01, random_prune=True, reps=5, device=0):
    """{count, scan, write, copy} times in ms of one rows x cols matrix in one launch (xv_logprob_to_post_kernel_time: the best of
    reps).  copy: a device-to-device copy of the input, which is what two reads of it cost at the copy bandwidth of this run."""
    import numpy as np
    L = lib()
    x = np.ascontiguousarray(logprobs, dtype=np.float32)
    if x.ndim != 2:
        raise XvError(XV_ERR_ARG, "logprob_to_post_kernel_time: a [rows, cols] matrix")
    ms = (ctypes.c_float * 4)()
    L.xv_logprob_to_post_kernel_time.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_float,
                                                 ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    _check(L.xv_logprob_to_post_kernel_time(device, x.ctypes.data, x.shape[0], x.shape[1], key.encode(), float(min_post), int(bool(random_prune)), reps, ms))
    return dict(zip(("count", "scan", "write", "copy"), [float(v) for v in ms]))


def fgmm_init_from_accs(occ, mean, cov, remove_low_count_gaussians=True):
    """fgmm-global-init-from-accs on host arrays (xv_fgmm_init_from_accs, fp64): dict(weights, means_invcovars, inv_covars, gconsts) of
    the Gaussians that survive, removed (indices), bad_gconsts, and inv_covars_f64: the survivors' inverse covariances before they are
    rounded to float32."""
    import numpy as np
    L = lib()
    o = np.ascontiguousarray(occ, dtype=np.float64)
    m = np.ascontiguousarray(mean, dtype=np.float64)
    c = np.ascontiguousarray(cov, dtype=np.float64)
    if m.ndim != 2 or o.shape != (m.shape[0],) or c.shape != (m.shape[0], m.shape[1] * (m.shape[1] + 1) // 2):
        raise XvError(XV_ERR_ARG, "fgmm_init_from_accs: occ [G], mean [G][D], cov [G][D (D + 1) / 2]")
    g, d = m.shape
    w, b, ic, gc = np.zeros(g, np.float32), np.zeros((g, d), np.float32), np.zeros(c.shape, np.float32), np.zeros(g, np.float32)
    removed = np.zeros(g, np.int32)
    ic64 = np.zeros(c.shape, np.float64)
    left, bad = ctypes.c_int32(), ctypes.c_int32()
    L.xv_fgmm_init_from_accs.argtypes = ([ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int32] + [ctypes.c_void_p] * 4
                                         + [ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p])
    _check(L.xv_fgmm_init_from_accs(g, d, o.ctypes.data, m.ctypes.data, c.ctypes.data, int(bool(remove_low_count_gaussians)), w.ctypes.data,
                                    b.ctypes.data, ic.ctypes.data, gc.ctypes.data, ctypes.byref(left), removed.ctypes.data, ctypes.byref(bad),
                                    ic64.ctypes.data))
    k = left.value
    gone = removed[:g - k].tolist()
    return dict(weights=w[:k].copy(), means_invcovars=b[:k].copy(), inv_covars=ic[:k].copy(), gconsts=gc[:k].copy(), removed=gone,
                bad_gconsts=int(bad.value), inv_covars_f64=np.delete(ic64, gone, axis=0))


class DgmmAccumulator:
    """The fp64 accumulators of diagonal UBM training on one device (xv_dgmm_acc_create): occ [G], mean [G][D] and var [G][D] (the sums
    of p x x).  flags: letters of "mvw" (v implies m, m implies w)."""

    def __init__(self, num_gauss, dim, flags="mvw", device=0):
        L = lib()
        self._h = ctypes.c_void_p()
        self.num_gauss, self.dim, self.flags = int(num_gauss), int(dim), flags
        L.xv_dgmm_acc_create.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _check(L.xv_dgmm_acc_create(device, self.num_gauss, self.dim, flags.encode(), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            L = lib()
            L.xv_dgmm_acc_destroy.argtypes = [ctypes.c_void_p]
            L.xv_dgmm_acc_destroy.restype = None
            L.xv_dgmm_acc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _feats(self, feats, who):
        import numpy as np
        x = np.ascontiguousarray(feats, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise XvError(XV_ERR_ARG, "%s: the features are not [frames, %d]" % (who, self.dim))
        return x

    def accumulate(self, feats, post):
        """One call: feats [frames, D]; post: per frame (indices, posteriors).  The accumulator kernels alone."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "accumulate")
        if len(post) != x.shape[0]:
            raise XvError(XV_ERR_ARG, "accumulate: one (indices, posteriors) pair per frame")
        off = np.zeros(x.shape[0] + 1, dtype=np.int32)
        for t, (i, _) in enumerate(post):
            off[t + 1] = off[t] + len(i)
        idx = np.ascontiguousarray(np.concatenate([np.asarray(i, np.int32) for i, _ in post]) if len(post) else np.zeros(0), dtype=np.int32)
        w = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32) for _, p in post]) if len(post) else np.zeros(0), dtype=np.float32)
        L.xv_dgmm_acc_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_dgmm_acc_add(self._h, x.ctypes.data, x.shape[0], off.ctypes.data, idx.ctypes.data, w.ctypes.data))

    def accumulate_gselect(self, diag, feats, gselect, return_loglikes=False):
        """The fused sparse E-step on a diagonal Ubm over gselect [frames, n].  Returns the per-frame log-sums, float32 [frames] (and
        the scores [frames, n])."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "accumulate_gselect")
        gs = np.ascontiguousarray(gselect, dtype=np.int32)
        if gs.ndim != 2 or gs.shape[0] != x.shape[0]:
            raise XvError(XV_ERR_ARG, "accumulate_gselect: a [frames, n] selection")
        logsum = np.zeros(x.shape[0], dtype=np.float32)
        ll = np.zeros(gs.shape, dtype=np.float32)
        L.xv_dgmm_acc_add_gselect.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_void_p]
        _check(L.xv_dgmm_acc_add_gselect(self._h, diag._h, x.ctypes.data, x.shape[0], gs.ctypes.data, gs.shape[1],
                                         ll.ctypes.data if return_loglikes else None, logsum.ctypes.data))
        return (logsum, ll) if return_loglikes else logsum

    def accumulate_dense_post(self, feats, post):
        """A caller's dense posteriors [frames, G] through the matrix-core accumulation kernel alone."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "accumulate_dense_post")
        p = np.ascontiguousarray(post, dtype=np.float32)
        if p.shape != (x.shape[0], self.num_gauss):
            raise XvError(XV_ERR_ARG, "accumulate_dense_post: posteriors [frames, %d]" % self.num_gauss)
        L.xv_dgmm_acc_add_dense_post.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        _check(L.xv_dgmm_acc_add_dense_post(self._h, x.ctypes.data, x.shape[0], p.ctypes.data))

    def accumulate_dense(self, diag, feats):
        """The fused dense E-step: every frame against every Gaussian of a diagonal Ubm.  Returns the per-frame log-sums."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "accumulate_dense")
        logsum = np.zeros(x.shape[0], dtype=np.float32)
        L.xv_dgmm_acc_add_dense.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        _check(L.xv_dgmm_acc_add_dense(self._h, diag._h, x.ctypes.data, x.shape[0], logsum.ctypes.data))
        return logsum

    def get(self):
        """(occ [G], mean [G, D], var [G, D]) as float64."""
        import numpy as np
        L = lib()
        g, d = self.num_gauss, self.dim
        occ, mean, var = np.zeros(g), np.zeros((g, d)), np.zeros((g, d))
        L.xv_dgmm_acc_get.argtypes = [ctypes.c_void_p] * 4
        _check(L.xv_dgmm_acc_get(self._h, occ.ctypes.data, mean.ctypes.data, var.ctypes.data))
        return occ, mean, var

    def kernel_time(self, diag, feats, gselect=None, dense=True, reps=3):
        """{sort, scores, softmax, acc} of one fused sparse call (with gselect) and {dense_logsum, dense_acc, dense_reduce} of one fused
        dense call, in ms (xv_dgmm_acc_kernel_time: the best of reps).  Every run adds to the accumulators."""
        import numpy as np
        L = lib()
        x = self._feats(feats, "kernel_time")
        gs = None if gselect is None else np.ascontiguousarray(gselect, dtype=np.int32)
        ms = (ctypes.c_float * 7)()
        L.xv_dgmm_acc_kernel_time.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
        _check(L.xv_dgmm_acc_kernel_time(self._h, diag._h, x.ctypes.data, x.shape[0], None if gs is None else gs.ctypes.data,
                                         0 if gs is None else gs.shape[1], int(bool(dense)), reps, ms))
        return dict(zip(("sort", "scores", "softmax", "acc", "dense_logsum", "dense_acc", "dense_reduce"), [float(v) for v in ms]))


def dgmm_est(weights, means_invvars, inv_vars, occ, mean, var, acc_flags="mvw", update_flags="mvw", min_gaussian_weight=1e-5,
             min_gaussian_occupancy=10.0, min_variance=0.001, remove_low_count_gaussians=True, mix_up=0, perturb_factor=0.01, seed=0):
    """The M-step of gmm-global-est on host arrays (xv_dgmm_est, fp64), then the split to mix_up Gaussians: dict(weights, means_invvars,
    inv_vars, gconsts) of the model that results, removed (indices), floored (variances, Gaussians), objf_before, objf_after, count,
    split_of (for every Gaussian the split added, the index it was copied from)."""
    import numpy as np
    L = lib()
    w0 = np.asarray(weights, dtype=np.float32)
    b0 = np.asarray(means_invvars, dtype=np.float32)
    iv0 = np.asarray(inv_vars, dtype=np.float32)
    if b0.ndim != 2 or w0.shape != (b0.shape[0],) or iv0.shape != b0.shape:
        raise XvError(XV_ERR_ARG, "dgmm_est: weights [G], means_invvars [G][D], inv_vars [G][D]")
    g, d = b0.shape
    o = np.ascontiguousarray(occ, dtype=np.float64)
    m = np.ascontiguousarray(mean, dtype=np.float64)
    c = np.ascontiguousarray(var, dtype=np.float64)
    if o.shape != (g,) or m.shape != (g, d) or c.shape != (g, d):
        raise XvError(XV_ERR_ARG, "dgmm_est: occ [G], mean [G][D], var [G][D]")
    cap = max(g, int(mix_up))
    w, b, iv = np.zeros(cap, np.float32), np.zeros((cap, d), np.float32), np.zeros((cap, d), np.float32)
    w[:g], b[:g], iv[:g] = w0, b0, iv0
    gc = np.zeros(cap, np.float32)
    removed = np.zeros(g, np.int32)
    split_of = np.zeros(max(cap, 1), np.int32)
    floored = np.zeros(2, np.int32)
    objf = np.zeros(3)
    left, n_removed = ctypes.c_int32(), ctypes.c_int32()
    L.xv_dgmm_est.argtypes = ([ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p] + [ctypes.c_void_p] * 3 + [ctypes.c_char_p] + [ctypes.c_double] * 3
                              + [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64] + [ctypes.c_void_p] * 4
                              + [ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_void_p] * 3)
    _check(L.xv_dgmm_est(g, d, acc_flags.encode(), o.ctypes.data, m.ctypes.data, c.ctypes.data, update_flags.encode(), min_gaussian_weight,
                         min_gaussian_occupancy, min_variance, int(bool(remove_low_count_gaussians)), int(mix_up), perturb_factor, int(seed),
                         w.ctypes.data, b.ctypes.data, iv.ctypes.data, gc.ctypes.data, ctypes.byref(left), removed.ctypes.data,
                         ctypes.byref(n_removed), floored.ctypes.data, objf.ctypes.data, split_of.ctypes.data))
    k, nr = left.value, n_removed.value
    return dict(weights=w[:k].copy(), means_invvars=b[:k].copy(), inv_vars=iv[:k].copy(), gconsts=gc[:k].copy(),
                removed=removed[:nr].tolist(), floored=(int(floored[0]), int(floored[1])), objf_before=float(objf[0]),
                objf_after=float(objf[1]), count=float(objf[2]), split_of=split_of[:max(0, k - (g - nr))].tolist())


def ivex_read(rxfilename):
    """A final.ie (binary or text; "file", "-", "cmd |") as host arrays: dict(w_vec [G], M [G][D][S], sigma_inv [G][D (D + 1) / 2],
    prior_offset).  Host only."""
    import numpy as np
    L = lib()
    L.xv_ivex_read.argtypes = [ctypes.c_char_p] + [ctypes.POINTER(ctypes.c_int32)] * 3 + [ctypes.c_void_p] * 3 + [ctypes.POINTER(ctypes.c_double)]
    g, d, s = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(L.xv_ivex_read(rxfilename.encode(), ctypes.byref(g), ctypes.byref(d), ctypes.byref(s), None, None, None, None))
    G, D, S = g.value, d.value, s.value
    w_vec, M, sig = np.zeros(G), np.zeros((G, D, S)), np.zeros((G, D * (D + 1) // 2))
    p = ctypes.c_double()
    _check(L.xv_ivex_read(rxfilename.encode(), None, None, None, w_vec.ctypes.data, M.ctypes.data, sig.ctypes.data, ctypes.byref(p)))
    return dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=p.value)


def _ivex_arrays(w_vec, M, sigma_inv, who):
    import numpy as np
    M = np.ascontiguousarray(M, dtype=np.float64)
    w_vec = np.ascontiguousarray(w_vec, dtype=np.float64)
    sig = np.ascontiguousarray(sigma_inv, dtype=np.float64)
    if M.ndim != 3 or w_vec.shape != (M.shape[0],) or sig.shape != (M.shape[0], M.shape[1] * (M.shape[1] + 1) // 2):
        raise XvError(XV_ERR_ARG, who + ": w_vec [G], M [G][D][S], sigma_inv [G][D (D + 1) / 2]")
    return w_vec, M, sig


def ivex_write(wxfilename, w_vec, M, sigma_inv, prior_offset, binary=True):
    """Host arrays to a final.ie (text: 17 significant digits).  Host only."""
    L = lib()
    w_vec, M, sig = _ivex_arrays(w_vec, M, sigma_inv, "ivex_write")
    L.xv_ivex_write.argtypes = [ctypes.c_char_p] + [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_double]
    _check(L.xv_ivex_write(wxfilename.encode(), int(bool(binary)), M.shape[0], M.shape[1], M.shape[2], w_vec.ctypes.data, M.ctypes.data,
                           sig.ctypes.data, float(prior_offset)))


def _pack_posteriors(post_list, off, who):
    """post_list[u][t] = (indices, weights) -> (post_off [rows + 1], post_idx, post_w)"""
    import numpy as np
    if len(post_list) != len(off) - 1 or any(len(p) != off[u + 1] - off[u] for u, p in enumerate(post_list)):
        raise XvError(XV_ERR_ARG, who + ": one posterior per utterance, one (indices, weights) entry per frame")
    counts = [len(f[0]) for p in post_list for f in p]
    post_off = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=post_off[1:])
    idx = [np.asarray(f[0], dtype=np.int32).reshape(-1) for p in post_list for f in p]
    w = [np.asarray(f[1], dtype=np.float32).reshape(-1) for p in post_list for f in p]
    post_idx = np.ascontiguousarray(np.concatenate(idx)) if idx else np.zeros(0, np.int32)
    post_w = np.ascontiguousarray(np.concatenate(w)) if w else np.zeros(0, np.float32)
    if post_idx.shape != post_w.shape:
        raise XvError(XV_ERR_ARG, who + ": a frame's indices and weights have one length")
    return post_off, post_idx, post_w


class IvectorExtractor:
    """An i-vector extractor on one device (xv_ivex_create / xv_ivex_load): the derived variables are computed there once.
    IvectorExtractor(w_vec, M, sigma_inv, prior_offset) from host arrays, IvectorExtractor.load(rxfilename) from a final.ie."""

    def __init__(self, w_vec=None, M=None, sigma_inv=None, prior_offset=0.0, device=0, _handle=None):
        L = lib()
        self._h = _handle
        if self._h is None:
            w_vec, M, sig = _ivex_arrays(w_vec, M, sigma_inv, "IvectorExtractor")
            L.xv_ivex_create.argtypes = [ctypes.c_int] + [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)]
            h = ctypes.c_void_p()
            _check(L.xv_ivex_create(device, M.shape[0], M.shape[1], M.shape[2], w_vec.ctypes.data, M.ctypes.data, sig.ctypes.data,
                                    float(prior_offset), ctypes.byref(h)))
            self._h = h
        L.xv_ivex_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int32)] * 3
        g, d, s = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(L.xv_ivex_info(self._h, ctypes.byref(g), ctypes.byref(d), ctypes.byref(s)))
        self.num_gauss, self.feat_dim, self.ivector_dim = g.value, d.value, s.value

    @classmethod
    def load(cls, rxfilename, device=0):
        L = lib()
        L.xv_ivex_load.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        h = ctypes.c_void_p()
        _check(L.xv_ivex_load(device, rxfilename.encode(), ctypes.byref(h)))
        return cls(_handle=h)

    def close(self):
        if self._h:
            L = lib()
            L.xv_ivex_destroy.argtypes = [ctypes.c_void_p]
            L.xv_ivex_destroy.restype = None
            L.xv_ivex_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def derived(self):
        """(SigmaInvM [G D][S], U [G][S (S + 1) / 2]) as the device computed them."""
        import numpy as np
        L = lib()
        G, D, S = self.num_gauss, self.feat_dim, self.ivector_dim
        sim, U = np.zeros((G * D, S)), np.zeros((G, S * (S + 1) // 2))
        L.xv_ivex_derived.argtypes = [ctypes.c_void_p] * 3
        _check(L.xv_ivex_derived(self._h, sim.ctypes.data, U.ctypes.data))
        return sim, U

    def _inputs(self, feats_list, post_list, who):
        packed, off, cols = _pack_matrices(feats_list, who)
        if cols != self.feat_dim:
            raise XvError(XV_ERR_ARG, "%s: the features have %d columns, the model %d" % (who, cols, self.feat_dim))
        return (packed, off) + _pack_posteriors(post_list, off, who)

    def extract(self, feats_list, post_list, return_details=False, acoustic_weight=1.0, max_count=0.0):
        """feats_list[u]: float32 [frames, D]; post_list[u][t] = (Gaussian indices, posteriors) of frame t.  Returns (ivectors
        float32 [n, S], status int32 [n], auxf_change float64 [n]); return_details: also a dict of gamma [n, G], X [n, G D],
        linear [n, S] and quadratic [n, S, S] (Q, symmetric), all float64 as the device formed them."""
        import numpy as np
        L = lib()
        packed, off, post_off, post_idx, post_w = self._inputs(feats_list, post_list, "extract")
        n, G, D, S = len(off) - 1, self.num_gauss, self.feat_dim, self.ivector_dim
        P = S * (S + 1) // 2
        iv, status, auxf = np.zeros((n, S), np.float32), np.zeros(n, np.int32), np.zeros(n)
        det = dict(gamma=np.zeros((n, G)), X=np.zeros((n, G * D)), linear=np.zeros((n, S)), quadratic=np.zeros((n, P))) if return_details else {}
        ptr = lambda k: det[k].ctypes.data if return_details else None
        L.xv_ivex_extract.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 7
        _check(L.xv_ivex_extract(self._h, packed.ctypes.data, off.ctypes.data, n, post_off.ctypes.data, post_idx.ctypes.data,
                                 post_w.ctypes.data, float(acoustic_weight), float(max_count), iv.ctypes.data, status.ctypes.data,
                                 auxf.ctypes.data, ptr("gamma"), ptr("X"), ptr("linear"), ptr("quadratic")))
        if not return_details:
            return iv, status, auxf
        r, c = np.tril_indices(S)
        Q = np.zeros((n, S, S))
        Q[:, r, c] = det["quadratic"]
        Q[:, c, r] = det["quadratic"]
        det["quadratic"] = Q
        return iv, status, auxf, det

    def kernel_time(self, feats_list, post_list, reps=5):
        """{stats, quadratic, linear, solve, derive} kernel times in ms of one call (xv_ivex_kernel_time: the best of reps)."""
        L = lib()
        packed, off, post_off, post_idx, post_w = self._inputs(feats_list, post_list, "kernel_time")
        ms = (ctypes.c_float * 5)()
        L.xv_ivex_kernel_time.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_void_p]
        _check(L.xv_ivex_kernel_time(self._h, packed.ctypes.data, off.ctypes.data, len(off) - 1, post_off.ctypes.data, post_idx.ctypes.data,
                                     post_w.ctypes.data, reps, ms))
        return dict(zip(("stats", "quadratic", "linear", "solve", "derive"), [float(x) for x in ms]))


def _ivex_stats_arrays(G, D, S, has_variances):
    import numpy as np
    P = S * (S + 1) // 2
    return dict(scalars=np.zeros(3), gamma=np.zeros(G), Y=np.zeros((G, D, S)), R=np.zeros((G, P)),
                S=np.zeros((G, D * (D + 1) // 2)) if has_variances else None, ivector_sum=np.zeros(S), ivector_scatter=np.zeros(P))


def _ivex_stats_out(a):
    out = dict(num_ivectors=float(a["scalars"][0]), auxf=float(a["scalars"][1]), frames=float(a["scalars"][2]))
    out.update({k: a[k] for k in ("gamma", "Y", "R", "S", "ivector_sum", "ivector_scatter")})
    return out


def _ivex_stats_in(stats, who):
    """the dict of IvexAccumulator.get() -> (G, D, S, has_variances, the seven pointers' arrays)"""
    import numpy as np
    Y = np.ascontiguousarray(stats["Y"], dtype=np.float64)
    if Y.ndim != 3:
        raise XvError(XV_ERR_ARG, who + ": Y [G][D][S]")
    G, D, S = Y.shape
    P = S * (S + 1) // 2
    has = stats.get("S") is not None
    arr = dict(scalars=np.array([stats["num_ivectors"], stats["auxf"], stats["frames"]], dtype=np.float64), Y=Y)
    for k, shape in (("gamma", (G,)), ("R", (G, P)), ("S", (G, D * (D + 1) // 2)), ("ivector_sum", (S,)), ("ivector_scatter", (P,))):
        if k == "S" and not has:
            arr[k] = None
            continue
        arr[k] = np.ascontiguousarray(stats[k], dtype=np.float64)
        if arr[k].shape != shape:
            raise XvError(XV_ERR_ARG, "%s: %s has shape %s, the statistics ask for %s" % (who, k, arr[k].shape, shape))
    return G, D, S, has, arr


def _ptr(a):
    return None if a is None else a.ctypes.data


def ivex_stats_read(rxfilename):
    """The statistics file of ivector-extractor-acc-stats as the dict of IvexAccumulator.get().  Host only."""
    L = lib()
    L.xv_ivex_stats_read.argtypes = [ctypes.c_char_p] + [ctypes.POINTER(ctypes.c_int32)] * 4 + [ctypes.c_void_p] * 7
    g, d, s, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(L.xv_ivex_stats_read(rxfilename.encode(), ctypes.byref(g), ctypes.byref(d), ctypes.byref(s), ctypes.byref(v), *([None] * 7)))
    a = _ivex_stats_arrays(g.value, d.value, s.value, bool(v.value))
    _check(L.xv_ivex_stats_read(rxfilename.encode(), None, None, None, None, a["scalars"].ctypes.data, a["gamma"].ctypes.data, a["Y"].ctypes.data,
                                a["R"].ctypes.data, _ptr(a["S"]), a["ivector_sum"].ctypes.data, a["ivector_scatter"].ctypes.data))
    return _ivex_stats_out(a)


def ivex_stats_write(wxfilename, stats, binary=True):
    """The dict of IvexAccumulator.get() to a statistics file (text: 17 significant digits).  Host only."""
    L = lib()
    G, D, S, has, a = _ivex_stats_in(stats, "ivex_stats_write")
    L.xv_ivex_stats_write.argtypes = [ctypes.c_char_p] + [ctypes.c_int32] * 5 + [ctypes.c_void_p] * 7
    _check(L.xv_ivex_stats_write(wxfilename.encode(), int(bool(binary)), G, D, S, int(has), a["scalars"].ctypes.data, a["gamma"].ctypes.data,
                                 a["Y"].ctypes.data, a["R"].ctypes.data, _ptr(a["S"]), a["ivector_sum"].ctypes.data, a["ivector_scatter"].ctypes.data))


def ivex_init(weights, means_invcovars, inv_covars, ivector_dim=400, seed=0):
    """ivector-extractor-init on host arrays: a full-covariance UBM (float32 weights [G], means_invcovars [G][D], inv_covars
    [G][D (D + 1) / 2]) -> dict(w_vec, M, sigma_inv, prior_offset).  The same seed gives the same bytes.  Host only."""
    import numpy as np
    L = lib()
    w = np.ascontiguousarray(weights, dtype=np.float32)
    b = np.ascontiguousarray(means_invcovars, dtype=np.float32)
    ic = np.ascontiguousarray(inv_covars, dtype=np.float32)
    if b.ndim != 2 or w.shape != (b.shape[0],) or ic.shape != (b.shape[0], b.shape[1] * (b.shape[1] + 1) // 2):
        raise XvError(XV_ERR_ARG, "ivex_init: weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2]")
    G, D = b.shape
    S = int(ivector_dim)
    w_vec, M, sig = np.zeros(G), np.zeros((G, D, max(S, 1))), np.zeros((G, D * (D + 1) // 2))
    p = ctypes.c_double()
    L.xv_ivex_init.argtypes = [ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [
        ctypes.POINTER(ctypes.c_double)]
    _check(L.xv_ivex_init(G, D, w.ctypes.data, b.ctypes.data, ic.ctypes.data, S, int(seed) & (2 ** 64 - 1), w_vec.ctypes.data, M.ctypes.data,
                          sig.ctypes.data, ctypes.byref(p)))
    return dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=p.value)


def ivex_est(stats, w_vec, M, sigma_inv, prior_offset, variance_floor_factor=0.1, gaussian_min_count=100.0, diagonalize=True, num_threads=1):
    """The M-step of ivector-extractor-est (host, fp64) on the dict of IvexAccumulator.get().  Returns dict(w_vec, M, sigma_inv,
    prior_offset, V [S][S], gauss_updated, gauss_skipped, eig_floored, var_floored, var_floored_gauss, prior_floored, impr_proj,
    impr_var, impr_prior); the improvements are per frame."""
    import numpy as np
    L = lib()
    w_vec, M, sig = _ivex_arrays(w_vec, M, sigma_inv, "ivex_est")
    M, sig = M.copy(), sig.copy()
    G, D, S, has, a = _ivex_stats_in(stats, "ivex_est")
    if M.shape != (G, D, S):
        raise XvError(XV_ERR_ARG, "ivex_est: the statistics' shape %s is not the model's %s" % ((G, D, S), M.shape))
    p = ctypes.c_double(float(prior_offset))
    counts, impr, V = np.zeros(6, np.int32), np.zeros(3), np.zeros((S, S))
    L.xv_ivex_est.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 7 + [ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32] + [
        ctypes.c_void_p] * 3 + [ctypes.POINTER(ctypes.c_double)] + [ctypes.c_void_p] * 3
    _check(L.xv_ivex_est(G, D, S, int(has), a["scalars"].ctypes.data, a["gamma"].ctypes.data, a["Y"].ctypes.data, a["R"].ctypes.data, _ptr(a["S"]),
                         a["ivector_sum"].ctypes.data, a["ivector_scatter"].ctypes.data, float(variance_floor_factor), float(gaussian_min_count),
                         int(bool(diagonalize)), int(num_threads), w_vec.ctypes.data, M.ctypes.data, sig.ctypes.data, ctypes.byref(p),
                         counts.ctypes.data, impr.ctypes.data, V.ctypes.data))
    out = dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=p.value, V=V)
    out.update(zip(("gauss_updated", "gauss_skipped", "eig_floored", "var_floored", "var_floored_gauss", "prior_floored"), [int(c) for c in counts]))
    out.update(zip(("impr_proj", "impr_var", "impr_prior"), [float(x) for x in impr]))
    return out


def ivex_rank_update(A, B, C, slots, M, N, device=0):
    """The update kernel of extractor training alone (xv_ivex_rank_update): C[:M, :N] += A[:slots, :M].T @ B[:slots, :N] on the
    device; A [64][M], B [64][N], C [rows >= M][ld >= N] float64.  Returns the new C; what lies outside [M][N] comes back as it went."""
    import numpy as np
    L = lib()
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    C = np.array(C, dtype=np.float64, order="C")
    if A.shape != (64, M) or B.shape != (64, N) or C.ndim != 2:
        raise XvError(XV_ERR_ARG, "ivex_rank_update: A [64][M], B [64][N], C [rows][ld]")
    L.xv_ivex_rank_update.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int32] + [ctypes.c_int64] * 4
    _check(L.xv_ivex_rank_update(device, A.ctypes.data, B.ctypes.data, C.ctypes.data, int(slots), int(M), int(N), C.shape[0], C.shape[1]))
    return C


class IvexAccumulator:
    """The fp64 statistics of i-vector extractor training on the model's device (xv_ivex_acc_create; semantics in csrc/ivex_train.h).
    They are a function of the model and the ordered sequence of accepted utterances: how accumulate() calls split them changes no bit."""

    def __init__(self, model, update_variances=True, compute_auxf=True):
        L = lib()
        self.model = model   # the device model must outlive the accumulators
        self.update_variances = bool(update_variances)
        self._h = ctypes.c_void_p()
        L.xv_ivex_acc_create.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
        _check(L.xv_ivex_acc_create(model._h, int(self.update_variances), int(bool(compute_auxf)), ctypes.byref(self._h)))

    def close(self):
        if self._h:
            L = lib()
            L.xv_ivex_acc_destroy.argtypes = [ctypes.c_void_p]
            L.xv_ivex_acc_destroy.restype = None
            L.xv_ivex_acc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate(self, feats_list, post_list):
        """The inputs of IvectorExtractor.extract.  Returns status int32 [n]: 1 for an utterance whose Q is not positive definite (it
        contributes to nothing)."""
        import numpy as np
        L = lib()
        packed, off, post_off, post_idx, post_w = self.model._inputs(feats_list, post_list, "accumulate")
        status = np.zeros(len(off) - 1, np.int32)
        L.xv_ivex_acc_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4
        _check(L.xv_ivex_acc_add(self._h, packed.ctypes.data, off.ctypes.data, len(off) - 1, post_off.ctypes.data, post_idx.ctypes.data,
                                 post_w.ctypes.data, status.ctypes.data))
        return status

    def get(self):
        """Flushes what is pending and returns dict(num_ivectors, auxf, frames, gamma [G], Y [G][D][S], R [G][P], S [G][D (D + 1) / 2]
        or None, ivector_sum [S], ivector_scatter [P])."""
        L = lib()
        m = self.model
        a = _ivex_stats_arrays(m.num_gauss, m.feat_dim, m.ivector_dim, self.update_variances)
        L.xv_ivex_acc_get.argtypes = [ctypes.c_void_p] * 8
        _check(L.xv_ivex_acc_get(self._h, a["scalars"].ctypes.data, a["gamma"].ctypes.data, a["Y"].ctypes.data, a["R"].ctypes.data, _ptr(a["S"]),
                                 a["ivector_sum"].ctypes.data, a["ivector_scatter"].ctypes.data))
        return _ivex_stats_out(a)

    def pending(self):
        """The pending utterances as the posterior kernel left them: dict(m [n][S], scatter [n][P], logdet [n], auxf [n])."""
        import numpy as np
        L = lib()
        S = self.model.ivector_dim
        P = S * (S + 1) // 2
        m, sc, ld, ax = np.zeros((64, S)), np.zeros((64, P)), np.zeros(64), np.zeros(64)
        n = ctypes.c_int32()
        L.xv_ivex_acc_pending.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)] + [ctypes.c_void_p] * 4
        _check(L.xv_ivex_acc_pending(self._h, ctypes.byref(n), m.ctypes.data, sc.ctypes.data, ld.ctypes.data, ax.ctypes.data))
        k = n.value
        return dict(m=m[:k].copy(), scatter=sc[:k].copy(), logdet=ld[:k].copy(), auxf=ax[:k].copy())

    def kernel_time(self, feats_list, post_list, reps=3):
        """{posterior, rank_update_R, rank_update_Y} kernel times in ms of one accumulate() and flush (the best of reps).  Every run
        adds the call's statistics to the accumulators."""
        L = lib()
        packed, off, post_off, post_idx, post_w = self.model._inputs(feats_list, post_list, "kernel_time")
        ms = (ctypes.c_float * 3)()
        L.xv_ivex_acc_kernel_time.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int32] + [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_void_p]
        _check(L.xv_ivex_acc_kernel_time(self._h, packed.ctypes.data, off.ctypes.data, len(off) - 1, post_off.ctypes.data, post_idx.ctypes.data,
                                         post_w.ctypes.data, reps, ms))
        return dict(zip(("posterior", "rank_update_R", "rank_update_Y"), [float(x) for x in ms]))


def kernel_tdnn_gemm(desc):
    _check(lib().xv_kernel_tdnn_gemm(ctypes.byref(desc)))


def last_gemm_kernel():
    """Name of the kernel the calling thread's last kernel_tdnn_gemm launched, e.g. 'tdnn_gemm_kernel_sk<fp16x2,act,8>'."""
    return lib().xv_last_gemm_kernel().decode()


def plan_gemm(desc, cus=0, policy=None):
    """What kernel_tdnn_gemm(desc) would launch, without a device (csrc/gemm_plan.h): a GemmPlan.  cus > 0: a device of that many
    CUs under the default knobs, else the current device and XVEC_DEBUG.  policy: dict(variant, sk_mf, sk_lanes, stagger_pct) to
    state the knobs (missing ones at their defaults; needs cus > 0)."""
    L = lib()
    out = GemmPlan()
    if policy is None:
        L.xv_plan_gemm.argtypes = [ctypes.POINTER(GemmDesc), ctypes.c_int32, ctypes.POINTER(GemmPlan)]
        _check(L.xv_plan_gemm(ctypes.byref(desc), cus, ctypes.byref(out)))
    else:
        k = dict(dict(variant=0, sk_mf=8, sk_lanes=4, stagger_pct=85), **policy)
        L.xv_plan_gemm_policy.argtypes = [ctypes.POINTER(GemmDesc)] + [ctypes.c_int32] * 5 + [ctypes.POINTER(GemmPlan)]
        _check(L.xv_plan_gemm_policy(ctypes.byref(desc), cus, k["variant"], k["sk_mf"], k["sk_lanes"], k["stagger_pct"], ctypes.byref(out)))
    return out


def kernel_first_layer(desc):
    _check(lib().xv_kernel_first_layer(ctypes.byref(desc)))


def kernel_prep_input(desc):
    _check(lib().xv_kernel_prep_input(ctypes.byref(desc)))


def kernel_pool_finalise(desc):
    _check(lib().xv_kernel_pool_finalise(ctypes.byref(desc)))


def kernel_frame_output(desc):
    _check(lib().xv_kernel_frame_output(ctypes.byref(desc)))


def bucket_sort(keys, seg_off, num_keys, device=0, pairs=None):
    """The stable counting sort by key of the UBM, GMM and i-vector statistics, inside every segment [seg_off[s], seg_off[s + 1])
    of keys (int32, each in [0, num_keys)).  Returns (bucket_start [segments, num_keys + 1], sorted [pairs]): absolute positions
    of the buckets and the pair indices, ascending inside a bucket.  pairs: len(keys) unless given."""
    import numpy as np
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int32)
    n_seg = len(seg_off) - 1
    pairs = len(keys) if pairs is None else int(pairs)
    start = np.zeros((max(n_seg, 0), max(int(num_keys), 0) + 1), dtype=np.int32)
    out = np.zeros(max(pairs, 0), dtype=np.int32)
    L = lib()
    L.xv_bucket_sort.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                 ctypes.c_void_p, ctypes.c_void_p]
    _check(L.xv_bucket_sort(int(device), keys.ctypes.data, pairs, seg_off.ctypes.data, n_seg, int(num_keys), start.ctypes.data, out.ctypes.data))
    return start, out


def pack_mx_residual(w, w_hi_f16, segs, walk64=False):
    """e2m1 residual plane + E8M0 scales [n_pad, K / 32] (one per block of four K steps and lane group) of XV_PREC_FP16MX
    for one weight matrix (host; no GPU).
    w: float32 [n_pad, K]; w_hi_f16: uint16 [n_pad, K] (fp16 bit patterns); segs: [(source id, row shift, k_len)]."""
    import numpy as np
    w = np.ascontiguousarray(w, dtype=np.float32)
    hi = np.ascontiguousarray(w_hi_f16, dtype=np.uint16)
    n_pad, K = w.shape
    src = np.array([s[0] for s in segs], dtype=np.int32)
    shift = np.array([s[1] for s in segs], dtype=np.int32)
    klen = np.array([s[2] for s in segs], dtype=np.int32)
    assert int(klen.sum()) == K and K % 128 == 0
    w4 = np.zeros((n_pad, K // 128 * 64), dtype=np.uint8)
    sc = np.zeros((n_pad, K // 32), dtype=np.uint8)
    fn = lib().xv_pack_mx_residual64 if walk64 else lib().xv_pack_mx_residual   # walk64: the K order of tdnn_gemm_kernel_p8
    _check(fn(w.ctypes.data, hi.ctypes.data, n_pad, len(segs), src.ctypes.data, shift.ctypes.data,
              klen.ctypes.data, w4.ctypes.data, sc.ctypes.data))
    return w4, sc


def pack_mx_weights(w, segs, walk64=False):
    """4-bit image of a weight matrix for the second K walk of XV_PREC_FP16MX2 + its scales [n_pad, K / 32] (natural order).
    walk64: in the order of tdnn_gemm_kernel_p8's second walk, rows of 2 K bytes (GemmDesc.ldw4b = 2 K then)."""
    import numpy as np
    w = np.ascontiguousarray(w, dtype=np.float32)
    n_pad, K = w.shape
    src = np.array([s[0] for s in segs], dtype=np.int32)
    shift = np.array([s[1] for s in segs], dtype=np.int32)
    klen = np.array([s[2] for s in segs], dtype=np.int32)
    assert int(klen.sum()) == K and np.all(klen % (256 if walk64 else 128) == 0)
    w4b = np.zeros((n_pad, 2 * K if walk64 else K // 2), dtype=np.uint8)
    sc = np.zeros((n_pad, K // 32), dtype=np.uint8)
    fn = lib().xv_pack_mx_weights64 if walk64 else lib().xv_pack_mx_weights
    _check(fn(w.ctypes.data, n_pad, len(segs), src.ctypes.data, shift.ctypes.data, klen.ctypes.data, w4b.ctypes.data, sc.ctypes.data))
    return w4b, sc


def tile_mx_scales(scales, epilogue):
    """natural [n_pad, K / 32] scales of pack_mx_residual -> the staging order GemmDesc.w4_scale wants for `epilogue`."""
    import numpy as np
    sc = np.ascontiguousarray(scales, dtype=np.uint8)
    out = np.zeros(sc.size, dtype=np.uint8)
    _check(lib().xv_tile_mx_scales(sc.ctypes.data, sc.shape[0], sc.shape[1] * 32, int(epilogue), out.ctypes.data))
    return out
