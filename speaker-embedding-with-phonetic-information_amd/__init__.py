"""Host-side Python mirror of the C ABI in include/xvec_hip.h (ctypes; no torch types cross it).

The reference's interface for this path is a command line (Kaldi's `nnet3-xvector-compute`, call sites
egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:86-93); the product is the C++/HIP library
`libxvec_hip.so` plus the drop-in executables under bin/.  This package only exists so that tests/ and
bench.py can drive the same C ABI from Python; it contains no compute and no fallback: if the shared
library is missing or no gfx950 device is present, calls fail loudly.

_abi.py states the ABI once (constants, struct mirrors, every function's signature) and loads the library; the
other modules hold the wrappers, one module per stage of the C sources.  Every public name lives here, except those of
score normalisation and of nnet-am-compute, which came later and stay in their modules (asnorm, for include/xvec_hip_asnorm.h;
nnet2, for include/xvec_hip_nnet2.h).
"""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# XVEC_LIB: an alternative build of the same library (kernel experiments: tools/ab_libs.sh); never set in production
LIB_PATH = os.environ.get("XVEC_LIB") or os.path.join(_HERE, "libxvec_hip.so")
BIN_DIR = os.path.join(_HERE, "bin")

from ._abi import (ABI_SYMBOLS, EPI_ACT, EPI_F32, EPI_STATS, MFMA_PASSES, PREC_AUTO, PREC_BF16, PREC_BF16X3, PREC_DEFAULT,  # noqa: E402,F401
                   PREC_FP16, PREC_FP16MX, PREC_FP16MX2, PREC_FP16X2, PREC_FP16X3, PREC_FP16X3E, PRECISION_NAMES, PRECISIONS,
                   XV_ERR_ARG, XV_ERR_DEVICE, XV_ERR_INTERNAL, XV_ERR_IO, XV_ERR_MODEL, XV_OK, Calibration, FirstLayerDesc,
                   FrameOutputDesc, GemmDesc, GemmPlan, GemmPlanGroup, MfccOptions, ModelInfo, PoolFinaliseDesc, PrepInputDesc,
                   ReverbOptions, SegDesc, VadOptions, XvError, _check, lib)
from ._marshal import _segments  # noqa: E402,F401
from . import asnorm  # noqa: E402,F401  (score normalisation: a module of its own, as its header is)
from . import nnet2  # noqa: E402,F401  (nnet-am-compute: the same)
from .backend import (backend_apply, lda_estimate, plda_adapt, plda_estimate, plda_score, plda_transform, scatter_stats,  # noqa: E402,F401
                      segment_mean)
from .extractor import (Context, Model, Watchdog, calibration_file_publish, calibration_file_read, create_broadcast,  # noqa: E402,F401
                        plan_chunks, recognize_feature_pipeline)
from .frontend import (WINDOW_TYPES, add_deltas, apply_cmvn, apply_cmvn_select, cmvn_norm, cmvn_sliding, cmvn_stats, compress,  # noqa: E402,F401
                       compressed_size, mfcc, mfcc_num_frames, mfcc_options, read_wave, recognize_cmvn_pipeline,
                       recognize_wav_pipeline, reverb_options, reverb_output_length, reverberate, utt_seed, vad, write_wave)
from .ivector import (IvectorExtractor, IvexAccumulator, ivex_est, ivex_init, ivex_rank_update, ivex_read, ivex_stats_read,  # noqa: E402,F401
                      ivex_stats_write, ivex_write)
from .kernels import (bucket_sort, kernel_first_layer, kernel_frame_output, kernel_pool_finalise, kernel_prep_input,  # noqa: E402,F401
                      kernel_tdnn_gemm, last_gemm_kernel, pack_mx_residual, pack_mx_weights, plan_gemm, tile_mx_scales)
from .ubm import (DgmmAccumulator, FgmmAccumulator, Ubm, dgmm_est, fgmm_est, fgmm_gconsts, fgmm_init_from_accs, fgmm_to_gmm,  # noqa: E402,F401
                  logprob_to_post, logprob_to_post_kernel_time, merge_vads, ubm_kernel_time, vad_from_frame_likes)


def build(verbose=False):
    """Compile every HIP/C++ source for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError("building libxvec_hip.so failed")
    return LIB_PATH
