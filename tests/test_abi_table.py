"""CPU tests of the package's one statement of the C ABI (_abi.py) against include/xvec_hip.h itself: every prototype's return type,
parameter count and parameter types, every mirrored struct's members, and the public names the package re-exports from its stage
modules.  Needs no library: only the header's text and the table."""
import ctypes
import importlib
import os
import re
import types

import helpers as H

P = H.pkg()
ABI = importlib.import_module(P.__name__ + "._abi")
HEADER = os.path.join(H.ROOT, "include", "xvec_hip.h")

SCALARS = {"int": ctypes.c_int, "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int16_t": ctypes.c_int16, "uint16_t": ctypes.c_uint16,
           "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double, "char": ctypes.c_char}
RETURNS = dict({k: SCALARS[k] for k in ("size_t", "int64_t", "uint64_t", "double")}, **{"xv_status": ctypes.c_int, "void": None,
                                                                                          "const char*": ctypes.c_char_p})
STRUCTS = {"xv_model_info_t": P.ModelInfo, "xv_seg_desc": P.SegDesc, "xv_gemm_desc": P.GemmDesc, "xv_gemm_plan_group": P.GemmPlanGroup,
           "xv_gemm_plan": P.GemmPlan, "xv_first_layer_desc": P.FirstLayerDesc, "xv_prep_input_desc": P.PrepInputDesc,
           "xv_pool_finalise_desc": P.PoolFinaliseDesc, "xv_frame_output_desc": P.FrameOutputDesc, "xv_calibration": P.Calibration,
           "xv_mfcc_options": P.MfccOptions, "xv_vad_options": P.VadOptions, "xv_reverb_options": P.ReverbOptions}
OPAQUE = ("xv_model", "xv_ctx", "xv_ubm", "xv_fgmm_acc", "xv_dgmm_acc", "xv_ivex", "xv_ivex_acc")


def _header():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """[(return type, name, [parameter declarations])]"""
    out = []
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\**)\s*\b(xv_\w+)\s*\(([^)]*)\)\s*;", _header()):
        params = params.strip()
        out.append((" ".join(ret.split()).replace(" *", "*"), name, [] if params in ("", "void") else [p.strip() for p in params.split(",")]))
    return out


def _declaration(decl):
    """'const int32_t* const* x' -> ('int32_t', 2): the base type and the number of stars"""
    m = re.match(r"^(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)\s*\w*$", " ".join(decl.split()))
    assert m, decl
    return m.group(1), m.group(2).count("*")


def _is_pointer_class(t):
    return isinstance(t, type) and issubclass(t, ctypes._Pointer)


def _pointer_matches(py, base, stars):
    """whether the ctypes class py may stand for a C parameter of `stars` >= 1 stars on `base`"""
    if py is ctypes.c_void_p:
        return True
    if py is ctypes.c_char_p:
        return base == "char" and stars == 1
    if not _is_pointer_class(py):
        return False
    pointee = py._type_
    if stars > 1:
        return _pointer_matches(pointee, base, stars - 1)
    if base in STRUCTS:
        return pointee is STRUCTS[base]
    return base in SCALARS and pointee is SCALARS[base]


def test_the_header_has_the_prototypes_the_table_lists_in_its_order():
    names = [name for _, name, _ in _prototypes()]
    assert len(names) == 136 and len(set(names)) == 136
    assert names == list(ABI.SIGNATURES) == P.ABI_SYMBOLS


def test_every_signature_matches_its_prototype():
    wrong = []
    for ret, name, params in _prototypes():
        restype, argtypes = ABI.SIGNATURES[name]
        if ret not in RETURNS or restype is not RETURNS[ret]:
            wrong.append("%s returns %s, the table says %r" % (name, ret, restype))
        if len(argtypes) != len(params):
            wrong.append("%s has %d parameters, the table %d" % (name, len(params), len(argtypes)))
            continue
        for i, (decl, py) in enumerate(zip(params, argtypes)):
            base, stars = _declaration(decl)
            assert base in SCALARS or base in STRUCTS or base in OPAQUE or base == "void", decl
            ok = _pointer_matches(py, base, stars) if stars else (base in SCALARS and py is SCALARS[base])
            if not ok:
                wrong.append("%s parameter %d `%s`: the table says %r" % (name, i, decl, py))
    assert not wrong, "\n".join(wrong)


def _struct_members(body):
    """'int32_t a, b; const void* p; xv_seg_desc seg[8];' -> [(name, base, is pointer, array length or 0)]"""
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"^(?:const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for item in m.group(3).split(","):
            a = re.match(r"^\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item)
            assert a, decl
            out.append((a.group(1), m.group(1), bool(m.group(2)), int(a.group(2) or 0)))
    return out


def test_every_struct_mirror_has_the_header_s_members():
    bodies = {name: body for body, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;", _header())}
    assert sorted(bodies) == sorted(STRUCTS)
    wrong = []
    for cname, py in STRUCTS.items():
        members = _struct_members(bodies[cname])
        if [m[0] for m in members] != [f[0] for f in py._fields_]:
            wrong.append("%s: members %s, the mirror has %s" % (cname, [m[0] for m in members], [f[0] for f in py._fields_]))
            continue
        for (name, base, pointer, length), (_, ftype) in zip(members, py._fields_):
            element = ctypes.c_void_p if pointer else STRUCTS.get(base) or SCALARS.get(base)
            assert element is not None, (cname, name, base)
            if length:
                ok = issubclass(ftype, ctypes.Array) and ftype._length_ == length and ftype._type_ is element
            else:
                ok = ftype is element
            if not ok:
                wrong.append("%s.%s: the header says %s%s%s, the mirror %r" % (cname, name, base, "*" if pointer else "",
                                                                                "[%d]" % length if length else "", ftype))
    assert not wrong, "\n".join(wrong)


# sorted(n for n in dir(package) if not n.startswith("_")) without the modules, as it was when the package was one file
PUBLIC_NAMES = """ABI_SYMBOLS BIN_DIR CSRC Calibration Context DgmmAccumulator EPI_ACT EPI_F32 EPI_STATS FgmmAccumulator FirstLayerDesc
FrameOutputDesc GemmDesc GemmPlan GemmPlanGroup IvectorExtractor IvexAccumulator LIB_PATH MFMA_PASSES MfccOptions Model ModelInfo
PRECISIONS PRECISION_NAMES PREC_AUTO PREC_BF16 PREC_BF16X3 PREC_DEFAULT PREC_FP16 PREC_FP16MX PREC_FP16MX2 PREC_FP16X2 PREC_FP16X3
PREC_FP16X3E PoolFinaliseDesc PrepInputDesc ReverbOptions SegDesc Ubm VadOptions WINDOW_TYPES Watchdog XV_ERR_ARG XV_ERR_DEVICE
XV_ERR_INTERNAL XV_ERR_IO XV_ERR_MODEL XV_OK XvError add_deltas apply_cmvn apply_cmvn_select backend_apply bucket_sort build
calibration_file_publish calibration_file_read cmvn_norm cmvn_sliding cmvn_stats compress compressed_size create_broadcast dgmm_est
fgmm_est fgmm_gconsts fgmm_init_from_accs fgmm_to_gmm ivex_est ivex_init ivex_rank_update ivex_read ivex_stats_read ivex_stats_write
ivex_write kernel_first_layer kernel_frame_output kernel_pool_finalise kernel_prep_input kernel_tdnn_gemm last_gemm_kernel
lda_estimate lib logprob_to_post logprob_to_post_kernel_time merge_vads mfcc mfcc_num_frames mfcc_options pack_mx_residual
pack_mx_weights plan_chunks plan_gemm plda_adapt plda_estimate plda_score plda_transform read_wave recognize_cmvn_pipeline
recognize_feature_pipeline recognize_wav_pipeline reverb_options reverb_output_length reverberate scatter_stats segment_mean
tile_mx_scales ubm_kernel_time utt_seed vad vad_from_frame_likes write_wave""".split()


def test_the_package_keeps_its_public_names():
    assert len(PUBLIC_NAMES) == 112
    names = sorted(n for n in dir(P) if not n.startswith("_") and not isinstance(getattr(P, n), types.ModuleType))
    assert names == sorted(PUBLIC_NAMES), sorted(set(names) ^ set(PUBLIC_NAMES))
    assert callable(P._check) and callable(P._segments)   # what tests and tools use of the private helpers
