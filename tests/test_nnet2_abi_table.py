"""include/xvec_hip_nnet2.h against _abi.NNET2_SIGNATURES and _abi.Nnet2Info, as tests/test_abi_table.py holds the main table to
xvec_hip.h: every prototype's return type, parameter count and parameter types, the struct's members, and where the Python names
live.  Needs the header's text, the table and (for the exports) the built library; no GPU."""
import ctypes
import importlib
import os
import re

import helpers as H
import test_abi_table as T

P = H.pkg()
ABI = importlib.import_module(P.__name__ + "._abi")
NAMES = ["xv_nnet2_open", "xv_nnet2_close", "xv_nnet2_get_info", "xv_nnet2_plan", "xv_nnet2_compute", "xv_nnet2_compute_layers",
         "xv_nnet2_kernel_affine", "xv_nnet2_kernel_row", "xv_nnet2_kernel_head"]


def _header():
    text = open(os.path.join(H.ROOT, "include", "xvec_hip_nnet2.h")).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_the_table_of_the_companion_header_matches_its_prototypes():
    table = ABI.NNET2_SIGNATURES
    protos = re.findall(r"\b((?:const\s+)?\w+\s*\**)\s*\b(xv_\w+)\s*\(([^)]*)\)\s*;", _header())
    assert [name for _, name, _ in protos] == list(table) == NAMES
    assert not set(table) & set(P.ABI_SYMBOLS) and not set(table) & set(ABI.ASNORM_SIGNATURES) and all(hasattr(P.lib(), name) for name in table)
    for ret, name, params in protos:
        restype, argtypes = table[name]
        params = [p.strip() for p in params.split(",")]
        assert restype is T.RETURNS[" ".join(ret.split())] and len(argtypes) == len(params), name
        for decl, py in zip(params, argtypes):
            base, stars = T._declaration(decl)
            if base == "xv_nnet2":                       # the opaque handle: an address, or where one is written
                ok = (stars == 1 and py is ctypes.c_void_p) or (stars == 2 and py is ABI.PVP)
            elif base == "xv_nnet2_info_t":
                ok = stars == 1 and T._is_pointer_class(py) and py._type_ is ABI.Nnet2Info
            else:
                ok = T._pointer_matches(py, base, stars) if stars else py is T.SCALARS[base]
            assert ok, (name, decl, py)


def test_the_info_struct_mirrors_the_header():
    body = re.search(r"typedef\s+struct\s+xv_nnet2_info_t\s*\{([^}]*)\}\s*xv_nnet2_info_t\s*;", _header()).group(1)
    members = T._struct_members(body)
    assert [m[0] for m in members] == [f[0] for f in ABI.Nnet2Info._fields_]
    for (name, base, pointer, length), (_, ftype) in zip(members, ABI.Nnet2Info._fields_):
        assert not pointer and not length and ftype is T.SCALARS[base], name
    flags = dict(re.findall(r"#define\s+XV_NNET2_(\w+)\s+(\d+)", _header()))
    assert (int(flags["APPLY_LOG"]), int(flags["DIVIDE_BY_PRIORS"]), int(flags["PAD_INPUT"])) == (P.nnet2.APPLY_LOG, P.nnet2.DIVIDE_BY_PRIORS, P.nnet2.PAD_INPUT)


def test_the_python_names_live_in_their_module():
    for name in ("Nnet2", "plan", "kernel_affine", "kernel_row", "kernel_head"):
        assert callable(getattr(P.nnet2, name)) and not hasattr(P, name)
