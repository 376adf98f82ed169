"""nnet-am-compute (include/xvec_hip_nnet2.h): the forward pass of an nnet2 acoustic model - the senone posteriors
of the DNN i-vector path -, its block plan, and one launch each of its three kernels.  Reached as <package>.nnet2.<name>."""
import ctypes
from ctypes import byref

import numpy as np

from ._abi import Nnet2Info, _check, _Handle, lib
from ._marshal import _f32, _i32, _pack_matrices, _ptr_or_null, _require, _split

APPLY_LOG, DIVIDE_BY_PRIORS, PAD_INPUT = 1, 2, 4
NONLIN = {"none": 0, "pnorm": 1, "relu": 2}
LO_SCALE = 2048.0   # a plane pair stands for hi + lo / LO_SCALE


def _info_dict(info):
    return {name: int(getattr(info, name)) for name, _ in Nnet2Info._fields_}


def plan(info, rows, block_rows=0, workspace_bytes=0):
    """How a packed sequence of `rows` rows passes through the device workspace: (rows_per_block, n_blocks, bytes).  info: the dict
    Nnet2.info gives, or one with the same keys.  Host only, no GPU needed."""
    c = Nnet2Info(**{k: int(v) for k, v in info.items()})
    rpb, nb, nbytes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _check(lib().xv_nnet2_plan(byref(c), rows, block_rows, workspace_bytes, byref(rpb), byref(nb), byref(nbytes)))
    return rpb.value, nb.value, nbytes.value


class Nnet2(_Handle):
    """An nnet2 acoustic model (final.mdl, binary or text).  Opening it needs no GPU; compute() does."""
    _destroy = "xv_nnet2_close"

    def __init__(self, rxfilename):
        h = ctypes.c_void_p()
        _check(lib().xv_nnet2_open(str(rxfilename).encode(), byref(h)))
        self._h = h
        c = Nnet2Info()
        _check(lib().xv_nnet2_get_info(self._h, byref(c)))
        self.info = _info_dict(c)

    def out_rows(self, t, pad_input=True):
        if t <= 0:
            return 0
        return t if pad_input else max(0, t - self.info["left_context"] - self.info["right_context"])

    def compute(self, utts, apply_log=False, divide_by_priors=False, pad_input=True, block_rows=0, device=0, return_ms=False, layers=False):
        """One [T_u, output_dim] float32 matrix per utterance (no rows for an utterance that is empty or, without pad_input,
        shorter than the context).  layers: the third value is the device time of every layer and, last, of the head."""
        feats, off, cols = _pack_matrices(utts, "nnet2 compute")
        _require(cols in (0, self.info["input_dim"]), "nnet2 compute: the features have %d columns, the model takes %d" % (cols, self.info["input_dim"]))
        flags = (APPLY_LOG if apply_log else 0) | (DIVIDE_BY_PRIORS if divide_by_priors else 0) | (PAD_INPUT if pad_input else 0)
        out_off = np.zeros(len(off), np.int64)
        out_off[1:] = np.cumsum([self.out_rows(int(off[u + 1] - off[u]), pad_input) for u in range(len(off) - 1)])
        out = np.empty((int(out_off[-1]), self.info["output_dim"]), np.float32)
        if layers:
            ms = np.zeros(self.info["num_layers"] + 1, np.float32)
            _check(lib().xv_nnet2_compute_layers(self._h, device, _ptr_or_null(feats), off.ctypes.data, len(off) - 1, flags, block_rows,
                                                 _ptr_or_null(out), ms.ctypes.data))
            return _split(out, out_off), ms
        ms = ctypes.c_float(0)
        _check(lib().xv_nnet2_compute(self._h, device, _ptr_or_null(feats), off.ctypes.data, len(off) - 1, flags, block_rows, _ptr_or_null(out),
                                      byref(ms) if return_ms else None))
        res = _split(out, out_off)
        return (res, ms.value) if return_ms else res


def kernel_affine(x, context, w, bias, device=0):
    """One launch of the spliced affine: out[t] = bias + sum_c w[:, c k:(c + 1) k] x[t + context[c]], rows outside x reading as
    zero.  x [rows, k], w [n, len(context) k]."""
    x, w, b, ctx = _f32(x), _f32(w), _f32(bias), _i32(context)
    _require(x.ndim == 2 and w.ndim == 2 and ctx.ndim == 1 and w.shape[1] == ctx.size * x.shape[1] and b.shape == (w.shape[0],),
             "nnet2 affine: the shapes do not agree")
    out = np.empty((x.shape[0], w.shape[0]), np.float32)
    _check(lib().xv_nnet2_kernel_affine(device, _ptr_or_null(x), x.shape[0], x.shape[1], _ptr_or_null(ctx), ctx.size, _ptr_or_null(w),
                                        _ptr_or_null(b), w.shape[0], _ptr_or_null(out)))
    return out


def kernel_row(pre, out_dim, nonlin="none", normalize=False, device=0, planes=False):
    """One launch of the row kernel on pre [rows, in_dim]: the values the two fp16 planes stand for, float64 [rows, out_dim]
    (planes: the raw (hi, lo) uint16 arrays [rows, ld] instead)."""
    x = _f32(pre)
    _require(x.ndim == 2, "nnet2 row kernel: pre must be a matrix")
    ld = -(-out_dim // 32) * 32
    hi, lo = np.empty((x.shape[0], ld), np.uint16), np.empty((x.shape[0], ld), np.uint16)
    _check(lib().xv_nnet2_kernel_row(device, _ptr_or_null(x), x.shape[0], x.shape[1], out_dim, NONLIN[nonlin], 1 if normalize else 0,
                                     _ptr_or_null(hi), _ptr_or_null(lo)))
    if planes:
        return hi, lo
    return (hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64) / LO_SCALE)[:, :out_dim]


def kernel_head(logits, sizes=None, priors=None, apply_log=False, device=0):
    """One launch of the head on logits [rows, n]: softmax, group sums, priors, log."""
    x = _f32(logits)
    _require(x.ndim == 2, "nnet2 head: logits must be a matrix")
    sz = None if sizes is None else _i32(sizes)
    n_out = x.shape[1] if sz is None else sz.size
    pr = None if priors is None else _f32(priors)
    _require(pr is None or pr.shape == (n_out,), "nnet2 head: one prior per output")
    out = np.empty((x.shape[0], n_out), np.float32)
    _check(lib().xv_nnet2_kernel_head(device, _ptr_or_null(x), x.shape[0], x.shape[1], None if sz is None else sz.ctypes.data,
                                      0 if sz is None else sz.size, None if pr is None else pr.ctypes.data, 1 if apply_log else 0,
                                      _ptr_or_null(out)))
    return out
