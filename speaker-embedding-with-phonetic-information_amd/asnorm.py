"""Adaptive score normalisation (include/xvec_hip_asnorm.h): the PLDA ratio of all pairs of two tables, the
statistics of each row's N largest scores, the two fused, and the plan of the fused path.  Reached as <package>.asnorm.<name>."""
import ctypes
from ctypes import byref

import numpy as np

from ._abi import _check, lib
from ._marshal import _f32, _f64, _ptr_or_null, _require


def plda_score_dense(u, num_u, v, psi, device=0, return_ms=False):
    """plda_score for EVERY pair, as one fp64 matrix product on the device: float64 [n_u, n_v], element [i, j] the ratio of
    enrolment row i (mean of num_u[i] examples) against test row j.  A score depends on its pair and psi alone: the same
    bits wherever the pair sits in whichever tables."""
    u, v, num_u, ps = _f32(u), _f32(v), _f64(num_u), _f64(psi)
    _require(u.ndim == 2 and v.ndim == 2 and u.shape[1] == v.shape[1] and ps.shape == (u.shape[1],) and num_u.shape == (u.shape[0],),
             "dense PLDA scoring: the shapes do not agree")
    scores = np.empty((u.shape[0], v.shape[0]), np.float64)
    ms = ctypes.c_float(0)
    _check(lib().xv_plda_score_dense(device, _ptr_or_null(u), _ptr_or_null(num_u), u.shape[0], _ptr_or_null(v), v.shape[0], u.shape[1],
                                     ps.ctypes.data, _ptr_or_null(scores), byref(ms)))
    return (scores, ms.value) if return_ms else scores


def topn_stats(scores, n, device=0, return_ms=False):
    """Per row of scores [rows, cols] (finite float64) on the device: (mean, std) of its n largest values, selected exactly
    (among values equal to the n-th largest: the lowest columns); std is the population standard deviation, two-pass."""
    x = _f64(scores)
    _require(x.ndim == 2, "top-N statistics: scores must be a matrix")
    mean, std = np.empty(x.shape[0]), np.empty(x.shape[0])
    ms = ctypes.c_float(0)
    _check(lib().xv_topn_stats(device, _ptr_or_null(x), x.shape[0], x.shape[1], n, _ptr_or_null(mean), _ptr_or_null(std), byref(ms)))
    return (mean, std, ms.value) if return_ms else (mean, std)


def plda_cohort_stats(u, num_u, v, psi, n, by_column=False, device=0, return_ms=False):
    """topn_stats(plda_score_dense(u, num_u, v, psi), n) without the matrix leaving the device, bit for bit; with by_column
    the statistics of the transposed matrix (one per row of v, over all rows of u).  Returns (mean, std)."""
    u, v, num_u, ps = _f32(u), _f32(v), _f64(num_u), _f64(psi)
    _require(u.ndim == 2 and v.ndim == 2 and u.shape[1] == v.shape[1] and ps.shape == (u.shape[1],) and num_u.shape == (u.shape[0],),
             "PLDA cohort statistics: the shapes do not agree")
    rows = v.shape[0] if by_column else u.shape[0]
    mean, std = np.empty(rows), np.empty(rows)
    ms = ctypes.c_float(0)
    _check(lib().xv_plda_cohort_stats(device, _ptr_or_null(u), _ptr_or_null(num_u), u.shape[0], _ptr_or_null(v), v.shape[0], u.shape[1],
                                      ps.ctypes.data, 1 if by_column else 0, n, _ptr_or_null(mean), _ptr_or_null(std), byref(ms)))
    return (mean, std, ms.value) if return_ms else (mean, std)


def plda_dense_plan(rows, cols, dim, workspace_bytes=0):
    """How the dense scoring passes a rows x cols score matrix through a device workspace of at most workspace_bytes (0: the
    default): (rows_per_chunk, n_chunks, chunk_bytes).  Host only, no GPU needed."""
    rpc, nc, cb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _check(lib().xv_plda_dense_plan(rows, cols, dim, workspace_bytes, byref(rpc), byref(nc), byref(cb)))
    return rpc.value, nc.value, cb.value
