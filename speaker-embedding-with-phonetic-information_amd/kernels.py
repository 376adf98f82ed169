"""Entry points of single kernels and of the host helpers their tests need: the GEMM and its planner, the frame-level and small
kernels, the counting sort, the MX packers."""
from ctypes import byref

import numpy as np

from ._abi import GemmPlan, _check, lib
from ._marshal import _f32, _i32


def kernel_tdnn_gemm(desc):
    _check(lib().xv_kernel_tdnn_gemm(byref(desc)))


def last_gemm_kernel():
    """Name of the kernel the calling thread's last kernel_tdnn_gemm launched, e.g. 'tdnn_gemm_kernel_sk<fp16x2,act,8>'."""
    return lib().xv_last_gemm_kernel().decode()


def plan_gemm(desc, cus=0, policy=None):
    """What kernel_tdnn_gemm(desc) would launch, without a device (csrc/gemm_plan.h): a GemmPlan.  cus > 0: a device of that many
    CUs under the default knobs, else the current device and XVEC_DEBUG.  policy: dict(variant, sk_mf, sk_lanes, stagger_pct) to
    state the knobs (missing ones at their defaults; needs cus > 0)."""
    out = GemmPlan()
    if policy is None:
        _check(lib().xv_plan_gemm(byref(desc), cus, byref(out)))
    else:
        k = dict(dict(variant=0, sk_mf=8, sk_lanes=4, stagger_pct=85), **policy)
        _check(lib().xv_plan_gemm_policy(byref(desc), cus, k["variant"], k["sk_mf"], k["sk_lanes"], k["stagger_pct"], byref(out)))
    return out


def kernel_first_layer(desc):
    _check(lib().xv_kernel_first_layer(byref(desc)))


def kernel_prep_input(desc):
    _check(lib().xv_kernel_prep_input(byref(desc)))


def kernel_pool_finalise(desc):
    _check(lib().xv_kernel_pool_finalise(byref(desc)))


def kernel_frame_output(desc):
    _check(lib().xv_kernel_frame_output(byref(desc)))


def bucket_sort(keys, seg_off, num_keys, device=0, pairs=None):
    """The stable counting sort by key of the UBM, GMM and i-vector statistics, inside every segment [seg_off[s], seg_off[s + 1])
    of keys (int32, each in [0, num_keys)).  Returns (bucket_start [segments, num_keys + 1], sorted [pairs]): absolute positions
    of the buckets and the pair indices, ascending inside a bucket.  pairs: len(keys) unless given."""
    keys, seg_off = _i32(keys), _i32(seg_off)
    n_seg = len(seg_off) - 1
    pairs = len(keys) if pairs is None else int(pairs)
    start = np.zeros((max(n_seg, 0), max(int(num_keys), 0) + 1), dtype=np.int32)
    out = np.zeros(max(pairs, 0), dtype=np.int32)
    _check(lib().xv_bucket_sort(int(device), keys.ctypes.data, pairs, seg_off.ctypes.data, n_seg, int(num_keys), start.ctypes.data, out.ctypes.data))
    return start, out


def _walk(segs):
    """[(source id, row shift, k_len)] -> the three int32 arrays of a K walk"""
    return [np.array([s[j] for s in segs], dtype=np.int32) for j in range(3)]


def pack_mx_residual(w, w_hi_f16, segs, walk64=False):
    """e2m1 residual plane + E8M0 scales [n_pad, K / 32] (one per block of four K steps and lane group) of XV_PREC_FP16MX
    for one weight matrix (host; no GPU).
    w: float32 [n_pad, K]; w_hi_f16: uint16 [n_pad, K] (fp16 bit patterns); segs: [(source id, row shift, k_len)]."""
    w = _f32(w)
    hi = np.ascontiguousarray(w_hi_f16, dtype=np.uint16)
    n_pad, K = w.shape
    src, shift, klen = _walk(segs)
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
    w = _f32(w)
    n_pad, K = w.shape
    src, shift, klen = _walk(segs)
    assert int(klen.sum()) == K and np.all(klen % (256 if walk64 else 128) == 0)
    w4b = np.zeros((n_pad, 2 * K if walk64 else K // 2), dtype=np.uint8)
    sc = np.zeros((n_pad, K // 32), dtype=np.uint8)
    fn = lib().xv_pack_mx_weights64 if walk64 else lib().xv_pack_mx_weights
    _check(fn(w.ctypes.data, n_pad, len(segs), src.ctypes.data, shift.ctypes.data, klen.ctypes.data, w4b.ctypes.data, sc.ctypes.data))
    return w4b, sc


def tile_mx_scales(scales, epilogue):
    """natural [n_pad, K / 32] scales of pack_mx_residual -> the staging order GemmDesc.w4_scale wants for `epilogue`."""
    sc = np.ascontiguousarray(scales, dtype=np.uint8)
    out = np.zeros(sc.size, dtype=np.uint8)
    _check(lib().xv_tile_mx_scales(sc.ctypes.data, sc.shape[0], sc.shape[1] * 32, int(epilogue), out.ctypes.data))
    return out
