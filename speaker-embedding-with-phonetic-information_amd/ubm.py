"""The GMM-UBM stage: models on the device, selection and posteriors, the GMM classifiers, diagonal and full-covariance training."""
import ctypes
from ctypes import byref

import numpy as np

from ._abi import _check, _Handle, lib
from ._marshal import _f32, _f64, _full_gmm, _i32, _ms, _pack_matrices, _ptr, _ptr_or_null, _require, _selection, _split


def fgmm_to_gmm(weights, means_invcovars, inv_covars):
    """fgmm-global-to-gmm on the host in fp64: weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2] (packed lower
    triangles) -> (gconsts [G], means_invvars [G][D], inv_vars [G][D]) of the diagonal image."""
    w, b, ic = _full_gmm(weights, means_invcovars, inv_covars, "fgmm_to_gmm")
    g, d = b.shape
    gc, mi, iv = np.zeros(g, np.float32), np.zeros((g, d), np.float32), np.zeros((g, d), np.float32)
    _check(lib().xv_fgmm_to_gmm(g, d, w.ctypes.data, b.ctypes.data, ic.ctypes.data, gc.ctypes.data, mi.ctypes.data, iv.ctypes.data))
    return gc, mi, iv


def fgmm_gconsts(weights, means_invcovars, inv_covars):
    """The gconsts the tools recompute after they read a full model (xv_fgmm_gconsts: fp64 on the host, stored as float32)."""
    w, b, ic = _full_gmm(weights, means_invcovars, inv_covars, "fgmm_gconsts")
    gc = np.zeros(b.shape[0], np.float32)
    _check(lib().xv_fgmm_gconsts(b.shape[0], b.shape[1], w.ctypes.data, b.ctypes.data, ic.ctypes.data, gc.ctypes.data, None))
    return gc


class Ubm(_Handle):
    """A GMM on one device, uploaded once (xv_ubm_diag_create / xv_ubm_full_create).  Ubm.diag(gconsts, means_invvars, inv_vars)
    selects Gaussians; Ubm.full(gconsts, means_invcovars, inv_covars_packed) turns a selection into posteriors."""
    _destroy = "xv_ubm_destroy"

    def __init__(self, handle, num_gauss, dim, full):
        self._h, self.num_gauss, self.dim, self.is_full = handle, num_gauss, dim, full

    @classmethod
    def _create(cls, fn_name, device, gconsts, a, b, full):
        gc, a, b = _f32(gconsts), _f32(a), _f32(b)
        _require(a.ndim == 2 and gc.shape == (a.shape[0],), "Ubm: gconsts [G] and a [G][D] matrix")
        g, d = a.shape
        _require(b.shape == ((g, d * (d + 1) // 2) if full else (g, d)), "Ubm: the second matrix does not have the model's shape")
        h = ctypes.c_void_p()
        _check(getattr(lib(), fn_name)(device, g, d, gc.ctypes.data, a.ctypes.data, b.ctypes.data, byref(h)))
        return cls(h, g, d, full)

    @classmethod
    def diag(cls, gconsts, means_invvars, inv_vars, device=0):
        return cls._create("xv_ubm_diag_create", device, gconsts, means_invvars, inv_vars, False)

    @classmethod
    def full(cls, gconsts, means_invcovars, inv_covars, device=0):
        return cls._create("xv_ubm_full_create", device, gconsts, means_invcovars, inv_covars, True)

    def _feats(self, who, feats_list):
        packed, off, cols = _pack_matrices(feats_list, who)
        _require(cols == self.dim, "%s: the features have %d columns, the model %d" % (who, cols, self.dim))
        return packed, off, len(off) - 1

    def gselect(self, feats_list, n, return_loglikes=False):
        """The n best Gaussians per frame, best first: a list of int32 [frames, n] (and of float32 log-likelihoods)."""
        packed, off, nu = self._feats("gselect", feats_list)
        rows = packed.shape[0]
        idx = np.zeros((rows, max(n, 1)), dtype=np.int32)
        ll = np.zeros((rows, max(n, 1)), dtype=np.float32)
        _check(lib().xv_ubm_gselect(self._h, packed.ctypes.data, off.ctypes.data, nu, n, idx.ctypes.data,
                                    ll.ctypes.data if return_loglikes else None, None))
        return (_split(idx, off), _split(ll, off)) if return_loglikes else _split(idx, off)

    def post(self, feats_list, gselect_list, min_post=0.0, return_details=False):
        """Posteriors over the selected Gaussians: per utterance a list (one entry per frame) of (int32 indices, float32
        posteriors).  return_details: also the lists of log-likelihoods [frames, n] and of per-frame log-sums [frames]."""
        packed, off, nu = self._feats("post", feats_list)
        sel, n = _selection(gselect_list, off, "post")
        rows = packed.shape[0]
        count = np.zeros(rows, dtype=np.int32)
        idx = np.zeros((rows, n), dtype=np.int32)
        post = np.zeros((rows, n), dtype=np.float32)
        ll = np.zeros((rows, n), dtype=np.float32)
        logsum = np.zeros(rows, dtype=np.float32)
        _check(lib().xv_ubm_post(self._h, packed.ctypes.data, off.ctypes.data, nu, sel.ctypes.data, n, float(min_post), count.ctypes.data,
                                 idx.ctypes.data, post.ctypes.data, ll.ctypes.data, logsum.ctypes.data, None))
        out = [[(idx[t, :count[t]].copy(), post[t, :count[t]].copy()) for t in range(off[u], off[u + 1])] for u in range(nu)]
        return (out, _split(ll, off), _split(logsum, off)) if return_details else out

    def rerank(self, feats_list, gselect_list, n, return_loglikes=False, return_ms=False):
        """Second-stage selection by a full model (fgmm-gselect --gselect=): the min(n, n_in) best of every frame's preselection,
        best first, as a list of int32 [frames, min(n, n_in)] (and of the float32 log-likelihoods; return_ms: and the device
        times {sort, scores, rerank} in ms)."""
        packed, off, nu = self._feats("rerank", feats_list)
        _require(gselect_list is not None, "rerank: a preselection is needed")
        sel, n_in = _selection(gselect_list, off, "rerank")
        keep = max(1, min(n, n_in))
        rows = packed.shape[0]
        idx = np.zeros((rows, keep), dtype=np.int32)
        ll = np.zeros((rows, keep), dtype=np.float32)
        ms = (ctypes.c_float * 3)()
        _check(lib().xv_ubm_full_gselect(self._h, packed.ctypes.data, off.ctypes.data, nu, sel.ctypes.data, n_in, n, idx.ctypes.data,
                                         ll.ctypes.data if return_loglikes else None, ms if return_ms else None))
        out = [_split(idx, off)]
        if return_loglikes:
            out.append(_split(ll, off))
        if return_ms:
            out.append(_ms(("sort", "full", "rerank"), ms))
        return out[0] if len(out) == 1 else tuple(out)

    def frame_likes(self, feats_list, gselect_list=None, average=False):
        """Per-frame log-likelihoods of a full model over each frame's selection (fgmm-global-get-frame-likes): a list of float32
        [frames].  gselect_list None: every component, for models of at most 64.  average: one float32 per utterance instead, the
        frames summed in float64 in frame order, divided by their number and rounded once."""
        packed, off, nu = self._feats("frame_likes", feats_list)
        sel, n = (None, 0) if gselect_list is None else _selection(gselect_list, off, "frame_likes")
        likes = np.zeros(packed.shape[0], dtype=np.float32)
        _check(lib().xv_ubm_frame_likes(self._h, packed.ctypes.data, off.ctypes.data, nu, _ptr(sel), n, likes.ctypes.data, None))
        per_utt = _split(likes, off)
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
    cls = [_f32(v) for v in likes]
    _require(cls and all(v.ndim == 1 and v.shape == cls[0].shape for v in cls),
             "vad_from_frame_likes: one [frames] array per class, all of one length")
    n = len(cls)
    pr = None if priors is None else _f32(priors)
    mp = None if map is None else _i32(map)
    _require((pr is None or pr.shape == (n,)) and (mp is None or mp.shape == (n,)),
             "vad_from_frame_likes: %d classes need %d priors and %d map entries" % (n, n, n))
    ptrs = (ctypes.c_void_p * n)(*[v.ctypes.data for v in cls])
    out = np.zeros(cls[0].shape[0], dtype=np.float32)
    _check(lib().xv_vad_from_frame_likes(n, ptrs, out.shape[0], _ptr(pr), _ptr(mp), out.ctypes.data))
    return out


def merge_vads(a, b, map=None):
    """merge-vads on the host: 1 where both are 1 without a map; with a map, a sequence of (a, b, c) triples, the pair (a, b)
    gives c and a pair that is not in the map is an error that names it."""
    a, b = _f32(a), _f32(b)
    _require(a.ndim == 1 and a.shape == b.shape, "merge_vads: two [frames] arrays of one length")
    tri = np.zeros((0, 3), dtype=np.int32) if map is None else _i32(map).reshape(-1, 3)
    out = np.zeros(a.shape[0], dtype=np.float32)
    _check(lib().xv_merge_vads(a.ctypes.data, b.ctypes.data, a.shape[0], _ptr_or_null(tri), len(tri), out.ctypes.data))
    return out


def ubm_kernel_time(diag, full, feats_list, n=20, min_post=0.025, reps=5):
    """{deltas, gselect, sort, full, softmax} kernel times in ms of one batch (xv_ubm_kernel_time: the best of reps)."""
    packed, off, cols = _pack_matrices(feats_list, "ubm_kernel_time")
    ms = (ctypes.c_float * 5)()
    _check(lib().xv_ubm_kernel_time(diag._h, full._h, packed.ctypes.data, off.ctypes.data, len(off) - 1, n, float(min_post), reps, ms))
    return _ms(("deltas", "gselect", "sort", "full", "softmax"), ms)


class _GmmAccumulator(_Handle):
    """What the fp64 accumulators of diagonal and full-covariance UBM training share.  A subclass names its functions' prefix and
    gives the columns of the third array of get() in _second_width(dim)."""
    _prefix = None

    def __init__(self, num_gauss, dim, flags="mvw", device=0):
        self._h = ctypes.c_void_p()
        self.num_gauss, self.dim, self.flags = int(num_gauss), int(dim), flags
        _check(self._fn("create")(device, self.num_gauss, self.dim, flags.encode(), byref(self._h)))

    def _fn(self, what):
        return getattr(lib(), self._prefix + what)

    def _feats(self, feats, who):
        x = _f32(feats)
        _require(x.ndim == 2 and x.shape[1] == self.dim, "%s: the features are not [frames, %d]" % (who, self.dim))
        return x

    def _gselect(self, feats, gselect):
        x = self._feats(feats, "accumulate_gselect")
        gs = _i32(gselect)
        _require(gs.ndim == 2 and gs.shape[0] == x.shape[0], "accumulate_gselect: a [frames, n] selection")
        return x, gs

    def accumulate(self, feats, post):
        """One call: feats [frames, D]; post: per frame (indices, posteriors), as Ubm.post returns them for one utterance.  The
        accumulator kernels alone."""
        x = self._feats(feats, "accumulate")
        _require(len(post) == x.shape[0], "accumulate: one (indices, posteriors) pair per frame")
        off = np.zeros(x.shape[0] + 1, dtype=np.int32)
        for t, (i, _) in enumerate(post):
            off[t + 1] = off[t] + len(i)
        idx = _i32(np.concatenate([np.asarray(i, np.int32) for i, _ in post]) if len(post) else np.zeros(0))
        w = _f32(np.concatenate([np.asarray(p, np.float32) for _, p in post]) if len(post) else np.zeros(0))
        _check(self._fn("add")(self._h, x.ctypes.data, x.shape[0], off.ctypes.data, idx.ctypes.data, w.ctypes.data))

    def get(self):
        """(occ [G], mean [G, D], and cov [G, D (D + 1) / 2] or var [G, D]) as float64."""
        g, d = self.num_gauss, self.dim
        occ, mean, second = np.zeros(g), np.zeros((g, d)), np.zeros((g, self._second_width(d)))
        _check(self._fn("get")(self._h, occ.ctypes.data, mean.ctypes.data, second.ctypes.data))
        return occ, mean, second


class FgmmAccumulator(_GmmAccumulator):
    """The fp64 accumulators of full-covariance UBM training on one device (xv_fgmm_acc_create): occ [G], mean [G][D] and the packed
    lower triangles cov [G][D (D + 1) / 2].  flags: letters of "mvw" (v implies m, m implies w)."""
    _prefix, _destroy = "xv_fgmm_acc_", "xv_fgmm_acc_destroy"

    @staticmethod
    def _second_width(d):
        return d * (d + 1) // 2

    def accumulate_gselect(self, full, feats, gselect):
        """The fused E-step: the posteriors of full.post(min_post=0) over gselect [frames, n] never leave the device.  Returns the
        per-frame log-sums, float32 [frames]."""
        x, gs = self._gselect(feats, gselect)
        logsum = np.zeros(x.shape[0], dtype=np.float32)
        _check(lib().xv_fgmm_acc_add_gselect(self._h, full._h, x.ctypes.data, x.shape[0], gs.ctypes.data, gs.shape[1], logsum.ctypes.data))
        return logsum

    def kernel_time(self, full, feats, gselect, reps=5):
        """{sort, full, softmax, acc} kernel times in ms of one fused call (xv_fgmm_acc_kernel_time: the best of reps).  Every run adds
        to the accumulators."""
        x = self._feats(feats, "kernel_time")
        gs = _i32(gselect)
        ms = (ctypes.c_float * 4)()
        _check(lib().xv_fgmm_acc_kernel_time(self._h, full._h, x.ctypes.data, x.shape[0], gs.ctypes.data, gs.shape[1], reps, ms))
        return _ms(("sort", "full", "softmax", "acc"), ms)


class DgmmAccumulator(_GmmAccumulator):
    """The fp64 accumulators of diagonal UBM training on one device (xv_dgmm_acc_create): occ [G], mean [G][D] and var [G][D] (the sums
    of p x x).  flags: letters of "mvw" (v implies m, m implies w)."""
    _prefix, _destroy = "xv_dgmm_acc_", "xv_dgmm_acc_destroy"

    @staticmethod
    def _second_width(d):
        return d

    def accumulate_gselect(self, diag, feats, gselect, return_loglikes=False):
        """The fused sparse E-step on a diagonal Ubm over gselect [frames, n].  Returns the per-frame log-sums, float32 [frames] (and
        the scores [frames, n])."""
        x, gs = self._gselect(feats, gselect)
        logsum = np.zeros(x.shape[0], dtype=np.float32)
        ll = np.zeros(gs.shape, dtype=np.float32)
        _check(lib().xv_dgmm_acc_add_gselect(self._h, diag._h, x.ctypes.data, x.shape[0], gs.ctypes.data, gs.shape[1],
                                             ll.ctypes.data if return_loglikes else None, logsum.ctypes.data))
        return (logsum, ll) if return_loglikes else logsum

    def accumulate_dense_post(self, feats, post):
        """A caller's dense posteriors [frames, G] through the matrix-core accumulation kernel alone."""
        x = self._feats(feats, "accumulate_dense_post")
        p = _f32(post)
        _require(p.shape == (x.shape[0], self.num_gauss), "accumulate_dense_post: posteriors [frames, %d]" % self.num_gauss)
        _check(lib().xv_dgmm_acc_add_dense_post(self._h, x.ctypes.data, x.shape[0], p.ctypes.data))

    def accumulate_dense(self, diag, feats):
        """The fused dense E-step: every frame against every Gaussian of a diagonal Ubm.  Returns the per-frame log-sums."""
        x = self._feats(feats, "accumulate_dense")
        logsum = np.zeros(x.shape[0], dtype=np.float32)
        _check(lib().xv_dgmm_acc_add_dense(self._h, diag._h, x.ctypes.data, x.shape[0], logsum.ctypes.data))
        return logsum

    def kernel_time(self, diag, feats, gselect=None, dense=True, reps=3):
        """{sort, scores, softmax, acc} of one fused sparse call (with gselect) and {dense_logsum, dense_acc, dense_reduce} of one fused
        dense call, in ms (xv_dgmm_acc_kernel_time: the best of reps).  Every run adds to the accumulators."""
        x = self._feats(feats, "kernel_time")
        gs = None if gselect is None else _i32(gselect)
        ms = (ctypes.c_float * 7)()
        _check(lib().xv_dgmm_acc_kernel_time(self._h, diag._h, x.ctypes.data, x.shape[0], _ptr(gs), 0 if gs is None else gs.shape[1],
                                             int(bool(dense)), reps, ms))
        return _ms(("sort", "scores", "softmax", "acc", "dense_logsum", "dense_acc", "dense_reduce"), ms)


def fgmm_est(weights, means_invcovars, inv_covars, occ, mean, cov, acc_flags="mvw", update_flags="mvw", min_gaussian_weight=1e-5,
             min_gaussian_occupancy=100.0, variance_floor=0.001, max_condition=1e5, remove_low_count_gaussians=True):
    """The M-step of fgmm-global-est on host arrays (xv_fgmm_est, fp64): dict(weights, means_invcovars, inv_covars, gconsts) of the
    Gaussians that survive, removed (indices), floored (eigenvalues, Gaussians), objf_before, objf_after, count."""
    w, b, ic = (a.copy() for a in _full_gmm(weights, means_invcovars, inv_covars, "fgmm_est"))   # the call updates them in place
    g, d = b.shape
    o, m, c = _f64(occ), _f64(mean), _f64(cov)
    _require(o.shape == (g,) and m.shape == (g, d) and c.shape == ic.shape, "fgmm_est: occ [G], mean [G][D], cov [G][D (D + 1) / 2]")
    gc = np.zeros(g, np.float32)
    removed = np.zeros(g, np.int32)
    floored = np.zeros(2, np.int32)
    objf = np.zeros(3)
    left = ctypes.c_int32()
    _check(lib().xv_fgmm_est(g, d, acc_flags.encode(), o.ctypes.data, m.ctypes.data, c.ctypes.data, update_flags.encode(), min_gaussian_weight,
                             min_gaussian_occupancy, variance_floor, max_condition, int(bool(remove_low_count_gaussians)), w.ctypes.data,
                             b.ctypes.data, ic.ctypes.data, gc.ctypes.data, byref(left), removed.ctypes.data, floored.ctypes.data,
                             objf.ctypes.data))
    k = left.value
    return dict(weights=w[:k].copy(), means_invcovars=b[:k].copy(), inv_covars=ic[:k].copy(), gconsts=gc[:k].copy(),
                removed=removed[:g - k].tolist(), floored=(int(floored[0]), int(floored[1])), objf_before=float(objf[0]),
                objf_after=float(objf[1]), count=float(objf[2]))


def logprob_to_post(logprobs_list, keys, min_post=0.01, random_prune=True, frame_budget=0, device=0, return_details=False):
    """logprob-to-post on the device (xv_logprob_to_post): per utterance a list (one entry per row) of (int32 columns, float32
    weights), columns ascending.  keys: the utterance keys, which key the random pruning.  frame_budget: rows per launch (0: the
    default); the result does not depend on it.  return_details: also dict(num_nan, ms=(count, scan, write))."""
    packed, off, cols = _pack_matrices(logprobs_list, "logprob_to_post")
    nu, rows = len(off) - 1, packed.shape[0]
    _require(len(keys) == nu, "logprob_to_post: one key per matrix")
    if rows == 0:
        out = [[] for _ in range(nu)]
        return (out, dict(num_nan=0, ms=(0.0, 0.0, 0.0))) if return_details else out
    ckeys = (ctypes.c_char_p * max(nu, 1))(*[k.encode() for k in keys])
    pair_off = np.zeros(rows + 1, dtype=np.int64)
    need, num_nan = ctypes.c_int64(0), ctypes.c_int64(0)
    ms = (ctypes.c_float * 3)()
    capacity = min(rows * cols, max(1 << 16, rows * 64))
    while True:
        idx = np.zeros(capacity, dtype=np.int32)
        w = np.zeros(capacity, dtype=np.float32)
        _check(lib().xv_logprob_to_post(device, packed.ctypes.data, off.ctypes.data, nu, cols, ckeys, float(min_post), int(bool(random_prune)),
                                        int(frame_budget), capacity, pair_off.ctypes.data, idx.ctypes.data, w.ctypes.data, byref(need),
                                        byref(num_nan), ms))
        if need.value <= capacity:
            break
        capacity = need.value
    out = [[(idx[pair_off[t]:pair_off[t + 1]].copy(), w[pair_off[t]:pair_off[t + 1]].copy()) for t in range(off[u], off[u + 1])] for u in range(nu)]
    return (out, dict(num_nan=int(num_nan.value), ms=tuple(float(v) for v in ms))) if return_details else out


def logprob_to_post_kernel_time(logprobs, key="utt", min_post=0.01, random_prune=True, reps=5, device=0):
    """{count, scan, write, copy} times in ms of one rows x cols matrix in one launch (xv_logprob_to_post_kernel_time: the best of
    reps).  copy: a device-to-device copy of the input, which is what two reads of it cost at the copy bandwidth of this run."""
    x = _f32(logprobs)
    _require(x.ndim == 2, "logprob_to_post_kernel_time: a [rows, cols] matrix")
    ms = (ctypes.c_float * 4)()
    _check(lib().xv_logprob_to_post_kernel_time(device, x.ctypes.data, x.shape[0], x.shape[1], key.encode(), float(min_post),
                                                int(bool(random_prune)), reps, ms))
    return _ms(("count", "scan", "write", "copy"), ms)


def fgmm_init_from_accs(occ, mean, cov, remove_low_count_gaussians=True):
    """fgmm-global-init-from-accs on host arrays (xv_fgmm_init_from_accs, fp64): dict(weights, means_invcovars, inv_covars, gconsts) of
    the Gaussians that survive, removed (indices), bad_gconsts, and inv_covars_f64: the survivors' inverse covariances before they are
    rounded to float32."""
    o, m, c = _f64(occ), _f64(mean), _f64(cov)
    _require(m.ndim == 2 and o.shape == (m.shape[0],) and c.shape == (m.shape[0], m.shape[1] * (m.shape[1] + 1) // 2),
             "fgmm_init_from_accs: occ [G], mean [G][D], cov [G][D (D + 1) / 2]")
    g, d = m.shape
    w, b, ic, gc = np.zeros(g, np.float32), np.zeros((g, d), np.float32), np.zeros(c.shape, np.float32), np.zeros(g, np.float32)
    removed = np.zeros(g, np.int32)
    ic64 = np.zeros(c.shape, np.float64)
    left, bad = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().xv_fgmm_init_from_accs(g, d, o.ctypes.data, m.ctypes.data, c.ctypes.data, int(bool(remove_low_count_gaussians)), w.ctypes.data,
                                        b.ctypes.data, ic.ctypes.data, gc.ctypes.data, byref(left), removed.ctypes.data, byref(bad),
                                        ic64.ctypes.data))
    k = left.value
    gone = removed[:g - k].tolist()
    return dict(weights=w[:k].copy(), means_invcovars=b[:k].copy(), inv_covars=ic[:k].copy(), gconsts=gc[:k].copy(), removed=gone,
                bad_gconsts=int(bad.value), inv_covars_f64=np.delete(ic64, gone, axis=0))


def dgmm_est(weights, means_invvars, inv_vars, occ, mean, var, acc_flags="mvw", update_flags="mvw", min_gaussian_weight=1e-5,
             min_gaussian_occupancy=10.0, min_variance=0.001, remove_low_count_gaussians=True, mix_up=0, perturb_factor=0.01, seed=0):
    """The M-step of gmm-global-est on host arrays (xv_dgmm_est, fp64), then the split to mix_up Gaussians: dict(weights, means_invvars,
    inv_vars, gconsts) of the model that results, removed (indices), floored (variances, Gaussians), objf_before, objf_after, count,
    split_of (for every Gaussian the split added, the index it was copied from)."""
    w0 = np.asarray(weights, dtype=np.float32)
    b0 = np.asarray(means_invvars, dtype=np.float32)
    iv0 = np.asarray(inv_vars, dtype=np.float32)
    _require(b0.ndim == 2 and w0.shape == (b0.shape[0],) and iv0.shape == b0.shape, "dgmm_est: weights [G], means_invvars [G][D], inv_vars [G][D]")
    g, d = b0.shape
    o, m, c = _f64(occ), _f64(mean), _f64(var)
    _require(o.shape == (g,) and m.shape == (g, d) and c.shape == (g, d), "dgmm_est: occ [G], mean [G][D], var [G][D]")
    cap = max(g, int(mix_up))
    w, b, iv = np.zeros(cap, np.float32), np.zeros((cap, d), np.float32), np.zeros((cap, d), np.float32)
    w[:g], b[:g], iv[:g] = w0, b0, iv0
    gc = np.zeros(cap, np.float32)
    removed = np.zeros(g, np.int32)
    split_of = np.zeros(max(cap, 1), np.int32)
    floored = np.zeros(2, np.int32)
    objf = np.zeros(3)
    left, n_removed = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().xv_dgmm_est(g, d, acc_flags.encode(), o.ctypes.data, m.ctypes.data, c.ctypes.data, update_flags.encode(), min_gaussian_weight,
                             min_gaussian_occupancy, min_variance, int(bool(remove_low_count_gaussians)), int(mix_up), perturb_factor, int(seed),
                             w.ctypes.data, b.ctypes.data, iv.ctypes.data, gc.ctypes.data, byref(left), removed.ctypes.data,
                             byref(n_removed), floored.ctypes.data, objf.ctypes.data, split_of.ctypes.data))
    k, nr = left.value, n_removed.value
    return dict(weights=w[:k].copy(), means_invvars=b[:k].copy(), inv_vars=iv[:k].copy(), gconsts=gc[:k].copy(),
                removed=removed[:nr].tolist(), floored=(int(floored[0]), int(floored[1])), objf_before=float(objf[0]),
                objf_after=float(objf[1]), count=float(objf[2]), split_of=split_of[:max(0, k - (g - nr))].tolist())
