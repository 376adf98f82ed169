"""i-vectors: the extractor on the device, its files, the statistics of its training and their M-step."""
import ctypes
from ctypes import byref

import numpy as np

from ._abi import _check, _Handle, lib
from ._marshal import _f64, _full_gmm, _ms, _pack_matrices, _ptr, _require


def ivex_read(rxfilename):
    """A final.ie (binary or text; "file", "-", "cmd |") as host arrays: dict(w_vec [G], M [G][D][S], sigma_inv [G][D (D + 1) / 2],
    prior_offset).  Host only."""
    L = lib()
    g, d, s = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(L.xv_ivex_read(rxfilename.encode(), byref(g), byref(d), byref(s), None, None, None, None))
    G, D, S = g.value, d.value, s.value
    w_vec, M, sig = np.zeros(G), np.zeros((G, D, S)), np.zeros((G, D * (D + 1) // 2))
    p = ctypes.c_double()
    _check(L.xv_ivex_read(rxfilename.encode(), None, None, None, w_vec.ctypes.data, M.ctypes.data, sig.ctypes.data, byref(p)))
    return dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=p.value)


def _ivex_arrays(w_vec, M, sigma_inv, who):
    M, w_vec, sig = _f64(M), _f64(w_vec), _f64(sigma_inv)
    _require(M.ndim == 3 and w_vec.shape == (M.shape[0],) and sig.shape == (M.shape[0], M.shape[1] * (M.shape[1] + 1) // 2),
             who + ": w_vec [G], M [G][D][S], sigma_inv [G][D (D + 1) / 2]")
    return w_vec, M, sig


def ivex_write(wxfilename, w_vec, M, sigma_inv, prior_offset, binary=True):
    """Host arrays to a final.ie (text: 17 significant digits).  Host only."""
    w_vec, M, sig = _ivex_arrays(w_vec, M, sigma_inv, "ivex_write")
    _check(lib().xv_ivex_write(wxfilename.encode(), int(bool(binary)), M.shape[0], M.shape[1], M.shape[2], w_vec.ctypes.data, M.ctypes.data,
                               sig.ctypes.data, float(prior_offset)))


def _pack_posteriors(post_list, off, who):
    """post_list[u][t] = (indices, weights) -> (post_off [rows + 1], post_idx, post_w)"""
    _require(len(post_list) == len(off) - 1 and all(len(p) == off[u + 1] - off[u] for u, p in enumerate(post_list)),
             who + ": one posterior per utterance, one (indices, weights) entry per frame")
    counts = [len(f[0]) for p in post_list for f in p]
    post_off = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=post_off[1:])
    idx = [np.asarray(f[0], dtype=np.int32).reshape(-1) for p in post_list for f in p]
    w = [np.asarray(f[1], dtype=np.float32).reshape(-1) for p in post_list for f in p]
    post_idx = np.ascontiguousarray(np.concatenate(idx)) if idx else np.zeros(0, np.int32)
    post_w = np.ascontiguousarray(np.concatenate(w)) if w else np.zeros(0, np.float32)
    _require(post_idx.shape == post_w.shape, who + ": a frame's indices and weights have one length")
    return post_off, post_idx, post_w


class IvectorExtractor(_Handle):
    """An i-vector extractor on one device (xv_ivex_create / xv_ivex_load): the derived variables are computed there once.
    IvectorExtractor(w_vec, M, sigma_inv, prior_offset) from host arrays, IvectorExtractor.load(rxfilename) from a final.ie."""
    _destroy = "xv_ivex_destroy"

    def __init__(self, w_vec=None, M=None, sigma_inv=None, prior_offset=0.0, device=0, _handle=None):
        L = lib()
        self._h = _handle
        if self._h is None:
            w_vec, M, sig = _ivex_arrays(w_vec, M, sigma_inv, "IvectorExtractor")
            h = ctypes.c_void_p()
            _check(L.xv_ivex_create(device, M.shape[0], M.shape[1], M.shape[2], w_vec.ctypes.data, M.ctypes.data, sig.ctypes.data,
                                    float(prior_offset), byref(h)))
            self._h = h
        g, d, s = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(L.xv_ivex_info(self._h, byref(g), byref(d), byref(s)))
        self.num_gauss, self.feat_dim, self.ivector_dim = g.value, d.value, s.value

    @classmethod
    def load(cls, rxfilename, device=0):
        h = ctypes.c_void_p()
        _check(lib().xv_ivex_load(device, rxfilename.encode(), byref(h)))
        return cls(_handle=h)

    def derived(self):
        """(SigmaInvM [G D][S], U [G][S (S + 1) / 2]) as the device computed them."""
        G, D, S = self.num_gauss, self.feat_dim, self.ivector_dim
        sim, U = np.zeros((G * D, S)), np.zeros((G, S * (S + 1) // 2))
        _check(lib().xv_ivex_derived(self._h, sim.ctypes.data, U.ctypes.data))
        return sim, U

    def _inputs(self, feats_list, post_list, who):
        """(the six arguments every call on utterances starts with after the handle, the number of utterances)"""
        packed, off, cols = _pack_matrices(feats_list, who)
        _require(cols == self.feat_dim, "%s: the features have %d columns, the model %d" % (who, cols, self.feat_dim))
        arrays = (packed, off) + _pack_posteriors(post_list, off, who)
        n = len(off) - 1
        return arrays, (packed.ctypes.data, off.ctypes.data, n) + tuple(a.ctypes.data for a in arrays[2:]), n

    def extract(self, feats_list, post_list, return_details=False, acoustic_weight=1.0, max_count=0.0):
        """feats_list[u]: float32 [frames, D]; post_list[u][t] = (Gaussian indices, posteriors) of frame t.  Returns (ivectors
        float32 [n, S], status int32 [n], auxf_change float64 [n]); return_details: also a dict of gamma [n, G], X [n, G D],
        linear [n, S] and quadratic [n, S, S] (Q, symmetric), all float64 as the device formed them."""
        keep, args, n = self._inputs(feats_list, post_list, "extract")
        G, D, S = self.num_gauss, self.feat_dim, self.ivector_dim
        P = S * (S + 1) // 2
        iv, status, auxf = np.zeros((n, S), np.float32), np.zeros(n, np.int32), np.zeros(n)
        det = dict(gamma=np.zeros((n, G)), X=np.zeros((n, G * D)), linear=np.zeros((n, S)), quadratic=np.zeros((n, P))) if return_details else {}
        _check(lib().xv_ivex_extract(self._h, *args, float(acoustic_weight), float(max_count), iv.ctypes.data, status.ctypes.data,
                                     auxf.ctypes.data, *[_ptr(det.get(k)) for k in ("gamma", "X", "linear", "quadratic")]))
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
        keep, args, n = self._inputs(feats_list, post_list, "kernel_time")
        ms = (ctypes.c_float * 5)()
        _check(lib().xv_ivex_kernel_time(self._h, *args, reps, ms))
        return _ms(("stats", "quadratic", "linear", "solve", "derive"), ms)


_STATS_KEYS = ("scalars", "gamma", "Y", "R", "S", "ivector_sum", "ivector_scatter")   # the seven arrays, in the ABI's order


def _ivex_stats_arrays(G, D, S, has_variances):
    P = S * (S + 1) // 2
    return dict(scalars=np.zeros(3), gamma=np.zeros(G), Y=np.zeros((G, D, S)), R=np.zeros((G, P)),
                S=np.zeros((G, D * (D + 1) // 2)) if has_variances else None, ivector_sum=np.zeros(S), ivector_scatter=np.zeros(P))


def _ivex_stats_ptrs(a):
    return [_ptr(a[k]) for k in _STATS_KEYS]


def _ivex_stats_out(a):
    out = dict(num_ivectors=float(a["scalars"][0]), auxf=float(a["scalars"][1]), frames=float(a["scalars"][2]))
    out.update({k: a[k] for k in _STATS_KEYS[1:]})
    return out


def _ivex_stats_in(stats, who):
    """the dict of IvexAccumulator.get() -> (G, D, S, has_variances, the seven pointers' arrays)"""
    Y = _f64(stats["Y"])
    _require(Y.ndim == 3, who + ": Y [G][D][S]")
    G, D, S = Y.shape
    P = S * (S + 1) // 2
    has = stats.get("S") is not None
    arr = dict(scalars=np.array([stats["num_ivectors"], stats["auxf"], stats["frames"]], dtype=np.float64), Y=Y)
    for k, shape in (("gamma", (G,)), ("R", (G, P)), ("S", (G, D * (D + 1) // 2)), ("ivector_sum", (S,)), ("ivector_scatter", (P,))):
        if k == "S" and not has:
            arr[k] = None
            continue
        arr[k] = _f64(stats[k])
        _require(arr[k].shape == shape, "%s: %s has shape %s, the statistics ask for %s" % (who, k, arr[k].shape, shape))
    return G, D, S, has, arr


def ivex_stats_read(rxfilename):
    """The statistics file of ivector-extractor-acc-stats as the dict of IvexAccumulator.get().  Host only."""
    L = lib()
    g, d, s, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(L.xv_ivex_stats_read(rxfilename.encode(), byref(g), byref(d), byref(s), byref(v), *([None] * 7)))
    a = _ivex_stats_arrays(g.value, d.value, s.value, bool(v.value))
    _check(L.xv_ivex_stats_read(rxfilename.encode(), None, None, None, None, *_ivex_stats_ptrs(a)))
    return _ivex_stats_out(a)


def ivex_stats_write(wxfilename, stats, binary=True):
    """The dict of IvexAccumulator.get() to a statistics file (text: 17 significant digits).  Host only."""
    G, D, S, has, a = _ivex_stats_in(stats, "ivex_stats_write")
    _check(lib().xv_ivex_stats_write(wxfilename.encode(), int(bool(binary)), G, D, S, int(has), *_ivex_stats_ptrs(a)))


def ivex_init(weights, means_invcovars, inv_covars, ivector_dim=400, seed=0):
    """ivector-extractor-init on host arrays: a full-covariance UBM (float32 weights [G], means_invcovars [G][D], inv_covars
    [G][D (D + 1) / 2]) -> dict(w_vec, M, sigma_inv, prior_offset).  The same seed gives the same bytes.  Host only."""
    w, b, ic = _full_gmm(weights, means_invcovars, inv_covars, "ivex_init")
    G, D = b.shape
    S = int(ivector_dim)
    w_vec, M, sig = np.zeros(G), np.zeros((G, D, max(S, 1))), np.zeros((G, D * (D + 1) // 2))
    p = ctypes.c_double()
    _check(lib().xv_ivex_init(G, D, w.ctypes.data, b.ctypes.data, ic.ctypes.data, S, int(seed) & (2 ** 64 - 1), w_vec.ctypes.data, M.ctypes.data,
                              sig.ctypes.data, byref(p)))
    return dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=p.value)


def ivex_est(stats, w_vec, M, sigma_inv, prior_offset, variance_floor_factor=0.1, gaussian_min_count=100.0, diagonalize=True, num_threads=1):
    """The M-step of ivector-extractor-est (host, fp64) on the dict of IvexAccumulator.get().  Returns dict(w_vec, M, sigma_inv,
    prior_offset, V [S][S], gauss_updated, gauss_skipped, eig_floored, var_floored, var_floored_gauss, prior_floored, impr_proj,
    impr_var, impr_prior); the improvements are per frame."""
    w_vec, M, sig = _ivex_arrays(w_vec, M, sigma_inv, "ivex_est")
    M, sig = M.copy(), sig.copy()
    G, D, S, has, a = _ivex_stats_in(stats, "ivex_est")
    _require(M.shape == (G, D, S), "ivex_est: the statistics' shape %s is not the model's %s" % ((G, D, S), M.shape))
    p = ctypes.c_double(float(prior_offset))
    counts, impr, V = np.zeros(6, np.int32), np.zeros(3), np.zeros((S, S))
    _check(lib().xv_ivex_est(G, D, S, int(has), *_ivex_stats_ptrs(a), float(variance_floor_factor), float(gaussian_min_count),
                             int(bool(diagonalize)), int(num_threads), w_vec.ctypes.data, M.ctypes.data, sig.ctypes.data, byref(p),
                             counts.ctypes.data, impr.ctypes.data, V.ctypes.data))
    out = dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=p.value, V=V)
    out.update(zip(("gauss_updated", "gauss_skipped", "eig_floored", "var_floored", "var_floored_gauss", "prior_floored"), [int(c) for c in counts]))
    out.update(zip(("impr_proj", "impr_var", "impr_prior"), [float(x) for x in impr]))
    return out


def ivex_rank_update(A, B, C, slots, M, N, device=0):
    """The update kernel of extractor training alone (xv_ivex_rank_update): C[:M, :N] += A[:slots, :M].T @ B[:slots, :N] on the
    device; A [64][M], B [64][N], C [rows >= M][ld >= N] float64.  Returns the new C; what lies outside [M][N] comes back as it went."""
    A, B = _f64(A), _f64(B)
    C = np.array(C, dtype=np.float64, order="C")
    _require(A.shape == (64, M) and B.shape == (64, N) and C.ndim == 2, "ivex_rank_update: A [64][M], B [64][N], C [rows][ld]")
    _check(lib().xv_ivex_rank_update(device, A.ctypes.data, B.ctypes.data, C.ctypes.data, int(slots), int(M), int(N), C.shape[0], C.shape[1]))
    return C


class IvexAccumulator(_Handle):
    """The fp64 statistics of i-vector extractor training on the model's device (xv_ivex_acc_create; semantics in csrc/ivex_train.h).
    They are a function of the model and the ordered sequence of accepted utterances: how accumulate() calls split them changes no bit."""
    _destroy = "xv_ivex_acc_destroy"

    def __init__(self, model, update_variances=True, compute_auxf=True):
        self.model = model   # the device model must outlive the accumulators
        self.update_variances = bool(update_variances)
        self._h = ctypes.c_void_p()
        _check(lib().xv_ivex_acc_create(model._h, int(self.update_variances), int(bool(compute_auxf)), byref(self._h)))

    def accumulate(self, feats_list, post_list):
        """The inputs of IvectorExtractor.extract.  Returns status int32 [n]: 1 for an utterance whose Q is not positive definite (it
        contributes to nothing)."""
        keep, args, n = self.model._inputs(feats_list, post_list, "accumulate")
        status = np.zeros(n, np.int32)
        _check(lib().xv_ivex_acc_add(self._h, *args, status.ctypes.data))
        return status

    def get(self):
        """Flushes what is pending and returns dict(num_ivectors, auxf, frames, gamma [G], Y [G][D][S], R [G][P], S [G][D (D + 1) / 2]
        or None, ivector_sum [S], ivector_scatter [P])."""
        m = self.model
        a = _ivex_stats_arrays(m.num_gauss, m.feat_dim, m.ivector_dim, self.update_variances)
        _check(lib().xv_ivex_acc_get(self._h, *_ivex_stats_ptrs(a)))
        return _ivex_stats_out(a)

    def pending(self):
        """The pending utterances as the posterior kernel left them: dict(m [n][S], scatter [n][P], logdet [n], auxf [n])."""
        S = self.model.ivector_dim
        P = S * (S + 1) // 2
        m, sc, ld, ax = np.zeros((64, S)), np.zeros((64, P)), np.zeros(64), np.zeros(64)
        n = ctypes.c_int32()
        _check(lib().xv_ivex_acc_pending(self._h, byref(n), m.ctypes.data, sc.ctypes.data, ld.ctypes.data, ax.ctypes.data))
        k = n.value
        return dict(m=m[:k].copy(), scatter=sc[:k].copy(), logdet=ld[:k].copy(), auxf=ax[:k].copy())

    def kernel_time(self, feats_list, post_list, reps=3):
        """{posterior, rank_update_R, rank_update_Y} kernel times in ms of one accumulate() and flush (the best of reps).  Every run
        adds the call's statistics to the accumulators."""
        keep, args, n = self.model._inputs(feats_list, post_list, "kernel_time")
        ms = (ctypes.c_float * 3)()
        _check(lib().xv_ivex_acc_kernel_time(self._h, *args, reps, ms))
        return _ms(("posterior", "rank_update_R", "rank_update_Y"), ms)
