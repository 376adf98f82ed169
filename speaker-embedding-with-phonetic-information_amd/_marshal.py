"""What the wrappers of every stage share in turning Python arguments into the C ABI's buffers."""
import numpy as np

from ._abi import XV_ERR_ARG, XvError


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _require(ok, msg):
    if not ok:
        raise XvError(XV_ERR_ARG, msg)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _ptr_or_null(a):
    """NULL for an array without elements"""
    return a.ctypes.data if a.size else None


def _split(a, off):
    """copies of the rows [off[u], off[u + 1]) of a, one per utterance"""
    return [a[off[u]:off[u + 1]].copy() for u in range(len(off) - 1)]


def _ms(names, ms):
    return dict(zip(names, [float(x) for x in ms]))


def _segments(segments):
    off = np.zeros(len(segments) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in segments])
    idx = _i32(np.concatenate([np.asarray(s, dtype=np.int32) for s in segments]) if len(segments) else np.zeros(0, np.int32))
    return off, idx


def _ragged(arrays, dtype):
    xs = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in arrays]
    off = np.zeros(len(xs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in xs])
    flat = np.concatenate(xs) if xs else np.zeros(0, dtype)
    if flat.size == 0:
        flat = np.zeros(1, dtype)
    return flat, off


def _pack_matrices(mats, what):
    ms = [_f32(m) for m in mats]
    _require(all(m.ndim == 2 for m in ms), "%s: every matrix must be two-dimensional" % what)
    widths = {m.shape[1] for m in ms if m.shape[0] > 0}
    _require(len(widths) <= 1, "%s: the matrices of one call share their column count" % what)
    cols = widths.pop() if widths else 0
    off = np.zeros(len(ms) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m.shape[0] if cols else 0 for m in ms])
    rows = [m for m in ms if m.shape[0] > 0 and cols]
    packed = np.concatenate(rows, axis=0) if rows else np.zeros((0, max(cols, 1)), np.float32)
    return np.ascontiguousarray(packed), off, cols


def _selection(gselect_list, off, who):
    """one [frames, n] selection per utterance -> ([rows, n] int32, n)"""
    gs = [_i32(g) for g in gselect_list]
    nu = len(off) - 1
    _require(nu > 0 and len(gs) == nu and all(g.ndim == 2 and g.shape[0] == off[u + 1] - off[u] and g.shape[1] == gs[0].shape[1]
                                              for u, g in enumerate(gs)),
             "%s: one [frames, n] selection per utterance, all of one n" % who)
    return np.ascontiguousarray(np.concatenate(gs, axis=0)), gs[0].shape[1]


def _full_gmm(weights, means_invcovars, inv_covars, who):
    """float32 weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2] of a full-covariance model"""
    w, b, ic = _f32(weights), _f32(means_invcovars), _f32(inv_covars)
    _require(b.ndim == 2 and w.shape == (b.shape[0],) and ic.shape == (b.shape[0], b.shape[1] * (b.shape[1] + 1) // 2),
             who + ": weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2]")
    return w, b, ic
