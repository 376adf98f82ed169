"""The speaker-level back-end and PLDA: mean subtraction, transforms, length normalisation, scatter statistics, scoring, estimation."""
import ctypes
from ctypes import byref

import numpy as np

from ._abi import _check, lib
from ._marshal import _f32, _f64, _i32, _ptr, _ptr_or_null, _require, _segments


def backend_apply(x, mean=None, transform=None, normalize=False, scaleup=True, device=0, return_ratio=False):
    """Speaker-level back-end on the device: ivector-subtract-global-mean -> transform-vec -> ivector-normalize-length
    (egs/sre/v2/run_sre10.sh:238-241), each stage optional.  x: [n, dim] float32.  Returns [n, out_dim] (and the length
    ratios when asked)."""
    x = _f32(x)
    n, dim = x.shape
    t_rows = t_cols = 0
    if mean is not None:
        mean = _f32(mean)
        _require(mean.shape == (dim,), "mean has shape %s, vectors have dimension %d" % (mean.shape, dim))
    if transform is not None:
        transform = _f32(transform)
        t_rows, t_cols = transform.shape
    out = np.empty((n, t_rows if transform is not None else dim), dtype=np.float32)
    ratio = np.empty(n, dtype=np.float32)
    _check(lib().xv_backend_apply(device, x.ctypes.data, n, dim, _ptr(mean), _ptr(transform), t_rows, t_cols, 1 if normalize else 0,
                                  1 if scaleup else 0, out.ctypes.data, ratio.ctypes.data))
    return (out, ratio) if return_ratio else out


def segment_mean(x, segments, acc64=False, device=0):
    """ivector-mean on the device: row s of the result is the mean of x[segments[s]] (rows added in list order;
    fp32 accumulator like the per-speaker loop, fp64 with acc64=True like the global mean)."""
    x = _f32(x)
    n, dim = x.shape
    off, idx = _segments(segments)
    out = np.empty((len(segments), dim), dtype=np.float32)
    _check(lib().xv_segment_mean(device, x.ctypes.data, n, dim, off.ctypes.data, _ptr_or_null(idx), len(segments), 1 if acc64 else 0,
                                 out.ctypes.data))
    return out


def scatter_stats(x, segments, device=0, return_ms=False):
    """Scatter statistics of the PLDA back-end on the device (fp64): segment s holds the rows x[segments[s]].  Returns
    (s_tot, sums, s_bet): sum of x_i x_i^T over every listed row [dim, dim], per-segment sums [n_seg, dim] and
    sum_s sums_s sums_s^T / n_s [dim, dim]; with return_ms also the kernel time."""
    x = _f32(x)
    n, dim = x.shape
    off, idx = _segments(segments)
    s_tot, s_bet, sums = np.empty((dim, dim)), np.empty((dim, dim)), np.empty((len(segments), dim))
    ms = ctypes.c_float(0)
    _check(lib().xv_scatter_stats(device, x.ctypes.data if n else None, n, dim, off.ctypes.data, _ptr_or_null(idx), len(segments),
                                  s_tot.ctypes.data, sums.ctypes.data if len(segments) else None, s_bet.ctypes.data, byref(ms)))
    return (s_tot, sums, s_bet, ms.value) if return_ms else (s_tot, sums, s_bet)


def plda_transform(x, transform, offset, psi, num=None, normalize=True, simple=False, device=0, return_ms=False):
    """Kaldi's Plda::TransformIvector on the device for every row of x [n, dim] (num: example count per row, default 1).
    Returns (y float32 [n, dim], scale float64 [n]) (and the kernel time with return_ms)."""
    x = _f32(x)
    n, dim = x.shape
    t, off, ps = _f64(transform), _f64(offset), _f64(psi)
    _require(t.shape == (dim, dim) and off.shape == (dim,) and ps.shape == (dim,),
             "PLDA model shapes do not match the vectors' dimension %d" % dim)
    num = _f64(np.ones(n) if num is None else num)
    y = np.empty((n, dim), np.float32)
    scale = np.empty(n, np.float64)
    ms = ctypes.c_float(0)
    _check(lib().xv_plda_transform(device, x.ctypes.data, n, dim, t.ctypes.data, off.ctypes.data, ps.ctypes.data, num.ctypes.data,
                                   1 if normalize else 0, 1 if simple else 0, y.ctypes.data, scale.ctypes.data, byref(ms)))
    return (y, scale, ms.value) if return_ms else (y, scale)


def plda_score(u, num_u, v, psi, trials, device=0, return_ms=False):
    """Kaldi's Plda::LogLikelihoodRatio on the device: trials [m, 2] of (enrolment row of u, test row of v), u [n_u, dim]
    transformed enrolment vectors with example counts num_u, v [n_v, dim] transformed test vectors.  Returns float64 [m]."""
    u, v, num_u, ps = _f32(u), _f32(v), _f64(num_u), _f64(psi)
    tr = np.ascontiguousarray(np.asarray(trials, dtype=np.int32).reshape(-1, 2))
    scores = np.empty(len(tr), np.float64)
    ms = ctypes.c_float(0)
    _check(lib().xv_plda_score(device, u.ctypes.data, num_u.ctypes.data, u.shape[0], v.ctypes.data, v.shape[0], u.shape[1], ps.ctypes.data,
                               tr.ctypes.data if len(tr) else None, len(tr), scores.ctypes.data if len(tr) else None, byref(ms)))
    return (scores, ms.value) if return_ms else scores


def lda_estimate(s_tot, s_bet, n, mean, lda_dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda's estimator on the host (no GPU needed) from the scatter statistics of n mean-subtracted
    vectors: the [lda_dim, dim + 1] float32 matrix [L | -L mean]."""
    s_tot, s_bet, mean = _f64(s_tot), _f64(s_bet), _f32(mean)
    dim = s_tot.shape[0]
    out = np.empty((lda_dim, dim + 1), np.float32)
    fl = ctypes.c_int32(0)
    _check(lib().xv_lda_estimate(dim, n, s_tot.ctypes.data, s_bet.ctypes.data, mean.ctypes.data, total_covariance_factor,
                                 covariance_floor, lda_dim, out.ctypes.data if lda_dim > 0 else None, byref(fl)))
    return out


def plda_estimate(sums, counts, s_tot, s_bet, num_em_iters=10):
    """ivector-compute-plda's EM on the host (no GPU needed) from per-speaker sums [n_spk, dim], counts [n_spk] and the
    scatter statistics of the same rows.  Returns (mean, transform, psi), float64."""
    sums, counts, s_tot, s_bet = _f64(sums), _i32(counts), _f64(s_tot), _f64(s_bet)
    n_spk, dim = sums.shape
    mean, transform, psi = np.empty(dim), np.empty((dim, dim)), np.empty(dim)
    fl = ctypes.c_int32(0)
    _check(lib().xv_plda_estimate(dim, n_spk, sums.ctypes.data, counts.ctypes.data, s_tot.ctypes.data, s_bet.ctypes.data, num_em_iters,
                                  mean.ctypes.data, transform.ctypes.data, psi.ctypes.data, byref(fl)))
    return mean, transform, psi


def plda_adapt(n, m, v, mean, transform, psi, mean_diff_scale=1.0, within_covar_scale=0.3, between_covar_scale=0.7):
    """ivector-adapt-plda's update on the host (no GPU needed) from the statistics of n unlabelled vectors, m = sum x [dim]
    and v = sum x x^T [dim, dim] (scatter_stats with one segment of every row: sums[0] and s_tot), and the model (mean,
    transform, psi).  Returns (mean, transform, psi, s), float64; s: the eigenvalues of the adaptation covariance in the
    space where the model's total covariance is I, descending."""
    m, v, mean, transform, psi = _f64(m), _f64(v), _f64(mean), _f64(transform), _f64(psi)
    dim = mean.shape[0]
    _require(m.shape == (dim,) and v.shape == (dim, dim) and transform.shape == (dim, dim) and psi.shape == (dim,),
             "PLDA adaptation: statistics and model shapes do not agree on dimension %d" % dim)
    mean_out, transform_out, psi_out, s = np.empty(dim), np.empty((dim, dim)), np.empty(dim), np.empty(dim)
    _check(lib().xv_plda_adapt(dim, int(n), m.ctypes.data, v.ctypes.data, mean.ctypes.data, transform.ctypes.data, psi.ctypes.data,
                               mean_diff_scale, within_covar_scale, between_covar_scale, mean_out.ctypes.data,
                               transform_out.ctypes.data, psi_out.ctypes.data, s.ctypes.data))
    return mean_out, transform_out, psi_out, s
