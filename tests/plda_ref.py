"""fp64 numpy restatement of the PLDA back-end (stage 7 of egs/sre/v2/run_sre10.sh:221-252) for the tests.

Semantics are upstream Kaldi's [UPSTREAM, recalled]: ivector/plda.cc (PldaStats, PldaEstimator's two-covariance EM,
Plda::TransformIvector / GetNormalizationFactor / LogLikelihoodRatio / SmoothWithinClassCovariance), ivector/
ivector-extractor.cc's LDA helpers (CovarianceStats, ComputeNormalizingTransform, ComputeLdaTransform) and
ivectorbin/{ivector-compute-lda,ivector-compute-plda,ivector-copy-plda,ivector-plda-scoring,compute-eer}.cc.  None of
it is vendored in the reference; parity with Kaldi itself stays unpinned, as for oracle/backend.py.

  scatter:   S_tot = sum_i x_i x_i^T, s_k = sum_{i in k} x_i, S_bet = sum_k s_k s_k^T / n_k
  LDA:       total = S_tot / N, within = (S_tot - S_bet) / N, M = f total + (1 - f) within,
             Tn = diag(s^-1/2) U^T from eig(M) (floored at floor * s_max), eig(Tn (total - within) Tn^T) = (s', U'),
             L = U'[:, :dim]^T Tn, output [L | -L mean]
  PLDA EM:   W = B = I; per iteration Wstats = offset scatter (count N - K), per class (in order of n)
             mixed = (B^-1 + n W^-1)^-1, m = mu_k - sum / K, w = mixed n W^-1 m,
             Bstats += mixed + w w^T, Wstats += n mixed + n (m - w)(m - w)^T (counts + 1 each); W, B = stats / counts.
             Output mean = sum / K, C = chol(W), eig(C^-1 B C^-T) = (psi, U) floored at 0, transform = U^T C^-1.
  smoothing: c = 1 + s psi, psi /= c, transform rows *= c^-1/2
  transform: y = T (x - mean); y *= sqrt(dim / sum y^2 / (psi + 1/n)) (or sqrt(dim) / |y|), stored as float32
  LLR:       m = n psi/(n psi + 1) u, var = 1 + psi/(n psi + 1);
             -1/2 [sum log var + sum (v - m)^2 / var] + 1/2 [sum log(1 + psi) + sum v^2 / (1 + psi)]
  EER:       sort both lists; first p (p + 1 < |tgt|) with non[q] < tgt[p], q = |non| - 1 - floor(|non| p / |tgt|);
             EER = p / |tgt| at threshold tgt[p]
"""
import numpy as np


def eig_desc(a):
    """Symmetric eigendecomposition, eigenvalues descending (Kaldi's SortSvd); eigenvectors are columns."""
    s, u = np.linalg.eigh((a + a.T) / 2)
    order = np.argsort(-s, kind="stable")
    return s[order], u[:, order]


def scatter_stats(x, segments):
    x = np.asarray(x, np.float64)
    idx = np.concatenate([np.asarray(s, np.int64) for s in segments]) if len(segments) else np.zeros(0, np.int64)
    xs = x[idx]
    s_tot = xs.T @ xs
    sums = np.stack([x[np.asarray(s, np.int64)].sum(0) if len(s) else np.zeros(x.shape[1]) for s in segments]) \
        if len(segments) else np.zeros((0, x.shape[1]))
    n = np.array([len(s) for s in segments], np.float64)
    nz = n > 0
    s_bet = (sums[nz] / n[nz, None]).T @ sums[nz] if nz.any() else np.zeros((x.shape[1], x.shape[1]))
    return s_tot, sums, (s_bet + s_bet.T) / 2


def lda_from_stats(s_tot, s_bet, n, mean, lda_dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    total = s_tot / n
    within = (s_tot - s_bet) / n
    m = total_covariance_factor * total + (1 - total_covariance_factor) * within
    s, u = eig_desc(m)
    s = np.maximum(s, covariance_floor * s[0])
    tn = (s ** -0.5)[:, None] * u.T
    s2, u2 = eig_desc(tn @ (total - within) @ tn.T)
    lin = (u2[:, :lda_dim].T @ tn).astype(np.float32)
    off = -(lin.astype(np.float64) @ np.asarray(mean, np.float64))
    return np.concatenate([lin, off[:, None].astype(np.float32)], axis=1)


def global_mean(x):
    """ivector-mean's / ComputeAndSubtractMean's mean: fp64 accumulation of fp32 vectors, stored as fp32."""
    return np.asarray(x, np.float64).mean(0).astype(np.float32)


def lda(x, speakers, lda_dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda on vectors x [N, D] (float32) with one speaker label per row."""
    x = np.asarray(x, np.float32)
    mean = global_mean(x)
    xc = (x - mean).astype(np.float32)
    groups = {}
    for i, s in enumerate(speakers):
        groups.setdefault(s, []).append(i)
    s_tot, _, s_bet = scatter_stats(xc, list(groups.values()))
    return lda_from_stats(s_tot, s_bet, len(x), mean, lda_dim, total_covariance_factor, covariance_floor)


def plda_em(sums, counts, s_tot, s_bet, num_em_iters=10):
    """Returns (mean, transform, psi, W, B): the model and the final within / between covariances."""
    counts = np.asarray(counts)
    k, dim = sums.shape
    means = sums / counts[:, None]
    total = means.sum(0)
    offset_scatter = s_tot - s_bet
    order = np.argsort(counts, kind="stable")
    n_total = counts.sum()
    w = np.eye(dim)
    b = np.eye(dim)
    for _ in range(num_em_iters):
        ws, wc = offset_scatter.copy(), float(n_total - k)
        bs, bc = np.zeros((dim, dim)), 0.0
        w_inv, b_inv = np.linalg.inv(w), np.linalg.inv(b)
        n = -1
        for c in order:
            if counts[c] != n:
                n = counts[c]
                mixed = np.linalg.inv(b_inv + n * w_inv)
            m = means[c] - total / k
            wv = mixed @ (n * (w_inv @ m))
            mw = m - wv
            bs += mixed + np.outer(wv, wv)
            ws += n * mixed + n * np.outer(mw, mw)
            bc += 1
            wc += 1
        w, b = ws / wc, bs / bc
    c = np.linalg.cholesky(w)
    ci = np.linalg.inv(c)
    psi, u = eig_desc(ci @ b @ ci.T)
    psi = np.maximum(psi, 0.0)
    return total / k, u.T @ ci, psi, w, b


def plda(x, segments, num_em_iters=10):
    """ivector-compute-plda: (mean, transform, psi) from vectors x and the rows of every speaker."""
    s_tot, sums, s_bet = scatter_stats(x, segments)
    mean, t, psi, _, _ = plda_em(sums, [len(s) for s in segments], s_tot, s_bet, num_em_iters)
    return mean, t, psi


def smooth(transform, psi, s):
    """ivector-copy-plda --smoothing=s (s != 0)."""
    c = 1.0 + s * psi
    return transform * (c ** -0.5)[:, None], psi / c


def transform_ivector(x, mean, transform, psi, num=1, normalize=True, simple=False):
    """Plda::TransformIvector for rows of x; returns (y float32, scale float64)."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    y = x @ transform.T - transform @ mean
    num = np.broadcast_to(np.asarray(num, np.float64), (len(x),))
    dim = y.shape[1]
    if simple:
        scale = np.sqrt(dim) / np.linalg.norm(y, axis=1)
    else:
        scale = np.sqrt(dim / ((y * y) / (psi[None, :] + 1.0 / num[:, None])).sum(1))
    if normalize:
        y = y * scale[:, None]
    return y.astype(np.float32), scale


def llr(u, n, v, psi):
    """Plda::LogLikelihoodRatio of a transformed enrolment vector u (mean of n) against a transformed test vector v."""
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    mean = n * psi / (n * psi + 1.0) * u
    var = 1.0 + psi / (n * psi + 1.0)
    given = -0.5 * (np.log(var).sum() + ((v - mean) ** 2 / var).sum())
    without = -0.5 * (np.log(1.0 + psi).sum() + (v * v / (1.0 + psi)).sum())
    return given - without


# ------------------------------------------------------------------------------------------------ helpers of the kernel tests
# (tests/test_gpu_backend_kernels.py and its CPU half tests/test_backend_kernels_ref.py): inputs on which every summation order
# gives the same bits, and np.longdouble restatements whose own error is some 2^-11 of a float64 rounding.
def ragged_lengths(rng, allowed, total=None, count=None):
    """Segment lengths drawn from `allowed` (which holds 1 unless `count` is given): either lengths that sum to `total`, every
    third one followed by an empty segment, or `count` lengths.  The first and the last segment are empty either way."""
    allowed = sorted(set(int(a) for a in allowed))
    if count is not None:
        assert count >= 2
        return [0] + [int(rng.choice(allowed)) for _ in range(count - 2)] + [0]
    lengths, left = [], int(total)
    while left > 0:
        k = int(rng.choice([a for a in allowed if 0 < a <= left]))
        lengths.append(k)
        if len(lengths) % 3 == 0:
            lengths.append(0)
        left -= k
    return [0] + lengths + [0]


def segments_of_lengths(rng, lengths, n_table):
    """Row lists of the given lengths into a table of n_table rows: random draws, so rows repeat within and across segments;
    every segment of four rows or more is a descending run."""
    segs = []
    for k in lengths:
        idx = rng.integers(0, n_table, k)
        segs.append([int(i) for i in (np.sort(idx)[::-1] if k >= 4 else idx)])
    return segs


def integer_vectors(seed, n, dim, low=-8, high=8):
    """float32 rows of integers in [low, high]"""
    return np.random.default_rng(seed).integers(low, high + 1, (n, dim)).astype(np.float32)


def scatter_stats_exact(x, segments):
    """scatter_stats of integer rows and segments whose lengths are powers of two, in int64: (s_tot, sums, s_bet, largest) as
    float64, every one exact.  s_bet is sum_s (n_max / n_s) s s^T in int64, divided by the power of two n_max at the end.
    `largest` is the largest absolute partial sum that any order of any of the three sums can reach, in units of the smallest
    term (1, or 1 / n_max for s_bet): below 2^53, float64 holds every partial sum of every order exactly."""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi, x)
    dim = xi.shape[1]
    idx = np.concatenate([np.asarray(s, np.int64) for s in segments]) if len(segments) else np.zeros(0, np.int64)
    rows = xi[idx]
    s_tot = rows.T @ rows
    sums = np.stack([xi[np.asarray(s, np.int64)].sum(0) for s in segments]) if len(segments) else np.zeros((0, dim), np.int64)
    abs_sums = np.stack([np.abs(xi[np.asarray(s, np.int64)]).sum(0) for s in segments]) if len(segments) \
        else np.zeros((0, dim), np.int64)
    n = np.array([len(s) for s in segments], np.int64)
    nz = n > 0
    assert np.all(n[nz] & (n[nz] - 1) == 0), "segment lengths must be powers of two"
    n_max = int(n.max()) if nz.any() else 1
    w = (n_max // n[nz])[:, None]
    scaled = (sums[nz] * w).T @ sums[nz]
    largest = max(int((np.abs(rows).T @ np.abs(rows)).max(initial=0)), int(abs_sums.max(initial=0)),
                  int(((np.abs(sums[nz]) * w).T @ np.abs(sums[nz])).max(initial=0)))
    return s_tot.astype(np.float64), sums.astype(np.float64), scaled.astype(np.float64) / n_max, largest


def sequential_sums(x, segments):
    """sums[s]: the rows of segment s added one at a time in list order, in float64"""
    x = np.asarray(x, np.float32)
    out = np.zeros((len(segments), x.shape[1]))
    for s, seg in enumerate(segments):
        for i in seg:
            out[s] += x[i].astype(np.float64)
    return out


def integer_plda_model(seed, dim, zero_every=4):
    """(transform, offset, psi) for TransformIvector on integers: T in [-4, 4], offset in [-16, 16], psi in [0, 6] descending
    with an exact 0 in every zero_every-th place and in the last.  Row 0 of T is even and offset[0] odd, so y[0] is odd for
    every integer x: no transformed vector is zero."""
    rng = np.random.default_rng(seed)
    t = rng.integers(-4, 5, (dim, dim)).astype(np.float64)
    t[0] = 2 * rng.integers(-2, 3, dim)
    offset = rng.integers(-16, 17, dim).astype(np.float64)
    offset[0] = 2 * int(rng.integers(-8, 8)) + 1
    psi = np.sort(rng.uniform(0.0, 6.0, dim))[::-1].copy()
    psi[zero_every - 1::zero_every] = 0.0
    psi[-1] = 0.0
    return t, offset, psi


def scoring_case(seed, dim, n_u, n_v):
    """(u, num_u, v, psi) for LogLikelihoodRatio: psi is 0 in every fourth place (and in the last when dim > 1) and in [2, 6]
    elsewhere, num_u cycles through 1, 2.5, 3, 2, 1.5 (all in [1, 3]), u and v are float32 draws with the model's total
    variance 1 + psi.  The kernel test's error bound rests on these ranges."""
    rng = np.random.default_rng(seed)
    psi = np.sort(rng.uniform(2.0, 6.0, dim))[::-1].copy()
    psi[3::4] = 0.0
    if dim > 1:
        psi[-1] = 0.0
    sd = np.sqrt(1.0 + psi)
    u = (rng.standard_normal((n_u, dim)) * sd).astype(np.float32)
    v = (rng.standard_normal((n_v, dim)) * sd).astype(np.float32)
    num_u = np.array([(1.0, 2.5, 3.0, 2.0, 1.5)[k % 5] for k in range(n_u)])
    return u, num_u, v, psi


def transform_ivector_ld(x, transform, offset, psi, num=1, simple=False):
    """Plda::TransformIvector in np.longdouble, on the device's own terms (offset = -T mean): (y, scale), neither rounded;
    the normalised vector is y * scale[:, None]."""
    L = np.longdouble
    x = np.atleast_2d(np.asarray(x)).astype(L)
    y = x @ np.asarray(transform).astype(L).T + np.asarray(offset).astype(L)
    num = np.broadcast_to(np.asarray(num).astype(L), (len(x),))
    dim = L(y.shape[1])
    if simple:
        scale = np.sqrt(dim) / np.sqrt((y * y).sum(1))
    else:
        scale = np.sqrt(dim / ((y * y) / (np.asarray(psi).astype(L)[None, :] + L(1) / num[:, None])).sum(1))
    return y, scale


def llr_ld(u, num_u, v, psi):
    """Plda::LogLikelihoodRatio of every row of u (means of num_u examples) against every row of v, in np.longdouble:
    (llr, size), both [n_u, n_v]; size = 1/2 (sum |log(1 + psi)| + sum |log var| + sum (v - m)^2 / var + sum v^2 / (1 + psi)),
    the sum of the absolute values of the terms that llr is made of."""
    L = np.longdouble
    u = np.atleast_2d(np.asarray(u)).astype(L)
    v = np.atleast_2d(np.asarray(v)).astype(L)
    psi = np.asarray(psi).astype(L)[None, :]
    n = np.broadcast_to(np.asarray(num_u).astype(L), (len(u),))[:, None]
    mean = n * psi / (n * psi + 1) * u                         # [n_u, dim]
    var = 1 + psi / (n * psi + 1)
    quad_given = ((v[None, :, :] - mean[:, None, :]) ** 2 / var[:, None, :]).sum(2)
    quad_without = (v * v / (1 + psi)).sum(1)[None, :]
    log_given = np.log(var).sum(1)[:, None]
    log_without = np.log(1 + psi).sum()
    llr_all = -(log_given + quad_given) / 2 + (log_without + quad_without) / 2
    size = (np.abs(np.log(var)).sum(1)[:, None] + quad_given + np.abs(np.log(1 + psi)).sum() + quad_without) / 2
    return llr_all, size


def eer(target, nontarget):
    """compute-eer: (EER as a fraction, threshold), on float32 scores like the tool's BaseFloat."""
    tgt = np.sort(np.asarray(target, np.float32))
    non = np.sort(np.asarray(nontarget, np.float32))
    if not len(tgt) or not len(non):
        raise ValueError("need target and non-target scores")
    p = 0
    while p + 1 < len(tgt):
        q = max(len(non) - 1 - int(len(non) * p * 1.0 / len(tgt)), 0)
        if non[q] < tgt[p]:
            break
        p += 1
    return float(np.float32(p * 1.0 / len(tgt))), float(tgt[p])


def write_plda(path, mean, transform, psi, binary=True, double=True):
    """A Plda object file: <Plda> mean transform psi </Plda> (DV/DM, or FV/FM with double=False)."""
    from oracle import kaldi_io as kio
    with open(path, "wb") as f:
        if binary:
            f.write(b"\0B")
        f.write(b"<Plda> ")
        kio.write_vector(f, mean, binary, double)
        kio.write_matrix(f, transform, binary, double)
        kio.write_vector(f, psi, binary, double)
        f.write(b"</Plda> " if binary else b"</Plda> \n")


def read_plda(path):
    """(mean, transform, psi) as float64 from a binary or text Plda object file."""
    from oracle import kaldi_io as kio
    with open(path, "rb") as f:
        binary = f.read(2) == b"\0B"
        if not binary:
            f.seek(0)
        assert kio.read_token(f) == "<Plda>"
        if binary:
            mean = kio.read_vector(f, True)
            tag = kio.read_token(f)
            rows, cols = kio.read_int32(f), kio.read_int32(f)
            dt = "<f8" if tag == "DM" else "<f4"
            t = np.frombuffer(f.read(rows * cols * int(dt[2])), dtype=dt).reshape(rows, cols)
            psi = kio.read_vector(f, True)
        else:
            mean = np.array(kio._read_text_vector_or_matrix(f)[0])
            t = np.array(kio._read_text_vector_or_matrix(f))
            psi = np.array(kio._read_text_vector_or_matrix(f)[0])
        assert kio.read_token(f) == "</Plda>"
    return np.asarray(mean, np.float64), np.asarray(t, np.float64), np.asarray(psi, np.float64)
