"""numpy restatement of diagonal UBM training (csrc/dubm_train.h), in float64 on the float32 values the tools see: the generator, the
frame sampling, the initialisation, the scores, the statistics of both E-steps with the sums of their absolute terms, the M-step,
Split and the accumulator file.  Built on ubm_ref.py and ubm_train_ref.py."""
import io
import math
import struct

import numpy as np

import ubm_ref as R
import ubm_train_ref as T

F = np.float32
FLAG_M, FLAG_V, FLAG_W = T.FLAG_M, T.FLAG_V, T.FLAG_W
parse_flags, augment_flags = T.parse_flags, T.augment_flags
M64 = (1 << 64) - 1
ENTRY_SAMPLE, ENTRY_INIT, ENTRY_SPLIT = 1 << 60, 2 << 60, 3 << 60


# ------------------------------------------------------------------------------------------------------------- the generator
def mix(seed, counter):
    """the top 53 bits of splitmix64's output function on seed * 0x9E3779B97F4A7C15 + counter"""
    z = (seed * 0x9E3779B97F4A7C15 + counter) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 11


def draw_a(seed, e):
    return mix(seed, (2 * e) & M64)


def draw_b(seed, e):
    return mix(seed, (2 * e + 1) & M64)


def gauss(seed, e):
    u1, u2 = (draw_a(seed, e) + 1.0) / 2.0 ** 53, draw_b(seed, e) / 2.0 ** 53
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586476925286766559 * u2)


# ------------------------------------------------------------------------------------------------------------- sampling, initialisation
def sample_frames(x, num_frames, seed):
    """the rows of x in reading order -> (kept [min(T, num_frames), D], rows read)"""
    x = np.asarray(x, F)
    kept = x[:num_frames].copy()
    for r in range(num_frames + 1, len(x) + 1):
        e = ENTRY_SAMPLE + r
        if draw_a(seed, e) / 2.0 ** 53 < num_frames / r:
            kept[draw_b(seed, e) % num_frames] = x[r - 1]
    return kept, len(x)


def init_from_frames(x, G, seed):
    """-> (weights, means_invvars, inv_vars) float32 and the frames drawn; the sums run over the frames in ascending order, as the tool's"""
    x = np.asarray(x, F)
    n, D = x.shape
    assert n >= 10 * G, "Too few frames to train on"
    x64 = x.astype(np.float64)
    mean = np.cumsum(x64, axis=0)[-1] / float(n)
    var = np.cumsum(x64 * x64, axis=0)[-1] / float(n) - mean * mean
    assert np.all(var > 0)
    used, frames, attempt = set(), [], 0
    for _ in range(G):
        while True:
            f = draw_a(seed, ENTRY_INIT + attempt) % n
            attempt += 1
            if f not in used:
                break
        used.add(f)
        frames.append(f)
    inv = 1.0 / var
    iv = np.tile(inv.astype(F), (G, 1))
    mi = (x64[frames] * inv[None]).astype(F)
    return np.full(G, F(1.0 / G)), mi, iv, frames


# ------------------------------------------------------------------------------------------------------------- scores
def gconsts32(weights, means_invvars, inv_vars):
    """the gconsts as the tools store them after they read or change a model"""
    return R.diag_gconsts(weights, means_invvars, inv_vars).astype(F)


def chain_scores(x, gconsts, means_invvars, inv_vars):
    """the float32 chain acc = fmaf(-1/2 iv_d, fl(x_d x_d), fmaf(mi_d, x_d, acc)) from acc = gconst, d ascending.  Every fused
    multiply-add is formed in float64 (the product is exact there) and rounded to float32: equal to the device's bits wherever no
    float64 sum falls within 2^-53 relative of a float32 rounding boundary, and always on the integer models."""
    x, mi = np.asarray(x, F), np.asarray(means_invvars, F)
    v = (F(-0.5) * np.asarray(inv_vars, F)).astype(F)
    acc = np.tile(np.asarray(gconsts, F)[None], (len(x), 1))
    q = (x * x).astype(F)
    for d in range(x.shape[1]):
        acc = (mi[None, :, d].astype(np.float64) * x[:, d, None].astype(np.float64) + acc.astype(np.float64)).astype(F)
        acc = (v[None, :, d].astype(np.float64) * q[:, d, None].astype(np.float64) + acc.astype(np.float64)).astype(F)
    return acc


def score_bound(x, gconsts, means_invvars, inv_vars):
    """|chain - float64| <= gamma(2 D + 4) sum |terms| per (frame, Gaussian), as test_gpu_ubm.random_case derives it"""
    D = np.asarray(x).shape[1]
    return R.gamma(2 * D + 1 + 3) * R.diag_abs_terms(x, gconsts, means_invvars, inv_vars)


# ------------------------------------------------------------------------------------------------------------- statistics
def acc_stats(feats, frame, gauss_, p, G, flags=7):
    """pairs (frame[k], gauss[k], p[k]) -> (occ [G], mean [G, D], var [G, D]) in float64; a pair whose p is 0 does not exist; the
    arrays the augmented flags do not name stay zero"""
    x = np.asarray(feats, F).astype(np.float64)
    frame, gauss_ = np.asarray(frame, np.int64), np.asarray(gauss_, np.int64)
    p = np.asarray(p, F).astype(np.float64)
    flags = augment_flags(flags)
    D = x.shape[1]
    occ, mean, var = np.zeros(G), np.zeros((G, D)), np.zeros((G, D))
    keep = p != 0
    frame, gauss_, p = frame[keep], gauss_[keep], p[keep]
    np.add.at(occ, gauss_, p)
    if flags & FLAG_M:
        np.add.at(mean, gauss_, p[:, None] * x[frame])
    if flags & FLAG_V:
        np.add.at(var, gauss_, p[:, None] * (x[frame] * x[frame]))
    return occ, mean, var


def abs_terms(feats, frame, gauss_, p, G):
    """the sums of the absolute values of the terms of acc_stats, and the number of pairs per Gaussian"""
    x = np.abs(np.asarray(feats, F))
    p = np.abs(np.asarray(p, F))
    occ, mean, var = acc_stats(x, frame, gauss_, p, G, 7)
    return occ, mean, var, np.bincount(np.asarray(gauss_, np.int64)[p != 0], minlength=G)


def dense_stats(feats, post, flags=7):
    """dense posteriors [T, G] (float32 values, widened) -> (occ, mean, var) in float64"""
    x = np.asarray(feats, F).astype(np.float64)
    p = np.asarray(post, F).astype(np.float64)
    flags = augment_flags(flags)
    occ = p.sum(0)
    mean = p.T @ x if flags & FLAG_M else np.zeros((p.shape[1], x.shape[1]))
    var = p.T @ (x * x) if flags & FLAG_V else np.zeros((p.shape[1], x.shape[1]))
    return occ, mean, var


def dense_e_step(x, gconsts, means_invvars, inv_vars):
    """the float64 E-step against all Gaussians: (post [T, G], logsum [T])"""
    ll = R.diag_loglikes(x, gconsts, means_invvars, inv_vars)
    return R.posteriors(ll)


def weighted_error_bound(x, post, e):
    """sum_t c_t p_tg |term| for occ, mean and var, c_t = exp(2 e_t + 16 2^-24) - 1, plus n_g 2^-52 sum_t p |term|: what an error of
    e_t in every score of frame t and the softmax's own float32 roundings can move a statistic by, and the summation's share.
    post [T, G] float64 with zeros where there is no pair."""
    ax = np.abs(np.asarray(x, F).astype(np.float64))
    c = np.expm1(2.0 * np.asarray(e, np.float64) + 16.0 * 2.0 ** -24)
    n_g = (post != 0).sum(0).astype(np.float64)
    out = []
    for t in (np.ones((len(ax), 1)), ax, ax * ax):
        first = (post * c[:, None]).T @ t
        total = post.T @ t
        out.append(first + (n_g * 2.0 ** -52)[:, None] * total)
    return out[0][:, 0], out[1], out[2]


# ------------------------------------------------------------------------------------------------------------- the file
def accs_bytes(occ, mean, var, flags, binary=True):
    """the accumulator file; the float64 arrays are rounded to float32 here, once"""
    occ, mean, var = np.asarray(occ, F), np.asarray(mean, F), np.asarray(var, F)
    G, D = mean.shape
    f = io.BytesIO()
    f.write(b"\0B" if binary else b"")
    R._tok(f, "<GMMACCS>")
    R._tok(f, "<VECSIZE>")
    R._int(f, D, binary)
    R._tok(f, "<NUMCOMPONENTS>")
    R._int(f, G, binary)
    R._tok(f, "<FLAGS>")
    f.write(b"\x02" + struct.pack("<H", flags) if binary else b"%d " % flags)
    R._tok(f, "<OCCUPANCY>")
    R._vec(f, occ, binary)
    R._tok(f, "<MEANACCS>")
    R._mat(f, mean, binary)
    if flags & FLAG_V:
        R._tok(f, "<DIAGVARACCS>")
        R._mat(f, var, binary)
    R._tok(f, "</GMMACCS>")
    return f.getvalue()


def read_accs(data):
    """-> dict(dim, num_gauss, flags, occ, mean, var) with float32 arrays (var zeros without v)"""
    i = R._In(data)
    b = R._header(i)
    assert i.token() == "<GMMACCS>"
    assert i.token() == "<VECSIZE>"
    D = i.int32(b)
    assert i.token() == "<NUMCOMPONENTS>"
    G = i.int32(b)
    assert i.token() == "<FLAGS>"
    if b:
        assert i.take(1) == b"\x02"
        flags = struct.unpack("<H", i.take(2))[0]
    else:
        flags = int(i.token())
    assert i.token() == "<OCCUPANCY>"
    occ = i.vector(b)
    assert i.token() == "<MEANACCS>"
    mean = i.matrix(b)
    var = np.zeros((G, D), F)
    if flags & FLAG_V:
        assert i.token() == "<DIAGVARACCS>"
        var = i.matrix(b)
    assert i.token() == "</GMMACCS>"
    assert occ.shape == (G,) and mean.shape == (G, D) and var.shape == (G, D)
    return dict(dim=D, num_gauss=G, flags=flags, occ=occ, mean=mean, var=var)


# ------------------------------------------------------------------------------------------------------------- the M-step
def ml_objective(gconsts, mi, iv, occ, mean, var, acc_flags):
    obj = float(np.dot(occ, np.asarray(gconsts, np.float64)))
    if acc_flags & FLAG_M:
        obj += float((mean * np.asarray(mi, np.float64)).sum())
    if acc_flags & FLAG_V:
        obj -= 0.5 * float((var * np.asarray(iv, np.float64)).sum())
    return obj


def dgmm_est(weights, means_invvars, inv_vars, occ, mean, var, acc_flags=7, update_flags="mvw", min_gaussian_weight=1e-5,
             min_gaussian_occupancy=10.0, min_variance=0.001, remove_low_count_gaussians=True):
    """-> dict(weights, means_invvars, inv_vars (float32, of the Gaussians that survive), gconsts (float64), removed, floored (variances,
    Gaussians), objf_before, objf_after, count, log: [(level, text)] as gmm-global-est words them)."""
    w0, mi, iv = np.array(weights, F), np.array(means_invvars, F), np.array(inv_vars, F)
    occ, mean, var = (np.asarray(a, np.float64) for a in (occ, mean, var))
    G, D = mi.shape
    upd = parse_flags(update_flags)
    assert not upd & ~acc_flags
    upd_m, upd_v, upd_w = bool(upd & FLAG_M), bool(upd & FLAG_V), bool(upd & FLAG_W)
    before = ml_objective(gconsts32(w0, mi, iv), mi, iv, occ, mean, var, acc_flags)
    occ_sum = float(occ.sum())
    w = np.zeros(G)
    removed, log = [], []
    floored_elements = floored_gauss = 0
    for g in range(G):
        prob = occ[g] / occ_sum if occ_sum > 0 else 1.0 / G
        if occ[g] > min_gaussian_occupancy and prob > min_gaussian_weight:
            w[g] = prob
            if not acc_flags & FLAG_M:
                continue
            mu_old = mi[g].astype(np.float64) / iv[g].astype(np.float64)
            mu = mean[g] / occ[g]
            v = None
            if acc_flags & FLAG_V:
                v = var[g] / occ[g] - mu * mu
                if not upd_m:
                    v = v + (mu - mu_old) * (mu - mu_old)
                low = v < min_variance
                if low.any():
                    floored_elements += int(low.sum())
                    floored_gauss += 1
                    v = np.where(low, min_variance, v)
            if not (upd_m or upd_v):
                continue
            inv = 1.0 / v if upd_v else iv[g].astype(np.float64)
            if upd_v:
                iv[g] = inv.astype(F)
            mi[g] = ((mu if upd_m else mu_old) * inv).astype(F)
        elif remove_low_count_gaussians and len(removed) < G - 1:
            log.append(("WARNING", "Too little data - removing Gaussian (weight %g, occupation count %g, vector size %d)" % (prob, occ[g], D)))
            removed.append(g)
            w[g] = float(w0[g])   # until it is taken out it counts with its old weight
        else:
            log.append(("WARNING", "Gaussian has too little data but not removing it because %s%d, occ = %g, weight = %g" % (
                "it is the last Gaussian: i = " if remove_low_count_gaussians else "remove-low-count-gaussians == false: i = ", g, occ[g], prob)))
            w[g] = max(prob, min_gaussian_weight)
    wf = (w / w.sum()).astype(F) if upd_w else w0
    after = ml_objective(gconsts32(wf, mi, iv), mi, iv, occ, mean, var, acc_flags)
    keep = np.array([g for g in range(G) if g not in removed])
    if removed:
        wf = (wf[keep].astype(np.float64) / wf[keep].astype(np.float64).sum()).astype(F)
        mi, iv = mi[keep], iv[keep]
    log.append(("LOG", "Overall objective function improvement is %g per frame over %g frames" % ((after - before) / occ_sum, occ_sum)))
    if floored_elements:
        log.append(("WARNING", "%d variances floored in %d Gaussians." % (floored_elements, floored_gauss)))
    return dict(weights=wf, means_invvars=mi, inv_vars=iv, gconsts=R.diag_gconsts(wf, mi, iv), removed=removed,
                floored=(floored_elements, floored_gauss), objf_before=before, objf_after=after, count=occ_sum, log=log)


def split(weights, means_invvars, inv_vars, target, perturb, seed, stream=0):
    """DiagGmm::Split -> (weights, means_invvars, inv_vars) float32 and, for every Gaussian added, the index it was copied from"""
    w, mi, iv = (list(np.asarray(a, F)) for a in (weights, means_invvars, inv_vars))
    D = len(mi[0])
    split_of = []
    while len(w) < target:
        cur = len(w)
        best = int(np.argmax(np.asarray(w, F)))   # the first of the largest
        w[best] = F(w[best] / F(2.0))
        w.append(w[best])
        r = np.array([gauss(seed, ENTRY_SPLIT + (stream << 36) + cur * D + d) for d in range(D)]) * np.sqrt(iv[best].astype(np.float64))
        base = mi[best].astype(np.float64)
        iv.append(iv[best].copy())
        mi.append((base + perturb * r).astype(F))
        mi[best] = (base - perturb * r).astype(F)
        split_of.append(best)
    return np.asarray(w, F), np.stack(mi).astype(F), np.stack(iv).astype(F), split_of


def em_iteration(x, weights, means_invvars, inv_vars, **est):
    """one iteration of gmm-global-init-from-feats in float64: the dense E-step, then the M-step.  -> (dgmm_est's dict, the
    likelihood per frame)"""
    gc = gconsts32(weights, means_invvars, inv_vars)
    post, logsum = dense_e_step(x, gc, means_invvars, inv_vars)
    x64 = np.asarray(x, F).astype(np.float64)
    occ, mean, var = post.sum(0), post.T @ x64, post.T @ (x64 * x64)   # the float64 posteriors, not rounded
    return dgmm_est(weights, means_invvars, inv_vars, occ, mean, var, **est), float(logsum.mean())
