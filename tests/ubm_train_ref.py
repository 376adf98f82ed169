"""numpy restatement of full-covariance UBM training (csrc/ubm_train.h), in float64 on the float32 values the tools see, plus the
accumulator file in Python (binary and text, write and read).  Built on ubm_ref.py."""
import io
import struct

import numpy as np

import ubm_ref as R

F = np.float32
FLAG_M, FLAG_V, FLAG_W = 1, 2, 4


def parse_flags(letters):
    return sum({"m": FLAG_M, "v": FLAG_V, "w": FLAG_W}[c] for c in set(letters))


def augment_flags(flags):
    if flags & FLAG_V:
        flags |= FLAG_M
    if flags & FLAG_M:
        flags |= FLAG_W
    return flags


def tri(d):
    return d * (d + 1) // 2


# ------------------------------------------------------------------------------------------------------------- host tools
def gmm_to_fgmm(weights, means_invvars, inv_vars):
    """-> (gconsts float64 [G], means_invcovars, inv_covars packed) of the full image of a diagonal model"""
    mi, iv = np.asarray(means_invvars, F), np.asarray(inv_vars, F)
    G, D = mi.shape
    ic = np.zeros((G, tri(D)), F)
    diag = np.array([tri(d) + d for d in range(D)])
    ic[:, diag] = iv
    return R.full_gconsts(weights, mi, ic), mi, ic


def subsample(x, n, offset=0):
    """-> the rows kept (n > 0) or repeated (n < 0); None when no row is kept"""
    x = np.asarray(x)
    out = x[offset::n] if n > 0 else np.repeat(x, -n, axis=0)
    return out if len(out) else None


# ------------------------------------------------------------------------------------------------------------- accumulation
def acc_stats(feats, frame, gauss, p, G, flags):
    """pairs (frame[k], gauss[k], p[k]) -> (occ [G], mean [G, D], cov [G, tri D]) in float64; the arrays the augmented flags do not
    name stay zero.  Products of widened float32 values, summed pair by pair in bucket order."""
    x = np.asarray(feats, F).astype(np.float64)
    frame, gauss = np.asarray(frame, np.int64), np.asarray(gauss, np.int64)
    p = np.asarray(p, F).astype(np.float64)
    flags = augment_flags(flags)
    D = x.shape[1]
    occ, mean, cov = np.zeros(G), np.zeros((G, D)), np.zeros((G, tri(D)))
    il = np.tril_indices(D)
    for g in range(G):
        k = np.nonzero((gauss == g) & (p != 0))[0]
        if not len(k):
            continue
        xg, pg = x[frame[k]], p[k]
        occ[g] = pg.sum()
        if flags & FLAG_M:
            mean[g] = (pg[:, None] * xg).sum(0)
        if flags & FLAG_V:
            cov[g] = ((pg[:, None] * xg).T @ xg)[il]
    return occ, mean, cov


def abs_terms(feats, frame, gauss, p, G):
    """the sums of the absolute values of the terms of acc_stats, and the number of pairs per Gaussian"""
    x = np.abs(np.asarray(feats, F).astype(np.float64))
    occ, mean, cov = acc_stats(x, frame, gauss, np.abs(np.asarray(p, F)), G, 7)
    return occ, mean, cov, np.bincount(np.asarray(gauss)[np.asarray(p, F) != 0], minlength=G)


def post_pairs(post):
    """per frame (indices, posteriors) -> (frame, gauss, p) of the pairs"""
    frame = np.concatenate([np.full(len(i), t) for t, (i, _) in enumerate(post)]) if len(post) else np.zeros(0, np.int64)
    gauss = np.concatenate([np.asarray(i, np.int64) for i, _ in post]) if len(post) else np.zeros(0, np.int64)
    p = np.concatenate([np.asarray(q, F) for _, q in post]) if len(post) else np.zeros(0, F)
    return frame.astype(np.int64), gauss, p


# ------------------------------------------------------------------------------------------------------------- the file
def accs_bytes(occ, mean, cov, flags, binary=True):
    """the accumulator file; the float64 arrays are rounded to float32 here, once"""
    occ, mean, cov = np.asarray(occ, F), np.asarray(mean, F), np.asarray(cov, F)
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
        R._tok(f, "<FULLVARACCS>")
        for c in cov:
            R._packed(f, c, D, binary)
    R._tok(f, "</GMMACCS>")
    return f.getvalue()


def read_accs(data):
    """-> dict(dim, num_gauss, flags, occ, mean, cov) with float32 arrays (cov zeros without v)"""
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
    cov = np.zeros((G, tri(D)), F)
    if flags & FLAG_V:
        assert i.token() == "<FULLVARACCS>"
        cov = np.stack([i.packed(b) for _ in range(G)])
    assert i.token() == "</GMMACCS>"
    assert occ.shape == (G,) and mean.shape == (G, D) and cov.shape == (G, tri(D))
    return dict(dim=D, num_gauss=G, flags=flags, occ=occ, mean=mean, cov=cov)


# ------------------------------------------------------------------------------------------------------------- the M-step
def ml_objective(gconsts, b, ic, occ, mean, cov, acc_flags):
    obj = float(np.dot(occ, np.asarray(gconsts, np.float64)))
    if acc_flags & FLAG_M:
        obj += float((mean * np.asarray(b, np.float64)).sum())
    if acc_flags & FLAG_V:
        D = b.shape[1]
        for g in range(len(occ)):
            obj -= 0.5 * float(np.trace(R.unpack(cov[g], D) @ R.unpack(ic[g], D)))
    return obj


def fgmm_est(weights, means_invcovars, inv_covars, occ, mean, cov, acc_flags=7, update_flags="mvw", min_gaussian_weight=1e-5,
             min_gaussian_occupancy=100.0, variance_floor=0.001, max_condition=1e5, remove_low_count_gaussians=True):
    """-> dict(weights, means_invcovars, inv_covars (float32, of the Gaussians that survive), gconsts (float64), removed, floored
    (eigenvalues, Gaussians), objf_before, objf_after, count, log: [(level, text)] as fgmm-global-est words them)."""
    w0, b, ic = np.array(weights, F), np.array(means_invcovars, F), np.array(inv_covars, F)
    occ, mean, cov = (np.asarray(a, np.float64) for a in (occ, mean, cov))
    G, D = b.shape
    upd = parse_flags(update_flags)
    assert not upd & ~acc_flags
    upd_m, upd_v, upd_w = bool(upd & FLAG_M), bool(upd & FLAG_V), bool(upd & FLAG_W)
    before = ml_objective(R.full_gconsts(w0, b, ic).astype(F), b, ic, occ, mean, cov, acc_flags)
    occ_sum = float(occ.sum())
    w = np.zeros(G)
    removed, log = [], []
    floored_elements = floored_gauss = 0
    for g in range(G):
        prob = occ[g] / occ_sum if occ_sum > 0 else 1.0 / G
        if occ[g] > min_gaussian_occupancy and prob > min_gaussian_weight:
            w[g] = prob
            if not (upd_m or upd_v):
                continue
            mu = mean[g] / occ[g]
            inv = R.unpack(ic[g], D)
            mu_old = None if upd_m else np.linalg.inv(inv) @ b[g].astype(np.float64)
            if upd_v:
                c = R.unpack(cov[g], D) / occ[g] - np.outer(mu, mu)
                if not upd_m:
                    c += np.outer(mu_old - mu, mu_old - mu)
                s, u = np.linalg.eigh(c)
                floor = max(variance_floor, np.abs(s).max() / max_condition)
                low = s < floor
                if low.any():
                    floored_elements += int(low.sum())
                    floored_gauss += 1
                    c = (u * np.where(low, floor, s)) @ u.T
                inv = np.linalg.inv(c)
                inv = 0.5 * (inv + inv.T)
                ic[g] = R.pack(inv).astype(F)
            b[g] = (inv @ (mu if upd_m else mu_old)).astype(F)
        elif remove_low_count_gaussians and len(removed) < G - 1:
            log.append(("WARNING", "Too little data - removing Gaussian (weight %g, occupation count %g, vector size %d)" % (prob, occ[g], D)))
            removed.append(g)
            w[g] = float(w0[g])   # until it is taken out it counts with its old weight
        else:
            log.append(("WARNING", "Gaussian has too little data but not removing it because %s%d, occ = %g, weight = %g" % (
                "it is the last Gaussian: i = " if remove_low_count_gaussians else "remove-low-count-gaussians == false: i = ", g, occ[g], prob)))
            w[g] = max(prob, min_gaussian_weight)
    wf = (w / w.sum()).astype(F) if upd_w else w0
    after = ml_objective(R.full_gconsts(wf, b, ic).astype(F), b, ic, occ, mean, cov, acc_flags)
    keep = np.array([g for g in range(G) if g not in removed])
    if removed:
        wf = (wf[keep].astype(np.float64) / wf[keep].astype(np.float64).sum()).astype(F)
        b, ic = b[keep], ic[keep]
    log.append(("LOG", "Overall objective function improvement is %g per frame over %g frames" % ((after - before) / occ_sum, occ_sum)))
    if floored_elements:
        log.append(("WARNING", "%d variances floored in %d Gaussians." % (floored_elements, floored_gauss)))
    return dict(weights=wf, means_invcovars=b, inv_covars=ic, gconsts=R.full_gconsts(wf, b, ic), removed=removed,
                floored=(floored_elements, floored_gauss), objf_before=before, objf_after=after, count=occ_sum, log=log)


# ------------------------------------------------------------------------------------------------------------- EM on the restatement
def e_step(x, weights, b, ic, n, flags=7):
    """one pass of gmm-gselect on the diagonal image, then the full-covariance E-step: (occ, mean, cov, total log-likelihood)"""
    gd, mi, iv = R.fgmm_to_gmm(weights, b, ic)
    sel = R.gselect(R.diag_loglikes(x, gd, mi, iv), n)
    gc = R.full_gconsts(weights, b, ic).astype(F)
    post, logsum = R.posteriors(R.full_loglikes(x, gc, b, ic, sel))
    frame = np.repeat(np.arange(len(x)), n)
    occ, mean, cov = acc_stats(x, frame, sel.reshape(-1), post.astype(F).reshape(-1), len(weights), flags)
    return occ, mean, cov, float(logsum.sum())
