"""i-vector extractor training restated in numpy (float64): the statistics of ivector-extractor-acc-stats, the update of
ivector-extractor-est and the initialisation of ivector-extractor-init.  [UPSTREAM, recalled]: written from the documented behaviour
of Kaldi's ivector/ivector-extractor.cc and ivectorbin/ivector-extractor-*.cc of early 2018; Kaldi is not part of the reference
tree, so parity with a Kaldi binary is not pinned.  Independent of csrc/ivex_train.h, which states the same semantics."""
import math

import numpy as np

import ivector_ref as R

LOG_2PI = math.log(2.0 * math.pi)


def gconsts(sigma_inv, D):
    return np.array([-0.5 * (D * LOG_2PI - np.linalg.slogdet(R.unpack(s, D))[1]) for s in sigma_inv])


def second_moment(x, post, G):
    """S_ug [G][D][D] = sum_t w x x', float64 on the float32 inputs"""
    x = np.asarray(x, np.float32).astype(np.float64)
    out = np.zeros((G, x.shape[1], x.shape[1]))
    for t, (idx, w) in enumerate(post):
        for g, v in zip(idx, w):
            out[g] += float(v) * np.outer(x[t], x[t])
    return out


def e_step(x, post, model, sim_U=None):
    """One utterance: dict(ok, gamma, X [G][D], m, var, scatter, logdet, S2 [G][D][D], auxf_post (the part of the objective that needs
    the posterior), auxf_post_abs (the sum of the absolute values of its terms), l, Q)."""
    M, sig, p = model["M"], model["sigma_inv"], model["prior_offset"]
    G, D, S = M.shape
    e = R.extract(x, post, M, sig, p, sim_U=sim_U)
    l, Q, m = e["linear"], e["quadratic"], e["x"]
    ok = bool(np.all(np.linalg.eigvalsh(Q) > 0))
    var = np.linalg.inv(Q)
    var = 0.5 * (var + var.T)
    e0 = np.zeros(S)
    e0[0] = p
    la, Qa = l - e0, Q - np.eye(S)
    terms = [la @ m, -0.5 * m @ Qa @ m, -0.5 * np.sum(var * Qa), -0.5 * np.sum((m - e0) ** 2), -0.5 * np.trace(var),
             -0.5 * np.linalg.slogdet(Q)[1], 0.5 * S]
    abs_terms = (np.abs(la) @ np.abs(m) + 0.5 * np.abs(m) @ np.abs(Qa) @ np.abs(m) + 0.5 * np.sum(np.abs(var * Qa)) + 0.5 * np.sum((m - e0) ** 2)
                 + 0.5 * np.trace(var) + 0.5 * abs(np.linalg.slogdet(Q)[1]) + 0.5 * S)
    return dict(ok=ok, gamma=e["gamma"], X=e["X"].reshape(G, D), m=m, var=var, scatter=var + np.outer(m, m), logdet=-np.linalg.slogdet(Q)[1],
                S2=second_moment(x, post, G), auxf_post=float(sum(terms)), auxf_post_abs=float(abs_terms), l=l, Q=Q)


def zero_stats(G, D, S, update_variances=True):
    P = S * (S + 1) // 2
    return dict(num_ivectors=0.0, auxf=0.0, frames=0.0, gamma=np.zeros(G), Y=np.zeros((G, D, S)), R=np.zeros((G, P)),
                S=np.zeros((G, D * (D + 1) // 2)) if update_variances else None, ivector_sum=np.zeros(S), ivector_scatter=np.zeros(P))


def add_stats(a, b):
    out = {}
    for k in a:
        out[k] = None if a[k] is None else a[k] + b[k]
    return out


def accumulate(utts, model, update_variances=True, with_abs=False):
    """utts: [(x, post)].  Returns the statistics, and with_abs also the same dict of sums of absolute values of the terms (what an
    any-order summation bound is made of) and the number of accepted utterances' terms."""
    M, sig, w_vec = model["M"], model["sigma_inv"], model["w_vec"]
    G, D, S = M.shape
    sim_U = R.derived(M, sig)
    st, ab = zero_stats(G, D, S, update_variances), zero_stats(G, D, S, update_variances)
    gc = gconsts(sig, D)
    sinv = [R.unpack(s, D) for s in sig]
    for x, post in utts:
        e = e_step(x, post, model, sim_U)
        if not e["ok"]:
            continue
        sc = R.pack(e["scatter"])
        st["num_ivectors"] += 1
        st["gamma"] += e["gamma"]
        st["Y"] += e["X"][:, :, None] * e["m"][None, None, :]
        st["R"] += e["gamma"][:, None] * sc[None, :]
        st["ivector_sum"] += e["m"]
        st["ivector_scatter"] += sc
        ab["gamma"] += np.abs(e["gamma"])
        ab["Y"] += np.abs(e["X"])[:, :, None] * np.abs(e["m"])[None, None, :]
        ab["R"] += np.abs(e["gamma"])[:, None] * np.abs(sc)[None, :]
        ab["ivector_sum"] += np.abs(e["m"])
        ab["ivector_scatter"] += np.abs(sc)
        if update_variances:
            st["S"] += np.stack([R.pack(s) for s in e["S2"]])
            xa = np.abs(np.asarray(x, np.float32).astype(np.float64))
            ab["S"] += np.stack([R.pack(s) for s in second_moment(xa, post, G)])
            tr = np.array([np.sum(sinv[g] * e["S2"][g]) for g in range(G)])
            tr_abs = np.array([np.sum(np.abs(sinv[g] * e["S2"][g])) for g in range(G)])
        else:
            tr = tr_abs = e["gamma"] * D
        wg = e["gamma"] * (np.log(w_vec) + gc)
        st["auxf"] += float(np.sum(wg) - 0.5 * np.sum(tr) + e["auxf_post"])
        ab["auxf"] += float(np.sum(np.abs(wg)) + 0.5 * np.sum(tr_abs) + e["auxf_post_abs"])
        st["frames"] += float(np.sum(e["gamma"]))
        ab["frames"] += float(np.sum(e["gamma"]))
    return (st, ab) if with_abs else st


def _eig_desc(a):
    s, u = np.linalg.eigh(a)
    return s[::-1].copy(), u[:, ::-1].copy()


def m_step(stats, model, variance_floor_factor=0.1, gaussian_min_count=100.0, diagonalize=True):
    """Returns dict(w_vec, M, sigma_inv, prior_offset, V, updated [G] bool, eig_floored, var_floored, var_floored_gauss, prior_floored,
    impr_proj, impr_var, impr_prior, cond_R [G] (of the floored R_g), raw [G][D][D], floor matrix F)."""
    M = np.array(model["M"], dtype=np.float64)
    sig = np.array(model["sigma_inv"], dtype=np.float64)
    w_vec, p = np.asarray(model["w_vec"], np.float64), float(model["prior_offset"])
    G, D, S = M.shape
    gamma, Y = stats["gamma"], stats["Y"]
    frames = float(np.sum(gamma))
    updated = gamma >= gaussian_min_count
    eig_floored, impr_proj, cond_R = 0, 0.0, np.ones(G)
    abs_proj = abs_var = 0.0   # the sums of the absolute values of the objectives' terms, before and after: what their errors scale with
    Rg = [R.unpack(stats["R"][g], S) for g in range(G)]
    for g in np.flatnonzero(updated):
        lam, U = _eig_desc(Rg[g])
        floor = max(1e-40, lam.max() / 1e4)
        eig_floored += int(np.sum(lam < floor))
        lam = np.maximum(lam, floor)
        cond_R[g] = lam.max() / lam.min()
        sinv = R.unpack(sig[g], D)
        objf = lambda m: float(np.sum((sinv @ m) * Y[g]) - 0.5 * np.sum((sinv @ m) * (m @ Rg[g])))
        objf_abs = lambda m: float(np.sum(np.abs((sinv @ m) * Y[g])) + 0.5 * np.sum(np.abs((sinv @ m) * (m @ Rg[g]))))
        before = objf(M[g])
        abs_proj += objf_abs(M[g])
        M[g] = M[g] + (Y[g] - M[g] @ Rg[g]) @ (U / lam) @ U.T
        impr_proj += objf(M[g]) - before
        abs_proj += objf_abs(M[g])
    var_floored = var_floored_gauss = 0
    impr_var, raw, F = 0.0, np.zeros((G, D, D)), None
    if stats["S"] is not None and np.any(updated):
        for g in np.flatnonzero(updated):
            ym = Y[g] @ M[g].T
            raw[g] = R.unpack(stats["S"][g], D) - ym - ym.T + M[g] @ Rg[g] @ M[g].T
            raw[g] = 0.5 * (raw[g] + raw[g].T)
        F = variance_floor_factor * raw[updated].sum(axis=0) / gamma[updated].sum()
        L = np.linalg.cholesky(F)
        Linv = np.linalg.inv(L)
        for g in np.flatnonzero(updated):
            t, W = _eig_desc(Linv @ (raw[g] / gamma[g]) @ Linv.T)
            n = int(np.sum(t < 1.0))
            var_floored += n
            var_floored_gauss += 1 if n else 0
            LW = L @ W
            new_inv = np.linalg.inv((LW * np.maximum(t, 1.0)) @ LW.T)
            new_inv = 0.5 * (new_inv + new_inv.T)
            objf = lambda si: float(-0.5 * np.sum(si * raw[g]) + 0.5 * gamma[g] * np.linalg.slogdet(si)[1])
            impr_var += objf(new_inv) - objf(R.unpack(sig[g], D))
            for si in (new_inv, R.unpack(sig[g], D)):
                abs_var += float(0.5 * np.sum(np.abs(si * raw[g])) + 0.5 * gamma[g] * abs(np.linalg.slogdet(si)[1]))
            sig[g] = R.pack(new_inv)
    n = stats["num_ivectors"]
    mu = stats["ivector_sum"] / n
    C = R.unpack(stats["ivector_scatter"], S) / n - np.outer(mu, mu)
    s, Pm = _eig_desc(C)
    e0 = np.zeros(S)
    e0[0] = 1.0
    prior_floored = int(np.sum(s < 1e-7))
    s = np.maximum(s, 1e-7)
    impr_prior = n * (-0.5 * (np.sum(np.log(s)) + S) + 0.5 * (np.trace(C) + np.sum((mu - p * e0) ** 2)))
    abs_prior = n * (0.5 * (np.sum(np.abs(np.log(s))) + S) + 0.5 * (np.trace(C) + np.sum((mu - p * e0) ** 2)))
    T = Pm.T / np.sqrt(s)[:, None]
    Tinv = Pm * np.sqrt(s)[None, :]
    v = T @ mu
    vn = float(np.linalg.norm(v))
    a = v / vn - e0
    if np.linalg.norm(a) > 0:
        a /= np.linalg.norm(a)
    H = np.eye(S) - 2.0 * np.outer(a, a)
    V, Vinv = H @ T, Tinv @ H
    if diagonalize and S > 1:
        Uavg = sum(w_vec[g] * M[g].T @ R.unpack(sig[g], D) @ M[g] for g in range(G))
        A = Vinv.T @ Uavg @ Vinv
        B = A[1:, 1:]
        _, E = _eig_desc(0.5 * (B + B.T))
        Rot = np.eye(S)
        Rot[1:, 1:] = E.T
        V, Vinv = Rot @ V, Vinv @ Rot.T
    M = M @ Vinv
    return dict(w_vec=w_vec, M=M, sigma_inv=sig, prior_offset=vn, V=V, updated=updated, eig_floored=eig_floored, var_floored=var_floored,
                var_floored_gauss=var_floored_gauss, prior_floored=prior_floored, impr_proj=impr_proj / frames, impr_var=impr_var / frames,
                impr_prior=impr_prior / frames, abs_proj=abs_proj / frames, abs_var=abs_var / frames, abs_prior=abs_prior / frames,
                num_ivectors=n, frames=frames, cond_R=cond_R, raw=raw, F=F, mu=mu, C=C)


# ------------------------------------------------------------------------------------------------------------------- init
_MASK = (1 << 64) - 1


def _mix(seed, counter):
    z = (seed * 0x9E3779B97F4A7C15 + counter) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    z ^= z >> 31
    return z >> 11


def init_normal(seed, n):
    """the n first entries of the generator of ivector-extractor-init"""
    out = np.zeros(n)
    for e in range(n):
        u1 = (_mix(seed, 2 * e) + 1) / 2.0 ** 53
        u2 = _mix(seed, 2 * e + 1) / 2.0 ** 53
        out[e] = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    return out


def init_model(weights, means, covars, S, seed=0, normal=None):
    """weights [G], means [G][D], covars [G][D][D] -> the model ivector-extractor-init builds; normal: the [G][D][S] draws to use
    instead of the generator's"""
    G, D = means.shape
    M = np.array(normal if normal is not None else init_normal(seed, G * D * S).reshape(G, D, S), dtype=np.float64)
    M[:, :, 0] = means / 100.0
    sig = np.stack([R.pack(np.linalg.inv(c)) for c in covars])
    return dict(w_vec=np.asarray(weights, np.float64), M=M, sigma_inv=sig, prior_offset=100.0)


# ------------------------------------------------------------------------------------------------------------------- EM data
def em_data(seed, G=4, D=5, S=3, n_utts=200, T=50):
    """Utterances drawn from a true model (y ~ N(e_0, I), one-hot posteriors with a random Gaussian per frame, x = M_g y + noise with
    covariances near (1 + g / 4) I, rounded to float) and the initial model built as ivector-extractor-init builds it, from per-Gaussian
    sample means and covariances."""
    rng = np.random.default_rng(seed)
    M_true = rng.normal(size=(G, D, S))
    chol = []
    for g in range(G):
        A = rng.normal(size=(D, D)) * 0.1
        chol.append(np.linalg.cholesky((1.0 + g / 4.0) * np.eye(D) + A @ A.T))
    utts, all_x, all_g = [], [], []
    for _ in range(n_utts):
        y = rng.normal(size=S)
        y[0] += 1.0
        gs = rng.integers(0, G, T)
        x = np.stack([M_true[g] @ y + chol[g] @ rng.normal(size=D) for g in gs]).astype(np.float32)
        utts.append((x, [(np.array([g], np.int32), np.array([1.0], np.float32)) for g in gs]))
        all_x.append(x.astype(np.float64))
        all_g.append(gs)
    X, gs = np.concatenate(all_x), np.concatenate(all_g)
    means = np.stack([X[gs == g].mean(axis=0) for g in range(G)])
    covars = np.stack([np.cov(X[gs == g].T, bias=True) for g in range(G)])
    weights = np.array([np.mean(gs == g) for g in range(G)])
    model = init_model(weights, means, covars, S, normal=rng.normal(size=(G, D, S)))
    return utts, model
