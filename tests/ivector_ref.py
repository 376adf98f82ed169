"""i-vector extraction restated in numpy (float64), and final.ie laid down byte by byte.  [UPSTREAM, recalled]: written from the
documented behaviour of Kaldi's ivector/ivector-extractor.cc and ivectorbin/ivector-extract.cc of early 2018; Kaldi is not part of
the reference tree, so parity with a Kaldi binary is not pinned.  Independent of csrc/ivex.h, which states the same semantics."""
import io
import struct

import numpy as np


def packed_index(r, c):
    """where element (r, c), r >= c, of a symmetric matrix sits in its packed lower triangle"""
    assert r >= c
    return r * (r + 1) // 2 + c


def pack(sym):
    r, c = np.tril_indices(sym.shape[0])
    return np.asarray(sym, np.float64)[r, c]


def unpack(packed, dim):
    out = np.zeros((dim, dim))
    r, c = np.tril_indices(dim)
    out[r, c] = packed
    out[c, r] = packed
    return out


def derived(M, sigma_inv):
    """SigmaInvM [G D][S] and U [G][S (S + 1) / 2] from M [G][D][S] and the packed inverse covariances [G][D (D + 1) / 2]"""
    G, D, S = M.shape
    sim = np.stack([unpack(sigma_inv[g], D) @ M[g] for g in range(G)])
    U = np.stack([pack(M[g].T @ sim[g]) for g in range(G)])
    return sim.reshape(G * D, S), U


def scale_posteriors(post, acoustic_weight=1.0, max_count=0.0):
    """post: per frame (indices, float32 weights).  Returns (the scaled posterior, the float32 scale, whether max-count bit)."""
    total = 0.0
    for _, w in post:
        for v in np.asarray(w, np.float32):
            total += float(v)
    tot = acoustic_weight * float(np.float32(total))
    clipped = max_count > 0 and tot > max_count
    scale = np.float32(acoustic_weight * max_count / tot) if clipped else np.float32(acoustic_weight)
    return [(np.asarray(i, np.int64), np.asarray(w, np.float32) * scale) for i, w in post], scale, clipped


def stats(x, post, G):
    """gamma [G] and X [G][D]: float64, frames in ascending order"""
    x = np.asarray(x, np.float32)
    gamma, X = np.zeros(G), np.zeros((G, x.shape[1]))
    for t, (idx, w) in enumerate(post):
        for g, v in zip(idx, w):
            gamma[g] += float(v)
            X[g] += float(v) * x[t].astype(np.float64)
    return gamma, X


def terms(sim, U, gamma, X, prior_offset):
    """l [S] and Q [S][S]"""
    S = sim.shape[1]
    l = sim.T @ X.reshape(-1)
    l[0] += prior_offset
    return l, unpack(gamma @ U, S) + np.eye(S)


def auxf(l, Q, v):
    return float(l @ v - 0.5 * v @ Q @ v)


def extract(x, post, M, sigma_inv, prior_offset, acoustic_weight=1.0, max_count=0.0, sim_U=None):
    """dict(ivector float32 [S], x float64 [S], auxf_change, gamma, X, linear, quadratic)"""
    G, D, S = M.shape
    sim, U = sim_U if sim_U is not None else derived(M, sigma_inv)
    scaled, _, _ = scale_posteriors(post, acoustic_weight, max_count)
    gamma, X = stats(x, scaled, G)
    l, Q = terms(sim, U, gamma, X, prior_offset)
    sol = np.linalg.solve(Q, l)
    e0 = np.zeros(S)
    e0[0] = prior_offset
    out = sol.copy()
    out[0] -= prior_offset
    return dict(ivector=out.astype(np.float32), x=sol, auxf_change=auxf(l, Q, sol) - auxf(l, Q, e0), gamma=gamma, X=X.reshape(-1),
                linear=l, quadratic=Q)


# ----------------------------------------------------------------------------------------------------------------- final.ie
def _tok(f, t):
    f.write(t.encode() + b" ")


def _int(f, v, binary):
    f.write(b"\x04" + struct.pack("<i", v) if binary else b"%d " % v)


def _num(v):
    return repr(float(v)).encode()   # the shortest text that reads back as the same float64


def _vec(f, v, binary):
    v = np.asarray(v, np.float64)
    if binary:
        f.write(b"DV ")
        _int(f, len(v), True)
        f.write(v.astype("<f8").tobytes())
    else:
        f.write(b" [ " + b"".join(_num(a) + b" " for a in v) + b"]\n")


def _mat(f, m, binary):
    m = np.asarray(m, np.float64)
    if binary:
        f.write(b"DM ")
        _int(f, m.shape[0], True)
        _int(f, m.shape[1], True)
        f.write(m.astype("<f8").tobytes())
    elif m.shape[0] == 0:
        f.write(b" [ ]\n")
    else:
        f.write(b" [")
        for row in m:
            f.write(b"\n  " + b"".join(_num(a) + b" " for a in row))
        f.write(b"]\n")


def _packed(f, p, dim, binary):
    p = np.asarray(p, np.float64)
    if binary:
        f.write(b"DP ")
        _int(f, dim, True)
        f.write(p.astype("<f8").tobytes())
    else:
        f.write(b" [\n")
        k = 0
        for i in range(dim):
            f.write(b"  " + b"".join(_num(a) + b" " for a in p[k:k + i + 1]))
            k += i + 1
            f.write(b"]\n" if i + 1 == dim else b"\n")


def ie_bytes(w_vec, M, sigma_inv, prior_offset, binary=True, w_rows=0, closing="</IvectorExtractor>"):
    """<IvectorExtractor> <w> DM <w_vec> DV <M> int32 G, G x DM <SigmaInv> G x DP <IvectorOffset> double </IvectorExtractor>"""
    G, D, S = M.shape
    f = io.BytesIO()
    if binary:
        f.write(b"\0B")
    _tok(f, "<IvectorExtractor>")
    _tok(f, "<w>")
    _mat(f, np.zeros((w_rows, S + 1 if w_rows else 0)), binary)
    _tok(f, "<w_vec>")
    _vec(f, w_vec, binary)
    _tok(f, "<M>")
    _int(f, G, binary)
    for g in range(G):
        _mat(f, M[g], binary)
    _tok(f, "<SigmaInv>")
    for g in range(G):
        _packed(f, sigma_inv[g], D, binary)
    _tok(f, "<IvectorOffset>")
    f.write(b"\x08" + struct.pack("<d", prior_offset) if binary else _num(prior_offset) + b" ")
    _tok(f, closing)
    if not binary:
        f.write(b"\n")
    return f.getvalue()


# ----------------------------------------------------------------------------------------------------------------- test models
def integer_model(seed, G, D, S):
    """M in [-2, 2]; Sigma^-1 = L L' with L unit lower triangular and about a tenth of its strict lower part in {-1, 1}: integer
    and positive definite.  Every derived variable is then an integer that float64 holds exactly."""
    rng = np.random.default_rng(seed)
    M = rng.integers(-2, 3, (G, D, S)).astype(np.float64)
    sig = np.zeros((G, D * (D + 1) // 2))
    for g in range(G):
        L = np.tril(rng.choice([-1.0, 1.0], (D, D)) * (rng.random((D, D)) < 0.1), -1) + np.eye(D)
        sig[g] = pack(L @ L.T)
    return dict(w_vec=np.full(G, 1.0 / G), M=M, sigma_inv=sig, prior_offset=float(rng.integers(1, 4)))


def zero_leading_columns(model, s0):
    """the model with the first s0 columns of every M_g set to zero: rows and columns below s0 of every U_g vanish, so the leading
    s0 x s0 block of every Q is the identity, nothing couples it to the rest, and no pivot before index s0 can be bad"""
    out = dict(model, M=np.array(model["M"], dtype=np.float64))
    out["M"][:, :, :s0] = 0.0
    return out


def random_model(seed, G, D, S, m_scale=0.3):
    """Sigma^-1 = A A' / D + I, M Gaussian scaled so that Q stays well conditioned: Q - I grows with S at a fixed scale, so a large
    S wants a smaller m_scale (tests/ivector_cases.py's m_scale_for)"""
    rng = np.random.default_rng(seed)
    M = rng.normal(0.0, m_scale, (G, D, S))
    sig = np.zeros((G, D * (D + 1) // 2))
    for g in range(G):
        A = rng.normal(size=(D, D))
        sig[g] = pack(A @ A.T / D + np.eye(D))
    return dict(w_vec=np.full(G, 1.0 / G), M=M, sigma_inv=sig, prior_offset=float(rng.uniform(1.0, 3.0)))


def integer_utterance(seed, T, G, D, n=3, empty_every=0):
    """features in [-4, 4], posteriors 2^-k with k <= 3 on up to n distinct Gaussians per frame"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (T, D)).astype(np.float32)
    post = []
    for t in range(T):
        k = 0 if (empty_every and t % empty_every == 1) else int(rng.integers(1, min(n, G) + 1))
        post.append((rng.permutation(G)[:k].astype(np.int32), (2.0 ** -rng.integers(0, 4, k)).astype(np.float32)))
    return x, post
