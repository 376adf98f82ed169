"""numpy restatement of the GMM classifiers (csrc/gmm_classify.h): second-stage Gaussian selection by a full-covariance model, frame
likelihoods, the VAD from frame likelihoods and the merging of two VADs.  Restated from the documented behaviour of Kaldi's
gmm/full-gmm.cc (GaussianSelectionPreselect), fgmmbin/fgmm-gselect.cc, fgmmbin/fgmm-global-get-frame-likes.cc,
ivectorbin/compute-vad-from-frame-likes.cc and ivectorbin/merge-vads.cc of early 2018: parity with a Kaldi binary is not pinned by
any test here.  The scores themselves are ubm_ref.full_loglikes."""
import io
import struct

import numpy as np

import ubm_ref as R

F = np.float32


# ------------------------------------------------------------------------------------------------------------------- ranking
def score_key(scores):
    """float32 -> uint32 with the same order, -inf below every finite score and a place for every NaN (the device's key).  The key
    is that of score + 0: the two zeros are one score"""
    b = (np.ascontiguousarray(scores, F) + F(0)).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def rerank(loglikes, preselect, n_out):
    """loglikes, preselect: [T, n_in] (slot order).  -> (indices, log-likelihoods), each [T, min(n_out, n_in)], best first: score
    descending, then Gaussian ascending, then slot ascending.  Duplicates of a preselection are kept as they come.  The scores
    are ranked as float32 (exact for the callers whose float64 scores are float32 values)."""
    ll = np.asarray(loglikes)
    pre = np.asarray(preselect, np.int64)
    assert ll.shape == pre.shape and ll.ndim == 2 and n_out >= 1
    T, n_in = ll.shape
    keep = min(n_out, n_in)
    key = score_key(ll.astype(F)).astype(np.int64)
    idx = np.zeros((T, keep), np.int32)
    out = np.zeros((T, keep), ll.dtype)
    slots = np.arange(n_in)
    for t in range(T):
        order = np.lexsort((slots, pre[t], -key[t]))[:keep]   # the last key is the primary one
        idx[t] = pre[t][order]
        out[t] = ll[t][order]
    return idx, out


def logsumexp(loglikes):
    """[T, n] -> [T] float64; a frame whose scores are all -inf gives -inf"""
    ll = np.asarray(loglikes, np.float64)
    mx = ll.max(1)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(mx), safe + np.log(np.exp(ll - safe[:, None]).sum(1)), mx)


def average_like(likes):
    """the float32 frame likelihoods summed in float64 in frame order, divided by their number, rounded once"""
    tot = 0.0
    for x in np.asarray(likes, F).tolist():
        tot += x
    return F(tot / len(likes))


# ------------------------------------------------------------------------------------------------------------------- decisions
def vad_from_frame_likes(likes, priors=None, label_map=None):
    """likes: one [T] array per class.  Frame t: the first j that maximises like_j + log(prior_j) in float32 (a later class wins by
    strict > only); the label is label_map[j], or j"""
    likes = [np.asarray(v, F) for v in likes]
    n = len(likes)
    if priors is not None:
        assert len(priors) == n and all(p > 0 for p in priors)
    lp = [F(0) if priors is None else F(np.log(np.float64(F(p)))) for p in (priors if priors is not None else [1] * n)]
    out = np.zeros(len(likes[0]), F)
    for t in range(len(out)):
        best, best_score = 0, F(likes[0][t] + lp[0])
        for j in range(1, n):
            s = F(likes[j][t] + lp[j])
            if s > best_score:
                best, best_score = j, s
        out[t] = label_map[best] if label_map is not None else best
    return out


def merge_vads(a, b, triples=None):
    """without triples 1 iff both are 1; with (a, b, c) triples the pair (a, b) gives c, KeyError for a pair without one"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    assert a.shape == b.shape
    if triples is None:
        return ((a == 1) & (b == 1)).astype(F)
    m = {(int(x), int(y)): int(z) for x, y, z in triples}
    return np.array([m[(int(x), int(y))] for x, y in zip(a, b)], F)


# ------------------------------------------------------------------------------------------------------------------- models
def integer_full_model(G, D):
    """The full-covariance half of test_gpu_ubm.integer_models, the same recipe: small integers, gconst_g carries g * 2^-10, which
    makes every score of a frame different from every other (the rest of a score is a multiple of 1/2)."""
    rng = np.random.default_rng(1000 * G + D)
    g = np.arange(G)
    ic = np.zeros((G, D * (D + 1) // 2), F)
    for k in range(G):
        a = np.tril(rng.integers(-1, 2, (D, D)), -1).astype(np.float64)
        ic[k] = R.pack(a + a.T + np.diag(rng.integers(1, 3, D)))
    return dict(gconsts=(rng.integers(-8, 9, G) + g * 2.0 ** -10).astype(F), means_invcovars=rng.integers(-2, 3, (G, D)).astype(F),
                inv_covars=ic)


# ------------------------------------------------------------------------------------------------------------------- tables
def float_table_bytes(items, binary=True):
    """items: [(key, float)]: text "key value\\n"; binary "key " then \\0B, the size byte 4 and the four bytes"""
    f = io.BytesIO()
    for key, v in items:
        f.write(key.encode() + b" ")
        if binary:
            f.write(b"\0B\x04" + struct.pack("<f", v))
        else:
            f.write(b"%.9g\n" % float(F(v)))
    return f.getvalue()


def read_float_table(data):
    """-> [(key, float32)] of a text or binary float table"""
    out, p = [], 0
    while p < len(data):
        e = data.index(b" ", p)
        key = data[p:e].decode()
        p = e + 1
        if data[p:p + 2] == b"\0B":
            assert data[p + 2:p + 3] == b"\x04"
            out.append((key, F(struct.unpack("<f", data[p + 3:p + 7])[0])))
            p += 7
        else:
            e = data.index(b"\n", p)
            out.append((key, F(float(data[p:e].decode().strip()))))
            p = e + 1
    return out


def vector_table_bytes(items, binary=True):
    """items: [(key, float vector)]"""
    f = io.BytesIO()
    for key, v in items:
        v = np.asarray(v, F)
        f.write(key.encode() + b" ")
        if binary:
            f.write(b"\0BFV \x04" + struct.pack("<i", v.size) + v.tobytes())
        else:
            f.write(b" [ " + b"".join(b"%.9g " % float(x) for x in v) + b"]\n")
    return f.getvalue()


def read_vector_table(data):
    """-> [(key, float32 vector)] of a text or binary table of float vectors"""
    out, p = [], 0
    while p < len(data):
        e = data.index(b" ", p)
        key = data[p:e].decode()
        p = e + 1
        if data[p:p + 2] == b"\0B":
            assert data[p + 2:p + 5] == b"FV " and data[p + 5:p + 6] == b"\x04", data[p:p + 8]
            n = struct.unpack("<i", data[p + 6:p + 10])[0]
            out.append((key, np.frombuffer(data[p + 10:p + 10 + 4 * n], F).copy()))
            p += 10 + 4 * n
        else:
            e = data.index(b"]", p)
            words = data[p:e].decode().split()
            assert words[0] == "["
            out.append((key, np.array([float(w) for w in words[1:]], F)))
            p = data.index(b"\n", e) + 1
    return out
