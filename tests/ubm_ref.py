"""numpy restatement of the GMM-UBM stage (csrc/ubm.h): add-deltas in float32 exactly as the header states it, everything else
in float64, plus the model and table files in Python (binary and text, write and read)."""
import io
import struct

import numpy as np

F = np.float32
LOG2PI = float(np.log(2.0 * np.pi))


# ------------------------------------------------------------------------------------------------------------------- deltas
def delta_scales(order, window):
    scales = [np.ones(1, F)]
    for _ in range(order):
        prev = scales[-1]
        cur = np.zeros(prev.size + 2 * window, F)
        normalizer = F(0)
        for j in range(-window, window + 1):
            normalizer = F(normalizer + F(j * j))
            for k in range(prev.size):
                cur[k + j + window] = F(cur[k + j + window] + F(F(j) * prev[k]))
        scales.append((cur * F(1.0 / float(normalizer))).astype(F))
    return scales


def add_deltas(x, order=2, window=2, truncate=0):
    x = np.asarray(x, F)
    if truncate > 0:
        x = x[:, :truncate]
    T, D = x.shape
    out = np.zeros((T, (order + 1) * D), F)
    t = np.arange(T)
    for i, sc in enumerate(delta_scales(order, window)):
        half = i * window
        acc = np.zeros((T, D), F)
        for j in range(-half, half + 1):
            s = sc[j + half]
            if s == 0:
                continue
            acc = (acc + (s * x[np.clip(t + j, 0, T - 1)]).astype(F)).astype(F)
        out[:, i * D:(i + 1) * D] = acc
    return out


# ------------------------------------------------------------------------------------------------------------------- models
def unpack(packed, dim):
    """[tri] packed lower triangle -> symmetric [dim, dim] float64"""
    a = np.zeros((dim, dim))
    a[np.tril_indices(dim)] = np.asarray(packed, np.float64)
    return a + np.tril(a, -1).T


def pack(sym):
    return np.asarray(sym)[np.tril_indices(np.asarray(sym).shape[0])]


def diag_gconsts(weights, means_invvars, inv_vars):
    w, mi, iv = (np.asarray(a, np.float64) for a in (weights, means_invvars, inv_vars))
    return np.log(w) - 0.5 * (LOG2PI * mi.shape[1] - np.log(iv).sum(1) + (mi * mi / iv).sum(1))


def full_gconsts(weights, means_invcovars, inv_covars):
    w, b = np.asarray(weights, np.float64), np.asarray(means_invcovars, np.float64)
    out = np.zeros(len(w))
    for g in range(len(w)):
        a = unpack(inv_covars[g], b.shape[1])
        sign, logdet_inv = np.linalg.slogdet(a)
        out[g] = np.log(w[g]) - 0.5 * (LOG2PI * b.shape[1] - logdet_inv + b[g] @ np.linalg.solve(a, b[g]))
    return out


def fgmm_to_gmm(weights, means_invcovars, inv_covars):
    b = np.asarray(means_invcovars, np.float64)
    G, D = b.shape
    mi, iv = np.zeros((G, D)), np.zeros((G, D))
    for g in range(G):
        sigma = np.linalg.inv(unpack(inv_covars[g], D))
        iv[g] = 1.0 / np.diag(sigma)
        mi[g] = (sigma @ b[g]) * iv[g]
    return diag_gconsts(weights, mi, iv), mi, iv


def diag_loglikes(x, gconsts, means_invvars, inv_vars):
    x = np.asarray(x, np.float64)
    return (np.asarray(gconsts, np.float64)[None] + x @ np.asarray(means_invvars, np.float64).T
            - 0.5 * (x * x) @ np.asarray(inv_vars, np.float64).T)


def diag_abs_terms(x, gconsts, means_invvars, inv_vars):
    """S of the summation bound: the sum of the absolute values of the 2 D + 1 terms"""
    x = np.abs(np.asarray(x, np.float64))
    return (np.abs(np.asarray(gconsts, np.float64))[None] + x @ np.abs(np.asarray(means_invvars, np.float64)).T
            + 0.5 * (x * x) @ np.abs(np.asarray(inv_vars, np.float64)).T)


def gselect(loglikes, n):
    """the n largest per frame, descending; equal scores: the lower index first"""
    return np.argsort(-loglikes, axis=1, kind="stable")[:, :n].astype(np.int32)


def full_loglikes(x, gconsts, means_invcovars, inv_covars, sel, absolute=False):
    """[T, n] log-likelihoods of the selected Gaussians (absolute: the sums of the absolute values of the D^2 + D + 1 terms)"""
    x = np.asarray(x, np.float64)
    b = np.asarray(means_invcovars, np.float64)
    D = x.shape[1]
    out = np.zeros(sel.shape)
    for g in np.unique(sel):
        a = unpack(inv_covars[g], D)
        t, s = np.nonzero(sel == g)
        xg = x[t]
        if absolute:
            out[t, s] = abs(float(gconsts[g])) + np.abs(xg) @ np.abs(b[g]) + 0.5 * np.einsum("ti,ij,tj->t", np.abs(xg), np.abs(a), np.abs(xg))
        else:
            out[t, s] = float(gconsts[g]) + xg @ b[g] - 0.5 * np.einsum("ti,ij,tj->t", xg, a, xg)
    return out


def gamma(m):
    u = 2.0 ** -24
    return m * u / (1.0 - m * u)


def posteriors(loglikes, min_post=0.0):
    """[T, n] float64 posteriors with the pruned ones at 0, and the per-frame log-sums.  A frame whose largest selected
    log-likelihood is not finite has no posterior: every slot is 0 and the log-sum is that largest value (-inf, or NaN)."""
    ll = np.asarray(loglikes, np.float64)
    mx = ll.max(1, keepdims=True)   # a NaN in the row makes it NaN
    bad = ~np.isfinite(mx[:, 0])
    if bad.any():
        good = np.where(bad[:, None], 0.0, ll)
        p, logsum = posteriors(good, min_post)
        p[bad] = 0.0
        logsum[bad] = mx[bad, 0]
        return p, logsum
    e = np.exp(ll - mx)
    s = e.sum(1, keepdims=True)
    p = e / s
    if min_post != 0.0:
        arg = ll.argmax(1)
        p = np.where(p < min_post, 0.0, p)
        kept = p.sum(1)
        for t in range(len(p)):
            if kept[t] == 0.0:
                p[t, arg[t]] = 1.0
            else:
                p[t] /= kept[t]
    return p, (mx + np.log(s))[:, 0]


def scale_post(post, scale):
    if scale == 1.0:
        return post
    if scale == 0.0:
        return [[] for _ in post]
    return [[(i, float(F(F(p) * F(scale)))) for i, p in frame] for frame in post]


# ------------------------------------------------------------------------------------------------------------------- files
def _tok(f, t):
    f.write(t.encode() + b" ")


def _int(f, v, binary):
    f.write(b"\x04" + struct.pack("<i", v) if binary else b"%d " % v)


def _vec(f, v, binary):
    v = np.asarray(v, F)
    if binary:
        f.write(b"FV ")
        _int(f, v.size, True)
        f.write(v.tobytes())
    else:
        f.write(b" [ " + b"".join(b"%.9g " % float(x) for x in v) + b"]\n")


def _mat(f, m, binary):
    m = np.asarray(m, F)
    if binary:
        f.write(b"FM ")
        _int(f, m.shape[0], True)
        _int(f, m.shape[1], True)
        f.write(np.ascontiguousarray(m).tobytes())
    else:
        f.write(b" [\n")
        for r, row in enumerate(m):
            f.write(b"  " + b"".join(b"%.9g " % float(x) for x in row) + (b"]\n" if r + 1 == len(m) else b"\n"))


def _packed(f, p, dim, binary):
    p = np.asarray(p, F)
    if binary:
        f.write(b"FP ")
        _int(f, dim, True)
        f.write(p.tobytes())
    else:
        f.write(b" [\n")
        k = 0
        for i in range(dim):
            f.write(b"  " + b"".join(b"%.9g " % float(x) for x in p[k:k + i + 1]) + (b"]\n" if i + 1 == dim else b"\n"))
            k += i + 1


def diag_gmm_bytes(weights, means_invvars, inv_vars, binary=True, gconsts=None):
    f = io.BytesIO()
    f.write(b"\0B" if binary else b"")
    _tok(f, "<DiagGMM>")
    if gconsts is not None:
        _tok(f, "<GCONSTS>")
        _vec(f, gconsts, binary)
    _tok(f, "<WEIGHTS>")
    _vec(f, weights, binary)
    _tok(f, "<MEANS_INVVARS>")
    _mat(f, means_invvars, binary)
    _tok(f, "<INV_VARS>")
    _mat(f, inv_vars, binary)
    _tok(f, "</DiagGMM>")
    return f.getvalue()


def full_gmm_bytes(weights, means_invcovars, inv_covars, binary=True, gconsts=None):
    f = io.BytesIO()
    f.write(b"\0B" if binary else b"")
    _tok(f, "<FullGMM>")
    if gconsts is not None:
        _tok(f, "<GCONSTS>")
        _vec(f, gconsts, binary)
    _tok(f, "<WEIGHTS>")
    _vec(f, weights, binary)
    _tok(f, "<MEANS_INVCOVARS>")
    _mat(f, means_invcovars, binary)
    _tok(f, "<INV_COVARS>")
    dim = np.asarray(means_invcovars).shape[1]
    for p in inv_covars:
        _packed(f, p, dim, binary)
    _tok(f, "</FullGMM>")
    return f.getvalue()


class _In:
    def __init__(self, data):
        self.d, self.p = data, 0

    def peek(self):
        return self.d[self.p:self.p + 1]

    def take(self, n):
        out = self.d[self.p:self.p + n]
        assert len(out) == n, "unexpected end of data"
        self.p += n
        return out

    def token(self):
        while self.peek().isspace():
            self.p += 1
        a = self.p
        while self.p < len(self.d) and not self.d[self.p:self.p + 1].isspace():
            self.p += 1
        out = self.d[a:self.p].decode()
        self.p += 1
        return out

    def int32(self, binary):
        if binary:
            assert self.take(1) == b"\x04"
            return struct.unpack("<i", self.take(4))[0]
        return int(self.token())

    def float32(self, binary):
        if binary:
            assert self.take(1) == b"\x04"
            return struct.unpack("<f", self.take(4))[0]
        return float(self.token())

    def numbers(self):
        """text ' [ ... ]' -> (values, number of rows)"""
        assert self.token() == "["
        vals, rows, in_row = [], 0, False
        while True:
            while self.peek() in (b" ", b"\t"):
                self.p += 1
            c = self.peek()
            if c == b"\n":
                self.p += 1
                rows += in_row
                in_row = False
            elif c == b"]":
                self.p += 1
                rows += in_row
                if self.peek() == b"\n":
                    self.p += 1
                return np.array(vals, np.float64), rows
            else:
                vals.append(float(self.token()))
                self.p -= 1   # token() took the separator: it may be the newline that closes a row
                in_row = True

    def vector(self, binary):
        if not binary:
            return self.numbers()[0].astype(F)
        t = self.token()
        n = self.int32(True)
        return np.frombuffer(self.take(n * (4 if t == "FV" else 8)), F if t == "FV" else np.float64).astype(F)

    def matrix(self, binary):
        if not binary:
            v, rows = self.numbers()
            return v.astype(F).reshape(rows, -1)
        t = self.token()
        r, c = self.int32(True), self.int32(True)
        return np.frombuffer(self.take(r * c * (4 if t == "FM" else 8)), F if t == "FM" else np.float64).astype(F).reshape(r, c)

    def packed(self, binary):
        if not binary:
            return self.numbers()[0].astype(F)
        t = self.token()
        assert t in ("FP", "DP"), t
        d = self.int32(True)
        n = d * (d + 1) // 2
        return np.frombuffer(self.take(n * (4 if t == "FP" else 8)), F if t == "FP" else np.float64).astype(F)


def _header(i):
    if i.d[i.p:i.p + 2] == b"\0B":
        i.p += 2
        return True
    return False


def read_diag_gmm(data):
    """-> dict(gconsts, weights, means_invvars, inv_vars)"""
    i = _In(data)
    b = _header(i)
    assert i.token() == "<DiagGMM>"
    out = {}
    t = i.token()
    if t == "<GCONSTS>":
        out["gconsts"] = i.vector(b)
        t = i.token()
    assert t == "<WEIGHTS>", t
    out["weights"] = i.vector(b)
    assert i.token() == "<MEANS_INVVARS>"
    out["means_invvars"] = i.matrix(b)
    assert i.token() == "<INV_VARS>"
    out["inv_vars"] = i.matrix(b)
    assert i.token() == "</DiagGMM>"
    return out


def read_full_gmm(data):
    i = _In(data)
    b = _header(i)
    assert i.token() == "<FullGMM>"
    out = {}
    t = i.token()
    if t == "<GCONSTS>":
        out["gconsts"] = i.vector(b)
        t = i.token()
    assert t == "<WEIGHTS>", t
    out["weights"] = i.vector(b)
    assert i.token() == "<MEANS_INVCOVARS>"
    out["means_invcovars"] = i.matrix(b)
    assert i.token() == "<INV_COVARS>"
    out["inv_covars"] = np.stack([i.packed(b) for _ in out["weights"]])
    assert i.token() == "</FullGMM>"
    return out


def gselect_table_bytes(items, binary=True):
    """items: [(key, int array [T, n] or list of lists)]"""
    f = io.BytesIO()
    for key, sel in items:
        f.write(key.encode() + b" ")
        if binary:
            f.write(b"\0B")
            _int(f, len(sel), True)
            for row in sel:
                row = np.asarray(row, np.int32)
                f.write(b"\x04" + struct.pack("<i", row.size) + row.tobytes())
        else:
            f.write(b"".join(b"".join(b"%d " % int(v) for v in row) + b"; " for row in sel) + b"\n")
    return f.getvalue()


def post_table_bytes(items, binary=True):
    """items: [(key, [[(index, posterior), ...] per frame])]"""
    f = io.BytesIO()
    for key, post in items:
        f.write(key.encode() + b" ")
        if binary:
            f.write(b"\0B")
            _int(f, len(post), True)
            for frame in post:
                _int(f, len(frame), True)
                for idx, p in frame:
                    _int(f, int(idx), True)
                    f.write(b"\x04" + struct.pack("<f", p))
        else:
            f.write(b"".join(b"[ " + b"".join(b"%d %.9g " % (int(i), float(p)) for i, p in frame) + b"] " for frame in post) + b"\n")
    return f.getvalue()


def _entries(data):
    i = _In(data)
    while True:
        while i.peek().isspace():
            i.p += 1
        if i.p >= len(i.d):
            return
        key = i.token()
        yield key, i, _header(i)


def _line(i):
    e = i.d.index(b"\n", i.p)
    out = i.d[i.p:e].decode().split()
    i.p = e + 1
    return out


def read_gselect_table(data):
    out = []
    for key, i, b in _entries(data):
        if b:
            sel = []
            for _ in range(i.int32(True)):
                assert i.take(1) == b"\x04"
                k = struct.unpack("<i", i.take(4))[0]
                sel.append(np.frombuffer(i.take(4 * k), np.int32).tolist())
        else:
            sel, cur = [], []
            for w in _line(i):
                if w == ";":
                    sel.append(cur)
                    cur = []
                else:
                    cur.append(int(w))
            assert not cur
        out.append((key, sel))
    return out


def read_post_table(data):
    out = []
    for key, i, b in _entries(data):
        post = []
        if b:
            for _ in range(i.int32(True)):
                post.append([(i.int32(True), i.float32(True)) for _ in range(i.int32(True))])
        else:
            words = _line(i)
            k = 0
            while k < len(words):
                assert words[k] == "["
                e = words.index("]", k)
                post.append([(int(words[j]), float(words[j + 1])) for j in range(k + 1, e, 2)])
                k = e + 1
        out.append((key, post))
    return out


# ------------------------------------------------------------------------------------------------------------------- synthetic models
def random_full_model(seed, G, D, spread=3.0):
    """Sigma_g = A A' / D + I, means spread * N(0, 1): (weights, means [G, D] float64, means_invcovars, inv_covars packed), the
    stored arrays in float32"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, G)
    w = (w / w.sum()).astype(F)
    means = spread * rng.normal(size=(G, D))
    b, ic = np.zeros((G, D), F), np.zeros((G, D * (D + 1) // 2), F)
    for g in range(G):
        a = rng.normal(size=(D, D))
        inv = np.linalg.inv(a @ a.T / D + np.eye(D))
        inv = 0.5 * (inv + inv.T)
        ic[g] = pack(inv).astype(F)
        b[g] = (unpack(ic[g], D) @ means[g]).astype(F)
    return w, means, b, ic


def frames_around(seed, means, T, noise=1.0):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, len(means), T)
    return (means[g] + noise * rng.normal(size=(T, means.shape[1]))).astype(F)
