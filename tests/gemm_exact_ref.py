"""Exact reference of the spliced-GEMM kernels (tdnn_gemm_kernel, _v2, _sk<4|8>, _p8 and split-K), plain numpy.

The operands are built so that every product and every partial sum of a launch is an exact fp32 number: hi planes hold
small integers, lo planes small integer multiples of one power of two 2^-q, bias and BatchNorm offset multiples of the same
unit, the BatchNorm scale a power of two.  Under the precondition

    sum |terms| * 2^q < 2^24    for every output element (epilogue values and statistics sums included)

any order of summation gives the same fp32 bits, so every kernel variant, every stream-K cut and every epilogue has exactly
one right answer per element and the GPU tests compare bit patterns with no tolerance.  The precondition is a condition on
the operands, checked on the CPU (check_precondition); it is not derived from what a kernel returns.

What a precision sums is taken from csrc/kernels.h (PrecXPlanes, PrecWPlanes, PrecPasses), the launch rules from
csrc/kernels.hip (launch_one, sk_applicable, launch_one_sk, launch_one_p8 and the partition at the top of
tdnn_gemm_kernel_sk / tdnn_gemm_kernel_p8), the walk order from PlanWalkGroups / PlanWalkSteps / PlanWalkSteps64."""
import numpy as np

KBM, KBN, KBK = 128, 128, 32
HALO = 32                      # rows kept around every plane (the engine's kHalo)
BIT_BUDGET = 24                # bits of an fp32 significand: the precondition's bound is 2^BIT_BUDGET

PREC_BF16X3, PREC_BF16, PREC_FP16, PREC_FP16X3, PREC_FP16X2 = 0, 1, 2, 3, 4
PREC_FP16MX, PREC_FP16MX2, PREC_FP16X3E, PREC_FP16MXE = 6, 7, 8, 9
EPI_ACT, EPI_F32, EPI_STATS = 0, 1, 2
PREC_NAME = {0: "bf16x3", 1: "bf16", 2: "fp16", 3: "fp16x3", 4: "fp16x2", 5: "auto", 6: "fp16mx", 7: "fp16mx2", 8: "fp16x3e",
             9: "fp16mxe"}
EPI_NAME = {0: "act", 1: "f32", 2: "stats", 3: "splitk"}

SENT16 = 0xABCD                # what the output buffers hold where nothing may be written
SENT8 = 0xA5
SENT_F32 = np.float32(-7.0)
SENT_U32 = 0xDEADBEEF


# ---- kernels.h: what a precision is -----------------------------------------------------------------------------------------------
def prec_f16(p):
    return p in (2, 3, 4, 5, 6, 7, 8, 9)


def prec_mx(p):
    return p in (6, 7, 9)


def prec_mx2(p):
    return p == 7


def prec_emits_lo4(p):
    return p in (7, 8, 9)


def prec_x_planes(p):
    return 2 if p in (0, 3, 8) else 1


def prec_w_planes(p):
    return 2 if p in (0, 3, 4, 5, 6, 7, 8, 9) else 1


def prec_passes(p):
    return prec_x_planes(p) + prec_w_planes(p) - 1


def lo4_scale_pitch(ld):
    return ((ld >> 6) + 3) & ~3


def splitk_steps_per_slice(ksteps):
    per = (ksteps + 23) // 24
    return 4 if per < 4 else per


def splitk_slices(ksteps):
    per = splitk_steps_per_slice(ksteps)
    return (ksteps + per - 1) // per


# ---- 16-bit formats ---------------------------------------------------------------------------------------------------------------
def rne16(z, f16):
    """fp32 values (given as float64 or float32, exactly representable in fp32) -> 16-bit patterns, round to nearest even."""
    z32 = np.asarray(z, dtype=np.float32)
    if f16:
        with np.errstate(over="ignore"):
            return z32.astype(np.float16).view(np.uint16)
    u = z32.view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(z32), np.uint16(0x7FC0), r)


def trunc16(z, f16):
    """The wrong conversion (round towards zero): what test_gemm_exact_ref.py shows the operands distinguish from rne16."""
    z32 = np.asarray(z, dtype=np.float32)
    if not f16:
        return (z32.view(np.uint32) >> 16).astype(np.uint16)
    h = z32.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(z32)
    return np.where(over, h.view(np.uint16) - 1, h.view(np.uint16)).astype(np.uint16)


def val16(u, f16):
    """16-bit patterns -> float64"""
    u = np.asarray(u, dtype=np.uint16)
    if f16:
        return u.view(np.float16).astype(np.float64)
    return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def nan16(f16):
    return 0x7E00 if f16 else 0x7FC0


# ---- the 4-bit (e2m1) images: restatements of the planes epilogue and of the weight packer ---------------------------------------
E2M1_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _q_e2m1(t):
    """round to nearest (ties to the even code) onto the e2m1 grid, saturating at 6 - v_cvt_scalef32_pk_fp4_f16 / _f32"""
    t = np.asarray(t, dtype=np.float64)
    a = np.abs(t)
    idx = ((a > 0.25).astype(np.int64) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    return np.sign(t) * E2M1_GRID[idx]


def _lo4_plane(x32, xh):
    """What the planes epilogue of XV_PREC_FP16MX2 / FP16X3E / FP16MXE writes next to the fp16 plane xh (values) of the fp32
    values x32: the e2m1 codes of r = x32 - xh with one scale 2^(E - 13) per row and 64 columns (E = exponent of the block's
    largest |x32|: every residual then lies in [-4, 4]), packed two per byte; the E8M0 scale bytes (rows padded to whole
    dwords); and the decoded values.  numpy arrays in, (uint8 [rows, n / 2], uint8 [rows, pitch], float64 [rows, n]) out."""
    x32 = np.asarray(x32, dtype=np.float32)
    r = x32.astype(np.float64) - np.asarray(xh, dtype=np.float64)
    rows, n = r.shape
    b = r.reshape(rows, n // 64, 64)
    m = np.abs(x32).reshape(rows, n // 64, 64).max(axis=2, keepdims=True)
    ebits = ((m.view(np.uint32) >> 23) & 255).astype(np.int64)
    e8 = np.where(ebits < 113, 100, np.where(ebits > 254, 241, ebits - 13))
    sc = 2.0 ** (e8.astype(np.float64) - 127)
    q = _q_e2m1(b / sc)
    code = (np.abs(q)[..., None] == E2M1_GRID).argmax(axis=-1) | ((b < 0).astype(np.int64) << 3)
    code = code.reshape(rows, n)
    packed = np.ascontiguousarray((code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8))
    e8p = np.zeros((rows, lo4_scale_pitch(n)), dtype=np.uint8)
    e8p[:, :n // 64] = e8.reshape(rows, n // 64).astype(np.uint8)
    return packed, e8p, (q * sc).reshape(rows, n)


def _w4_image(W):
    """4-bit image of the weights for the second walk: per row and 32 consecutive columns the smallest power of two 2^E
    with max |w| / 2^E <= 6, codes to nearest even - what xv_pack_mx_weights packs (values only)"""
    W = np.asarray(W, dtype=np.float64)
    n, K = W.shape
    b = W.reshape(n, K // 32, 32)
    m = np.abs(b).max(axis=2, keepdims=True)
    E = np.ceil(np.log2(np.maximum(m, 1e-300) / 6.0))
    sc = 2.0 ** E
    return (_q_e2m1(b / sc) * sc).reshape(n, K)


def _decode_lo4(lo4, lo4s, n_cols):
    """4-bit residual plane [rows, n_cols / 2] + E8M0 scales [rows, >= n_cols / 64] -> float64 [rows, n_cols]"""
    b = np.asarray(lo4, dtype=np.uint8)[:, :n_cols // 2]
    nib = np.stack([b & 15, b >> 4], axis=-1).reshape(b.shape[0], n_cols)
    val = np.where(nib & 8, -1.0, 1.0) * E2M1_GRID[nib & 7]
    sc = 2.0 ** (np.asarray(lo4s)[:, :n_cols // 64].astype(np.float64) - 127)
    return val * np.repeat(sc, 64, axis=1)


# ---- the K walk (kernels.h) -------------------------------------------------------------------------------------------------------
def plan_walk_groups(src_key, row_shift, ksteps):
    """PlanWalkGroups: consecutive segments over one source with the same length at uniformly spaced, increasing offsets
    (span <= 16 rows) form a group.  Returns dicts with first_seg, nshift, ksteps, shift0, dstep, wcol0, wstride."""
    out, wcol, j, nseg = [], 0, 0, len(src_key)
    while j < nseg:
        G = dict(first_seg=j, ksteps=ksteps[j], nshift=1, shift0=row_shift[j], dstep=0, wcol0=wcol, wstride=ksteps[j] * KBK)
        k = j + 1
        while k < nseg and src_key[k] == src_key[j] and ksteps[k] == ksteps[j]:
            d = row_shift[k] - row_shift[k - 1]
            if d <= 0 or (G["nshift"] > 1 and d != G["dstep"]) or row_shift[k] - row_shift[j] > 16:
                break
            G["dstep"] = d
            G["nshift"] += 1
            k += 1
        wcol += G["nshift"] * G["wstride"]
        out.append(G)
        j = k
    return out


def seg_groups(segs):
    """segs: [(source, ld, row_shift, k_len)].  The launcher's key: same plane pointers and leading dimension."""
    return plan_walk_groups([(s[0], s[1]) for s in segs], [s[2] for s in segs], [s[3] // KBK for s in segs])


def walk_steps(groups):
    """PlanWalkSteps: every 32-column step in walk order as (group, chunk, offset index, weight column)."""
    out = []
    for i, g in enumerate(groups):
        for kk in range(g["ksteps"]):
            for ij in range(g["nshift"]):
                out.append((i, kk, ij, g["wcol0"] + ij * g["wstride"] + kk * KBK))
    return out


def walk_tiles64(groups):
    """The K tiles (64 columns) of tdnn_gemm_kernel_p8 in its walk order (PlanWalkSteps64): (group, chunk, offset index)."""
    out = []
    for i, g in enumerate(groups):
        for c in range(g["ksteps"] // 2):
            for ij in range(g["nshift"]):
                out.append((i, c, ij, g["wcol0"] + ij * g["wstride"] + 2 * c * KBK))
    return out


def classify_cut(steps, k):
    """What lies on both sides of a cut in front of step k of a walk (0 < k < len(steps))."""
    a, b = steps[k - 1], steps[k]
    if a[0] != b[0]:
        return "group_boundary"
    return "between_offsets" if a[1] == b[1] else "between_chunks"


# ---- which kernel a launch runs (kernels.hip: launch_prec / launch_one under the default policy) ------------------------------------
def _sk_lds(prec, mf):
    return (3 * (prec_x_planes(prec) * (64 * mf + 16) * KBK * 2 + prec_w_planes(prec) * KBM * KBK * 2) + 1536 + 2 * 1536 +
            (3 * (64 * mf + 16) * 4 if prec_mx2(prec) else 0))


def sk_applicable(prec, mf, m_tiles, n_tiles, cus):
    if _sk_lds(prec, mf) > 160 * 1024:
        return False
    rows = m_tiles * KBM
    if rows % (64 * mf):
        return False
    grid = cus // 8 * 8
    if grid < 8:
        return False
    if (rows // (64 * mf) // 8) * n_tiles >= grid // 8:
        return True
    return mf == 8 and rows // (64 * mf) // 8 >= 4 and (m_tiles // 2) * n_tiles > cus


def sk_regime(prec, mf, m_tiles, n_tiles, cus):
    """1: every workgroup gets at least a tile's worth of steps; 2: the rule for launches between the regimes; 0: not applicable"""
    if not sk_applicable(prec, mf, m_tiles, n_tiles, cus):
        return 0
    return 1 if (m_tiles * KBM // (64 * mf) // 8) * n_tiles >= cus // 8 * 8 // 8 else 2


def p8_applicable(prec, m_tiles, n_tiles, segs, ksplit=0):
    if prec == PREC_FP16MXE:
        prec = PREC_FP16MX
    if prec not in (PREC_FP16, PREC_FP16MX, PREC_FP16MX2):
        return False
    if (m_tiles & 1) or (n_tiles & 1) or ksplit > 1:
        return False
    mx, mx2 = prec != PREC_FP16, prec == PREC_FP16MX2
    t = 0
    for g, s in ((g, segs[g["first_seg"]]) for g in seg_groups(segs)):
        if g["ksteps"] % (8 if mx2 else 4 if mx else 2) or s[1] % (256 if mx2 else 64):
            return False
        t += (g["ksteps"] >> 1) * g["nshift"]
    return t >= 2 and not (t & 1)


def mx_applicable(prec, m_tiles, segs):
    total = sum(s[3] // KBK for s in segs)
    if (m_tiles & 1) or (total & 3):
        return False
    for g, s in ((g, segs[g["first_seg"]]) for g in seg_groups(segs)):
        if (g["ksteps"] * g["nshift"]) % 4:
            return False
        if prec_mx2(prec) and (g["ksteps"] % 4 or s[1] % 128):
            return False
    return True


def select_kernel(prec, epi, m_tiles, n_tiles, segs, cus, p8=0, ksplit=0):
    """Name of the kernel xv_kernel_tdnn_gemm launches, as last_gemm_kernel() spells it; None when the launch is refused."""
    P, E = PREC_NAME[prec], EPI_NAME[epi]
    if prec in (PREC_FP16X3E, PREC_FP16MXE) and (ksplit > 1 or epi != EPI_ACT):
        return None
    if prec_mx(prec) and (ksplit > 1 or epi == EPI_F32):
        return None
    if ksplit > 1:
        if prec > PREC_FP16X3 or p8 or epi not in (EPI_ACT, EPI_F32):
            return None
        return "tdnn_gemm_kernel<%s,splitk>" % P
    if p8:
        ok = (prec in (PREC_FP16, PREC_FP16MX, PREC_FP16MX2) and epi in (EPI_ACT, EPI_STATS)) or (prec == PREC_FP16MXE and epi == EPI_ACT)
        return "tdnn_gemm_kernel_p8<%s,%s>" % (P, E) if ok and p8_applicable(prec, m_tiles, n_tiles, segs) else None
    total = sum(s[3] // KBK for s in segs)
    if prec_mx(prec):
        if not mx_applicable(prec, m_tiles, segs):
            return None
        if sk_applicable(prec, 8, m_tiles, n_tiles, cus):
            return "tdnn_gemm_kernel_sk<%s,%s,8>" % (P, E)
        return "tdnn_gemm_kernel_v2<%s,%s>" % (P, E)
    if prec == PREC_FP16X2 or total >= 32:
        if sk_applicable(prec, 8, m_tiles, n_tiles, cus):
            return "tdnn_gemm_kernel_sk<%s,%s,8>" % (P, E)
        if prec_x_planes(prec) == 2 and sk_applicable(prec, 4, m_tiles, n_tiles, cus):
            return "tdnn_gemm_kernel_sk<%s,%s,4>" % (P, E)
    if (m_tiles & 1) == 0:
        return "tdnn_gemm_kernel_v2<%s,%s>" % (P, E)
    return "tdnn_gemm_kernel<%s,%s>" % (P, E)


# ---- the stream-K and p8 partitions -------------------------------------------------------------------------------------------------
def _lanes(n_col_tiles, per_xcd, start=4):
    l = start
    while l > 1 and (n_col_tiles % l or per_xcd % l):
        l >>= 1
    return l


def _deal(sk_mtiles, cpl, lanes, ng, S, cut):
    """Per workgroup (xcd, group, lane): its parts as (kind, row tile, column tile, first step, end step), in the order it runs
    them: tail part (the first steps of a tile it shares with the next workgroup), whole tiles, head part (the last steps of
    the tile the previous workgroup began)."""
    out = []
    for xcd in range(8):
        tb0, tb1 = sk_mtiles * xcd // 8, sk_mtiles * (xcd + 1) // 8
        allsteps = (tb1 - tb0) * cpl * S
        for g in range(ng):
            s0, s1 = cut(allsteps, g), cut(allsteps, g + 1)
            if s1 <= s0:
                continue
            k_head, k_tail = s0 % S, s1 % S
            t_first, t_end = (s0 + S - 1) // S, s1 // S
            for lane in range(lanes):
                where = lambda tile: (tb0 + tile // cpl, lane * cpl + tile % cpl)
                parts = []
                if k_tail:
                    parts.append(("tail",) + where(t_end) + (0, k_tail))
                parts += [("whole",) + where(t) + (0, S) for t in range(t_first, t_end)]
                if k_head:
                    parts.append(("head",) + where(t_first - 1) + (k_head, S))
                out.append(dict(xcd=xcd, group=g, lane=lane, parts=parts))
    return out


def sk_partition(prec, mf, m_tiles, n_tiles, segs, cus):
    """tdnn_gemm_kernel_sk<prec, ., mf> on a device of `cus` CUs: (workgroups, column lanes, parts per workgroup).  Steps are
    those of the whole walk (kPrecFp16Mx2: the S first-walk steps followed by S / 4 steps of the second walk)."""
    grid = cus // 8 * 8
    sk_mtiles = m_tiles * KBM // (64 * mf)
    lanes = _lanes(n_tiles, grid // 8)
    tiles_min = max(1, (sk_mtiles // 8) * (n_tiles // lanes))
    ng = min(grid // 8 // lanes, tiles_min)
    SH = sum(s[3] // KBK for s in segs)
    S = SH + (SH // 4 if prec_mx2(prec) else 0)
    kq = 4 if prec_mx(prec) else 1
    cpl = n_tiles // lanes
    if prec_mx2(prec):
        def cut(allsteps, g):
            s = allsteps * g // ng
            k = s % S
            if k < SH:
                k &= ~3
            return s - s % S + k
    else:
        def cut(allsteps, g):
            return (allsteps // kq) * g // ng * kq
    return 8 * lanes * ng, lanes, _deal(sk_mtiles, cpl, lanes, ng, S, cut)


def p8_partition(prec, m_tiles, n_tiles, segs, cus, whole=False):
    """tdnn_gemm_kernel_p8: steps are K tiles of 64 columns (kPrecFp16Mx2: followed by the tiles of 256 4-bit columns)."""
    groups = seg_groups(segs)
    S = sum((g["ksteps"] >> 1) * g["nshift"] for g in groups)
    S_lo = sum((g["ksteps"] // 4 >> 1) * g["nshift"] for g in groups) if prec_mx2(prec) else 0
    ST = S + S_lo
    sk_mtiles, nt = m_tiles >> 1, n_tiles >> 1
    grid = cus // 8 * 8
    lanes = _lanes(nt, grid // 8)
    if nt % 3 == 0 and nt <= 6 and grid // 8 >= nt:
        lanes = nt
    tiles_min = max(1, (sk_mtiles // 8) * (nt // lanes))
    ng = min(grid // 8 // lanes, tiles_min)

    def cut(allsteps, g):
        s = allsteps * g // ng
        if whole:
            return (s + ST // 2) // ST * ST
        k = s % ST
        if k < S:
            k &= ~1
        return s - s % ST + k
    return 8 * lanes * ng, lanes, _deal(sk_mtiles, nt // lanes, lanes, ng, ST, cut)


def cut_classes(partition, steps, S):
    """Summary of a partition: lengths of its head and tail parts, and what each cut position separates (steps: the walk)."""
    heads, tails, kinds, pos = set(), set(), set(), set()
    for wg in partition:
        for kind, _, _, kb, ke in wg["parts"]:
            if kind == "head":
                heads.add(ke - kb)
                pos.add(kb)
            elif kind == "tail":
                tails.add(ke - kb)
                pos.add(ke)
    for k in pos:
        if k < len(steps):
            kinds.add(classify_cut(steps, k))
    return dict(heads=heads, tails=tails, kinds=kinds, positions=pos, S=S)


def covers_every_tile_once(partition, m_tiles_k, n_tiles_k, S):
    """every (row tile, column tile) of the launch is covered by parts whose step ranges tile [0, S) exactly"""
    cov = {}
    for wg in partition:
        for _, mt, nt, kb, ke in wg["parts"]:
            cov.setdefault((mt, nt), []).append((kb, ke))
    if set(cov) != {(m, n) for m in range(m_tiles_k) for n in range(n_tiles_k)}:
        return False
    for r in cov.values():
        r.sort()
        if r[0][0] != 0 or r[-1][1] != S or any(r[i][1] != r[i + 1][0] for i in range(len(r) - 1)):
            return False
    return True


# ---- cases --------------------------------------------------------------------------------------------------------------------------
class Case(object):
    """One launch.  segs: [(source, ld, row_shift, k_len)]; q: the unit is 2^-q; amp_x / amp_w: hi planes hold integers in
    [-amp, amp]; lo_amp: lo planes hold m * 2^-q with |m| <= lo_amp; dens: fraction of non-zero hi entries; bn_exp: the
    BatchNorm scale of column n is 2^bn_exp[n % len(bn_exp)]."""

    def __init__(self, name, prec, epi, rows, n_pad, segs, relu=True, bn=True, m_valid=None, ksplit=0, p8=0, q=4, amp_x=3, amp_w=3,
                 lo_amp=7, dens=0.75, bn_exp=(-1, 0, 1), seed=0, gmax=False, kernel=None, expect=None):
        self.name, self.prec, self.epi, self.rows, self.n_pad, self.segs = name, prec, epi, rows, n_pad, list(segs)
        self.relu, self.bn, self.ksplit, self.p8 = relu, bn, ksplit, p8
        self.m_valid = rows if m_valid is None else m_valid
        self.q, self.amp_x, self.amp_w, self.lo_amp, self.dens, self.bn_exp, self.seed = q, amp_x, amp_w, lo_amp, dens, bn_exp, seed
        self.gmax = gmax and epi == EPI_ACT
        self.kernel = kernel              # the kernel the case is about (asserted against select_kernel and against the device)
        self.expect = expect or {}        # cut classes the case claims: heads / tails (sets of lengths), kinds, lanes, regime
        self.K = sum(s[3] for s in self.segs)
        # weight columns K .. ldw hold NaN (the block-scaled modes keep ldw = K: their 4-bit planes are laid out by K)
        self.ldw = self.K if prec_mx(prec) else self.K + 32
        self.ldo = n_pad + 64             # gaps behind the n_pad columns of every output hold the sentinel
        self.ldf = n_pad + 4
        self.ldp = n_pad + 3
        self.src_ld = {}
        self.src_k = {}
        for s in self.segs:
            self.src_ld[s[0]] = max(self.src_ld.get(s[0], 0), s[1])
            self.src_k[s[0]] = max(self.src_k.get(s[0], 0), s[3])

    @property
    def m_tiles(self):
        return self.rows // KBM

    @property
    def n_tiles(self):
        return self.n_pad // KBN

    @property
    def ksteps(self):
        return self.K // KBK

    def __repr__(self):
        return self.name


def make_operands(c):
    """Planes as the kernel takes them (uint16 bit patterns, halo rows included) and their values (float64)."""
    rng = np.random.default_rng(1000 + c.seed)
    f16 = prec_f16(c.prec)
    u = 2.0 ** -c.q
    xs = prec_x_planes(c.prec) == 2
    ws = prec_w_planes(c.prec) == 2

    def ints(shape, amp, dens):
        v = rng.integers(-amp, amp + 1, shape).astype(np.float64)
        return v * (rng.random(shape) < dens)

    def lo_plane(shape):
        m = rng.integers(-c.lo_amp, c.lo_amp + 1, shape).astype(np.float64) * (rng.random(shape) < c.dens)
        m[..., 0] = np.where(m[..., 0] == 0, 3.0, m[..., 0])   # column 0: both lo planes non-zero at the same k (a lo * lo term would show)
        return m * u

    ops = dict(X=[], Xv=[])
    for i in sorted(c.src_ld):
        ld, k = c.src_ld[i], c.src_k[i]
        n = c.rows + 2 * HALO
        hi = ints((n, ld), c.amp_x, c.dens)
        halo = np.r_[0:HALO, HALO + c.rows:n]
        hi[halo] = np.where(hi[halo] == 0, 1.0, hi[halo])       # halo rows are read: non-zero integers
        lo = lo_plane((n, ld)) if xs else None
        hb = rne16(hi, f16)
        lb = rne16(lo, f16) if xs else None
        assert np.array_equal(val16(hb, f16), hi) and (lb is None or np.array_equal(val16(lb, f16), lo))
        if xs and f16:   # fp16 normal numbers or zero
            assert np.all((lo == 0) | (np.abs(lo) >= 2.0 ** -14))
        hb[:, k:] = nan16(f16)                                  # columns no segment may read
        if xs:
            lb[:, k:] = nan16(f16)
        ops["X"].append((hb, lb))
        ops["Xv"].append((hi, lo))
    wh = ints((c.n_pad, c.K), c.amp_w, c.dens)
    wl = lo_plane((c.n_pad, c.K)) if ws else None
    whb = np.full((c.n_pad, c.ldw), nan16(f16), dtype=np.uint16)
    whb[:, :c.K] = rne16(wh, f16)
    wlb = None
    if ws:
        wlb = np.full((c.n_pad, c.ldw), nan16(f16), dtype=np.uint16)
        wlb[:, :c.K] = rne16(wl, f16)
        assert np.array_equal(val16(wlb[:, :c.K], f16), wl)
    assert np.array_equal(val16(whb[:, :c.K], f16), wh)
    ops["W"], ops["Wv"] = (whb, wlb), (wh, wl)
    ops["bias"] = (rng.integers(-8, 9, c.n_pad) * u).astype(np.float32)
    e = np.array([c.bn_exp[n % len(c.bn_exp)] for n in range(c.n_pad)])
    ops["scale"] = (2.0 ** e).astype(np.float32)
    ops["offset"] = (rng.integers(-8, 9, c.n_pad) * u).astype(np.float32)
    ngrp = c.rows // 16
    first = rng.integers(0, 10, ngrp).astype(np.int8)
    last = np.minimum(16, first + rng.integers(0, 17, ngrp)).astype(np.int8)
    first[0], last[0] = 0, 16                                   # everything counts
    if ngrp > 1:
        first[1], last[1] = 5, 5                                # nothing does
    ops["range"] = np.ascontiguousarray(np.stack([first, last], 1))
    return ops


def _products(c, Xv, Wv, fn):
    """sum over the segments of the products the precision defines (kernels.h): three-pass hi . hi + hi . lo + lo . hi, fp16x2
    x . w_hi + x . w_lo, single-pass one product.  hi . hi + hi . lo is formed as hi . (w_hi + w_lo): the sum of the two weight
    planes is exact in fp64, so it is the same number for one matrix product less."""
    wh, wl = Wv
    acc, k0 = 0.0, 0
    for (si, ld, shift, klen) in c.segs:
        xh, xl = Xv[si]
        r = slice(HALO + shift, HALO + shift + c.rows)
        w1 = wh[:, k0:k0 + klen]
        acc = acc + fn(xh[r, :klen], w1 + wl[:, k0:k0 + klen] if prec_w_planes(c.prec) == 2 else w1)
        if prec_x_planes(c.prec) == 2:
            acc = acc + fn(xl[r, :klen], w1)                                        # lo . hi
        k0 += klen
    return acc


def exact_fp32(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.all((a.astype(np.float32).astype(np.float64) == a) | np.isnan(a)))


def reference_z(c, ops, Xv=None):
    """fp64: the products each precision defines, bias, ReLU (a NaN stays a NaN), the BatchNorm fma - every intermediate an
    exact fp32 number (asserted)."""
    acc = _products(c, ops["Xv"] if Xv is None else Xv, ops["Wv"], lambda x, w: x @ w.T)
    z = acc + ops["bias"].astype(np.float64)
    assert exact_fp32(acc) and exact_fp32(z)
    if c.relu:
        with np.errstate(invalid="ignore"):
            z = np.where(z < 0, 0.0, z)
    if c.bn:
        z = z * ops["scale"].astype(np.float64) + ops["offset"].astype(np.float64)
        assert exact_fp32(z)
    return z


def check_precondition(c, ops, budget=BIT_BUDGET):
    """sum |terms| * 2^q < 2^budget for every output element: the products, the bias, the BatchNorm fma (whose unit is
    2^-(q - min(0, exponent of the scale))), the values the planes epilogue rounds, and both statistics sums.  Returns the
    largest of the bounds in bits."""
    u = 2.0 ** c.q
    Xa = [(np.abs(h), None if l is None else np.abs(l)) for h, l in ops["Xv"]]
    Wa = (np.abs(ops["Wv"][0]), None if ops["Wv"][1] is None else np.abs(ops["Wv"][1]))
    a = _products(c, Xa, Wa, lambda x, w: x @ w.T) + np.abs(ops["bias"].astype(np.float64))
    worst = float(a.max() * u)
    if c.bn:
        e = np.log2(ops["scale"].astype(np.float64))
        assert np.all(e == np.round(e)), "BatchNorm scales are powers of two"
        u = u * 2.0 ** max(0.0, -float(e.min()))
        a = a * ops["scale"].astype(np.float64) + np.abs(ops["offset"].astype(np.float64))
        worst = max(worst, float(a.max() * u))
    if prec_f16(c.prec) and c.epi == EPI_ACT:
        assert a.max() < 60000.0, "the fp16 output plane must not overflow"
    if c.epi == EPI_STATS:
        g = a.reshape(c.rows // 16, 16, c.n_pad)
        worst = max(worst, float(g.sum(axis=1).max() * u), float((g * g).sum(axis=1).max() * u * u))
    bits = np.log2(max(worst, 1.0))
    assert worst < 2.0 ** budget, "%s: sum |terms| needs %.2f bits, budget %d" % (c.name, bits, budget)
    return bits


def reference(c, ops, z=None):
    """What the launch must leave in its output buffers, bit for bit (buffers start out filled with the sentinels)."""
    f16 = prec_f16(c.prec)
    z = reference_z(c, ops) if z is None else z
    out = {}
    if c.epi == EPI_F32:
        o = np.full((c.rows, c.ldf), SENT_F32, dtype=np.float32)
        o[:c.m_valid, :c.n_pad] = z[:c.m_valid].astype(np.float32)
        out["f32"] = o
    elif c.epi == EPI_ACT:
        hi = rne16(z, f16)
        o = np.full((c.rows, c.ldo), SENT16, dtype=np.uint16)
        o[:, :c.n_pad] = hi
        out["hi"] = o
        if prec_emits_lo4(c.prec):
            packed, e8, _ = _lo4_plane(z.astype(np.float32), val16(hi, f16))
            o4 = np.full((c.rows, c.ldo // 2), SENT8, dtype=np.uint8)
            o4[:, :c.n_pad // 2] = packed
            o4s = np.full((c.rows, lo4_scale_pitch(c.ldo)), SENT8, dtype=np.uint8)
            o4s[:, :c.n_pad // 64] = e8[:, :c.n_pad // 64]
            out["lo4"], out["lo4s"] = o4, o4s
        elif prec_x_planes(c.prec) == 2:
            res = z - val16(hi, f16)
            assert exact_fp32(res)
            o = np.full((c.rows, c.ldo), SENT16, dtype=np.uint16)
            o[:, :c.n_pad] = rne16(res, f16)
            out["lo"] = o
        if c.gmax:
            rt = ops["range"].astype(np.int64)
            r16 = np.arange(16)[None, :]
            counted = (r16 >= rt[:, :1]) & (r16 < rt[:, 1:])
            m = (np.abs(z).reshape(c.rows // 16, 16, c.n_pad) * counted[:, :, None]).max(axis=(1, 2))
            out["gmax"] = m.astype(np.float32).view(np.uint32)
    else:
        rt = ops["range"].astype(np.int64)
        r16 = np.arange(16)[None, :]
        mask = ((r16 >= rt[:, :1]) & (r16 < rt[:, 1:]))[:, :, None]
        zz = z.reshape(c.rows // 16, 16, c.n_pad)
        s1, s2 = np.where(mask, zz, 0.0).sum(axis=1), np.where(mask, zz * zz, 0.0).sum(axis=1)
        assert exact_fp32(s1) and exact_fp32(s2) and exact_fp32(zz * zz)
        o = np.full((c.rows // 16, 2, c.ldp), SENT_F32, dtype=np.float32)
        o[:, 0, :c.n_pad], o[:, 1, :c.n_pad] = s1, s2
        out["partial"] = o
    return out


def reference_loops(c, ops):
    """The same z by a triple loop in Python floats (tiny cases only): what reference_z is checked against."""
    wh, wl = ops["Wv"]
    z = np.zeros((c.rows, c.n_pad))
    for r in range(c.rows):
        for n in range(c.n_pad):
            s, k0 = 0.0, 0
            for (si, ld, shift, klen) in c.segs:
                xh, xl = ops["Xv"][si]
                for k in range(klen):
                    s += xh[HALO + r + shift, k] * wh[n, k0 + k]
                    if prec_w_planes(c.prec) == 2:
                        s += xh[HALO + r + shift, k] * wl[n, k0 + k]
                    if prec_x_planes(c.prec) == 2:
                        s += xl[HALO + r + shift, k] * wh[n, k0 + k]
                k0 += klen
            s += float(ops["bias"][n])
            if c.relu and s < 0:
                s = 0.0
            if c.bn:
                s = s * float(ops["scale"][n]) + float(ops["offset"][n])
            z[r, n] = s
    return z


# ---- the case list --------------------------------------------------------------------------------------------------------------------
def kname(variant, prec, epi, mf=0):
    if mf:
        return "tdnn_gemm_kernel%s<%s,%s,%d>" % (variant, PREC_NAME[prec], EPI_NAME[epi], mf)
    return "tdnn_gemm_kernel%s<%s,%s>" % (variant, PREC_NAME[prec], EPI_NAME[epi])


SEGS_SMALL = [(0, 64, -3, 32), (0, 64, 0, 32), (0, 64, 3, 32), (1, 96, 1, 64)]   # a group of three offsets + a second source, k_len < ld
PRECS = (0, 1, 2, 3, 4, 8)


def _epis(prec):
    return (0,) if prec == PREC_FP16X3E else (0, 1, 2)


def _tune(prec, epi, ksteps):
    """Value ranges and sparsity by case: the statistics sums square the outputs, long K sums more terms."""
    # q = 8: the results carry 12 to 16 significant bits, more than either 16-bit format holds, so the planes epilogue rounds
    # nearly every value (and meets ties); lo planes use up to seven significant bits
    kw = dict(q=8, amp_x=3, amp_w=3, lo_amp=100, dens=0.75)
    if epi == EPI_STATS:
        kw.update(q=2, amp_x=2, amp_w=2, lo_amp=3, dens=0.35, bn_exp=(-1, 0))
    if ksteps >= 16:
        kw.update(dens=min(kw["dens"], 0.5))
    if ksteps >= 16 and epi == EPI_STATS:
        kw.update(dens=0.12, amp_x=1, amp_w=2)
    return kw


def per_tile_cases(prec, epi):
    """tdnn_gemm_kernel (128-row tiles): odd tile counts 1, 3, 9 x column tiles 1, 3; the fp32 epilogue at every m_valid edge."""
    out = []
    for mt in (1, 3, 9):
        for nt in (1, 3):
            rows = mt * KBM
            for mv in ((0, 1, rows - 1, rows) if epi == EPI_F32 else (rows,)):
                out.append(Case("tile_p%d_e%d_m%d_n%d_v%d" % (prec, epi, mt, nt, mv), prec, epi, rows, nt * KBN, SEGS_SMALL,
                                m_valid=mv, seed=mt * 7 + nt, gmax=True, kernel=kname("", prec, epi), **_tune(prec, epi, 5)))
    return out


def v2_cases(prec, epi):
    """tdnn_gemm_kernel_v2 (256-row tiles): 2 row tiles of 128, and 22 = 11 tiles of 256, not a multiple of 8."""
    out = []
    for mt, nt in ((2, 1), (2, 3), (22, 1), (22, 3)):
        rows = mt * KBM
        for mv in ((0, 1, rows - 1, rows) if (epi == EPI_F32 and nt == 1) else (rows,)):
            out.append(Case("v2_p%d_e%d_m%d_n%d_v%d" % (prec, epi, mt, nt, mv), prec, epi, rows, nt * KBN, SEGS_SMALL,
                            m_valid=mv, seed=100 + mt + nt, gmax=True, kernel=kname("_v2", prec, epi), **_tune(prec, epi, 5)))
    return out


# the walk-planning cases: (name, segs, groups PlanWalkGroups must form as (first segment, offsets))
WALKS = [
    ("one_group", [(0, 64, -3, 32), (0, 64, 0, 32), (0, 64, 3, 32)], [(0, 3)]),
    ("non_uniform", [(0, 64, -3, 32), (0, 64, 0, 32), (0, 64, 1, 32)], [(0, 2), (2, 1)]),
    ("decreasing", [(0, 64, 3, 32), (0, 64, 0, 32), (0, 64, -3, 32)], [(0, 1), (1, 1), (2, 1)]),
    ("span16", [(0, 64, -8, 64), (0, 64, 8, 64)], [(0, 2)]),
    ("span17", [(0, 64, -8, 64), (0, 64, 9, 64)], [(0, 1), (1, 1)]),
    ("pm15", [(0, 32, -15, 32), (0, 32, 15, 32)], [(0, 1), (1, 1)]),
    ("repeated", [(0, 64, 2, 64), (0, 64, 2, 64)], [(0, 1), (1, 1)]),
    ("two_ld", [(0, 64, -1, 64), (1, 96, 1, 96)], [(0, 1), (1, 1)]),
    ("klen_lt_ld", [(0, 96, -2, 64), (0, 96, 2, 64)], [(0, 2)]),
    ("eight", [(0, 32, o, 32) for o in (-7, -5, -3, -1, 1, 3, 5, 7)], [(0, 8)]),
    ("eight_mixed", [(0, 32, -4, 32), (0, 32, 0, 32), (1, 64, 0, 32), (0, 32, 4, 32), (1, 64, -2, 32), (1, 64, 2, 32), (1, 64, 6, 32),
                     (0, 32, 15, 32)], [(0, 2), (2, 1), (3, 1), (4, 3), (7, 1)]),
]


def walk_cases(walk):
    """every walk on the per-tile kernel (which walks segment by segment) and on the 256-row kernel (which stages a group's rows
    once per chunk), three-pass fp16 into fp32 and two-pass fp16 into planes"""
    name, segs, _ = next(w for w in WALKS if w[0] == walk)
    out = []
    for mt, variant in ((1, ""), (2, "_v2")):
        for prec, epi in ((3, 1), (4, 0)):
            out.append(Case("walk_%s_m%d_p%d" % (name, mt, prec), prec, epi, mt * KBM, KBN, segs, seed=200 + mt,
                            kernel=kname(variant, prec, epi), **_tune(prec, epi, len(segs) * 2)))
    return out


SPLITK_STEPS = (8, 9, 12, 16, 20, 24, 28, 32, 36, 40, 44, 47, 48)   # 2 .. 12 slices: every count the rule yields for 8 .. 48 steps


def splitk_cases(steps):
    out = []
    a = steps // 3 * KBK
    segs = [(0, max(a, 32), -1, a), (1, steps * KBK - a, 2, steps * KBK - a)] if a else [(0, steps * KBK, 1, steps * KBK)]
    for prec, epi in ((0, 0), (3, 1), (1, 1), (2, 0)):
        out.append(Case("splitk_s%d_p%d_e%d" % (steps, prec, epi), prec, epi, KBM, 2 * KBN, segs, ksplit=splitk_slices(steps),
                        m_valid=77 if epi == EPI_F32 else None, seed=300 + steps, kernel="tdnn_gemm_kernel<%s,splitk>" % PREC_NAME[prec],
                        **_tune(prec, epi, steps)))
    return out


# Stream-K.  Eight K steps: a group of three offsets (steps 0 1 2: chunk 0 at offsets -3 0 3), a second source of two chunks (3 4),
# another group (5 6 7).  With 9 column tiles per lane and 8 workgroup groups per XCD block the cuts fall at 9 g S / 8: one at every
# step 1 .. 7 - heads and tails of every length from 1 to S - 1, cuts between offsets (1, 2, 6, 7), on group boundaries (3, 5) and
# between the chunks of a source (4).
SEGS_SK8 = [(0, 32, -3, 32), (0, 32, 0, 32), (0, 32, 3, 32), (1, 64, 1, 64), (0, 32, -2, 32), (0, 32, 2, 32), (0, 32, 6, 32)]
SEGS_SK32 = [(0, 256, -3, 256), (0, 256, 0, 256), (0, 256, 3, 256), (1, 256, 1, 256)]    # 32 steps: what the other modes need for stream-K


def sk_min_m_tiles(prec, mf, n_tiles, cus, regime):
    """smallest number of 128-row tiles that sk_applicable admits in the given regime"""
    step = 64 * mf // KBM
    for mt in range(step, 4096, step):
        if sk_regime(prec, mf, mt, n_tiles, cus) == regime:
            return mt
    raise AssertionError("no row count reaches regime %d" % regime)


SK_NAMES = ["lanes4_act", "lanes4_f32", "lanes4_stats", "lanes2_act", "lanes1_f32", "regime2_act", "regime2_stats", "sk4_fp16x3_f32",
            "sk4_bf16x3_act", "sk4_fp16x3e_act", "sk8_fp16_act", "sk8_bf16_stats"]


def sk_case(name, cus=256):
    """Stream-K cases by name; the shapes follow the CU count (column tiles per lane = workgroup groups per XCD block + 1)."""
    g8 = cus // 8 * 8 // 8
    every = set(range(1, 8))
    kinds = {"group_boundary", "between_offsets", "between_chunks"}

    def mk(prec, epi, mf, n_tiles, regime, segs, expect, extra=0, **kw):
        mt = sk_min_m_tiles(prec, mf, n_tiles, cus, regime) + extra    # extra 128-row tiles: a tile count the groups do not divide
        t = _tune(prec, epi, sum(s[3] for s in segs) // KBK)
        t.update(kw)
        return Case("sk_" + name, prec, epi, mt * KBM, n_tiles * KBN, segs, seed=400 + len(name), gmax=True,
                    kernel=kname("_sk", prec, epi, mf), expect=dict(expect, regime=regime, mf=mf), **t)
    if name.startswith("lanes4"):
        epi = {"act": 0, "f32": 1, "stats": 2}[name.split("_")[1]]
        nt = 4 * (g8 // 4 + 1)     # lanes 4, g8 / 4 groups, g8 / 4 + 1 column tiles per lane
        return mk(4, epi, 8, nt, 1, SEGS_SK8, dict(lanes=4, heads=every, tails=every, kinds=kinds))
    if name == "lanes2_act":
        # one column tile per lane: one more 512-row tile per XCD block than the block has groups
        return mk(4, 0, 8, 2, 1, SEGS_SK8, dict(lanes=2, heads=every, tails=every, kinds=kinds), extra=32)
    if name == "lanes1_f32":
        c = mk(4, 1, 8, 1, 1, SEGS_SK8, dict(lanes=1, heads=every, tails=every, kinds=kinds), extra=32)
        c.m_valid = c.rows - 1          # the m_valid guard of the stream-K epilogue
        return c
    if name.startswith("regime2"):
        epi = {"act": 0, "stats": 2}[name.split("_")[1]]
        # one 512-row tile more than a multiple of eight: the block that gets it has 25 tiles for 20 groups
        return mk(4, epi, 8, 5, 2, SEGS_SK8, dict(lanes=1, heads={2, 4, 6}, tails={2, 4, 6}), extra=4)
    if name.startswith("sk4"):
        prec, epi = {"fp16x3_f32": (3, 1), "bf16x3_act": (0, 0), "fp16x3e_act": (8, 0)}[name[4:]]
        nt = 4 * (g8 // 4 + 1)
        return mk(prec, epi, 4, nt, 1, SEGS_SK32, dict(lanes=4, heads={4, 28}, tails={4, 28}, kinds=kinds), dens=0.3, amp_x=2, amp_w=2)
    prec, epi = {"sk8_fp16_act": (2, 0), "sk8_bf16_stats": (1, 2)}[name]
    nt = 4 * (g8 // 4 + 1)
    return mk(prec, epi, 8, nt, 1, SEGS_SK32, dict(lanes=4, heads={4, 28}, tails={4, 28}, kinds=kinds))


# tdnn_gemm_kernel_p8 (fp16): K tiles of 64 columns, cuts at even tiles
SEGS_P8 = [(0, 128, -2, 128), (0, 128, 0, 128), (0, 128, 2, 128), (1, 64, 1, 64), (1, 64, 4, 64)]   # 6 + 2 = 8 K tiles
P8_NAMES = ["min_act", "min_stats", "rows3_act", "lanes3_act", "lanes6_stats", "dealt_act", "dealt_stats"]


def p8_case(name, cus=256):
    g8 = cus // 8 * 8 // 8
    epi = 0 if name.endswith("act") else 2
    t = _tune(PREC_FP16, epi, 16)
    kw = dict(seed=500 + len(name), gmax=True, p8=1, kernel=kname("_p8", PREC_FP16, epi))
    if name.startswith("min"):        # 2 x 2 tiles of 128: one tile of 256 x 256
        return Case("p8_" + name, 2, epi, 256, 256, SEGS_P8, expect=dict(lanes=1), **dict(kw, **t))
    if name.startswith("rows3"):      # three row tiles: five XCD blocks without tiles
        return Case("p8_" + name, 2, epi, 3 * 256, 512, SEGS_P8, expect=dict(lanes=2, empty_blocks=5), **dict(kw, **t))
    if name.startswith("lanes3"):
        return Case("p8_" + name, 2, epi, 2 * 256, 3 * 256, SEGS_P8, expect=dict(lanes=3), **dict(kw, **t))
    if name.startswith("lanes6"):
        return Case("p8_" + name, 2, epi, 2 * 256, 6 * 256, SEGS_P8, expect=dict(lanes=6), **dict(kw, **t))
    # dealt: four column tiles -> four lanes, g8 / 4 groups per XCD block, g8 / 4 + 1 row tiles per block: cuts at 9 g ST / 8 rounded
    # down to even tiles: in front of the first pair's successor (2), in the middle (4), in front of the last pair (ST - 2)
    rows = (g8 // 4 + 1) * 8 * 256
    return Case("p8_" + name, 2, epi, rows, 4 * 256, SEGS_P8, expect=dict(lanes=4, heads={2, 4, 6}, tails={2, 4, 6}), **dict(kw, **t))


def footprint_case(kernel, epi, cus=256):
    """the four kernels once each (p8 has no fp32 epilogue: planes only)"""
    if kernel == "tile":
        return Case("fp_tile_e%d" % epi, 3, epi, 3 * KBM, KBN, SEGS_SMALL, seed=600, kernel=kname("", 3, epi), **_tune(3, epi, 5))
    if kernel == "v2":
        return Case("fp_v2_e%d" % epi, 3, epi, 4 * KBM, KBN, SEGS_SMALL, seed=601, kernel=kname("_v2", 3, epi), **_tune(3, epi, 5))
    if kernel == "sk":
        c = sk_case("lanes4_act" if epi == 0 else "lanes4_f32", cus)
        c.name, c.gmax = "fp_sk_e%d" % epi, False
        return c
    c = p8_case("rows3_act", cus)
    c.name, c.gmax = "fp_p8_e0", False
    return c


def footprint_rows(c, src, r0, c0):
    """rows of the output that depend on element (r0, c0) of source plane src (r0 relative to logical row 0)"""
    rows = set()
    for (si, ld, shift, klen) in c.segs:
        if si == src and c0 < klen and 0 <= r0 - shift < c.rows:
            rows.add(r0 - shift)
    return sorted(rows)


def check_sk_claims(c, cus):
    """the case selects the kernel it names and its partition has the cut classes it claims (shared with the GPU tests)"""
    mf = c.expect["mf"]
    assert select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, cus) == c.kernel, c
    assert sk_regime(c.prec, mf, c.m_tiles, c.n_tiles, cus) == c.expect["regime"]
    if c.expect["regime"] == 1 and c.name.startswith("sk_lanes4"):   # the smallest row count the rule admits
        assert not sk_applicable(c.prec, mf, c.m_tiles - 64 * mf // KBM, c.n_tiles, cus)
    grid, lanes, part = sk_partition(c.prec, mf, c.m_tiles, c.n_tiles, c.segs, cus)
    steps = walk_steps(seg_groups(c.segs))
    assert covers_every_tile_once(part, c.rows // (64 * mf), c.n_tiles, len(steps))
    cc = cut_classes(part, steps, len(steps))
    assert lanes == c.expect["lanes"], (lanes, c.expect)
    for key in ("heads", "tails", "kinds"):
        assert c.expect.get(key, set()) <= cc[key], (c, key, cc[key])
    return grid, lanes, cc


def check_p8_claims(c, cus):
    assert select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, cus, p8=1) == c.kernel, c
    grid, lanes, part = p8_partition(c.prec, c.m_tiles, c.n_tiles, c.segs, cus)
    tiles = walk_tiles64(seg_groups(c.segs))
    assert covers_every_tile_once(part, c.m_tiles // 2, c.n_tiles // 2, len(tiles))
    cc = cut_classes(part, tiles, len(tiles))
    assert lanes == c.expect["lanes"], (lanes, c.expect)
    assert all(p % 2 == 0 for p in cc["positions"])          # a pair of K tiles is never cut
    for key in ("heads", "tails"):
        assert c.expect.get(key, set()) <= cc[key], (c, key, cc[key])
    if "empty_blocks" in c.expect:
        assert 8 - len({w["xcd"] for w in part}) == c.expect["empty_blocks"]
    return grid, lanes, cc


# ---- the block-scaled modes (fp16mx, fp16mx2, fp16mxe): operands every quantiser returns unchanged ---------------------------------------
# Activations: e2m1 grid values times 2^(E - 2), E the exponent of their 16-row group's maximum (what the consumer derives its
# scale from); E alternates between 0 and 1 from group to group and every group holds a 4 * 2^(E - 2) that fixes it.  Rows that a
# time offset pairs with a neighbouring group's scale (the first and last MX_EDGE rows of a group, the halo) hold only 0, +-1, +-2
# times their scale, which stay on the grid under a scale one binade away.  fp16mx2: x = fp16(x) + residual, the residual a grid
# value times 2^(Eb - 13), Eb the exponent of the row's 64-column block maximum, only on elements large enough that fp16(x) drops
# exactly it.  Weights: w_hi in 0 .. +-3 (on the grid under every scale the 4-bit weight image can choose, so the image of
# w = w_hi + residual is w_hi), residual m * 2^-14, m in +-{1, 2, 3, 4, 6}, pointing away from zero (fp16(w) = w_hi).  The common
# unit of all products is 2^-17.
MX_EDGE = 4          # |row_shift| of the MX cases stays below this
MX_Q = 17


def make_mx_operands(c):
    rng = np.random.default_rng(2000 + c.seed)
    assert prec_mx(c.prec) and all(abs(s[2]) < MX_EDGE and s[1] == s[3] for s in c.segs)
    n = c.rows + 2 * HALO
    r16 = np.arange(n) % 16
    edge = (r16 < MX_EDGE) | (r16 >= 16 - MX_EDGE) | (np.arange(n) < HALO) | (np.arange(n) >= HALO + c.rows)
    E = np.array([0, 1, 1, 0])[(np.arange(n) // 16) % 4].astype(np.float64)
    ops = dict(Xh=[], X32=[], gmax=[], lo4=[])
    full = np.array([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    for i in sorted(c.src_ld):
        ld = c.src_ld[i]
        g = rng.choice(full, (n, ld)) * rng.choice([-1.0, 1.0], (n, ld)) * (rng.random((n, ld)) < c.dens)
        ge = rng.choice([1.0, 2.0], (n, ld)) * rng.choice([-1.0, 1.0], (n, ld)) * (rng.random((n, ld)) < c.dens)
        g[edge] = ge[edge]
        g[r16 == 8, 0] = 4.0                                     # fixes the group's exponent (an interior row)
        xh = g * (2.0 ** (E - 2))[:, None]
        x = xh.copy()
        if prec_mx2(c.prec):
            blk = np.abs(xh).reshape(n, ld // 64, 64)
            m = blk.max(axis=2, keepdims=True)
            eb = np.floor(np.log2(np.maximum(m, 2.0 ** -20)))
            ok = (blk >= 2.0 ** (eb - 1)) & (blk > 0)
            rho = rng.choice([0.0, 0.5, 1.0], blk.shape) * 2.0 ** (eb - 13) * ok
            x = xh + np.sign(xh) * rho.reshape(n, ld)
        x32 = x.astype(np.float32)
        hb = x32.astype(np.float16)
        assert np.array_equal(x32.astype(np.float64), x) and np.array_equal(hb.astype(np.float64), xh)
        body = np.abs(xh[HALO:HALO + c.rows]).reshape(c.rows // 16, 16, ld).max(axis=(1, 2))
        ops["Xh"].append(hb.view(np.uint16))
        ops["X32"].append(x32)
        ops["gmax"].append(body.astype(np.float32).view(np.uint32))
        ops["lo4"].append(_lo4_plane(x32, xh) if prec_mx2(c.prec) else None)
    wh = rng.integers(-3, 4, (c.n_pad, c.K)).astype(np.float64) * (rng.random((c.n_pad, c.K)) < c.dens_w)
    mres = rng.choice([1.0, 2.0, 3.0, 4.0, 6.0], wh.shape) * (rng.random(wh.shape) < 0.5)
    w = wh + np.sign(wh) * mres * 2.0 ** -14
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w) and np.array_equal(w32.astype(np.float16).astype(np.float64), wh)
    ops["W32"], ops["Wh"], ops["Wv"] = w32, w32.astype(np.float16).view(np.uint16), wh
    u = 2.0 ** -3
    ops["bias"] = (rng.integers(-8, 9, c.n_pad) * u).astype(np.float32)
    ops["scale"] = (2.0 ** np.array([c.bn_exp[k % len(c.bn_exp)] for k in range(c.n_pad)])).astype(np.float32)
    ops["offset"] = (rng.integers(-8, 9, c.n_pad) * u).astype(np.float32)
    ngrp = c.rows // 16
    first = rng.integers(0, 10, ngrp).astype(np.int8)
    last = np.minimum(16, first + rng.integers(0, 17, ngrp)).astype(np.int8)
    first[0], last[0] = 0, 16
    first[1], last[1] = 5, 5
    ops["range"] = np.ascontiguousarray(np.stack([first, last], 1))
    return ops


def mx_step_of_col(c):
    """K step (in the walk order of the kernel the case runs) of every weight column"""
    groups = seg_groups(c.segs)
    out = np.empty(c.K, dtype=np.int64)
    if c.p8:
        for t, (_, _, _, wcol) in enumerate(walk_tiles64(groups)):
            out[wcol:wcol + 32], out[wcol + 32:wcol + 64] = 2 * t, 2 * t + 1
    else:
        for s, (_, _, _, wcol) in enumerate(walk_steps(groups)):
            out[wcol:wcol + 32] = s
    return out


def mx_pack(c, ops, P):
    """the library's own packers: residual plane + scales, and for fp16mx2 the 4-bit weight image + scales"""
    segs3 = [(s[0], s[2], s[3]) for s in c.segs]
    pk = {}
    pk["w4"], pk["w4s"] = P.pack_mx_residual(ops["W32"], ops["Wh"], segs3, walk64=bool(c.p8))
    if prec_mx2(c.prec):
        pk["w4b"], pk["w4bs"] = P.pack_mx_weights(ops["W32"], segs3, walk64=bool(c.p8))
    return pk


def reference_z_mx(c, ops, pk):
    """x . w_hi + q4(x / sx) sx . q4((w - w_hi) / sw) sw [+ q4(x - fp16(x)) . q4(w)], bias, ReLU, BatchNorm - with the assertion
    that every quantiser returns these operands unchanged, so that the reference and the device cannot differ by a rounding choice"""
    wh = ops["Wv"]
    R_ = ops["W32"].astype(np.float64) - wh
    sidx = 4 * (mx_step_of_col(c) // 4) + (np.arange(c.K) % 32) // 8
    sw = 2.0 ** (pk["w4s"].astype(np.float64)[:, sidx] - 127)
    assert np.array_equal(_q_e2m1(R_ / sw) * sw, R_), "weight residuals are on the grid of the packer's scales"
    if prec_mx2(c.prec):
        assert np.array_equal(_w4_image(ops["W32"]), wh), "the 4-bit weight image is w_hi"
    acc = np.zeros((c.rows, c.n_pad))
    bound = np.zeros((c.rows, c.n_pad))
    k0 = 0
    for (si, ld, shift, klen) in c.segs:
        r = slice(HALO + shift, HALO + shift + c.rows)
        xs = val16(ops["Xh"][si], True)[r, :klen]
        eb = np.clip((ops["gmax"][si] >> 23) & 255, 16, 200).astype(np.float64).repeat(16)[:, None]
        sx = 2.0 ** (eb - 2 - 127)
        assert np.array_equal(_q_e2m1(xs / sx) * sx, xs), "activations are on the grid under the scale of every row they meet"
        wcols = (wh + R_)[:, k0:k0 + klen]
        acc += xs @ wcols.T
        bound += np.abs(xs) @ np.abs(wcols).T
        if prec_mx2(c.prec):
            dec = ops["lo4"][si][2]
            assert np.array_equal(dec, ops["X32"][si].astype(np.float64) - val16(ops["Xh"][si], True)), "residual plane is exact"
            acc += dec[r, :klen] @ wh[:, k0:k0 + klen].T
            bound += np.abs(dec[r, :klen]) @ np.abs(wh[:, k0:k0 + klen]).T
        k0 += klen
    # the precondition: sum |terms| * 2^q < 2^24, q = 17 (18 in the columns whose BatchNorm scale is 1/2)
    bound = (bound + np.abs(ops["bias"])) * ops["scale"].astype(np.float64) + np.abs(ops["offset"])
    qq = MX_Q + np.maximum(0.0, -np.log2(ops["scale"].astype(np.float64)))         # per column
    bits = np.log2((bound * 2.0 ** qq).max())
    assert bits < BIT_BUDGET, "%s: %.2f bits" % (c.name, bits)
    z = acc + ops["bias"].astype(np.float64)
    assert exact_fp32(acc) and exact_fp32(z)
    z = np.where(z < 0, 0.0, z) * ops["scale"].astype(np.float64) + ops["offset"].astype(np.float64)
    assert exact_fp32(z)
    return z


SEGS_MX = [(0, 128, -3, 128), (0, 128, 0, 128), (0, 128, 3, 128), (1, 128, 1, 128)]     # 16 steps; fp16mx2: + 4 of the second walk
SEGS_MX_P8 = [(0, 256, -2, 256), (0, 256, 2, 256)]                                      # 8 K tiles of 64; fp16mx2: + 2 of 256 4-bit columns
MX_NAMES = ["v2_fp16mx", "v2_fp16mx2", "v2_fp16mxe", "sk_fp16mx", "sk_fp16mx2", "p8_small_fp16mx", "p8_small_fp16mx2", "p8_small_fp16mxe",
            "p8_dealt_fp16mx", "p8_dealt_fp16mx2"]


_MX_SK_SHAPES = {}


def _mx_sk_shape(prec, cus):
    if (prec, cus) not in _MX_SK_SHAPES:
        SH = sum(s[3] for s in SEGS_MX) // KBK
        best = None
        for nt in range(1, 41):
            for mt in range(4, 161, 4):
                if (best is not None and mt * nt >= best[0]) or not sk_applicable(prec, 8, mt, nt, cus):
                    continue
                _, lanes, part = sk_partition(prec, 8, mt, nt, SEGS_MX, cus)
                pos = {p[3] for w in part for p in w["parts"] if p[0] == "head"}
                if (pos if prec != 7 else (any(p < SH for p in pos) and SH in pos and any(p > SH for p in pos))):
                    best = (mt * nt, mt, nt, lanes)
        assert best is not None, "no launch reaches the cut classes on %d CUs" % cus
        _MX_SK_SHAPES[(prec, cus)] = best[1:]
    return _MX_SK_SHAPES[(prec, cus)]


def mx_case(name, cus=256):
    """planes epilogue only: the statistics sums square values whose unit is 2^-17 and cannot be exact"""
    prec = {"fp16mx": 6, "fp16mx2": 7, "fp16mxe": 9}[name.split("_")[-1]]
    g8 = cus // 8 * 8 // 8
    kw = dict(relu=True, bn=True, bn_exp=(-1, 0), seed=700 + len(name) + prec, gmax=True, dens=0.1)

    def mk(rows, n_pad, segs, kernel, p8=0, expect=None):
        c = Case("mx_" + name, prec, EPI_ACT, rows, n_pad, segs, p8=p8, kernel=kernel, expect=expect or {}, **kw)
        c.dens_w = 0.2
        return c
    if name.startswith("v2"):
        return mk(6 * KBM, 2 * KBN, SEGS_MX, kname("_v2", prec, 0))
    if name.startswith("sk"):
        # the smallest launch whose cuts fall where the case claims: fp16mx - inside the walk, at multiples of four steps;
        # fp16mx2 - in the first walk, at the seam and in the second walk
        mt, nt, lanes = _mx_sk_shape(prec, cus)
        return mk(mt * KBM, nt * KBN, SEGS_MX, kname("_sk", prec, 0, 8), expect=dict(lanes=lanes, seam=prec == 7, mf=8))
    if name.startswith("p8_small"):
        return mk(3 * 256, 512, SEGS_MX_P8, kname("_p8", prec, 0), p8=1)
    return mk((g8 // 4 + 1) * 8 * 256, 4 * 256, SEGS_MX_P8, kname("_p8", prec, 0), p8=1, expect=dict(lanes=4, dealt=True))


def mx_cut_summary(c, cus):
    """cut positions of an MX case (steps of the whole walk), and where the second walk begins"""
    groups = seg_groups(c.segs)
    if c.p8:
        first = sum((g["ksteps"] >> 1) * g["nshift"] for g in groups)
        _, lanes, part = p8_partition(c.prec, c.m_tiles, c.n_tiles, c.segs, cus)
    else:
        first = c.ksteps
        _, lanes, part = sk_partition(c.prec, 8, c.m_tiles, c.n_tiles, c.segs, cus)
    pos = sorted({p[3] for w in part for p in w["parts"] if p[0] == "head"})
    spans = any(p[0] != "whole" and p[3] < first < p[4] for w in part for p in w["parts"])
    return dict(lanes=lanes, first_walk=first, positions=pos, part_across_walks=spans, partition=part)


def check_mx_claims(c, cus):
    """the partition of a stream-K / p8 MX case covers every tile once and has the cuts the case claims"""
    s = mx_cut_summary(c, cus)
    first, pos = s["first_walk"], s["positions"]
    if c.p8:
        total = first + (sum((g["ksteps"] // 4 >> 1) * g["nshift"] for g in seg_groups(c.segs)) if prec_mx2(c.prec) else 0)
        assert covers_every_tile_once(s["partition"], c.m_tiles // 2, c.n_tiles // 2, total)
        assert all(p % 2 == 0 for p in pos if p < first)                     # a pair of K tiles is never cut
        if c.expect.get("dealt"):
            assert {2, first - 2} <= set(pos), pos                          # behind the first pair, in front of the last
            if prec_mx2(c.prec):
                assert s["part_across_walks"] and first in pos               # a part across the two walks, and a cut at the seam
    else:
        total = first + (first // 4 if prec_mx2(c.prec) else 0)
        assert covers_every_tile_once(s["partition"], c.rows // 512, c.n_tiles, total)
        assert all(p % 4 == 0 for p in pos if p < first) and any(0 < p < first for p in pos)   # a 128-deep block is never cut
        if prec_mx2(c.prec):
            assert first in pos and any(p > first for p in pos), pos       # the seam and the second walk
    assert s["lanes"] == c.expect.get("lanes", s["lanes"])
    return s
