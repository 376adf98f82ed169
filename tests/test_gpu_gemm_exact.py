"""The spliced-GEMM kernels bit for bit: tdnn_gemm_kernel, _v2, _sk<4|8>, _p8 and split-K through xv_kernel_tdnn_gemm against the
exact fp64 reference of gemm_exact_ref.py.  The operands make every product and every partial sum an exact fp32 number (the
precondition is asserted on the CPU, test_gemm_exact_ref.py), so no comparison here has a tolerance: np.array_equal on bit
patterns over whole buffers - the gaps behind n_pad, the rows at and above m_valid and guard rows around every output included.
Every case asserts the name of the kernel that ran; stream-K and p8 cases recompute their kernel and their cut classes from the
device's own CU count and fail (not skip) when a class is not reached."""
import numpy as np
import pytest

import gemm_exact_ref as R
from helpers import pkg as _pkg

pytestmark = pytest.mark.gpu

HALO = R.HALO
GUARD = 16     # sentinel rows in front of and behind every output buffer


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _guarded(rows, width, sentinel, dtype):
    """device buffer [GUARD + rows + GUARD, width] full of the sentinel"""
    return _dev(np.full((rows + 2 * GUARD,) + tuple(width), sentinel, dtype=dtype))


def launch(c, ops, X=None):
    """One launch of case c.  Returns (kernel name, {output name: (numpy buffer with guard rows, rows per guard)})."""
    torch = _torch()
    P = _pkg()
    X = ops["X"] if X is None else X
    d = P.GemmDesc()
    d.precision, d.epilogue, d.nseg = c.prec, c.epi, len(c.segs)
    planes = []
    for hb, lb in X:
        h = _dev(hb)
        l = _dev(lb) if lb is not None else None
        planes.append((h, l))
    for j, (si, ld, shift, klen) in enumerate(c.segs):
        h, l = planes[si]
        pitch = c.src_ld[si] * 2
        d.seg[j].hi = h.data_ptr() + HALO * pitch
        d.seg[j].lo = (l.data_ptr() + HALO * pitch) if l is not None else None
        d.seg[j].ld, d.seg[j].row_shift, d.seg[j].k_len = c.src_ld[si], shift, klen
    wh = _dev(ops["W"][0])
    wl = _dev(ops["W"][1]) if ops["W"][1] is not None else None
    d.w_hi, d.w_lo, d.ldw = wh.data_ptr(), (wl.data_ptr() if wl is not None else None), c.ldw
    d.rows, d.n_pad = c.rows, c.n_pad
    bias, scale, offset = _dev(ops["bias"]), _dev(ops["scale"]), _dev(ops["offset"])
    d.bias, d.scale, d.offset = bias.data_ptr(), scale.data_ptr(), offset.data_ptr()
    d.relu, d.bn = int(c.relu), int(c.bn)
    d.hip_stream = None
    d.p8, d.ksplit = c.p8, c.ksplit
    rng = _dev(ops["range"])
    bufs = {}
    if c.epi == R.EPI_ACT:
        bufs["hi"] = (_guarded(c.rows, (c.ldo,), R.SENT16, np.uint16), np.uint16, GUARD)
        d.out_hi, d.ldo = bufs["hi"][0].data_ptr() + GUARD * c.ldo * 2, c.ldo
        if R.prec_emits_lo4(c.prec):
            p4, ps = c.ldo // 2, R.lo4_scale_pitch(c.ldo)
            bufs["lo4"] = (_guarded(c.rows, (p4,), R.SENT8, np.uint8), np.uint8, GUARD)
            bufs["lo4s"] = (_guarded(c.rows, (ps,), R.SENT8, np.uint8), np.uint8, GUARD)
            d.out_lo4, d.out_lo4_scale = bufs["lo4"][0].data_ptr() + GUARD * p4, bufs["lo4s"][0].data_ptr() + GUARD * ps
        elif R.prec_x_planes(c.prec) == 2:
            bufs["lo"] = (_guarded(c.rows, (c.ldo,), R.SENT16, np.uint16), np.uint16, GUARD)
            d.out_lo = bufs["lo"][0].data_ptr() + GUARD * c.ldo * 2
        if c.gmax:   # [guard word | rows / 16 zeros | guard word]
            g = np.zeros(c.rows // 16 + 2, dtype=np.uint32)
            g[0] = g[-1] = R.SENT_U32
            bufs["gmax"] = (_dev(g), np.uint32, 1)
            d.gmax_out, d.out_range = bufs["gmax"][0].data_ptr() + 4, rng.data_ptr()
    elif c.epi == R.EPI_F32:
        bufs["f32"] = (_guarded(c.rows, (c.ldf,), R.SENT_F32, np.float32), np.uint32, GUARD)
        d.out_f32, d.ldf, d.m_valid = bufs["f32"][0].data_ptr() + GUARD * c.ldf * 4, c.ldf, c.m_valid
    else:
        gg = 2   # guard groups
        bufs["partial"] = (_dev(np.full((c.rows // 16 + 2 * gg, 2, c.ldp), R.SENT_F32, dtype=np.float32)), np.uint32, gg)
        d.partial, d.ldp, d.grp_range = bufs["partial"][0].data_ptr() + gg * 2 * c.ldp * 4, c.ldp, rng.data_ptr()
    torch.cuda.synchronize()
    P.kernel_tdnn_gemm(d)
    name = P.last_gemm_kernel()
    torch.cuda.synchronize()
    return name, {k: (_host(t, dt), g) for k, (t, dt, g) in bufs.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(c, what, got, want):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (c, what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s %s: %d of %d elements differ, first at %s: got 0x%x, want 0x%x; rows %d..%d, columns %d..%d" % (
            c.name, what, len(bad), got.size, i, got[i], want[i], bad[:, 0].min(), bad[:, 0].max(), bad[:, -1].min(), bad[:, -1].max()))


def check_outputs(c, outs, want):
    """every buffer against the reference, its guard rows against the sentinel"""
    assert set(outs) == set(want), (set(outs), set(want))
    for k, (buf, g) in outs.items():
        body = buf[g:len(buf) - g]
        assert_bits(c, k, body, want[k])
        sent = {"gmax": R.SENT_U32}.get(k)
        guard = np.concatenate([buf[:g], buf[len(buf) - g:]])
        if sent is None:
            sent = _bits(np.array([{1: R.SENT8, 2: R.SENT16}.get(buf.dtype.itemsize, R.SENT_F32)], dtype=want[k].dtype))[0]
        assert np.all(_bits(guard) == sent), "%s %s: rows outside the launch were written" % (c.name, k)


def run_case(c, kernel=None):
    ops = R.make_operands(c)
    R.check_precondition(c, ops)
    want = R.reference(c, ops)
    name, outs = launch(c, ops)
    assert name == (kernel or c.kernel), (c, name)
    check_outputs(c, outs, want)
    return name


# ---- per-tile and 256-row kernels -----------------------------------------------------------------------------------------------------
PREC_EPI = [(p, e) for p in R.PRECS for e in R._epis(p)]


@pytest.mark.parametrize("prec,epi", PREC_EPI)
def test_per_tile_kernel(prec, epi):
    """tdnn_gemm_kernel: 1, 3 and 9 row tiles x 1 and 3 column tiles, m_valid 0, 1, rows - 1 and rows (fp32 epilogue)"""
    cus = _cus()
    for c in R.per_tile_cases(prec, epi):
        assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, cus) == c.kernel
        run_case(c)


@pytest.mark.parametrize("prec,epi", PREC_EPI)
def test_v2_kernel(prec, epi):
    """tdnn_gemm_kernel_v2: 2 and 22 row tiles of 128 (11 of 256: not a multiple of 8)"""
    cus = _cus()
    for c in R.v2_cases(prec, epi):
        assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, cus) == c.kernel
        run_case(c)


@pytest.mark.parametrize("walk", [w[0] for w in R.WALKS])
def test_walk_planning(walk):
    for c in R.walk_cases(walk):
        run_case(c)


@pytest.mark.parametrize("steps", R.SPLITK_STEPS)
def test_split_k(steps):
    """every slice count the engine's rule yields for 8 to 48 K steps, planes and fp32 epilogues"""
    for c in R.splitk_cases(steps):
        run_case(c)


# ---- stream-K and p8: kernel and cut classes from the device's CU count ---------------------------------------------------------------
@pytest.mark.parametrize("name", R.SK_NAMES)
def test_stream_k(name):
    cus = _cus()
    c = R.sk_case(name, cus)
    grid, lanes, cc = R.check_sk_claims(c, cus)
    kernel = run_case(c)
    print("%s: %d x %d, %d K steps, %s on %d CUs: grid %d, %d lanes, regime %d, heads %s tails %s cuts %s" % (
        c.name, c.rows, c.n_pad, c.ksteps, kernel, cus, grid, lanes, c.expect["regime"], sorted(cc["heads"]), sorted(cc["tails"]),
        sorted(cc["kinds"])))


@pytest.mark.parametrize("name", R.P8_NAMES)
def test_p8(name):
    cus = _cus()
    c = R.p8_case(name, cus)
    grid, lanes, cc = R.check_p8_claims(c, cus)
    kernel = run_case(c)
    print("%s: %d x %d, %d K tiles, %s on %d CUs: grid %d, %d lanes, heads %s tails %s" % (
        c.name, c.rows, c.n_pad, cc["S"], kernel, cus, grid, lanes, sorted(cc["heads"]), sorted(cc["tails"])))


# ---- dependency footprint -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,epi", [("tile", 0), ("tile", 1), ("v2", 0), ("v2", 1), ("sk", 0), ("sk", 1), ("p8", 0)])
def test_dependency_footprint(kernel, epi):
    """One NaN at X[r0, c0] of source 0 - r0 in the body, in the first 16-row group, in the halo: exactly the rows r0 - shift_j of
    the segments that hold column c0 are NaN, in every column; every other element of the planes / of the fp32 rows (gaps and
    guard rows included) has the bits of the clean run.  (The cases record no group maxima and emit no 4-bit residual.)"""
    c = R.footprint_case(kernel, epi, _cus())
    ops = R.make_operands(c)
    R.check_precondition(c, ops)
    name, clean = launch(c, ops)
    assert name == c.kernel
    check_outputs(c, clean, R.reference(c, ops))
    f16 = R.prec_f16(c.prec)
    c0 = 5
    for r0 in (c.rows // 2 + 37, 3, -2):
        X = [(h.copy(), None if l is None else l.copy()) for h, l in ops["X"]]
        X[0][0][HALO + r0, c0] = R.nan16(f16)
        name, outs = launch(c, ops, X)
        assert name == c.kernel
        rows = R.footprint_rows(c, 0, r0, c0)
        assert rows, (c, r0)
        for k, (buf, g) in outs.items():
            ref = clean[k][0]
            got = buf.copy()
            body = got[g:len(got) - g]
            if k in ("hi", "lo"):
                assert np.all(np.isnan(R.val16(body[rows][:, :c.n_pad], f16))), (c, k, r0)
            elif k == "f32":
                live = [r for r in rows if r < c.m_valid]
                assert np.all(np.isnan(body[live][:, :c.n_pad].view(np.float32))), (c, k, r0)
            assert k in ("hi", "lo", "f32"), k
            body[rows, :c.n_pad] = ref[g:len(ref) - g][rows, :c.n_pad]      # everything else: the clean run
            assert_bits(c, "%s beside the footprint of row %d" % (k, r0), got, ref)


# ---- the block-scaled modes ---------------------------------------------------------------------------------------------------------------
def launch_mx(c, ops, pk):
    """One launch of an MX case (planes epilogue): fp16 planes + group maxima, the library's packed 4-bit planes, and for fp16mx2
    the activations' residual planes."""
    torch = _torch()
    P = _pkg()
    d = P.GemmDesc()
    d.precision, d.epilogue, d.nseg = c.prec, c.epi, len(c.segs)
    src = []
    for i in range(len(ops["Xh"])):
        lo4 = ops["lo4"][i]
        src.append((_dev(ops["Xh"][i]), _dev(ops["gmax"][i]), None if lo4 is None else _dev(lo4[0]), None if lo4 is None else _dev(lo4[1])))
    for j, (si, ld, shift, klen) in enumerate(c.segs):
        h, gm, l4, l4s = src[si]
        d.seg[j].hi, d.seg[j].lo = h.data_ptr() + HALO * ld * 2, None
        d.seg[j].ld, d.seg[j].row_shift, d.seg[j].k_len = ld, shift, klen
        d.seg[j].gmax = gm.data_ptr()
        if l4 is not None:
            d.seg[j].lo4 = l4.data_ptr() + HALO * (ld // 2)
            d.seg[j].lo4_scale = l4s.data_ptr() + HALO * l4s.shape[1]
    wh, w4 = _dev(ops["Wh"]), _dev(pk["w4"])
    w4s = _dev(P.tile_mx_scales(pk["w4s"], c.epi))
    d.w_hi, d.w_lo, d.ldw = wh.data_ptr(), None, c.K
    d.w4, d.ldw4, d.w4_scale = w4.data_ptr(), c.K // 128 * 64, w4s.data_ptr()
    if R.prec_mx2(c.prec):
        w4b = _dev(pk["w4b"])
        w4bs = _dev(P.tile_mx_scales(pk["w4bs"], c.epi))
        d.w4b, d.ldw4b, d.w4b_scale = w4b.data_ptr(), (2 * c.K if c.p8 else c.K // 2), w4bs.data_ptr()
    d.rows, d.n_pad = c.rows, c.n_pad
    bias, scale, offset, rng = _dev(ops["bias"]), _dev(ops["scale"]), _dev(ops["offset"]), _dev(ops["range"])
    d.bias, d.scale, d.offset = bias.data_ptr(), scale.data_ptr(), offset.data_ptr()
    d.relu, d.bn, d.hip_stream, d.p8, d.ksplit = 1, 1, None, c.p8, 0
    bufs = {"hi": (_guarded(c.rows, (c.ldo,), R.SENT16, np.uint16), np.uint16, GUARD)}
    d.out_hi, d.out_lo, d.ldo = bufs["hi"][0].data_ptr() + GUARD * c.ldo * 2, None, c.ldo
    if R.prec_emits_lo4(c.prec):
        p4, ps = c.ldo // 2, R.lo4_scale_pitch(c.ldo)
        bufs["lo4"] = (_guarded(c.rows, (p4,), R.SENT8, np.uint8), np.uint8, GUARD)
        bufs["lo4s"] = (_guarded(c.rows, (ps,), R.SENT8, np.uint8), np.uint8, GUARD)
        d.out_lo4, d.out_lo4_scale = bufs["lo4"][0].data_ptr() + GUARD * p4, bufs["lo4s"][0].data_ptr() + GUARD * ps
    g = np.zeros(c.rows // 16 + 2, dtype=np.uint32)
    g[0] = g[-1] = R.SENT_U32
    bufs["gmax"] = (_dev(g), np.uint32, 1)
    d.gmax_out, d.out_range = bufs["gmax"][0].data_ptr() + 4, rng.data_ptr()
    torch.cuda.synchronize()
    P.kernel_tdnn_gemm(d)
    name = P.last_gemm_kernel()
    torch.cuda.synchronize()
    return name, {k: (_host(t, dt), gd) for k, (t, dt, gd) in bufs.items()}


@pytest.mark.parametrize("name", R.MX_NAMES)
def test_block_scaled_modes(name):
    """fp16mx, fp16mx2 and fp16mxe on the 256-row kernel, stream-K and p8: operands that every quantiser returns unchanged (asserted
    by reference_z_mx with the library's own packers), so the fp16 plane, its 4-bit residual image and scale bytes, and the group
    maxima have one right answer per element.  fp16mx2 on stream-K is cut in the first walk, at the seam and in the second walk;
    on p8 a part runs across the two walks."""
    cus = _cus()
    c = R.mx_case(name, cus)
    assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, cus, p8=c.p8) == c.kernel
    if not name.startswith("v2"):
        R.check_mx_claims(c, cus)
    ops = R.make_mx_operands(c)
    pk = R.mx_pack(c, ops, _pkg())
    want = R.reference(c, ops, z=R.reference_z_mx(c, ops, pk))
    kernel, outs = launch_mx(c, ops, pk)
    assert kernel == c.kernel, (c, kernel)
    check_outputs(c, outs, want)
