"""The extractor's frame-level and small kernels one launch at a time, through their entries in the C ABI (xv_kernel_first_layer,
xv_kernel_prep_input, xv_kernel_pool_finalise, xv_kernel_frame_output, and split-K / out_range of xv_kernel_tdnn_gemm): every device
row of a launch against a plain fp64 restatement of the operation - chunk edges, padding rows and alignment gaps included, which a
pooled embedding averages away.  References, operand scaling and bars are those of test_gpu_kernels.py."""
import functools

import numpy as np
import pytest

from helpers import pkg as _pkg
from test_gpu_kernels import (HALO, OUT_Q, P8_TDNN3, TDNN3, TOL, _decode_lo4, _lo4_plane, _run_case, _run_mx_case, _split,
                              _torch)

pytestmark = pytest.mark.gpu

XV_ERR_ARG = 4
LENS = [1, 15, 16, 17, 64, 100, 7]


# ---------------------------------------------------------------------------------------------------------------------
# the device-row layout of a batch and the input plane X_dev it defines
def _layout(lens, pad_left, pad_right, rows, gap_after=3, gap_groups=2, first_src_row=5):
    """chunks back to back on 16-row boundaries, gap_groups unused 16-row groups behind chunk gap_after, the rest of `rows` unused"""
    row_off = np.zeros(len(lens) + 1, dtype=np.int32)
    row_off[0] = first_src_row
    row_off[1:] = first_src_row + np.cumsum(lens)
    dev_off = np.zeros(len(lens), dtype=np.int32)
    at = 0
    for b, T in enumerate(lens):
        dev_off[b] = at
        at += (T + pad_left + pad_right + 15) // 16 * 16
        if b == gap_after:
            at += 16 * gap_groups
    assert at <= rows, (at, rows)
    return row_off, dev_off


def _x_dev(feats, row_off, dev_off, pad_left, pad_right, rows, ld):
    """row r of chunk b at t = r - dev_off[b] < len + pad_left + pad_right holds source frame clamp(t - pad_left, 0, len - 1);
    every other row, and every column beyond the feature dimension, is zero"""
    x = np.zeros((rows, ld), dtype=np.float32)
    dim = feats.shape[1]
    for b in range(len(dev_off)):
        T = int(row_off[b + 1] - row_off[b])
        t = np.arange(T + pad_left + pad_right)
        x[dev_off[b] + t, :dim] = feats[row_off[b] + np.clip(t - pad_left, 0, T - 1)]
    return x


def _feats(row_off, dim, amp, seed):
    """the packed rows of the batch between rows that belong to nobody (NaN: whoever reads them shows)"""
    rng = np.random.default_rng(seed)
    f = np.full((int(row_off[-1]) + 3, dim), np.nan, dtype=np.float32)
    f[row_off[0]:row_off[-1]] = rng.standard_normal((int(row_off[-1] - row_off[0]), dim)) * amp
    return f


def _grp_utt(row_off, dev_off, pad_left, pad_right, rows):
    g = np.full(rows // 16, -1, dtype=np.int32)
    for b in range(len(dev_off)):
        T = int(row_off[b + 1] - row_off[b])
        g[dev_off[b] // 16:(dev_off[b] + (T + pad_left + pad_right + 15) // 16 * 16) // 16] = b
    return g


# ---------------------------------------------------------------------------------------------------------------------
# tdnn_first_kernel
def _first_case(dim, offsets, prec=3, n_pad=128, lens=LENS, rows=512, pads=(7, 9), row0=0, nrows=None, max_wgs=0, seed=0,
                out_range=False, gap_after=3, want_ref=True):
    """One launch of xv_kernel_first_layer.  Returns a dict: hi / lo (raw planes as int16 arrays), value (what the planes say,
    float64), ref (float64 [rows, n_pad]), gmax / gmax_ref."""
    torch = _torch()
    P = _pkg()
    dev = torch.device("cuda:0")
    nrows = rows - row0 if nrows is None else nrows
    pl, pr = pads
    noff = len(offsets)
    f16 = prec != 0
    dt = torch.float16 if f16 else torch.bfloat16
    amp = 16.0 if prec in (3, 4, 8) else 1.0        # as _run_case: the fp16 residual planes stay normal numbers
    row_off, dev_off = _layout(lens, pl, pr, rows, gap_after=gap_after)
    feats = _feats(row_off, dim, amp, seed)
    seg_pad = (dim + 31) // 32 * 32                  # the generic walk: every Append() term padded to whole K steps
    ldw = noff * seg_pad
    K = noff * dim
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = (torch.randn(n_pad, ldw, generator=g) * (amp * amp / np.sqrt(K))).to(dev)     # padding columns too: they must not be read
    bias = (torch.randn(n_pad, generator=g) * 0.1).to(dev)
    scale = ((torch.rand(n_pad, generator=g) + 0.5) / 4).to(dev)   # (K is as short as 1: keeps the fp16 planes inside their range)
    offset = (torch.randn(n_pad, generator=g) * 0.1).to(dev)
    Wh, Wl = _split(W, 3 if f16 else 0, torch, True)
    feats_d = torch.from_numpy(feats).to(dev)

    d = P.FirstLayerDesc()
    d.feats, d.row_offsets, d.dev_off, d.B = feats_d.data_ptr(), row_off.ctypes.data, dev_off.ctypes.data, len(lens)
    d.rows, d.pad_left, d.pad_right = rows, pl, pr
    d.dim, d.noff = dim, noff
    for j, o in enumerate(offsets):
        d.off[j] = o
    d.w_hi, d.w_lo, d.ldw, d.seg_pad, d.n_pad = Wh.data_ptr(), Wl.data_ptr(), ldw, seg_pad, n_pad
    d.epi_prec = prec
    d.bias, d.scale, d.offset, d.relu, d.bn = bias.data_ptr(), scale.data_ptr(), offset.data_ptr(), 1, 1
    SENT = -7.0
    oh = torch.full((rows, n_pad), SENT, dtype=dt, device=dev)
    ol = torch.full((rows, n_pad), SENT, dtype=dt, device=dev)
    d.out_hi, d.ldo = oh.data_ptr(), n_pad
    d.out_lo = ol.data_ptr() if prec in (0, 3) else None
    if prec == 8:
        o4 = torch.zeros(rows, n_pad // 2, dtype=torch.uint8, device=dev)
        o4s = torch.zeros(rows, (n_pad // 64 + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        d.out_lo4, d.out_lo4_scale = o4.data_ptr(), o4s.data_ptr()
    d.row0, d.nrows, d.max_wgs = row0, nrows, max_wgs
    counted = None
    if out_range:
        rng = np.random.default_rng(seed)
        first = rng.integers(0, 10, rows // 16).astype(np.int8)
        last = np.minimum(16, first + rng.integers(0, 17, rows // 16)).astype(np.int8)
        first[1], last[1] = 5, 5        # nothing counts
        first[2], last[2] = 0, 16       # everything does
        rt = torch.from_numpy(np.stack([first, last], 1).copy()).to(dev)
        gm = torch.zeros(rows // 16, dtype=torch.int32, device=dev)
        d.gmax_out, d.out_range = gm.data_ptr(), rt.data_ptr()
        counted = (np.arange(16)[None, :] >= first[:, None]) & (np.arange(16)[None, :] < last[:, None])
    torch.cuda.synchronize()
    P.kernel_first_layer(d)
    torch.cuda.synchronize()
    res = {"hi": oh.view(torch.int16).cpu().numpy(), "lo": ol.view(torch.int16).cpu().numpy(), "sentinel": SENT,
           "hi_f": oh.double().cpu().numpy()}
    if prec in (0, 3):
        res["value"] = oh.double().cpu().numpy() + ol.double().cpu().numpy()
    elif prec == 8:
        res["value"] = oh.double().cpu().numpy() + _decode_lo4(o4, o4s, n_pad)
    else:
        res["value"] = oh.double().cpu().numpy()
    if not want_ref:
        return res
    # ---- the reference, from scratch: X_dev, quantised as the kernel quantises it (hi + lo), spliced and multiplied in fp64
    X = torch.from_numpy(_x_dev(feats, row_off, dev_off, pl, pr, rows, dim)).to(dev)
    assert bool(torch.isfinite(X).all())
    xh, xl = _split(X, 3 if f16 else 0, torch, True)
    Xq = torch.zeros(rows + 2 * HALO, dim, dtype=torch.float64, device=dev)     # rows outside [0, rows) are zero
    Xq[HALO:HALO + rows] = xh.double() + xl.double()
    Wq = Wh.double() + Wl.double()
    z = torch.zeros(rows, n_pad, dtype=torch.float64, device=dev)
    for j, o in enumerate(offsets):
        z += Xq[HALO + o:HALO + o + rows] @ Wq[:, j * seg_pad:j * seg_pad + dim].T
    z = torch.clamp(z + bias.double(), min=0) * scale.double() + offset.double()
    res["ref"] = z.cpu().numpy()
    if out_range:
        res["gmax"] = gm.view(torch.float32).cpu().numpy()
        res["gmax_ref"] = (np.abs(z.float().cpu().numpy()).reshape(rows // 16, 16, n_pad) * counted[:, :, None]).max(axis=(1, 2))
        res["empty"] = ~counted.any(axis=1)
    return res


def _check_first(res, prec, row0=0, nrows=None):
    ref = res["ref"]
    nrows = ref.shape[0] - row0 if nrows is None else nrows
    sl = slice(row0, row0 + nrows)
    got, want = res["value"][sl], ref[sl]
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    if prec == 8:   # the two assertions of test_gemm_planes_epilogue_with_4bit_residual
        blk = np.abs(want).reshape(want.shape[0], -1, 64).max(axis=2, keepdims=True)
        rel = (err.reshape(want.shape[0], -1, 64) / np.maximum(blk, 1e-30)).max()
        print("first layer, precision 8: block-relative error %.3g, rms %.3g of %.3g" %
              (rel, np.sqrt((err ** 2).mean()), np.sqrt((want ** 2).mean())))
        assert rel < 2.0 ** -13 * 1.05 + TOL[3], rel
        assert np.sqrt((err ** 2).mean()) < 0.25 * 2.0 ** -12 * np.sqrt((want ** 2).mean())
        return
    bar = TOL[4] + OUT_Q[4] if prec == 4 else TOL[3] + OUT_Q[prec]
    e = err.max() / np.abs(want).max()
    print("first layer, precision %d: max error / max |ref| = %.3g (bar %.3g)" % (prec, e, bar))
    assert e < bar, (e, int(err.max(axis=1).argmax()) + row0)
    # rows outside the launched region keep what was there
    hi = res["hi_f"]
    assert np.all(hi[:row0] == res["sentinel"]) and np.all(hi[row0 + nrows:] == res["sentinel"])


FIRST_SHAPES = [(23, (-2, -1, 0, 1, 2)), (5, (-2, -1, 0, 1, 2)), (24, (-2, -1, 0, 1, 2)),
                (16, (-7, -1, 0, 2, 4, 5, 6, 8)),     # K = 128 exactly: no spare column in the compact image
                (16, (-15, 0, 15)), (8, (-15, -9, 0, 15)), (1, (0,)),
                (13, (2, -1, 0)),                      # not monotonic
                (8, (3, 5, 9)), (8, (-9, -5, -3))]     # all positive / all negative: the unit's own frames are never read


@pytest.mark.parametrize("pads", [(0, 0), (7, 9)], ids=["nopad", "pad7_9"])
@pytest.mark.parametrize("dim,offsets", FIRST_SHAPES, ids=["%d_%s" % (d, "_".join(str(o) for o in o_)) for d, o_ in FIRST_SHAPES])
def test_first_layer_every_device_row(dim, offsets, pads):
    """Chunks of 1 .. 100 frames, a gap of unused groups between two of them and behind the last, source rows that start at 5 with
    NaN around them: every device row - chunk edges (clamped or replicated), rows that read the neighbouring chunk, padding rows,
    unused groups - against the fp64 splice of the quantised input plane."""
    _check_first(_first_case(dim, offsets, prec=3, pads=pads, seed=3), 3)


@pytest.mark.parametrize("n_pad", [128, 384, 512, 640, 1152])
def test_first_layer_column_groups(n_pad):
    # 128 / 384: waves without columns; 640: a second column group of 128 columns; 1152: three groups
    _check_first(_first_case(23, (-2, -1, 0, 1, 2), prec=3, n_pad=n_pad, seed=4), 3)


@pytest.mark.parametrize("pads", [(0, 0), (7, 9)], ids=["nopad", "pad7_9"])
@pytest.mark.parametrize("prec", [0, 3, 4, 8])
def test_first_layer_planes_of_every_precision(prec, pads):
    _check_first(_first_case(23, (-2, -1, 0, 1, 2), prec=prec, pads=pads, seed=5), prec)


@pytest.mark.parametrize("pads", [(0, 0), (7, 9)], ids=["nopad", "pad7_9"])
def test_first_layer_region_launch(pads):
    """rows [256, 512) of the same layout: the region starts inside a chunk, and the rows in front of it keep the sentinel"""
    res = _first_case(23, (-2, -1, 0, 1, 2), prec=3, pads=pads, row0=256, nrows=256, seed=6)
    _check_first(res, 3, row0=256, nrows=256)
    assert np.all(res["hi"][:256] == res["hi"][0, 0]) and np.all(res["lo"][:256] == res["lo"][0, 0])


def _ragged_lens(total_rows, seed):
    rng = np.random.default_rng(seed)
    lens, at = [], 0
    while True:
        T = int(rng.integers(1, 300))
        if at + (T + 15) // 16 * 16 + 64 > total_rows:
            return lens
        lens.append(T)
        at += (T + 15) // 16 * 16


def test_first_layer_table_window_is_rebuilt():
    """One workgroup for 200 row blocks (12 800 rows of ragged chunks): its window of the group table (96 row blocks) is rebuilt
    twice.  Same bits as the launch the launcher would size itself, and both agree with the reference."""
    lens = _ragged_lens(200 * 64 - 32, 7)
    kw = dict(prec=3, lens=lens, rows=200 * 64, pads=(0, 0), seed=7, gap_after=len(lens) // 2)
    one = _first_case(23, (-2, -1, 0, 1, 2), max_wgs=1, **kw)
    many = _first_case(23, (-2, -1, 0, 1, 2), max_wgs=0, want_ref=False, **kw)
    _check_first(one, 3)
    assert np.array_equal(one["hi"], many["hi"]) and np.array_equal(one["lo"], many["lo"])


@pytest.mark.parametrize("prec", [3, 8])
def test_first_layer_group_maxima_respect_out_range(prec):
    res = _first_case(23, (-2, -1, 0, 1, 2), prec=prec, seed=8, out_range=True)
    _check_first(res, prec)
    assert np.allclose(res["gmax"], res["gmax_ref"], rtol=1e-4, atol=0), (res["gmax"][:6], res["gmax_ref"][:6])
    assert np.all(res["gmax"][res["empty"]] == 0) and res["empty"].any()


@pytest.mark.parametrize("dim,offsets,nrows", [(30, (0,), 512),             # dp = 32: the feature buffers do not fit the LDS
                                               (23, (-15, 0, 15), 512),     # (64 + 30) x 24 staged elements: more than four per thread
                                               (8, (0, 16), 512),           # beyond the loader's +-15
                                               (23, (-2, -1, 0, 1, 2), 96)],
                         ids=["dp32", "span30_dp24", "offset16", "nrows96"])
def test_first_layer_refuses_what_the_kernel_cannot_run(dim, offsets, nrows):
    P = _pkg()
    with pytest.raises(P.XvError) as e:
        _first_case(dim, offsets, prec=3, nrows=nrows, want_ref=False)
    assert e.value.status == XV_ERR_ARG, e.value


# ---------------------------------------------------------------------------------------------------------------------
# prep_input_kernel
def _prep_case(prec, dim, ld, pads, rows=512, lens=LENS, n_zero=0):
    torch = _torch()
    P = _pkg()
    dev = torch.device("cuda:0")
    pl, pr = pads
    row_off, dev_off = _layout(lens, pl, pr, rows)
    feats = _feats(row_off, dim, 16.0 if prec == 3 else 1.0, 11)
    split = prec in (0, 3)
    dt = torch.float16 if prec in (2, 3) else torch.bfloat16
    t = [torch.from_numpy(a).to(dev) for a in (feats, row_off, dev_off, _grp_utt(row_off, dev_off, pl, pr, rows))]
    oh = torch.full((rows, ld), 3.0, dtype=dt, device=dev)
    ol = torch.full((rows, ld), 3.0, dtype=dt, device=dev)
    zw = torch.full((n_zero + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    d = P.PrepInputDesc()
    d.precision = prec
    d.feats, d.src_off, d.dev_off, d.grp_utt = (x.data_ptr() for x in t)
    d.rows, d.dim, d.ld = rows, dim, ld
    d.out_hi, d.out_lo = oh.data_ptr(), (ol.data_ptr() if split else None)
    d.pad_left, d.pad_right = pl, pr
    if n_zero:
        d.zero_words, d.n_zero_words = zw.data_ptr(), n_zero
    torch.cuda.synchronize()
    P.kernel_prep_input(d)
    torch.cuda.synchronize()
    X = torch.from_numpy(_x_dev(feats, row_off, dev_off, pl, pr, rows, ld)).to(dev)
    wh, wl = _split(X, prec, torch, split)
    assert torch.equal(oh.view(torch.int16), wh.view(torch.int16))
    if split:
        assert torch.equal(ol.view(torch.int16), wl.view(torch.int16))
    else:
        assert bool((ol == 3.0).all())
    return zw.cpu().numpy()


@pytest.mark.parametrize("pads", [(0, 0), (7, 9)], ids=["nopad", "pad7_9"])
@pytest.mark.parametrize("dim,ld", [(23, 32), (32, 32), (40, 64)])
@pytest.mark.parametrize("prec", [0, 1, 2, 3])
def test_prep_input_planes_are_the_split_of_the_input_plane(prec, dim, ld, pads):
    """every conversion is round-to-nearest-even on both sides: the planes are compared as bits (edge replication, zero rows of the
    padding and of unused groups, zero columns beyond the feature dimension)"""
    _prep_case(prec, dim, ld, pads)


def test_prep_input_clears_more_words_than_it_has_threads():
    zw = _prep_case(3, 23, 32, (0, 0), rows=128, lens=[1, 15, 16, 17], n_zero=5000)   # 512 threads for 5000 words
    assert np.all(zw[:5000] == 0) and zw[5000] == 0x5a5a5a5a


# ---------------------------------------------------------------------------------------------------------------------
# group maxima with out_range on the GEMM kernels
@pytest.mark.parametrize("p8", [0, 1])
@pytest.mark.parametrize("rows", ["small", "stream_k"])
def test_gemm_group_maxima_respect_out_range(rows, p8):
    """GemmArgs::out_range keeps a chunk's 4-bit scales independent of its neighbours in the batch: rows outside the range of their
    group (computed from another chunk's frames, or alignment padding) do not enter the recorded maximum."""
    if p8:
        out, ref = _run_mx_case(0, 100 * 256 if rows == "stream_k" else 3 * 256, 512, P8_TDNN3, seed=24, p8=1, out_range=True)
        tol = 2e-5 + 2.0 ** -10
    else:
        out, ref = _run_mx_case(0, 66 * 512 if rows == "stream_k" else 768, 512, TDNN3, seed=13, out_range=True)
        tol = TOL[4] + OUT_Q[4]
    assert np.abs(out - ref).max() / np.abs(ref).max() < tol


# ---------------------------------------------------------------------------------------------------------------------
# split-K: tdnn_gemm_kernel<.., kEpiSplitK> + splitk_reduce_kernel.  K -> slices by the engine's rule (at least 4 steps per slice, at
# most 24 slices): 224 -> 2 (last slice 3 steps), 896 -> 7, 1024 -> 8, 1056 -> 9 (last 1 step), 2048 -> 16, 2080 -> 17 (last 1
# step), 3008 -> 24 (94 steps, last slice 2)
SPLITK = [(224, 2), (896, 7), (1024, 8), (1056, 9), (2048, 16), (2080, 17), (3008, 24)]


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("prec", [0, 1, 2, 3])
@pytest.mark.parametrize("K,slices", SPLITK, ids=["k%d_s%d" % ks for ks in SPLITK])
def test_gemm_split_k(K, slices, prec, epi):
    out, ref = _run_case(prec, epi, 128, 256, [(0, K, 0, K)], relu=True, bn=True, seed=31, m_valid=70 if epi == 1 else None,
                         ksplit=slices)
    if epi == 1:
        assert np.all(out[70:] == -7.0)
        out, ref = out[:70], ref[:70]
    err = np.abs(out - ref).max() / np.abs(ref).max()
    bar = TOL[prec] + (OUT_Q[prec] if epi == 0 else 0)
    print("split-K %d slices, precision %d, epilogue %d: %.3g (bar %.3g)" % (slices, prec, epi, err, bar))
    assert err < bar, err


def test_gemm_split_k_refusals():
    P = _pkg()
    for prec, epi in ((4, 1), (8, 0)):
        with pytest.raises(P.XvError):
            _run_case(prec, epi, 128, 256, [(0, 256, 0, 256)], relu=True, bn=True, seed=1, ksplit=2)
    for prec in (6, 7, 9):
        with pytest.raises(P.XvError):
            _run_mx_case(0, 768, 512, TDNN3, seed=11, prec=prec, ksplit=12)
    with pytest.raises(P.XvError) as e:      # not the number of slices the rule gives for this K
        _run_case(3, 1, 128, 256, [(0, 256, 0, 256)], relu=True, bn=True, seed=1, ksplit=3)
    assert e.value.status == XV_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# pool_finalise_kernel
@pytest.mark.parametrize("prec", [0, 1, 2, 3])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("dim", [1500, 128])
def test_pool_finalise_is_kaldis_rounding_sequence(dim, B, prec):
    """Bit-exact: the partials summed in fp64 in group order, then float32 only - / n, a separately rounded mu * mu, the
    subtraction, the floor, the square root, every one correctly rounded on both sides.  Chunk 0 pools ONE frame (its variance
    cancels to exactly the floor), column 3 is constant in every chunk."""
    torch = _torch()
    P = _pkg()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100 + dim + B)
    counts = [1, 37, 16, 400, 250][:B]
    ldp = (dim + 127) // 128 * 128
    floor = np.float32(1e-10)
    g0, g1, parts = [], [], [np.full((2, 2, ldp), 7.0, np.float32)]     # two groups in front that belong to nobody
    for n in counts:
        y = (rng.standard_normal((n, dim)) * 3 + rng.standard_normal(dim)).astype(np.float32)
        y[:, 3] = 1.5
        g0.append(sum(p.shape[0] for p in parts))
        ng = (n + 15) // 16
        yp = np.zeros((ng * 16, ldp), np.float32)
        yp[:n, :dim] = y
        yp = yp.reshape(ng, 16, ldp)
        s = yp.astype(np.float64).sum(axis=1).astype(np.float32)
        q = (yp * yp).astype(np.float64).sum(axis=1).astype(np.float32) if n > 1 else yp[:, 0] * yp[:, 0]
        parts.append(np.stack([s, q], axis=1))
        g1.append(g0[-1] + ng)
    partial = np.concatenate(parts)
    # ---- emulation
    mu = np.zeros((B, dim), np.float32)
    sd = np.zeros((B, dim), np.float32)
    for b in range(B):
        s1 = np.zeros(dim, np.float64)
        s2 = np.zeros(dim, np.float64)
        for g in range(g0[b], g1[b]):
            s1 += partial[g, 0, :dim].astype(np.float64)
            s2 += partial[g, 1, :dim].astype(np.float64)
        n = np.float32(counts[b])
        m = s1.astype(np.float32) / n
        ex2 = s2.astype(np.float32) / n
        m2 = m * m
        var = np.maximum(ex2 - m2, floor)
        mu[b], sd[b] = m, np.sqrt(var)
        assert m.dtype == np.float32 and sd.dtype == np.float32
    assert np.all(sd[0] == np.sqrt(floor)) and np.all(sd[:, 3] == np.sqrt(floor)) and np.all(mu[:, 3] == 1.5)
    if B > 1:
        assert np.all(sd[1:, :3] > 1.0)
    split = prec in (0, 3)
    dt = torch.float16 if prec in (2, 3) else torch.bfloat16
    ld = (2 * dim + 31) // 32 * 32 + 32
    oh = torch.full((B, ld), 3.0, dtype=dt, device=dev)
    ol = torch.full((B, ld), 3.0, dtype=dt, device=dev)
    t = [torch.from_numpy(np.asarray(a)).to(dev) for a in (partial, np.array(g0, np.int32), np.array(g1, np.int32), np.array(counts, np.int32))]
    d = P.PoolFinaliseDesc()
    d.precision, d.partial, d.ldp = prec, t[0].data_ptr(), ldp
    d.utt_grp0, d.utt_grp1, d.utt_count = t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr()
    d.B, d.dim, d.var_floor = B, dim, float(floor)
    d.out_hi, d.out_lo, d.ld = oh.data_ptr(), (ol.data_ptr() if split else None), ld
    torch.cuda.synchronize()
    P.kernel_pool_finalise(d)
    torch.cuda.synchronize()
    want = torch.from_numpy(np.concatenate([mu, sd], axis=1)).to(dev)
    wh, wl = _split(want, prec, torch, split)
    assert torch.equal(oh[:, :2 * dim].view(torch.int16), wh.view(torch.int16))
    assert bool((oh[:, 2 * dim:] == 3.0).all())
    if split:
        assert torch.equal(ol[:, :2 * dim].view(torch.int16), wl.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------
# frame_output kernels
# |out - ref| <= LSM_ABS + ulp_f32(|ref|): the bound test_gpu_frames.py puts on a row's normalisation + the rounding of the result.
# A float32 emulation of the kernels' order of summation (per-thread strided sums, a 64-lane tree, four wave sums) on these inputs
# stays within 4.4e-6 (worst row: dim 16385) - test_log_softmax_bar_covers_the_kernels_order_of_summation asserts it.
LSM_ABS = 2e-5
LSM_DIMS = [100, 2048, 2052, 3856, 5139, 8196, 16384, 16385, 20000]


@functools.lru_cache(maxsize=None)
def _logits(dim, half=False):
    x = (np.random.default_rng(dim).standard_normal((5, dim)) * 8).astype(np.float32)
    return x.astype(np.float16) if half else x


def _lsm_ref(x):
    x = x.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def _lsm_check(out, ref):
    err = np.abs(out.astype(np.float64) - ref)
    bar = LSM_ABS + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print("log-softmax: max |out - ref| = %.3g" % err.max())
    assert np.all(err <= bar), (err.max(), int((err - bar).argmax()))


def _lsm_emulation(x, vec):
    """float32, in the kernels' order: thread t of 256 sums exp(x - max) over its columns in increasing order (vector kernels: four
    consecutive columns per step), a butterfly over the 64 lanes of a wave, (w0 + w1) + (w2 + w3)"""
    x = x.astype(np.float32)
    dim = x.shape[0]
    m = x.max()
    if vec:   # step i: columns (t + 256 i) * 4 + (0 .. 3); columns beyond the row add exp(-inf) = 0
        cols = np.stack([(np.arange(256) + 256 * (j // 4)) * 4 + j % 4 for j in range(4 * ((dim + 1023) // 1024))], axis=1)
    else:
        cols = np.stack([np.arange(256) + 256 * i for i in range((dim + 255) // 256)], axis=1)
    acc = np.zeros(256, np.float32)
    for i in range(cols.shape[1]):
        c = cols[:, i]
        ok = c < dim
        e = np.exp((x[np.where(ok, c, 0)] - m).astype(np.float32)).astype(np.float32)
        acc = (acc + np.where(ok, e, np.float32(0))).astype(np.float32)
    w = acc.reshape(4, 64)
    for dlt in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ dlt]).astype(np.float32)
    tot = np.float32(np.float32(w[0, 0] + w[1, 0]) + np.float32(w[2, 0] + w[3, 0]))
    lse = np.float32(m + np.log(tot, dtype=np.float32))
    return (x - lse).astype(np.float32)


def test_log_softmax_bar_covers_the_kernels_order_of_summation():
    worst = 0.0
    for dim in LSM_DIMS:
        x = _logits(dim)
        ref = _lsm_ref(x)
        for r in range(x.shape[0]):
            em = _lsm_emulation(x[r], vec=dim % 4 == 0 and dim <= 16384)
            err = np.abs(em.astype(np.float64) - ref[r])
            worst = max(worst, err.max())
            assert np.all(err <= LSM_ABS + np.spacing(np.abs(ref[r]).astype(np.float32)))
    print("emulated log-softmax: worst |out - ref| = %.3g" % worst)
    assert worst < LSM_ABS / 2      # (else the constant would have to be 2 x this)


def _frame_output(x, dim, log_softmax=1, out_row=(3, 0, 2), out_ld=None, out_shift=0, half=False):
    torch = _torch()
    P = _pkg()
    dev = torch.device("cuda:0")
    ld = x.shape[1]
    src = torch.from_numpy(x).to(dev)
    n_out = 3
    out_ld = out_ld or (dim + 3) // 4 * 4
    buf = torch.full((n_out * out_ld + 8,), 9.0, dtype=torch.float32, device=dev)
    d = P.FrameOutputDesc()
    if half:
        d.src16 = src.data_ptr()
    else:
        d.src = src.data_ptr()
    d.ld, d.n_out, d.dim, d.log_softmax = ld, n_out, dim, log_softmax
    rows_t = None
    if out_row is not None:
        rows_t = torch.tensor(out_row, dtype=torch.int32, device=dev)
        d.out_row = rows_t.data_ptr()
    d.out, d.out_ld = buf.data_ptr() + 4 * out_shift, out_ld
    torch.cuda.synchronize()
    P.kernel_frame_output(d)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    out = b[out_shift:out_shift + n_out * out_ld].reshape(n_out, out_ld)
    assert np.all(out[:, dim:] == 9.0) and np.all(b[:out_shift] == 9.0) and np.all(b[out_shift + n_out * out_ld:] == 9.0)
    return out[:, :dim], list(out_row) if out_row is not None else list(range(n_out))


def _padded(x):
    """[5, dim] -> [5, ld] with ld a multiple of four floats (what a vector kernel needs) and columns nobody may read as logits"""
    dim = x.shape[1]
    p = np.full((x.shape[0], (dim + 3) // 4 * 4 + 4), 1e4, dtype=x.dtype)
    p[:, :dim] = x
    return p


@pytest.mark.parametrize("out_row", [(3, 0, 2), None], ids=["gather", "rows_in_order"])
@pytest.mark.parametrize("dim", LSM_DIMS)
def test_frame_output_log_softmax(dim, out_row):
    # floats per thread N = 8: 100, 2048; 16: 2052, 3856; 32: 5139 (scalar loads: not a multiple of four); 64: 8196, 16384; wider
    # rows take the three-pass kernel
    x = _logits(dim)
    out, rows = _frame_output(_padded(x), dim, out_row=out_row)
    _lsm_check(out, _lsm_ref(x)[rows])


@pytest.mark.parametrize("dim", [2048, 5139, 16384])
def test_frame_output_log_softmax_of_fp16_logits(dim):
    x = _logits(dim, half=True)
    out, rows = _frame_output(_padded(x), dim, half=True)
    _lsm_check(out, _lsm_ref(x)[rows])


@pytest.mark.parametrize("how", ["odd_out_ld", "out_off_by_one_float"])
def test_frame_output_scalar_path_at_a_vector_friendly_dim(how):
    x = _logits(2048)
    if how == "odd_out_ld":
        out, rows = _frame_output(_padded(x), 2048, out_ld=2049)
    else:
        out, rows = _frame_output(_padded(x), 2048, out_shift=1)
    _lsm_check(out, _lsm_ref(x)[rows])


@pytest.mark.parametrize("out_row", [(3, 0, 2), None], ids=["gather", "rows_in_order"])
@pytest.mark.parametrize("dim", [100, 2048, 5139])
def test_frame_output_plain_gather_is_bit_equal(dim, out_row):
    x = _logits(dim)
    out, rows = _frame_output(_padded(x), dim, log_softmax=0, out_row=out_row)
    assert np.array_equal(out.view(np.int32), x[rows].view(np.int32))
