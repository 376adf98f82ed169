"""CPU half of the exact GEMM tests (gemm_exact_ref.py): the reference against a triple loop, the precondition under which
every summation order gives the same fp32 bits for every case of tests/test_gpu_gemm_exact.py, the kernel each case selects on
256 CUs and the cut classes its partition contains.  No GPU; the block-scaled cases call the library's host-side packers."""
import numpy as np
import pytest

import gemm_exact_ref as R

CUS = 256


def _check_case(c):
    ops = R.make_operands(c)
    bits = R.check_precondition(c, ops)
    assert bits < R.BIT_BUDGET
    return ops


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", R.PRECS)
def test_reference_matches_a_triple_loop(prec):
    c = R.Case("tiny", prec, R.EPI_F32 if prec != 8 else R.EPI_ACT, 16, 8, [(0, 32, -1, 32), (0, 32, 1, 32), (1, 64, 2, 32)], q=4)
    ops = R.make_operands(c)
    assert np.array_equal(R.reference_z(c, ops), R.reference_loops(c, ops))


def test_reference_sums_the_products_kernels_h_defines():
    """one element by hand, independent of the plane predicates the reference and the triple loop share: x = 3 + 2/16 at k = 0 and
    -2 + 1/16 at k = 1, w = 2 - 3/16 and 1 + 5/16; no bias, ReLU or BatchNorm"""
    xh, xl, wh, wl = np.array([3.0, -2.0]), np.array([2 / 16, 1 / 16]), np.array([2.0, 1.0]), np.array([-3 / 16, 5 / 16])
    want = {0: 3.125, 3: 3.125, 8: 3.125,        # hi.hi + hi.lo + lo.hi = 4 - 1.1875 + 0.3125 (a lo.lo term would subtract 1 / 256)
            4: 2.8125,                            # x.w_hi + x.w_lo = 4 - 1.1875
            1: 4.0, 2: 4.0}                       # one product
    for prec, z0 in want.items():
        c = R.Case("hand", prec, R.EPI_F32, 1, 1, [(0, 32, 0, 32)], relu=False, bn=False)
        X = np.zeros((1 + 2 * R.HALO, 32))
        W = np.zeros((1, 32))
        Xh, Xl, Wh, Wl = X.copy(), X.copy(), W.copy(), W.copy()
        Xh[R.HALO, :2], Xl[R.HALO, :2], Wh[0, :2], Wl[0, :2] = xh, xl, wh, wl
        ops = dict(Xv=[(Xh, Xl)], Wv=(Wh, Wl), bias=np.zeros(1, dtype=np.float32))
        assert R.reference_z(c, ops)[0, 0] == z0, prec


def test_three_pass_operands_would_show_a_lo_lo_product():
    c = R.Case("t", 3, 1, 128, 128, R.SEGS_SMALL, relu=False, bn=False)
    ops = R.make_operands(c)
    z = R.reference_z(c, ops)
    k0 = 0
    extra = np.zeros_like(z)
    for (si, ld, shift, klen) in c.segs:
        xl = ops["Xv"][si][1][R.HALO + shift: R.HALO + shift + c.rows, :klen]
        extra += xl @ ops["Wv"][1][:, k0:k0 + klen].T
        k0 += klen
    # both lo planes are non-zero at the same k in every row and column (column 0 of every segment): the sum of the lo . lo
    # products is non-zero in all but a few elements where it cancels, and fp32 keeps the difference
    assert np.mean(extra != 0) > 0.95
    assert np.mean((z + extra).astype(np.float32) != z.astype(np.float32)) > 0.95


@pytest.mark.parametrize("prec", [0, 3])
def test_planes_epilogue_distinguishes_truncation_from_rounding(prec):
    c = R.per_tile_cases(prec, 0)[0]
    ops = R.make_operands(c)
    z = R.reference_z(c, ops)
    f16 = R.prec_f16(prec)
    hi = R.rne16(z, f16)
    assert np.mean(hi != R.trunc16(z, f16)) > 0.1
    back = R.val16(hi, f16)                      # ties exist, and they went to the even pattern
    ulp = np.abs(R.val16(hi + 1, f16) - back)
    tie = (np.abs(z - back) * 2 == ulp) & (z != 0)
    assert tie.sum() > 10 and np.all(hi[tie] % 2 == 0)
    # hi + lo reproduce z where 2 x 11 (2 x 8) bits hold it, and hi is the nearest 16-bit number
    assert np.all(np.abs(z - R.val16(hi, f16)) <= np.abs(z - R.val16(R.trunc16(z, f16), f16)))


def test_rne16_ties_go_to_even():
    assert list(R.rne16(np.array([2049.0, 2051.0, 2050.0]), True)) == list(np.array([2048.0, 2052.0, 2050.0], dtype=np.float16).view(np.uint16))
    assert list(R.rne16(np.array([257.0, 259.0, 258.0]), False)) == [0x4380, 0x4382, 0x4381]
    assert R.rne16(np.array([np.nan]), False)[0] == 0x7FC0


def test_e2m1_helpers_round_trip():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((16, 128)) * 100).astype(np.float32)
    xh = x.astype(np.float16).astype(np.float64)
    packed, e8, dec = R._lo4_plane(x, xh)
    assert np.array_equal(R._decode_lo4(packed, e8, 128), dec)
    assert np.array_equal(R._q_e2m1(R.E2M1_GRID), R.E2M1_GRID) and R._q_e2m1(np.array([0.25, 0.75, 2.5, 7.0])).tolist() == [0.0, 1.0, 2.0, 6.0]
    w = rng.integers(-6, 7, (4, 64)).astype(np.float64)
    w[:, 0] = 6
    img = R._w4_image(w)
    assert np.array_equal(img[np.isin(np.abs(w), R.E2M1_GRID)], w[np.isin(np.abs(w), R.E2M1_GRID)])


def test_device_side_quantisers_of_the_old_tests_equal_the_numpy_ones():
    """tests/test_gpu_kernels.py evaluates _q_e2m1 and _lo4_plane on device tensors (its launches are large); here the same
    functions on CPU tensors against the numpy restatements, ties, saturation and the scale clamps included"""
    import torch
    import test_gpu_kernels as old
    rng = np.random.default_rng(1)
    t = np.concatenate([rng.standard_normal(4096) * 3, [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, 7.0, -0.25, -2.5, 0.0]])
    assert np.array_equal(old._q_e2m1(torch.from_numpy(t), torch).numpy(), R._q_e2m1(t))
    x = (rng.standard_normal((32, 192)) * np.exp(rng.standard_normal((32, 1)) * 4)).astype(np.float32)
    x[0, :64] = 0
    x[1, :64] = 1e-8
    xh = x.astype(np.float16)
    got = old._lo4_plane(torch.from_numpy(x), torch.from_numpy(xh), torch)
    want = R._lo4_plane(x, xh.astype(np.float64))
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)
    w = rng.standard_normal((8, 128))
    assert np.array_equal(old._w4_image(torch.from_numpy(w), torch).numpy(), R._w4_image(w))


# ---- walk planning ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [w[0] for w in R.WALKS])
def test_plan_walk_groups(walk):
    _, segs, want = next(w for w in R.WALKS if w[0] == walk)
    groups = R.seg_groups(segs)
    assert [(g["first_seg"], g["nshift"]) for g in groups] == want
    steps = R.walk_steps(groups)
    assert len(steps) == sum(s[3] for s in segs) // R.KBK
    assert sorted(s[3] for s in steps) == list(range(0, sum(s[3] for s in segs), R.KBK))    # every weight column once
    for g in groups:
        assert g["nshift"] == 1 or (g["dstep"] > 0 and g["dstep"] * (g["nshift"] - 1) <= 16)


def test_splitk_rule_yields_every_slice_count():
    assert sorted({R.splitk_slices(s) for s in range(8, 49)}) == list(range(2, 13))
    assert sorted({R.splitk_slices(s) for s in R.SPLITK_STEPS}) == list(range(2, 13))
    assert R.splitk_slices(94) == 24 and R.splitk_steps_per_slice(94) == 4 and R.splitk_steps_per_slice(100) == 5


# ---- every GPU case: precondition, kernel, cut classes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", R.PRECS)
def test_per_tile_and_v2_cases(prec):
    for epi in R._epis(prec):
        for c in R.per_tile_cases(prec, epi) + R.v2_cases(prec, epi):
            assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, CUS) == c.kernel, c
            if c.m_valid == c.rows:      # (the m_valid variants share the operands' distribution)
                _check_case(c)


@pytest.mark.parametrize("walk", [w[0] for w in R.WALKS])
def test_walk_cases(walk):
    for c in R.walk_cases(walk):
        assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, CUS) == c.kernel, c
        _check_case(c)


@pytest.mark.parametrize("steps", R.SPLITK_STEPS)
def test_splitk_cases(steps):
    for c in R.splitk_cases(steps):
        assert c.ksteps == steps and c.ksplit == R.splitk_slices(steps)
        assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, CUS, ksplit=c.ksplit) == c.kernel
        _check_case(c)


@pytest.mark.parametrize("name", R.SK_NAMES)
def test_stream_k_cases(name):
    c = R.sk_case(name, CUS)
    grid, lanes, cc = R.check_sk_claims(c, CUS)
    if name.startswith("lanes"):
        # heads and tails shorter than the three-stage ring, a head of S - 1 steps, a cut on a walk-group boundary and one
        # between the time offsets of a group
        assert {1, 2, 3, len(R.walk_steps(R.seg_groups(c.segs))) - 1} <= cc["heads"] and {1, 2, 3} <= cc["tails"]
        assert {"group_boundary", "between_offsets"} <= cc["kinds"]
    _check_case(c)


def test_stream_k_cases_cover_the_lane_counts_and_both_regimes():
    cs = [R.sk_case(n, CUS) for n in R.SK_NAMES]
    assert {c.expect["lanes"] for c in cs} == {1, 2, 4}
    assert {c.expect["regime"] for c in cs} == {1, 2}
    assert {c.expect["mf"] for c in cs} == {4, 8}


@pytest.mark.parametrize("name", R.P8_NAMES)
def test_p8_cases(name):
    c = R.p8_case(name, CUS)
    grid, lanes, cc = R.check_p8_claims(c, CUS)
    if name.startswith("dealt"):
        n = len(R.walk_tiles64(R.seg_groups(c.segs)))
        assert {2, n - 2} <= cc["positions"]     # cuts behind the first pair of K tiles and in front of the last
    _check_case(c)


@pytest.mark.parametrize("kernel,epi", [("tile", 0), ("tile", 1), ("v2", 0), ("v2", 1), ("sk", 0), ("sk", 1), ("p8", 0)])
def test_footprint_cases(kernel, epi):
    c = R.footprint_case(kernel, epi, CUS)
    assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, CUS, p8=c.p8) == c.kernel
    # the rows that depend on one element: a row per segment that holds its column
    assert R.footprint_rows(c, 0, 5, 0) == sorted({5 - s[2] for s in c.segs if s[0] == 0 and 0 <= 5 - s[2] < c.rows})
    assert R.footprint_rows(c, 0, -2, 0) == sorted({-2 - s[2] for s in c.segs if s[0] == 0 and -2 - s[2] >= 0})


def test_precondition_is_a_condition():
    c = R.Case("big", 3, 2, 128, 128, [(0, 512, 0, 512)], q=6, amp_x=15, amp_w=15, dens=1.0)
    with pytest.raises(AssertionError):
        R.check_precondition(c, R.make_operands(c))


# ---- the block-scaled modes: every quantiser returns the operands unchanged (asserted inside reference_z_mx), with the library's packers ----
@pytest.mark.parametrize("name", R.MX_NAMES)
def test_mx_cases(name):
    from helpers import pkg
    c = R.mx_case(name, CUS)
    assert R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, CUS, p8=c.p8) == c.kernel
    if not name.startswith("v2"):
        R.check_mx_claims(c, CUS)
    ops = R.make_mx_operands(c)
    z = R.reference_z_mx(c, ops, R.mx_pack(c, ops, pkg()))
    hi = R.rne16(z, True)
    assert np.mean(R.val16(hi, True) != z) > 0.2            # the fp16 plane rounds: the residual image has something to hold
    for g in ops["gmax"]:                                    # every group's exponent is fixed, and neighbouring groups differ
        e = (g >> 23) & 255
        assert set(np.unique(e)) == {127, 128} and np.any(e[1:] != e[:-1])
