"""CPU tests of the GEMM launch planner (csrc/gemm_plan.cc) through xv_plan_gemm: which kernel a launch runs, its grid, lanes and
LDS, and the K-walk groups, at several CU counts and under every knob - against the restatement of the launch rules in
gemm_exact_ref.py (select_kernel, sk_partition, p8_partition, _sk_lds, seg_groups), which was written from the rules and is compared
with the device bit for bit at 256 CUs by test_gpu_gemm_exact.py.  No device: the descriptors carry distinct dummy addresses, which
the planner only compares and tests for null."""
import re

import pytest

import gemm_exact_ref as R
from helpers import pkg as _pkg

CUS = (7, 8, 16, 64, 120, 256, 304)
XV_ERR_DEVICE, XV_ERR_ARG = 3, 4
MAX_LDS = 160 * 1024          # the LDS of a gfx950 CU


def desc_of(c):
    """The descriptor test_gpu_gemm_exact.py builds for case c, with made-up addresses (one 1 MiB window per source)."""
    P = _pkg()
    d = P.GemmDesc()
    d.precision, d.epilogue, d.nseg = c.prec, c.epi, len(c.segs)
    mx, mx2 = R.prec_mx(c.prec), R.prec_mx2(c.prec)
    for j, (si, ld, shift, klen) in enumerate(c.segs):
        base = 0x10000000 + si * 0x100000
        d.seg[j].hi = base
        d.seg[j].lo = base + 0x40000 if R.prec_x_planes(c.prec) == 2 else None
        d.seg[j].ld, d.seg[j].row_shift, d.seg[j].k_len = c.src_ld[si], shift, klen
        if mx:
            d.seg[j].gmax = base + 0x80000
        if mx2:
            d.seg[j].lo4, d.seg[j].lo4_scale = base + 0xA0000, base + 0xC0000
    d.w_hi, d.ldw = 0x20000000, c.ldw
    d.w_lo = 0x20100000 if (R.prec_w_planes(c.prec) == 2 and not mx) else None
    if mx:
        d.w4, d.ldw4, d.w4_scale = 0x20200000, c.K // 128 * 64, 0x20300000
    if mx2:
        d.w4b, d.ldw4b, d.w4b_scale = 0x20400000, (2 * c.K if c.p8 else c.K // 2), 0x20500000
    d.rows, d.n_pad = c.rows, c.n_pad
    d.bias, d.scale, d.offset = 0x30000000, 0x30010000, 0x30020000
    d.relu, d.bn, d.hip_stream, d.p8, d.ksplit = int(c.relu), int(c.bn), None, c.p8, c.ksplit
    if c.epi == R.EPI_ACT:
        d.out_hi, d.ldo = 0x40000000, c.ldo
        if R.prec_emits_lo4(c.prec):
            d.out_lo4, d.out_lo4_scale = 0x41000000, 0x42000000
        elif R.prec_x_planes(c.prec) == 2:
            d.out_lo = 0x43000000
    elif c.epi == R.EPI_F32:
        d.out_f32, d.ldf, d.m_valid = 0x44000000, c.ldf, c.m_valid
    else:
        d.partial, d.ldp, d.grp_range = 0x45000000, c.ldp, 0x46000000
    return d


def kernel_of(plan):
    return None if plan.refused else plan.kernel.decode()


def _plain_cases():
    out = []
    for prec in R.PRECS:
        for epi in R._epis(prec):
            out += R.per_tile_cases(prec, epi) + R.v2_cases(prec, epi)
    for w in R.WALKS:
        out += R.walk_cases(w[0])
    for steps in R.SPLITK_STEPS:
        out += R.splitk_cases(steps)
    return out


def _shaped_cases(cus):
    """the cases whose shapes follow a CU count, built for that count.  Not every case exists at every count: the rule for launches
    between the regimes needs at least four 512-row tiles per XCD block that are still fewer than the block's workgroups, i. e. more
    than 160 CUs for the five column tiles of the regime2 cases - the search of gemm_exact_ref.py then finds no row count and says so"""
    out = []
    for make, names in ((R.sk_case, R.SK_NAMES), (R.p8_case, R.P8_NAMES), (R.mx_case, R.MX_NAMES)):
        for n in names:
            try:
                out.append(make(n, cus))
            except AssertionError as e:
                assert cus != 256 and str(e).startswith(("no row count reaches regime 2", "no launch reaches the cut classes")), (n, cus, e)
    return out


PLAIN = _plain_cases()


def check_plan(c, cus):
    """kernel, grid, lanes, LDS and workspace of the plan of case c on cus CUs; returns the kernel name"""
    P = _pkg()
    plan = P.plan_gemm(desc_of(c), cus)
    want = R.select_kernel(c.prec, c.epi, c.m_tiles, c.n_tiles, c.segs, cus, p8=c.p8, ksplit=c.ksplit)
    if c.p8 and cus < 8:          # no XCD block gets a workgroup
        want = None
    got = kernel_of(plan)
    assert got == want, (c, cus, got, want)
    if got is None:
        return None
    assert 0 < plan.lds_bytes <= MAX_LDS and plan.grid_x >= 1 and plan.grid_y == max(1, c.ksplit)
    m = re.match(r"tdnn_gemm_kernel_sk<\w+,\w+,(\d)>", got)
    if m:
        mf = int(m.group(1))
        grid, lanes, _ = R.sk_partition(c.prec, mf, c.m_tiles, c.n_tiles, c.segs, cus)
        assert (plan.grid_x, plan.lanes, plan.mf, plan.block) == (grid, lanes, mf, 512), (c, cus)
        assert plan.lds_bytes == R._sk_lds(c.prec, mf)
        assert plan.sk_mtiles == c.rows // (64 * mf) and plan.groups_per_xcd == grid // 8 // lanes
        assert plan.workspace_bytes == grid * 64 * mf * R.KBN * 4        # a slot of raw fp32 accumulators per workgroup
    elif "_p8<" in got:
        grid, lanes, _ = R.p8_partition(c.prec, c.m_tiles, c.n_tiles, c.segs, cus)
        assert (plan.grid_x, plan.lanes, plan.block) == (grid, lanes, 512), (c, cus)
        groups = R.seg_groups(c.segs)
        assert plan.p8_ktiles == sum((g["ksteps"] >> 1) * g["nshift"] for g in groups)
        assert plan.p8_ktiles_lo == (sum((g["ksteps"] // 4 >> 1) * g["nshift"] for g in groups) if R.prec_mx2(c.prec) else 0)
        assert plan.sk_mtiles == c.m_tiles // 2 and plan.groups_per_xcd == grid // 8 // lanes and plan.p8_whole == 0
        assert plan.workspace_bytes == grid * 256 * 256 * 4
    else:
        assert plan.workspace_bytes == 0 and plan.lanes == 0
    return got


@pytest.mark.parametrize("cus", CUS)
def test_kernel_grid_lanes_and_lds_follow_the_launch_rules(cus):
    names = [check_plan(c, cus) for c in PLAIN + _shaped_cases(256)]
    if cus >= 8 and cus != 256:       # where the rules admit a persistent kernel at all: also the shapes made for this count
        names += [check_plan(c, cus) for c in _shaped_cases(cus)]
    if cus >= 8:
        for c in _shaped_cases(cus):
            assert kernel_of(_pkg().plan_gemm(desc_of(c), cus)) == c.kernel, (c, cus)
        for v in ("_sk<", "_p8<", "_v2<", "kernel<"):      # every family is planned at this CU count
            assert any(n and v in n for n in names), v


def test_seven_cus_leave_no_persistent_kernel():
    for c in _shaped_cases(256):
        got = kernel_of(_pkg().plan_gemm(desc_of(c), 7))
        if c.p8:
            assert got is None, c
        else:
            assert got is not None and ("_v2<" in got or got.startswith("tdnn_gemm_kernel<")), (c, got)


def _groups(plan, first, n):
    return [{k: getattr(plan.grp[first + i], k) for k in ("ld", "ksteps", "nshift", "shift0", "dstep", "wcol0", "wstride", "ld4s")}
            for i in range(n)]


@pytest.mark.parametrize("walk", [w[0] for w in R.WALKS])
def test_first_walk_groups(walk):
    _, segs, formed = next(w for w in R.WALKS if w[0] == walk)
    want = R.seg_groups(segs)
    assert [(g["first_seg"], g["nshift"]) for g in want] == formed
    for c in R.walk_cases(walk):
        plan = _pkg().plan_gemm(desc_of(c), 256)
        assert not plan.refused and plan.ngrp == len(want) and plan.ngrp_lo == 0 and plan.lo_ksteps == 0
        for got, g in zip(_groups(plan, 0, plan.ngrp), want):
            assert got == dict(ld=segs[g["first_seg"]][1], ksteps=g["ksteps"], nshift=g["nshift"], shift0=g["shift0"], dstep=g["dstep"],
                               wcol0=g["wcol0"], wstride=g["wstride"], ld4s=0), (c, got, g)


@pytest.mark.parametrize("name", [n for n in R.MX_NAMES if n.endswith("fp16mx2")])
def test_second_walk_groups(name):
    c = R.mx_case(name)
    plan = _pkg().plan_gemm(desc_of(c), 256)
    assert kernel_of(plan) == c.kernel
    first, second = _groups(plan, 0, plan.ngrp), _groups(plan, plan.ngrp, plan.ngrp_lo)
    want = R.seg_groups(c.segs)
    assert plan.ngrp == plan.ngrp_lo == len(want)
    for a, b, g in zip(first, second, want):
        assert (a["ksteps"], a["nshift"], a["wcol0"]) == (g["ksteps"], g["nshift"], g["wcol0"])
        assert b == dict(a, ld=a["ld"] // 4, ksteps=a["ksteps"] // 4, ld4s=R.lo4_scale_pitch(a["ld"])), (a, b)
    assert plan.lo_ksteps == sum(b["ksteps"] * b["nshift"] for b in second) == c.ksteps // 4


def _refused(d, status, message):
    """the planner refuses the descriptor, and so does the launch entry - before it looks for a device - in its own words"""
    P = _pkg()
    plan = P.plan_gemm(d, 256)
    assert plan.refused and plan.kernel == b""
    with pytest.raises(P.XvError) as e:
        P.kernel_tdnn_gemm(d)
    assert e.value.status == status and message in str(e.value), str(e.value)


def test_refusals():
    base = R.v2_cases(3, 0)[0]
    for nseg in (0, 9):
        d = desc_of(base)
        d.nseg = nseg
        _refused(d, XV_ERR_ARG, "xv_kernel_tdnn_gemm: bad geometry")
    for name in ("v2_fp16mx", "v2_fp16mx2", "v2_fp16mxe"):
        d = desc_of(R.mx_case(name))
        d.ksplit = 2
        _refused(d, XV_ERR_ARG, "split-K needs XV_PREC_BF16X3 .. XV_PREC_FP16X3, epilogue 0 or 1 and no p8")
        d = desc_of(R.mx_case(name))
        d.epilogue, d.out_f32, d.ldf, d.m_valid = R.EPI_F32, 0x44000000, 260, 768
        _refused(d, XV_ERR_DEVICE, "tdnn_gemm launch: invalid argument")
    for c in (R.v2_cases(R.PREC_FP16X3E, 0)[0], R.mx_case("v2_fp16mxe")):
        for drop in ("out_lo4", "out_lo4_scale"):
            d = desc_of(c)
            assert kernel_of(_pkg().plan_gemm(d, 256)) == c.kernel
            setattr(d, drop, None)
            _refused(d, XV_ERR_DEVICE, "tdnn_gemm launch: invalid argument")
    p8 = R.p8_case("min_act")
    odd_rows = R.Case("p8_odd_rows", 2, 0, 3 * R.KBM, 256, R.SEGS_P8, p8=1)
    odd_tiles = R.Case("p8_odd_tiles", 2, 0, 256, 256, [(0, 64, 0, 64), (1, 128, 1, 128)], p8=1)      # 1 + 2 K tiles
    mx2 = R.mx_case("p8_small_fp16mx2")
    mx2_ld = R.Case("p8_mx2_ld", 7, 0, mx2.rows, mx2.n_pad, [(0, 320, -2, 256), (0, 320, 2, 256)], p8=1)
    assert kernel_of(_pkg().plan_gemm(desc_of(p8), 256)) == p8.kernel and kernel_of(_pkg().plan_gemm(desc_of(mx2), 256)) == mx2.kernel
    for c in (odd_rows, odd_tiles, mx2_ld):
        _refused(desc_of(c), XV_ERR_ARG, "xv_kernel_tdnn_gemm: p8 needs XV_PREC_FP16, XV_PREC_FP16MX or XV_PREC_FP16MX2")


def _planned(policy, cases=None):
    P = _pkg()
    return [(c, P.plan_gemm(desc_of(c), 256, policy=policy)) for c in (PLAIN + _shaped_cases(256) if cases is None else cases)]


def test_knob_gemm_variant():
    """knobs.h / gemm_plan.h: 1 = the 128-row kernel (the block-scaled modes have none: they keep the 256-row one), 2 = the per-tile
    kernels instead of the persistent grid, 4 = stream-K wherever it applies; p8 and split-K are the caller's choice, not the knob's"""
    default = {c.name: kernel_of(p) for c, p in _planned(dict())}
    for c, p in _planned(dict(variant=1)):
        k = kernel_of(p)
        if c.p8 or c.ksplit > 1:
            assert k == default[c.name]
        elif R.prec_mx(c.prec):
            assert "_v2<" in k, (c, k)
        else:
            assert k.startswith("tdnn_gemm_kernel<"), (c, k)
    for c, p in _planned(dict(variant=2)):
        k = kernel_of(p)
        assert "_sk<" not in k and (k == default[c.name] or "_sk<" in default[c.name]), (c, k)
    wide = R.sk_case("sk8_fp16_act")
    short_k = R.Case("short_k", R.PREC_FP16, 0, wide.rows, wide.n_pad, R.SEGS_SK8)       # single pass, 8 K steps: per tile by default
    assert [kernel_of(p) for _, p in _planned(dict(), [short_k])] == ["tdnn_gemm_kernel_v2<fp16,act>"]
    assert [kernel_of(p) for _, p in _planned(dict(variant=4), [short_k])] == ["tdnn_gemm_kernel_sk<fp16,act,8>"]
    assert [kernel_of(p) for _, p in _planned(dict(variant=3), [short_k])] == ["tdnn_gemm_kernel_v2<fp16,act>"]      # not a value: the default


def test_knob_sk_mf():
    seen4 = 0
    for c, p in _planned(dict(sk_mf=4)):
        k = kernel_of(p)
        assert k is None or ",8>" not in k, (c, k)
        seen4 += k is not None and ",4>" in k
        if R.prec_mx(c.prec) and not c.p8:       # 512-row stream-K tiles or the 256-row kernel, nothing else
            assert "_v2<" in k
    assert seen4 >= 3


@pytest.mark.parametrize("cap", (1, 2))
def test_knob_sk_lanes(cap):
    wide = 0
    for c, p in _planned(dict(sk_lanes=cap), [R.sk_case(n) for n in R.SK_NAMES]):
        assert "_sk<" in kernel_of(p) and p.lanes <= cap and c.n_tiles % p.lanes == 0 and p.grid_x == 8 * p.lanes * p.groups_per_xcd, c
        wide += c.expect["lanes"] > cap and p.lanes == cap
    assert wide >= 3


def test_knob_gemm_stagger():
    """the stagger window: gemm_stagger percent of the modelled tile time (K steps x (400 + 600 per pass) + 14000 cycles), in units of
    2048 cycles, for launches of more than two workgroups per CU"""
    P = _pkg()
    c = R.v2_cases(3, 0)[3]          # 11 x 3 tiles of 256 rows: 48 workgroups
    model = c.ksteps * (400 + 600 * R.prec_passes(c.prec)) + 14000
    for pct in (0, 85, 100):
        assert P.plan_gemm(desc_of(c), 16, policy=dict(stagger_pct=pct)).stagger_units == model * pct // 100 // 2048
    assert P.plan_gemm(desc_of(c), 16).stagger_units == model * 85 // 100 // 2048 > 0
    assert P.plan_gemm(desc_of(c), 24).stagger_units == 0 and P.plan_gemm(desc_of(c), 24).grid_x == 48


def test_planner_sweep_under_asan_ubsan():
    """`host_selftest gemm_plan` (make sanitize: plain g++ with AddressSanitizer + UBSan, its own main): PlanGemm and the
    applicability predicates over shapes x modes x CU counts x knobs, valid or not, stay inside GemmArgs"""
    import os
    import subprocess

    import helpers as H
    csrc = os.path.join(H.ROOT, H.PKG_NAME, "csrc")
    r = subprocess.run(["make", "-C", csrc, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "host_selftest_asan"), "gemm_plan"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and "host_selftest: gemm_plan ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
