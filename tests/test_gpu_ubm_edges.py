"""GPU tests of the GMM-UBM kernels (csrc/ubm_kernels.hip) at their edges: equal scores through the tile merge of the selection
kernel, gconsts of -infinity, frames whose scores are not finite (the rule of csrc/ubm.h: such a frame has no posterior) up to the
accumulators of the fused E-steps and the command line, every dimension at which the full-covariance kernel changes its
instantiation or stops padding, the two zeros, and deltas beyond order 3.  Exact against the float64 restatement (tests/ubm_ref.py)
on the integer models of test_gpu_ubm.py, bit for bit where two runs of the device are compared."""
import re

import numpy as np
import pytest

import gmm_classify_ref as C
import helpers as H
import ubm_ref as R
from oracle import kaldi_io as kio
from test_gpu_ubm import DB, FB, FRAMES, FT, GT, _sh, _split, integer_models, random_case

pytestmark = pytest.mark.gpu
P = H.pkg()
NS = [1, 3, 20, 63, 64]
G3 = 2 * GT + 5   # three tiles of the selection kernel, the last one of 5 Gaussians


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_posts(a, b):
    return len(a) == len(b) and all(np.array_equal(i0, i1) and np.array_equal(_bits(p0), _bits(p1)) for (i0, p0), (i1, p1) in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------- A: ties
def tied_model(B, G, D):
    """Gaussian g is a copy of Gaussian g % B of integer_models(B, D), gconst included: copies score the same to the bit"""
    base, _ = integer_models(B, D)
    src = np.arange(G) % B
    return {k: v[src].copy() for k, v in base.items()}


def _select_exactly(diag, G, D, ns, seed, inside_a_tie=False, distinct=None):
    """every T of FRAMES and every n: the selection and its log-likelihoods are the restatement's; -> the selections by (T, n).
    inside_a_tie: the n-th and the (n + 1)-th best are one score, so that the index alone decides the cut, in every frame ("all")
    or, where groups of 5 and 6 equals end at n in some frames, in at least one frame of every n ("some").  distinct: the number of
    different scores every frame must have (G: no ties)."""
    dm = P.Ubm.diag(**diag)
    rng = np.random.default_rng(seed)
    out, cut_inside = {}, {n: 0 for n in ns}
    for T in FRAMES:
        x = rng.integers(-4, 5, (T, D)).astype(np.float32)
        # every product and every partial sum is a multiple of 2^-12 below 2^12 in magnitude: 24 bits, whatever the order
        with np.errstate(invalid="ignore"):
            assert np.nan_to_num(R.diag_abs_terms(x, **diag), posinf=0.0).max() * 2.0 ** 12 < 2.0 ** 24
            ll = R.diag_loglikes(x, **diag)
        assert not np.isnan(ll).any()
        assert distinct is None or all(len(np.unique(row)) == distinct for row in ll), "the restatement has a tie of its own"
        srt = -np.sort(-ll, axis=1)
        for n in ns:
            want = R.gselect(ll, n)
            if inside_a_tie:
                inside = np.take_along_axis(ll, want[:, n - 1:n], 1)[:, 0] == srt[:, n]
                assert inside.all() or inside_a_tie == "some", (T, n)
                cut_inside[n] += int(inside.sum())
            (sel,), (got_ll,) = dm.gselect([x], n, return_loglikes=True)
            assert np.array_equal(sel, want), (T, n, "selection")
            assert np.array_equal(got_ll.astype(np.float64), np.take_along_axis(ll, want, 1)), (T, n, "log-likelihoods")
            out[T, n] = sel
    if inside_a_tie:
        print("frames (of %d) whose cut falls inside a group of equals, by n: %s" % (sum(FRAMES), cut_inside))
        assert all(cut_inside.values())
    return out


def test_every_score_five_or_six_times_over_three_tiles_selects_by_index():
    """B = 50 distinct Gaussians dealt over G = 2 GT + 5: a score occurs 5 or 6 times and its copies lie in all three tiles, so
    the running list meets equal scores from a later tile at every n, and the cut after n falls inside a group of equals."""
    B, D = 50, 23
    diag = tied_model(B, G3, D)
    got = _select_exactly(diag, G3, D, NS, seed=1, inside_a_tie="some", distinct=B)
    # a group comes out whole and ascending: g, g + B, g + 2 B, ...
    for sel in (got[T, 64] for T in FRAMES):
        assert np.all((sel[:, 1:5] - sel[:, :4]) == B) and np.all(sel[:, 0] < B)


def test_identical_gaussians_select_the_first_n():
    """B = 1: whatever a later tile offers equals what the list holds, and nothing is displaced"""
    got = _select_exactly(tied_model(1, G3, 23), G3, 23, NS, seed=2, inside_a_tie="all", distinct=1)
    for (T, n), sel in got.items():
        assert np.array_equal(sel, np.tile(np.arange(n, dtype=np.int32), (T, 1))), (T, n)


def test_a_tie_across_the_tile_seam_keeps_the_lower_index():
    """Gaussian GT, alone in the second tile, is a copy of Gaussian 0"""
    D = 23
    diag = tied_model(GT, GT + 1, D)
    got = _select_exactly(diag, GT + 1, D, [1, GT // 2], seed=3, distinct=GT)
    both = 0
    for (T, n), sel in got.items():
        for row in sel.tolist():
            if n == 1:
                assert row[0] != GT
            elif GT in row:   # right behind Gaussian 0
                assert row[row.index(GT) - 1] == 0 and row.index(GT) > 0
                both += 1
    assert both > 0, "no frame had the pair inside the selection"


def test_the_copied_gaussian_leads_on_its_own_mean_at_the_seam():
    """the seam at n = 1 where it decides: a frame at which the copied Gaussian beats every other, found on the restatement"""
    D = 23
    diag = tied_model(GT, GT + 1, D)
    rng = np.random.default_rng(4)
    x = rng.integers(-4, 5, (40 * FB, D)).astype(np.float32)
    ll = R.diag_loglikes(x, **diag)
    lead = np.nonzero(ll.argmax(1) == 0)[0]
    assert len(lead) > 0
    x = x[np.sort(np.concatenate([lead, np.arange(FB + 1)]))[:2 * FB + 3]]
    ll = R.diag_loglikes(x, **diag)
    assert R.diag_abs_terms(x, **diag).max() * 2.0 ** 12 < 2.0 ** 24
    assert (ll[:, 0] == ll.max(1)).any() and np.array_equal(ll[:, 0], ll[:, GT])
    dm = P.Ubm.diag(**diag)
    for n in (1, 2, GT // 2):
        want = R.gselect(ll, n)
        (sel,), (got_ll,) = dm.gselect([x], n, return_loglikes=True)
        assert np.array_equal(sel, want) and np.array_equal(got_ll.astype(np.float64), np.take_along_axis(ll, want, 1)), n
    assert not (dm.gselect([x], 1)[0] == GT).any()


def test_fewer_distinct_scores_than_n():
    """G = 65 copies of two Gaussians, n = 64: the better one's copies ascending, then the other's, one left out"""
    got = _select_exactly(tied_model(2, 65, 23), 65, 23, [64], seed=5, inside_a_tie="all", distinct=2)
    for sel in got.values():
        for row in sel.tolist():
            first = row[0] % 2
            k = 33 if first == 0 else 32
            assert row[:k] == list(range(first, 65, 2)) and row[k:] == list(range(1 - first, 65, 2))[:64 - k]


# ------------------------------------------------------------------------------------------------------------------- B: gconsts of -inf
def _with_minus_inf(model, which):
    out = {k: v.copy() for k, v in model.items()}
    out["gconsts"][np.asarray(which, int)] = -np.inf
    return out


def test_a_first_tile_of_minus_infinities_is_displaced():
    diag, _ = integer_models(G3, 23)
    got = _select_exactly(_with_minus_inf(diag, np.arange(GT)), G3, 23, NS, seed=6)
    for sel in got.values():
        assert sel.min() >= GT   # GT + 5 finite scores are left: more than any n


@pytest.mark.parametrize("keep", [[GT + 7], [5, GT + 7, 2 * GT + 1], [3, 90, GT, GT + 100, 2 * GT, 2 * GT + 4]])
def test_the_finite_few_come_first_then_minus_infinities_by_index(keep):
    diag, _ = integer_models(G3, 23)
    rest = np.setdiff1d(np.arange(G3), keep)
    dm_model = _with_minus_inf(diag, rest)
    k = len(keep)
    ns = [n for n in NS if n > k]
    got = _select_exactly(dm_model, G3, 23, ns, seed=7)
    dm = P.Ubm.diag(**dm_model)
    x = np.random.default_rng(7).integers(-4, 5, (FB + 1, 23)).astype(np.float32)
    for (T, n), sel in got.items():
        assert np.array_equal(np.sort(sel[:, :k], 1), np.tile(keep, (T, 1))), (T, n)
        assert np.array_equal(sel[:, k:], np.tile(rest[:n - k], (T, 1))), (T, n, "ascending index, across the tiles")
    (sel,), (ll,) = dm.gselect([x], 64, return_loglikes=True)
    assert np.all(np.isfinite(ll[:, :k])) and np.all(np.isneginf(ll[:, k:]))


def test_a_model_of_minus_infinities_selects_the_first_n():
    diag, _ = integer_models(G3, 23)
    got = _select_exactly(_with_minus_inf(diag, np.arange(G3)), G3, 23, NS, seed=8)
    for (T, n), sel in got.items():
        assert np.array_equal(sel, np.tile(np.arange(n, dtype=np.int32), (T, 1))), (T, n)
    dm = P.Ubm.diag(**_with_minus_inf(diag, np.arange(G3)))
    _, (ll,) = dm.gselect([np.ones((FB + 1, 23), np.float32)], 64, return_loglikes=True)
    assert np.all(np.isneginf(ll))


@pytest.mark.parametrize("min_post", [0.0, 0.025])
def test_minus_infinite_slots_have_posterior_zero_and_are_not_emitted(min_post):
    """The random model of test_gpu_ubm.py with every third gconst at -inf: every frame's selection mixes finite and -inf slots.
    The finite slots are within that file's bound of the restatement's posteriors, the log-sum is the finite slots' own."""
    G, n, D = GT + 1, 30, 23
    x, diag, full, ll_d, _ = random_case(G, D)
    dead = np.arange(1, G, 3)
    full_inf = _with_minus_inf(full, dead)
    fm = P.Ubm.full(**full_inf)
    sel = R.gselect(ll_d, n)
    is_dead = np.isin(sel, dead)
    assert np.all(is_dead.any(1)) and np.all((~is_dead).any(1)), "a frame does not mix"
    (post,), (got_ll,), (logsum,) = fm.post([x], [sel], min_post=min_post, return_details=True)
    with np.errstate(invalid="ignore"):
        ll = R.full_loglikes(x, sel=sel, **full_inf)
    eps = R.gamma(D * D + D + 1 + 3) * R.full_loglikes(x, sel=sel, absolute=True, **full)   # the finite gconsts: the slots that count
    assert np.all(np.isneginf(got_ll[is_dead])) and np.all(np.isneginf(ll[is_dead]))
    err = np.abs(got_ll[~is_dead] - ll[~is_dead])
    print("worst error / bound %.3g" % float((err / eps[~is_dead]).max()))
    assert np.all(err <= eps[~is_dead])
    e = np.where(is_dead, 0.0, eps).max(1)
    raw, want_logsum = R.posteriors(ll, 0.0)
    want, _ = R.posteriors(ll, min_post)
    assert not raw[is_dead].any() and not want[is_dead].any() and raw[~is_dead].min() > 2.0 ** -120
    # the log-sum of the finite slots alone, in float64
    alone = np.array([np.logaddexp.reduce(ll[t][~is_dead[t]]) for t in range(len(x))])
    np.testing.assert_allclose(want_logsum, alone, rtol=1e-14)
    assert np.all(np.abs(logsum - alone) <= e + 8 * 2.0 ** -24 * (np.abs(alone) + np.log(n) + 1.0))
    margin = np.expm1(2 * e)
    near = (np.abs(raw - min_post) <= margin[:, None] * min_post).any(1) if min_post else np.zeros(len(x), bool)
    print("frames excused by the min-post margin: %d of %d" % (int(near.sum()), len(near)))
    assert near.mean() <= 0.05
    for t in range(len(x)):
        idx, p = post[t]
        assert abs(float(p.sum()) - 1.0) < 1e-5 and not np.isin(idx, dead).any(), t
        if near[t]:
            continue
        keep = want[t] != 0.0
        assert idx.tolist() == sel[t][keep].tolist(), t
        assert np.all(np.abs(p - want[t][keep]) <= margin[t] * want[t][keep]), t


# ------------------------------------------------------------------------------------------------------------------- C: frames without a posterior
DEAD6 = [2, 5, 9, 13, 17, 20]


def _bad_batch(G, n, D, T, bad_pick, seed):
    """integer frames and picks of n of G Gaussians; -> (x, pick) good, (x, pick) with frame 1 picking bad_pick (gconsts of -inf)
    and frames FB - 1 and FB holding a NaN"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (T, D)).astype(np.float32)
    pick = np.stack([rng.permutation(G)[:n] for _ in range(T)]).astype(np.int32)
    assert np.all((~np.isin(pick, bad_pick)).any(1)), "a good frame has no finite slot"
    xb, pb = x.copy(), pick.copy()
    pb[1] = bad_pick
    xb[FB - 1, D // 2] = np.nan
    xb[FB, :] = np.nan
    return (x, pick), (xb, pb)


@pytest.mark.parametrize("min_post", [0.0, 0.025])
def test_frames_without_a_finite_score_come_back_empty_and_disturb_nothing(min_post):
    G, n, D, T = 21, 6, 23, 2 * FB + 3
    _, full = integer_models(G, D)
    fm = P.Ubm.full(**_with_minus_inf(full, DEAD6))
    (x, pick), (xb, pb) = _bad_batch(G, n, D, T, DEAD6, seed=11)
    bad = [1, FB - 1, FB]
    (post,), (ll,), (logsum,) = fm.post([x], [pick], min_post=min_post, return_details=True)
    (post_b,), (ll_b,), (logsum_b,) = fm.post([xb], [pb], min_post=min_post, return_details=True)
    for t in bad:
        idx, p = post_b[t]
        assert len(idx) == 0 and len(p) == 0, (t, idx, p)
    assert np.isneginf(logsum_b[1]) and np.all(np.isneginf(ll_b[1]))
    assert np.isnan(logsum_b[FB - 1]) and np.isnan(logsum_b[FB]) and np.all(np.isnan(ll_b[[FB - 1, FB]]))
    ok = np.setdiff1d(np.arange(T), bad)
    assert np.all(np.isfinite(logsum[ok]))
    assert np.array_equal(_bits(ll_b[ok]), _bits(ll[ok])) and np.array_equal(_bits(logsum_b[ok]), _bits(logsum[ok]))
    assert _same_posts([post_b[t] for t in ok], [post[t] for t in ok])
    # the restatement says the same of the bad frames
    with np.errstate(invalid="ignore"):
        want, want_logsum = R.posteriors(ll_b.astype(np.float64), min_post)
    assert not want[bad].any() and np.isneginf(want_logsum[1]) and np.all(np.isnan(want_logsum[[FB - 1, FB]]))


def test_a_nan_frame_is_selected_alone():
    """the selection of a frame that holds a NaN is n distinct Gaussians, and its block's other frames do not notice"""
    n, D, T = 20, 23, 2 * FB + 3
    diag, _ = integer_models(G3, D)
    dm = P.Ubm.diag(**diag)
    x = np.random.default_rng(12).integers(-4, 5, (T, D)).astype(np.float32)
    xb = x.copy()
    xb[FB + 2, 5] = np.nan
    xb[3, :] = np.nan
    (sel,), (ll,) = dm.gselect([x], n, return_loglikes=True)
    (sel_b,), (ll_b,) = dm.gselect([xb], n, return_loglikes=True)
    ok = np.setdiff1d(np.arange(T), [3, FB + 2])
    assert np.array_equal(sel_b[ok], sel[ok]) and np.array_equal(_bits(ll_b[ok]), _bits(ll[ok]))
    for t in (3, FB + 2):
        assert len(set(sel_b[t].tolist())) == n and sel_b[t].min() >= 0 and sel_b[t].max() < G3, sel_b[t]
        assert np.all(np.isnan(ll_b[t]))


def _acc_bits(acc):
    return [np.ascontiguousarray(a, np.float64).view(np.uint64) for a in acc.get()]


@pytest.mark.parametrize("kind", ["full", "diag"])
def test_the_fused_e_steps_leave_frames_without_a_posterior_out(kind):
    """2 FB + 3 frames of which one holds a NaN and one selects gconsts of -inf only: occupancies, means and (co)variances are those
    of the call without the two, bit for bit, and the log-sums of the others too.  (Before the rule of csrc/ubm.h such a frame
    carried NaN weights into every Gaussian it had selected.)"""
    G, n, D, T = 9, 4, 17, 2 * FB + 3
    dead = [1, 3, 6, 8]
    diag, full = integer_models(G, D)
    rng = np.random.default_rng(13)
    x = rng.integers(-2, 3, (T, D)).astype(np.float32)
    live = np.setdiff1d(np.arange(G), dead)
    # a live Gaussian in a slot of its own choosing, three of the other eight around it: most frames mix live and dead slots
    gs = np.stack([rng.permutation(np.concatenate([[g], rng.permutation(np.setdiff1d(np.arange(G), [g]))[:n - 1]]))
                   for g in rng.choice(live, T)]).astype(np.int32)
    nan_frame, inf_frame = 1, FB
    x[nan_frame, D - 1] = np.nan
    gs[inf_frame] = dead
    ok = np.setdiff1d(np.arange(T), [nan_frame, inf_frame])
    assert np.all((~np.isin(gs[ok], dead)).any(1)), "a good frame has no finite slot"
    if kind == "full":
        model = P.Ubm.full(**_with_minus_inf(full, dead))
        make = lambda: P.FgmmAccumulator(G, D, "mvw")
    else:
        model = P.Ubm.diag(**_with_minus_inf(diag, dead))
        make = lambda: P.DgmmAccumulator(G, D, "mvw")
    with_bad, without = make(), make()
    logsum_b = with_bad.accumulate_gselect(model, x, gs)
    logsum = without.accumulate_gselect(model, x[ok], gs[ok])
    got, want = with_bad.get(), without.get()
    for name, a, b in zip(("occupancy", "mean", "(co)variance"), got, want):
        print("%s %s: NaN in %d of %d sums, largest difference %.3g" % (kind, name, int(np.isnan(a).sum()), a.size, float(np.nanmax(np.abs(a - b)))))
    assert np.isnan(logsum_b[nan_frame]) and np.isneginf(logsum_b[inf_frame])
    assert np.array_equal(_bits(logsum_b[ok]), _bits(logsum)) and np.all(np.isfinite(logsum))
    for name, a, b in zip(("occupancy", "mean", "(co)variance"), _acc_bits(with_bad), _acc_bits(without)):
        assert np.array_equal(a, b), (kind, name)
    assert want[0].sum() == pytest.approx(len(ok), rel=1e-6)   # every good frame's posteriors add up to 1


def test_gselect_to_post_writes_an_empty_frame_for_a_nan_frame(tmp_path):
    G, D, n, T, bad = 12, 10, 5, 20, 7
    w, means, b, ic = R.random_full_model(41, G, D, spread=1.0)
    (tmp_path / "final.ubm").write_bytes(R.full_gmm_bytes(w, b, ic, True))
    x = R.frames_around(42, means, T, noise=1.0)
    rng = np.random.default_rng(43)
    gs = np.stack([rng.permutation(G)[:n] for _ in range(T)]).astype(np.int32)
    xb = x.copy()
    xb[bad, 2] = np.nan
    keep = np.arange(T) != bad
    outs = {}
    for name, feats, sel in (("bad", xb, gs), ("good", x[keep], gs[keep])):
        kio.write_ark_matrices(str(tmp_path / (name + ".ark")), [("utt", feats)])
        (tmp_path / (name + ".gs")).write_bytes(R.gselect_table_bytes([("utt", sel)], True))
        r = _sh("fgmm-global-gselect-to-post --min-post=0.025 %s/final.ubm ark:%s/%s.ark ark:%s/%s.gs ark,t:-" % (tmp_path, tmp_path, name, tmp_path, name))
        assert r.returncode == 0, r.stderr
        assert r.stdout.startswith(b"utt ") and r.stdout.endswith(b"\n") and r.stdout.count(b"\n") == 1
        outs[name] = re.findall(rb"\[[^\]]*\]", r.stdout)
        if name == "bad":
            (key, frames), = R.read_post_table(r.stdout)
            assert key == "utt" and len(frames) == T and frames[bad] == [] and all(frames[:bad] + frames[bad + 1:])
    assert len(outs["bad"]) == T and len(outs["good"]) == T - 1
    assert outs["bad"][bad] == b"[ ]"
    assert outs["bad"][:bad] + outs["bad"][bad + 1:] == outs["good"]
    assert all(len(f.split()) > 2 for f in outs["good"])


# ------------------------------------------------------------------------------------------------------------------- D: dimension edges
D_FULL = [31, 32, 33, 63, 64, 65, 95, 96]   # NC = 4 up to 32, 8 up to 64, 12 up to 96; 32, 64 and 96 fill the LDS image without padding


def _full_scores_exactly(G, n, D, T, rng, every_gaussian=False):
    _, full = integer_models(G, D)
    fm = P.Ubm.full(**full)
    x = rng.integers(-2, 3, (T, D)).astype(np.float32)
    if every_gaussian:
        pick = np.stack([rng.permutation(G) for _ in range(T)]).astype(np.int32)
    else:   # popular Gaussians, repeats across frames, any order inside a frame
        pick = np.stack([rng.permutation(G)[:n] for _ in range(T)]).astype(np.int32)
        pick[::3, 0] = pick[0, 0]
    # every product and every partial sum is a multiple of 2^-10 below 2^14 in magnitude: 24 bits, whatever the order
    assert R.full_loglikes(x, sel=pick, absolute=True, **full).max() * 2.0 ** 10 < 2.0 ** 24
    want = R.full_loglikes(x, sel=pick, **full)
    _, (got,), _ = fm.post([x], [pick], return_details=True)
    assert np.array_equal(got.astype(np.float64), want), (G, n, D, T)


@pytest.mark.parametrize("D", D_FULL)
def test_full_scores_are_exact_at_every_dimension_edge(D):
    rng = np.random.default_rng(100 + D)
    for T in FRAMES:
        _full_scores_exactly(21, 20, D, T, rng)


@pytest.mark.parametrize("D", [32, 64, 96])
def test_full_scores_are_exact_with_64_slots_where_the_image_has_no_padding(D):
    rng = np.random.default_rng(200 + D)
    for T in FRAMES:
        _full_scores_exactly(G3, 64, D, T, rng)


@pytest.mark.parametrize("D", [32, 64, 96])
def test_every_instantiation_is_exact_with_two_workgroups_per_gaussian(D):
    T, G = 8 * FB + 3, 20
    assert _split(T, G, G) == 2 and T > 2 * FT
    _full_scores_exactly(G, G, D, T, np.random.default_rng(300 + D), every_gaussian=True)


@pytest.mark.parametrize("G,n,D", [(GT + 1, 20, 32), (GT + 1, 20, 33), (GT + 1, 20, 64), (GT + 1, 20, 95), (GT + 1, 20, 96), (G3, 64, 96)])
def test_selection_is_exact_at_the_dimension_edges(G, n, D):
    """(2 GT + 5, 64, 96) is the launch with the most LDS: 39040 B static and 24576 B of frames"""
    diag, _ = integer_models(G, D)
    _select_exactly(diag, G, D, [n], seed=400 + G + D, distinct=G)


# ------------------------------------------------------------------------------------------------------------------- E: the two zeros
def _zero_pair_model(G, twin, D=3):
    """Gaussian 0 scores -0.0 on a frame of zeros (gconst -0.0, negative means_invvars), Gaussian `twin` is the same with gconst
    +0.0 and scores +0.0; the others score -1 - g"""
    gc = -1.0 - np.arange(G, dtype=np.float32)
    gc[0], gc[twin] = -0.0, 0.0
    assert np.signbit(gc[0]) and not np.signbit(gc[twin])
    return dict(gconsts=gc, means_invvars=np.full((G, D), -1.0, np.float32), inv_vars=np.ones((G, D), np.float32))


@pytest.mark.parametrize("G,twin", [(2, 1), (GT + 2, GT)])
def test_the_two_zeros_are_one_score_and_the_lower_index_comes_first(G, twin):
    model = _zero_pair_model(G, twin)
    dm = P.Ubm.diag(**model)
    for T in FRAMES:
        x = np.zeros((T, 3), np.float32)
        ll = R.diag_loglikes(x, **model)
        assert np.all(ll[:, 0] == 0.0) and np.all(ll[:, twin] == 0.0) and np.all(ll[:, 1:twin] < 0.0) and np.all(ll[:, twin + 1:] < 0.0)
        for n in (1, 2):
            want = R.gselect(ll, n)
            assert want[0].tolist() == [0, twin][:n]
            (sel,), (got_ll,) = dm.gselect([x], n, return_loglikes=True)
            assert np.array_equal(sel, want), (T, n, sel[0].tolist())
            assert np.all(got_ll == 0.0), (T, n)   # == : either zero


def test_zero_scores_rerank_by_index():
    """Gaussians with gconsts -0.0 and +0.0 and nothing else on a frame of zeros: the full-covariance kernel adds its sums, which
    are +0.0, to the gconst, so both score +0.0 (no score of that kernel is -0.0) and the lower index comes first"""
    G, D = 4, 5
    full = {k: v.copy() for k, v in C.integer_full_model(G, D).items()}
    full["gconsts"][:] = [-3.0, 0.0, -1.0, -0.0]
    full["gconsts"][3] = -0.0
    assert np.signbit(full["gconsts"][3])
    fm = P.Ubm.full(**full)
    for T in FRAMES:
        x = np.zeros((T, D), np.float32)
        pre = np.tile(np.array([3, 0, 1, 2], np.int32), (T, 1))
        scores = R.full_loglikes(x, sel=pre, **full)
        want_idx, want_ll = C.rerank(scores, pre, 4)
        assert want_idx[0].tolist() == [1, 3, 2, 0]
        (idx,), (ll,) = fm.rerank([x], [pre], 4, return_loglikes=True)
        assert np.array_equal(idx, want_idx) and np.all(ll.astype(np.float64) == want_ll), T


# ------------------------------------------------------------------------------------------------------------------- F: deltas
@pytest.mark.parametrize("window", [1, 3])
@pytest.mark.parametrize("order", [4, 8])
def test_deltas_of_order_four_and_eight_equal_the_restatement_bit_for_bit(order, window):
    rng = np.random.default_rng(100 * order + window)
    for width in (1, 96):
        mats = [rng.normal(0.0, 10.0, size=(t, width)).astype(np.float32) for t in (1, 2, DB + 1)]
        for truncate in sorted({0, width - 1}):
            got = P.add_deltas(mats, order=order, window=window, truncate=truncate)
            for x, g in zip(mats, got):
                want = R.add_deltas(x, order, window, truncate)
                assert g.shape == want.shape == (len(x), (order + 1) * (truncate or width))
                assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (x.shape, width, truncate)
