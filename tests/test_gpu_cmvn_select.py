"""GPU tests of the affine map behind the row selection (csrc/cmvn_kernels.hip cmvn_apply_select, through xv_cmvn_apply_select), one
launch at a time: bit for bit the selected rows of the numpy restatement tests/cmvn_ref.py - and so of what apply-cmvn writes,
since selecting rows commutes with an element-wise map."""
import functools
import os
import re

import numpy as np
import pytest

import cmvn_ref as R
import helpers as H

pytestmark = pytest.mark.gpu
P = H.pkg()

# the kernel's rows per workgroup, read from its header: the utterance lengths straddle it and the launch takes several workgroups
RB = int(re.search(r"kCmvnSelectRows = (\d+);", open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "cmvn_kernels.h")).read()).group(1))
assert RB == 64
COLS = [1, 23, 40, 64, 65, 96]
# utterance 3 has nothing selected; utterance 5 has no statistics (utt_norm -1) and stands between two that are kept
ROWS = [1, 7, RB - 1, RB, RB, RB + 1, 4 * RB + 1, RB + 1]
NOTHING, LEFT_OUT = 3, 5
UTT_NORM = [0, 1, 0, 2, 2, -1, 1, 3]   # utterances 0 and 2, 1 and 6, 3 and 4 share a norm; norm 3 has one utterance


@functools.lru_cache(maxsize=None)
def case(cols):
    rng = np.random.default_rng(4000 + cols)
    mats = [rng.normal(20.0, 3.0, size=(r, cols)).astype(np.float32) for r in ROWS]
    # norms with variances: scales that are no powers of two, so that x * s is inexact and the sum rounds a second time
    stats = [R.stats(mats[0]) + R.stats(mats[2]), R.stats(mats[1]) + R.stats(mats[6]), R.stats(mats[3]) + R.stats(mats[4]), R.stats(mats[7])]
    norms = np.stack([R.cmvn_norm(st, norm_vars=True) for st in stats])
    off = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int32)
    sel_row, sel_utt = [], []
    for u, r in enumerate(ROWS):
        if u in (NOTHING, LEFT_OUT):
            continue
        keep = rng.random(r) < 0.6
        keep[rng.integers(0, r)] = True       # a voiced frame in every kept utterance
        if r > 16:
            keep[3:11] = False                    # a gap, and a run behind it
            keep[11:16] = True
        for t in np.flatnonzero(keep):
            sel_row.append(off[u] + t)
            sel_utt.append(u)
    if len(sel_row) % RB == 0:                    # the last workgroup is to be partly filled
        sel_row.pop()
        sel_utt.pop()
    sel_row, sel_utt = np.array(sel_row, np.int32), np.array(sel_utt, np.int32)
    full = np.concatenate([R.apply(x, norms[max(n, 0)]) for x, n in zip(mats, UTT_NORM)])
    return mats, norms, off, sel_row, sel_utt, full


@pytest.mark.parametrize("cols", COLS)
def test_selected_rows_equal_the_restatement_bit_for_bit(cols):
    mats, norms, off, sel_row, sel_utt, full = case(cols)
    assert len(sel_row) > 3 * RB                  # several workgroups, the last one partly filled
    assert len(sel_row) % RB != 0
    got = P.apply_cmvn_select(mats, norms, UTT_NORM, sel_row, sel_utt)
    want = full[sel_row]
    assert got.shape == want.shape == (len(sel_row), cols) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the expectation tells a contracted kernel apart: somewhere the fused multiply-add (the exact product of two floats is a
    # double; the sum is formed in fp64 and rounded once) gives another float than the product and the sum rounded in turn
    x = np.concatenate(mats)[sel_row].astype(np.float64)
    nm = norms[np.array(UTT_NORM)[sel_utt]].astype(np.float64)
    fused = (x * nm[:, 1, :] + nm[:, 0, :]).astype(np.float32)
    differ = int(np.count_nonzero(fused.view(np.uint32) != want.view(np.uint32)))
    print("cols %d: %d of %d elements differ under a fused multiply-add" % (cols, differ, want.size))
    assert differ > 0


@pytest.mark.parametrize("cols", [23, 65])
def test_every_row_selected_equals_apply_cmvn_itself(cols):
    mats, norms, off, _, _, _ = case(cols)
    kept = [u for u in range(len(ROWS)) if u != LEFT_OUT]
    sel_row = np.concatenate([np.arange(off[u], off[u + 1]) for u in kept]).astype(np.int32)
    sel_utt = np.concatenate([np.full(ROWS[u], u) for u in kept]).astype(np.int32)
    got = P.apply_cmvn_select(mats, norms, UTT_NORM, sel_row, sel_utt)
    whole = P.apply_cmvn([mats[u] for u in kept], norms, [UTT_NORM[u] for u in kept])
    want = np.concatenate(whole)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_an_empty_selection_and_bad_tables():
    mats, norms, off, sel_row, sel_utt, _ = case(23)
    none = P.apply_cmvn_select(mats, norms, UTT_NORM, [], [])
    assert none.shape == (0, 23)
    # the kernel trusts its tables, so the host checks them: a row outside its utterance, a row of the utterance without a norm
    for bad_row, bad_utt in (([int(off[1])], [0]), ([int(off[LEFT_OUT])], [LEFT_OUT]), ([0], [len(ROWS)]), ([-1], [0])):
        with pytest.raises(P.XvError):
            P.apply_cmvn_select(mats, norms, UTT_NORM, bad_row, bad_utt)
