"""The numpy restatement of the GMM classifiers (tests/gmm_classify_ref.py) against cases worked by hand, and the library's two
host-only entry points (xv_vad_from_frame_likes, xv_merge_vads) against it.  No GPU."""
import os

import numpy as np
import pytest

import gmm_classify_ref as C
import helpers as H

INF = float("inf")
# the restatement's twin: the same semantics in words, next to the code that implements them
HEADER = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "gmm_classify.h")).read()


def test_both_statements_say_that_parity_with_kaldi_is_unpinned():
    for text in (HEADER, C.__doc__):
        assert "parity with a Kaldi binary is" in text and "not pinned" in " ".join(text.split())
        for source in ("gmm/full-gmm.cc", "fgmmbin/fgmm-gselect.cc", "fgmmbin/fgmm-global-get-frame-likes.cc",
                       "ivectorbin/compute-vad-from-frame-likes.cc", "ivectorbin/merge-vads.cc"):
            assert source in text, source
    # the order the header states is the one the restatement ranks by
    assert "score" in HEADER and "then Gaussian ascending, then slot ascending" in " ".join(HEADER.replace("//", "").split())


def test_ranking_orders_by_score_then_gaussian_then_slot():
    #            slot:  0     1     2     3     4
    ll = np.array([[1.0, 3.0, 3.0, -2.0, 3.0]], np.float32)
    pre = np.array([[7, 9, 4, 1, 4]], np.int32)
    # three scores of 3: Gaussian 4 (slot 2), Gaussian 4 again (slot 4: the later slot), Gaussian 9; then 1.0, then -2.0
    idx, out = C.rerank(ll, pre, 5)
    assert idx.tolist() == [[4, 4, 9, 7, 1]]
    assert out.tolist() == [[3.0, 3.0, 3.0, 1.0, -2.0]]
    idx, out = C.rerank(ll, pre, 2)
    assert idx.tolist() == [[4, 4]] and out.tolist() == [[3.0, 3.0]]
    idx, _ = C.rerank(ll, pre, 4)
    assert idx.tolist() == [[4, 4, 9, 7]]


def test_duplicates_are_kept_as_they_come():
    ll = np.array([[0.5, 0.5, 0.5], [2.0, 1.0, 2.0]], np.float32)
    pre = np.array([[3, 3, 3], [5, 6, 5]], np.int32)
    idx, out = C.rerank(ll, pre, 3)
    assert idx.tolist() == [[3, 3, 3], [5, 5, 6]]
    assert out.tolist() == [[0.5, 0.5, 0.5], [2.0, 2.0, 1.0]]


def test_minus_infinity_ranks_last_and_n_out_above_n_in_keeps_all():
    ll = np.array([[-INF, -1e30, 0.0, -INF]], np.float32)
    pre = np.array([[0, 1, 2, 3]], np.int32)
    idx, out = C.rerank(ll, pre, 50)
    assert idx.shape == (1, 4)
    assert idx.tolist() == [[2, 1, 0, 3]]
    assert out[0, :2].tolist() == [0.0, np.float32(-1e30)] and np.all(np.isneginf(out[0, 2:]))
    # the two zeros are one score, as on the device (the key of score + 0); NaNs have a place (a positive one above +inf)
    key = C.score_key(np.array([-INF, -1.0, -0.0, 0.0, 1.0, INF, np.nan], np.float32))
    assert np.diff(key.astype(np.int64)).tolist()[2] == 0 and np.all(np.delete(np.diff(key.astype(np.int64)), 2) > 0)
    # so equal zeros of either sign go by Gaussian, then slot, like any other tie
    idx, out = C.rerank(np.array([[0.0, -0.0, 0.0, -1.0]], np.float32), np.array([[5, 2, 1, 0]], np.int32), 4)
    assert idx.tolist() == [[1, 2, 5, 0]] and out.tolist() == [[0.0, 0.0, 0.0, -1.0]]
    assert np.signbit(out[0]).tolist() == [False, True, False, True]   # the scores themselves come back as they were


def test_logsumexp_and_average():
    ll = np.array([[0.0, 0.0], [-INF, 5.0], [-INF, -INF], [1000.0, 1000.0]])
    got = C.logsumexp(ll)
    assert got[0] == pytest.approx(np.log(2.0), abs=1e-15) and got[1] == 5.0 and np.isneginf(got[2])
    assert got[3] == pytest.approx(1000.0 + np.log(2.0), abs=1e-12)
    # 2^24 + 1 + 1 in float32 would lose both ones; the fp64 sum keeps them, and the division rounds once
    v = np.array([2.0 ** 24, 1.0, 1.0, 2.0], np.float32)
    assert C.average_like(v) == np.float32((2.0 ** 24 + 4.0) / 4.0)
    assert C.average_like(np.array([-3.5], np.float32)) == np.float32(-3.5)


def test_vad_decisions_by_hand():
    speech = np.array([-1.0, -5.0, -2.0, -2.0], np.float32)
    noise = np.array([-2.0, -1.0, -2.0, -2.5], np.float32)
    music = np.array([-3.0, -4.0, -2.0, -2.25], np.float32)
    # the tie of frame 2 goes to the first class
    assert C.vad_from_frame_likes([speech, noise, music]).tolist() == [0.0, 1.0, 0.0, 0.0]
    # log(0.8 / 0.1) = 2.08 in favour of the third class: it takes every frame but the one where the second leads it by 3
    assert C.vad_from_frame_likes([speech, noise, music], priors=[0.1, 0.1, 0.8]).tolist() == [2.0, 1.0, 2.0, 2.0]
    assert C.vad_from_frame_likes([speech, noise, music], label_map=[1, 0, 2]).tolist() == [1.0, 0.0, 1.0, 1.0]


def test_merge_by_hand():
    a = np.array([1, 1, 0, 0, 1], np.float32)
    b = np.array([1, 0, 1, 2, 2], np.float32)
    assert C.merge_vads(a, b).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    triples = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (1, 1, 1), (1, 2, 2)]
    assert C.merge_vads(a, b, triples).tolist() == [1.0, 0.0, 0.0, 0.0, 2.0]
    with pytest.raises(KeyError):
        C.merge_vads(a, b, triples[:-1])


def test_float_and_vector_tables_round_trip():
    items = [("utt-a", np.float32(-71.25)), ("utt-b", np.float32(0.1))]
    for binary in (True, False):
        assert C.read_float_table(C.float_table_bytes(items, binary)) == items
    assert C.float_table_bytes(items[:1], False) == b"utt-a -71.25\n"
    assert C.float_table_bytes(items[:1], True) == b"utt-a \0B\x04" + np.float32(-71.25).tobytes()
    vecs = [("u1", np.array([0.0, 1.0, 2.0], np.float32)), ("u2", np.array([1.5], np.float32))]
    for binary in (True, False):
        got = C.read_vector_table(C.vector_table_bytes(vecs, binary))
        assert [k for k, _ in got] == ["u1", "u2"] and all(np.array_equal(g, v) for (_, g), (_, v) in zip(got, vecs))


# ------------------------------------------------------------------------------------------------------------------- the library, host only
def test_the_library_decides_as_the_restatement_does():
    P = H.pkg()
    rng = np.random.default_rng(5)
    likes = [rng.integers(-6, 1, 200).astype(np.float32) for _ in range(3)]   # small integers: many ties
    assert np.array_equal(P.vad_from_frame_likes(likes), C.vad_from_frame_likes(likes))
    assert np.array_equal(P.vad_from_frame_likes(likes, map=[0, 1, 2]), C.vad_from_frame_likes(likes))
    # priors whose logs are far from any difference of two integers: the decisions do not hang on a rounding
    pri = [0.25, 0.3, 0.45]
    assert np.array_equal(P.vad_from_frame_likes(likes, priors=pri, map=[1, 0, 2]), C.vad_from_frame_likes(likes, pri, [1, 0, 2]))
    assert len(set(P.vad_from_frame_likes(likes, priors=pri).tolist())) == 3
    with pytest.raises(P.XvError, match="not positive"):
        P.vad_from_frame_likes(likes, priors=[0.5, 0.0, 0.5])
    a = rng.integers(0, 2, 300).astype(np.float32)
    b = rng.integers(0, 3, 300).astype(np.float32)
    assert np.array_equal(P.merge_vads(a, b), C.merge_vads(a, b))
    triples = [(x, y, (x * y + y) % 3) for x in range(2) for y in range(3)]
    assert np.array_equal(P.merge_vads(a, b, map=triples), C.merge_vads(a, b, triples))
    with pytest.raises(P.XvError, match=r"pair \(1, 2\)") as e:
        P.merge_vads(np.array([0, 1], np.float32), np.array([1, 2], np.float32), map=triples[:-1])
    assert e.value.status == P.XV_ERR_IO
