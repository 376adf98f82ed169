"""The counting sort by key (csrc/bucket_sort.h) on its own, through xv_bucket_sort: exact equality with numpy's stable sort inside
every segment, at the sizes where a chunk, a segment or the key scan changes its path."""
import os
import re

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
P = H.pkg()

_HDR = open(os.path.join(H.ROOT, H.PKG_NAME, "csrc", "bucket_sort.h")).read()
C = int(re.search(r"kBucketSortChunk = (\d+);", _HDR).group(1))
MAX_SEG = int(re.search(r"kBucketSortMaxSegments = (\d+);", _HDR).group(1))


def reference(keys, seg_off, num_keys):
    """(bucket_start [segments][num_keys + 1], sorted [pairs]) restated with numpy"""
    keys = np.asarray(keys, np.int64)
    start = np.zeros((len(seg_off) - 1, num_keys + 1), np.int32)
    order = np.zeros(len(keys), np.int32)
    for s in range(len(seg_off) - 1):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        seg = keys[a:b]
        order[a:b] = a + np.argsort(seg, kind="stable")
        start[s] = a + np.searchsorted(np.sort(seg), np.arange(num_keys + 1))
    return start, order


def check(keys, seg_off, num_keys):
    keys = np.asarray(keys, np.int32)
    seg_off = np.asarray(seg_off, np.int32)
    want_start, want_sorted = reference(keys, seg_off, num_keys)
    assert want_start.shape == (len(seg_off) - 1, num_keys + 1) and want_sorted.shape == keys.shape
    assert np.array_equal(want_start[:, 0], seg_off[:-1]) and np.array_equal(want_start[:, -1], seg_off[1:])
    start, order = P.bucket_sort(keys, seg_off, num_keys)
    assert start.dtype == np.int32 and order.dtype == np.int32
    assert np.array_equal(start, want_start)
    assert np.array_equal(order, want_sorted)
    return start, order


def interleaved(lengths, seed):
    """one key per entry of lengths, key k on lengths[k] pairs, dealt over the list"""
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(len(lengths)), lengths)).astype(np.int32)


def test_one_segment_bucket_lengths_around_the_chunk():
    lengths = [0, 1, 3, C - 1, C, C + 1, 2 * C + 3]
    keys = interleaved(lengths, 1)
    start, _ = check(keys, [0, len(keys)], len(lengths))
    assert np.diff(start[0]).tolist() == lengths


def test_one_segment_every_pair_on_one_key():
    n = 2 * C + 3   # ranks up to C - 1, and the key's counts in three chunks
    _, order = check(np.full(n, 2, np.int32), [0, n], 5)
    assert np.array_equal(order, np.arange(n))


@pytest.mark.parametrize("num_keys", [1, 256, 257, 600])
def test_one_segment_number_of_keys(num_keys):
    keys = np.random.default_rng(num_keys).integers(0, num_keys, 3 * C + 77).astype(np.int32)
    check(keys, [0, len(keys)], num_keys)


@pytest.mark.parametrize("pairs", [C, C + 1])
def test_one_segment_pairs_at_the_chunk(pairs):
    keys = np.random.default_rng(pairs).integers(0, 40, pairs).astype(np.int32)
    check(keys, [0, pairs], 40)


def test_no_pairs():
    start, order = check(np.zeros(0, np.int32), [0, 0], 7)
    assert not start.any() and order.size == 0


SEG_LENGTHS = [0, 1, C - 1, C, C + 1, 2 * C + 3, 0, 5]


def test_segments_around_the_chunk_and_empty():
    seg_off = np.concatenate([[0], np.cumsum(SEG_LENGTHS)])
    keys = np.random.default_rng(2).integers(0, 9, seg_off[-1]).astype(np.int32)
    start, _ = check(keys, seg_off, 9)
    for s in (0, 6):   # a segment with no pairs: a constant row
        assert np.all(start[s] == seg_off[s])


def test_64_short_segments():
    rng = np.random.default_rng(3)
    seg_off = np.concatenate([[0], np.cumsum(rng.integers(0, 41, MAX_SEG))])
    keys = rng.integers(0, 300, seg_off[-1]).astype(np.int32)
    check(keys, seg_off, 300)


def test_64_empty_segments():
    start, order = check(np.zeros(0, np.int32), np.zeros(MAX_SEG + 1, np.int32), 11)
    assert start.shape == (MAX_SEG, 12) and not start.any() and order.size == 0


def test_one_list_whole_and_cut_into_segments():
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 50, 3 * C + 10).astype(np.int32)
    _, whole = check(keys, [0, len(keys)], 50)
    seg_off = np.array([0, 7, 7, C + 7, 2 * C + 7, len(keys)])
    _, cut = check(keys, seg_off, 50)
    assert np.array_equal(whole, np.argsort(keys, kind="stable"))
    for s in range(len(seg_off) - 1):
        a, b = seg_off[s], seg_off[s + 1]
        assert np.array_equal(cut[a:b], a + np.argsort(keys[a:b], kind="stable"))
        # the segment's pairs of the whole list's order, in that order, are the segment's own sort
        assert np.array_equal(whole[(whole >= a) & (whole < b)], cut[a:b])


def refused(keys, seg_off, num_keys, pairs=None):
    with pytest.raises(P.XvError) as e:
        P.bucket_sort(np.asarray(keys, np.int32), np.asarray(seg_off, np.int32), num_keys, pairs=pairs)
    assert e.value.status == P.XV_ERR_ARG


def test_refusals():
    keys = np.array([0, 1, 2, 1, 0], np.int32)
    refused(np.zeros(0, np.int32), [0], 3)                                    # no segment
    refused(np.zeros(0, np.int32), np.zeros(MAX_SEG + 2, np.int32), 3)        # 65 segments
    refused(keys, [0, 4, 3, 5], 3)                                            # a decreasing table
    refused(keys, [0, 2, 4], 3)                                               # the table ends before the pairs do
    refused(keys, [0, 2, 6], 3, pairs=5)                                      # ... and after
    refused(keys, [0, 5], 2)                                                  # a key equal to num_keys
    refused(np.array([0, -1, 1], np.int32), [0, 3], 3)                        # a negative key
    check(keys, [0, 2, 5], 3)                                                 # the same list, taken
