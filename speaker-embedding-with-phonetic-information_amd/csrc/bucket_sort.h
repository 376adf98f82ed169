// The counting sort by key that the UBM posteriors, the GMM accumulators and the i-vector statistics start with: it buckets
// (frame, Gaussian) pairs by Gaussian so that one workgroup or wave walks a Gaussian's bucket front to back with no float atomic.
// Kept out of kernels.hip for the reason ubm_kernels.* are: KERNELS_SHA names the x-vector extraction kernels only.
//
// `pairs` keys in [0, num_keys) are sorted inside each of num_segments consecutive segments of the list (segment s is
// [seg_off[s], seg_off[s + 1])); the order inside a bucket is ascending pair index.  One segment is the flat sort: the same
// kernels but for the scan over the chunks, which the launcher picks by num_segments.  The list is cut into chunks of
// kBucketSortChunk pairs that never cross a segment.  Integer work only.
//   bucket_sort_rank         one workgroup per chunk: the chunk's keys go to LDS, a pair's rank is the number of earlier pairs
//                            of the chunk with its key, and the last pair of each key writes the chunk's count of it.
//   bucket_sort_scan_chunks  the counts become the chunk's offset inside the bucket, the total goes to the bucket table.  Several
//                            segments: one thread per (segment, key) walks the segment's chunks in a [chunk][key] histogram.  One
//                            segment (_flat): one workgroup per key scans its row of a [key][chunk] histogram; at 2048 keys and 1300
//                            chunks the walk costs 0.08 ms more per sort (profiles/bucket_sort_ab.md).
//   bucket_sort_scan_keys    one workgroup per segment: the exclusive scan of the totals, from seg_off[s].
//   bucket_sort_place        one thread per pair: pair -> bucket start + chunk offset + rank.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device.h"

namespace xv {

constexpr int kBucketSortThreads = 256;
constexpr int kBucketSortChunk = 1024;       // pairs per workgroup of the ranking kernel: a multiple of kBucketSortThreads
constexpr int kBucketSortMaxSegments = 64;

struct BucketSortArgs {
  const int32_t* keys;      // [pairs] each in [0, num_keys) (the host checks)
  int pairs, num_keys, num_segments;
  // the segment table, by value: entries beyond num_segments are not read
  int32_t seg_off[kBucketSortMaxSegments + 1];      // first pair of the segment; [num_segments] = pairs
  int32_t seg_chunk0[kBucketSortMaxSegments + 1];   // first chunk of the segment: the launcher fills it
  int32_t* local_rank;      // [pairs]
  int32_t* chunk_hist;      // chunks * num_keys counts, zero before the launch; the scan turns them into offsets inside the bucket
  int64_t hist_chunk_stride, hist_key_stride;       // (chunk, key) is at chunk * chunk stride + key * key stride: the launcher fills them
  int32_t* bucket_start;    // [num_segments][num_keys + 1] absolute pair positions; a segment with no pairs gets a constant row
  int32_t* sorted;          // [pairs] pair indices, bucket after bucket
};

// The chunks of a.seg_off, or -1 for what the launcher refuses whatever the pointers are: pairs outside [0, INT32_MAX],
// num_keys < 1, num_segments outside [1, kBucketSortMaxSegments], a table that does not rise from 0 to pairs.
int64_t BucketSortChunks(const BucketSortArgs& a);
// rank, the two scans, placement.  The scans run for pairs == 0 as well: every bucket_start entry is then 0.
// hipErrorInvalidValue where BucketSortChunks refuses and for a null pointer the kernels would read or write.
hipError_t launch_bucket_sort(const BucketSortArgs& a, hipStream_t s);

// The sort's buffers on one device: they live as long as the object and only grow.
struct BucketSorter {
  DevBuf rank, hist;
  DevBuf start, sorted;   // the result: bucket_start and sorted of BucketSortArgs
  // d_keys: [pairs] on the device; seg_off: [num_segments + 1] on the host.  Sizes the buffers, clears the histogram and
  // launches; returns what launch_bucket_sort does (nothing is allocated for arguments it refuses).
  hipError_t Run(const int32_t* d_keys, int64_t pairs, const int32_t* seg_off, int num_segments, int num_keys, hipStream_t stream);
};

}  // namespace xv
