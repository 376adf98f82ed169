// The counting sort by key: see bucket_sort.h.
#include "bucket_sort.h"

#include <string.h>

namespace xv {
namespace {

constexpr int kChunkQuarters = kBucketSortChunk / kBucketSortThreads;   // a workgroup's threads cover a chunk in this many steps
static_assert(kBucketSortChunk % kBucketSortThreads == 0, "whole steps");

struct ChunkSpan {
  int seg, p0, cnt;   // the chunk's segment, its first pair and its pairs (1 .. kBucketSortChunk)
};

// Chunk c of the launch.  Its segment is the last one whose first chunk is not beyond c: the segments without pairs before it
// start at the same chunk.
__device__ inline ChunkSpan chunk_span(const BucketSortArgs& a, int c) {
  int lo = 0, hi = a.num_segments;   // answer in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.seg_chunk0[mid] <= c) lo = mid;
    else hi = mid;
  }
  ChunkSpan s;
  s.seg = lo;
  s.p0 = a.seg_off[lo] + (c - a.seg_chunk0[lo]) * kBucketSortChunk;
  const int left = a.seg_off[lo + 1] - s.p0;
  s.cnt = left < kBucketSortChunk ? left : kBucketSortChunk;
  return s;
}

__global__ __launch_bounds__(kBucketSortThreads) void bucket_sort_rank_kernel(const BucketSortArgs a) {
  __shared__ int32_t ks[kBucketSortChunk];
  const int c = blockIdx.x;
  const ChunkSpan ch = chunk_span(a, c);
#pragma unroll   // the loads of a thread are in flight together
  for (int q = 0; q < kChunkQuarters; ++q) {
    const int i = q * kBucketSortThreads + threadIdx.x;
    if (i < ch.cnt) ks[i] = a.keys[ch.p0 + i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ch.cnt; i += kBucketSortThreads) {
    const int32_t k = ks[i];
    int rank = 0, later = 0;
    for (int j = 0; j < ch.cnt; ++j) {
      const int eq = ks[j] == k ? 1 : 0;
      rank += eq & (j < i ? 1 : 0);
      later |= eq & (j > i ? 1 : 0);
    }
    a.local_rank[ch.p0 + i] = rank;
    if (!later) a.chunk_hist[c * a.hist_chunk_stride + k * a.hist_key_stride] = rank + 1;   // the chunk's count of k, written by its last pair
  }
}

// Several segments, histogram [chunk][key].  grid (key tiles, segments): the walk over a segment's chunks is coalesced across
// the keys, and a thread has the counts of kScanBatch chunks in flight.
constexpr int kScanBatch = 8;
__global__ __launch_bounds__(kBucketSortThreads) void bucket_sort_scan_chunks_kernel(const BucketSortArgs a) {
  const int k = blockIdx.x * kBucketSortThreads + threadIdx.x, s = blockIdx.y;
  if (k >= a.num_keys) return;
  const int c1 = a.seg_chunk0[s + 1];
  int32_t run = 0;
  for (int c = a.seg_chunk0[s]; c < c1; c += kScanBatch) {
    int32_t* h = a.chunk_hist + (int64_t)c * a.num_keys + k;
    int32_t v[kScanBatch];
#pragma unroll
    for (int j = 0; j < kScanBatch; ++j) v[j] = c + j < c1 ? h[(int64_t)j * a.num_keys] : 0;
#pragma unroll
    for (int j = 0; j < kScanBatch; ++j) {
      if (c + j < c1) h[(int64_t)j * a.num_keys] = run;
      run += v[j];
    }
  }
  a.bucket_start[(int64_t)s * (a.num_keys + 1) + k] = run;
}

// data[0 .. n) -> base + its exclusive prefix sums, in place; returns the sum.  All threads of the workgroup call it.
__device__ int32_t block_exclusive_scan(int32_t* data, int n, int32_t base) {
  __shared__ int32_t part[kBucketSortThreads];
  const int tid = threadIdx.x;
  const int per = (n + kBucketSortThreads - 1) / kBucketSortThreads;
  const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += data[i];
  part[tid] = sum;
  __syncthreads();
  for (int step = 1; step < kBucketSortThreads; step <<= 1) {
    const int32_t add = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int32_t run = base + part[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    const int32_t v = data[i];
    data[i] = run;
    run += v;
  }
  const int32_t all = part[kBucketSortThreads - 1];
  __syncthreads();   // part is free for the next call
  return all;
}

// One segment, histogram [key][chunk]: one workgroup per key scans the key's row.  A flat sort of a million pairs has a thousand
// chunks, which the walk above would leave to the few workgroups that the keys fill.
__global__ __launch_bounds__(kBucketSortThreads) void bucket_sort_scan_chunks_flat_kernel(const BucketSortArgs a) {
  const int k = blockIdx.x;
  const int32_t all = block_exclusive_scan(a.chunk_hist + k * a.hist_key_stride, a.seg_chunk0[1], 0);
  if (threadIdx.x == 0) a.bucket_start[k] = all;
}

__global__ __launch_bounds__(kBucketSortThreads) void bucket_sort_scan_keys_kernel(const BucketSortArgs a) {
  const int s = blockIdx.x;
  int32_t* start = a.bucket_start + (int64_t)s * (a.num_keys + 1);
  block_exclusive_scan(start, a.num_keys, a.seg_off[s]);
  if (threadIdx.x == 0) start[a.num_keys] = a.seg_off[s + 1];
}

// one thread per pair: kChunkQuarters workgroups per chunk
__global__ __launch_bounds__(kBucketSortThreads) void bucket_sort_place_kernel(const BucketSortArgs a) {
  const int c = blockIdx.x / kChunkQuarters;
  const ChunkSpan ch = chunk_span(a, c);
  const int i = (blockIdx.x % kChunkQuarters) * kBucketSortThreads + threadIdx.x;
  if (i >= ch.cnt) return;
  const int32_t* start = a.bucket_start + (int64_t)ch.seg * (a.num_keys + 1);
  const int32_t k = a.keys[ch.p0 + i];
  a.sorted[start[k] + a.chunk_hist[c * a.hist_chunk_stride + k * a.hist_key_stride] + a.local_rank[ch.p0 + i]] = ch.p0 + i;
}

}  // namespace

int64_t BucketSortChunks(const BucketSortArgs& a) {
  if (a.pairs < 0 || a.num_keys < 1 || a.num_segments < 1 || a.num_segments > kBucketSortMaxSegments) return -1;
  if (a.seg_off[0] != 0 || a.seg_off[a.num_segments] != a.pairs) return -1;
  int64_t chunks = 0;
  for (int s = 0; s < a.num_segments; ++s) {
    if (a.seg_off[s + 1] < a.seg_off[s]) return -1;
    chunks += CeilDiv((int64_t)a.seg_off[s + 1] - a.seg_off[s], kBucketSortChunk);
  }
  return chunks;
}

hipError_t launch_bucket_sort(const BucketSortArgs& args, hipStream_t s) {
  const int64_t chunks = BucketSortChunks(args);
  if (chunks < 0 || !args.bucket_start) return hipErrorInvalidValue;
  if (chunks > 0 && (!args.keys || !args.local_rank || !args.chunk_hist || !args.sorted)) return hipErrorInvalidValue;
  BucketSortArgs a = args;
  a.seg_chunk0[0] = 0;
  for (int i = 0; i < a.num_segments; ++i)
    a.seg_chunk0[i + 1] = a.seg_chunk0[i] + (int32_t)CeilDiv((int64_t)a.seg_off[i + 1] - a.seg_off[i], kBucketSortChunk);
  // the layout of the histogram follows the chunk scan that reads it: rows of one key's chunks for one segment, of one chunk's keys else
  a.hist_chunk_stride = a.num_segments == 1 ? 1 : a.num_keys;
  a.hist_key_stride = a.num_segments == 1 ? chunks : 1;
  const dim3 threads(kBucketSortThreads);
  if (chunks > 0) hipLaunchKernelGGL(bucket_sort_rank_kernel, dim3((unsigned)chunks), threads, 0, s, a);
  if (a.num_segments == 1) {
    hipLaunchKernelGGL(bucket_sort_scan_chunks_flat_kernel, dim3((unsigned)a.num_keys), threads, 0, s, a);
  } else {
    const unsigned key_tiles = (unsigned)CeilDiv(a.num_keys, kBucketSortThreads);
    hipLaunchKernelGGL(bucket_sort_scan_chunks_kernel, dim3(key_tiles, (unsigned)a.num_segments), threads, 0, s, a);
  }
  hipLaunchKernelGGL(bucket_sort_scan_keys_kernel, dim3((unsigned)a.num_segments), threads, 0, s, a);
  if (chunks > 0) hipLaunchKernelGGL(bucket_sort_place_kernel, dim3((unsigned)(chunks * kChunkQuarters)), threads, 0, s, a);
  return hipGetLastError();
}

hipError_t BucketSorter::Run(const int32_t* d_keys, int64_t pairs, const int32_t* seg_off, int num_segments, int num_keys, hipStream_t stream) {
  if (pairs < 0 || pairs > INT32_MAX || !seg_off || num_segments < 1 || num_segments > kBucketSortMaxSegments) return hipErrorInvalidValue;
  BucketSortArgs a;
  memset(&a, 0, sizeof a);
  a.keys = d_keys;
  a.pairs = (int)pairs;
  a.num_keys = num_keys;
  a.num_segments = num_segments;
  for (int s = 0; s <= num_segments; ++s) a.seg_off[s] = seg_off[s];
  const int64_t chunks = BucketSortChunks(a);
  if (chunks < 0) return hipErrorInvalidValue;
  const size_t hist_bytes = (size_t)chunks * num_keys * 4;
  rank.Reserve((size_t)pairs * 4);
  hist.Reserve(hist_bytes);
  start.Reserve((size_t)num_segments * (num_keys + 1) * 4);
  sorted.Reserve((size_t)pairs * 4);
  Check(hipMemsetAsync(hist.p, 0, hist_bytes, stream), "hipMemsetAsync");
  a.local_rank = rank.as<int32_t>();
  a.chunk_hist = hist.as<int32_t>();
  a.bucket_start = start.as<int32_t>();
  a.sorted = sorted.as<int32_t>();
  return launch_bucket_sort(a, stream);
}

}  // namespace xv
