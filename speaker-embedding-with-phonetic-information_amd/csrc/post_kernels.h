// Device kernels of logprob-to-post (semantics in post.h): a matrix of log-probabilities, several thousand columns wide, becomes
// sparse (column, weight) pairs row by row.  Kept out of kernels.hip for the reason compress_kernels.* are: KERNELS_SHA names the
// extraction kernels only.
//
// A launch works on rows [row0, row0 + rows) of a call's packed matrices; x points at row row0.  The size of the output is not
// known in advance and a row's count has no bound but its width, so there are two passes over the input and a scan between them:
//   logprob_post_count   one wave per row (kPostThreads / 64 rows per workgroup).  The wave walks the row in tiles of kPostTile
//                        columns, kPostTile / 64 independent dword loads per lane (lane l of load k holds column
//                        c0 + 64 k + l: every load is one contiguous 256-byte line, whatever the alignment of the row), decides
//                        every column, and adds the popcounts of the wave ballots.  count[r] and nan[r] are written by lane 0.
//   logprob_post_scan    one workgroup: off[0 .. rows] = the exclusive prefix sums of count (int32: the host keeps
//                        rows * cols of a launch below 2^31).  kPostScanThreads * 4 bytes of LDS.
//   logprob_post_write   the count pass again, expf and the draw recomputed from the input (nothing is staged between the passes;
//                        the second read comes from L2 / the memory-side cache where the launch fits, which was worth 4 % when
//                        measured: profiles/logprob_post_bench.md).  A kept column's slot is
//                        off[r] + (kept in the tiles before) + (kept in the loads before it in this tile) + popcount(ballot of
//                        its load & lanes below): columns stay ascending.  idx and w are written with plain vector stores.
// Neither pass uses LDS, a barrier, an atomic of any kind or a scalar-memory write; a row's count and content depend on that row,
// its utterance's seed and its index within the utterance alone.
//
// Precision.  p = expf(x) is HIP's device expf, whose documented maximum error is 1 ulp (HIP documentation, "HIP math API",
// single-precision table: expf 1 ulp); tests/test_gpu_logprob_post.py holds a kept p to that plus the rounding of the fp64 value
// to fp32: 2 ulp.  p / min_post is compiled as a correctly rounded division (Makefile).  A pruned entry's weight is min_post's
// bits.
// Limits: the number of columns is an int32 and otherwise limited by memory alone; the pairs of one launch fit an int32.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kPostThreads = 256;       // 4 waves = 4 rows per workgroup
constexpr int kPostTile = 512;          // columns per step of a wave: 8 loads of 64
constexpr int kPostScanThreads = 256;   // the scan's one workgroup; its LDS is kPostScanThreads * 4 bytes
constexpr int kPostCountLdsBytes = 0, kPostWriteLdsBytes = 0, kPostScanLdsBytes = kPostScanThreads * 4;

struct LogprobPostArgs {
  const float* x;            // [rows][cols], the launch's rows
  int64_t row0;              // the first row's index in the call
  int rows, cols;
  const int32_t* row_off;    // [n_utts + 1] of the call
  const uint64_t* utt_seed;  // [n_utts]; read only with random_prune and min_post > 0
  int n_utts;
  float min_post;
  int random_prune;
  int32_t* count;            // [rows]
  int32_t* nan;              // [rows] NaN inputs of the row
  int32_t* off;              // [rows + 1]
  int32_t* idx;              // [off[rows]]
  float* w;                  // [off[rows]]
};

hipError_t launch_logprob_post_count(const LogprobPostArgs& a, hipStream_t s);
hipError_t launch_logprob_post_scan(const LogprobPostArgs& a, hipStream_t s);
hipError_t launch_logprob_post_write(const LogprobPostArgs& a, hipStream_t s);

}  // namespace xv
