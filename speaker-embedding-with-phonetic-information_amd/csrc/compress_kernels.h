// Device kernels of the feature compressor (copy-feats --compress=true: Kaldi's CompressedMatrix, semantics in compress.h).
// Kept out of kernels.hip for the reason feat_kernels.* are: KERNELS_SHA names the extraction kernels only.
//
// A launch works on a ragged batch of row-major fp32 matrices that share a column count: packed rows plus row_off[n + 1].  Three
// launches per batch, whatever n is; each takes a list of work items (matrix, block) built by the host (compress.cc):
//   cmp_minmax  exact minimum / maximum of every matrix and its non-finite flag: integer atomics on the order-preserving image
//               of the floats, so the result does not depend on the order of arrival
//   cmp_select  "CM" matrices only: per (matrix, column) the two inner order statistics by a radix select - four passes of eight
//               bits over that image, both ranks at once, histograms in LDS - and the column minimum / maximum; writes the
//               column headers.  Exact selection: the header words are compared for equality with the host restatement
//   cmp_encode  the global header and the codes: "CM" bytes leave column-major through an LDS transpose, "CM2" / "CM3" codes
//               row-major.  Rows are read as they lie in memory (consecutive lanes, consecutive columns) in every kernel
// Every expression of the format is evaluated in fp32 with one rounding per operation (the file is compiled with contraction
// off and hipcc's correctly rounded division), as tests/compress_ref.py states it.  A matrix's bytes depend on the matrix and the
// method only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kCmpMinmaxThreads = 256;
constexpr int kCmpMinmaxChunk = 16384;    // elements per workgroup of cmp_minmax
constexpr int kCmpSelectThreads = 1024;
constexpr int kCmpSelectCols = 24;        // columns per workgroup of cmp_select (two histograms of 256 bins each: 48 KiB of LDS)
constexpr int kCmpEncodeThreads = 256;
constexpr int kCmpEncodeRows = 128;       // rows per workgroup of cmp_encode
constexpr int kCmpEncodeCols = 64;        // columns per LDS tile of cmp_encode

// per matrix, written by cmp_minmax; the host initialises it to {0xffffffff, 0, 0, 0}
struct CmpStats {
  uint32_t min_key, max_key;   // order-preserving images of the minimum and the maximum
  uint32_t nonfinite;          // != 0: the matrix holds a NaN or an infinity
  uint32_t pad;
};

struct CmpArgs {
  const float* feats;          // [row_off[n]][cols]
  const int32_t* row_off;      // [n + 1]
  const int64_t* obj_off;      // [n] where each object starts in out, a multiple of 4
  CmpStats* stats;             // [n]
  uint8_t* out;
  int n, cols;
  int method;                  // 1 automatic, 2 "CM", 3 "CM2", 5 "CM3"
  const int32_t* item_mat;     // [n_items] work items of the launch: the matrix ...
  const int32_t* item_blk;     // ... and the block of it
  int n_items;
};

hipError_t launch_cmp_minmax(const CmpArgs& a, hipStream_t s);
hipError_t launch_cmp_select(const CmpArgs& a, hipStream_t s);
hipError_t launch_cmp_encode(const CmpArgs& a, hipStream_t s);

}  // namespace xv
