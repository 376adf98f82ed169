// nnet-am-compute: the forward pass of an nnet2 acoustic model (nnet2_model.h) on the device.  A stage of its own, like post,
// ubm and ivex: its kernels are nnet2_kernels.*, nothing of the extractor's engine is used.  DESIGN.md section 3.13.
//
// Semantics (tests/nnet2_ref.py states them in fp64):
//   splice      row t of the output is the concatenation, in context order, of input rows t + c
//   p-norm      y[j] = sqrt(sum_{i<G} x[jG + i]^2), G = in / out
//   normalize   y = x * max(2^-66, (1/D) sum x^2)^-1/2 per row
//   softmax     subtract the row maximum, exponentiate, divide by the sum, floor at 1e-20
//   sum-group   sums over consecutive groups of the given sizes
//   priors      column j times 1 / prior[j] (kNnet2DivideByPriors; an error when the model has none or of another dimension)
//   log         floor at 1e-20, natural logarithm (kNnet2ApplyLog)
//   padding     kNnet2PadInput: the utterance is extended by left-context copies of its first row and right-context copies of its
//               last row, T rows out for T in; without it T - left - right rows out (none when T <= left + right).
// A frame's output row is the same bits alone, in any batch, at any position in its utterance's blocks: every sum is formed in
// an order that is a function of the frame's own inputs (nnet2_kernels.h).
//
// Layout.  The extended utterances are packed back to back into one sequence of S rows; every layer is computed at every row of
// the sequence (a row near an utterance's edge reads its neighbour's rows, and is context only: computed, never consumed).  The
// sequence passes through the device in blocks of rows_per_block rows plus left + right rows of overlap, and every buffer has
// halo rows at both ends, so that no shifted read leaves it.  Nnet2Plan is the pure host function that sizes the blocks.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "nnet2_model.h"

namespace xv {

// An argument the stage refuses (the C entries give XV_ERR_ARG for it): the one place the arguments are checked.
struct Nnet2ArgError : public KioError {
  explicit Nnet2ArgError(const std::string& m) : KioError(m) {}
};

enum { kNnet2ApplyLog = 1, kNnet2DivideByPriors = 2, kNnet2PadInput = 4 };

constexpr int64_t kNnet2DefaultWorkspace = (int64_t)256 << 20;
constexpr int64_t kNnet2MaxBlockRows = 1 << 20;

// What the plan needs of a model.
struct Nnet2Dims {
  int input_dim = 0, output_dim = 0, softmax_dim = 0, left_context = 0, right_context = 0;
  int max_plane_cols = 0;   // the widest (hi, lo) plane row, in halves: layer inputs padded to the K tile
  int max_pre_cols = 0;     // the widest fp32 pre-activation row
  int halo = 0;             // the largest |offset| of any splice
};
Nnet2Dims DimsOf(const Nnet2Model& m);

struct Nnet2BlockPlan {
  int64_t rows_per_block = 0, n_blocks = 0, bytes = 0;   // block b: rows [b rows_per_block, min(rows, (b + 1) rows_per_block))
};
// Pure.  rows: the length of the packed sequence; block_rows <= 0: the most that fit workspace_bytes (<= 0: the default), at most
// kNnet2MaxBlockRows; block_rows > 0: that many, if they fit.  false with *why: a workspace that does not hold one block.
bool Nnet2Plan(const Nnet2Dims& d, int64_t rows, int64_t block_rows, int64_t workspace_bytes, Nnet2BlockPlan* plan, std::string* why);
// bytes of device workspace for blocks of `block_rows` rows
int64_t Nnet2BlockBytes(const Nnet2Dims& d, int64_t block_rows);

// The model with its weights on a device (uploaded by the first Compute, to that call's device).
class Nnet2 {
 public:
  explicit Nnet2(const std::string& rxfilename);
  ~Nnet2();
  const Nnet2Model& model() const { return model_; }
  const Nnet2Dims& dims() const { return dims_; }
  // the rows utterance of t rows gives
  int64_t OutRows(int64_t t, int flags) const;
  // Nnet2ArgError: unknown flags, or kNnet2DivideByPriors on a model without priors of the output dimension
  void CheckFlags(int flags) const;
  // feats [row_off[n_utts]][input_dim], out [sum OutRows][output_dim].  layer_ms (optional): num_layers + 1 device times, the
  // last one the head's, each summed over the blocks.
  void Compute(int device, const float* feats, const int32_t* row_off, int n_utts, int flags, int64_t block_rows, float* out, float* device_ms,
               float* layer_ms = nullptr);

 private:
  struct Device;
  void Upload(int device);
  Nnet2Model model_;
  Nnet2Dims dims_;
  std::unique_ptr<Device> dev_;
};

// One launch each on caller data (the unit tests).
// x [rows][k] fp32 is split by the input-preparation launch into planes with `halo` zero rows at both ends; then the affine
// launch: out[t][j] = bias[j] + sum_c sum_i w[j][c k + i] x[t + context[c]][i], rows outside [0, rows) reading as zero.
void Nnet2KernelAffine(int device, const float* x, int rows, int k, const int32_t* context, int n_ctx, const float* w, const float* bias, int n, float* out);
// pre [rows][in_dim] -> hi, lo [rows][ld] (ld = out_dim rounded up to 32)
void Nnet2KernelRow(int device, const float* pre, int rows, int in_dim, int out_dim, int nonlin, bool normalize, uint16_t* hi, uint16_t* lo);
// logits [rows][n] -> out [rows][n_groups or n]; sizes / priors may be null
void Nnet2KernelHead(int device, const float* logits, int rows, int n, const int32_t* sizes, int n_groups, const float* priors, bool apply_log, float* out);

}  // namespace xv
