// Device kernels of i-vector extractor training: the E-step of ivector-extractor-acc-stats (semantics in ivex_train.h).  Kept out
// of kernels.hip for the reason ivex_kernels.* are: KERNELS_SHA names the x-vector extraction kernels only.
//
// They run behind the launches of IvexExtract (ivex_kernels.h), which leave, per utterance of a launch group, gamma, X, the linear
// term l, the packed Q, the Cholesky factor L of Q in the lower triangle of the solve's [S + 1][S] workspace and the fp64 solution
// m.  Everything is fp64; no floating-point value goes through an atomic, nothing uses scratch, and every sum has an order that is
// a function of the utterance and the model (posterior kernel) or of the slots (rank update, small sums) alone.
//   ivex_posterior      one workgroup per accepted utterance, which it finds in src[] and whose pending slot is slot[].
//                         1. Z = L^-1 into zwork [S][S] by rows: Z[i][j] = (delta_ij - sum_{k = j}^{i - 1} L[i][k] Z[k][j]) / L[i][i],
//                            k ascending; thread j owns columns j, j + kIvexPosteriorThreads, ... and reads back only what it wrote itself.
//                         2. Var[a][b] = sum_{k = a}^{S - 1} Z[k][a] Z[k][b] (a >= b, k ascending), one thread per packed element;
//                            scatter = Var + m_a m_b goes to the slot.  On the way the thread gathers its share of tr Var,
//                            tr(Var Q_a) and m' Q_a m, Q_a = Q - I from the packed Q.
//                         3. logdet Var = -2 sum_i log L[i][i], i ascending, by one thread.
//                         4. the utterance's part of the objective that needs the posterior,
//                              l_a . m - m' Q_a m / 2 - tr(Var Q_a) / 2 - (|m - p e_0|^2 + tr Var) / 2 + logdet Var / 2 + S / 2,
//                            l_a = l - p e_0, the threads' shares added by a fixed tree.
//                         5. gamma, X and m of the utterance are copied to the slot.
//   ivex_rank_update    C[M][N] += A' B, A [kIvexTrainSlots][M], B [kIvexTrainSlots][N], on v_mfma_f64_16x16x4_f64 (fragment maps in
//                       ivex_kernels.h).  A workgroup owns 64 rows of C, one row tile of 16 per wave, and kIvexRankColTiles column
//                       tiles of 16; a wave keeps its 16 rows of A' for all 64 k in registers (16 doubles per lane), and per
//                       column tile loads the B fragments and the C tile, issues 16 MFMAs with k ascending and stores C.  Rows
//                       beyond M, columns beyond N and slots beyond `count` are masked to zero in registers and never stored.
//                       One kernel serves R (M = G, N = P, A = gamma, B = scatter) and Y (M = G D, N = S, A = X, B = m).
//   ivex_small_sums     one thread per element of gamma [G], ivector_sum [S], ivector_scatter [P] and the objective: the slots
//                       below `count` added in slot order to one temporary, which is added to the running sum once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace xv {

constexpr int kIvexTrainThreads = 256;
constexpr int kIvexPosteriorThreads = 1024;   // the posterior kernel waits on memory: 40.8 ms with sixteen waves per utterance, 66.4 ms with four (profiles/ivex_train_bench.md)
constexpr int kIvexTrainSlots = 64;      // pending utterances of one rank update (the K of the update; a multiple of 4)
constexpr int kIvexRankColTiles = 8;     // column tiles of 16 a workgroup of the rank update walks

struct IvexPosteriorArgs {
  int n;                                 // workgroups: accepted utterances of this launch, <= kIvexTrainSlots
  uint8_t src[kIvexTrainSlots];          // utterance of the launch group
  uint8_t slot[kIvexTrainSlots];         // pending slot it takes
  int G, D, S;
  double prior_offset;
  // per utterance of the launch group, as IvexExtract left them
  const double* gamma;       // [B][G]
  const double* X;           // [B][G D]
  const double* linear;      // [B][S]
  const double* quadratic;   // [B][S (S + 1) / 2] packed Q
  const double* work;        // [B][S + 1][S]: L in the lower triangle
  const double* solution;    // [B][S] the fp64 solution, with the prior offset
  double* zwork;             // [kIvexTrainSlots][S][S], by slot
  // the pending slots
  double* p_gamma;           // [slots][G]
  double* p_X;               // [slots][G D]
  double* p_m;               // [slots][S]
  double* p_scatter;         // [slots][P]
  double* p_logdet;          // [slots]
  double* p_auxf;            // [slots]
};

struct IvexRankUpdateArgs {
  const double* A;   // [kIvexTrainSlots][M]
  const double* B;   // [kIvexTrainSlots][N]
  double* C;         // [M][ldc]
  int count;         // filled slots, 0 .. kIvexTrainSlots
  int64_t M, N, ldc;
};

struct IvexSmallSumsArgs {
  int count, G, S;
  const double* p_gamma;     // [slots][G]
  const double* p_m;         // [slots][S]
  const double* p_scatter;   // [slots][P]
  const double* p_auxf;      // [slots]
  double* gamma;             // [G]
  double* ivector_sum;       // [S]
  double* ivector_scatter;   // [P]
  double* auxf;              // [1]
};

hipError_t launch_ivex_posterior(const IvexPosteriorArgs& a, hipStream_t s);
hipError_t launch_ivex_rank_update(const IvexRankUpdateArgs& a, hipStream_t s);
hipError_t launch_ivex_small_sums(const IvexSmallSumsArgs& a, hipStream_t s);

}  // namespace xv
