// What full-covariance and diagonal UBM training share on the host: the update flags, the accumulators with their file, and the
// skeleton of the M-step.  The specifications stay with the two kinds (ubm_train.h, dubm_train.h); nothing here opens a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "kio.h"

namespace xv {

// "mvw" in any order -> the bits of ubm_train_kernels.h (m = 1, v = 2, w = 4), not augmented; KioError for any other letter.
int ParseGmmFlags(const std::string& letters);
int AugmentGmmFlags(int flags);   // v implies m, m implies w
std::string GmmFlagLetters(int flags);

// ---- the accumulators on the host, of either kind
struct GmmAccs {
  int num_gauss = 0, dim = 0, flags = 0;   // flags: augmented
  bool full = false;                       // the kind, set before Init: FgmmAccs and DgmmAccs are the two by name
  // [G], [G][D], and the second-order sums [G][D (D + 1) / 2] packed lower triangles (full) or [G][D]; mean / second are all
  // zeros without m / v
  std::vector<double> occ, mean, second;
  size_t second_width() const { return full ? (size_t)dim * (dim + 1) / 2 : (size_t)dim; }
  void Init(int num_gauss, int dim, int flags);
};
struct FgmmAccs : GmmAccs {
  FgmmAccs() { full = true; }
};
struct DgmmAccs : GmmAccs {};
// The file of ubm_train.h / dubm_train.h; the two differ in the section that v adds (<FULLVARACCS>, <DIAGVARACCS>) and a->full
// says which one is expected: a file without v reads as either kind.
// add = false: *a becomes the file's.  add = true: the file's values are added to *a, whose shape and flags must be the file's.
void ReadGmmAccsFile(const std::string& rxfilename, bool add, GmmAccs* a);
void WriteGmmAccsFile(const std::string& wxfilename, bool binary, const GmmAccs& a);

// ---- the M-step (host, fp64)
struct GmmEstResult {
  double objf_before = 0.0, objf_after = 0.0, count = 0.0;   // count: sum of occ
  int floored_elements = 0, floored_gauss = 0;
  std::vector<int32_t> removed;                                // ascending
  std::vector<std::string> warnings;
};
// What GmmEst needs of a kind: its model's arrays, its three thresholds and the two steps that differ.
struct GmmEstKind {
  int* num_gauss = nullptr;
  int dim = 0;
  std::vector<float>* weights = nullptr;
  std::vector<std::pair<std::vector<float>*, size_t>> rows;   // the per-Gaussian parameter arrays and their widths
  double min_gaussian_weight = 0.0, min_gaussian_occupancy = 0.0;
  bool remove_low_count_gaussians = true;
  bool gconsts_before = false;                      // recompute the gconsts before the first objective
  std::function<void()> gconsts;                    // ComputeGconsts of the model
  std::function<double()> objective;                // of the accumulators on the model as it stands
  std::function<void(int g, double occ)> update;    // the parameters of a Gaussian that is kept; counts its floors itself
};
// Steps 1 to 7 of ubm_train.h around kind.update: the checks, the objective before, every Gaussian's weight and fate with its
// warning, the renormalisation with w among the update flags, the gconsts, the objective after, the removal.
void GmmEst(const GmmAccs& accs, int update_flags, const GmmEstKind& kind, GmmEstResult* res);
// Takes the rows g with remove[g] out of rows [remove.size()][width].
void RemoveGmmRows(const std::vector<char>& remove, size_t width, std::vector<float>* rows);

}  // namespace xv
