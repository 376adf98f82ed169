#include "gmm_train.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <sstream>

#include "gmm_sparse_acc.h"
#include "ubm_train_kernels.h"

namespace xv {

int ParseGmmFlags(const std::string& letters) {
  int flags = 0;
  for (char c : letters) {
    if (c == 'm') flags |= kFgmmFlagMeans;
    else if (c == 'v') flags |= kFgmmFlagVariances;
    else if (c == 'w') flags |= kFgmmFlagWeights;
    else throw KioError("Invalid element '" + std::string(1, c) + "' of the update flags '" + letters + "': they are made of m, v and w");
  }
  return flags;
}

int AugmentGmmFlags(int flags) {
  if (flags & kFgmmFlagVariances) flags |= kFgmmFlagMeans;
  if (flags & kFgmmFlagMeans) flags |= kFgmmFlagWeights;
  return flags;
}

std::string GmmFlagLetters(int flags) {
  std::string s;
  if (flags & kFgmmFlagMeans) s += 'm';
  if (flags & kFgmmFlagVariances) s += 'v';
  if (flags & kFgmmFlagWeights) s += 'w';
  return s;
}

void GmmAccs::Init(int g, int d, int f) {
  if (g < 1 || d < 1 || f < 0 || f > 7) throw KioError("GMM accumulators: bad shape or flags");
  num_gauss = g;
  dim = d;
  flags = AugmentGmmFlags(f);
  occ.assign((size_t)g, 0.0);
  mean.assign((size_t)g * d, 0.0);
  second.assign((size_t)g * second_width(), 0.0);
}

void ReadGmmAccsFile(const std::string& rxfilename, bool add, GmmAccs* a) {
  Input in;
  in.Open(rxfilename);
  const bool binary = ReadBinaryHeader(in);
  ExpectToken(in, binary, "<GMMACCS>");
  ExpectToken(in, binary, "<VECSIZE>");
  const int dim = ReadInt32(in, binary);
  ExpectToken(in, binary, "<NUMCOMPONENTS>");
  const int G = ReadInt32(in, binary);
  ExpectToken(in, binary, "<FLAGS>");
  int flags;
  if (binary) {
    if (in.Get() != 2) throw KioError("expected uint16 (size byte 2) in " + in.Name());
    uint16_t v;
    in.Read(&v, 2);
    flags = v;
  } else {
    flags = ReadInt32(in, false);
  }
  if (dim < 1 || G < 1 || flags < 0 || flags > 7 || AugmentGmmFlags(flags) != flags)
    throw KioError("GMM accumulators with dimension " + std::to_string(dim) + ", " + std::to_string(G) + " components and flags " + std::to_string(flags));
  if (!add) a->Init(G, dim, flags);
  else if (a->dim != dim || a->num_gauss != G || a->flags != flags)
    throw KioError("the accumulators of " + in.Name() + " (dimension " + std::to_string(dim) + ", " + std::to_string(G) + " components, flags " +
                   GmmFlagLetters(flags) + ") cannot be added to ones of dimension " + std::to_string(a->dim) + ", " + std::to_string(a->num_gauss) +
                   " components, flags " + GmmFlagLetters(a->flags));
  ExpectToken(in, binary, "<OCCUPANCY>");
  std::vector<float> v;
  ReadVector(in, binary, &v);
  if ((int)v.size() != G) throw KioError("<OCCUPANCY> has " + std::to_string(v.size()) + " values for " + std::to_string(G) + " components");
  for (int g = 0; g < G; ++g) a->occ[g] += (double)v[g];
  ExpectToken(in, binary, "<MEANACCS>");
  Matrix m;
  ReadMatrix(in, binary, &m);
  if (m.rows != G || m.cols != dim) throw KioError("<MEANACCS> is " + std::to_string(m.rows) + " x " + std::to_string(m.cols));
  for (size_t i = 0; i < (size_t)G * dim; ++i) a->mean[i] += (double)m.Data()[i];
  if (flags & kFgmmFlagVariances) {
    if (a->full) {
      ExpectToken(in, binary, "<FULLVARACCS>");
      for (int g = 0; g < G; ++g) {
        v.clear();
        if (ReadPackedMatrix(in, binary, &v) != dim) throw KioError("a covariance accumulator does not have the dimension " + std::to_string(dim));
        double* c = a->second.data() + (size_t)g * a->second_width();
        for (size_t i = 0; i < v.size(); ++i) c[i] += (double)v[i];
      }
    } else {
      ExpectToken(in, binary, "<DIAGVARACCS>");
      ReadMatrix(in, binary, &m);
      if (m.rows != G || m.cols != dim) throw KioError("<DIAGVARACCS> is " + std::to_string(m.rows) + " x " + std::to_string(m.cols));
      for (size_t i = 0; i < (size_t)G * dim; ++i) a->second[i] += (double)m.Data()[i];
    }
  }
  ExpectToken(in, binary, "</GMMACCS>");
  if (in.Close() != 0) throw KioError("the command of " + rxfilename + " failed");
}

void WriteGmmAccsFile(const std::string& wxfilename, bool binary, const GmmAccs& a) {
  Output out;
  out.Open(wxfilename);
  if (binary) out.Write("\0B", 2);
  WriteToken(out, binary, "<GMMACCS>");
  WriteToken(out, binary, "<VECSIZE>");
  WriteInt32(out, binary, a.dim);
  WriteToken(out, binary, "<NUMCOMPONENTS>");
  WriteInt32(out, binary, a.num_gauss);
  WriteToken(out, binary, "<FLAGS>");
  if (binary) {
    const uint16_t v = (uint16_t)a.flags;
    out.Put((char)2);
    out.Write(&v, 2);
  } else {
    WriteInt32(out, false, a.flags);
  }
  std::vector<float> f(a.occ.begin(), a.occ.end());   // the one rounding
  WriteToken(out, binary, "<OCCUPANCY>");
  WriteVector(out, binary, f.data(), a.num_gauss);
  Matrix m;
  m.rows = a.num_gauss;
  m.cols = a.dim;
  m.data.assign(a.mean.begin(), a.mean.end());
  WriteToken(out, binary, "<MEANACCS>");
  WriteMatrix(out, binary, m);
  if (a.flags & kFgmmFlagVariances) {
    if (a.full) {
      const size_t tri = a.second_width();
      WriteToken(out, binary, "<FULLVARACCS>");
      for (int g = 0; g < a.num_gauss; ++g) {
        f.assign(a.second.begin() + (size_t)g * tri, a.second.begin() + (size_t)(g + 1) * tri);
        WritePackedMatrix(out, binary, f.data(), a.dim);
      }
    } else {
      m.data.assign(a.second.begin(), a.second.end());
      WriteToken(out, binary, "<DIAGVARACCS>");
      WriteMatrix(out, binary, m);
    }
  }
  WriteToken(out, binary, "</GMMACCS>");
  if (out.Close() != 0) throw KioError("error closing output " + wxfilename);
}

void RemoveGmmRows(const std::vector<char>& remove, size_t width, std::vector<float>* rows) {
  size_t kept = 0;
  for (size_t g = 0; g < remove.size(); ++g) {
    if (remove[g]) continue;
    if (kept != g) std::copy(rows->begin() + g * width, rows->begin() + (g + 1) * width, rows->begin() + kept * width);
    ++kept;
  }
  rows->resize(kept * width);
}

void GmmEst(const GmmAccs& accs, int update_flags, const GmmEstKind& k, GmmEstResult* res) {
  const int G = *k.num_gauss, D = k.dim;
  if (accs.num_gauss != G || accs.dim != D)
    throw KioError("the accumulators (" + std::to_string(accs.num_gauss) + " components of dimension " + std::to_string(accs.dim) + ") are not the model's (" +
                   std::to_string(G) + " of dimension " + std::to_string(D) + ")");
  if (update_flags & ~accs.flags)
    throw KioError("the update flags '" + GmmFlagLetters(update_flags) + "' name statistics that the accumulators (flags '" + GmmFlagLetters(accs.flags) + "') do not have");
  *res = GmmEstResult();
  if (k.gconsts_before) k.gconsts();
  res->objf_before = k.objective();
  double occ_sum = 0.0;
  for (int g = 0; g < G; ++g) occ_sum += accs.occ[g];
  res->count = occ_sum;
  std::vector<float>& weights = *k.weights;
  std::vector<double> w((size_t)G);
  std::vector<char> remove((size_t)G, 0);
  for (int g = 0; g < G; ++g) {
    const double occ = accs.occ[g];
    const double prob = occ_sum > 0.0 ? occ / occ_sum : 1.0 / G;
    if (occ > k.min_gaussian_occupancy && prob > k.min_gaussian_weight) {
      w[g] = prob;
      k.update(g, occ);
    } else if (k.remove_low_count_gaussians && (int)res->removed.size() < G - 1) {
      std::ostringstream msg;
      msg << "Too little data - removing Gaussian (weight " << prob << ", occupation count " << occ << ", vector size " << D << ")";
      res->warnings.push_back(msg.str());
      res->removed.push_back(g);
      remove[g] = 1;
      w[g] = (double)weights[g];   // until it is taken out it counts with its old weight
    } else {
      std::ostringstream msg;
      msg << "Gaussian has too little data but not removing it because "
          << (k.remove_low_count_gaussians ? "it is the last Gaussian: i = " : "remove-low-count-gaussians == false: i = ") << g << ", occ = " << occ
          << ", weight = " << prob;
      res->warnings.push_back(msg.str());
      w[g] = std::max(prob, k.min_gaussian_weight);
    }
  }
  if (update_flags & kFgmmFlagWeights) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += w[g];
    for (int g = 0; g < G; ++g) weights[g] = (float)(w[g] / sum);
  }
  k.gconsts();
  res->objf_after = k.objective();
  if (!res->removed.empty()) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g)
      if (!remove[g]) sum += (double)weights[g];
    RemoveGmmRows(remove, 1, &weights);
    for (float& x : weights) x = (float)((double)x / sum);
    for (const auto& r : k.rows) RemoveGmmRows(remove, r.second, r.first);
    *k.num_gauss = G - (int)res->removed.size();
    k.gconsts();
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
void GmmSparseAcc::Reset(int g) {
  UseDevice(device, who_needs);
  num_gauss = g;
  occ.Reserve((size_t)g * 8);
  mean.Reserve((size_t)g * dim * 8);
  second.Reserve((size_t)g * second_width * 8);
  Check(hipMemset(occ.p, 0, (size_t)g * 8), "hipMemset");
  Check(hipMemset(mean.p, 0, (size_t)g * dim * 8), "hipMemset");
  Check(hipMemset(second.p, 0, (size_t)g * second_width * 8), "hipMemset");
}

int64_t GmmSparseAcc::UploadPairs(const char* who_c, const float* host_feats, int64_t rows, const int32_t* post_off, const int32_t* post_idx,
                                  const float* post_w) {
  const std::string who = who_c;
  if (rows < 0 || rows > INT32_MAX - 1 || !post_off) throw KioError(who + ": bad argument");
  if (post_off[0] != 0) throw KioError(who + ": the posterior offsets must start at 0");
  for (int64_t t = 0; t < rows; ++t)
    if (post_off[t + 1] < post_off[t]) throw KioError(who + ": the posterior offsets must not decrease");
  const int64_t pairs = post_off[rows];
  if (pairs == 0) return 0;
  if (!host_feats || !post_idx || !post_w) throw KioError(who + ": null buffer");
  for (int64_t i = 0; i < pairs; ++i)
    if (post_idx[i] < 0 || post_idx[i] >= num_gauss)
      throw KioError(who + ": the posteriors name Gaussian " + std::to_string(post_idx[i]) + "; the accumulators have " + std::to_string(num_gauss));
  std::vector<int32_t> pair_frame((size_t)pairs);
  for (int64_t t = 0; t < rows; ++t)
    for (int32_t i = post_off[t]; i < post_off[t + 1]; ++i) pair_frame[i] = (int32_t)t;
  UseDevice(device, who_needs);
  feats.Upload(host_feats, (size_t)rows * dim * 4, "copy features");
  idx.Upload(post_idx, (size_t)pairs * 4, "copy the posterior indices");
  w.Upload(post_w, (size_t)pairs * 4, "copy the posteriors");
  frame.Upload(pair_frame, "copy the posteriors' frames");
  return pairs;
}

float GmmSparseAcc::Sort(const int32_t* d_gauss, int64_t pairs, bool timed) {
  const int32_t seg_off[2] = {0, (int32_t)pairs};
  EventTimer tm(timed);
  tm.Start();
  Check(sort.Run(d_gauss, pairs, seg_off, 1, num_gauss, nullptr), "bucket_sort launch");
  return timed ? tm.Stop() : 0.f;
}

float GmmSparseAcc::Accumulate(FgmmAccArgs a, const std::function<void(int64_t, size_t)>& refuse, hipError_t (*launch)(const FgmmAccArgs&, hipStream_t),
                               const char* launch_name, bool timed) {
  item_start.Reserve((size_t)(num_gauss + 1) * 4);
  a.dim = dim;
  a.num_gauss = num_gauss;
  a.flags = flags;
  a.item_start = item_start.as<int32_t>();
  a.occ = occ.as<double>();
  a.mean = mean.as<double>();
  a.cov = second.as<double>();
  // the grid and the partial sums are sized by a bound on the number of items, so that no count comes back between the launches:
  // a bucket that is not empty has at most one chunk that is not full
  const int64_t bound = a.pairs / kFgmmAccPairChunk + std::min<int64_t>(num_gauss, a.pairs);
  const size_t partial_bytes = (size_t)bound * (1 + dim + second_width) * 8;
  refuse(bound, partial_bytes);
  a.num_items = (int)bound;
  partial.Reserve(partial_bytes);
  a.partial = partial.as<double>();
  EventTimer tm(timed);
  tm.Start();
  Check(launch_fgmm_acc_items(a, nullptr), "fgmm_acc_items launch");
  Check(launch(a, nullptr), launch_name);
  return timed ? tm.Stop() : 0.f;
}

void GmmSparseAcc::Get(double* host_occ, double* host_mean, double* host_second, const char* second_what) const {
  UseDevice(device, who_needs);
  if (host_occ) occ.Download(host_occ, (size_t)num_gauss * 8, "copy the occupancies");
  if (host_mean) mean.Download(host_mean, (size_t)num_gauss * dim * 8, "copy the mean accumulators");
  if (host_second) second.Download(host_second, (size_t)num_gauss * second_width * 8, second_what);
}

}  // namespace xv
