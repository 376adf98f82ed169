#include "cmvn.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cmvn_kernels.h"
#include "device.h"
#include "kernels.h"

// CmvnNorm is compared with tests/cmvn_ref.py for equality: var = s / n - mean * mean in two roundings, not a fused one
#pragma clang fp contract(off)

namespace xv {
namespace {

const char kWhoNeeds[] = "the CMVN kernels need";

// The batch on the device: row offsets, the float rows (uploaded, or expanded from the stored objects) and the work items of
// the matrices that take part (keep == nullptr: all of them).
struct DeviceBatch {
  DevBuf feats, row_off, mat_item0, cm, cm_off;
  WorkItems items;
  std::vector<int32_t> h_item0;
  int n_items = 0;
  CmvnArgs args;
  DeviceBatch(const char* who, const float* host_feats, const int32_t* off, int n, int cols, const CmvnCompressed* c,
              const int32_t* keep) {
    CheckOffsets(who, off, n);
    h_item0.assign(1, 0);
    int max_rows = 0;
    for (int u = 0; u < n; ++u) {
      const int rows = off[u + 1] - off[u];
      max_rows = rows > max_rows ? rows : max_rows;
      if (!keep || keep[u] >= 0) items.Add(u, CeilDiv(rows, kCmvnRowBlock));
      h_item0.push_back(items.size());
    }
    n_items = items.size();
    const size_t total = (size_t)off[n] * cols;
    memset(&args, 0, sizeof args);
    row_off.Upload(off, (size_t)(n + 1) * 4, "copy row offsets");
    if (c && total) {
      if (cols > 64) throw KioError(std::string(who) + ": compressed input with more than 64 columns (the device expansion's limit)");
      if (!c->bytes || !c->off) throw KioError(std::string(who) + ": null compressed input");
      for (int u = 0; u < n; ++u) {
        const int rows = off[u + 1] - off[u];
        const size_t need = 16 + (size_t)cols * 8 + (size_t)rows * cols;
        int32_t rc[2];
        if (c->off[u] < 0 || (size_t)c->off[u] + need > c->nbytes) throw KioError(std::string(who) + ": compressed object out of bounds");
        memcpy(rc, c->bytes + c->off[u] + 8, 8);
        if (rc[0] != rows || rc[1] != cols) throw KioError(std::string(who) + ": compressed object does not have the shape of its matrix");
      }
      feats.Alloc(total * 4);
      cm.Upload(c->bytes, c->nbytes, "copy compressed features");
      cm_off.Upload(c->off, (size_t)n * 8, "copy object offsets");
      CmExpandArgs ca;
      ca.cm = cm.as<uint8_t>();
      ca.cm_off = cm_off.as<int64_t>();
      ca.raw_off = row_off.as<int32_t>();
      ca.n_utts = n;
      ca.dim = cols;
      ca.max_rows = max_rows;
      ca.out = feats.as<float>();
      Check(launch_cm_expand(ca, nullptr), "cm_expand launch");
    } else {
      if (total && !host_feats) throw KioError(std::string(who) + ": null input");
      feats.Upload(host_feats, total * 4, "copy features");
    }
    items.Upload();
    mat_item0.Upload(h_item0, "copy work items");
    args.feats = feats.as<float>();
    args.row_off = row_off.as<int32_t>();
    args.n = n;
    args.cols = cols;
    args.item_mat = items.d_unit.as<int32_t>();
    args.item_blk = items.d_blk.as<int32_t>();
    args.n_items = n_items;
    args.mat_item0 = mat_item0.as<int32_t>();
  }
};

}  // namespace

bool ParseSkipDims(const std::string& value, std::vector<int>* dims) {
  dims->clear();
  if (value.empty()) return true;
  size_t a = 0;
  for (;;) {
    const size_t b = value.find(':', a);
    const std::string t = value.substr(a, b == std::string::npos ? std::string::npos : b - a);
    if (t.empty() || t.size() > 6 || t.find_first_not_of("0123456789") != std::string::npos) return false;
    dims->push_back(atoi(t.c_str()));
    if (b == std::string::npos) return true;
    a = b + 1;
  }
}

int CmvnNorm(const double* stats, int cols, bool norm_means, bool norm_vars, bool reverse, const int* skip_dims, int n_skip,
             float* norm) {
  if (!stats || !norm || cols < 1 || n_skip < 0 || (n_skip && !skip_dims)) throw CmvnArgError("cmvn-norm: bad argument");
  if (norm_vars && !norm_means) throw CmvnArgError("You cannot normalize the variance but not the mean.");
  const double count = stats[cols];
  if (!(count >= 1.0)) {
    char buf[128];
    snprintf(buf, sizeof buf, "Insufficient stats for cepstral mean and variance normalization: count = %g", count);
    throw KioError(buf);
  }
  std::vector<char> skip((size_t)cols, 0);
  for (int i = 0; i < n_skip; ++i) {
    if (skip_dims[i] < 0 || skip_dims[i] >= cols)
      throw CmvnArgError("skip-dims: dimension " + std::to_string(skip_dims[i]) + " is out of range for " + std::to_string(cols) + " columns");
    skip[skip_dims[i]] = 1;
  }
  int floored = 0;
  for (int d = 0; d < cols; ++d) {
    if (!norm_means) {
      norm[d] = 0.f;
      norm[cols + d] = 1.f;
      continue;
    }
    const double s0 = skip[d] ? 0.0 : stats[d], s1 = skip[d] ? count : stats[cols + 1 + d];
    const double mean = s0 / count;
    double scale = 1.0, offset = reverse ? mean : -mean;
    if (norm_vars) {
      const double sq = s1 / count;
      const double m2 = mean * mean;
      double var = sq - m2;
      if (var < 1.0e-20) {
        var = 1.0e-20;
        ++floored;
      }
      if (reverse) {
        scale = sqrt(var);
      } else {
        scale = 1.0 / sqrt(var);
        const double ms = mean * scale;
        offset = -ms;
      }
    }
    norm[d] = (float)offset;
    norm[cols + d] = (float)scale;
  }
  return floored;
}

void CmvnStats(int device, const float* feats, const int32_t* row_off, int n, int cols, double* stats, float* device_ms,
               const CmvnCompressed* cm) {
  if (device_ms) *device_ms = 0.f;
  if (n < 0 || cols < 1 || !row_off || (n > 0 && !stats)) throw KioError("cmvn-stats: bad argument");
  if (n == 0) return;
  UseDevice(device, kWhoNeeds);
  DeviceBatch b("cmvn-stats", feats, row_off, n, cols, cm, nullptr);
  DevBuf partial, d_stats;
  partial.Alloc((size_t)b.n_items * 2 * cols * 8);
  const size_t sbytes = (size_t)n * 2 * (cols + 1) * 8;
  d_stats.Alloc(sbytes);
  b.args.partial = partial.as<double>();
  b.args.stats = d_stats.as<double>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_cmvn_stats(b.args, nullptr), "cmvn_stats launch");
  if (device_ms) *device_ms = tm.Stop();
  d_stats.Download(stats, sbytes, "copy statistics");
}

void CmvnApply(int device, const float* feats, const int32_t* row_off, int n, int cols, const float* norms, int n_norms,
               const int32_t* utt_norm, float* out, float* device_ms, const CmvnCompressed* cm) {
  if (device_ms) *device_ms = 0.f;
  if (n < 0 || cols < 1 || !row_off || n_norms < 0 || (n > 0 && !utt_norm)) throw KioError("cmvn-apply: bad argument");
  if (n == 0 || row_off[n] == 0) return;
  if (!out) throw KioError("cmvn-apply: null output");
  for (int u = 0; u < n; ++u)
    if (utt_norm[u] < -1 || utt_norm[u] >= n_norms) throw KioError("cmvn-apply: a matrix names a norm that is not in the table");
  if (n_norms > 0 && !norms) throw KioError("cmvn-apply: null norm table");
  UseDevice(device, kWhoNeeds);
  DeviceBatch b("cmvn-apply", feats, row_off, n, cols, cm, utt_norm);
  if (b.n_items == 0) return;
  const size_t bytes = (size_t)row_off[n] * cols * 4;
  DevBuf d_norms, d_utt_norm, d_out;
  d_norms.Upload(norms, (size_t)n_norms * 2 * cols * 4, "copy norms");
  d_utt_norm.Upload(utt_norm, (size_t)n * 4, "copy norm indices");
  d_out.Alloc(bytes);
  b.args.norms = d_norms.as<float>();
  b.args.utt_norm = d_utt_norm.as<int32_t>();
  b.args.out = d_out.as<float>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_cmvn_apply(b.args, nullptr), "cmvn_apply launch");
  if (device_ms) *device_ms = tm.Stop();
  // rows of the matrices that were left out hold nothing: only the others are copied back
  Check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  for (int u = 0; u < n; ++u) {
    if (utt_norm[u] < 0 || row_off[u + 1] == row_off[u]) continue;
    int v = u;
    while (v + 1 < n && utt_norm[v + 1] >= 0) ++v;   // one copy per run of kept matrices
    const size_t o = (size_t)row_off[u] * cols, e = (size_t)row_off[v + 1] * cols;
    Check(hipMemcpy(out + o, d_out.as<float>() + o, (e - o) * 4, hipMemcpyDeviceToHost), "copy normalised features");
    u = v;
  }
}

void CmvnApplySelect(int device, const float* feats, const int32_t* row_off, int n, int cols, const float* norms, int n_norms,
                     const int32_t* utt_norm, const int32_t* sel_row, const int32_t* sel_utt, int n_out, float* out, float* device_ms) {
  if (device_ms) *device_ms = 0.f;
  if (n < 0 || cols < 1 || !row_off || n_norms < 0 || n_out < 0 || (n > 0 && !utt_norm) || (n_out > 0 && (!sel_row || !sel_utt || !out)))
    throw KioError("cmvn-apply-select: bad argument");
  const int64_t rows = CheckOffsets("cmvn-apply-select", row_off, n);
  if (rows > 0 && !feats) throw KioError("cmvn-apply-select: null input");
  if (n_norms > 0 && !norms) throw KioError("cmvn-apply-select: null norm table");
  // the kernel trusts its tables: every kept row is a row of its utterance, and that utterance has a norm
  for (int i = 0; i < n_out; ++i) {
    const int u = sel_utt[i];
    if (u < 0 || u >= n || sel_row[i] < row_off[u] || sel_row[i] >= row_off[u + 1])
      throw KioError("cmvn-apply-select: a selected row is not a row of its utterance");
    if (utt_norm[u] < 0 || utt_norm[u] >= n_norms) throw KioError("cmvn-apply-select: a selected row's utterance names no norm of the table");
  }
  if (n_out == 0) return;
  UseDevice(device, kWhoNeeds);
  DevBuf d_feats, d_norms, d_utt_norm, d_row, d_utt, d_out;
  d_feats.Upload(feats, (size_t)rows * cols * 4, "copy features");
  d_norms.Upload(norms, (size_t)n_norms * 2 * cols * 4, "copy norms");
  d_utt_norm.Upload(utt_norm, (size_t)n * 4, "copy norm indices");
  d_row.Upload(sel_row, (size_t)n_out * 4, "copy selected rows");
  d_utt.Upload(sel_utt, (size_t)n_out * 4, "copy selected rows");
  d_out.Alloc((size_t)n_out * cols * 4);
  CmvnSelectArgs a;
  a.raw = d_feats.as<float>();
  a.cols = cols;
  a.norms = d_norms.as<float>();
  a.utt_norm = d_utt_norm.as<int32_t>();
  a.sel_row = d_row.as<int32_t>();
  a.sel_utt = d_utt.as<int32_t>();
  a.n_out = n_out;
  a.out = d_out.as<float>();
  EventTimer tm(device_ms != nullptr);
  tm.Start();
  Check(launch_cmvn_apply_select(a, nullptr), "cmvn_apply_select launch");
  if (device_ms) *device_ms = tm.Stop();
  Check(hipDeviceSynchronize(), "hipDeviceSynchronize");
  d_out.Download(out, (size_t)n_out * cols * 4, "copy normalised features");
}

}  // namespace xv
