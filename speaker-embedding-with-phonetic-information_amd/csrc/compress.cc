#include "compress.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include "compress_kernels.h"
#include "device.h"
#include "engine.h"
#include "kio.h"

namespace xv {

std::string CompressionMethodError(int method) {
  if (method == 1 || method == 2 || method == 3 || method == 5) return "";
  if (method == 4 || method == 6 || method == 7)
    return "compression method " + std::to_string(method) + " (a fixed range) is not built: 1 (automatic), 2 (speech feature), 3 (two bytes) and 5 (one byte) are";
  return "invalid compression method " + std::to_string(method);
}

bool CompressedSize(int rows, int cols, int method, size_t* nbytes, const char** format) {
  if (!CompressionMethodError(method).empty() || rows < 0 || cols < 0) return false;
  const char* f = "CM";
  size_t n = 16;
  if (rows > 0 && cols > 0) {
    const bool cm = method == 2 || (method == 1 && rows > 8);
    f = cm ? "CM" : method == 5 ? "CM3" : "CM2";
    n += cm ? (size_t)cols * 8 + (size_t)rows * cols : (size_t)rows * cols * (method == 5 ? 1 : 2);
  }
  if (nbytes) *nbytes = n;
  if (format) *format = f;
  return true;
}

void CompressMatrices(int device, const float* feats, const int32_t* row_off, int n, int cols, int method, uint8_t* out_bytes,
                      int64_t* out_off, int32_t* nonfinite, float* device_ms) {
  if (device_ms) *device_ms = 0.f;
  if (n < 0 || cols < 0 || !row_off || !out_off) throw KioError("compress: bad argument");
  const std::string bad = CompressionMethodError(method);
  if (!bad.empty()) throw KioError(bad);
  // the packed objects the caller gets, and the same with every start a multiple of 4 for the device (32-bit header stores)
  std::vector<int64_t> dev_off(n);
  int64_t dev_total = 0;
  out_off[0] = 0;
  WorkItems minmax, select, encode;
  for (int u = 0; u < n; ++u) {
    const int rows = row_off[u + 1] - row_off[u];
    if (rows < 0) throw KioError("compress: row offsets must not decrease");
    size_t nb = 0;
    CompressedSize(rows, cols, method, &nb, nullptr);
    out_off[u + 1] = out_off[u] + (int64_t)nb;
    dev_off[u] = dev_total;
    dev_total += ((int64_t)nb + 3) & ~(int64_t)3;
    if (nonfinite) nonfinite[u] = 0;
    if (rows == 0 || cols == 0) continue;
    if ((int64_t)rows * cols / kCmpMinmaxChunk >= INT32_MAX) throw KioError("compress: matrix too large");
    minmax.Add(u, CeilDiv((int64_t)rows * cols, kCmpMinmaxChunk));
    if (method == 2 || (method == 1 && rows > 8)) select.Add(u, CeilDiv(cols, kCmpSelectCols));
    encode.Add(u, CeilDiv(rows, kCmpEncodeRows));
  }
  if (n > 0 && out_off[n] > 0 && !out_bytes) throw KioError("compress: null output");
  std::vector<uint8_t> host((size_t)dev_total, 0);
  if (encode.size() > 0) {
    if (!feats) throw KioError("compress: null input");
    UseDevice(device, "the compression kernels need");
    DevBuf d_feats, d_row_off, d_obj_off, d_stats, d_out;
    const size_t total_rows = (size_t)row_off[n];
    d_feats.Upload(feats, total_rows * cols * 4, "copy features");
    d_row_off.Upload(std::vector<int32_t>(row_off, row_off + n + 1), "copy row offsets");
    d_obj_off.Upload(dev_off, "copy object offsets");
    CmpStats init;
    init.min_key = 0xffffffffu;
    init.max_key = 0u;
    init.nonfinite = 0u;
    init.pad = 0u;
    const std::vector<CmpStats> stats0((size_t)n, init);
    d_out.Alloc((size_t)dev_total);
    Check(hipMemset(d_out.p, 0, (size_t)dev_total), "hipMemset");   // the objects of empty matrices are 16 zero bytes
    minmax.Upload();
    select.Upload();
    encode.Upload();
    CmpArgs a;
    a.feats = d_feats.as<float>();
    a.row_off = d_row_off.as<int32_t>();
    a.obj_off = d_obj_off.as<int64_t>();
    a.out = d_out.as<uint8_t>();
    a.n = n;
    a.cols = cols;
    a.method = method;
    EventTimer tm(device_ms != nullptr);
    d_stats.Upload(stats0, "copy statistics");
    a.stats = d_stats.as<CmpStats>();
    tm.Start();
    a.item_mat = minmax.d_unit.as<int32_t>();
    a.item_blk = minmax.d_blk.as<int32_t>();
    a.n_items = minmax.size();
    Check(launch_cmp_minmax(a, nullptr), "minimum / maximum kernel launch");
    if (select.size() > 0) {
      a.item_mat = select.d_unit.as<int32_t>();
      a.item_blk = select.d_blk.as<int32_t>();
      a.n_items = select.size();
      Check(launch_cmp_select(a, nullptr), "selection kernel launch");
    }
    a.item_mat = encode.d_unit.as<int32_t>();
    a.item_blk = encode.d_blk.as<int32_t>();
    a.n_items = encode.size();
    Check(launch_cmp_encode(a, nullptr), "encode kernel launch");
    if (device_ms) *device_ms = tm.Stop();
    d_out.Download(host.data(), (size_t)dev_total, "copy objects");
    std::vector<CmpStats> stats((size_t)n);
    d_stats.Download(stats.data(), (size_t)n * sizeof(CmpStats), "copy statistics");
    for (int u = 0; u < n; ++u) {
      if (row_off[u + 1] == row_off[u]) continue;
      float range;
      memcpy(&range, host.data() + dev_off[u] + 4, 4);
      const bool finite_range = range - range == 0.f;
      if (nonfinite && (stats[u].nonfinite || !finite_range)) nonfinite[u] = 1;
    }
  }
  for (int u = 0; u < n; ++u) memcpy(out_bytes + out_off[u], host.data() + dev_off[u], (size_t)(out_off[u + 1] - out_off[u]));
}

void CmvnSliding(int device, const float* raw, const int32_t* raw_off, int n, int cols, int cmn_window, int min_cmn_window,
                 bool center, float* out) {
  if (n < 0 || !raw_off || cols < 1) throw KioError("cmvn-sliding: bad argument");
  if (cols > 64) throw KioError("cmvn-sliding: more than 64 feature columns (the device front-end's limit)");
  for (int u = 0; u < n; ++u)
    if (raw_off[u + 1] < raw_off[u] || raw_off[0] != 0) throw KioError("cmvn-sliding: row offsets must start at 0 and not decrease");
  const int rows = n > 0 ? raw_off[n] : 0;
  if (rows == 0) return;
  if (!raw || !out) throw KioError("cmvn-sliding: null buffer");
  // every row is kept: the selection lists are the identity
  std::vector<int32_t> sel_row((size_t)rows), sel_utt((size_t)rows);
  for (int u = 0; u < n; ++u)
    for (int r = raw_off[u]; r < raw_off[u + 1]; ++r) {
      sel_row[r] = r;
      sel_utt[r] = u;
    }
  UseDevice(device, "the feature front-end's kernels need");
  const FrontEndBytes z = FrontEndSizes(rows, n, rows, cols);
  DevBuf d_raw, d_prefix, d_out, d_tab;
  d_raw.Alloc(z.raw);
  d_prefix.Alloc(z.prefix);
  d_out.Alloc(z.out);
  d_tab.Alloc(z.tab);
  const FrontEndBuffers b = {d_raw.p, d_prefix.p, d_out.p, d_tab.p};
  FrontEndRun(nullptr, b, cols, raw, raw_off, n, sel_row.data(), sel_utt.data(), rows, cmn_window, center, min_cmn_window, out);
}

}  // namespace xv
