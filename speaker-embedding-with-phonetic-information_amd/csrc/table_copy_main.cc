// copy-feats / copy-vector - minimal equivalents of the Kaldi table-copy tools, built on kio.
//   copy-feats  [--binary=true|false] [--compress=true|false] [--compression-method=1|2|3|5] [--write-num-frames=<wspecifier>]
//               [--device=<gpu>] <matrix-rspecifier> <matrix-wspecifier>
//   copy-vector [--binary=true|false] <vector-rspecifier> <vector-wspecifier>
// They exist so that recipes and tests can move features / embeddings between ark, scp and text forms on a
// Kaldi-less box (the reference pipes features through such tools, extract_xvectors_new.sh:79), and they
// exercise every reader/writer path of kio (FM/DM/CM/CM2/CM3/text in; FM/FV/text, ark+scp out).
// --compress=true is honoured only in a process whose environment has XVEC_COMPRESS=1 (read once): the matrices
// are then read ahead in batches, compressed on the HIP device (compress.h) and written as CM / CM2 / CM3 objects, and without a
// GPU the tool fails (exit 255).  Without the switch --compress and --compression-method are accepted and ignored, the floats are
// written as they are and no device is touched.  A text wspecifier ignores --compress either way, as Kaldi does.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "cli.h"
#include "compress.h"
#include "kio.h"

namespace {

constexpr int64_t kBatchFrames = 1 << 18;   // frames read ahead per device call; one longer matrix is a batch of its own

// The matrices of one device call, written in table order once they are compressed.
struct CompressBatch {
  std::vector<std::string> keys;
  std::vector<float> feats;
  std::vector<int32_t> off = {0};
  int cols = -1;
  void Clear() {
    keys.clear();
    feats.clear();
    off.assign(1, 0);
    cols = -1;
  }
};

long FlushCompressed(const char* prog, int device, int method, CompressBatch* b, xv::TableWriter* w, xv::TableWriter* wn) {
  const int n = (int)b->keys.size();
  if (n == 0) return 0;
  std::vector<int64_t> out_off(n + 1);
  std::vector<int32_t> bad(n, 0);
  size_t total = 0;
  for (int u = 0; u < n; ++u) {
    size_t nb = 0;
    xv::CompressedSize(b->off[u + 1] - b->off[u], b->cols, method, &nb, nullptr);
    total += nb;
  }
  std::vector<uint8_t> bytes(total);
  xv::CompressMatrices(device, b->feats.data(), b->off.data(), n, b->cols, method, bytes.data(), out_off.data(), bad.data());
  long compressed = 0;
  for (int u = 0; u < n; ++u) {
    const int rows = b->off[u + 1] - b->off[u];
    if (bad[u]) {
      fprintf(stderr, "WARNING (%s) %s: the matrix holds a value that is not finite; writing it uncompressed\n", prog, b->keys[u].c_str());
      xv::Matrix m;
      m.rows = rows;
      m.cols = b->cols;
      m.data.assign(b->feats.begin() + (size_t)b->off[u] * b->cols, b->feats.begin() + (size_t)b->off[u + 1] * b->cols);
      w->WriteMat(b->keys[u], m);
    } else {
      const char* format = "CM";
      xv::CompressedSize(rows, b->cols, method, nullptr, &format);
      w->WriteCompressed(b->keys[u], format, bytes.data() + out_off[u], (size_t)(out_off[u + 1] - out_off[u]));
      ++compressed;
    }
    if (wn) wn->WriteInt32(b->keys[u], rows);
  }
  b->Clear();
  return compressed;
}

}  // namespace

int main(int argc, char** argv) {
  const char* prog = strrchr(argv[0], '/') ? strrchr(argv[0], '/') + 1 : argv[0];
  xv::InstallMappedFileFaultHandler(prog);
  const bool vectors = strstr(prog, "vector") != nullptr;
  try {
    std::vector<std::string> pos;
    std::string num_frames_wspecifier;   // copy-feats --write-num-frames=<int32 wspecifier> (steps/make_mfcc.sh:88: utt2num_frames)
    bool compress = false;
    int method = 1, device = -1;
    for (int i = 1; i < argc; ++i) {
      std::string a = argv[i];
      if (a.compare(0, 2, "--") == 0 && pos.empty()) {
        if (!vectors && a.compare(0, 19, "--write-num-frames=") == 0) num_frames_wspecifier = a.substr(19);
        if (!vectors && a == "--compress") compress = true;
        if (!vectors && a.compare(0, 11, "--compress=") == 0) compress = xv::ToBool("compress", a.substr(11));
        if (!vectors && a.compare(0, 21, "--compression-method=") == 0) method = xv::ToInt("compression-method", a.substr(21));
        if (!vectors && a.compare(0, 9, "--device=") == 0) device = xv::ToInt("device", a.substr(9));
        continue;  // the others: ark,t: / ark: in the wspecifier decides the form
      }
      pos.push_back(a);
    }
    if (pos.size() != 2) {
      fprintf(stderr, "Usage: %s [options] <rspecifier> <wspecifier>\n", prog);
      return 1;
    }
    // the switch of the process environment, read once; a text table is never compressed
    const char* sw = getenv("XVEC_COMPRESS");
    const bool honour = !vectors && compress && sw && strcmp(sw, "1") == 0 && xv::ParseWspecifier(pos[1]).binary;
    if (honour) {
      const std::string refused = xv::CompressionMethodError(method);
      if (!refused.empty()) throw xv::KioError(refused);
      device = xv::PickDevice(device);
    }
    xv::TableWriter w(pos[1]);
    long n = 0, bad = 0, compressed = 0;
    std::unique_ptr<xv::TableWriter> wn;
    if (!num_frames_wspecifier.empty()) wn.reset(new xv::TableWriter(num_frames_wspecifier));
    if (!vectors) {
      xv::SequentialMatrixReader r(pos[0]);
      std::string key, err;
      xv::Matrix m;
      CompressBatch batch;
      while (r.Next(&key, &m, &err)) {
        if (!err.empty()) {
          fprintf(stderr, "WARNING (%s) %s: %s\n", prog, key.c_str(), err.c_str());
          ++bad;
          continue;
        }
        ++n;
        if (!honour) {
          w.WriteMat(key, m);
          if (wn) wn->WriteInt32(key, m.rows);
          continue;
        }
        const int cols = m.rows > 0 ? m.cols : 0;   // a matrix without rows joins any batch
        if (batch.cols >= 0 && cols != 0 && cols != batch.cols) compressed += FlushCompressed(prog, device, method, &batch, &w, wn.get());
        if (cols != 0 || batch.cols < 0) batch.cols = cols;
        batch.keys.push_back(key);
        if (cols != 0) batch.feats.insert(batch.feats.end(), m.Data(), m.Data() + (size_t)m.rows * m.cols);
        batch.off.push_back(batch.off.back() + (cols != 0 ? m.rows : 0));
        if (batch.off.back() >= kBatchFrames) compressed += FlushCompressed(prog, device, method, &batch, &w, wn.get());
      }
      compressed += FlushCompressed(prog, device, method, &batch, &w, wn.get());
    } else {
      // vectors: a vector table is read through the matrix reader's text/binary object layer
      xv::RspecifierOptions o = xv::ParseRspecifier(pos[0]);
      if (o.is_scp) {
        xv::RandomAccessVectorReader rr(pos[0]);
        xv::Input in;
        in.Open(o.rxfilename);
        std::string line;
        int c;
        while ((c = in.Get()) >= 0) {
          if (c != '\n') {
            line.push_back((char)c);
            continue;
          }
          size_t sp = line.find_first_of(" \t");
          std::string key = line.substr(0, sp);
          if (!key.empty()) {
            const std::vector<float>& v = rr.Value(key);
            w.WriteVec(key, v.data(), (int)v.size());
            ++n;
          }
          line.clear();
        }
      } else {
        xv::SequentialVectorReader rd(pos[0]);
        std::string key, err;
        std::vector<float> v;
        while (rd.Next(&key, &v, &err)) {
          w.WriteVec(key, v.data(), (int)v.size());
          ++n;
        }
      }
    }
    w.Close();
    if (wn) wn->Close();
    if (compress && !vectors) {
      if (honour)
        fprintf(stderr, "LOG (%s) --compress=true honoured (XVEC_COMPRESS=1, method %d, device %d): compressed %ld matrices\n", prog, method,
                device, compressed);
      else
        fprintf(stderr, "LOG (%s) --compress=true ignored (%s): compressed 0 matrices\n", prog,
                xv::ParseWspecifier(pos[1]).binary ? "XVEC_COMPRESS is not 1" : "a text table");
    }
    fprintf(stderr, "LOG (%s) Copied %ld %s%s\n", prog, n, vectors ? "vectors" : "feature matrices",
            bad ? " (some entries failed)" : "");
    return n > 0 ? 0 : 1;
  } catch (const std::exception& e) {
    fprintf(stderr, "ERROR (%s) %s\n", prog, e.what());
    return -1;
  }
}
