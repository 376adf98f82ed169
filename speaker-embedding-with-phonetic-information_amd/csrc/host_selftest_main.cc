// Host-only self test of the parsers that face untrusted input (model files, feature / vector archives), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by `make sanitize` (plain g++, no HIP: kio.cc, nnet3_raw.cc,
// program.cc, feat_batch.cc, cli.cc have no device dependency).  GPU AddressSanitizer is not available on the target pool, so this is where
// memory errors of the host layer are caught.
//
//   host_selftest <model.raw> <output-node> <features.ark> [variants per kind, default 200]
//
// 1. parses the model, lowers it, re-emits it and parses the copy again;
// 2. reads the archive and re-writes it through the table writer in binary and text form;
// 2b. binary archives: the index pass of the parallel table readers (MatrixTableIndexer + ReadIndexedMatrix) must deliver
//     exactly what the sequential reader delivers, through the archive itself and through a script file of its offsets;
// 3. replays both files truncated at `variants` positions and with 1.5 x `variants` single bits flipped: every variant must either parse or
//    throw KioError - never crash, hang or trip a sanitizer.
//
//   host_selftest walk <dir>
//
// runs the feature-batch walk, the keyed lookups and the joins of feat_batch.h / feat_join.h over the cases <dir>/walk_cases.txt
// names and prints one line per event - batch boundaries, join outcomes, the groups handed on (tests/test_feat_walk_host.py
// computes the same dump from the inputs).
//
//   host_selftest tables <dir>
//
// reads every table <dir>/cases.txt names through the reader the line names and prints one line per event - key, dimensions
// and a 64-bit hash of the value's bytes, or the error text - so that what the table readers deliver is pinned byte for byte
// (tests/test_table_readers.py compares the dump with the one recorded under tests/golden/table_readers/).
//
//   host_selftest gemm_plan
//
// sweeps the GEMM launch planner (gemm_plan.cc: plain host code, no device) over shapes, modes, CU counts and knobs.
//
//   host_selftest cli <path of a config file to write>
//
// drives a synthetic tool table (cli.h: one option of every kind, under each combination of the tool properties) through the
// option lookup with well-formed, malformed, empty, underscore-spelled, unknown and refused input, then through CliMain with a
// --config file and through the three name rules of ToolsMain.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "batch_source.h"
#include "cli.h"
#include "feat_join.h"
#include "gemm_plan.h"
#include "kio.h"
#include "nnet3_raw.h"
#include "program.h"

namespace {

std::string Slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::ostringstream o;
  o << f.rdbuf();
  return o.str();
}

// returns 0 parsed, 1 rejected with KioError
int TryModel(const std::string& bytes, const std::string& node) {
  try {
    xv::RawNnet net;
    net.Read(bytes);
    if (!node.empty()) net.ApplyNnetConfig("output-node name=output input=" + node + "\n");
    xv::TdnnProgram p = xv::LowerToProgram(net, "output");
    (void)p.Describe();
    (void)p.Macs(400);
    return 0;
  } catch (const xv::KioError&) {
    return 1;
  } catch (const std::bad_alloc&) {
    return 1;   // an absurd dimension in a corrupted header
  } catch (const std::length_error&) {
    return 1;
  }
}

int TryArchive(const std::string& bytes) {
  try {
    xv::Input in;
    in.OpenMemory(bytes.data(), bytes.size());
    for (int n = 0; n < 100000; ++n) {
      std::string key;
      if (!xv::ReadKey(in, &key)) break;
      const bool binary = xv::ReadBinaryHeader(in);
      xv::Matrix m;
      xv::ReadMatrix(in, binary, &m);
    }
    return 0;
  } catch (const xv::KioError&) {
    return 1;
  } catch (const std::bad_alloc&) {
    return 1;
  } catch (const std::length_error&) {
    return 1;
  }
}

// The indexed readers against the sequential one: same keys, same matrices, same order.  Returns 0 ok, 1 mismatch,
// 2 "not addressable" (text archive: the caller checks that this is what usable() says).
int CheckIndexer(const std::string& rspec, const std::string& seq_rspec, long* views) {
  xv::FileMapper mapper;
  xv::MatrixTableIndexer idx(rspec);
  if (!idx.usable()) return 2;
  xv::SequentialMatrixReader rd(seq_rspec);
  xv::ArchiveCursor cursor;
  std::string key, err;
  xv::Matrix want, got;
  xv::MatrixTableIndexer::Entry e;
  for (;;) {
    const bool a = idx.Next(&e), b = rd.Next(&key, &want, &err);
    if (a != b) return 1;
    if (!a) return 0;
    if (!e.error.empty() || !err.empty() || e.key != key) return 1;
    xv::ReadIndexedMatrix(e, &cursor, &got);
    if (got.rows != want.rows || got.cols != want.cols || got.data != want.data) return 1;
    if (e.rows >= 0 && (e.rows != want.rows || e.cols != want.cols)) return 1;
    // the VIEW of the same object in the mapped file (what the reader threads of a table job hand out): a binary float matrix
    // must be viewable and hold the same bytes (compared with memcmp: the view has the archive's alignment, not a float's)
    xv::Matrix view;
    if (mapper.View(e, &view, true)) {
      ++*views;
      if (view.rows != want.rows || view.cols != want.cols || !view.data.empty()) return 1;
      if (view.cm) {   // a compressed view: what the device front-end uploads; expanded here it is what the reader delivers
        xv::Matrix full;
        xv::ExpandCompressedView(view, &full);
        if (full.rows != want.rows || full.cols != want.cols || full.data != want.data) return 1;
      } else if (memcmp(view.Data(), want.data.data(), want.data.size() * sizeof(float)) != 0) {
        return 1;
      }
    }
  }
}

// a damaged archive through the index pass: every variant either indexes + reads or throws KioError
int TryIndexedFile(const std::string& path) {
  try {
    xv::MatrixTableIndexer idx("ark:" + path);
    if (!idx.usable()) return 1;
    xv::ArchiveCursor cursor;
    xv::MatrixTableIndexer::Entry e;
    xv::Matrix m;
    xv::FileMapper mapper;
    for (int n = 0; n < 100000 && idx.Next(&e); ++n) {
      xv::Matrix view;
      if (mapper.View(e, &view, true) && (long)view.rows * view.cols > 0) {   // a view of a damaged file must stay inside the file
        if (view.cm) {
          xv::Matrix full;
          xv::ExpandCompressedView(view, &full);   // touches every byte of the object
        } else {
          volatile unsigned char first = *(const unsigned char*)view.Data();
          volatile unsigned char last = ((const unsigned char*)view.Data())[(size_t)view.rows * view.cols * 4 - 1];
          (void)first;
          (void)last;
        }
      }
      xv::ReadIndexedMatrix(e, &cursor, &m);
    }
    return 0;
  } catch (const xv::KioError&) {
    return 1;
  } catch (const std::bad_alloc&) {
    return 1;
  } catch (const std::length_error&) {
    return 1;
  }
}

// ------------------------------------------------------------------------------------- host_selftest tables <dir>
// FNV-1a over the value's bytes
struct Hash {
  uint64_t h = 1469598103934665603ull;
  void Add(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  }
  void AddInt(int32_t v) { Add(&v, 4); }
};

std::string Describe(const xv::Matrix& m) {
  Hash h;
  h.Add(m.Data(), (size_t)m.rows * m.cols * sizeof(float));
  char buf[64];
  snprintf(buf, sizeof buf, "%dx%d\t%016llx", m.rows, m.cols, (unsigned long long)h.h);
  return buf;
}
std::string Describe(const std::vector<float>& v) {
  Hash h;
  h.Add(v.data(), v.size() * sizeof(float));
  char buf[64];
  snprintf(buf, sizeof buf, "%zu\t%016llx", v.size(), (unsigned long long)h.h);
  return buf;
}
std::string Describe(int rows, int cols, const std::vector<double>& v) {
  Hash h;
  h.Add(v.data(), v.size() * sizeof(double));
  char buf[64];
  snprintf(buf, sizeof buf, "%dx%d\t%016llx", rows, cols, (unsigned long long)h.h);
  return buf;
}
std::string Describe(const xv::IntVecVec& v) {
  Hash h;
  size_t total = 0;
  for (const auto& l : v) {
    h.AddInt((int32_t)l.size());
    h.Add(l.data(), l.size() * 4);
    total += l.size();
  }
  char buf[64];
  snprintf(buf, sizeof buf, "%zu/%zu\t%016llx", v.size(), total, (unsigned long long)h.h);
  return buf;
}
std::string Describe(const xv::Posterior& p) {
  Hash h;
  size_t total = 0;
  for (const auto& frame : p) {
    h.AddInt((int32_t)frame.size());
    for (const auto& e : frame) {
      h.AddInt(e.first);
      h.Add(&e.second, 4);
    }
    total += frame.size();
  }
  char buf[64];
  snprintf(buf, sizeof buf, "%zu/%zu\t%016llx", p.size(), total, (unsigned long long)h.h);
  return buf;
}

void Event(const std::string& tag, const std::string& key, const std::string& what) {
  printf("%s\t%s\t%s\n", tag.c_str(), key.c_str(), what.c_str());
}

// kSorted: the readers of Gaussian selections and posteriors also say whether the rspecifier promised sorted keys
template <class Reader, class Value, bool kSorted = false>
void DumpSequential(const std::string& tag, const std::string& rspec) {
  Reader rd(rspec);
  if constexpr (kSorted) Event(tag, "-", std::string("sorted\t") + (rd.sorted() ? "1" : "0"));
  std::string key, err;
  Value v;
  while (rd.Next(&key, &v, &err)) Event(tag, key, err.empty() ? Describe(v) : "error\t" + err);
  Event(tag, "-", "close\t" + std::to_string(rd.Close()));
}

// the index pass, the read of every entry it located and the view of the same object in the mapped file
void DumpIndexed(const std::string& tag, const std::string& rspec) {
  xv::MatrixTableIndexer idx(rspec);
  Event(tag, "-", std::string("usable\t") + (idx.usable() ? "1" : "0"));
  if (!idx.usable()) return;
  xv::FileMapper mapper;
  xv::ArchiveCursor cursor;
  xv::MatrixTableIndexer::Entry e;
  while (idx.Next(&e)) {
    char where[96];
    snprintf(where, sizeof where, "\toffset=%ld\trows=%d\tcols=%d", e.offset, e.rows, e.cols);
    Event(tag, e.key, "rx=" + e.rx + where);
    if (!e.error.empty()) {
      Event(tag, e.key, "error\t" + e.error);
      continue;
    }
    try {
      xv::Matrix m, view;
      xv::ReadIndexedMatrix(e, &cursor, &m);
      Event(tag, e.key, Describe(m));
      if (!mapper.View(e, &view, true)) {
        Event(tag, e.key, "view\tnone");
      } else if (view.cm) {
        xv::Matrix full;
        xv::ExpandCompressedView(view, &full);
        Event(tag, e.key, "view\tcompressed\t" + Describe(full));
      } else {
        Event(tag, e.key, "view\tfloat\t" + Describe(view));
      }
    } catch (const std::exception& ex) {
      Event(tag, e.key, std::string("thrown\t") + ex.what());
    }
  }
}

// ops: "has:KEY", "value:KEY", "forget:KEY", in the order given
template <class Reader, class Fn>
void DumpRandomAccess(const std::string& tag, const std::string& rspec, const std::vector<std::string>& ops, Fn value) {
  Reader rd(rspec);
  for (const std::string& op : ops) {
    const size_t c = op.find(':');
    const std::string what = op.substr(0, c), key = op.substr(c + 1);
    try {
      if (what == "has") Event(tag, key, std::string("has\t") + (rd.HasKey(key) ? "1" : "0"));
      else Event(tag, key, what + "\t" + value(rd, what, key));
    } catch (const std::exception& ex) {
      Event(tag, key, what + "\tthrown\t" + ex.what());
    }
  }
}

template <class Map, class Fn>
void DumpMap(const std::string& tag, const Map& table, Fn text) {
  std::vector<std::string> keys;
  for (const auto& kv : table) keys.push_back(kv.first);
  std::sort(keys.begin(), keys.end());
  for (const std::string& k : keys) Event(tag, k, text(table.at(k)));
}

std::vector<std::string> SplitTabs(const std::string& s) {
  std::vector<std::string> out;
  size_t a = 0;
  for (;;) {
    const size_t b = s.find('\t', a);
    out.push_back(s.substr(a, b == std::string::npos ? b : b - a));
    if (b == std::string::npos) return out;
    a = b + 1;
  }
}

int RunTables(const char* dir) {
  if (chdir(dir) != 0) {
    fprintf(stderr, "host_selftest: cannot enter %s\n", dir);
    return 2;
  }
  std::ifstream cases("cases.txt");
  if (!cases) {
    fprintf(stderr, "host_selftest: no cases.txt in %s\n", dir);
    return 2;
  }
  std::string line;
  while (std::getline(cases, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::vector<std::string> f = SplitTabs(line);
    if (f.size() < 2) {
      fprintf(stderr, "host_selftest: bad line in cases.txt: %s\n", line.c_str());
      return 2;
    }
    const std::string reader = f[0], rspec = f[1], tag = reader + "\t" + rspec;
    const std::vector<std::string> ops(f.begin() + 2, f.end());
    try {
      if (reader == "seq-matrix") DumpSequential<xv::SequentialMatrixReader, xv::Matrix>(tag, rspec);
      else if (reader == "seq-vector") DumpSequential<xv::SequentialVectorReader, std::vector<float>>(tag, rspec);
      else if (reader == "seq-gselect") DumpSequential<xv::SequentialGselectReader, xv::IntVecVec, true>(tag, rspec);
      else if (reader == "seq-posterior") DumpSequential<xv::SequentialPosteriorReader, xv::Posterior, true>(tag, rspec);
      else if (reader == "indexed") DumpIndexed(tag, rspec);
      else if (reader == "ra-vector")
        DumpRandomAccess<xv::RandomAccessVectorReader>(tag, rspec, ops, [](xv::RandomAccessVectorReader& rd, const std::string& what, const std::string& key) {
          if (what == "forget") {
            rd.Forget(key);
            return std::string("done");
          }
          return Describe(rd.Value(key));
        });
      else if (reader == "ra-double-matrix")
        DumpRandomAccess<xv::RandomAccessDoubleMatrixReader>(tag, rspec, ops, [](xv::RandomAccessDoubleMatrixReader& rd, const std::string&, const std::string& key) {
          const auto& v = rd.Value(key);
          return Describe(v.rows, v.cols, v.data);
        });
      else if (reader == "int32") DumpMap(tag, xv::ReadInt32Table(rspec), [](int32_t v) { return std::to_string(v); });
      else if (reader == "float")
        DumpMap(tag, xv::ReadFloatTable(rspec), [](float v) {
          char buf[32];
          snprintf(buf, sizeof buf, "%.9g", v);
          return std::string(buf);
        });
      else if (reader == "token") DumpMap(tag, xv::ReadTokenTable(rspec), [](const std::string& v) { return v; });
      else if (reader == "token-list")
        for (const xv::TokenList& e : xv::ReadTokenVectorTable(rspec)) {
          std::string all;
          for (const std::string& t : e.tokens) all += (all.empty() ? "" : " ") + t;
          Event(tag, e.key, std::to_string(e.tokens.size()) + "\t" + all);
        }
      else {
        fprintf(stderr, "host_selftest: unknown reader %s in cases.txt\n", reader.c_str());
        return 2;
      }
    } catch (const std::exception& ex) {
      Event(tag, "-", std::string("thrown\t") + ex.what());
    }
  }
  return 0;
}

// --------------------------------------------------------------------------------------- host_selftest walk <dir>
template <class V>
std::string Join(const V& v) {
  std::ostringstream o;
  for (size_t i = 0; i < v.size(); ++i) o << (i ? "," : "") << v[i];
  return o.str();
}
template <class T>
std::string HashOf(const std::vector<T>& v) {
  Hash h;
  h.Add(v.data(), v.size() * sizeof(T));
  char buf[32];
  snprintf(buf, sizeof buf, "%016llx", (unsigned long long)h.h);
  return buf;
}
std::string Outcome(const xv::Joined& j) {
  const char* names[] = {"ok", "not-found", "wrong-size", "ragged"};
  return std::string(names[j.outcome]) + "\tsize=" + std::to_string(j.size) + "\twidth=" + std::to_string(j.width);
}

// One case per line of <dir>/walk_cases.txt, fields separated by tabs; every case prints its line first.
//   batches <read-ahead> <policy 0|1|2> <feats>:          the batches of the walk, then the number of entries counted as errors
//   groups <read-ahead> <dim> <num-gauss> <feats> <gselect or ->:   the groups of the packer, then its count
//   join-gselect <read-ahead> <feats> <gselect>:           FindGselect for every key of every batch
//   join-post <read-ahead> <feats> <post>:                 FindFrames for every key, and per batch what Append made of the accepted
// The warnings go to stderr, as in the tools.
int RunWalk(const char* dir) {
  if (chdir(dir) != 0) {
    fprintf(stderr, "host_selftest: cannot enter %s\n", dir);
    return 2;
  }
  std::ifstream cases("walk_cases.txt");
  std::string line;
  while (std::getline(cases, line)) {
    if (line.empty() || line[0] == '#') continue;
    const std::vector<std::string> f = SplitTabs(line);
    printf("case\t%s\n", line.c_str());
    try {
      const int64_t ahead = f.size() > 1 ? atol(f[1].c_str()) : 0;
      auto boundary = [](const xv::FeatBatchReader::Batch& b) {
        printf("batch\tkeys=%s\tcols=%d\trow_off=%s\n", Join(b.keys).c_str(), b.cols, Join(b.row_off).c_str());
      };
      if (f[0] == "batches" && f.size() == 4) {
        xv::FeatBatchWalk walk(f[3], ahead, false, (xv::FeatProblems)atoi(f[2].c_str()));
        printf("errors\t%ld\n", walk.Run(boundary));
      } else if (f[0] == "groups" && f.size() == 6) {
        xv::GselectGroupWalk walk(atoi(f[2].c_str()), atoi(f[3].c_str()), f[4], f[5] == "-" ? "" : f[5], ahead);
        printf("errors\t%ld\n", walk.Run([](const xv::GselectGroup& g) {
          printf("group\twidth=%d\tkeys=%s\toff=%s\tfeats=%s\tgs=%s\n", g.n, Join(g.keys).c_str(), Join(g.off).c_str(), HashOf(g.feats).c_str(), HashOf(g.gs).c_str());
        }));
      } else if (f[0] == "join-gselect" && f.size() == 4) {
        xv::FeatBatchWalk walk(f[2], ahead, false, xv::FeatProblems::kCount);
        xv::GselectLookup table(f[3]);
        walk.Run([&](const xv::FeatBatchReader::Batch& b) {
          boundary(b);
          for (size_t u = 0; u < b.keys.size(); ++u) {
            xv::IntVecVec sel;
            Event("join", b.keys[u], Outcome(xv::FindGselect(&table, b.keys[u], b.row_off[u + 1] - b.row_off[u], &sel)));
          }
        });
      } else if (f[0] == "join-post" && f.size() == 4) {
        xv::FeatBatchWalk walk(f[2], ahead, false, xv::FeatProblems::kCount);
        xv::PosteriorLookup table(f[3]);
        walk.Run([&](const xv::FeatBatchReader::Batch& b) {
          boundary(b);
          std::vector<int32_t> post_off(1, 0), post_idx;
          std::vector<float> post_w, feats;
          for (size_t u = 0; u < b.keys.size(); ++u) {
            xv::Posterior p;
            const xv::Joined j = xv::FindFrames(&table, b.keys[u], b.row_off[u + 1] - b.row_off[u], &p);
            Event("join", b.keys[u], Outcome(j));
            if (j.outcome != xv::Joined::kOk) continue;
            xv::Append(p, &post_off, &post_idx, &post_w);
            xv::AppendRows(b, u, &feats);
          }
          printf("post\tpost_off=%s\tpost_idx=%s\tpost_w=%s\tfeats=%s\n", Join(post_off).c_str(), HashOf(post_idx).c_str(), HashOf(post_w).c_str(), HashOf(feats).c_str());
        });
      } else {
        fprintf(stderr, "host_selftest: bad line in walk_cases.txt: %s\n", line.c_str());
        return 2;
      }
    } catch (const std::exception& ex) {
      printf("thrown\t%s\n", ex.what());
    }
    fflush(stdout);
  }
  return 0;
}

// PlanGemm over walks x shapes x precisions x epilogues x p8 x split-K x CU counts x knobs: whatever it is asked, a plan stays
// inside GemmArgs (at most 2 * kMaxSeg groups) and a launch it accepts has a grid, a block and an LDS size a CU holds.
int RunGemmPlan() {
  static char mem[64];   // addresses to tell sources apart by; never dereferenced
  struct S {
    int src, ld, shift, ksteps;
  };
  const std::vector<std::vector<S>> walks = {
      {{0, 64, -3, 1}, {0, 64, 0, 1}, {0, 64, 3, 1}, {1, 96, 1, 2}},
      {{0, 32, -4, 1}, {0, 32, 0, 1}, {1, 64, 0, 1}, {0, 32, 4, 1}, {1, 64, -2, 1}, {1, 64, 2, 1}, {1, 64, 6, 1}, {0, 32, 15, 1}},
      {{0, 128, 0, 4}, {1, 128, 0, 4}, {2, 128, 0, 4}, {3, 128, 0, 4}, {4, 128, 0, 4}, {5, 128, 0, 4}, {6, 128, 0, 4}, {7, 128, 0, 4}},   // 8 + 8 groups
      {{0, 256, -2, 8}, {0, 256, 2, 8}},
      {{0, 128, -2, 4}, {0, 128, 0, 4}, {0, 128, 2, 4}, {1, 64, 1, 2}, {1, 64, 4, 2}},
      {{0, 1536, 0, 48}},
  };
  long plans = 0, accepted = 0;
  for (const auto& w : walks)
    for (int mt : {1, 2, 3, 8, 22, 64, 300})
      for (int nt : {1, 2, 3, 4, 6, 12})
        for (int prec = -1; prec <= 10; ++prec)
          for (int epi = 0; epi <= 3; ++epi)
            for (int mode = 0; mode < 4; ++mode)   // plain, p8, split-K, planes missing
              for (int cus : {0, 7, 8, 16, 64, 120, 256, 304})
                for (int knobs = 0; knobs < 5; ++knobs) {
                  xv::GemmArgs a;
                  memset(&a, 0, sizeof a);
                  a.nseg = (int)w.size();
                  for (int j = 0; j < a.nseg; ++j) {
                    a.seg[j].hi = (const uint16_t*)(mem + 8 * w[j].src);
                    a.seg[j].ld = w[j].ld;
                    a.seg[j].row_shift = w[j].shift;
                    a.seg[j].ksteps = w[j].ksteps;
                    a.total_ksteps += w[j].ksteps;
                    if (mode != 3) {
                      a.seg[j].gmax = (const unsigned*)mem;
                      a.seg[j].lo4 = a.seg[j].lo4s = (const uint8_t*)mem;
                    }
                  }
                  a.m_tiles = mt;
                  a.n_tiles = nt;
                  if (mode != 3) {
                    a.w4 = a.w4_scale = a.w4b = a.w4b_scale = (const uint8_t*)mem;
                    a.out_lo4 = a.out_lo4s = (uint8_t*)mem;
                    a.ldw4 = a.ldw4b = 64;
                  }
                  a.p8 = mode == 1;
                  a.p8_whole = knobs % 3;
                  if (mode == 2) {
                    a.ksteps_per_slice = xv::SplitKStepsPerSlice(a.total_ksteps);
                    a.ksplit = (a.total_ksteps + a.ksteps_per_slice - 1) / a.ksteps_per_slice;
                    a.splitk_ws = (float*)mem;
                  }
                  const xv::GemmPolicy pol = knobs == 0 ? xv::DefaultGemmPolicy(cus) : xv::MakeGemmPolicy(cus, knobs, 4 * (knobs & 3), knobs - 1, 50 * knobs);
                  const xv::GemmPlan p = xv::PlanGemm(a, prec, epi, pol);
                  ++plans;
                  const xv::GemmArgs& b = p.args;
                  bool ok = b.ngrp >= 0 && b.ngrp_lo >= 0 && b.ngrp + b.ngrp_lo <= 2 * xv::kMaxSeg;
                  if (p.ok) {
                    ++accepted;
                    char name[96];
                    xv::GemmKernelName(p, name, sizeof name);
                    ok = ok && p.grid_x >= 1 && p.grid_y >= 1 && (p.block == 256 || p.block == 512) && p.lds > 0 && p.lds <= xv::kGemmMaxLds && strlen(name) > 16;
                    if (p.sk_ws_bytes) ok = ok && cus >= 8 && p.grid_x <= cus && b.sk_lanes >= 1 && p.grid_x % (8 * b.sk_lanes) == 0 && b.sk_mtiles >= 1;
                  }
                  if (!ok) {
                    fprintf(stderr, "host_selftest: bad plan (walk of %d, %d x %d tiles, precision %d, epilogue %d, mode %d, %d CUs, knobs %d)\n", a.nseg, mt,
                            nt, prec, epi, mode, cus, knobs);
                    return 1;
                  }
                }
  // the predicates the engine calls are defined on the same group builder and must not walk past kMaxSeg segments either
  xv::GemmArgs a;
  memset(&a, 0, sizeof a);
  for (int nseg : {-1, 0, 9, 1000}) {
    a.nseg = nseg;
    if (xv::gemm_mx_applicable(a) || xv::gemm_mx2_applicable(a) || xv::gemm_p8_applicable(a, xv::kPrecFp16)) return 1;
  }
  printf("host_selftest: gemm_plan ok (%ld plans, %ld accepted)\n", plans, accepted);
  return accepted > 0 && accepted < plans ? 0 : 1;
}

// What SetOption makes of --name=value: 'k' ok, 'u' unknown, 'b' a bad value, 't' thrown.
char Outcome(const xv::CliTool& tool, const std::string& name, const std::string& value, std::string* what = nullptr) {
  try {
    const xv::OptionResult r = xv::SetOption(tool, name, value);
    return r == xv::OptionResult::kOk ? 'k' : r == xv::OptionResult::kUnknown ? 'u' : 'b';
  } catch (const xv::KioError& e) {
    if (what) *what = e.what();
    return 't';
  }
}

int RunCli(const std::string& config_path) {
  int failures = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok) fprintf(stderr, "host_selftest: cli: %s\n", what), ++failures;
  };
  for (int props = 0; props < 8; ++props) {
    bool b = false;
    int i = 0, lax = 0, any = 0;
    float f = 0.f;
    double d = 0.0;
    std::string s, last;
    uint64_t seed = 0;
    xv::CliTool t = {"synthetic", "Usage: synthetic\n",
                     {xv::Bool("a-bool", &b), xv::Int("an-int", &i), xv::Float("a-float", &f), xv::Double("a-double", &d), xv::String("a-string", &s),
                      xv::Seed("a-seed", &seed), xv::LaxInt("lax-int", &lax), xv::Ignored("ignored"), xv::Int("dropped-int", nullptr),
                      xv::Bool("dropped-bool", nullptr), xv::Double("dropped-double", nullptr), xv::Refused("refused", "--refused is refused"),
                      xv::RefusedIfTrue("not-true", "--not-true=true is refused"), xv::RefusedIfNonZero("only-zero", "--only-zero is refused"),
                      xv::Custom("even", [](const std::string&, const std::string& v) { return !v.empty() && (v.back() - '0') % 2 == 0; }),
                      xv::Custom("", [&](const std::string& n, const std::string& v) { return n.compare(0, 4, "any-") == 0 ? (last = n + "=" + v, ++any, true) : false; })},
                     0, -1, [](const std::vector<std::string>&) { return 0; }};
    t.underscores = (props & 1) != 0;
    t.bad_value_line = (props & 2) != 0;
    t.config_file = (props & 4) != 0;
    const char bad = t.bad_value_line ? 'b' : 't';
    // well-formed
    expect(Outcome(t, "a-bool", "") == 'k' && b, "an empty boolean is true");
    expect(Outcome(t, "a-bool", "false") == 'k' && !b, "a-bool=false");
    expect(Outcome(t, "an-int", "-12") == 'k' && i == -12, "an-int=-12");
    expect(Outcome(t, "a-float", "0.5") == 'k' && f == 0.5f, "a-float=0.5");
    expect(Outcome(t, "a-double", "1e-3") == 'k' && d == 1e-3, "a-double=1e-3");
    expect(Outcome(t, "a-string", "x=y") == 'k' && s == "x=y", "a-string");
    expect(Outcome(t, "a-seed", "18446744073709551615") == 'k' && seed == UINT64_MAX, "a-seed");
    expect(Outcome(t, "lax-int", "7up") == 'k' && lax == 7 && Outcome(t, "lax-int", "abc") == 'k' && lax == 0, "lax-int takes anything");
    expect(Outcome(t, "ignored", "whatever") == 'k', "ignored");
    expect(Outcome(t, "dropped-int", "3") == 'k' && Outcome(t, "dropped-bool", "t") == 'k' && Outcome(t, "dropped-double", "2.5") == 'k', "dropped, well-formed");
    expect(Outcome(t, "not-true", "false") == 'k' && Outcome(t, "only-zero", "0") == 'k' && Outcome(t, "even", "42") == 'k', "not refused");
    expect(Outcome(t, "any-thing", "1") == 'k' && any == 1 && last == "any-thing=1", "the nameless escape hatch");
    // malformed and empty
    std::string what;
    expect(Outcome(t, "a-bool", "maybe", &what) == bad && (bad == 'b' || what == "Invalid format for boolean argument --a-bool=maybe"), "a-bool=maybe");
    expect(Outcome(t, "an-int", "1x", &what) == bad && (bad == 'b' || what == "Invalid integer option --an-int=1x"), "an-int=1x");
    expect(Outcome(t, "an-int", "") == bad && Outcome(t, "a-float", "") == bad && Outcome(t, "a-double", "") == bad, "empty numbers");
    expect(Outcome(t, "a-double", "1.0.0", &what) == bad && (bad == 'b' || what == "Invalid floating-point option --a-double=1.0.0"), "a-double=1.0.0");
    expect(Outcome(t, "dropped-int", "x") == bad && Outcome(t, "dropped-bool", "x") == bad && Outcome(t, "dropped-double", "x") == bad, "dropped, malformed");
    expect(Outcome(t, "a-seed", "-1") == 't' && Outcome(t, "a-seed", "") == 't' && Outcome(t, "a-seed", "1e3") == 't', "a-seed, malformed");
    expect(Outcome(t, "not-true", "perhaps") == bad && Outcome(t, "only-zero", "") == bad, "refusals check the value first");
    expect(Outcome(t, "even", "3") == 'b', "the escape hatch's false is a bad value");
    expect(i == -12 && f == 0.5f && d == 1e-3 && !b, "a malformed value leaves the target alone");
    // refused
    expect(Outcome(t, "refused", "", &what) == 't' && what == "--refused is refused", "refused");
    expect(Outcome(t, "not-true", "true", &what) == 't' && what == "--not-true=true is refused", "not-true=true");
    expect(Outcome(t, "only-zero", "2", &what) == 't' && what == "--only-zero is refused", "only-zero=2");
    // underscores: read as dashes, and named with dashes in an error, only where the tool says so
    expect(Outcome(t, "an_int", "5") == (t.underscores ? 'k' : 'u') && i == (t.underscores ? 5 : -12), "an_int=5");
    if (t.underscores && !t.bad_value_line) expect(Outcome(t, "an_int", "x", &what) == 't' && what == "Invalid integer option --an-int=x", "an_int=x");
    expect(Outcome(t, "any_thing", "2") == (t.underscores ? 'k' : 'u'), "any_thing=2");
    // unknown, and the common three: after the table, and not where --config is a file
    expect(Outcome(t, "no-such", "1") == 'u' && Outcome(t, "a-boo", "1") == 'u' && Outcome(t, "", "") == 'u', "unknown");
    for (const char* c : {"verbose", "print-args", "config"}) expect(Outcome(t, c, "x") == (t.config_file ? 'u' : 'k'), c);
    expect(Outcome(t, "print_args", "x") == (t.config_file || !t.underscores ? 'u' : 'k'), "print_args");
  }
  // a tool's own --verbose comes before the common one
  int verbose = 0;
  xv::CliTool v = {"verbose", "Usage: verbose\n", {xv::Int("verbose", &verbose)}, 0, 0, [](const std::vector<std::string>&) { return 0; }};
  expect(Outcome(v, "verbose", "x") == 't' && Outcome(v, "verbose", "2") == 'k' && verbose == 2, "the tool's own --verbose");

  // CliMain: the file first, the command line second; the count; kUsageError; an exception; --help
  {
    std::ofstream f(config_path);
    f << "# a comment\n\n--an-int=1 # first\n--a-string=from the file\n";
  }
  int i = 0, ran = 0;
  std::string s;
  xv::CliTool c = {"synthetic", "Usage: synthetic <a> [<b>]\n", {xv::Int("an-int", &i), xv::String("a-string", &s)}, 1, 2,
                   [&](const std::vector<std::string>& pos) { return ++ran, pos[0] == "usage" ? xv::kUsageError : pos[0] == "throw" ? throw xv::KioError("thrown") : 7; }};
  c.config_file = true;
  const std::string config = "--config=" + config_path;
  auto cli = [&](std::vector<const char*> args) {
    args.insert(args.begin(), "/somewhere/synthetic");
    return xv::CliMain((int)args.size(), const_cast<char**>(args.data()), c);
  };
  expect(cli({"--an-int=2", config.c_str(), "a"}) == 7 && i == 2 && s == "from the file" && ran == 1, "the command line wins over the file");
  expect(cli({config.c_str()}) == 1 && cli({config.c_str(), "a", "b", "c"}) == 1 && ran == 1, "a wrong count is the usage, and the tool does not run");
  expect(cli({"a", "--an-int=x"}) == 7 && ran == 2, "an option behind a positional is a positional");
  expect(cli({"usage"}) == 1 && cli({"throw"}) == 255 && ran == 4, "kUsageError and an exception");
  expect(cli({"--help", "--no-such"}) == 0 && cli({"--no-such", "a"}) == 255 && cli({"--an-int=x", "a"}) == 255 && ran == 4, "--help, unknown, malformed");
  expect(cli({"--config=/nonexistent/dir/x.conf", "a"}) == 255 && ran == 4, "a config file that is not there");
  unlink(config_path.c_str());

  // ToolsMain: every tool returns its index
  std::vector<xv::CliTool> tools;
  const char* names[] = {"tool-one", "tool-one-more", "other"};
  for (int k = 0; k < 3; ++k) tools.push_back({names[k], "Usage\n", {}, 0, 0, [k](const std::vector<std::string>&) { return 10 + k; }});
  tools[2].match = "oth";
  auto as = [&](const char* argv0, xv::NameRule rule, const char* fallback) {
    char* args[] = {const_cast<char*>(argv0), nullptr};
    return xv::ToolsMain(1, args, tools, rule, fallback);
  };
  expect(as("bin/tool-one-more", xv::NameRule::kContains, "other") == 10, "kContains takes the first of the table that fits");
  expect(as("x-oth.bak", xv::NameRule::kContains, "tool-one") == 12 && as("zz", xv::NameRule::kContains, "tool-one-more") == 11, "match and fallback");
  expect(as("bin/tool-one-more", xv::NameRule::kExact, "other") == 11 && as("x-tool-one", xv::NameRule::kExact, "other") == 12, "kExact");
  expect(as("other", xv::NameRule::kExactOrRefuse, nullptr) == 12 && as("x-other", xv::NameRule::kExactOrRefuse, nullptr) == 255, "kExactOrRefuse");
  printf("host_selftest: cli %s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}

// ---------------------------------------------------- host_selftest batches <rspecifier> <readers> <views 0|1>
// The table loop's batch source (batch_source.h) with limits of 16 rows and 4 utterances: one line per batch - keys with their
// row counts, a hash of the rows - then the read-failure count, the pipe's status and the error; warnings go to stderr.
int RunBatches(const std::string& rspec, int readers, bool views) {
  xv::BatchSourceOptions o;
  o.max_rows = 16;
  o.max_utts = 4;
  o.n_readers = readers;
  o.views = views;
  std::mutex warn_mu;
  try {
    xv::BatchSource src(rspec, o, [&warn_mu](const std::string& m) {
      std::lock_guard<std::mutex> lk(warn_mu);
      fprintf(stderr, "WARNING %s\n", m.c_str());
    });
    printf("addressable\t%d\n", src.addressable() ? 1 : 0);
    src.Start();
    xv::Batch b;
    while (src.Next(&b)) {
      Hash h;
      std::string keys;
      for (const xv::Utt& u : b.utts) {
        keys += (keys.empty() ? "" : ",") + u.key + ":" + std::to_string(u.feats.rows) + "x" + std::to_string(u.feats.cols);
        h.Add(u.feats.Data(), (size_t)u.feats.rows * u.feats.cols * sizeof(float));
      }
      printf("batch\t%s\t%016llx%s\n", keys.c_str(), (unsigned long long)h.h, b.last ? "\tlast" : "");
      src.Recycle(std::move(b));
      b = xv::Batch();
    }
    src.Finish();
    printf("fail_read\t%ld\nstatus\t%d\nerror\t%s\n", src.num_fail_read(), src.reader_status(), src.error().c_str());
  } catch (const std::exception& ex) {
    printf("thrown\t%s\n", ex.what());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 5 && strcmp(argv[1], "batches") == 0) return RunBatches(argv[2], atoi(argv[3]), atoi(argv[4]) != 0);
  if (argc == 2 && strcmp(argv[1], "gemm_plan") == 0) return RunGemmPlan();
  if (argc == 3 && strcmp(argv[1], "cli") == 0) return RunCli(argv[2]);
  if (argc == 3 && strcmp(argv[1], "tables") == 0) return RunTables(argv[2]);
  if (argc == 3 && strcmp(argv[1], "walk") == 0) return RunWalk(argv[2]);
  if (argc != 4 && argc != 5) {
    fprintf(stderr, "usage: host_selftest <model.raw> <output-node> <features.ark> [variants]\n       host_selftest tables <dir>\n");
    return 2;
  }
  const int variants = argc == 5 ? atoi(argv[4]) : 200;
  const std::string model = Slurp(argv[1]), node = argv[2], ark = Slurp(argv[3]);
  if (model.empty() || ark.empty()) {
    fprintf(stderr, "host_selftest: empty input\n");
    return 2;
  }
  // 1. round trips
  xv::RawNnet net;
  net.Read(model);
  // (the writer re-emits components verbatim, so it keeps the flavour of its input)
  const int same = (model.size() >= 2 && model[0] == '\0' && model[1] == 'B') ? 1 : 0;
  for (int binary = same; binary <= same; ++binary) {
    const std::string tmp = std::string(argv[1]) + (binary ? ".selftest.bin" : ".selftest.txt");
    {
      xv::Output out;
      out.Open(tmp);
      net.Write(out, binary != 0);
      out.Close();
    }
    if (TryModel(Slurp(tmp), node) != 0) {
      fprintf(stderr, "host_selftest: re-emitted model (%s) does not parse\n", binary ? "binary" : "text");
      return 1;
    }
    remove(tmp.c_str());
  }
  if (TryModel(model, node) != 0 || TryArchive(ark) != 0) {
    fprintf(stderr, "host_selftest: the pristine inputs do not parse\n");
    return 1;
  }
  {
    xv::SequentialMatrixReader rd(std::string("ark:") + argv[3]);
    const std::string tb = std::string(argv[3]) + ".selftest.bin", tt = std::string(argv[3]) + ".selftest.txt";
    {
      xv::TableWriter wb("ark:" + tb), wt("ark,t:" + tt);
      std::string key, err;
      xv::Matrix m;
      while (rd.Next(&key, &m, &err)) {
        wb.WriteMat(key, m);
        wt.WriteMat(key, m);
      }
    }
    if (TryArchive(Slurp(tb)) != 0 || TryArchive(Slurp(tt)) != 0) {
      fprintf(stderr, "host_selftest: re-written archive does not parse\n");
      return 1;
    }
    // 2b. the index pass: the binary copy through the archive and through a script file of its offsets; the text copy
    // is not addressable and must say so
    {
      const std::string ts = std::string(argv[3]) + ".selftest.scp";
      {
        xv::TableWriter ws("ark,scp:" + tb + "," + ts);
        xv::SequentialMatrixReader rd2(std::string("ark:") + argv[3]);
        std::string key, err;
        xv::Matrix m;
        while (rd2.Next(&key, &m, &err)) ws.WriteMat(key, m);
      }
      long views = 0;
      if (CheckIndexer("ark:" + tb, "ark:" + tb, &views) != 0 || CheckIndexer("scp:" + ts, "ark:" + tb, &views) != 0 ||
          CheckIndexer("ark:" + tt, "ark:" + tt, &views) != 2) {
        fprintf(stderr, "host_selftest: the indexed table readers disagree with the sequential reader\n");
        return 1;
      }
      if (views == 0) {
        fprintf(stderr, "host_selftest: no object of the binary archive could be viewed in the mapped file\n");
        return 1;
      }
      // the input archive itself, when it is binary: it may hold COMPRESSED objects (the stored form of the recipes' features),
      // whose views the device front-end uploads as they are
      {
        xv::MatrixTableIndexer probe(std::string("ark:") + argv[3]);
        if (probe.usable()) {
          long v2 = 0;
          if (CheckIndexer(std::string("ark:") + argv[3], std::string("ark:") + argv[3], &v2) != 0) {
            fprintf(stderr, "host_selftest: the indexed readers / views disagree with the sequential reader on the input archive\n");
            return 1;
          }
          const std::string orig = Slurp(argv[3]), to = std::string(argv[3]) + ".selftest.dmg2";
          unsigned st2 = 4242;
          for (int i = 0; i < variants; ++i) {
            std::string bad = orig;
            st2 = st2 * 1664525u + 1013904223u;
            if (i % 2) bad.resize(orig.size() * (size_t)(i + 1) / (variants + 2));
            else bad[st2 % bad.size()] = (char)(bad[st2 % bad.size()] ^ (1u << ((st2 >> 20) & 7)));
            {
              std::ofstream f(to, std::ios::binary);
              f.write(bad.data(), (std::streamsize)bad.size());
            }
            (void)TryIndexedFile(to);
          }
          remove(to.c_str());
        }
      }
      // damaged copies of the binary archive through the index pass (truncations and bit flips, on disk: the indexer seeks)
      const std::string good = Slurp(tb), td = std::string(argv[3]) + ".selftest.dmg";
      unsigned state = 777;
      for (int i = 0; i < variants; ++i) {
        std::string bad = good;
        state = state * 1664525u + 1013904223u;
        if (i % 2) bad.resize(good.size() * (size_t)(i + 1) / (variants + 2));
        else bad[state % bad.size()] = (char)(bad[state % bad.size()] ^ (1u << ((state >> 20) & 7)));
        {
          std::ofstream f(td, std::ios::binary);
          f.write(bad.data(), (std::streamsize)bad.size());
        }
        (void)TryIndexedFile(td);
      }
      remove(td.c_str());
      remove(ts.c_str());
    }
    remove(tb.c_str());
    remove(tt.c_str());
  }
  // 2. truncations and byte flips
  long parsed = 0, rejected = 0;
  auto replay = [&](const std::string& good, bool is_model) {
    const size_t n = good.size();
    for (int i = 1; i <= variants; ++i) {
      const size_t cut = n * i / (variants + 1);
      const int r = is_model ? TryModel(good.substr(0, cut), node) : TryArchive(good.substr(0, cut));
      (r ? rejected : parsed)++;
    }
    unsigned state = 12345;
    for (int i = 0; i < variants * 3 / 2; ++i) {
      state = state * 1664525u + 1013904223u;
      std::string bad = good;
      // most flips in the first 4 KiB (tokens, dimensions), the rest anywhere
      const size_t pos = (i % 3 ? state % (n < 4096 ? n : 4096) : state % n);
      bad[pos] = (char)(bad[pos] ^ (1u << ((state >> 20) & 7)));
      const int r = is_model ? TryModel(bad, node) : TryArchive(bad);
      (r ? rejected : parsed)++;
    }
  };
  replay(model, true);
  replay(ark, false);
  printf("host_selftest: ok (%ld damaged variants parsed, %ld rejected cleanly)\n", parsed, rejected);
  return 0;
}
