// ivector-compute-lda / ivector-compute-plda / ivector-copy-plda / ivector-adapt-plda / ivector-plda-scoring /
// ivector-plda-scoring-asnorm / compute-eer -
// drop-in command lines for the back-end stage of the recipes (stage 7 of egs/sre/v2/run_sre10.sh:221-252;
// v5/run_sre10.sh:105-137, stage 2 of v2/run_sre16.sh:76-175), one executable dispatching on its name:
//   ivector-compute-lda [--dim=100 --total-covariance-factor=0.0 --covariance-floor=1e-6 --binary=true]
//                       <ivector-rspecifier> <utt2spk-rspecifier> <lda-matrix-out>                      run_sre10.sh:229-231
//   ivector-compute-plda [--num-em-iters=10 --binary=true] <spk2utt-rspecifier> <ivector-rspecifier> <plda-out>   :234-236
//   ivector-copy-plda [--smoothing=0.0 --binary=true] <plda-in> <plda-out>                                       :243
//   ivector-adapt-plda [--mean-diff-scale=1.0 --within-covar-scale=0.3 --between-covar-scale=0.7 --binary=true]
//                      <plda-in> <ivectors-rspecifier> <plda-out>                       stage 2 of v2/run_sre16.sh:97-101
//   ivector-plda-scoring [--normalize-length=true --simple-length-normalization=false --num-utts=<rspecifier>]
//                        <plda> <train-ivector-rspecifier> <test-ivector-rspecifier> <trials-rxfilename> <scores-wxfilename>
//                                                                                                           :240-246
//   ivector-plda-scoring-asnorm [the options of ivector-plda-scoring, --top-n=300 --train-stats=<wx> --test-stats=<wx>]
//                        <plda> <train-ivector-rspecifier> <test-ivector-rspecifier> <cohort-ivector-rspecifier>
//                        <trials-rxfilename> <scores-wxfilename>          (not in the recipes: INTEGRATION.md)
//   compute-eer <scores-rxfilename>    ("score target|nontarget" lines; the EER in percent on stdout)           :252
// The statistics over the vectors (for the adaptation: one segment that lists every vector), the PLDA transform of the
// vectors and the per-trial scores run on the HIP device (plda.h); without a GPU these tools fail (exit 255).  compute-eer
// is host arithmetic only.  Semantics are upstream Kaldi's [UPSTREAM, recalled] (ivectorbin/*.cc, ivector/plda.cc); log
// lines and exit codes follow the Kaldi idiom (0 iff something was written, 1 if nothing was, 255 on an error).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <numeric>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "backend.h"
#include "cli.h"
#include "kio.h"
#include "plda.h"

namespace {

struct Args {
  std::vector<std::string> pos;         // set by main() for the tool that runs
  bool binary = true;
  int lda_dim = 100;                    // ivector-compute-lda --dim
  double total_covariance_factor = 0.0;
  double covariance_floor = 1e-6;
  int num_em_iters = 10;                // ivector-compute-plda
  double smoothing = 0.0;               // ivector-copy-plda
  double mean_diff_scale = 1.0;         // ivector-adapt-plda
  double within_covar_scale = 0.3;
  double between_covar_scale = 0.7;
  bool normalize_length = true;         // ivector-plda-scoring
  bool simple_length_norm = false;
  std::string num_utts;
  int top_n = 300;                      // ivector-plda-scoring-asnorm
  std::string train_stats, test_stats;
  int device = -1;
};

// A whole vector table; a failed input pipe is an error.
void ReadAll(const std::string& rspecifier, xv::Packed* p, long* n_err) {
  xv::SequentialVectorReader r(rspecifier);
  xv::ReadBatch(r, -1, p, n_err);
  const int st = r.Close();
  if (st != 0) throw xv::KioError("the input pipe of " + rspecifier + " exited with status " + std::to_string(st));
}

// Rows of `p` grouped into segments (in the order of `groups`), for the scatter kernel.
struct Segments {
  std::vector<int32_t> off = {0}, idx;
  void Add(const std::vector<int32_t>& rows) {
    idx.insert(idx.end(), rows.begin(), rows.end());
    off.push_back((int32_t)idx.size());
  }
  int n() const { return (int)off.size() - 1; }
};

void WriteFloatMatrixObject(const std::string& wx, bool binary, int rows, int cols, const std::vector<float>& data) {
  xv::Matrix m;
  m.rows = rows;
  m.cols = cols;
  m.data = data;
  xv::Output out;
  out.Open(wx);
  if (binary) out.Write("\0B", 2);
  xv::WriteMatrix(out, binary, m);
  out.Close();
}

int ComputeLda(const Args& a) {
  if (a.pos.size() != 3) return xv::kUsageError;
  const int dev = xv::PickDevice(a.device);
  xv::Packed p;
  long n_err = 0;
  ReadAll(a.pos[0], &p, &n_err);
  const std::unordered_map<std::string, std::string> utt2spk = xv::ReadTokenTable(a.pos[1]);
  // the utterances with a speaker, packed; speakers in order of first appearance
  std::vector<float> x;
  std::map<std::string, int> spk_index;
  std::vector<std::vector<int32_t>> spk_rows;
  int n_done = 0;
  for (int i = 0; i < p.n(); ++i) {
    auto it = utt2spk.find(p.keys[i]);
    if (it == utt2spk.end()) {
      XWARN("No speaker for utterance " << p.keys[i]);
      ++n_err;
      continue;
    }
    auto s = spk_index.emplace(it->second, (int)spk_rows.size());
    if (s.second) spk_rows.emplace_back();
    spk_rows[s.first->second].push_back(n_done++);
    x.insert(x.end(), p.data.begin() + (size_t)i * p.dim, p.data.begin() + (size_t)(i + 1) * p.dim);
  }
  XLOG("Read " << n_done << " utterances, " << n_err << " with errors.");
  if (n_done == 0) throw xv::KioError("Did not read any utterances.");
  const int dim = p.dim;
  if (a.lda_dim < 1 || a.lda_dim > dim)
    throw xv::KioError("--dim=" + std::to_string(a.lda_dim) + " is out of range: the iVectors have dimension " + std::to_string(dim));
  // global mean (fp64 accumulation) and its subtraction, on the device
  std::vector<int32_t> all_off = {0, n_done}, all_idx(n_done);
  for (int i = 0; i < n_done; ++i) all_idx[i] = i;
  std::vector<float> mean(dim), xc(x.size());
  xv::SegmentMean(dev, x.data(), n_done, dim, all_off.data(), all_idx.data(), 1, /*acc64=*/true, mean.data());
  double mn = 0;
  for (float m : mean) mn += (double)m * m;
  XLOG("2-norm of iVector mean is " << sqrt(mn));
  xv::BackendOptions o;
  o.mean = mean.data();
  xv::BackendApply(dev, x.data(), n_done, dim, o, xc.data(), nullptr);
  Segments seg;
  for (const auto& rows : spk_rows) seg.Add(rows);
  std::vector<double> s_tot((size_t)dim * dim), s_bet((size_t)dim * dim);
  XLOG("Computing within-class covariance.");
  xv::ScatterStats(dev, xc.data(), n_done, dim, seg.off.data(), seg.idx.data(), seg.n(), s_tot.data(), nullptr, s_bet.data());
  std::vector<float> lda((size_t)a.lda_dim * (dim + 1));
  const int floored = xv::LdaFromStats(dim, n_done, s_tot.data(), s_bet.data(), mean.data(), a.total_covariance_factor,
                                       a.covariance_floor, a.lda_dim, lda.data());
  if (floored > 0) XWARN("Floored " << floored << " eigenvalues of covariance");
  WriteFloatMatrixObject(a.pos[2], a.binary, a.lda_dim, dim + 1, lda);
  XLOG("Wrote LDA transform to " << a.pos[2]);
  return 0;
}

int ComputePlda(const Args& a) {
  if (a.pos.size() != 3) return xv::kUsageError;
  const int dev = xv::PickDevice(a.device);
  const std::vector<xv::TokenList> spk2utt = xv::ReadTokenVectorTable(a.pos[0]);
  xv::Packed p;
  long n_read_err = 0;
  ReadAll(a.pos[1], &p, &n_read_err);
  std::unordered_map<std::string, int> row;
  for (int i = 0; i < p.n(); ++i) row.emplace(p.keys[i], i);
  Segments seg;
  std::vector<int32_t> counts;
  long num_spk_done = 0, num_spk_err = 0, num_utt_done = 0, num_utt_err = 0;
  for (const xv::TokenList& e : spk2utt) {
    if (e.tokens.empty()) throw xv::KioError("Speaker with no utterances.");
    std::vector<int32_t> rows;
    for (const std::string& utt : e.tokens) {
      auto it = row.find(utt);
      if (it == row.end()) {
        XWARN("No iVector present in input for utterance " << utt);
        ++num_utt_err;
      } else {
        rows.push_back(it->second);
        ++num_utt_done;
      }
    }
    if (rows.empty()) {
      XWARN("Not producing output for speaker " << e.key << " since no utterances had iVectors");
      ++num_spk_err;
    } else {
      seg.Add(rows);
      counts.push_back((int32_t)rows.size());
      ++num_spk_done;
    }
  }
  XLOG("Accumulated stats from " << num_spk_done << " speakers (" << num_spk_err << " with no utterances), consisting of "
                                 << num_utt_done << " utterances (" << num_utt_err << " absent from input).");
  if (num_spk_done == 0) throw xv::KioError("No stats accumulated, unable to estimate PLDA.");
  if (num_spk_done == num_utt_done) throw xv::KioError("No speakers with multiple utterances, unable to estimate PLDA.");
  const int dim = p.dim;
  std::vector<double> s_tot((size_t)dim * dim), s_bet((size_t)dim * dim), sums((size_t)seg.n() * dim);
  xv::ScatterStats(dev, p.data.data(), p.n(), dim, seg.off.data(), seg.idx.data(), seg.n(), s_tot.data(), sums.data(), s_bet.data());
  xv::Plda plda;
  std::vector<std::string> log;
  const int floored = xv::PldaFromStats(dim, seg.n(), sums.data(), counts.data(), s_tot.data(), s_bet.data(), a.num_em_iters,
                                        &plda, &log);
  for (const std::string& l : log) XLOG(l);
  if (floored > 0) XWARN("Floored " << floored << " eigenvalues of between-class variance to zero.");
  xv::WritePlda(a.pos[2], a.binary, plda);
  return 0;
}

std::string VecText(const std::vector<double>& v) {
  std::ostringstream o;
  o << " [ ";
  for (double x : v) o << x << " ";
  o << "]";
  return o.str();
}

int CopyPlda(const Args& a) {
  if (a.pos.size() != 2) return xv::kUsageError;
  xv::Plda plda;
  xv::ReadPlda(a.pos[0], &plda);
  if (a.smoothing != 0.0) {
    if (a.smoothing < 0.0 || a.smoothing > 1.0) throw xv::KioError("--smoothing must be in [0, 1]");
    XLOG("Smoothing within-class covariance by " << a.smoothing << ", Psi is initially: " << VecText(plda.psi));
    plda.SmoothWithinClassCovariance(a.smoothing);
    XLOG("New value of Psi is " << VecText(plda.psi));
  }
  xv::WritePlda(a.pos[1], a.binary, plda);
  return 0;
}

// PldaUnsupervisedAdaptor: the vectors' sum and scatter (fp64, on the device, xv::ScatterStats with one segment that
// lists every row), then the update on the host (xv::AdaptPlda).
int AdaptPlda(const Args& a) {
  if (a.pos.size() != 3) return xv::kUsageError;
  const int dev = xv::PickDevice(a.device);
  xv::Plda plda;
  xv::ReadPlda(a.pos[0], &plda);
  xv::Packed p;
  long n_err = 0;
  ReadAll(a.pos[1], &p, &n_err);
  XLOG("Accumulated stats from " << p.n() << " iVectors.");
  if (p.n() == 0) throw xv::KioError("No iVectors read: there are no statistics to adapt the PLDA model with.");
  if (p.dim != plda.dim)
    throw xv::KioError("iVector dimension " + std::to_string(p.dim) + " does not match the PLDA dimension " + std::to_string(plda.dim));
  const int dim = p.dim;
  std::vector<int32_t> off = {0, p.n()}, idx(p.n());
  std::iota(idx.begin(), idx.end(), 0);
  std::vector<double> sum(dim), scatter((size_t)dim * dim);
  xv::ScatterStats(dev, p.data.data(), p.n(), dim, off.data(), idx.data(), 1, scatter.data(), sum.data(), nullptr);
  std::vector<std::string> log;
  xv::AdaptPlda(p.n(), sum.data(), scatter.data(), a.mean_diff_scale, a.within_covar_scale, a.between_covar_scale, &plda, nullptr,
                &log);
  for (const std::string& l : log) XLOG(l);
  xv::WritePlda(a.pos[2], a.binary, plda);
  return 0;
}

// Splits on blanks (" \t\r\n"), empty fields dropped.
void SplitFields(const std::string& line, std::vector<std::string>* f) {
  f->clear();
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && strchr(" \t\r\n", line[i])) ++i;
    size_t j = i;
    while (j < line.size() && !strchr(" \t\r\n", line[j])) ++j;
    if (j > i) f->push_back(line.substr(i, j - i));
    i = j;
  }
}

// Lines of an rxfilename, read in blocks.
class LineReader {
 public:
  explicit LineReader(const std::string& rx) { in_.Open(rx); }
  bool Next(std::string* line) {
    line->clear();
    for (;;) {
      if (pos_ == len_) {
        len_ = in_.ReadUpTo(buf_, sizeof buf_);
        pos_ = 0;
        if (len_ == 0) return !line->empty();
      }
      const char* nl = (const char*)memchr(buf_ + pos_, '\n', len_ - pos_);
      if (nl) {
        line->append(buf_ + pos_, nl - (buf_ + pos_));
        pos_ = nl - buf_ + 1;
        return true;
      }
      line->append(buf_ + pos_, len_ - pos_);
      pos_ = len_;
    }
  }
  int Close() { return in_.Close(); }

 private:
  xv::Input in_;
  char buf_[1 << 16];
  size_t pos_ = 0, len_ = 0;
};

// One table of ivector-plda-scoring and its kin, transformed by the model: the rows that are kept, in table order.
struct Side {
  xv::Packed p;
  std::vector<double> num;
  std::vector<float> y;
  std::unordered_map<std::string, int> row;
};
enum class SideKind { kTrain, kTest, kCohort };

// Reads a table and transforms it on the device; returns the sum of the renormalisation scales.  A training table takes its
// example counts from num_utts when --num-utts is given (a key without one is skipped and counted in *n_err).  finite_only:
// a value that is not finite is an error.
double LoadSide(const Args& a, int dev, const xv::Plda& plda, const std::unordered_map<std::string, int32_t>& num_utts,
                const std::string& rspec, SideKind kind, bool finite_only, Side* s, long* n_err) {
  const int dim = plda.dim;
  const bool is_train = kind == SideKind::kTrain;
  xv::Packed raw;
  long read_err = 0;
  ReadAll(rspec, &raw, &read_err);
  if (raw.n() > 0 && raw.dim != dim)
    throw xv::KioError("iVector dimension " + std::to_string(raw.dim) + " does not match the PLDA dimension " + std::to_string(dim));
  s->p.dim = dim;
  for (int i = 0; i < raw.n(); ++i) {
    const std::string& key = raw.keys[i];
    if (s->row.count(key))
      throw xv::KioError(std::string("Duplicate ") + (is_train ? "training iVector found for speaker "
                                                       : kind == SideKind::kTest ? "test iVector found for utterance "
                                                                                 : "cohort iVector found for utterance ") + key);
    if (finite_only)
      for (int d = 0; d < dim; ++d)
        if (!std::isfinite(raw.data[(size_t)i * dim + d])) throw xv::KioError("iVector " + key + " of " + rspec + " has a value that is not finite");
    double n = 1.0;
    if (is_train && !a.num_utts.empty()) {
      auto it = num_utts.find(key);
      if (it == num_utts.end()) {
        XWARN("Number of utterances not given for speaker " << key);
        ++*n_err;
        continue;
      }
      n = it->second;
      if (n < 1) throw xv::KioError("number of utterances for speaker " + key + " is not positive");
    }
    s->row.emplace(key, s->p.n());
    s->p.keys.push_back(key);
    s->p.data.insert(s->p.data.end(), raw.data.begin() + (size_t)i * dim, raw.data.begin() + (size_t)(i + 1) * dim);
    s->num.push_back(n);
  }
  std::vector<double> scale(s->p.n());
  s->y.resize(s->p.data.size());
  xv::PldaTransform(dev, s->p.data.data(), s->p.n(), dim, plda.transform.data(), plda.offset.data(), plda.psi.data(),
                    s->num.data(), a.normalize_length, a.simple_length_norm, s->y.data(), scale.data());
  double tot = 0;
  for (double x : scale) tot += x;
  return tot;
}

// The training and the test table, with the log lines of ivector-plda-scoring.
void LoadTrainAndTest(const Args& a, int dev, const xv::Plda& plda, const std::unordered_map<std::string, int32_t>& num_utts,
                      bool finite_only, Side* train, Side* test) {
  long n_train_err = 0, n_test_err = 0;
  XLOG("Reading train iVectors");
  const double train_scale = LoadSide(a, dev, plda, num_utts, a.pos[1], SideKind::kTrain, finite_only, train, &n_train_err);
  XLOG("Read " << train->p.n() << " training iVectors, errors on " << n_train_err);
  if (train->p.n() == 0) throw xv::KioError("No training iVectors present.");
  XLOG("Average renormalization scale on training iVectors was " << train_scale / train->p.n());
  XLOG("Reading test iVectors");
  const double test_scale = LoadSide(a, dev, plda, num_utts, a.pos[2], SideKind::kTest, finite_only, test, &n_test_err);
  XLOG("Read " << test->p.n() << " test iVectors.");
  if (test->p.n() == 0) throw xv::KioError("No test iVectors present.");
  XLOG("Average renormalization scale on test iVectors was " << test_scale / test->p.n());
}

// The trials of an rxfilename, in input order; lines whose keys are missing are skipped and counted.
struct Trials {
  std::vector<int32_t> pairs;       // (training row, test row) of every scored trial
  std::vector<std::string> names;   // "key1 key2 " of every scored trial
  long n_err = 0;
  long n() const { return (long)names.size(); }
};

void ReadTrials(const std::string& rx, const Side& train, const Side& test, Trials* t) {
  LineReader lr(rx);
  std::string line;
  std::vector<std::string> f;
  while (lr.Next(&line)) {
    SplitFields(line, &f);
    if (f.size() != 2)
      throw xv::KioError("Bad line " + std::to_string(t->names.size() + t->n_err) + " in input (expected two fields: key1 key2): " + line);
    auto i1 = train.row.find(f[0]);
    if (i1 == train.row.end()) {
      XWARN("Key " << f[0] << " not present in training iVectors.");
      ++t->n_err;
      continue;
    }
    auto i2 = test.row.find(f[1]);
    if (i2 == test.row.end()) {
      XWARN("Key " << f[1] << " not present in test iVectors.");
      ++t->n_err;
      continue;
    }
    t->pairs.push_back(i1->second);
    t->pairs.push_back(i2->second);
    t->names.push_back(f[0] + " " + f[1] + " ");
  }
  const int st = lr.Close();
  if (st != 0) throw xv::KioError("the trials command of " + rx + " exited with status " + std::to_string(st));
}

using Clock = std::chrono::steady_clock;
double Secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// "<names[i]><score as BaseFloat>" lines (the stream's default 6 significant digits) and the log line of their statistics.
void WriteScores(const std::string& wx, const std::vector<std::string>& names, const std::vector<double>& scores) {
  const long n_done = (long)names.size();
  xv::Output out;
  out.Open(wx);
  double sum = 0, sumsq = 0;
  std::ostringstream o;
  for (long i = 0; i < n_done; ++i) {
    const float s = (float)scores[i];   // BaseFloat, printed with the stream's default 6 significant digits
    sum += s;
    sumsq += (double)s * s;
    o << names[i] << s << '\n';
    if (o.tellp() > (1 << 20) || i + 1 == n_done) {
      out.Puts(o.str());
      o.str("");
    }
  }
  out.Close();
  if (n_done != 0) {
    const float mean = (float)(sum / n_done), scatter = (float)(sumsq / n_done), var = scatter - mean * mean;
    XLOG("Mean score was " << mean << ", standard deviation was " << sqrtf(var > 0 ? var : 0));
  }
}

int PldaScoring(const Args& a) {
  if (a.pos.size() != 5) return xv::kUsageError;
  const int dev = xv::PickDevice(a.device);
  xv::Plda plda;
  xv::ReadPlda(a.pos[0], &plda);
  const int dim = plda.dim;
  std::unordered_map<std::string, int32_t> num_utts;
  if (!a.num_utts.empty()) num_utts = xv::ReadInt32Table(a.num_utts);
  Side train, test;
  LoadTrainAndTest(a, dev, plda, num_utts, /*finite_only=*/false, &train, &test);

  const Clock::time_point t0 = Clock::now();
  Trials tr;
  ReadTrials(a.pos[3], train, test, &tr);
  const long n_done = tr.n();
  const Clock::time_point t1 = Clock::now();
  std::vector<double> scores(n_done);
  xv::PldaScore(dev, train.y.data(), train.num.data(), train.p.n(), test.y.data(), test.p.n(), dim, plda.psi.data(),
                tr.pairs.data(), n_done, scores.data());
  const Clock::time_point t2 = Clock::now();
  WriteScores(a.pos[4], tr.names, scores);
  const Clock::time_point t3 = Clock::now();
  XLOG("Processed " << n_done << " trials, " << tr.n_err << " had errors.");
  XLOG("Timing: trials read in " << Secs(t0, t1) << " s, scored on the device in " << Secs(t1, t2) << " s, written in "
                                 << Secs(t2, t3) << " s");
  return n_done != 0 ? 0 : 1;
}

// "key mean std" lines, one per listed row, in table order.
void WriteStats(const std::string& wx, const Side& s, const std::vector<int32_t>& rows, const std::vector<double>& mean,
                const std::vector<double>& std) {
  xv::Output out;
  out.Open(wx);
  std::ostringstream o;
  o.precision(17);
  for (size_t i = 0; i < rows.size(); ++i) o << s.p.keys[rows[i]] << ' ' << mean[i] << ' ' << std[i] << '\n';
  out.Puts(o.str());
  out.Close();
}

// Adaptive symmetric score normalisation: every trial's raw score s is ivector-plda-scoring's; the
// enrolment row e and the test row t of the trial are each scored against the whole cohort on the device, S_e[c] = LLR(e with
// num_e examples, c) and S_t[c] = LLR(c with one example, t), and the mean and standard deviation of the --top-n largest of
// each give 1/2 ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t).
int PldaScoringAsnorm(const Args& a) {
  if (a.pos.size() != 6) return xv::kUsageError;
  if (a.top_n < 2) throw xv::KioError("--top-n=" + std::to_string(a.top_n) + " is out of range: the statistics need at least two scores");
  const int dev = xv::PickDevice(a.device);
  xv::Plda plda;
  xv::ReadPlda(a.pos[0], &plda);
  const int dim = plda.dim;
  std::unordered_map<std::string, int32_t> num_utts;
  if (!a.num_utts.empty()) num_utts = xv::ReadInt32Table(a.num_utts);
  Side train, test, cohort;
  LoadTrainAndTest(a, dev, plda, num_utts, /*finite_only=*/true, &train, &test);
  XLOG("Reading cohort iVectors");
  long n_cohort_err = 0;
  const double cohort_scale = LoadSide(a, dev, plda, num_utts, a.pos[3], SideKind::kCohort, true, &cohort, &n_cohort_err);
  XLOG("Read " << cohort.p.n() << " cohort iVectors.");
  const int n_cohort = cohort.p.n();
  if (n_cohort < 2) throw xv::KioError("The cohort has " + std::to_string(n_cohort) + " iVectors: score normalisation needs at least two.");
  XLOG("Average renormalization scale on cohort iVectors was " << cohort_scale / n_cohort);
  int top_n = a.top_n;
  if (top_n > n_cohort) {
    XLOG("--top-n=" << top_n << " is more than the cohort holds: using all " << n_cohort << " cohort scores (S-norm).");
    top_n = n_cohort;
  }

  const Clock::time_point t0 = Clock::now();
  Trials tr;
  ReadTrials(a.pos[4], train, test, &tr);
  const long n_read = tr.n();
  const Clock::time_point t1 = Clock::now();
  std::vector<double> raw(n_read);
  xv::PldaScore(dev, train.y.data(), train.num.data(), train.p.n(), test.y.data(), test.p.n(), dim, plda.psi.data(),
                tr.pairs.data(), n_read, raw.data());
  // the rows that occur in a scored trial, in table order, and their place among those
  auto used = [&](const Side& s, int which, std::vector<int32_t>* rows, std::vector<int32_t>* place) {
    place->assign(s.p.n(), -1);
    for (long i = 0; i < n_read; ++i) (*place)[tr.pairs[2 * i + which]] = 0;
    for (int r = 0; r < s.p.n(); ++r)
      if ((*place)[r] == 0) {
        (*place)[r] = (int32_t)rows->size();
        rows->push_back(r);
      }
  };
  auto gather = [&](const Side& s, const std::vector<int32_t>& rows, std::vector<float>* y, std::vector<double>* num) {
    for (int32_t r : rows) {
      y->insert(y->end(), s.y.begin() + (size_t)r * dim, s.y.begin() + (size_t)(r + 1) * dim);
      num->push_back(s.num[r]);
    }
  };
  std::vector<int32_t> e_rows, e_place, t_rows, t_place;
  used(train, 0, &e_rows, &e_place);
  used(test, 1, &t_rows, &t_place);
  std::vector<float> e_y, t_y;
  std::vector<double> e_num, t_num;
  gather(train, e_rows, &e_y, &e_num);
  gather(test, t_rows, &t_y, &t_num);
  std::vector<double> e_mean(e_rows.size()), e_std(e_rows.size()), t_mean(t_rows.size()), t_std(t_rows.size());
  xv::PldaCohortStats(dev, e_y.data(), e_num.data(), (int)e_rows.size(), cohort.y.data(), n_cohort, dim, plda.psi.data(),
                      /*by_column=*/false, top_n, e_mean.data(), e_std.data());
  xv::PldaCohortStats(dev, cohort.y.data(), cohort.num.data(), n_cohort, t_y.data(), (int)t_rows.size(), dim, plda.psi.data(),
                      /*by_column=*/true, top_n, t_mean.data(), t_std.data());
  std::vector<std::string> names;
  std::vector<double> scores;
  long n_err = tr.n_err;
  for (long i = 0; i < n_read; ++i) {
    const int e = e_place[tr.pairs[2 * i]], t = t_place[tr.pairs[2 * i + 1]];
    if (e_std[e] == 0.0 || t_std[t] == 0.0) {
      XWARN("The cohort scores of " << (e_std[e] == 0.0 ? train.p.keys[tr.pairs[2 * i]] : test.p.keys[tr.pairs[2 * i + 1]])
                                   << " have standard deviation 0: not normalising trial " << tr.names[i]);
      ++n_err;
      continue;
    }
    names.push_back(tr.names[i]);
    scores.push_back(0.5 * ((raw[i] - e_mean[e]) / e_std[e] + (raw[i] - t_mean[t]) / t_std[t]));
  }
  const long n_done = (long)names.size();
  const Clock::time_point t2 = Clock::now();
  WriteScores(a.pos[5], names, scores);
  if (!a.train_stats.empty()) WriteStats(a.train_stats, train, e_rows, e_mean, e_std);
  if (!a.test_stats.empty()) WriteStats(a.test_stats, test, t_rows, t_mean, t_std);
  const Clock::time_point t3 = Clock::now();
  XLOG("Processed " << n_done << " trials, " << n_err << " had errors.");
  XLOG("Timing: trials read in " << Secs(t0, t1) << " s, scored and normalised on the device in " << Secs(t1, t2) << " s, written in "
                                 << Secs(t2, t3) << " s");
  return n_done != 0 ? 0 : 1;
}

int ComputeEer(const Args& a) {
  if (a.pos.size() != 1) return xv::kUsageError;
  LineReader lr(a.pos[0]);
  std::string line;
  std::vector<std::string> f;
  std::vector<float> tgt, non;
  while (lr.Next(&line)) {
    SplitFields(line, &f);
    if (f.size() != 2) throw xv::KioError("Invalid input line (must have two fields: score target|nontarget): " + line);
    char* end = nullptr;
    const float s = strtof(f[0].c_str(), &end);
    if (end == f[0].c_str() || *end || !isfinite(s)) throw xv::KioError("Invalid input line (first field must be float): " + line);
    if (f[1] == "target") tgt.push_back(s);
    else if (f[1] == "nontarget") non.push_back(s);
    else throw xv::KioError("Invalid input line (second field must be 'target' or 'nontarget'): " + line);
  }
  lr.Close();
  if (tgt.empty() && non.empty()) throw xv::KioError("Empty input.");
  if (tgt.empty()) throw xv::KioError("No target scores seen.");
  if (non.empty()) throw xv::KioError("No non-target scores seen.");
  std::sort(tgt.begin(), tgt.end());
  std::sort(non.begin(), non.end());
  size_t p = 0;
  const size_t nt = tgt.size();
  for (; p + 1 < nt; ++p) {
    const long nn = (long)non.size();
    long q = nn - 1 - (long)(nn * (double)p / (double)nt);
    if (q < 0) q = 0;
    if (non[q] < tgt[p]) break;
  }
  const float eer = (float)((double)p / (double)nt);
  XLOG("Equal error rate is " << 100.0 * eer << "%, at threshold " << tgt[p]);
  std::ostringstream o;
  o.precision(4);
  o << 100.0 * eer << '\n';
  fputs(o.str().c_str(), stdout);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  // Every tool knows --binary, --device and its own options only: a sibling's option is an unknown one.
  auto tool = [&](const char* name, const char* usage, std::vector<xv::CliOption> own, int (*run)(const Args&)) {
    xv::CliTool t = {name, usage, {xv::Bool("binary", &a.binary)}, 0, -1, [&a, run](const std::vector<std::string>& pos) { return a.pos = pos, run(a); }};
    t.options.insert(t.options.end(), own.begin(), own.end());
    t.options.push_back(xv::LaxInt("device", &a.device));
    t.underscores = false;
    t.bad_value_line = true;
    return t;
  };
  const std::vector<xv::CliTool> tools = {
      tool("ivector-compute-lda",
           "Compute an LDA matrix for iVector system.  Reads in iVectors per utterance, and an utt2spk file which it uses to\n"
           "help work out the within-speaker and between-speaker covariance matrices.  Outputs an LDA projection to a\n"
           "specified dimension.  By default it will normalize so that the projected within-class covariance is unit.\n"
           "Usage: ivector-compute-lda [options] <ivector-rspecifier> <utt2spk-rspecifier> <lda-matrix-out>\n"
           "Options: --dim=100 --total-covariance-factor=0.0 --covariance-floor=1e-06 --binary=true\n",
           {xv::Int("dim", &a.lda_dim), xv::Double("total-covariance-factor", &a.total_covariance_factor), xv::Double("covariance-floor", &a.covariance_floor)},
           ComputeLda),
      tool("ivector-compute-plda",
           "Computes a Plda object (for Probabilistic Linear Discriminant Analysis) from a set of iVectors.\n"
           "Usage: ivector-compute-plda [options] <spk2utt-rspecifier> <ivector-rspecifier> <plda-out>\n"
           "Options: --num-em-iters=10 --binary=true\n",
           {xv::Custom("num-em-iters", [&](const std::string&, const std::string& v) { return xv::ParseInt(v, &a.num_em_iters) && a.num_em_iters >= 0; })},
           ComputePlda),
      tool("ivector-copy-plda",
           "Copy a PLDA object, possibly applying smoothing to the within-class covariance\n"
           "Usage: ivector-copy-plda [--smoothing=0.0] [--binary=true] <plda-in> <plda-out>\n",
           {xv::Double("smoothing", &a.smoothing)}, CopyPlda),
      tool("ivector-adapt-plda",
           "Adapt a PLDA object using unsupervised adaptation-data iVectors from a different domain to the training data.\n"
           "Usage: ivector-adapt-plda [options] <plda-in> <ivectors-rspecifier> <plda-out>\n"
           "e.g.: ivector-adapt-plda plda ark:ivectors.ark plda.adapted\n"
           "Options: --mean-diff-scale=1.0 --within-covar-scale=0.3 --between-covar-scale=0.7 --binary=true\n",
           {xv::Double("mean-diff-scale", &a.mean_diff_scale), xv::Double("within-covar-scale", &a.within_covar_scale),
            xv::Double("between-covar-scale", &a.between_covar_scale)},
           AdaptPlda),
      tool("compute-eer",
           "Computes Equal Error Rate.  Input is a series of lines, each with two fields: the score and 'target' or\n"
           "'nontarget'.  The EER is printed in percent on the standard output.\n"
           "Usage: compute-eer <scores-in>\n"
           "e.g.: compute-eer -\n",
           {}, ComputeEer),
      tool("ivector-plda-scoring",
           "Computes log-likelihood ratios for trials using PLDA model.  The trials file has lines 'key1 key2' (speaker,\n"
           "utterance); the output has lines 'key1 key2 score'.\n"
           "Usage: ivector-plda-scoring <plda> <train-ivector-rspecifier> <test-ivector-rspecifier>\n"
           "                            <trials-rxfilename> <scores-wxfilename>\n"
           "Options: --num-utts=<rspecifier> --normalize-length=true --simple-length-normalization=false\n",
           {xv::Bool("normalize-length", &a.normalize_length), xv::Bool("simple-length-normalization", &a.simple_length_norm),
            xv::String("num-utts", &a.num_utts)},
           PldaScoring),
      tool("ivector-plda-scoring-asnorm",
           "Computes log-likelihood ratios for trials using PLDA model, as ivector-plda-scoring does, and normalises each with the\n"
           "statistics of its two sides against a cohort (adaptive symmetric normalisation, AS-norm): the mean and standard\n"
           "deviation of the --top-n highest scores of the speaker against the cohort, and of the cohort against the utterance.\n"
           "The output has lines 'key1 key2 normalised-score'.\n"
           "Usage: ivector-plda-scoring-asnorm [options] <plda> <train-ivector-rspecifier> <test-ivector-rspecifier>\n"
           "                                   <cohort-ivector-rspecifier> <trials-rxfilename> <scores-wxfilename>\n"
           "Options: --num-utts=<rspecifier> --normalize-length=true --simple-length-normalization=false --top-n=300\n"
           "         --train-stats=<wxfilename> --test-stats=<wxfilename>  ('key mean std' of every speaker / utterance in a trial)\n",
           {xv::Bool("normalize-length", &a.normalize_length), xv::Bool("simple-length-normalization", &a.simple_length_norm),
            xv::String("num-utts", &a.num_utts), xv::Int("top-n", &a.top_n), xv::String("train-stats", &a.train_stats),
            xv::String("test-stats", &a.test_stats)},
           PldaScoringAsnorm),
  };
  return xv::ToolsMain(argc, argv, tools, xv::NameRule::kExact, "ivector-plda-scoring");
}
