// kio - Kaldi table / object I/O without Kaldi.
//
// Replaces, for the one hot path, what the reference gets from Kaldi's util/ and matrix/ libraries
// (not vendored under /root/reference): rxfilename / wxfilename handling, rspecifier / wspecifier
// parsing, `SequentialBaseFloatMatrixReader` (features, extract_xvectors_new.sh:79) and
// `BaseFloatVectorWriter` (ark,scp output, extract_xvectors_new.sh:93).  The text matrix form is the
// one the reference's own Python reads/writes (egs/sre/v2/steps/libs/common.py:354-470).
// Formats: SURVEY.md App. B.1 / B.2.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <memory>
#include <stdexcept>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace xv {

struct KioError : public std::runtime_error {
  explicit KioError(const std::string& m) : std::runtime_error(m) {}
};

// ---------------------------------------------------------------------------------------------
// Byte source: regular file (optionally at an offset), stdin, or the stdout of `cmd |`.
class PipeDrain;   // kio.cc: a thread that keeps reading an input pipe into a ring of blocks

class Input {
 public:
  Input();
  ~Input();
  Input(const Input&) = delete;
  Input& operator=(const Input&) = delete;
  // rxfilename forms: "file", "file:123", "-", "cmd args |"
  // drain_pipe: for "cmd |" inputs, a second thread does the read(2) calls and the parser consumes from a ring of 1 MiB
  // blocks (feature archives through a pipe, extract_xvectors_new.sh:79: the syscalls and the kernel's copy out of the pipe
  // buffer then overlap the parsing and the copy into the batch; XVEC_DEBUG=pipe_drain=0 turns it off)
  void Open(const std::string& rxfilename, bool drain_pipe = false);
  void OpenMemory(const void* data, size_t n);
  void Seek(long offset);           // regular files / memory only
  bool IsRegularFile() const;       // an fopen'ed regular file (seekable): not a pipe, FIFO, device or standard input
  long FileTell();                  // regular files: current offset
  void Skip(long n);                // regular files: move n bytes ahead without reading them
  bool IsOpen() const { return f_ != nullptr || mem_ != nullptr; }
  // Close; for pipes returns the child's exit status (0 otherwise).
  int Close();
  int Peek();                       // next byte or EOF (-1), not consumed
  int Get();                        // next byte or EOF
  void Read(void* dst, size_t n);   // throws on short read
  size_t ReadUpTo(void* dst, size_t n);   // up to n bytes, fewer only at the end of the input
  bool Eof() { return Peek() < 0; }
  // memory sources only: look-ahead and position (used by the model parser)
  int PeekAt(size_t k) const { return (mem_ && mem_pos_ + k < mem_n_) ? mem_[mem_pos_ + k] : -1; }
  size_t Tell() const { return mem_pos_; }
  const std::string& Name() const { return name_; }

 private:
  FILE* f_ = nullptr;
  bool is_pipe_ = false, is_stdin_ = false;
  const unsigned char* mem_ = nullptr;
  size_t mem_n_ = 0, mem_pos_ = 0;
  bool mapped_ = false;   // mem_ is this object's read-only mapping of a regular file (Open): unmapped by Close
  std::string name_;
  std::unique_ptr<PipeDrain> drain_;
};

// Byte sink: file, stdout ("-"), or the stdin of `| cmd`.
class Output {
 public:
  Output() = default;
  ~Output();
  Output(const Output&) = delete;
  Output& operator=(const Output&) = delete;
  void Open(const std::string& wxfilename);
  bool IsOpen() const { return f_ != nullptr; }
  int Close();
  void Write(const void* src, size_t n);
  void Put(char c) { Write(&c, 1); }
  void Puts(const std::string& s) { Write(s.data(), s.size()); }
  void Flush();
  int64_t Tell() const { return pos_; }  // bytes written so far (offset for scp lines)
  const std::string& Name() const { return name_; }

 private:
  FILE* f_ = nullptr;
  bool is_pipe_ = false, is_stdout_ = false;
  int64_t pos_ = 0;
  std::string name_;
};

// ---------------------------------------------------------------------------------------------
// Object-level helpers (binary = the "\0B" flavour).
bool ReadBinaryHeader(Input& in);  // consumes "\0B" if present, returns whether it was
void ReadToken(Input& in, bool binary, std::string* tok);
void ExpectToken(Input& in, bool binary, const char* tok);
int32_t ReadInt32(Input& in, bool binary);
// float or double (binary: size byte 4 or 8), returned as double
double ReadFloatOrDouble(Input& in, bool binary);
bool ReadBool(Input& in, bool binary);
// Skips one self-describing scalar (int32/float/double/bool) - used for unknown optional fields.
void SkipScalar(Input& in, bool binary);

struct Matrix {
  int rows = 0, cols = 0;
  std::vector<float> data;  // row-major, no padding
  // A VIEW instead of a copy (ViewIndexedMatrix): rows x cols floats that live in a mapped archive file.  The address has the
  // alignment the archive gave it (a key of any length precedes the object): memcpy from it, never dereference it as float.
  const float* ext = nullptr;
  // ... or of a COMPRESSED matrix ("CM": one byte per element, Kaldi's default for stored features): cm points behind the "CM "
  // token of the object - {float min_value, range; int32 rows, cols; uint16 percentiles[cols][4]; uint8 data[cols][rows]},
  // cm_bytes of them, any alignment.  rows / cols are set, data is empty, ext is null: such a matrix can only be handed to the
  // device front-end (which expands it on the GPU, kernels.h CmExpandArgs) or expanded with ExpandCompressedView.
  const uint8_t* cm = nullptr;
  size_t cm_bytes = 0;
  const float* Data() const { return ext ? ext : data.data(); }
  float* Row(int r) { return data.data() + (size_t)r * cols; }
  const float* Row(int r) const { return Data() + (size_t)r * cols; }
};

// Reads FM / DM / CM / CM2 / CM3 (binary) or " [ ... ]" (text).
void ReadMatrix(Input& in, bool binary, Matrix* m);
// Regular files are read through read-only mappings (Input, FileMapper).  A file that is truncated by someone else WHILE a tool
// reads it turns a read into SIGBUS where read(2) would have returned short; the command-line tools call this once so that
// the process then ends like every other input error - "ERROR ... changed while it was being read", exit status 255 - instead
// of a bare signal.  (Not installed by the library itself: a host process owns its signal handlers.)
void InstallMappedFileFaultHandler(const char* program);
// Expands a compressed view (Matrix::cm) into floats on the host: *out owns them (the same floats ReadMatrix delivers).
void ExpandCompressedView(const Matrix& view, Matrix* out);
// Regular files, positioned behind the "\0B" of a binary matrix (FM / DM / CM / CM2 / CM3): reads the header only, reports the
// dimensions and moves to the end of the object (the index pass of the parallel table readers).
void SkipBinaryMatrix(Input& in, int* rows, int* cols);
// Reads FV / DV (binary) or " [ ... ]" (text).
void ReadVector(Input& in, bool binary, std::vector<float>* v);
// Double-precision objects (the PLDA model): readers accept FV/DV, FM/DM and text; writers write DV/DM, or text with
// 17 significant digits.
void ReadVectorDouble(Input& in, bool binary, std::vector<double>* v);
void ReadMatrixDouble(Input& in, bool binary, int* rows, int* cols, std::vector<double>* m);
void WriteVectorDouble(Output& out, bool binary, const double* v, int n);
void WriteMatrixDouble(Output& out, bool binary, const double* m, int rows, int cols);
void WriteToken(Output& out, bool binary, const char* tok);
void WriteInt32(Output& out, bool binary, int32_t v);
void WriteFloat(Output& out, bool binary, float v);
void WriteDouble(Output& out, bool binary, double v);
void WriteBool(Output& out, bool binary, bool v);
void WriteVector(Output& out, bool binary, const float* v, int n);
void WriteMatrix(Output& out, bool binary, const Matrix& m);

// ---------------------------------------------------------------------------------------------
// Table specifiers.
struct RspecifierOptions {
  bool is_scp = false;
  bool sorted = false, called_sorted = false, permissive = false, once = false, background = false;
  std::string rxfilename;
};
RspecifierOptions ParseRspecifier(const std::string& rspecifier);

struct WspecifierOptions {
  bool has_ark = false, has_scp = false;
  bool binary = true, flush = true, permissive = false;
  std::string ark_wxfilename, scp_wxfilename;
};
WspecifierOptions ParseWspecifier(const std::string& wspecifier);
// "ark:..." / "scp,p:..." is a table; anything else a file (Kaldi's ClassifyWspecifier / ClassifyRspecifier, as far as needed)
bool IsTable(const std::string& specifier);

// ---------------------------------------------------------------------------------------------
// The pieces every table reader is made of.
// The key of the next entry (white space before it is skipped, the one separator behind it consumed; a '\n' is left for the
// line logic of script files); false at the end of the input.
bool ReadKey(Input& in, std::string* key);
// "path:123" -> (path, 123); anything else - a pipe ("cmd |", whatever it contains), a whole file, a suffix that is not all
// digits - -> -1 with *path = rx.  The one place that knows the form; an offset of 0 is a position like any other to the
// callers, and not a seek to Input::Open.
long SplitOffset(const std::string& rx, std::string* path);
// One line of a script file: the key, then the rest of the line, trimmed (empty when there is none); false at the end.
bool ReadScpLine(Input& in, std::string* key, std::string* rx);

// Where an scp entry becomes an open, positioned Input.  A cursor owns the data file it used last: an entry of the same
// file is a seek (consecutive entries of a table usually share their archive; the file stays mapped in between), an entry of
// another file opens - maps - that one and drops the old, and what cannot be addressed (a pipe, a whole file) is opened
// for the one object and closed by Done().  One cursor per reading thread.
class ArchiveCursor {
 public:
  // an scp entry as it is written ("path:offset", "path", "cmd |"): the sequential readers.  A file is opened under the
  // entry's own text, which is what its errors then name.
  Input& AtEntry(const std::string& rx);
  // (path, offset >= 0), as SplitOffset and the indexer deliver them, or (rxfilename, -1): the file is opened under its
  // path and errors name the archive - the indexed and the random-access readers.
  Input& At(const std::string& path, long offset);
  void Done();    // the object was read: closes what is not addressable, keeps an archive
  void Reset();   // forgets the open file

 private:
  bool Holds(const std::string& path) const { return in_.IsOpen() && path_ == path; }
  Input in_;
  std::string path_;   // of the addressable file in_ holds; empty: none, or a one-shot input
};

// Sequential reader of a table ("ark:..." or "scp:...") of values of one type: Next() advances to the next entry and returns
// false at the end.  A corrupt archive is fatal (KioError), as in Kaldi; a problem with one entry of a script file (an
// unreadable file) comes back through `error` (non-empty) with the key set, and reading continues.  Close(): the exit status
// of an input pipe (valid after the table is exhausted), 0 if not a pipe.  sorted(): the rspecifier promised sorted keys (s):
// the caller may then merge by key instead of loading the table.  The value types: Matrix, std::vector<float>, IntVecVec and
// Posterior (below), each parsed by its Read function.
template <class T>
class SequentialTableReader {
 public:
  // drain_pipe: an archive through a pipe is read by a second thread (Input::Open).  permissive_skips: under the rspecifier's
  // p option an unreadable scp entry is skipped silently instead of reported.
  explicit SequentialTableReader(const std::string& rspecifier, bool drain_pipe = false, bool permissive_skips = false);
  bool Next(std::string* key, T* value, std::string* error);
  bool sorted() const { return opts_.sorted; }
  int Close() { return in_.Close(); }

 private:
  RspecifierOptions opts_;
  bool permissive_skips_;
  Input in_;             // the archive, or the script file
  ArchiveCursor data_;   // scp mode: the data file of the current entry
};
// float matrices (features); the only table that comes through the feature pipe of extract_xvectors_new.sh:79
struct SequentialMatrixReader : SequentialTableReader<Matrix> {
  explicit SequentialMatrixReader(const std::string& rspecifier) : SequentialTableReader(rspecifier, /*drain_pipe=*/true) {}
};
typedef SequentialTableReader<std::vector<float>> SequentialVectorReader;

// Index pass over a matrix table whose objects can be addressed individually: binary archives in a regular file ("ark:file")
// and script files whose entries are "path:offset" (or plain files).  Next() yields one entry without reading its data - key,
// where the object starts, and (binary objects) its dimensions - so that several threads can read a table's matrices in
// parallel and batches can be formed before the data is touched (table_extract.cc).  usable() is false for what can only
// be read front to back (pipes, standard input, text archives): use SequentialMatrixReader there.
class MatrixTableIndexer {
 public:
  struct Entry {
    std::string key;
    std::string rx;      // what to open: "path" (+ offset below) or a whole rxfilename (pipe, plain file) when offset < 0
    long offset = -1;    // byte offset of the object (its "\0B") inside rx, or -1
    int rows = -1, cols = -1;   // -1: not known without reading (text object, pipe)
    std::string error;   // the entry could not be located (scp mode): skip it with a warning
  };
  explicit MatrixTableIndexer(const std::string& rspecifier);
  bool usable() const { return usable_; }
  bool Next(Entry* e);

 private:
  RspecifierOptions opts_;
  Input in_;            // the archive, or the script file
  ArchiveCursor data_;  // scp mode: the data file of the previous entry
  bool usable_ = false;
};
// Reads the matrix an index entry points to through the calling thread's cursor.
void ReadIndexedMatrix(const MatrixTableIndexer::Entry& e, ArchiveCursor* cursor, Matrix* m);
// The same without touching the data: for a binary FLOAT matrix ("FM") at a known offset of a regular file, *m becomes a view of
// the file's pages (the file is mapped read-only once per FileMapper and path, and stays mapped while the FileMapper lives - a
// job owns one, so every view dies before the mapping does and a file rewritten between two jobs of one process is mapped
// anew).  The one host copy of such an utterance is then the one into the device's pinned staging buffer (table_extract.cc) -
// read(2) into a buffer of its own first was half of the host time of a table job.  false: anything else
// (compressed or double matrices, text, pipes, a header that does not check out): the caller reads it with ReadIndexedMatrix,
// which also words the error.  Thread-safe.
class FileMapper {
 public:
  FileMapper() = default;
  ~FileMapper();
  FileMapper(const FileMapper&) = delete;
  FileMapper& operator=(const FileMapper&) = delete;
  // allow_compressed: a "CM" object becomes a compressed view (Matrix::cm) instead of `false`
  bool View(const MatrixTableIndexer::Entry& e, Matrix* m, bool allow_compressed = false);

 private:
  struct Mapped {
    const uint8_t* base = nullptr;
    size_t size = 0;
  };
  Mapped Map(const std::string& path);
  std::mutex mu_;
  std::map<std::string, Mapped> maps_;   // by path; a file that could not be mapped is remembered with base == nullptr
};

// Random-access reader of a table.  An archive is loaded as a whole; the values of a script file are read when they are
// first asked for and kept, the archive of the previous lookup staying open - mapped - in between.  The first entry of a
// key wins.  Float vectors: vad.scp, "scp,s,cs:..."; double-precision matrices: cmvn.scp, one per speaker (FM / DM / text).
struct DoubleMatrix {
  int rows = 0, cols = 0;
  std::vector<double> data;
};
template <class T>
class RandomAccessTableReader {
 public:
  explicit RandomAccessTableReader(const std::string& rspecifier);
  bool HasKey(const std::string& key) const { return index_.count(key) != 0; }
  const T& Value(const std::string& key);   // KioError: the key is not in the table
  // scp tables: gives the memory of a loaded value back (it is read again if the key is asked for once more).  A table job
  // forgets the VAD decisions of a batch once the batch is on the device: kept, a hundred thousand four-minute recordings are
  // 10 GB of them by the end of the job.  (What Kaldi's "scp,s,cs:" options promise its reader it may do.)  A value that was
  // loaded with its whole archive cannot be read again and stays.
  void Forget(const std::string& key);

 private:
  struct Entry { std::string rx; T v; bool loaded = false; };
  std::vector<Entry> entries_;
  std::unordered_map<std::string, int> index_;
  ArchiveCursor data_;
};
typedef RandomAccessTableReader<std::vector<float>> RandomAccessVectorReader;
typedef RandomAccessTableReader<DoubleMatrix> RandomAccessDoubleMatrixReader;

// A text table of token lists, "key tok1 tok2 ...\n" per entry (spk2utt, "ark:$data/spk2utt").
struct TokenList {
  std::string key;
  std::vector<std::string> tokens;
};
std::vector<TokenList> ReadTokenVectorTable(const std::string& rspecifier);
// "key token" per line (utt2spk, "ark:$data/sre_combined/utt2spk"); any other number of tokens is an error.
std::unordered_map<std::string, std::string> ReadTokenTable(const std::string& rspecifier);
// Random-access int32 table, text ("key 12") or binary entries (num_utts.ark, what ivector-mean writes with Int32Writer).
std::unordered_map<std::string, int32_t> ReadInt32Table(const std::string& rspecifier);

// Whole-file Kaldi objects (with the optional binary header): mean.vec, transform.mat.
void ReadVectorObject(const std::string& rxfilename, std::vector<float>* v);
void ReadMatrixObject(const std::string& rxfilename, Matrix* m);
void WriteVectorObject(const std::string& wxfilename, bool binary, const float* v, int n);

// Writer of a table of float vectors / matrices: "ark:", "ark,t:", "ark,scp:a,b", "scp,ark:b,a".
class TableWriter {
 public:
  explicit TableWriter(const std::string& wspecifier);
  ~TableWriter();
  void WriteVec(const std::string& key, const float* v, int n);
  void WriteMat(const std::string& key, const Matrix& m);
  // A double-precision matrix ("DM"; text: 17 significant digits): the CMVN statistics compute-cmvn-stats writes.
  void WriteMatDouble(const std::string& key, const double* m, int rows, int cols);
  // A compressed matrix (compress.h): "key \0B<format> <object>", format "CM", "CM2" or "CM3" and the n bytes that follow the
  // token.  Binary tables only; the scp line points at the "\0B" like WriteMat's.
  void WriteCompressed(const std::string& key, const char* format, const void* bytes, size_t n);
  bool binary() const { return opts_.binary; }
  void WriteInt32(const std::string& key, int32_t v);   // Int32Writer (num_utts.ark)
  // BaseFloatWriter (the per-utterance averages of fgmm-global-get-frame-likes): text "key value\n"; binary the size byte 4 and
  // the four bytes.  What ReadFloatTable reads.
  void WriteFloat(const std::string& key, float v);
  // Int32VectorVectorWriter (Gaussian selection) and PosteriorWriter; the types are declared below the class
  void WriteIntVecVec(const std::string& key, const std::vector<std::vector<int32_t>>& v);
  void WritePosterior(const std::string& key, const std::vector<std::vector<std::pair<int32_t, float>>>& post);
  void Close();

 private:
  void Begin(const std::string& key);
  void End();
  WspecifierOptions opts_;
  Output ark_, scp_;
  std::string pending_scp_line_;
};

// ---------------------------------------------------------------------------------------------
// The objects of the GMM-UBM stage (sid/extract_ivectors.sh:58-70): restated from Kaldi's gmm/diag-gmm.cc, gmm/full-gmm.cc,
// util/kaldi-holder-inl.h and hmm/posterior.cc of early 2018.
//   <DiagGMM> [<GCONSTS> FV] <WEIGHTS> FV <MEANS_INVVARS> FM <INV_VARS> FM </DiagGMM>
//   <FullGMM> [<GCONSTS> FV] <WEIGHTS> FV <MEANS_INVCOVARS> FM <INV_COVARS> (FP|DP, int32 dim, dim (dim + 1) / 2 values: the
//             lower triangle row by row; text " [" rows "]") x num-components </FullGMM>
//   (<DiagGMMBegin> / <DiagGMMEnd> and <FullGMMBegin> / <FullGMMEnd> are accepted as Kaldi accepts them.)
// The readers leave the stored gconsts as they are (empty when the file has none); ubm.h recomputes them.
struct DiagGmmData {
  int num_gauss = 0, dim = 0;
  std::vector<float> gconsts, weights;          // [num_gauss]
  std::vector<float> means_invvars, inv_vars;   // [num_gauss][dim]
};
struct FullGmmData {
  int num_gauss = 0, dim = 0;
  std::vector<float> gconsts, weights;   // [num_gauss]
  std::vector<float> means_invcovars;    // [num_gauss][dim]
  std::vector<float> inv_covars;         // [num_gauss][dim (dim + 1) / 2], the packed lower triangles
};
void ReadDiagGmm(Input& in, bool binary, DiagGmmData* m);
void WriteDiagGmm(Output& out, bool binary, const DiagGmmData& m);
void ReadFullGmm(Input& in, bool binary, FullGmmData* m);
void WriteFullGmm(Output& out, bool binary, const FullGmmData& m);
// One packed lower triangle as the full model stores it (FP / DP; text " [ rows ]"): dim (dim + 1) / 2 values appended to
// *packed, the dimension returned; and its writer (FP).  The accumulators of ubm_train.h use them.
int ReadPackedMatrix(Input& in, bool binary, std::vector<float>* packed);
void WritePackedMatrix(Output& out, bool binary, const float* p, int dim);

// vector<vector<int32>> (binary: int32 size, then per list a size byte 4, a raw int32 count and the values; text: "a b ; c d ; \n")
typedef std::vector<std::vector<int32_t>> IntVecVec;
// Posterior (binary: int32 size, per frame int32 size and (int32, float) pairs, every scalar with its size byte; text:
// "[ idx post idx post ] [ ... ] \n")
typedef std::vector<std::vector<std::pair<int32_t, float>>> Posterior;
void ReadIntVecVec(Input& in, bool binary, IntVecVec* v);
void WriteIntVecVec(Output& out, bool binary, const IntVecVec& v);
void ReadPosterior(Input& in, bool binary, Posterior* p);
void WritePosterior(Output& out, bool binary, const Posterior& p);

// Sequential readers of the two tables ("ark:", "ark,s,cs:-", "scp,p:..."): the only ones that honour the p option.
struct SequentialGselectReader : SequentialTableReader<IntVecVec> {
  explicit SequentialGselectReader(const std::string& rspecifier) : SequentialTableReader(rspecifier, false, /*permissive_skips=*/true) {}
};
struct SequentialPosteriorReader : SequentialTableReader<Posterior> {
  explicit SequentialPosteriorReader(const std::string& rspecifier) : SequentialTableReader(rspecifier, false, /*permissive_skips=*/true) {}
};
// Random-access float table, text ("key 0.5") or binary entries (BaseFloatReader: the per-utterance scales of scale-post).
std::unordered_map<std::string, float> ReadFloatTable(const std::string& rspecifier);

}  // namespace xv
