// What the small drop-in tools share (ivector_tools_main.cc, plda_tools_main.cc, feat_tools_main.cc, wav_reverberate_main.cc):
// the program name and Kaldi-style log lines, scalar option parsing, device selection, --config files and the command-line
// driver.  Host only: kio.h and the standard library.  (nnet3-xvector-compute keeps its own, different, conventions.)
#pragma once
#include <stdint.h>

#include <functional>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace xv {

// The basename of argv[0]: what the executables dispatch on, and the name CliMain gives every message of the process.
std::string ProgramName(const char* argv0);

// "LEVEL (<prog>[xvec-hip-0.1]:main():<basename of file>:<line>) <msg>" on stderr.
void LogLine(const char* level, const char* file, int line, const std::string& msg);
#define XLOG(msg)                                     \
  do {                                                \
    std::ostringstream _o;                            \
    _o << msg;                                        \
    xv::LogLine("LOG", __FILE__, __LINE__, _o.str()); \
  } while (0)
#define XWARN(msg)                                        \
  do {                                                    \
    std::ostringstream _o;                                \
    _o << msg;                                            \
    xv::LogLine("WARNING", __FILE__, __LINE__, _o.str()); \
  } while (0)

// Scalars as Kaldi's ParseOptions reads them (an empty boolean is true); false for anything else.
bool ParseBool(const std::string& v, bool* out);
bool ParseInt(const std::string& v, int* out);
bool ParseDouble(const std::string& v, double* out);
// The same, throwing KioError with Kaldi's wording ("Invalid integer option --name=value").
bool ToBool(const std::string& name, const std::string& v);
float ToFloat(const std::string& name, const std::string& v);
int ToInt(const std::string& name, const std::string& v);
double ToDouble(const std::string& name, const std::string& v);
// A seed of our own generators: a non-negative decimal integer.
uint64_t ToSeed(const std::string& name, const std::string& v);

// An option's name with '-' for every '_': the tools that take both spellings compare this.
std::string Dashes(std::string name);
// --verbose, --print-args and --config: what the tools without config_file accept and ignore.
bool CommonOption(const std::string& dashed_name);

// --device if it was given (>= 0), else $XVEC_DEVICE, else 0.
int PickDevice(int requested);

// "--name=value" lines of a Kaldi config file ('#' starts a comment, blank lines allowed); KioError on anything else.
std::vector<std::pair<std::string, std::string>> ReadConfigFile(const std::string& path);

enum class OptionResult { kOk, kUnknown, kBadValue };
constexpr int kUsageError = -2;   // what CliTool::run returns for a wrong number of arguments

struct CliTool {
  const char* usage;
  // Applies one --name[=value]; may throw.
  std::function<OptionResult(const std::string& name, const std::string& value)> set;
  // The tool itself, given the positional arguments: the exit status, or kUsageError.
  std::function<int(const std::vector<std::string>& pos)> run;
  // true (feature and reverberation tools): --config=<file> is read here; the file's options are applied first and the
  // command line's second, all after the command line has been echoed, and an unknown one is named as --name=value.
  // false (ivector and PLDA tools): every option, --config included, goes to `set` as it is met, before the echo, and an
  // error names the argument as it was typed.
  bool config_file;
};

// Installs InstallMappedFileFaultHandler and sets the program name of the log lines, both from argv[0]; walks argv
// ("--name[=value]" until the first positional argument; a bare "--" is a positional; --help prints the usage and exits 0),
// echoes the command line, applies the options and runs the tool.  An unknown option or a bad value: "ERROR (<prog>) ..."
// and 255; kUsageError: the usage and 1; an exception: "ERROR (<prog>) <what>" and 255.  All of it on stderr.
int CliMain(int argc, char** argv, const CliTool& tool);

}  // namespace xv
