// What the drop-in tools share (every *_main.cc but nnet3-xvector-compute, nnet3-copy and copy-feats, which keep their own
// conventions): the program name and Kaldi-style log lines, scalar option parsing, device selection, --config files, and the
// command-line driver.  A tool is declared, not coded: a CliTool record holds its name, usage, options (CliOption records: a
// name, a kind and where the value goes), positional count and run function; an executable is a vector of them and one call of
// ToolsMain, which picks the record by the name the program was started under.  Host only: kio.h and the standard library.
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

// --device if it was given (>= 0), else $XVEC_DEVICE, else 0.
int PickDevice(int requested);

// "--name=value" lines of a Kaldi config file ('#' starts a comment, blank lines allowed); KioError on anything else.
std::vector<std::pair<std::string, std::string>> ReadConfigFile(const std::string& path);

constexpr int kUsageError = -2;   // what CliTool::run returns when only it can tell that the arguments are wrong

struct CliOption {
  enum Kind {
    kBool, kInt, kFloat, kDouble,   // checked as Kaldi's ParseOptions does; a null target: checked and dropped
    kString, kSeed,                 // as given; ToSeed
    kLaxInt,                        // atoi, unchecked: the --device of the tools that came first
    kIgnored,                       // accepted, not looked at
    kRefused, kRefusedIfTrue, kRefusedIfNonZero,   // throws `message` (the latter two after checking a bool / an int)
    kCustom,                        // custom(name, value); see Custom()
  };
  std::string name;   // without "--"
  Kind kind;
  void* target;
  std::string message;
  std::function<bool(const std::string& name, const std::string& value)> custom;
};
inline CliOption Bool(const char* name, bool* to) { return {name, CliOption::kBool, to, "", nullptr}; }
inline CliOption Int(const char* name, int* to) { return {name, CliOption::kInt, to, "", nullptr}; }
inline CliOption Float(const char* name, float* to) { return {name, CliOption::kFloat, to, "", nullptr}; }
inline CliOption Double(const char* name, double* to) { return {name, CliOption::kDouble, to, "", nullptr}; }
inline CliOption String(const char* name, std::string* to) { return {name, CliOption::kString, to, "", nullptr}; }
inline CliOption Seed(const char* name, uint64_t* to) { return {name, CliOption::kSeed, to, "", nullptr}; }
inline CliOption LaxInt(const char* name, int* to) { return {name, CliOption::kLaxInt, to, "", nullptr}; }
inline CliOption Ignored(const char* name) { return {name, CliOption::kIgnored, nullptr, "", nullptr}; }
inline CliOption Refused(const char* name, const char* message) { return {name, CliOption::kRefused, nullptr, message, nullptr}; }
inline CliOption RefusedIfTrue(const char* name, const char* message) { return {name, CliOption::kRefusedIfTrue, nullptr, message, nullptr}; }
inline CliOption RefusedIfNonZero(const char* name, const char* message) { return {name, CliOption::kRefusedIfNonZero, nullptr, message, nullptr}; }
// The escape hatch, for the few options that need code; it may throw.  false: the value is a bad one.  With the name "" it is
// asked about every option no record before it has taken, and false says that it does not know the option either.
inline CliOption Custom(const char* name, std::function<bool(const std::string& name, const std::string& value)> f) {
  return {name, CliOption::kCustom, nullptr, "", std::move(f)};
}

struct CliTool {
  const char* name;    // what the program is installed as
  const char* usage;
  // Looked up in this order; --verbose, --print-args and --config are accepted and ignored after them (not with config_file,
  // where --config is the file and a tool lists the other two if it takes them).
  std::vector<CliOption> options;
  int min_pos, max_pos;   // the positional arguments it takes, else the usage and 1; max_pos < 0: any number
  // The tool itself, given the positional arguments: the exit status, or kUsageError.
  std::function<int(const std::vector<std::string>& pos)> run;
  const char* match = nullptr;   // NameRule::kContains looks for this part of the name instead of the whole of it
  // What differs between the families of tools:
  bool underscores = true;    // --delta_order is --delta-order; errors name the option with dashes
  bool bad_value_line = false;   // a malformed value: "Invalid value for option <as typed>" instead of a KioError in Kaldi's wording
  // true (feature and reverberation tools): --config=<file> is read; the file's options are applied first and the command
  // line's second, all after the command line has been echoed, and an unknown one is named as --name=value.
  // false: every option, --config included, is applied as it is met, before the echo, and an error names the argument as it was typed.
  bool config_file = false;
};

// How an executable finds its tool by the basename of argv[0].
enum class NameRule {
  kContains,        // the first tool of the table whose name (or `match`) the program's name contains, else `fallback`
  kExact,           // the tool of that name, else `fallback`
  kExactOrRefuse,   // the tool of that name, else "<prog>: not one of <the table's names>" and 255
};

enum class OptionResult { kOk, kUnknown, kBadValue };
// Applies one --name[=value] by the tool's table; may throw.
OptionResult SetOption(const CliTool& tool, const std::string& name, const std::string& value);

// Installs InstallMappedFileFaultHandler and sets the program name of the log lines, both from argv[0]; walks argv
// ("--name[=value]" until the first positional argument; a bare "--" is a positional; --help prints the usage and exits 0),
// echoes the command line, applies the options and runs the tool.  An unknown option or a bad value: "ERROR (<prog>) ..."
// and 255; a wrong number of arguments or kUsageError: the usage and 1; an exception: "ERROR (<prog>) <what>" and 255.  All of
// it on stderr.
int CliMain(int argc, char** argv, const CliTool& tool);
// CliMain for the tool that `rule` picks; `fallback` names a tool of the table.
int ToolsMain(int argc, char** argv, const std::vector<CliTool>& tools, NameRule rule, const char* fallback = nullptr);

}  // namespace xv
