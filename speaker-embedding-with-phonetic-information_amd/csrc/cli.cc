#include "cli.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kio.h"

namespace xv {
namespace {

std::string g_prog = "xvec-hip";   // until CliMain sets it

const char* Basename(const char* path) {
  const char* slash = strrchr(path, '/');
  return slash ? slash + 1 : path;
}

std::string Dashes(std::string name) {
  for (char& c : name)
    if (c == '_') c = '-';
  return name;
}

}  // namespace

std::string ProgramName(const char* argv0) { return Basename(argv0); }

void LogLine(const char* level, const char* file, int line, const std::string& msg) {
  fprintf(stderr, "%s (%s[xvec-hip-0.1]:main():%s:%d) %s\n", level, g_prog.c_str(), Basename(file), line, msg.c_str());
}

bool ParseBool(const std::string& v, bool* out) {
  if (v == "true" || v == "t" || v == "1" || v.empty()) *out = true;
  else if (v == "false" || v == "f" || v == "0") *out = false;
  else return false;
  return true;
}

bool ParseInt(const std::string& v, int* out) {
  char* end = nullptr;
  const long l = strtol(v.c_str(), &end, 10);
  *out = (int)l;
  return !v.empty() && end && *end == 0;
}

bool ParseDouble(const std::string& v, double* out) {
  char* end = nullptr;
  *out = strtod(v.c_str(), &end);
  return !v.empty() && end && *end == 0;
}

bool ToBool(const std::string& name, const std::string& v) {
  bool b;
  if (!ParseBool(v, &b)) throw KioError("Invalid format for boolean argument --" + name + "=" + v);
  return b;
}

float ToFloat(const std::string& name, const std::string& v) { return (float)ToDouble(name, v); }

int ToInt(const std::string& name, const std::string& v) {
  int i;
  if (!ParseInt(v, &i)) throw KioError("Invalid integer option --" + name + "=" + v);
  return i;
}

double ToDouble(const std::string& name, const std::string& v) {
  double d;
  if (!ParseDouble(v, &d)) throw KioError("Invalid floating-point option --" + name + "=" + v);
  return d;
}

uint64_t ToSeed(const std::string& name, const std::string& v) {
  char* end = nullptr;
  const unsigned long long s = strtoull(v.c_str(), &end, 10);
  if (v.empty() || *end != '\0' || v[0] == '-') throw KioError("Invalid option --" + name + "=" + v + ": a non-negative integer is expected");
  return (uint64_t)s;
}

int PickDevice(int requested) {
  if (requested >= 0) return requested;
  const char* e = getenv("XVEC_DEVICE");
  return (e && *e) ? atoi(e) : 0;
}

std::vector<std::pair<std::string, std::string>> ReadConfigFile(const std::string& path) {
  Input in;
  in.Open(path);
  std::vector<std::pair<std::string, std::string>> out;
  std::string line;
  int c = 0;
  while (c >= 0) {
    line.clear();
    while ((c = in.Get()) >= 0 && c != '\n') line.push_back((char)c);
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    const size_t b = line.find_first_not_of(" \t\r");
    if (b == std::string::npos) continue;
    const size_t e = line.find_last_not_of(" \t\r");
    line = line.substr(b, e - b + 1);
    if (line.compare(0, 2, "--") != 0)
      throw KioError("Reading config file " + path + ": line '" + line + "' does not look like a line from a Kaldi command-line program's config file: should be of the form --x=y");
    const size_t eq = line.find('=');
    out.emplace_back(line.substr(2, eq == std::string::npos ? std::string::npos : eq - 2),
                     eq == std::string::npos ? std::string() : line.substr(eq + 1));
  }
  return out;
}

OptionResult SetOption(const CliTool& tool, const std::string& name, const std::string& v) {
  const std::string n = tool.underscores ? Dashes(name) : name;
  const bool lax = tool.bad_value_line;   // a malformed value is reported by the caller, not thrown
  for (const CliOption& o : tool.options) {
    if (o.name != n && !(o.kind == CliOption::kCustom && o.name.empty())) continue;
    bool b = false;
    int i = 0;
    double d = 0.0;
    switch (o.kind) {
      case CliOption::kBool:
      case CliOption::kRefusedIfTrue:
        if (lax && !ParseBool(v, &b)) return OptionResult::kBadValue;
        b = ToBool(n, v);
        if (o.kind == CliOption::kRefusedIfTrue && b) throw KioError(o.message);
        if (o.target) *(bool*)o.target = b;
        break;
      case CliOption::kInt:
      case CliOption::kRefusedIfNonZero:
        if (lax && !ParseInt(v, &i)) return OptionResult::kBadValue;
        i = ToInt(n, v);
        if (o.kind == CliOption::kRefusedIfNonZero && i != 0) throw KioError(o.message);
        if (o.target) *(int*)o.target = i;
        break;
      case CliOption::kFloat:
      case CliOption::kDouble:
        if (lax && !ParseDouble(v, &d)) return OptionResult::kBadValue;
        d = ToDouble(n, v);
        if (o.target && o.kind == CliOption::kFloat) *(float*)o.target = (float)d;
        if (o.target && o.kind == CliOption::kDouble) *(double*)o.target = d;
        break;
      case CliOption::kString: *(std::string*)o.target = v; break;
      case CliOption::kSeed: *(uint64_t*)o.target = ToSeed(n, v); break;
      case CliOption::kLaxInt: *(int*)o.target = atoi(v.c_str()); break;
      case CliOption::kIgnored: break;
      case CliOption::kRefused: throw KioError(o.message);
      case CliOption::kCustom:
        if (o.custom(n, v)) break;
        if (o.name.empty()) continue;
        return OptionResult::kBadValue;
    }
    return OptionResult::kOk;
  }
  const bool common = !tool.config_file && (n == "verbose" || n == "print-args" || n == "config");
  return common ? OptionResult::kOk : OptionResult::kUnknown;
}

int CliMain(int argc, char** argv, const CliTool& tool) {
  g_prog = Basename(argv[0]);
  InstallMappedFileFaultHandler(g_prog.c_str());
  const char* prog = g_prog.c_str();
  // `typed`: how an error names the option
  auto apply = [&](const std::string& name, const std::string& value, const std::string& typed) {
    const OptionResult r = SetOption(tool, name, value);
    if (r == OptionResult::kUnknown) fprintf(stderr, "ERROR (%s) Invalid option %s\n\n%s", prog, typed.c_str(), tool.usage);
    if (r == OptionResult::kBadValue) fprintf(stderr, "ERROR (%s) Invalid value for option %s\n", prog, typed.c_str());
    return r == OptionResult::kOk;
  };
  try {
    std::vector<std::string> pos;
    std::vector<std::pair<std::string, std::string>> options;
    std::string config, cmdline = g_prog;
    for (int i = 1; i < argc; ++i) {
      const std::string s = argv[i];
      cmdline += " " + s;
      if (s.compare(0, 2, "--") != 0 || s.size() == 2 || !pos.empty()) {
        pos.push_back(s);
        continue;
      }
      const size_t eq = s.find('=');
      const std::string name = s.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
      const std::string value = eq == std::string::npos ? "" : s.substr(eq + 1);
      if (name == "help") {
        fputs(tool.usage, stderr);
        return 0;
      }
      if (!tool.config_file) {
        if (!apply(name, value, s)) return 255;
      } else if (name == "config") {
        config = value;
      } else {
        options.emplace_back(name, value);
      }
    }
    fprintf(stderr, "%s \n", cmdline.c_str());
    if (!config.empty()) {
      const auto file = ReadConfigFile(config);
      options.insert(options.begin(), file.begin(), file.end());   // the command line comes second, and so wins
    }
    for (const auto& nv : options)
      if (!apply(nv.first, nv.second, "--" + nv.first + (nv.second.empty() ? "" : "=" + nv.second))) return 255;
    const bool count_ok = (int)pos.size() >= tool.min_pos && (tool.max_pos < 0 || (int)pos.size() <= tool.max_pos);
    const int rc = count_ok ? tool.run(pos) : kUsageError;
    if (rc != kUsageError) return rc;
    fputs(tool.usage, stderr);
    return 1;
  } catch (const std::exception& e) {
    fprintf(stderr, "ERROR (%s) %s\n", prog, e.what());
    return 255;
  }
}

int ToolsMain(int argc, char** argv, const std::vector<CliTool>& tools, NameRule rule, const char* fallback) {
  const std::string prog = ProgramName(argv[0]);
  const CliTool* chosen = nullptr;
  std::string names;
  for (const CliTool& t : tools) {
    const bool is = rule == NameRule::kContains ? prog.find(t.match ? t.match : t.name) != std::string::npos : prog == t.name;
    if (is && !chosen) chosen = &t;
    names += (names.empty() ? "" : ", ") + std::string(t.name);
  }
  if (!chosen && fallback && rule != NameRule::kExactOrRefuse)
    for (const CliTool& t : tools)
      if (strcmp(t.name, fallback) == 0) chosen = &t;
  if (!chosen) {
    fprintf(stderr, "%s: not one of %s\n", prog.c_str(), names.c_str());
    return 255;
  }
  return CliMain(argc, argv, *chosen);
}

}  // namespace xv
