// nnet3-copy shim - just enough of Kaldi's nnet3-copy for the one way the extraction scripts use it:
//   nnet="nnet3-copy --nnet-config=$dir/extract.config $srcdir/final.raw - |"
//   (egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:58-59)
// i.e. read a raw model, replace/add node lines (the output-node), write the model to a wxfilename.
// Components are re-emitted byte for byte.  Options outside that use (--edits, --learning-rate, ...) are
// rejected loudly rather than silently ignored, because they would change the model.
// A copy of the executable named nnet3-am-copy is the other half of the acoustic-model scripts' model pipe
//   raw_nnet="nnet3-am-copy --raw=true $srcdir/final.mdl - | nnet3-copy --nnet-config=$dir/extract.config - - |"
//   (egs/sre/v5/sid/nnet3_cvector/am/extract_bn.sh:57, cvector/extract_am_embedding.sh:56)
// i.e. read final.mdl, drop the transition model (skipped up to its closing token, nnet3_raw.h) and write the network as
// nnet3-copy would.  --raw=true is the one use: without it, or with any option that edits the model, the tool refuses.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "kio.h"
#include "nnet3_raw.h"

int main(int argc, char** argv) {
  const char* base = strrchr(argv[0], '/') ? strrchr(argv[0], '/') + 1 : argv[0];
  const bool am = strcmp(base, "nnet3-am-copy") == 0;
  const char* prog = am ? "nnet3-am-copy" : "nnet3-copy";
  const char* usage = am ? "Usage: nnet3-am-copy --raw=true [--binary=true|false] <mdl-in> <raw-nnet-out>\n"
                         : "Usage: nnet3-copy [--nnet-config=<file>] [--binary=true|false] <raw-nnet-in> <raw-nnet-out>\n";
  try {
    std::string nnet_config;
    bool binary = true, binary_set = false, raw = false;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
      std::string a = argv[i];
      if (a.compare(0, 2, "--") == 0 && pos.empty()) {
        size_t eq = a.find('=');
        std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
        std::string val = eq == std::string::npos ? "" : a.substr(eq + 1);
        if (name == "nnet-config" && !am) nnet_config = val;
        else if (name == "raw" && am) raw = eq == std::string::npos || val == "true" || val == "t" || val == "1";   // a bare --raw is Kaldi's "true"
        else if (name == "binary") {
          binary = !(val == "false" || val == "f" || val == "0");
          binary_set = true;
        } else if (name == "print-args" || name == "verbose") {
        } else if (name == "help") {
          fputs(usage, stderr);
          return 0;
        } else {
          fprintf(stderr, "%s (xvec-hip shim): option --%s is not supported by this shim\n", prog, name.c_str());
          return 1;
        }
      } else {
        pos.push_back(a);
      }
    }
    if (pos.size() != 2) {
      fputs(usage, stderr);
      return 1;
    }
    if (am && !raw) {
      fputs("nnet3-am-copy (xvec-hip shim): only --raw=true (write the network without the transition model) is supported by this shim\n", stderr);
      return 1;
    }
    xv::RawNnet net;
    if (am) net.ReadAcousticModelFrom(pos[0]);
    else net.ReadFrom(pos[0]);
    if (!nnet_config.empty()) {
      std::ifstream f(nnet_config);
      if (!f) throw xv::KioError("cannot open --nnet-config file " + nnet_config);
      std::stringstream ss;
      ss << f.rdbuf();
      net.ApplyNnetConfig(ss.str());
    }
    if (binary_set && binary != net.binary)
      throw xv::KioError("this shim cannot convert between binary and text models (input is " +
                         std::string(net.binary ? "binary" : "text") + ")");
    xv::Output out;
    out.Open(pos[1]);
    net.Write(out, net.binary);
    if (out.Close() != 0) throw xv::KioError("error closing output " + pos[1]);
    if (am) fprintf(stderr, "LOG (nnet3-am-copy[xvec-hip-0.1]:main()) Copied neural net from %s to raw format as %s\n", pos[0].c_str(), pos[1].c_str());
    else fprintf(stderr, "LOG (nnet3-copy[xvec-hip-0.1]:main()) Copied raw neural net from %s to %s\n", pos[0].c_str(), pos[1].c_str());
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "ERROR (%s[xvec-hip-0.1]:main()) %s\n", prog, e.what());
    return -1;
  }
}
